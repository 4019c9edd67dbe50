// glyf_table_kernels.h — a `glyf` face's resident form (leaves + the simple entries' bytes) built on the device from its `loca`
// and `glyf` tables (glyf_table_kernels.hip; vgsdf_font_create_tables of include/vgsdf.h): one lane per glyph id walks the
// glyph's component tree as Face::resident_table does; a count pass sizes the arrays, an emit pass of the same text writes them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vgsdf {

// the face, all addresses on the device.  Every read of loca / glyf is bounded by loca_entries and glyf_len.
struct GlyfTablesRef {
	const uint8_t *loca, *glyf; // the tables as they stand in the file (any alignment)
	uint32_t glyf_len;
	uint32_t loca_entries;      // entries of loca the walk may read (the host has checked them against the table's bytes)
	uint32_t loca_long;         // 0: u16 offsets in words, 1: u32 offsets in bytes
	uint32_t n_glyph_ids;
};

constexpr uint32_t kGlyfTableLanes = 64;  // glyph ids per workgroup: one wave
constexpr uint32_t kGlyfTableCounts = 4;  // u32 per glyph id the count pass leaves: stored bytes (not padded), leaves, slots, own cmd_cap
// the walk's stack: the composites above the one being read, [level][word][lane] in LDS.  The glyph at depth 31 is the
// deepest that is read (depth 32 fails), so at most 31 parents wait above it
constexpr uint32_t kGlyfTableLevels = 31, kGlyfTableFrameWords = 8;

// words of the passes' flags (each zeroed by the host; every writer stores 1)
enum : uint32_t {
	GLYF_FLAG_BUDGET = 0, // a glyph id past VGSDF_GLYF_MAX_COMPONENTS component records
	GLYF_FLAG_SLOTS = 1,  // a glyph id of more than 2^26 command slots
	GLYF_FLAG_EMIT = 2,   // emit pass: a leaf or a byte outside the counted ranges (never: both passes are one text)
	GLYF_FLAG_WORDS = 4,
};

} // namespace vgsdf

extern "C" {
// count pass: counts[4 g ..] = {byte_len of g's own simple entry (0: none), leaves, command slots, cmd_cap of the own entry}
int vgsdf_glyf_tables_count(const vgsdf::GlyfTablesRef *face, uint32_t *counts, uint32_t *flags, hipStream_t stream);
// emit pass: glyph id g's leaves to leaves[leaf_off[g] .. leaf_off[g + 1]) (48-byte vgsdf_glyf_part records), its own simple
// entry's bytes, zero-padded, to bytes[byte_at[g] .. byte_at[g + 1]); leaf_off and byte_at: u32[n_glyph_ids + 1] on the device
int vgsdf_glyf_tables_emit(const vgsdf::GlyfTablesRef *face, const uint32_t *leaf_off, const uint32_t *byte_at, void *leaves,
                           uint8_t *bytes, uint32_t *flags, hipStream_t stream);
}
