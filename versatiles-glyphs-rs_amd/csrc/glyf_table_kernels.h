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

// One face of a batch (vgsdf_fonts_create_tables), all addresses on the device: GlyfTablesRef's fields, where the face's
// workgroups and glyph ids begin in the launch, and, for the emit pass, its store (GlyfStoreLayout: the leaves at its start).
// The batch's counts lie at counts[4 * (glyph_base + g)], its byte_at at byte_at[glyph_base + f + g] (n_glyph_ids + 1 entries per
// face f), its flags at flags[GLYF_FLAG_WORDS * f].  Read through the scalar cache, as the family tables' face records are.
struct GlyfFaceRecord {
	uint64_t loca, glyf;
	uint32_t glyf_len, loca_entries, loca_long, n_glyph_ids;
	uint32_t first_block; // the workgroups of the faces before it that take part in this pass
	uint32_t glyph_base;  // the glyph ids of ALL faces before it
	uint64_t store;       // emit pass: the face's store; count pass: 0
	uint32_t bytes_at, leaf_off_at16; // emit pass: GlyfStoreLayout's bytes and leaf_off / 16 (a store may pass 4 GiB) inside the store
	uint32_t takes_part;  // 0: the face owns no workgroup of this pass (badly described; emit pass: refused or over the limit)
	uint32_t reserved;
};
static_assert(sizeof(GlyfFaceRecord) == 64, "one 64-byte record per face");

// what one batched call takes: the bisection's table and 64 MB of counts
constexpr uint32_t kGlyfBatchMaxFaces = 65536;
constexpr uint32_t kGlyfBatchMaxGlyphIds = 1u << 22;

} // namespace vgsdf

extern "C" {
// the two passes over all faces of a batch in one launch each; n_blocks > 0: the sum of ceil(n_glyph_ids / 64) over the faces that
// take part, which is what their first_block fields run over.  flags: GLYF_FLAG_WORDS zeroed words per face
int vgsdf_glyf_tables_batch_count(const vgsdf::GlyfFaceRecord *faces, uint32_t n_faces, uint32_t n_blocks, uint32_t *counts, uint32_t *flags,
                                  hipStream_t stream);
int vgsdf_glyf_tables_batch_emit(const vgsdf::GlyfFaceRecord *faces, uint32_t n_faces, uint32_t n_blocks, const uint32_t *byte_at,
                                 uint32_t *flags, hipStream_t stream);
// count pass: counts[4 g ..] = {byte_len of g's own simple entry (0: none), leaves, command slots, cmd_cap of the own entry}
int vgsdf_glyf_tables_count(const vgsdf::GlyfTablesRef *face, uint32_t *counts, uint32_t *flags, hipStream_t stream);
// emit pass: glyph id g's leaves to leaves[leaf_off[g] .. leaf_off[g + 1]) (48-byte vgsdf_glyf_part records), its own simple
// entry's bytes, zero-padded, to bytes[byte_at[g] .. byte_at[g + 1]); leaf_off and byte_at: u32[n_glyph_ids + 1] on the device
int vgsdf_glyf_tables_emit(const vgsdf::GlyfTablesRef *face, const uint32_t *leaf_off, const uint32_t *byte_at, void *leaves,
                           uint8_t *bytes, uint32_t *flags, hipStream_t stream);
}
