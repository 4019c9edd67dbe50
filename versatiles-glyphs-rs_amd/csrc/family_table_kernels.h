// family_table_kernels.h — a resident family's table built on the device from its faces' `cmap` and `hmtx` tables
// (family_table_kernels.hip; vgsdf_family_create_tables of include/vgsdf.h): one lane per code point of the BMP looks the code
// point up in the faces in order, a count pass sizes the table and an emit pass writes FamilyTableLayout (upload_layout.h) in place.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vgsdf {

// one face of the family, all addresses on the device.  Every read of cmap / hmtx is bounded by cmap_len / hmtx_len; the host has
// checked subtable offsets < cmap_len (vgsdf_family_create_tables).
struct FamilyFaceRef {
	uint64_t cmap, hmtx;  // the tables' bytes (hmtx: 0 with hmtx_len 0)
	uint64_t subtables;   // FamilySubtable[n_subtables]
	uint64_t off;         // the face's font: cmd_off (command font) or leaf_off (glyf font), u32[n_glyph_ids + 1]
	uint64_t leaves;      // glyf font: its vgsdf_glyf_part records; command font: 0
	uint32_t cmap_len, hmtx_len;
	uint32_t n_glyph_ids; // of the font
	uint16_t units_per_em, num_glyphs, num_hmetrics, n_subtables;
	uint32_t commands;    // 1: a command font
};
static_assert(sizeof(FamilyFaceRef) == 64, "one 64-byte record per face");
struct FamilySubtable {
	uint32_t off, format; // into cmap; 0 4 6 10 12 13
};

constexpr uint32_t kFamilyThreads = 256; // code points per workgroup
constexpr uint32_t kFamilyGroups = 0x10000u / kFamilyThreads;
constexpr uint32_t kFamilyCounts = 4;    // u32 per workgroup the count pass leaves: entries, command slots, leaves, 0

// bits of the passes' flag word
enum : uint32_t {
	FAMILY_FLAG_GLYPH = 1u, // a code point mapped to a glyph id at or past its font's n_glyph_ids (the entry is not followed)
};

} // namespace vgsdf

extern "C" {
// count pass: counts[4 w ..] = {entries, command slots mod 2^32, leaves mod 2^32, 0} of workgroup w's 256 code points; flags: one
// zeroed word
int vgsdf_family_tables_count(const vgsdf::FamilyFaceRef *faces, uint32_t n_faces, uint32_t *counts, uint32_t *flags, hipStream_t stream);
// emit pass: the n_entries = sum of the counted entries, each at its rank, into `table` (FamilyTableLayout(n_entries))
int vgsdf_family_tables_emit(const vgsdf::FamilyFaceRef *faces, uint32_t n_faces, const uint32_t *counts, uint32_t n_entries,
                             uint8_t *table, hipStream_t stream);
}
