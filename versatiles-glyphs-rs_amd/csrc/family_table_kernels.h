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
// what a face at a position adds (vgsdf_face_variation), in an array beside the faces' records (those are full): the `HVAR`
// bytes on the device and the factors of its store's regions.  Every read of hvar is bounded by hvar_len; the host has checked
// store_off + 8 <= hvar_len and map_off < hvar_len (vgsdf_family_create_tables_var).
struct FamilyFaceVar {
	uint64_t hvar;    // 0: a static face
	uint64_t scalars; // f32[n_regions]
	uint32_t hvar_len, store_off, map_off, n_regions; // map_off 0: no advance map
};
static_assert(sizeof(FamilyFaceVar) == 32, "one 32-byte record per face");
// what a placed `glyf` face WITHOUT an `HVAR` adds instead (rule G7 of host/ttf_face.hpp), in a second array beside the faces'
// records: the output of the phantom pass (gvar_advance_kernels.h) over the face, one f32 delta and one state byte per glyph id.
// Read for a face whose FamilyFaceVar has no hvar, by glyph ids below n_glyph_ids only.
struct FamilyFaceGvar {
	uint64_t delta;       // f32[n_glyph_ids]; 0: the face takes no delta from gvar
	uint64_t state;       // u8[n_glyph_ids]: GVAR_ADVANCE_NONE / _DELTA / _MALFORMED
	uint32_t n_glyph_ids; // of the description the pass ran over
	uint32_t pad;
};
static_assert(sizeof(FamilyFaceGvar) == 24, "one 24-byte record per face");
// the batched passes' table of one position: where the emit pass writes FamilyTableLayout(n_entries); table 0: nothing is emitted
struct FamilyBatchTable {
	uint64_t table;
	uint32_t n_entries, pad;
};
static_assert(sizeof(FamilyBatchTable) == 16, "one 16-byte record per position");
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
// zeroed word.  plane (0 .. 16): the code points are (plane << 16) + 0 .. 0xFFFF; the passes below it, which take none, run plane 0
int vgsdf_family_tables_count(const vgsdf::FamilyFaceRef *faces, uint32_t n_faces, uint32_t plane, uint32_t *counts, uint32_t *flags,
                              hipStream_t stream);
// emit pass: the n_entries = sum of the counted entries, each at its rank, into `table` (FamilyTableLayout(n_entries)); the table
// keeps the code points' low halves, pbf_fix the length of the full value
int vgsdf_family_tables_emit(const vgsdf::FamilyFaceRef *faces, uint32_t n_faces, uint32_t plane, const uint32_t *counts, uint32_t n_entries,
                             uint8_t *table, hipStream_t stream);
// the emit pass over faces some of which are at a position: var[n_faces] beside faces
int vgsdf_family_tables_emit_var(const vgsdf::FamilyFaceRef *faces, const vgsdf::FamilyFaceVar *var, uint32_t n_faces, const uint32_t *counts,
                                 uint32_t n_entries, uint8_t *table, hipStream_t stream);
// ... and some of which take their advance's delta from gvar's phantom points: gvar[n_faces] beside var[n_faces]
int vgsdf_family_tables_emit_gvar(const vgsdf::FamilyFaceRef *faces, const vgsdf::FamilyFaceVar *var, const vgsdf::FamilyFaceGvar *gvar,
                                  uint32_t n_faces, const uint32_t *counts, uint32_t n_entries, uint8_t *table, hipStream_t stream);
// The same passes for ONE face at n_positions positions, the position a second grid dimension (vgsdf_families_create_tables):
// faces[p] is the face with font p's store; counts[4 x kFamilyGroups x p ..] and flags[p] (zeroed) are position p's.
int vgsdf_family_tables_batch_count(const vgsdf::FamilyFaceRef *faces, uint32_t n_positions, uint32_t *counts, uint32_t *flags, hipStream_t stream);
// tables[p]: position p's table and its counted entries (table 0: skipped); var: NULL or [n_positions]; gvar: NULL or [n_positions]
// beside var[n_positions]
int vgsdf_family_tables_batch_emit(const vgsdf::FamilyFaceRef *faces, const vgsdf::FamilyFaceVar *var, const vgsdf::FamilyFaceGvar *gvar,
                                   uint32_t n_positions, const uint32_t *counts, const vgsdf::FamilyBatchTable *tables, hipStream_t stream);
}
