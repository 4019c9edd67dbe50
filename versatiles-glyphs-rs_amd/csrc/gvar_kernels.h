// gvar_kernels.h — the command store of a `glyf` face placed by `gvar`, built on the device from its `loca`, `glyf` and `gvar`
// tables (gvar_kernels.hip; vgsdf_font_create_gvar of include/vgsdf.h).  One lane per glyph id, workgroups of one wave, three
// passes: count (points of the glyph id's own entry; commands and coordinates of its component tree), deltas (rules G1 to G6 of
// host/ttf_face.hpp over the own entry, into `acc`), emit (the tree again, its points moved by `acc`, as kinds | coords).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vgsdf {

// the face, all addresses on the device.  Every read of loca / glyf / gvar is bounded by loca_entries, glyf_len and gvar_len;
// the host has checked that the gvar header, the shared tuples and the offset array lie inside gvar_len.
struct GvarRef {
	const uint8_t *loca, *glyf, *gvar; // the tables as they stand in the file (any alignment)
	const int16_t *coords;             // [n_axes] normalised, F2Dot14
	uint32_t glyf_len, loca_entries, loca_long, n_glyph_ids;
	uint32_t gvar_len, n_axes;
	uint32_t shared_count, shared_at, glyph_count, long_offsets, data_at; // the gvar header's fields
};

constexpr uint32_t kGvarLanes = 64;  // glyph ids per workgroup: one wave
constexpr uint32_t kGvarCounts = 4;  // u32 per glyph id the count pass leaves: own points (+ 4 phantom; 0: no entry that takes deltas), commands, coordinates, 0
// the tree walk's stack, [level][word][lane] in LDS: the composites above the one being read (glyf_table_kernels.h)
constexpr uint32_t kGvarLevels = 31, kGvarFrameWords = 8;

// words of the passes' flags (each zeroed by the host; every writer stores 1)
enum : uint32_t {
	GVAR_FLAG_RECORDS = 0,   // a glyph id past VGSDF_GLYF_MAX_COMPONENTS component records, or a composite entry of more than 65535
	GVAR_FLAG_CMDS = 1,      // a glyph id of more than 2^26 commands
	GVAR_FLAG_MALFORMED = 2, // deltas pass: a glyph id with malformed variation data
	GVAR_FLAG_DELTAS = 3,    // deltas pass: a glyph id past VGSDF_GVAR_MAX_DELTAS
	GVAR_FLAG_EMIT = 4,      // emit pass: a command or coordinate outside the counted ranges (never: both passes are one text)
	GVAR_FLAG_WORDS = 8,
};

// the deltas pass's scratch for the tuple in hand and the entry's decoded points, one element per point of the launch's slice
struct GvarScratch {
	float *sx, *sy;  // the tuple's scaled (then inferred) deltas
	int16_t *x, *y;  // the entry's original coordinates
	uint8_t *mark;   // bit 0: touched by the tuple in hand; bit 7: last point of its contour
};
constexpr uint32_t kGvarScratchBytesPerPoint = 4 + 4 + 2 + 2 + 1;

// one position of the batched emit pass (gvar_batch_kernels.hip; vgsdf_fonts_create_gvar), all addresses on the device: the
// position's sums, its store's cmd_off, and the staging of its context pass (dat_off, kinds, coords); flags: its GVAR_FLAG_WORDS
struct GvarPositionRef {
	const float *acc;
	const uint32_t *cmd_off, *dat_off;
	uint8_t *kinds;
	float *coords;
	uint32_t *flags;
};

} // namespace vgsdf

extern "C" {
// count pass: counts[4 g ..] = {points of g's own entry + 4 (0: none), commands, coordinates, 0}
int vgsdf_gvar_count(const vgsdf::GvarRef *face, uint32_t *counts, uint32_t *flags, hipStream_t stream);
// deltas pass over glyph ids [g0, g1): acc[2 * pt_at[g] ..] = the sums of g's own entry, x then y per point (pt_at: the running
// sum of the counts' own points, u32[n_glyph_ids + 1] on the device); scratch holds pt_at[g1] - pt_at[g0] points
int vgsdf_gvar_deltas(const vgsdf::GvarRef *face, uint32_t g0, uint32_t g1, const uint32_t *counts, const uint32_t *pt_at, float *acc,
                      const vgsdf::GvarScratch *scratch, uint32_t *flags, hipStream_t stream);
// emit pass: glyph id g's kinds to kinds[cmd_off[g] .. cmd_off[g + 1]), its coordinates to coords[dat_off[g] .. dat_off[g + 1])
int vgsdf_gvar_emit(const vgsdf::GvarRef *face, const uint32_t *counts, const uint32_t *pt_at, const float *acc, const uint32_t *cmd_off,
                    const uint32_t *dat_off, uint8_t *kinds, float *coords, uint32_t *flags, hipStream_t stream);
// the same face at many positions (gvar_batch_kernels.hip), one lane per (glyph id, position), position fastest.
// deltas pass over glyph ids [g0, g1) x positions [p0, p1), p1 > p0: coords_all holds face->n_axes coordinates per position
// (face->coords is not read), acc + p * acc_stride the sums of position p laid out as above, flags + p * GVAR_FLAG_WORDS its flag
// words; scratch holds (p1 - p0) stretches of slice = pt_at[g1] - pt_at[g0] points
int vgsdf_gvar_batch_deltas(const vgsdf::GvarRef *face, uint32_t g0, uint32_t g1, uint32_t p0, uint32_t p1, const int16_t *coords_all,
                            const uint32_t *counts, const uint32_t *pt_at, float *acc, uint64_t acc_stride, const vgsdf::GvarScratch *scratch,
                            uint32_t slice, uint32_t *flags, hipStream_t stream);
// emit pass over every glyph id x positions[0, n_positions), n_positions >= 1 (an array on the device)
int vgsdf_gvar_batch_emit(const vgsdf::GvarRef *face, const vgsdf::GvarPositionRef *positions, uint32_t n_positions, const uint32_t *counts,
                          const uint32_t *pt_at, hipStream_t stream);
}
