// gvar_advance_batch_kernels.h — the phantom pass (gvar_advance_kernels.h) of ONE `glyf` face at MANY positions in one launch
// (gvar_advance_batch_kernels.hip; vgsdf_gvar_advance_deltas_batch and vgsdf_families_create_tables of include/vgsdf.h).  One lane
// per (glyph id, position) pair, workgroups of one wave (kGvarLanes); a pair's index is glyph id x positions + position, as in
// gvar_batch_kernels.hip.  A lane does for its glyph id what a lane of gvar_advance_pass does, with its position's coordinates.
// O(1) state per lane, no scratch, no LDS.
#pragma once
#include "gvar_advance_kernels.h"

extern "C" {
// coords_all: n_axes coordinates per position.  delta[p * n_glyph_ids + g], state[p * n_glyph_ids + g]: position p's arrays are
// contiguous.  flags: GVAR_ADVANCE_FLAG_WORDS zeroed words for all positions (the one bound they raise, VGSDF_GVAR_MAX_DELTAS, is
// checked before a tuple is walked and looks at no coordinate).  n_positions >= 1, face->n_glyph_ids x n_positions below 2^32.
int vgsdf_gvar_advance_batch_pass(const vgsdf::GvarRef *face, const int16_t *coords_all, uint32_t n_positions, float *delta, uint8_t *state,
                                  uint32_t *flags, hipStream_t stream);
}
