// gvar_advance_kernels.h — the phantom pass: what a placed `glyf` face's advances take from `gvar` when the file has no `HVAR`
// (rule G7 of host/ttf_face.hpp; gvar_advance_kernels.hip; vgsdf_gvar_advance_deltas of include/vgsdf.h).  One lane per glyph
// id, workgroups of one wave (kGvarLanes), one pass: the point count n of the glyph id's own entry, then its tuples streamed with
// O(1) state — the position in the number list, the position in the delta stream, l and r.  No scratch, no LDS.
#pragma once
#include "gvar_kernels.h"

namespace vgsdf {

// the state byte of a glyph id (Face::kGvarAdvance* of host/ttf_face.hpp)
enum : uint32_t { GVAR_ADVANCE_NONE = 0, GVAR_ADVANCE_DELTA = 1, GVAR_ADVANCE_MALFORMED = 2 };
// words of the pass's flags (zeroed by the host; every writer stores 1)
enum : uint32_t {
	GVAR_ADVANCE_FLAG_DELTAS = 0, // a glyph id past VGSDF_GVAR_MAX_DELTAS (tuples x (n + 4)): its tuples were not walked
	GVAR_ADVANCE_FLAG_WORDS = 4,
};

} // namespace vgsdf

extern "C" {
// delta[g] = the f32 d = r - l of glyph id g (0 unless state[g] is GVAR_ADVANCE_DELTA), for g < face->n_glyph_ids
int vgsdf_gvar_advance_pass(const vgsdf::GvarRef *face, float *delta, uint8_t *state, uint32_t *flags, hipStream_t stream);
}
