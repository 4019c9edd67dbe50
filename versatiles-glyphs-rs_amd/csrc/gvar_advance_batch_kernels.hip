// gvar_advance_batch_kernels.hip — the phantom pass over (glyph id, position) pairs (gvar_advance_batch_kernels.h): ONE `glyf` face
// whose advances follow gvar's phantom points (rule G7 of host/ttf_face.hpp), at all positions of a call in one launch.  What a
// lane does for its pair is the text a lane of gvar_advance_pass runs for its glyph id (gvar_advance_device.inc over
// gvar_device.inc: own_point_count, then phantom_sums, G1 to G4 and G7, f32 as written — this unit is built with
// -ffp-contract=off); only F.coords differs, coords_all + position x n_axes.  A pair's index is glyph id x positions + position:
// the lanes of a wave that hold one glyph id at different positions are neighbours, read the same bytes of loca, glyf and gvar and
// branch alike up to where a tuple's scalar is 0 at one position and not at another.  Every read is bounded by loca_entries /
// glyf_len / gvar_len as there; the two stores are the pair's own, below n_positions x n_glyph_ids.
#include "gvar_advance_batch_kernels.h"

#include "gvar_limits.h"

namespace vgsdf {
namespace {

#include "gvar_device.inc"
#include "gvar_advance_device.inc"

__global__ __launch_bounds__(kGvarLanes) void gvar_advance_batch_pass(GvarRef F, const int16_t *coords_all, uint32_t np, float *delta,
                                                                      uint8_t *state, uint32_t *flags)
{
	const uint32_t pair = blockIdx.x * kGvarLanes + threadIdx.x; // (at most 65535 glyph ids x 64 positions)
	const uint32_t gid = pair / np, position = pair % np;
	if (gid >= F.n_glyph_ids)
		return;
	F.coords = coords_all + (size_t)position * F.n_axes;
	uint32_t n, st = GVAR_ADVANCE_MALFORMED;
	float d = 0.0f;
	if (own_point_count(F, gid, n)) {
		float l, r;
		st = phantom_sums(F, gid, n, l, r, flags);
		if (st == GVAR_ADVANCE_DELTA)
			d = r - l;
	}
	const size_t at = (size_t)position * F.n_glyph_ids + gid; // position-major: a position's arrays are contiguous
	delta[at] = d;
	state[at] = (uint8_t)st;
}

} // namespace
} // namespace vgsdf

extern "C" {

int vgsdf_gvar_advance_batch_pass(const vgsdf::GvarRef *face, const int16_t *coords_all, uint32_t n_positions, float *delta, uint8_t *state,
                                  uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids * n_positions + vgsdf::kGvarLanes - 1) / vgsdf::kGvarLanes;
	hipLaunchKernelGGL(vgsdf::gvar_advance_batch_pass, dim3(groups), dim3(vgsdf::kGvarLanes), 0, stream, *face, coords_all, n_positions, delta,
	                   state, flags);
	return (int)hipGetLastError();
}

} // extern "C"
