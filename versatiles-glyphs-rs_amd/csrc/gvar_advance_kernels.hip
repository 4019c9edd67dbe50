// gvar_advance_kernels.hip — the phantom pass (gvar_advance_kernels.h).  What a lane does for its glyph id is, step for step, the
// host reader's Face::gvar_advance_delta (host/ttf_face.cpp): Face::own_point_count over Face::glyph_data's loca rules and
// read_component's record sizes, then GvarTable::phantom_sums — rules G1 to G4 for the tuples, and of every applied tuple the x
// deltas of points n and n + 1, its numbers and all 2 x count of its deltas walked to their end so that malformed means what it
// means to the outline (rule G7 of host/ttf_face.hpp).  f32 as written (this unit is built with -ffp-contract=off).
// Every read is bounded by loca_entries / glyf_len / gvar_len (the host has checked the gvar header, the shared tuples and the
// offset array); the two stores are the lane's own glyph id's, below n_glyph_ids.  The readers are those of the gvar builder
// (gvar_device.inc: glyph_range, PointNumbers, DeltaStream, axis_factor), compiled here as its two units compile them.
#include "gvar_advance_kernels.h"

#include "gvar_limits.h"

namespace vgsdf {
namespace {

#include "gvar_device.inc"
#include "gvar_advance_device.inc"

__global__ __launch_bounds__(kGvarLanes) void gvar_advance_pass(GvarRef F, float *delta, uint8_t *state, uint32_t *flags)
{
	const uint32_t gid = blockIdx.x * kGvarLanes + threadIdx.x;
	if (gid >= F.n_glyph_ids)
		return;
	uint32_t n, st = GVAR_ADVANCE_MALFORMED;
	float d = 0.0f;
	if (own_point_count(F, gid, n)) {
		float l, r;
		st = phantom_sums(F, gid, n, l, r, flags);
		if (st == GVAR_ADVANCE_DELTA)
			d = r - l;
	}
	delta[gid] = d;
	state[gid] = (uint8_t)st;
}

} // namespace
} // namespace vgsdf

extern "C" {

int vgsdf_gvar_advance_pass(const vgsdf::GvarRef *face, float *delta, uint8_t *state, uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids + vgsdf::kGvarLanes - 1) / vgsdf::kGvarLanes;
	hipLaunchKernelGGL(vgsdf::gvar_advance_pass, dim3(groups), dim3(vgsdf::kGvarLanes), 0, stream, *face, delta, state, flags);
	return (int)hipGetLastError();
}

} // extern "C"
