// gvar_batch_kernels.hip — ONE `glyf` face placed by `gvar` at MANY positions in one call (vgsdf_fonts_create_gvar): the deltas
// pass and the emit pass of gvar_kernels.hip over (glyph id, position) pairs.  The count pass is that unit's own launch: it looks
// at flags only and is the same at every position.  What a lane does for its pair is the text the single call's kernels run
// (gvar_own_deltas.inc, gvar_tree_walk.inc over gvar_device.inc), with the position's coordinates, sums, store and flag words.
// A pair's index is glyph id x positions + position: the lanes of a wave that hold one glyph id at different positions are
// neighbours, read the same bytes of loca, glyf and gvar and branch alike up to where a tuple's scalar is 0 at one position and
// not at another; lanes of different glyph ids diverge as in the single call.  Every read is bounded as there; every store of
// the deltas pass lies inside the pair's own stretch of the position's sums and of the launch's scratch, every store of the emit
// pass inside the ranges the count pass has sized, in the position's own store.
#include "gvar_kernels.h"

#include "glyf_table_limits.h"
#include "gvar_limits.h"

namespace vgsdf {
namespace {

#include "gvar_device.inc"

// glyph ids [g0, g1) at positions [p0, p0 + np): coords_all holds n_axes coordinates per position, acc_first + p * acc_stride the
// sums of position p (as the single call's acc), flags_first + p * GVAR_FLAG_WORDS its flag words.  S0 holds np stretches of
// `slice` = pt_at[g1] - pt_at[g0] points, one per position of the launch: the decoded points are the same at every position,
// the marks and the tuple's deltas are not, and a lane keeps all five beside one another as the single call's lane does
__global__ __launch_bounds__(kGvarLanes) void gvar_batch_deltas_pass(GvarRef F, uint32_t g0, uint32_t g1, uint32_t p0, uint32_t np,
                                                                     const int16_t *coords_all, const uint32_t *counts, const uint32_t *pt_at,
                                                                     float *acc_first, uint64_t acc_stride, GvarScratch S0, uint32_t slice,
                                                                     uint32_t *flags_first)
{
	const uint32_t pair = blockIdx.x * kGvarLanes + threadIdx.x; // (at most 65535 glyph ids x 64 positions)
	const uint32_t gid = g0 + pair / np, pl = pair % np;
	if (gid >= g1)
		return;
	const uint32_t position = p0 + pl;
	F.coords = coords_all + (size_t)position * F.n_axes;
	float *acc_all = acc_first + (size_t)position * acc_stride;
	uint32_t *flags = flags_first + (size_t)position * GVAR_FLAG_WORDS;
	const size_t s = (size_t)pl * slice;
	const GvarScratch S{S0.sx + s, S0.sy + s, S0.x + s, S0.y + s, S0.mark + s};
#include "gvar_own_deltas.inc"
}

// every glyph id at the np positions of `positions` (those that are built): a lane emits its glyph id into its position's store
__global__ __launch_bounds__(kGvarLanes) void gvar_batch_emit_pass(GvarRef F, const GvarPositionRef *positions, uint32_t np, uint32_t *counts,
                                                                   const uint32_t *pt_at)
{
	__shared__ uint32_t stack[kGvarLevels][kGvarFrameWords][kGvarLanes];
	constexpr bool EMIT = true;
	const uint32_t lane = threadIdx.x, pair = blockIdx.x * kGvarLanes + lane, gid = pair / np;
	const GvarPositionRef R = positions[pair % np];
	const float *acc = R.acc;
	const uint32_t *cmd_off = R.cmd_off, *dat_off = R.dat_off;
	uint8_t *kinds = R.kinds;
	float *coords = R.coords;
	uint32_t *flags = R.flags;
#include "gvar_tree_walk.inc"
}

} // namespace
} // namespace vgsdf

extern "C" {

int vgsdf_gvar_batch_deltas(const vgsdf::GvarRef *face, uint32_t g0, uint32_t g1, uint32_t p0, uint32_t p1, const int16_t *coords_all,
                            const uint32_t *counts, const uint32_t *pt_at, float *acc, uint64_t acc_stride, const vgsdf::GvarScratch *scratch,
                            uint32_t slice, uint32_t *flags, hipStream_t stream)
{
	const uint32_t np = p1 - p0, groups = ((g1 - g0) * np + vgsdf::kGvarLanes - 1) / vgsdf::kGvarLanes;
	hipLaunchKernelGGL(vgsdf::gvar_batch_deltas_pass, dim3(groups), dim3(vgsdf::kGvarLanes), 0, stream, *face, g0, g1, p0, np, coords_all, counts,
	                   pt_at, acc, acc_stride, *scratch, slice, flags);
	return (int)hipGetLastError();
}

int vgsdf_gvar_batch_emit(const vgsdf::GvarRef *face, const vgsdf::GvarPositionRef *positions, uint32_t n_positions, const uint32_t *counts,
                          const uint32_t *pt_at, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids * n_positions + vgsdf::kGvarLanes - 1) / vgsdf::kGvarLanes;
	hipLaunchKernelGGL(vgsdf::gvar_batch_emit_pass, dim3(groups), dim3(vgsdf::kGvarLanes), 0, stream, *face, positions, n_positions,
	                   (uint32_t *)counts, pt_at);
	return (int)hipGetLastError();
}

} // extern "C"
