// gvar_kernels.hip — a placed `glyf` face's command store from its `loca`, `glyf` and `gvar` tables (gvar_kernels.h).  What a
// lane does for its glyph id is, step for step, the host reader's share for that glyph id (host/ttf_face.cpp): GvarWalker::walk
// over Face::glyph_data's loca rules, walk_simple's reader of a simple entry, read_component's records, GvarTable::accumulate
// (rules G1 to G5 of host/ttf_face.hpp) for the glyph id's own entry, Affine::then / map and ContourEmitter in f32 (this unit is
// built with -ffp-contract=off).  Every entry's sums are the same wherever in a tree it is met, so the deltas pass computes them
// once per glyph id and the emit pass reads them by glyph id.
// The tree walk has the shape of glyf_table_walk.inc — a loop over an explicit stack in LDS, the composite being read in
// registers — but is a text of its own: a record's offsets take the composite's sums BEFORE the transforms are combined (G6) and
// a leaf is decoded here instead of being described, and that file has no place for either.  Every read is bounded by
// loca_entries / glyf_len / gvar_len, every store of the deltas pass by the glyph id's counted points, every store of the emit
// pass by the ranges the count pass of the same text has sized.
// The text itself is in three files that gvar_batch_kernels.hip (one face at many positions) compiles too: gvar_device.inc (the
// readers, the emitter, accumulate), gvar_tree_walk.inc (the body of the count and emit kernels) and gvar_own_deltas.inc (the body
// of the deltas kernel); here are the kernels of one face at one position and their launchers.
#include "gvar_kernels.h"

#include "glyf_table_limits.h"
#include "gvar_limits.h"

namespace vgsdf {
namespace {

#include "gvar_device.inc"

// ---- GvarWalker::walk: the component tree of one glyph id; count and emit are this one text -----------------------------
template <bool EMIT>
__global__ __launch_bounds__(kGvarLanes) void gvar_tree_pass(GvarRef F, uint32_t *counts, const uint32_t *pt_at, const float *acc,
                                                             const uint32_t *cmd_off, const uint32_t *dat_off, uint8_t *kinds, float *coords,
                                                             uint32_t *flags)
{
	__shared__ uint32_t stack[kGvarLevels][kGvarFrameWords][kGvarLanes];
	const uint32_t lane = threadIdx.x, gid = blockIdx.x * kGvarLanes + lane;
#include "gvar_tree_walk.inc"
}

__global__ __launch_bounds__(kGvarLanes) void gvar_deltas_pass(GvarRef F, uint32_t g0, uint32_t g1, const uint32_t *counts,
                                                               const uint32_t *pt_at, float *acc_all, GvarScratch S, uint32_t *flags)
{
	const uint32_t gid = g0 + blockIdx.x * kGvarLanes + threadIdx.x;
	if (gid >= g1)
		return;
#include "gvar_own_deltas.inc"
}

} // namespace
} // namespace vgsdf

extern "C" {

int vgsdf_gvar_count(const vgsdf::GvarRef *face, uint32_t *counts, uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids + vgsdf::kGvarLanes - 1) / vgsdf::kGvarLanes;
	hipLaunchKernelGGL(vgsdf::gvar_tree_pass<false>, dim3(groups), dim3(vgsdf::kGvarLanes), 0, stream, *face, counts, (const uint32_t *)nullptr,
	                   (const float *)nullptr, (const uint32_t *)nullptr, (const uint32_t *)nullptr, (uint8_t *)nullptr, (float *)nullptr, flags);
	return (int)hipGetLastError();
}

int vgsdf_gvar_deltas(const vgsdf::GvarRef *face, uint32_t g0, uint32_t g1, const uint32_t *counts, const uint32_t *pt_at, float *acc,
                      const vgsdf::GvarScratch *scratch, uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (g1 - g0 + vgsdf::kGvarLanes - 1) / vgsdf::kGvarLanes;
	hipLaunchKernelGGL(vgsdf::gvar_deltas_pass, dim3(groups), dim3(vgsdf::kGvarLanes), 0, stream, *face, g0, g1, counts, pt_at, acc, *scratch,
	                   flags);
	return (int)hipGetLastError();
}

int vgsdf_gvar_emit(const vgsdf::GvarRef *face, const uint32_t *counts, const uint32_t *pt_at, const float *acc, const uint32_t *cmd_off,
                    const uint32_t *dat_off, uint8_t *kinds, float *coords, uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids + vgsdf::kGvarLanes - 1) / vgsdf::kGvarLanes;
	hipLaunchKernelGGL(vgsdf::gvar_tree_pass<true>, dim3(groups), dim3(vgsdf::kGvarLanes), 0, stream, *face, (uint32_t *)counts, pt_at, acc,
	                   cmd_off, dat_off, kinds, coords, flags);
	return (int)hipGetLastError();
}

} // extern "C"
