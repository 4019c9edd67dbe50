// sdf_margin_kernels.hip — `make margins` only (build/margins/libvgsdf.so; never part of the product library).
//
// Extra stampings of the default raster kernel (sdf_span_kernel.inc) that measure whether the test suite can see a
// numerical margin of DESIGN.md §4.1 that is WRONG: `base` (today's margins: must equal product variant 0 byte for byte),
// `count` (counters instead of pixels' timing: which branches a set of inputs reaches), and the weakened instances, each
// with one margin switched off (and, for three of them, at 1/2, 1/4, 1/8 of its value).  A weakened instance changes
// arithmetic only — a constant, or the outcome of a float comparison; never an index, a loop bound, an LDS size, a
// barrier or an address — so it touches no memory the product kernel does not touch.  It is expected to give wrong
// bytes on the directed sets of tests/raster_margin_sets.py; tests/test_gpu_raster_margins.py asserts that it does.
// (Instance 84, the stage's row margin: tests/stage_filter_sets.py and tests/test_gpu_stage_filters.py.)
//
// The file is compiled VG_MARGIN_PARTS times with -DVG_MARGIN_PART=0..6 (up to four instances each: the instances compile
// in parallel).  Kernel ids = vgsdf_set_variant ids 60..84, known to this build only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdf_span_support.h"

#ifndef VG_MARGIN_PART
#error "compile with -DVG_MARGIN_PART=0..6"
#endif
#define VG_MARGIN_PARTS 7
#define VG_CAT_(a, b) a##b
#define VG_CAT(a, b) VG_CAT_(a, b)

namespace vgsdf {

typedef void (*span_fn)(const SpanRec *, uint32_t, const double *, const double *, const double *, const double *,
                        uint32_t, uint8_t *, const float4 *, const PlanHeader *);
struct MarginInstance {
	int id;
	span_fn fn;
};

#if VG_MARGIN_PART == 0
// ---- 60 base: today's margins ----
#define VG_SPAN_KERNEL sdf_margin_span_base
#include "sdf_span_kernel.inc"
// ---- 61 count: VG_COUNT on, VG_STAMP off; counters summed per wave into g_span_dbg (vgsdf_margin_counters) ----
__device__ unsigned long long g_span_dbg[28];
#define VG_SPAN_KERNEL sdf_margin_span_count
#define VG_SPAN_COUNTED 1
#define VG_COUNT(stmt) stmt
#include "sdf_span_kernel.inc"
#undef VG_SPAN_COUNTED
// ---- 62 (a) dl := 0 and no `8 e <= f1`: the byte comes from the f32 bin whenever the pixel is not `far` ----
#define VG_SPAN_KERNEL sdf_margin_span_dl0
#define VG_M_DL(dl) ((void)(dl), 0.0f)
#define VG_M_E8(e, f1) ((void)(e), (void)(f1), true)
#include "sdf_span_kernel.inc"
// ---- 63 (b) e := 0 (h(F) and e64): the interval collapses in decide, in the carried bound and in Tk ----
#define VG_SPAN_KERNEL sdf_margin_span_e0
#define VG_M_E(e) ((void)(e), 0.0f)
#define VG_M_E64(e) ((void)(e), 0.0f)
#include "sdf_span_kernel.inc"
static const MarginInstance k_instances[] = {{60, sdf_margin_span_base}, {61, sdf_margin_span_count}, {62, sdf_margin_span_dl0}, {63, sdf_margin_span_e0}};

#elif VG_MARGIN_PART == 1
// ---- 64 (c) Tk := f1: only the filter's argmin (and its exact ties) is evaluated exactly ----
#define VG_SPAN_KERNEL sdf_margin_span_tkf1
#define VG_M_TK(tk, f1) ((void)(tk), (f1))
#include "sdf_span_kernel.inc"
// ---- 65 (d) r_g := 0 in the phase-1 candidate rule ----
#define VG_SPAN_KERNEL sdf_margin_span_rg0
#define VG_M_RG(r) ((void)(r), 0.0f)
#include "sdf_span_kernel.inc"
// ---- 66 (e) SAT 6.2 -> 3.0 in phase 1 (below the 5.97 px saturation distance outside) ----
#define VG_SPAN_KERNEL sdf_margin_span_sat3
#define VG_M_SAT 3.0f
#include "sdf_span_kernel.inc"
// ---- 67 (f) `far` 35.9 -> 20 ----
#define VG_SPAN_KERNEL sdf_margin_span_far20
#define VG_M_FAR 20.0f
#include "sdf_span_kernel.inc"
static const MarginInstance k_instances[] = {{64, sdf_margin_span_tkf1}, {65, sdf_margin_span_rg0}, {66, sdf_margin_span_sat3}, {67, sdf_margin_span_far20}};

#elif VG_MARGIN_PART == 2
// ---- 68 (g) `sane` always true: the filter is trusted at M >= 10^6 ----
#define VG_SPAN_KERNEL sdf_margin_span_sane
#define VG_M_SANE(Mc) ((void)(Mc), true)
#include "sdf_span_kernel.inc"
// ---- 69 (h) `bounded` always true: the group bounds are trusted at M >= 4096 ----
#define VG_SPAN_KERNEL sdf_margin_span_bounded
#define VG_M_BOUNDED(Mc) ((void)(Mc), true)
#include "sdf_span_kernel.inc"
// ---- 70 (i) chunk-box skip with R := 0 ----
#define VG_SPAN_KERNEL sdf_margin_span_boxr0
#define VG_M_BOX_R(r) ((void)(r), 0.0f)
#include "sdf_span_kernel.inc"
// ---- 71 (j) chunk-box skip without the row-band condition dy > 0 ----
#define VG_SPAN_KERNEL sdf_margin_span_boxband
#define VG_M_BOX_BAND(dy) ((void)(dy), true)
#include "sdf_span_kernel.inc"
static const MarginInstance k_instances[] = {{68, sdf_margin_span_sane}, {69, sdf_margin_span_bounded}, {70, sdf_margin_span_boxr0}, {71, sdf_margin_span_boxband}};

#elif VG_MARGIN_PART == 3
// ---- 72 (k) e64 := 0 alone ----
#define VG_SPAN_KERNEL sdf_margin_span_e64
#define VG_M_E64(e) ((void)(e), 0.0f)
#include "sdf_span_kernel.inc"
// ---- 73 (k) mabs0 := 0 alone ----
#define VG_SPAN_KERNEL sdf_margin_span_mabs0
#define VG_M_MABS0(m) ((void)(m), 0.0f)
#include "sdf_span_kernel.inc"
// ---- 74 (l) INFL, pad and 1.004 := 1 / 0 / 1 ----
#define VG_SPAN_KERNEL sdf_margin_span_infl
#define VG_M_INFL 1.0f
#define VG_M_PAD(Mc) ((void)(Mc), 0.0f)
#define VG_M_GRP_SLACK 1.0f
#include "sdf_span_kernel.inc"
// ---- graded record: 75 e / 2 ----
#define VG_SPAN_KERNEL sdf_margin_span_e_2
#define VG_M_E(e) ((e) * 0.5f)
#include "sdf_span_kernel.inc"
static const MarginInstance k_instances[] = {{72, sdf_margin_span_e64}, {73, sdf_margin_span_mabs0}, {74, sdf_margin_span_infl}, {75, sdf_margin_span_e_2}};

#elif VG_MARGIN_PART == 4
// ---- graded record: 76, 77 e / 4, e / 8; 78, 79 dl / 2, dl / 4 ----
#define VG_SPAN_KERNEL sdf_margin_span_e_4
#define VG_M_E(e) ((e) * 0.25f)
#include "sdf_span_kernel.inc"
#define VG_SPAN_KERNEL sdf_margin_span_e_8
#define VG_M_E(e) ((e) * 0.125f)
#include "sdf_span_kernel.inc"
#define VG_SPAN_KERNEL sdf_margin_span_dl_2
#define VG_M_DL(dl) ((dl) * 0.5f)
#include "sdf_span_kernel.inc"
#define VG_SPAN_KERNEL sdf_margin_span_dl_4
#define VG_M_DL(dl) ((dl) * 0.25f)
#include "sdf_span_kernel.inc"
static const MarginInstance k_instances[] = {{76, sdf_margin_span_e_4}, {77, sdf_margin_span_e_8}, {78, sdf_margin_span_dl_2}, {79, sdf_margin_span_dl_4}};

#elif VG_MARGIN_PART == 5
// ---- graded record: 80 dl / 8; 81, 82, 83 r_g / 2, / 4, / 8 ----
#define VG_SPAN_KERNEL sdf_margin_span_dl_8
#define VG_M_DL(dl) ((dl) * 0.125f)
#include "sdf_span_kernel.inc"
#define VG_SPAN_KERNEL sdf_margin_span_rg_2
#define VG_M_RG(r) ((r) * 0.5f)
#include "sdf_span_kernel.inc"
#define VG_SPAN_KERNEL sdf_margin_span_rg_4
#define VG_M_RG(r) ((r) * 0.25f)
#include "sdf_span_kernel.inc"
#define VG_SPAN_KERNEL sdf_margin_span_rg_8
#define VG_M_RG(r) ((r) * 0.125f)
#include "sdf_span_kernel.inc"
static const MarginInstance k_instances[] = {{80, sdf_margin_span_dl_8}, {81, sdf_margin_span_rg_2}, {82, sdf_margin_span_rg_4}, {83, sdf_margin_span_rg_8}};
#elif VG_MARGIN_PART == 6
// ---- 84 (m) E_row := 0: the stage takes a segment's bracket of rows from the f32 record wherever the record is finite ----
#define VG_SPAN_KERNEL sdf_margin_span_row_e0
#define VG_M_ROW_E(e) ((void)(e), 0.0f)
#include "sdf_span_kernel.inc"
static const MarginInstance k_instances[] = {{84, sdf_margin_span_row_e0}};

#else
#error "VG_MARGIN_PART out of range"
#endif

} // namespace vgsdf

// this part's instances: 0 launched (or the HIP error), -1 not one of mine
extern "C" __attribute__((visibility("hidden"))) int VG_CAT(vgsdf_margin_launch_p, VG_MARGIN_PART)(
    int kernel, uint32_t grid, uint32_t n_tiles_arg, const vgsdf::SpanRec *tiles, const double *sx, const double *sy,
    const double *ex, const double *ey, uint32_t seg_stride, uint8_t *out, const void *boxes, hipStream_t stream)
{
	for (const vgsdf::MarginInstance &m : vgsdf::k_instances)
		if (m.id == kernel) {
			hipLaunchKernelGGL(m.fn, dim3(grid), dim3(vgsdf::TPB), 0, stream, tiles, n_tiles_arg, sx, sy, ex, ey, seg_stride, out,
			                   (const float4 *)boxes, (const vgsdf::PlanHeader *)nullptr);
			return (int)hipGetLastError();
		}
	return -1;
}

#if VG_MARGIN_PART == 0
#define VG_MARGIN_PART_ARGS                                                                                                          \
	int kernel, uint32_t grid, uint32_t n_tiles_arg, const vgsdf::SpanRec *tiles, const double *sx, const double *sy, \
	    const double *ex, const double *ey, uint32_t seg_stride, uint8_t *out, const void *boxes, hipStream_t stream
extern "C" int vgsdf_margin_launch_p1(VG_MARGIN_PART_ARGS);
extern "C" int vgsdf_margin_launch_p2(VG_MARGIN_PART_ARGS);
extern "C" int vgsdf_margin_launch_p3(VG_MARGIN_PART_ARGS);
extern "C" int vgsdf_margin_launch_p4(VG_MARGIN_PART_ARGS);
extern "C" int vgsdf_margin_launch_p5(VG_MARGIN_PART_ARGS);
extern "C" int vgsdf_margin_launch_p6(VG_MARGIN_PART_ARGS);

extern "C" int vgsdf_margin_known(int kernel) { return kernel >= 60 && kernel <= 84; }

// called by vgsdf_launch_tiles of the margins build for the ids vgsdf_margin_known accepts
extern "C" int vgsdf_margin_launch(VG_MARGIN_PART_ARGS)
{
	int (*const parts[VG_MARGIN_PARTS])(VG_MARGIN_PART_ARGS) = {vgsdf_margin_launch_p0, vgsdf_margin_launch_p1, vgsdf_margin_launch_p2,
	                                                            vgsdf_margin_launch_p3, vgsdf_margin_launch_p4, vgsdf_margin_launch_p5,
	                                                            vgsdf_margin_launch_p6};
	for (auto part : parts) {
		const int e = part(kernel, grid, n_tiles_arg, tiles, sx, sy, ex, ey, seg_stride, out, boxes, stream);
		if (e != -1)
			return e;
	}
	return (int)hipErrorInvalidValue;
}

// Counters of the `count` instance (id 61), summed over every launch since the last reset.  out[0..7]: workgroups' waves,
// (pixel, group) pairs of phase 2, pooled rounds, wave tile-chunks, waves with undecided lanes, undecided lanes,
// waves whose phase-2 pool overflowed QCAP, waves with 1..VG_POOL_MAX undecided lanes (pooled exact evaluation),
// waves with more (every lane for itself) — nine values.  Call with the context's work complete (after a download).
extern "C" int vgsdf_margin_counters(unsigned long long *out, int reset)
{
	unsigned long long h[28] = {0};
	hipError_t e = hipSuccess;
	if (out != nullptr) {
		e = hipMemcpyFromSymbol(h, HIP_SYMBOL(vgsdf::g_span_dbg), sizeof(h), 0, hipMemcpyDeviceToHost);
		static const int idx[9] = {12, 13, 14, 15, 16, 17, 20, 21, 22};
		for (int i = 0; i < 9; i++)
			out[i] = h[idx[i]];
	}
	if (e == hipSuccess && reset) {
		const unsigned long long z[28] = {0};
		e = hipMemcpyToSymbol(HIP_SYMBOL(vgsdf::g_span_dbg), z, sizeof(z), 0, hipMemcpyHostToDevice);
	}
	return (int)e;
}

// The `count` instance's counters of phase 2's pair rounds, behind the nine above (which keep their places): out[0..1] =
// half rounds taken, sweeps that left behind phase 1 without a pair.  Same accumulation; vgsdf_margin_counters resets these too.
extern "C" int vgsdf_margin_pair_round_counters(unsigned long long *out)
{
	unsigned long long h[28] = {0};
	const hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(vgsdf::g_span_dbg), sizeof(h), 0, hipMemcpyDeviceToHost);
	for (int i = 0; i < 2; i++)
		out[i] = h[23 + i];
	return (int)e;
}

// The `count` instance's counter of the stage's f32 decision, behind those: out[0] = waves of a chunk whose f64 brackets ran (a
// lane's end point within E_row of a row centre).  Same accumulation; vgsdf_margin_counters resets it too.
extern "C" int vgsdf_margin_stage_filter_counters(unsigned long long *out)
{
	unsigned long long h[28] = {0};
	const hipError_t e = hipMemcpyFromSymbol(h, HIP_SYMBOL(vgsdf::g_span_dbg), sizeof(h), 0, hipMemcpyDeviceToHost);
	out[0] = h[25];
	return (int)e;
}
#endif
