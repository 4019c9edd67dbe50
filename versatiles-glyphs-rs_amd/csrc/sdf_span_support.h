// sdf_span_support.h — device helpers shared by the raster kernels of sdf_kernels.hip and by every stamping of
// sdf_span_kernel.inc (the product instance there; the margin instances of sdf_margin_kernels.hip, `make margins`).
// NOTE for profiles/traffic.json: bench.py keys the recorded PMC numbers of the raster kernel to the text of sdf_kernels.hip,
// sdf_span_kernel.inc and sdf_kernels.h only.  This header holds code of that kernel too (filter_err, sc_filter, quantise,
// exact_dist_sq, pix_pack and its readers) and is NOT part of that key: after an edit here that changes the kernel's instructions, collect the profile
// again (tools/profile.sh) or remove the entries, or bench.py keeps reporting numbers of the old instructions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "outline_kernels.h" // PlanHeader (guard of the chunk-box pass behind the device front-end)
#include "sdf_kernels.h"

namespace vgsdf {

constexpr int TPB = VGSDF_TILE_PIXELS; // 256 threads, one pixel each

// What the span kernel reads in place of a plan when it is launched without one (a resident batch: the host planned it):
// "ok", and every workgroup of the grid inside the list.  One scalar load for both cases, issued beside the load of the
// work-list entry (constant address space: the load stays scalar behind the choice between the two addresses; a plan is
// complete before the launch behind it starts).
typedef const __attribute__((address_space(4))) PlanHeader *plan_ptr;
static __constant__ const PlanHeader k_plan_absent = {0ull, 0ull, 0u, 0xFFFFFFFFu, 0u, 1u};

// Blocks are dealt round-robin over the 8 XCDs (b and b+8 share an L2).  Remap so that
// each XCD walks a contiguous range of tiles: tiles of one glyph (which re-read the same
// segment list) then hit the same L2.  Pure performance hint; any placement is correct.
__device__ __forceinline__ uint32_t xcd_remap(uint32_t b, uint32_t n_and_flag)
{
	constexpr uint32_t X = 8;
	if (n_and_flag & 0x80000000u) // host asked for dispatch order == list order
		return b;
	const uint32_t n = n_and_flag;
	uint32_t per = n / X, rem = n % X;
	uint32_t xcd = b % X, idx = b / X;
	// XCDs [0, rem) own per+1 tiles, the rest own per tiles
	uint32_t start = xcd * per + (xcd < rem ? xcd : rem);
	return start + idx;
}

// Rust `n.round() as u8` on a value already clamped to [0,255]
__device__ __forceinline__ uint8_t quantise(double best_sq, bool inside)
{
	double d = sqrt(best_sq);            // rtree_segments.rs:67 (correctly rounded)
	if (inside)
		d = -d;                          // renderer_precise.rs:71-73
	d = d * (256.0 / 8.0) + 64.0;        // :75  (two roundings, no FMA)
	double n = 255.0 - d;                // :76
	n = n < 0.0 ? 0.0 : n;
	n = n > 255.0 ? 255.0 : n;
	return (uint8_t)(int)round(n);       // :79  half away from zero
}

// Exact squared distance from p to segment (v,w): Segment::squared_distance_to_point,
// segment.rs:54-72,96-99 with Point::squared_distance_to, point.rs:38-42.  dx,dy,l2 are the
// reference's (w.x - v.x), (w.y - v.y) and v.squared_distance_to(w), bit for bit.
__device__ __forceinline__ double exact_dist_sq(double px, double py, double vx, double vy, double wx,
                                                double wy, double dx, double dy, double l2)
{
	const double pvx = px - vx, pvy = py - vy;
	const double t = (pvx * dx + pvy * dy) / l2; // NaN when l2 == 0 (0/0): masked by at_v below
	double qx = vx + t * dx, qy = vy + t * dy;
	const bool at_v = (l2 == 0.0) | (t < 0.0); // segment.rs:59-61, :65-66
	const bool at_w = t > 1.0;                 // :67-68
	qx = at_w ? wx : qx;
	qy = at_w ? wy : qy;
	qx = at_v ? vx : qx;
	qy = at_v ? vy : qy;
	const double ex = qx - px, ey = qy - py; // point.rs:39-40 (other - self)
	return ex * ex + ey * ey;
}

// ---------------------------------------------------------------------------------------
// Shared pieces of the filtered kernels (the default kernel at the end of sdf_kernels.hip, and the earlier
// generations kept in tools/experiments/sdf_retired.inc for development builds).
// ---------------------------------------------------------------------------------------
constexpr int FCHUNK = 256;      // segments per LDS stage: 20 B filter record + 32 B exact end points each
constexpr int DELTA_CAP = 2048;  // winding histogram cells per span: rows * (w + 1)

// smallest integer n in [A, B] with (double)n + c >= v   (B if none): exact f64 compares
__device__ __forceinline__ int first_ge(double v, double c, int A, int B)
{
	double a = ceil(v - c);
	a = a < (double)A ? (double)A : a;
	a = a > (double)B ? (double)B : a; // NaN ends up inside [A, B] too; the compares below are then false
	int n = (int)a;
	if (n > A && (double)(n - 1) + c >= v)
		n--;
	else if (n < B && (double)n + c < v)
		n++;
	return n;
}

// ---- The stage's f32 decision ahead of first_ge (sdf_span_kernel.inc; derivation in DESIGN.md §4.1, "The stage's integers").
// A segment's bracket of sample rows is ceil(t) of a real t that the f32 record gives to within a bound E_row: when t lies
// farther than E_row from every integer, ceil of the f32 value IS the exact integer, and only the other lanes take first_ge.
constexpr float STAGE_U = 5.9604644775390625e-08f;    // u = 2^-24
constexpr float STAGE_ROW_C = 6.0f * STAGE_U;         // E_row = 6 u M + 2^-22
constexpr float STAGE_ROW_ABS = 2.384185791015625e-07f;
constexpr float STAGE_M_MAX = 1.0e6f;                 // at and beyond it (the sweep's `sane`), and for a NaN, first_ge decides

// distance of a finite t from the nearest integer (v_fract_f32 is exact; 1 - fr rounds once, inside the bound's absolute term)
__device__ __forceinline__ float int_dist(float t)
{
	const float fr = __builtin_amdgcn_fractf(t);
	return __builtin_fminf(fr, 1.0f - fr);
}

// h(F): bound on |Ft - D| for a filter value F, coordinates bounded by M:
// 64 u M sqrt(F) + 32 u F + 2^-34 M^2 with u = 2^-24, evaluated with upward slack.
// The constants by name (defaults = the analysed values; only a `make margins` instance overrides one, see
// sdf_margin_kernels.hip): the span kernel's decide step uses the same ones in its fused form of h(F) + e64.
#ifndef VG_HERR_SLACK
#define VG_HERR_SLACK 1.001f               // covers the roundings of evaluating h itself
#endif
#ifndef VG_HERR_C1
#define VG_HERR_C1 3.814697265625e-06f     // 64 u
#endif
#ifndef VG_HERR_C2
#define VG_HERR_C2 1.9073486328125e-06f    // 32 u
#endif
#ifndef VG_HERR_C2S
#define VG_HERR_C2S 1.9092559814453125e-06f // VG_HERR_SLACK * VG_HERR_C2, one literal (the decide step's fused form)
#endif
#ifndef VG_HERR_C3
#define VG_HERR_C3 5.820766091346741e-11f  // 2^-34
#endif
#ifndef VG_E64_C
#define VG_E64_C 5.6843418860808015e-14f   // 2^-44: e64 = 2^-44 M (M + Mabs)
#endif
__device__ __forceinline__ float filter_err(float F, float M)
{
	return VG_HERR_SLACK * (VG_HERR_C1 * M * __builtin_sqrtf(F) + VG_HERR_C2 * F +
	                        VG_HERR_C3 * M * M);
}

__device__ __forceinline__ float sc_filter(float rpx, float rpy, float vx, float vy, float dx, float dy, float inv)
{
	const float pvx = rpx - vx, pvy = rpy - vy;
	const float t = __builtin_amdgcn_fmed3f(__builtin_fmaf(pvy, dy, pvx * dx) * inv, 0.0f, 1.0f);
	const float ex = __builtin_fmaf(-t, dx, pvx), ey = __builtin_fmaf(-t, dy, pvy);
	return __builtin_fmaf(ey, ey, ex * ex);
}

constexpr uint32_t SPAN_TILES = 4; // tiles a workgroup of the default kernel sweeps per staged chunk

// A pixel of a span in 4 bytes (the span kernel's st_pix): rpx = column - (w >> 1) + 0.5 as an f16 in the low half, the row's
// offset from the span's first row in the high half.  Exact for every bitmap the span kernel is given: the planner admits
// a width only if two histogram rows fit DELTA_CAP (work_plan.h, span_fits: 2 (w + 2) <= 2048), so w <= 1022, 2 rpx is an odd
// integer of magnitude <= 1023 (column 0 .. w - 1 against w >> 1 <= 511) and fits the 11-bit significand of an f16 at an
// exponent far inside its range; a span touches at most DELTA_CAP / (w + 1) < 1024 rows.  The height is not bounded that way,
// which is why the row is kept as an offset and not as a coordinate.
__device__ __forceinline__ uint32_t pix_pack(float rpx, uint32_t row_off)
{
	return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)rpx) | (row_off << 16);
}
__device__ __forceinline__ float pix_rpx(uint32_t e) { return (float)__builtin_bit_cast(_Float16, (uint16_t)e); }
__device__ __forceinline__ uint32_t pix_roff(uint32_t e) { return e >> 16; }
__device__ __forceinline__ int pix_col(float rpx, int hw) { return (int)(rpx - 0.5f) + hw; } // (rpx - 0.5 is an integer: exact)

// The rotation of workgroup b (sdf_span_kernel.inc: wave wv takes the 64-pixel quarter (wv + rot) & 3 of every tile): 0..3,
// wave-uniform, scalar arithmetic only.  The top two bits of a multiplicative hash: workgroups are dealt round-robin
// over the 8 XCDs and then over an XCD's CUs, so the workgroups that share a CU have equal low bits of b.
// tools/model_wave_shares.py restates this function and checks what it does to the three font batches.
constexpr uint32_t WAVE_ROT_MUL = 0x13C6EF37u;
__device__ __forceinline__ uint32_t wave_rot(uint32_t b)
{
	return (b * WAVE_ROT_MUL) >> 30;
}

// ---------------------------------------------------------------------------------------
// Wave-level scans and reductions on DPP row shifts and row broadcasts: one VALU instruction per step (the DPP move folds
// into the add / max that consumes it), no LDS permute.  A lane without a source lane, or in a row the step masks off,
// reads 0, the identity of the two unsigned operations.
// ALL 64 LANES MUST BE ACTIVE at every call of wave_scan_add, wave_max_u32 and wave_min_f64 (an inactive lane is a hole in
// the chain of row shifts, and the two reductions read their result from lane 63), and all 8 of a run at oct_max_u32:
// call them from wave-uniform control flow only, as the stage and the sweep do.
// ---------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint32_t dpp_or_zero(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xF, true);
}

// inclusive prefix sum over the 64 lanes.  Written out: the compiler folds the DPP move into v_max_u32 (below) but leaves
// v_mov_b32_dpp + v_add_u32 for the sum.  A DPP operand must not be read in the two wait states behind the VALU
// instruction that wrote it, hence the s_nop 1 ahead of every step; the compiler pads nothing inside the statement and
// does not know that its input is read through DPP, so the first step waits for itself too, and for the five states a
// DPP instruction needs behind a VALU write of EXEC (v_cmpx).  In the rows a broadcast step masks off the destination
// keeps its value, which is the operand: "+v".
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v)
{
	asm("s_nop 4\n\t"
	    "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
	    "s_nop 1\n\t"
	    "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
	    "s_nop 1\n\t"
	    "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
	    "s_nop 1\n\t"
	    "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
	    "s_nop 1\n\t"
	    "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t" // -> rows 1, 3
	    "s_nop 1\n\t"
	    "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" // -> rows 2, 3
	    : "+v"(v));
	return v;
}

// maximum over the 64 lanes, wave-uniform (lane 63 of the same six steps holds it)
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
	v = max(v, dpp_or_zero<0x111, 0xF>(v));
	v = max(v, dpp_or_zero<0x112, 0xF>(v));
	v = max(v, dpp_or_zero<0x114, 0xF>(v));
	v = max(v, dpp_or_zero<0x118, 0xF>(v));
	v = max(v, dpp_or_zero<0x142, 0xA>(v));
	v = max(v, dpp_or_zero<0x143, 0xC>(v));
	return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// maximum over each aligned run of 8 lanes, in all 8 of them
__device__ __forceinline__ uint32_t oct_max_u32(uint32_t v)
{
	v = max(v, dpp_or_zero<0xB1, 0xF>(v));  // quad_perm:[1,0,3,2]
	v = max(v, dpp_or_zero<0x4E, 0xF>(v));  // quad_perm:[2,3,0,1]
	v = max(v, dpp_or_zero<0x141, 0xF>(v)); // row_half_mirror: lane i of the 8 <-> lane 7 - i
	return v;
}

// minimum over the 64 lanes of values that are never NaN, wave-uniform.  (v_min_f64 has no DPP form: two moves per step;
// a lane without a source lane, or in a masked row, reads its own value.)
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_min_f64(double v)
{
	const int lo = __double2loint(v), hi = __double2hiint(v);
	const double other = __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false),
	                                      __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false));
	return other < v ? other : v;
}
__device__ __forceinline__ double wave_min_f64(double v)
{
	v = dpp_min_f64<0x111, 0xF>(v);
	v = dpp_min_f64<0x112, 0xF>(v);
	v = dpp_min_f64<0x114, 0xF>(v);
	v = dpp_min_f64<0x118, 0xF>(v);
	v = dpp_min_f64<0x142, 0xA>(v);
	v = dpp_min_f64<0x143, 0xC>(v);
	return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

} // namespace vgsdf
