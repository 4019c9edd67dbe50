// sdf_kernels.hip — hand-written HIP kernels (gfx950 / CDNA4) for the SDF raster.
//
// What it computes, per glyph and per output pixel (bit-exact with the reference):
//   renderer_precise()              /root/reference/src/render/renderer_precise.rs:8-84
//   min_distance_to_line_segment()  src/render/rtree_segments.rs:40-68
//   Segment::project_point_on / squared_distance_to_point   src/geometry/segment.rs:54-99
//   Point::squared_distance_to      src/geometry/point.rs:38-42
//
// Arithmetic contract: IEEE binary64, every operation rounded separately (compiled with
// -ffp-contract=off: no v_fma/v_fmac contraction of a*b+c), correctly rounded divide and
// sqrt, round-half-away quantisation.  Winding sign is the order-independent sum the
// reference builds with a sorted sweep (renderer_precise.rs:41-67).
//
// Mapping (MI355X): a "tile" = 256 consecutive OUTPUT bytes of one glyph bitmap (stores are
// coalesced row-major), one pixel per lane of a 256-thread workgroup (4 wave64).  Segments are
// staged through LDS in chunks of 256.  The default kernel (sdf_tiles_span, at the end of this
// file) sweeps up to 4 tiles of a glyph per staged chunk and looks, per pixel, only at the runs of
// the outline that bounds cannot rule out; the earlier generations above it are kept for A/B
// measurements and as independent bit-exact implementations in the tests.  The path is VALU bound,
// not HBM bound: see DESIGN.md §4 for the algorithm, the exactness argument and the roofline.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>

#include "sdf_span_support.h" // TPB, FCHUNK, quantise, exact_dist_sq, first_ge, filter_err, sc_filter: shared with the margin instances

namespace vgsdf {

constexpr int SEG_CHUNK = 512; // segments per LDS stage: 7 * 512 * 8 B = 28 KiB

// ---------------------------------------------------------------------------------------
// Variant 1: brute force.  Every pixel evaluates every segment.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void sdf_tiles_brute(const SpanRec *__restrict__ tiles,
                                                       uint32_t n_tiles,
                                                       const double *__restrict__ seg_sx,
                                                       const double *__restrict__ seg_sy,
                                                       const double *__restrict__ seg_ex,
                                                       const double *__restrict__ seg_ey, uint32_t seg_stride,
                                                       uint8_t *__restrict__ out)
{
	__shared__ double s_vx[SEG_CHUNK], s_vy[SEG_CHUNK], s_wx[SEG_CHUNK], s_wy[SEG_CHUNK];
	__shared__ double s_dx[SEG_CHUNK], s_dy[SEG_CHUNK], s_l2[SEG_CHUNK];

	const uint32_t tile = xcd_remap(blockIdx.x, n_tiles);
	const SpanRec g = tiles[tile]; // (the glyph's descriptor travels in the entry)
	const uint32_t npix = g.w * g.h;
	const uint32_t o = g.first + threadIdx.x; // index into the glyph's output bitmap
	const bool active = o < npix;
	const uint32_t oc = active ? o : npix - 1;
	const uint32_t row = oc / g.w;       // output row (top row first)
	const uint32_t x = oc - row * g.w;
	const uint32_t y = g.h - 1 - row;    // renderer_precise.rs:78 inverts Y
	const double px = (double)x + ((double)g.x0 + 0.5); // :27,62
	const double py = (double)y + ((double)g.y0 + 0.5); // :28,34

	double best = __builtin_huge_val(); // rtree_segments.rs:57
	int wn = 0;

	for (uint32_t c0 = 0; c0 < g.n_seg; c0 += SEG_CHUNK) {
		const uint32_t cnt = min((uint32_t)SEG_CHUNK, g.n_seg - c0);
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < cnt; i += TPB) {
			const size_t s = (size_t)(g.seg_off + c0 + i) * seg_stride; // stride 1: four SoA arrays; 4: {sx, sy, ex, ey} records
			const double vx = seg_sx[s], vy = seg_sy[s], wx = seg_ex[s], wy = seg_ey[s];
			const double dx = wx - vx, dy = wy - vy; // segment.rs:63 (w.x - v.x), (w.y - v.y)
			s_vx[i] = vx;
			s_vy[i] = vy;
			s_wx[i] = wx;
			s_wy[i] = wy;
			s_dx[i] = dx;
			s_dy[i] = dy;
			s_l2[i] = dx * dx + dy * dy; // point.rs:38-42 v.squared_distance_to(w)
		}
		__syncthreads();

		for (uint32_t i = 0; i < cnt; i++) {
			const double vx = s_vx[i], vy = s_vy[i], wx = s_wx[i], wy = s_wy[i];
			const double dx = s_dx[i], dy = s_dy[i], l2 = s_l2[i];

			const double d2 = exact_dist_sq(px, py, vx, vy, wx, wy, dx, dy, l2);
			best = d2 < best ? d2 : best;                // rtree_segments.rs:60-62

			// --- winding: renderer_precise.rs:41-51, 63-66 ---
			const bool up = (vy <= py) & (wy > py);
			const bool down = (vy > py) & (wy <= py);
			if (up | down) {
				const double tc = (py - vy) / dy;        // e.y - s.y == dy bit for bit
				const double xc = vx + tc * dx;
				if (xc <= px)
					wn -= up ? 1 : -1;
			}
		}
	}

	if (active)
		out[g.out_off + o] = quantise(best, wn != 0);
}

#ifdef VGSDF_DEV_VARIANTS
} // namespace vgsdf
#include "sdf_retired.inc" // tools/experiments/: earlier kernel generations (A/B measurements, `make dev` only: -I../tools/experiments)
namespace vgsdf {
#endif

// ---------------------------------------------------------------------------------------
// Chunk boxes (batch preparation, run once per resident batch): the bounding box of every chunk
// of 256 consecutive segments of a glyph, in f32 relative to the glyph origin (x0, y0).  The span
// kernel reads one float4 per chunk and skips chunks that can neither cross its sample rows nor
// hold a segment within reach of its pixels: a glyph with a long segment list (Noto Sans has one
// with 4368 segments = 18 chunks) no longer drags every tile through every chunk, and its chain
// of chunks stops setting the makespan of a small batch.
// Index of chunk c of glyph g: (seg_off[g] >> 8) + g + c — unique for a monotone seg_off, so no
// offset table is needed; the table has (total segments >> 8) + n_glyphs + 1 entries.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sdf_chunk_boxes(const GlyphDesc *__restrict__ glyphs, uint32_t n_glyphs,
                                                      const double *__restrict__ seg_sx,
                                                      const double *__restrict__ seg_sy,
                                                      const double *__restrict__ seg_ex,
                                                      const double *__restrict__ seg_ey, uint32_t seg_stride,
                                                      float4 *__restrict__ boxes, const PlanHeader *__restrict__ guard,
                                                      unsigned long long seg_cap)
{
	// behind the device front-end: the segment arrays hold nothing (and are smaller than the descriptors say)
	// when the batch is in error or did not fit its capacity guess; the host then launches again
	if (guard != nullptr && (guard->error || guard->n_segments > seg_cap))
		return;
	// grid = (glyphs, CHUNK_BOX_Y): chunk c of a glyph is taken by the wave with blockIdx.y == c % gridDim.y, so
	// the 18 chunks of a long glyph are not walked one after the other by a single wave
	// one wave per (glyph, chunk mod gridDim.y); four glyphs per workgroup (fewer, larger workgroups to dispatch)
	const uint32_t gi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (gi >= n_glyphs)
		return;
	const GlyphDesc g = glyphs[gi];
	if (g.n_seg <= 2 * FCHUNK) // the span kernel asks for boxes only when a glyph has more than two chunks
		return;
	for (uint32_t c = blockIdx.y; (uint64_t)c * FCHUNK < g.n_seg; c += gridDim.y) {
		const uint32_t c0 = c * FCHUNK;
		const uint32_t cnt = min((uint32_t)FCHUNK, g.n_seg - c0);
		float x0 = __builtin_inff(), y0 = __builtin_inff(), x1 = -__builtin_inff(), y1 = -__builtin_inff();
		bool bad = false;
		for (uint32_t i = lane; i < cnt; i += 64) {
			const size_t s = (size_t)(g.seg_off + c0 + i) * seg_stride;
			const double rvx = seg_sx[s] - (double)g.x0, rvy = seg_sy[s] - (double)g.y0;
			const double rwx = seg_ex[s] - (double)g.x0, rwy = seg_ey[s] - (double)g.y0;
			const float a = (float)rvx, b = (float)rvy, cx = (float)rwx, d = (float)rwy;
			bad |= !(fabsf(a) < 3.0e38f) || !(fabsf(b) < 3.0e38f) || !(fabsf(cx) < 3.0e38f) || !(fabsf(d) < 3.0e38f);
			x0 = fminf(x0, fminf(a, cx));
			x1 = fmaxf(x1, fmaxf(a, cx));
			y0 = fminf(y0, fminf(b, d));
			y1 = fmaxf(y1, fmaxf(b, d));
		}
		for (int sh = 32; sh > 0; sh >>= 1) {
			x0 = fminf(x0, __shfl_xor(x0, sh));
			y0 = fminf(y0, __shfl_xor(y0, sh));
			x1 = fmaxf(x1, __shfl_xor(x1, sh));
			y1 = fmaxf(y1, __shfl_xor(y1, sh));
		}
		const bool any_bad = __any(bad);
		if (lane == 0) {
			// non-finite coordinates: a box that contains everything (the chunk is never skipped)
			const float inf = __builtin_inff();
			boxes[chunk_box_index(g.seg_off, gi, c)] = any_bad ? make_float4(-inf, -inf, inf, inf) : make_float4(x0, y0, x1, y1);
		}
	}
}

#include "sdf_span_kernel.inc" // the default kernel: bounded groups over spans (sdf_tiles_span)

#ifdef VGSDF_DEV_VARIANTS
// development builds: the same kernel source a second time, with in-kernel stamps (cdna_hip_programming.md, "In-kernel
// stamps": read the SHARES, never this instance's run time) and counters, summed per wave into g_span_dbg
__device__ unsigned long long g_span_dbg[28];
#define VG_SPAN_KERNEL sdf_tiles_span_stamped
#define VG_SPAN_STAMPED 1
#define VG_STAMP(region)                                                                      \
	do {                                                                                      \
		unsigned long long t_;                                                                \
		__builtin_amdgcn_sched_barrier(0);                                                    \
		asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");           \
		__builtin_amdgcn_sched_barrier(0);                                                    \
		if ((region) >= 0)                                                                    \
			st_acc[(region) < 0 ? 0 : (region)] += t_ - st_last;                              \
		st_last = t_;                                                                         \
	} while (0)
#define VG_COUNT(stmt) stmt
#include "sdf_span_kernel.inc"
#undef VG_SPAN_STAMPED
#endif

} // namespace vgsdf

// ---------------------------------------------------------------------------------------
// launchers (host)
// ---------------------------------------------------------------------------------------
extern "C" int vgsdf_filtered_delta_cap(void) { return vgsdf::DELTA_CAP; }

extern "C" size_t vgsdf_chunk_box_bytes(uint64_t n_segments, uint32_t n_glyphs)
{
	return sizeof(float4) * (size_t)((n_segments >> 8) + n_glyphs + 2);
}

extern "C" int vgsdf_launch_chunk_boxes(const vgsdf::GlyphDesc *glyphs, uint32_t n_glyphs, const double *sx, const double *sy,
                                        const double *ex, const double *ey, uint32_t seg_stride, void *boxes,
                                        const void *guard, unsigned long long seg_cap, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	hipLaunchKernelGGL(vgsdf::sdf_chunk_boxes, dim3((n_glyphs + 3) / 4, 8), dim3(256), 0, stream, glyphs, n_glyphs, sx, sy, ex, ey,
	                   seg_stride, (float4 *)boxes, (const vgsdf::PlanHeader *)guard, seg_cap);
	return (int)hipGetLastError();
}

// The span kernel over a work list that outline_plan is still writing when this is enqueued: `grid` workgroups
// (a guess >= plan->n_main, else plan->ok is 0 and nothing runs), list order.
extern "C" int vgsdf_launch_span_planned(const vgsdf::SpanRec *tiles, uint32_t grid, const double *sx,
                                         const double *sy, const double *ex, const double *ey, uint32_t seg_stride, uint8_t *out,
                                         const void *boxes, const void *plan, hipStream_t stream)
{
	if (grid == 0)
		return 0;
	hipLaunchKernelGGL(vgsdf::sdf_tiles_span, dim3(grid), dim3(vgsdf::TPB), 0, stream, tiles, grid | 0x80000000u, sx, sy,
	                   ex, ey, seg_stride, out, (const float4 *)boxes, (const vgsdf::PlanHeader *)plan);
	return (int)hipGetLastError();
}

// kernel ids: 50 = the bounded-group span kernel (public variant 0), 1 = brute force, also the fallback
// for the tiles the host routes there: glyphs too wide for the winding histogram, or with >= 2^24
// segments.  Everything else exists only in development builds (-DVGSDF_DEV_VARIANTS).
#ifdef VGSDF_MARGIN_VARIANTS
// `make margins` only: the margin instances of the span kernel (sdf_margin_kernels.hip), ids 60..84
extern "C" int vgsdf_margin_known(int kernel);
extern "C" int vgsdf_margin_launch(int kernel, uint32_t grid, uint32_t n_tiles_arg, const vgsdf::SpanRec *tiles,
                                   const double *sx, const double *sy, const double *ex, const double *ey, uint32_t seg_stride,
                                   uint8_t *out, const void *boxes, hipStream_t stream);
#endif

extern "C" int vgsdf_kernel_known(int kernel)
{
#ifdef VGSDF_MARGIN_VARIANTS
	if (vgsdf_margin_known(kernel))
		return 1;
#endif
#ifdef VGSDF_DEV_VARIANTS
	switch (kernel) {
	case 10: case 12: case 22: case 23: case 30: case 45: case 58:
		return 1;
	}
#endif
	return kernel == 1 || kernel == 50;
}

extern "C" int vgsdf_launch_tiles(int variant, int list_order, const vgsdf::SpanRec *tiles, uint32_t n_tiles_in, const double *sx,
                                  const double *sy, const double *ex, const double *ey, uint32_t seg_stride,
                                  uint8_t *out, const void *boxes, hipStream_t stream)
{
	if (n_tiles_in == 0)
		return 0;
	const dim3 grid(n_tiles_in);
	// kernel argument: tile count, top bit set = dispatch in list order (no per-XCD remap)
	const uint32_t n_tiles = n_tiles_in | (list_order ? 0x80000000u : 0u);
	if (variant == 1)
		hipLaunchKernelGGL(vgsdf::sdf_tiles_brute, grid, dim3(vgsdf::TPB), 0, stream, tiles, n_tiles, sx,
		                   sy, ex, ey, seg_stride, out);
	else if (variant == 50) // bounded groups over spans of up to 4 tiles (tile list: first pixel | T)
		hipLaunchKernelGGL(vgsdf::sdf_tiles_span, grid, dim3(vgsdf::TPB), 0, stream, tiles, n_tiles, sx, sy, ex, ey,
		                   seg_stride, out, (const float4 *)boxes, (const vgsdf::PlanHeader *)nullptr);
#ifdef VGSDF_MARGIN_VARIANTS
	else if (vgsdf_margin_known(variant))
		return vgsdf_margin_launch(variant, n_tiles_in, n_tiles, tiles, sx, sy, ex, ey, seg_stride, out, boxes, stream);
#endif
#ifdef VGSDF_DEV_VARIANTS
	// development builds only (`make dev`): the stamped instance of the span kernel and the earlier generations
	else if (seg_stride != 1 && variant != 58) // the earlier generations read SoA arrays only
		return (int)hipErrorInvalidValue;
#define VG_LAUNCH_PK(A, C, P)                                                                            \
	hipLaunchKernelGGL((vgsdf::sdf_tiles_pk<A, C, P>), grid, dim3(vgsdf::TPB / P), 0, stream, tiles,  \
	                   n_tiles, sx, sy, ex, ey, out)
#define VG_LAUNCH_HIER(A, L)                                                                               \
	hipLaunchKernelGGL((vgsdf::sdf_tiles_hier<A, L>), grid, dim3(vgsdf::TPB), 0, stream, tiles, n_tiles,   \
	                   sx, sy, ex, ey, out)
#define VG_LAUNCH_FILTERED(A, C)                                                                          \
	hipLaunchKernelGGL((vgsdf::sdf_tiles_filtered<A, C>), grid, dim3(vgsdf::TPB), 0, stream, \
	                   tiles, n_tiles, sx, sy, ex, ey, out)
	else if (variant == 58) { // diagnostic: s_memtime stamps per phase; prints the shares of wave time on stderr
		unsigned long long h[28] = {0};
		(void)hipMemcpyToSymbolAsync(HIP_SYMBOL(vgsdf::g_span_dbg), h, sizeof(h), 0, hipMemcpyHostToDevice, stream);
		hipLaunchKernelGGL(vgsdf::sdf_tiles_span_stamped, grid, dim3(vgsdf::TPB), 0, stream, tiles, n_tiles, sx, sy, ex,
		                   ey, seg_stride, out, (const float4 *)boxes, (const vgsdf::PlanHeader *)nullptr);
		(void)hipStreamSynchronize(stream);
		(void)hipMemcpyFromSymbol(h, HIP_SYMBOL(vgsdf::g_span_dbg), sizeof(h), 0, hipMemcpyDeviceToHost);
		static const char *names[12] = {"overhead", "wait chunk-top barrier", "stage", "wait post-stage barrier", "wave-level cull",
		                                "-", "phase 1", "phase 2", "decide", "exact evaluation", "quantise+state", "epilogue"};
		unsigned long long tot = 0;
		for (int r = 0; r < 12; r++)
			tot += h[r];
		std::fprintf(stderr, "[vgsdf stamps] %llu waves, %.0f ticks per wave\n", h[12], h[12] ? (double)tot / (double)h[12] : 0.0);
		for (int r = 0; r < 12; r++)
			std::fprintf(stderr, "[vgsdf stamps]   %-26s %6.2f %%\n", names[r], tot ? 100.0 * (double)h[r] / (double)tot : 0.0);
		std::fprintf(stderr, "[vgsdf counts] wave tile-chunks %llu (+ %llu without a surviving group), surviving groups %.1f per wave tile-chunk, pairs %llu (%.1f), rounds %llu (%.2f), waves with undecided lanes %llu (%.3f per wave tile-chunk), undecided lanes %llu\n",
		             h[15], h[19], h[15] + h[19] ? (double)h[18] / (double)(h[15] + h[19]) : 0.0, h[13], h[15] ? (double)h[13] / (double)h[15] : 0.0, h[14],
		             h[15] ? (double)h[14] / (double)h[15] : 0.0, h[16], h[15] ? (double)h[16] / (double)h[15] : 0.0, h[17]);
	}
	else if (variant == 30) // bounded groups on 256-pixel tiles
		VG_LAUNCH_HIER(0, false);
	else if (variant == 45) // ... exact evaluation only where the byte is undecided
		VG_LAUNCH_HIER(0, true);
	else if (variant == 22) // packed filter, grouped selection
		VG_LAUNCH_PK(0, false, 1);
	else if (variant == 23) // ... with per-wave culling
		VG_LAUNCH_PK(0, true, 1);
	else if (variant == 12) // scalar filter, top-4 keys
		VG_LAUNCH_FILTERED(0, false);
	else if (variant == 10) // ... with per-wave culling
		VG_LAUNCH_FILTERED(0, true);
#endif
	else
		return (int)hipErrorInvalidValue;
	return (int)hipGetLastError();
}
