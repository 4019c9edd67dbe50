// outline_plan_kernels.hip — what turns the rects of the flattening passes (outline_kernels.hip) into a schedule and byte
// positions: outline_plan (one workgroup: descriptors, the raster's work list, totals, and with pbf_fix the place of every
// glyph's entry in the arena of finished PBF blocks) and pbf_entries, which writes the entry bytes around the bitmaps with
// pbf_place's arithmetic written out — the two stay side by side.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "outline_plan_kernels.h"
#include "sdf_kernels.h"
#include "upload_layout.h"
#include "work_plan.h"

namespace vgsdf {

// ---------------------------------------------------------------------------------------
// plan: ONE workgroup.  From the rects: the glyph descriptors (segment and output offsets: exclusive sums),
// the raster's work list and the totals the host reads back together with the rects.  The list follows the
// policy the host's planner of resident batches follows too (work_plan.h): class (main kernel / brute
// force), span length T per glyph, heaviest workgroup first (counting sort over 512 logarithmic weight
// buckets; the order inside a bucket is whatever the atomics give: it only shapes the schedule).
// ---------------------------------------------------------------------------------------
constexpr int kPlanThreads = 1024;
constexpr int kPlanBuckets = 512;

// block-wide exclusive sum of one value per thread (1024 threads = 16 waves); returns the exclusive prefix, sets total
__device__ __forceinline__ unsigned long long block_exclusive_sum(unsigned long long v, unsigned long long *s_wave /*[17]*/,
                                                                  unsigned long long &total)
{
	const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	unsigned long long incl = v;
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long o = __shfl_up(incl, d);
		if ((int)lane >= d)
			incl += o;
	}
	__syncthreads(); // s_wave free again
	if (lane == 63)
		s_wave[wv] = incl;
	__syncthreads();
	if (wv == 0) { // the 16 wave totals: one shuffle scan in the first wave
		constexpr int kWaves = kPlanThreads / 64;
		const unsigned long long t = lane < (uint32_t)kWaves ? s_wave[lane] : 0ull;
		unsigned long long in = t;
		for (int d = 1; d < kWaves; d <<= 1) {
			const unsigned long long o = __shfl_up(in, d);
			if ((int)lane >= d)
				in += o;
		}
		if (lane < (uint32_t)kWaves)
			s_wave[lane] = in - t;
		if (lane == (uint32_t)kWaves - 1)
			s_wave[kWaves] = in;
	}
	__syncthreads();
	total = s_wave[kPlanThreads / 64];
	return s_wave[wv] + incl - v;
}

// bytes of a protobuf varint
__device__ __forceinline__ uint32_t varint_len(unsigned long long v)
{
	const uint32_t bits = 64u - (uint32_t)__builtin_clzll(v | 1ull); // 1 .. 64 significant bits, 7 per byte
	return (bits + 6u) / 7u;
}

// In-place PBF assembly (vgsdf.h, vgsdf_outlines_packed::pbf_pre / pbf_fix): what glyph `r` occupies in the arena of
// finished PBF blocks — `pre` reserved bytes in front of it (the block's file and fontstack header when it is the first
// glyph of its block), then its `glyphs` entry of the fontstack message (src/protobuf/glyph.rs:10-41, fontstack.rs:9-25):
//   0x1A varint(msg) | 0x08 varint(id) | [0x12 varint(w h) bitmap] | 0x18 width 0x20 height 0x28 left 0x30 top 0x38 advance
// with width = w - 6, height = h - 6, left = x0 + 3, top = y0 + h - 27 (src/render/result.rs:66-76 after renderer.rs:146).
// fix = (1 + varint_len(id)) | (1 + varint_len(advance)) << 4, from the host (it knows id and advance).
// Returns the bytes taken, sets `bitmap_at` to the bitmap's offset in them.  The host writes the headers with the same
// arithmetic (csrc/host/pbf.hpp, pbf_entry_layout) once the rects are back.
__device__ __forceinline__ unsigned long long pbf_place(const OutlineRect &r, uint32_t pre, uint32_t fix, unsigned long long &bitmap_at)
{
	const uint32_t idlen = fix & 15u, advlen = fix >> 4;
	unsigned long long msg = idlen + advlen;
	const unsigned long long px = r.has_raster ? (unsigned long long)r.w * r.h : 0ull;
	uint32_t bm_hdr = 0;
	if (r.has_raster) {
		bm_hdr = 1u + varint_len(px);
		msg += bm_hdr + px;
		const uint32_t left = (uint32_t)r.x0 + 3u, top = (uint32_t)r.y0 + r.h - 27u; // two's complement, as i32 arithmetic wraps
		const uint32_t zl = (left << 1) ^ (uint32_t)((int32_t)left >> 31), zt = (top << 1) ^ (uint32_t)((int32_t)top >> 31);
		msg += 4u + varint_len(r.w - 6u) + varint_len(r.h - 6u) + varint_len(zl) + varint_len(zt);
	} else {
		msg += 8u; // PbfGlyph::empty: width, height, left, top = 0 (glyph.rs:60-70), one byte each behind its tag
	}
	const uint32_t ent_hdr = 1u + varint_len(msg);
	bitmap_at = (unsigned long long)pre + ent_hdr + idlen + bm_hdr;
	return (unsigned long long)pre + ent_hdr + msg;
}

// KEEP: glyphs per thread whose rects (and classification) stay in registers for all three passes; PBF: in-place placement
// is part of the unrolled passes (instances: <8, false> for packed bitmaps, <4, true> for in-place batches of <= 4096 glyphs;
// eight inlined placements spill the 1024-thread workgroup to scratch: 21 -> 26 us)
template <uint32_t KEEP, bool PBF>
__global__ __launch_bounds__(kPlanThreads) void outline_plan(const OutlineRect *__restrict__ rects, uint32_t n_glyphs, int span_list,
                                                             uint32_t delta_cap, uint32_t span_max, uint32_t span_budget,
                                                             uint32_t tile_cap, GlyphDesc *__restrict__ descs,
                                                             SpanRec *__restrict__ tiles, PlanHeader *__restrict__ hdr,
                                                             const uint32_t *__restrict__ error_flag, unsigned long long seg_cap,
                                                             unsigned long long out_cap, uint32_t launch_spans,
                                                             const uint32_t *__restrict__ pbf_pre, const uint8_t *__restrict__ pbf_fix,
                                                             unsigned long long *__restrict__ pbf_at, uint32_t *__restrict__ next_flag)
{
	__shared__ unsigned long long s_wave[kPlanThreads / 64 + 1];
	// the error word of the NEXT submission of this context (the two alternate): zeroed here, behind everything that could
	// still raise the previous use of that word, instead of a memset launch in front of every submission
	if (threadIdx.x == 0 && next_flag != nullptr)
		next_flag[0] = 0;
	__shared__ uint32_t s_hist[2][kPlanBuckets]; // spans per (class, bucket); then the bucket's write cursor
	__shared__ unsigned long long s_carry[2];
	const uint32_t tid = threadIdx.x;
	for (uint32_t i = tid; i < 2 * kPlanBuckets; i += kPlanThreads)
		(&s_hist[0][0])[i] = 0;
	if (tid == 0)
		s_carry[0] = s_carry[1] = 0;
	__syncthreads();
	// class (0 main / 1 brute), span length, span count and weight of a glyph (work_plan.h: the policy shared with the host)
	auto classify = [&](const OutlineRect &r, uint32_t &cls, uint32_t &T, uint32_t &nspans, uint32_t &weight) {
		const unsigned long long px = r.has_raster ? (unsigned long long)r.w * r.h : 0ull;
		cls = 0, T = 1, nspans = 0, weight = 0;
		if (px == 0 || px > 0xFFFFFFFFull - 256ull) // (a bitmap beyond 2^32 pixels is an error of the batch: no entries)
			return;
		const GlyphPlan gp = plan_glyph(px, r.w, r.n_segments, span_list != 0, delta_cap, span_max, span_budget);
		cls = gp.cls, T = gp.T, nspans = gp.n_spans, weight = gp.weight;
	};
	// pass A: descriptors (exclusive sums of segments and output bytes), span histogram.  Every thread takes a
	// contiguous run of glyphs: one block-wide scan of the runs' sums, then a running sum inside the run.
	bool bad = false;
	const uint32_t per = (n_glyphs + kPlanThreads - 1) / kPlanThreads;
	const uint32_t g_lo = min(tid * per, n_glyphs), g_hi = min(g_lo + per, n_glyphs);
	// a run of up to eight glyphs (batches of <= 8192 glyphs: every group the dispatcher forms) stays in registers with its classification, so
	// the rects are read once and classified once for both passes
	constexpr uint32_t kKeep = KEEP;
	const bool kept = per <= kKeep && (PBF || pbf_fix == nullptr);
	OutlineRect kr[kKeep];
	uint32_t kcls[kKeep], kT[kKeep], kn[kKeep], kw[kKeep];
#pragma unroll
	for (uint32_t j = 0; j < kKeep; j++) {
		kr[j].x0 = kr[j].y0 = 0;
		kr[j].w = kr[j].h = kr[j].n_segments = kr[j].has_raster = 0;
		kcls[j] = kT[j] = kn[j] = kw[j] = 0;
		if (kept && g_lo + j < g_hi) {
			kr[j] = rects[g_lo + j];
			classify(kr[j], kcls[j], kT[j], kn[j], kw[j]);
		}
	}
	{
		unsigned long long my_s = 0, my_p = 0;
		// output bytes of a glyph: its bitmap, or — in-place PBF assembly — everything it occupies in the arena
		auto sum_one = [&](uint32_t g, const OutlineRect &r) {
			if (r.has_raster) {
				my_s += r.n_segments;
				bad |= (unsigned long long)r.w * r.h > 0xFFFFFFFFull - 256ull;
			}
			if (pbf_fix != nullptr) {
				unsigned long long at;
				my_p += pbf_place(r, pbf_pre[g], pbf_fix[g], at);
			} else if (r.has_raster) {
				my_p += (unsigned long long)r.w * r.h;
			}
		};
		if (kept) {
#pragma unroll
			for (uint32_t j = 0; j < kKeep; j++) {
				if (kr[j].has_raster) { // (absent glyphs: zero rects)
					my_s += kr[j].n_segments;
					if (!(PBF && pbf_fix != nullptr))
						my_p += (unsigned long long)kr[j].w * kr[j].h;
					bad |= (unsigned long long)kr[j].w * kr[j].h > 0xFFFFFFFFull - 256ull;
				}
				if (PBF && pbf_fix != nullptr && g_lo + j < g_hi) {
					unsigned long long at;
					my_p += pbf_place(kr[j], pbf_pre[g_lo + j], pbf_fix[g_lo + j], at);
				}
			}
		} else {
			for (uint32_t g = g_lo; g < g_hi; g++)
				sum_one(g, rects[g]);
		}
		unsigned long long tot_s, tot_p;
		unsigned long long so = block_exclusive_sum(my_s, s_wave, tot_s);
		unsigned long long po = block_exclusive_sum(my_p, s_wave, tot_p);
		if (tid == 0) {
			s_carry[0] = tot_s;
			s_carry[1] = tot_p;
		}
		auto desc_one = [&](uint32_t g, const OutlineRect &r, uint32_t cls, uint32_t nspans, uint32_t weight, auto in_place) {
			const unsigned long long px = r.has_raster ? (unsigned long long)r.w * r.h : 0ull;
			const unsigned long long segs = r.has_raster ? r.n_segments : 0u;
			GlyphDesc d;
			d.seg_off = (uint32_t)so; // (the host rejects batches with more than 2^32 - 1 segments: header)
			d.n_seg = (uint32_t)segs;
			d.x0 = r.x0;
			d.y0 = r.y0;
			d.w = r.has_raster ? r.w : 0;
			d.h = r.has_raster ? r.h : 0;
			if (decltype(in_place)::value && pbf_fix != nullptr) {
				unsigned long long at;
				const unsigned long long took = pbf_place(r, pbf_pre[g], pbf_fix[g], at);
				d.out_off = po + at; // the raster stores the bitmap where the finished file has it
				pbf_at[g] = po + at; // (read back with the rects: the host writes the bytes around it)
				po += took;
			} else {
				d.out_off = po;
				po += px;
			}
			descs[g] = d;
			so += segs;
			if (nspans)
				atomicAdd(&s_hist[cls][weight_bucket(weight)], nspans);
		};
		if (kept) {
#pragma unroll
			for (uint32_t j = 0; j < kKeep; j++)
				if (g_lo + j < g_hi)
					desc_one(g_lo + j, kr[j], kcls[j], kn[j], kw[j], std::integral_constant<bool, PBF>{});
		} else {
			for (uint32_t g = g_lo; g < g_hi; g++) {
				const OutlineRect r = rects[g];
				uint32_t cls, T, nspans, weight;
				classify(r, cls, T, nspans, weight);
				desc_one(g, r, cls, nspans, weight, std::true_type{});
			}
		}
	}
	__syncthreads();
	// bucket bases: main class first (heaviest bucket first), then the brute-force class — one (class, bucket)
	// cell per thread
	__shared__ uint32_t s_nmain, s_nall;
	static_assert(2 * kPlanBuckets == kPlanThreads, "one histogram cell per thread");
	{
		const unsigned long long mine = (&s_hist[0][0])[tid];
		unsigned long long acc;
		const unsigned long long base_at = block_exclusive_sum(mine, s_wave, acc);
		(&s_hist[0][0])[tid] = (uint32_t)(base_at > 0xFFFFFFFFull ? 0xFFFFFFFFull : base_at);
		if (tid == kPlanBuckets) // first cell of the brute-force class: everything before it is main class
			s_nmain = (uint32_t)(base_at > 0x7FFFFFFFull ? 0x7FFFFFFFull : base_at);
		if (tid == 0)
			s_nall = (uint32_t)(acc > 0x7FFFFFFFull ? 0x80000000ull : acc);
	}
	__syncthreads();
	if (tid == 0) {
		const unsigned long long acc = s_nall;
		hdr->n_segments = s_carry[0];
		hdr->out_bytes = s_carry[1];
		hdr->n_spans = s_nall;
		hdr->n_main = s_nmain;
		hdr->error = error_flag[0] | (((s_carry[0] > 0xFFFFFFFFull) || (acc > 0x7FFFFFFFull)) ? 1u : 0u); // bit 0: sizes, bit 1: unknown command kind
		hdr->ok = 0;
	}
	__syncthreads();
	const bool any_bad = __syncthreads_or(bad);
	if (tid == 0 && any_bad)
		hdr->error |= 1u;
	// no work list for a batch in error (its sizes may be absurd), nor when the list does not fit: the host
	// grows it and runs the plan again
	if (any_bad || error_flag[0] != 0 || s_carry[0] > 0xFFFFFFFFull || s_nall > tile_cap || s_nall > 0x7FFFFFFFu)
		return;
	// (every glyph's entries are in place when the kernel ends: a launch enqueued behind it may read the list)
	if (tid == 0)
		hdr->ok = s_carry[0] <= seg_cap && s_carry[1] <= out_cap && s_nall == s_nmain && s_nmain <= launch_spans;
	// pass B: entries.  One per span of T tiles: the glyph's descriptor as pass A stored it (by this thread for a kept
	// glyph, else by another one in front of the barriers above), the glyph, and first pixel | T in the span list's main
	// class, else the first pixel.
	auto entries = [&](uint32_t g, const OutlineRect &r, uint32_t cls, uint32_t T, uint32_t nspans, uint32_t weight) {
		if (!nspans)
			return;
		uint32_t at = atomicAdd(&s_hist[cls][weight_bucket(weight)], nspans);
		const unsigned long long px = (unsigned long long)r.w * r.h;
		const GlyphDesc d = descs[g];
		for (unsigned long long p = 0; p < px; p += 256ull * T) {
			const uint32_t left = (uint32_t)((px - p + 255ull) >> 8);
			tiles[at++] = span_rec(d, g, span_list && cls == 0 ? ((uint32_t)p | min(T, left)) : (uint32_t)p);
		}
	};
	if (kept) {
#pragma unroll
		for (uint32_t j = 0; j < kKeep; j++)
			if (g_lo + j < g_hi)
				entries(g_lo + j, kr[j], kcls[j], kT[j], kn[j], kw[j]);
	} else {
		for (uint32_t g = tid; g < n_glyphs; g += kPlanThreads) {
			const OutlineRect r = rects[g];
			uint32_t cls, T, nspans, weight;
			classify(r, cls, T, nspans, weight);
			entries(g, r, cls, T, nspans, weight);
		}
	}
}

// In-place PBF assembly of a ranges submission: the bytes of every glyph's entry AROUND its bitmap, written on the device —
// what the host's write_pbf_entry_headers (csrc/host/pbf.cpp) writes for the other forms once the rects are back.  A lane per
// glyph, behind the plan: from the rect, the bitmap's position pbf_at[g] and the entry's id and advance (left by the upload
// kernel) it stores
//   0x1A varint(msg) 0x08 varint(id) [0x12 varint(w h)]                      ending at pbf_at[g]
//   0x18 width 0x20 height 0x28 zigzag(left) 0x30 zigzag(top) 0x38 advance   behind the bitmap (PbfGlyph::empty without a raster)
// with pbf_place's arithmetic, into `out`: wherever the submission's raster stores its bitmaps, under the same PlanHeader::ok
// guard (need_ok = 0: the launch the host repeats after a guess that did not hold).  No byte of a bitmap or of a task's
// reserved room is touched; plain byte stores.  It also notes where every task's reserved room begins (begin[task], and the
// arena's size behind the last): positions, valid whether or not the entries could be stored.
__device__ __forceinline__ uint8_t *put_varint(uint8_t *p, unsigned long long v)
{
	for (; v >= 0x80ull; v >>= 7)
		*p++ = (uint8_t)(v | 0x80ull);
	*p++ = (uint8_t)v;
	return p;
}
__global__ __launch_bounds__(256) void pbf_entries(const OutlineRect *__restrict__ rects, const unsigned long long *__restrict__ pbf_at,
                                                   const uint32_t *__restrict__ pbf_pre, const EntryName *__restrict__ names,
                                                   uint32_t n_glyphs, uint32_t n_tasks, const PlanHeader *__restrict__ hdr, uint32_t need_ok,
                                                   unsigned long long out_cap, uint8_t *__restrict__ out,
                                                   unsigned long long *__restrict__ begin)
{
	const uint32_t g = blockIdx.x * 256u + threadIdx.x;
	if (g >= n_glyphs || hdr->error != 0) // (the positions of a batch in error say nothing)
		return;
	const OutlineRect r = rects[g];
	const EntryName nm = names[g];
	const unsigned long long at = pbf_at[g];
	const uint32_t idlen = 1u + varint_len(nm.id), advlen = 1u + varint_len(nm.advance);
	const unsigned long long px = r.has_raster ? (unsigned long long)r.w * r.h : 0ull;
	uint32_t width = 0, height = 0, zl = 0, zt = 0, bm_hdr = 0;
	if (r.has_raster) {
		const uint32_t left = (uint32_t)r.x0 + 3u, top = (uint32_t)r.y0 + r.h - 27u; // two's complement, as i32 arithmetic wraps
		width = r.w - 6u, height = r.h - 6u;
		zl = (left << 1) ^ (uint32_t)((int32_t)left >> 31), zt = (top << 1) ^ (uint32_t)((int32_t)top >> 31);
		bm_hdr = 1u + varint_len(px);
	}
	const uint32_t back = 4u + varint_len(width) + varint_len(height) + varint_len(zl) + varint_len(zt) + advlen;
	const unsigned long long msg = (unsigned long long)idlen + bm_hdr + px + back;
	const uint32_t front = 1u + varint_len(msg) + idlen + bm_hdr;
	if (nm.task_first != 0 && nm.task_first <= n_tasks)
		begin[nm.task_first - 1u] = at - front - pbf_pre[g];
	if (g == n_glyphs - 1u)
		begin[n_tasks] = hdr->out_bytes;
	if (out == nullptr || (need_ok && hdr->ok == 0) || at < front || at + px + back > out_cap)
		return;
	uint8_t *p = out + (at - front);
	*p++ = 0x1A;
	p = put_varint(p, msg);
	*p++ = 0x08;
	p = put_varint(p, nm.id);
	if (r.has_raster) {
		*p++ = 0x12;
		p = put_varint(p, px);
	}
	p = out + at + px; // (behind the bitmap, which the raster stores)
	*p++ = 0x18;
	p = put_varint(p, width);
	*p++ = 0x20;
	p = put_varint(p, height);
	*p++ = 0x28;
	p = put_varint(p, zl);
	*p++ = 0x30;
	p = put_varint(p, zt);
	*p++ = 0x38;
	p = put_varint(p, nm.advance);
}

} // namespace vgsdf

using namespace vgsdf;

extern "C" int vgsdf_outline_plan(const OutlineRect *rects, uint32_t n_glyphs, int span_list, uint32_t delta_cap, uint32_t span_max,
                                  uint32_t span_budget, uint32_t tile_cap, GlyphDesc *descs, SpanRec *tiles, PlanHeader *hdr,
                                  const uint32_t *error_flag, unsigned long long seg_cap, unsigned long long out_cap,
                                  uint32_t launch_spans, const uint32_t *pbf_pre, const uint8_t *pbf_fix,
                                  unsigned long long *pbf_at, uint32_t *next_flag, hipStream_t stream)
{
	if (pbf_fix != nullptr && n_glyphs <= 4u * kPlanThreads)
		hipLaunchKernelGGL((outline_plan<4, true>), dim3(1), dim3(kPlanThreads), 0, stream, rects, n_glyphs, span_list, delta_cap, span_max,
		                   span_budget, tile_cap, descs, tiles, hdr, error_flag, seg_cap, out_cap, launch_spans, pbf_pre, pbf_fix, pbf_at, next_flag);
	else if (pbf_fix != nullptr && n_glyphs <= 8u * kPlanThreads)
		// groups of 4097 .. 8192 glyphs (the dispatcher's groups of several fonts: ~7000): eight placements per thread spill
		// to scratch, and still beat the unkept path below, which reads and classifies every rect twice (21 fonts in two
		// groups: 48 / 90 us per plan)
		hipLaunchKernelGGL((outline_plan<8, true>), dim3(1), dim3(kPlanThreads), 0, stream, rects, n_glyphs, span_list, delta_cap, span_max,
		                   span_budget, tile_cap, descs, tiles, hdr, error_flag, seg_cap, out_cap, launch_spans, pbf_pre, pbf_fix, pbf_at, next_flag);
	else
	hipLaunchKernelGGL((outline_plan<8, false>), dim3(1), dim3(kPlanThreads), 0, stream, rects, n_glyphs, span_list, delta_cap, span_max,
	                   span_budget, tile_cap, descs, tiles, hdr, error_flag, seg_cap, out_cap, launch_spans, pbf_pre, pbf_fix, pbf_at, next_flag);
	return (int)hipGetLastError();
}

extern "C" int vgsdf_pbf_entries(const OutlineRect *rects, const unsigned long long *pbf_at, const uint32_t *pbf_pre, const void *names,
                                 uint32_t n_glyphs, uint32_t n_tasks, const PlanHeader *hdr, bool need_ok, unsigned long long out_cap,
                                 uint8_t *out, unsigned long long *begin, hipStream_t stream)
{
	if (n_glyphs == 0)
		return 0;
	hipLaunchKernelGGL(pbf_entries, dim3((n_glyphs + 255u) / 256u), dim3(256), 0, stream, rects, pbf_at, pbf_pre, (const EntryName *)names,
	                   n_glyphs, n_tasks, hdr, need_ok ? 1u : 0u, out_cap, out, begin);
	return (int)hipGetLastError();
}
