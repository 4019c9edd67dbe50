// work_plan.h — the policy of the raster's work list, for both of its planners: the host's (work_list.cpp, resident
// batches of the C ABI) and the device's (outline_plan_kernels.hip, outline_plan).  Which glyphs go to brute force, the span
// length T, the spans per glyph, a workgroup's weight and the weight's bucket are decided here and nowhere else
// (tests/test_gpu_span_regimes.py restates the policy on purpose, as the independent check).
#pragma once
#include <stdint.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#define VGSDF_HD __host__ __device__ __forceinline__
#else
#define VGSDF_HD inline
#endif

namespace vgsdf {

// A workgroup that sweeps T consecutive tiles of 256 pixels touches (256 T - 2) / w + 2 rows; times the row stride (the
// kernel pads a row of w + 1 cells to an odd stride: at most w + 2) they must fit the winding histogram in LDS.  This is a
// safety condition of the span kernel, not a tuning choice.  (32-bit division: this runs per glyph on the end-to-end path)
VGSDF_HD bool span_fits(uint32_t w, uint32_t T, uint32_t delta_cap)
{
	return (unsigned long long)((256u * T - 2u) / w + 2u) * ((unsigned long long)w + 2u) <= delta_cap;
}

// tiles x chunks a workgroup of the span kernel sweeps at most.  16 is the best value for a batch that fills the chip
// several times over (Noto Sans Regular: 3023 workgroups on 1024 slots; 8 costs it 7 %: chunks are staged more often);
// a small batch is bounded by its longest workgroups instead, and halving them helps (Fira Sans, 1679 glyphs: 58.4 -> 52.2 us).
VGSDF_HD uint32_t default_span_budget(uint32_t n_glyphs) { return n_glyphs < 2048u ? 8u : 16u; }

struct GlyphPlan {
	uint32_t cls;     // 0: main kernel; 1: brute force (the histogram would not fit in LDS, or the segment index needs more than 24 bits)
	uint32_t T;       // tiles a workgroup sweeps per staged chunk, one after the other
	uint32_t n_spans; // entries of the glyph in the work list: one per T tiles
	uint32_t weight;  // segments x tiles swept per staged chunk (saturated): heaviest first inside a class
};

// The plan of one glyph of px = w * h pixels (0 < px <= 2^32 - 1 - 256) and n_seg segments.  T is the largest count
// <= span_max whose rows fit the histogram, with tiles x chunks bounded by span_budget so that the glyphs with long
// segment lists stay spread over many workgroups (they set the makespan of a small batch) while short ones are staged
// once; 1 outside the span list's main class.
VGSDF_HD GlyphPlan plan_glyph(unsigned long long px, uint32_t w, uint32_t n_seg, bool span_list, uint32_t delta_cap, uint32_t span_max,
                              uint32_t span_budget)
{
	GlyphPlan p;
	p.cls = 0;
	p.T = 1;
	if (!span_fits(w, 1, delta_cap) || n_seg >= (1u << 24)) {
		p.cls = 1;
	} else if (span_list) {
		const uint32_t chunks = (n_seg + 255u) / 256u;
		const uint32_t per_chunk = span_budget / (chunks > 1u ? chunks : 1u);
		const uint32_t budget_t = per_chunk > 1u ? per_chunk : 1u;
		const uint32_t t_hi = span_max < budget_t ? span_max : budget_t;
		for (p.T = t_hi; p.T > 1; p.T--)
			if (span_fits(w, p.T, delta_cap))
				break;
	}
	const unsigned long long t256 = (px + 255ull) >> 8;
	p.n_spans = (uint32_t)((t256 + p.T - 1) / p.T);
	const unsigned long long wgt = (unsigned long long)n_seg * (t256 < p.T ? t256 : p.T);
	p.weight = wgt > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)wgt;
	return p;
}

// The order inside a class is heaviest first to 1/16 of the weight (the exact order does not matter): 512 logarithmic
// buckets for a counting sort; bucket 0 = heaviest
VGSDF_HD uint32_t weight_bucket(uint32_t weight)
{
	if (weight < 16u)
		return 511u - weight;
	const uint32_t e = 31u - (uint32_t)__builtin_clz(weight);      // 4..31
	return 511u - ((e - 3u) * 16u + ((weight >> (e - 4u)) & 15u)); // 16..463 -> descending
}

// (host) the switches of the policy, read on every call: VGSDF_SPAN_MAX (1..4 tiles per span), VGSDF_SPAN_BUDGET (measured:
// 12-24 equally good for a large batch)
inline void span_policy_from_env(uint32_t n_glyphs, uint32_t &span_max, uint32_t &span_budget)
{
	const char *sm = getenv("VGSDF_SPAN_MAX");
	const int m = sm ? atoi(sm) : 4;
	span_max = (uint32_t)(m < 1 ? 1 : (m > 4 ? 4 : m));
	const char *sb = getenv("VGSDF_SPAN_BUDGET");
	const int b = sb ? atoi(sb) : 0;
	span_budget = sb ? (uint32_t)(b < 1 ? 1 : b) : default_span_budget(n_glyphs);
}

} // namespace vgsdf
