// work_list.cpp — the host's planner of a resident batch's work list (the segment entry points of the C ABI; the outline
// front-end plans on the device: outline_plan_kernels.hip, outline_plan).  The policy itself is work_plan.h's.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "device_internal.h"
#include "work_plan.h"

void build_descs_and_tiles(const vgsdf_batch *in, vgsdf::GlyphDesc *hd, vgsdf::SpanRec *ht, vgsdf_dbatch *b, bool span)
{
	static_assert(VGSDF_TILE_PIXELS == 256, "work_plan.h counts in tiles of 256 pixels");
	const uint32_t n = in->n_glyphs;
	const uint32_t delta_cap = (uint32_t)vgsdf_filtered_delta_cap();
	uint32_t span_max, span_budget;
	vgsdf::span_policy_from_env(n, span_max, span_budget);
	b->span_list = span;
	// the descriptors first: every entry of the work list carries a copy of its glyph's
	for (uint32_t g = 0; g < n; g++) {
		hd[g].seg_off = in->seg_off[g];
		hd[g].n_seg = in->seg_off[g + 1] - in->seg_off[g];
		hd[g].x0 = in->x0[g];
		hd[g].y0 = in->y0[g];
		hd[g].w = in->w[g];
		hd[g].h = in->h[g];
		hd[g].out_off = in->out_off[g];
	}
	const char *ord = std::getenv("VGSDF_TILE_ORDER");
	b->tile_order = ord ? std::atoi(ord) : 1;

	// One pass per glyph: its plan (class, span length T, spans, weight).  Inside the main class the heaviest workgroups
	// come first (the dispatcher hands workgroups out in list order, so the long ones start early and the tail is made of
	// short ones); the brute-force class and VGSDF_TILE_ORDER=0 keep glyph order (+ per-XCD contiguous remap in-kernel).
	// (thread_local scratch, addressed through plain references below: in a PIC shared object every
	// use of a thread_local name is a __tls_get_addr call)
	static thread_local std::vector<uint8_t> tl_span_t;
	static thread_local std::vector<uint64_t> tl_keys[2], tl_tmp; // (~weight << 32) | glyph: ascending = heaviest first
	static thread_local std::vector<uint2> tl_queue[8];
	std::vector<uint8_t> &span_t = tl_span_t;
	std::vector<uint64_t> *const keys = tl_keys, &tmp = tl_tmp;
	std::vector<uint2> *const queue = tl_queue;
	span_t.resize(n);
	uint64_t n_cls_spans[2] = {0, 0};
	for (int c = 0; c < 2; c++)
		keys[c].clear();
	for (uint32_t g = 0; g < n; g++) {
		const uint64_t px = (uint64_t)in->w[g] * in->h[g]; // <= 2^32 - 1 - 256 (validated by the callers)
		if (px == 0)
			continue;
		const vgsdf::GlyphPlan gp = vgsdf::plan_glyph(px, in->w[g], in->seg_off[g + 1] - in->seg_off[g], span, delta_cap, span_max, span_budget);
		span_t[g] = (uint8_t)gp.T;
		n_cls_spans[gp.cls] += gp.n_spans;
		keys[gp.cls].push_back(((uint64_t)(0xFFFFFFFFu - gp.weight) << 32) | g);
	}
	static const bool trace_l = std::getenv("VGSDF_TRACE") != nullptr;
	const double tl0 = trace_l ? fe_now() : 0;
	double tl_sort = 0, tl_deal = 0;
	uint64_t ti = 0;
	for (int cls = 0; cls < 2; cls++) {
		std::vector<uint64_t> &gl = keys[cls];
		const bool ordered = b->tile_order != 0 && cls == 0;
		const double ts0 = trace_l ? fe_now() : 0;
		if (ordered && gl.size() > 1) {
			// one counting pass over the weight buckets instead of a comparison sort (75 us for a 3000-glyph font)
			tmp.resize(gl.size());
			uint32_t hist[513] = {0};
			auto bucket = [](uint64_t key) { return vgsdf::weight_bucket(0xFFFFFFFFu - (uint32_t)(key >> 32)); };
			for (uint64_t k : gl)
				hist[bucket(k) + 1]++;
			for (int i = 0; i < 512; i++)
				hist[i + 1] += hist[i];
			for (uint64_t k : gl) // stable: glyph order inside a bucket
				tmp[hist[bucket(k)]++] = k;
			gl.swap(tmp);
		}
		const double ts1 = trace_l ? fe_now() : 0;
		tl_sort += ts1 - ts0;
		// entries of glyph g: one per span of T tiles (T = 1 unless this is the span list's main class), as (glyph, first pixel | T);
		// the list takes them as SpanRec, with the glyph's descriptor
		auto emit = [&](uint32_t g, auto &&push) {
			const uint64_t px = (uint64_t)in->w[g] * in->h[g];
			const uint32_t T = span_t[g];
			for (uint64_t p = 0; p < px; p += (uint64_t)VGSDF_TILE_PIXELS * T) { // 64-bit: p + 1024 may pass 2^32
				const uint32_t left = (uint32_t)((px - p + VGSDF_TILE_PIXELS - 1) >> 8);
				push(make_uint2(g, span && cls == 0 ? ((uint32_t)p | (T < left ? T : left)) : (uint32_t)p));
			}
		};
		if (ordered && n_cls_spans[cls] >= 64) {
			// Workgroups are dealt round-robin over the 8 XCDs (position p runs on XCD p % 8, each
			// with its own L2).  Keep all tiles of a glyph on ONE XCD so its segment list is fetched
			// into one L2 only: glyphs are dealt to the currently shortest of 8 per-XCD queues, and
			// the queues are interleaved position by position.
			size_t qlen[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			uint2 *qbuf[8];
			for (int q = 0; q < 8; q++) {
				if (queue[q].size() < n_cls_spans[cls])
					queue[q].resize(n_cls_spans[cls]); // plain arrays below: no capacity checks per entry
				qbuf[q] = queue[q].data();
			}
			for (uint64_t k : gl) {
				size_t best = 0;
				for (size_t m = 1; m < 8; m++)
					if (qlen[m] < qlen[best])
						best = m;
				uint2 *dst = qbuf[best];
				size_t len = qlen[best];
				emit((uint32_t)k, [&](uint2 e) { dst[len++] = e; });
				qlen[best] = len;
			}
			size_t taken[8] = {0, 0, 0, 0, 0, 0, 0, 0};
			const uint64_t last = ti + n_cls_spans[cls];
			while (ti < last)
				for (size_t k = 0; k < 8 && ti < last; k++) {
					size_t src = k; // position ti runs on XCD ti % 8 == k as long as no queue ran dry
					if (taken[src] >= qlen[src])
						for (size_t m = 0; m < 8; m++) // dry: borrow from the fullest queue
							if (qlen[m] - taken[m] > qlen[src] - taken[src])
								src = m;
					const uint2 e = qbuf[src][taken[src]++];
					ht[ti++] = vgsdf::span_rec(hd[e.x], e.x, e.y);
				}
		} else {
			for (uint64_t k : gl)
				emit((uint32_t)k, [&](uint2 e) { ht[ti++] = vgsdf::span_rec(hd[e.x], e.x, e.y); });
		}
		if (cls == 0)
			b->n_main = (uint32_t)ti;
		tl_deal += (trace_l ? fe_now() : 0) - ts1;
	}
	b->stats.n_tiles = ti; // workgroups actually launched (<= the 256-pixel tile count the list was sized for)
	if (trace_l)
		std::fprintf(stderr, "[vgsdf] list: sort %.3f ms, deal+emit %.3f ms (total after pass 1: %.3f)\n", tl_sort * 1e3, tl_deal * 1e3,
		             (fe_now() - tl0) * 1e3);
}
