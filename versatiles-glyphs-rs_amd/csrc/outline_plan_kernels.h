// outline_plan_kernels.h — launchers of outline_plan_kernels.hip: the plan behind the flattening passes' rects and the PBF
// entry bytes behind the plan.
#pragma once
#include "outline_kernels.h"
#include "sdf_kernels.h" // SpanRec: the entries of the work list the plan writes

extern "C" {
// seg_cap / out_cap / launch_spans: what PlanHeader::ok is decided against (capacity of the segment records, of the
// output buffer, grid of the raster launch enqueued behind the plan; launch_spans = 0: no such launch)
int vgsdf_outline_plan(const vgsdf::OutlineRect *rects, uint32_t n_glyphs, int span_list, uint32_t delta_cap, uint32_t span_max,
                       uint32_t span_budget, uint32_t tile_cap, vgsdf::GlyphDesc *descs, vgsdf::SpanRec *tiles, vgsdf::PlanHeader *hdr,
                       const uint32_t *error_flag, unsigned long long seg_cap, unsigned long long out_cap, uint32_t launch_spans,
                       const uint32_t *pbf_pre /* NULL: bitmaps packed back to back */, const uint8_t *pbf_fix,
                       unsigned long long *pbf_at /* [n_glyphs] positions of the bitmaps in the arena */,
                       uint32_t *next_flag /* may be NULL: a word the kernel zeroes (the next submission's error word) */, hipStream_t stream);
// behind the plan of a ranges submission with pbf_pre: the entry bytes around every bitmap into `out` (out_cap bytes; NULL: none;
// need_ok: only under PlanHeader::ok, as the raster enqueued behind the plan), and begin[n_tasks + 1]: where every task's
// reserved room starts, and the arena's size
int vgsdf_pbf_entries(const vgsdf::OutlineRect *rects, const unsigned long long *pbf_at, const uint32_t *pbf_pre, const void *names,
                      uint32_t n_glyphs, uint32_t n_tasks, const vgsdf::PlanHeader *hdr, bool need_ok, unsigned long long out_cap,
                      uint8_t *out, unsigned long long *begin, hipStream_t stream);
}
