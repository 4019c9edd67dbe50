// sdf_kernels.h — device-side data layout shared by the kernels and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VGSDF_TILE_PIXELS 256

namespace vgsdf {

// One glyph's raster job, 32 bytes (the "+32 descriptor" of SURVEY.md §8d).
// (x0,y0,w,h) = RenderResult{x0,y0,width,height}, /root/reference/src/render/result.rs:7-29.
struct GlyphDesc {
	uint32_t seg_off; // first segment in the SoA arrays
	uint32_t n_seg;
	int32_t x0, y0;
	uint32_t w, h;
	uint64_t out_off; // first byte of this glyph's bitmap in the output buffer
};
static_assert(sizeof(GlyphDesc) == 32, "GlyphDesc must stay 32 bytes");

// Index of the box of chunk c (256 segments) of glyph g in the chunk-box table: (seg_off[g] >> 8) + g + c — unique for a
// monotone seg_off, so no offset table is needed; the table has (total segments >> 8) + n_glyphs + 1 entries.
__device__ __forceinline__ uint32_t chunk_box_index(uint32_t seg_off, uint32_t glyph, uint32_t c) { return (seg_off >> 8) + glyph + c; }

// One entry of the raster's work list, written by both planners (work_list.cpp on the host, outline_plan on the device): the
// glyph's descriptor, copied, beside what the entry itself says.  A workgroup of sdf_tiles_span or sdf_tiles_brute reads its
// entry with one group of scalar loads and nothing behind it: the descriptor used to be a second, dependent load through the
// glyph index.  GlyphDesc[] stays for the passes that walk glyphs (chunk boxes, PBF entries, the union pass).
// 40 bytes: the descriptor's 32 are full at their documented ranges (32-bit offsets and rects, a 64-bit output offset), so the
// entry's own two words follow it; the loads of both parts are issued together and waited for once.
struct SpanRec {
	uint32_t seg_off; // = GlyphDesc of `glyph`
	uint32_t n_seg;
	int32_t x0, y0;
	uint32_t w, h;
	uint64_t out_off;
	uint32_t first; // main class of a span list: first pixel | T (T = 1..4 tiles of 256 pixels); else the first pixel
	uint32_t glyph; // index of the glyph (chunk_box_index)
};
static_assert(sizeof(SpanRec) == 40, "SpanRec: a GlyphDesc and two words");

__host__ __device__ __forceinline__ SpanRec span_rec(const GlyphDesc &d, uint32_t glyph, uint32_t first)
{
	SpanRec r;
	r.seg_off = d.seg_off, r.n_seg = d.n_seg;
	r.x0 = d.x0, r.y0 = d.y0, r.w = d.w, r.h = d.h;
	r.out_off = d.out_off;
	r.first = first, r.glyph = glyph;
	return r;
}

} // namespace vgsdf

// largest rows*(w+1) a tile of the filtered kernel may need (winding histogram in LDS)
extern "C" int vgsdf_filtered_delta_cap(void);

// 1 when vgsdf_launch_tiles of this build knows the kernel id (50 = span kernel, 1 = brute force; more
// only with -DVGSDF_DEV_VARIANTS)
extern "C" int vgsdf_kernel_known(int kernel);

// Segment layout: seg_stride 1 = four SoA arrays as the C ABI hands them (vgsdf_batch); 4 = records {sx, sy, ex, ey} of
// 32 bytes with sx / sy / ex / ey pointing at the four fields of record 0 (what the device front-end writes).
// tiles[i] = a SpanRec: the glyph's descriptor, its index, and the first output byte of the tile inside that glyph's bitmap
// list_order != 0: workgroups take tiles in list order; 0: per-XCD contiguous remap
extern "C" int vgsdf_launch_tiles(int variant, int list_order, const vgsdf::SpanRec *tiles, uint32_t n_tiles, const double *sx,
                                  const double *sy, const double *ex, const double *ey, uint32_t seg_stride,
                                  uint8_t *out, const void *boxes, hipStream_t stream);

// the span kernel over a device-planned work list that may still be in the making when the launch is enqueued (see .hip)
extern "C" int vgsdf_launch_span_planned(const vgsdf::SpanRec *tiles, uint32_t grid, const double *sx,
                                         const double *sy, const double *ex, const double *ey, uint32_t seg_stride, uint8_t *out,
                                         const void *boxes, const void *plan, hipStream_t stream);

// chunk boxes of a resident batch (sdf_chunk_boxes): table size, and the preparation launch.  `boxes`
// may be NULL in vgsdf_launch_tiles (no chunk is skipped then); only the span kernel reads it.
extern "C" size_t vgsdf_chunk_box_bytes(uint64_t n_segments, uint32_t n_glyphs);
// guard (may be NULL): a vgsdf::PlanHeader on the device; the pass does nothing when it reports an error or more
// segments than seg_cap (device front-end: the segment arrays are then empty)
extern "C" int vgsdf_launch_chunk_boxes(const vgsdf::GlyphDesc *glyphs, uint32_t n_glyphs, const double *sx, const double *sy,
                                        const double *ex, const double *ey, uint32_t seg_stride, void *boxes,
                                        const void *guard, unsigned long long seg_cap, hipStream_t stream);
