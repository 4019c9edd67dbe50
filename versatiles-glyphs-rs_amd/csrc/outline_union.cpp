// outline_union.cpp — union outlines (rule U) over resident batches: the count pass, the host's running sums,
// the new batch's arena, the emit pass into it, and the work list and chunk boxes over the new segments as vgsdf_batch_upload
// makes them.  vgsdf_outlines_union (outline_front_end.cpp, beside the state it replaces) runs the same function over the
// front-end's batch.
#include <cstring>
#include <new>
#include <vector>

#include "device_internal.h"
#include "outline_union_kernels.h"
#include "resident_build.h"

namespace {

// device memory of one call: piece_count u32[n] | piece_off u32[n + 1] | seg_first u32[n_in] | state u8[n]
struct UnionWork {
	size_t count = 0, off, seg_first, state, bytes;
	UnionWork(size_t n, size_t n_in) : off(4 * n), seg_first(off + 4 * (n + 1)), state(seg_first + 4 * n_in), bytes(state + n) {}
};

} // namespace

int union_resident(vgsdf_ctx *ctx, const char *entry, const vgsdf_dbatch *src, vgsdf_dbatch **out, uint8_t *state_out, bool own_output)
{
	*out = nullptr;
	if (src->stats.n_tiles != 0 && uses_span_list(ctx->variant) != src->span_list) {
		ctx->err = std::string(entry) + ": the batch was uploaded for a different kernel variant (tile list layout)";
		return VGSDF_E_ARG;
	}
	const uint32_t n = (uint32_t)src->stats.n_glyphs;
	const uint64_t n_in = src->stats.n_segments;
	(void)hipSetDevice(ctx->device);
	ctx->union_ms[0] = ctx->union_ms[1] = 0.0f;

	const UnionWork wat(n, (size_t)n_in);
	ScratchBuf work;
	PassEvents ev;
	if (hipError_t e = work.ensure(wat.bytes + 16); e != hipSuccess)
		return font_hip_error(ctx, entry, "hipMalloc", e);
	if (hipError_t e = ev.create(); e != hipSuccess)
		return font_hip_error(ctx, entry, "hipEventCreate", e);
	uint8_t *const dw = (uint8_t *)work.p;
	uint32_t *const d_count = (uint32_t *)(dw + wat.count), *const d_off = (uint32_t *)(dw + wat.off),
	                *const d_first = (uint32_t *)(dw + wat.seg_first);
	uint8_t *const d_state = dw + wat.state;

	// count pass; the descriptors come back with the counts: the new batch keeps their rects and out_off
	std::vector<vgsdf::GlyphDesc> hd(n);
	std::vector<uint32_t> count(n), seg_off((size_t)n + 1, 0);
	std::vector<uint8_t> state(n);
	Calls q(ctx->stream);
	q.record(ev.at[0]);
	q.launch([&] { return vgsdf_outline_union_count(src->d_glyphs, n, src->d_sx, src->d_sy, src->d_ex, src->d_ey, src->seg_stride, d_count, d_state, d_first, q.st); });
	q.record(ev.at[1]);
	if (n) {
		q.read_back(hd.data(), src->d_glyphs, sizeof(vgsdf::GlyphDesc) * (size_t)n);
		q.read_back(count.data(), d_count, 4 * (size_t)n);
		q.read_back(state.data(), d_state, n);
	}
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, entry, "count pass", q.e);
	ev.elapsed(ctx->union_ms, 0);

	// the running sums, bounded by what 32-bit segment offsets address
	uint64_t n_seg = 0, n_tiles = 0, n_pixels = 0, n_pairs = 0;
	std::vector<int32_t> x0(n), y0(n);
	std::vector<uint32_t> w(n), h(n);
	std::vector<uint64_t> out_off((size_t)n + 1, 0);
	for (uint32_t g = 0; g < n; g++) {
		n_seg += count[g];
		if (n_seg > 0xFFFFFFFFull) {
			ctx->err = std::string(entry) + ": the union has more than 2^32 - 1 segments";
			return VGSDF_E_ARG;
		}
		seg_off[g + 1] = (uint32_t)n_seg;
		x0[g] = hd[g].x0, y0[g] = hd[g].y0, w[g] = hd[g].w, h[g] = hd[g].h, out_off[g] = hd[g].out_off;
		const uint64_t px = (uint64_t)w[g] * h[g];
		n_tiles += (px + VGSDF_TILE_PIXELS - 1) / VGSDF_TILE_PIXELS;
		n_pixels += px;
		n_pairs += px * count[g];
	}
	out_off[n] = src->out_bytes;
	if (n_tiles > 0x7FFFFFFFull) {
		ctx->err = std::string(entry) + ": batch too large (tile count exceeds 2^31-1); split it";
		return VGSDF_E_ARG;
	}

	// the new batch: the arena of vgsdf_batch_upload, descriptors and work list staged by the host, segments by the emit pass
	vgsdf_dbatch *b = new (std::nothrow) vgsdf_dbatch();
	if (!b) {
		ctx->err = std::string(entry) + ": out of host memory";
		return VGSDF_E_OOM;
	}
	const BatchArena at(n, n_tiles, n_seg, own_output ? src->out_bytes : 0);
	b->stats.n_glyphs = n, b->stats.n_segments = n_seg, b->stats.n_pixels = n_pixels, b->stats.n_pairs = n_pairs, b->stats.n_tiles = n_tiles;
	b->stats.alg_bytes = 32 * n_seg + 32 * (uint64_t)n + n_pixels;
	b->out_bytes = src->out_bytes;
	b->input_bytes = at.input_bytes, b->arena_bytes = at.bytes;
	const size_t stage_bytes = at.sx; // descriptors and work list
	hipError_t e = hipMalloc(&b->d_arena, b->arena_bytes + 16);
	if (e == hipSuccess && stage_bytes)
		e = hipHostMalloc(&b->h_stage, stage_bytes, hipHostMallocDefault);
	if (e != hipSuccess) {
		vgsdf_batch_free(ctx, b);
		return font_hip_error(ctx, entry, "hipMalloc", e);
	}
	uint8_t *const da = (uint8_t *)b->d_arena, *const hs = (uint8_t *)b->h_stage;
	b->d_glyphs = (vgsdf::GlyphDesc *)(da + at.desc);
	b->d_tiles = (vgsdf::SpanRec *)(da + at.tiles);
	b->d_sx = (double *)(da + at.sx), b->d_sy = (double *)(da + at.sy), b->d_ex = (double *)(da + at.ex), b->d_ey = (double *)(da + at.ey);
	b->seg_stride = 1;
	b->d_out = own_output ? da + at.out : nullptr;
	b->d_boxes = da + at.boxes;
	if (n) {
		vgsdf_batch in{};
		in.n_glyphs = n, in.seg_off = seg_off.data();
		in.x0 = x0.data(), in.y0 = y0.data(), in.w = w.data(), in.h = h.data(), in.out_off = out_off.data();
		build_descs_and_tiles(&in, (vgsdf::GlyphDesc *)(hs + at.desc), (vgsdf::SpanRec *)(hs + at.tiles), b, uses_span_list(ctx->variant));
		q.copy(b->d_arena, b->h_stage, stage_bytes);
		q.copy(d_off, seg_off.data(), 4 * ((size_t)n + 1));
		q.record(ev.at[1]);
		q.launch([&] {
			return vgsdf_outline_union_emit(src->d_glyphs, n, src->d_sx, src->d_sy, src->d_ex, src->d_ey, src->seg_stride, d_state, d_first, d_off,
			                                b->d_sx, b->d_sy, b->d_ex, b->d_ey, 1, q.st);
		});
		q.record(ev.at[2]);
		if (b->span_list)
			q.launch([&] { return vgsdf_launch_chunk_boxes(b->d_glyphs, n, b->d_sx, b->d_sy, b->d_ex, b->d_ey, 1, b->d_boxes, nullptr, 0, q.st); });
		q.sync(); // the call's device memory goes with it
		if (q.failed()) {
			vgsdf_batch_free(ctx, b);
			return font_hip_error(ctx, entry, "emit pass", q.e);
		}
		ev.elapsed(ctx->union_ms, 1);
	}
	if (state_out && n)
		std::memcpy(state_out, state.data(), n);
	*out = b;
	return VGSDF_OK;
}

extern "C" {

int vgsdf_batch_union(vgsdf_ctx *ctx, const vgsdf_dbatch *b, vgsdf_dbatch **out, uint8_t *state)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!b || !out) {
		ctx->err = "vgsdf_batch_union: NULL argument";
		return VGSDF_E_ARG;
	}
	return union_resident(ctx, "vgsdf_batch_union", b, out, state, /*own_output=*/true);
}

int vgsdf_batch_segments_read(vgsdf_ctx *ctx, const vgsdf_dbatch *b, uint32_t *seg_off, double *sx, double *sy, double *ex, double *ey)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!b || !seg_off) {
		ctx->err = "vgsdf_batch_segments_read: NULL argument";
		return VGSDF_E_ARG;
	}
	(void)hipSetDevice(ctx->device);
	const uint32_t n = (uint32_t)b->stats.n_glyphs;
	const size_t n_seg = (size_t)b->stats.n_segments;
	const bool all = sx && sy && ex && ey;
	std::vector<vgsdf::GlyphDesc> hd(n);
	std::vector<double> rec;
	Calls q(ctx->stream);
	if (n)
		q.read_back(hd.data(), b->d_glyphs, sizeof(vgsdf::GlyphDesc) * (size_t)n);
	if (all && n_seg) {
		if (b->seg_stride == 1) {
			q.read_back(sx, b->d_sx, 8 * n_seg), q.read_back(sy, b->d_sy, 8 * n_seg);
			q.read_back(ex, b->d_ex, 8 * n_seg), q.read_back(ey, b->d_ey, 8 * n_seg);
		} else { // records {sx, sy, ex, ey}
			rec.resize(4 * n_seg);
			q.read_back(rec.data(), b->d_sx, 32 * n_seg);
		}
	}
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, "vgsdf_batch_segments_read", "read-back", q.e);
	seg_off[0] = 0;
	for (uint32_t g = 0; g < n; g++) {
		seg_off[g] = hd[g].seg_off;
		seg_off[g + 1] = hd[g].seg_off + hd[g].n_seg;
	}
	for (size_t i = 0; i * 4 < rec.size(); i++)
		sx[i] = rec[4 * i], sy[i] = rec[4 * i + 1], ex[i] = rec[4 * i + 2], ey[i] = rec[4 * i + 3];
	return VGSDF_OK;
}

void vgsdf_union_kernel_ms(const vgsdf_ctx *ctx, float ms[2]) { pass_ms_out(ctx ? ctx->union_ms : nullptr, ms); }

} // extern "C"
