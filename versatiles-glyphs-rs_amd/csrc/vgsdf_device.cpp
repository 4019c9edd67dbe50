// vgsdf_device.cpp — C-ABI layer of libvgsdf.so (include/vgsdf.h): contexts, HBM-resident
// batches, transfers and launches.  No CPU fallback lives here or anywhere in the
// product: if HIP is unusable every entry point reports VGSDF_E_HIP.
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "device_internal.h"

namespace {
thread_local std::string g_create_error;
}

bool is_pinned(const void *p, size_t bytes)
{
	if (!p)
		return false;
	for (const void *q : {p, (const void *)((const uint8_t *)p + (bytes ? bytes - 1 : 0))}) { // first and last byte
		hipPointerAttribute_t a;
		if (hipPointerGetAttributes(&a, q) != hipSuccess) {
			(void)hipGetLastError(); // plain malloc memory: clear the sticky error
			return false;
		}
		if (a.type != hipMemoryTypeHost)
			return false;
	}
	return true;
}

void *pinned_device_ptr(void *p, size_t bytes)
{
	if (!is_pinned(p, bytes))
		return nullptr;
	hipPointerAttribute_t a;
	if (hipPointerGetAttributes(&a, p) != hipSuccess) {
		(void)hipGetLastError();
		return nullptr;
	}
	return a.devicePointer;
}

// HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues per device (default 4), and streams that share a
// queue run one after the other.  A renderer keeps two groups in flight on two contexts of two streams each: four streams — as
// soon as the host holds any other stream (PyTorch, its own contexts) two of ours share a queue and the overlap of one group's
// front-end with the other's raster is gone (measured in bench.py's process: Noto Sans all files 8.9 instead of 11.2 M glyphs/s).
// The variable is read when the HIP runtime starts, i.e. at the process's first HIP call: when this library is loaded before
// that and the variable is unset, 8 queues are asked for.  A host that starts HIP first sets it itself.
// (VGSDF_KEEP_HW_QUEUES=1 in the environment: the library leaves the variable alone.)
__attribute__((constructor)) static void vgsdf_default_hw_queues()
{
	const char *keep = std::getenv("VGSDF_KEEP_HW_QUEUES");
	if (!(keep && keep[0] == '1'))
		(void)setenv("GPU_MAX_HW_QUEUES", "8", /*overwrite=*/0);
}


extern "C" {

int vgsdf_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

int vgsdf_create(int device_ordinal, vgsdf_ctx **out)
{
	if (!out) {
		g_create_error = "vgsdf_create: out is NULL";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0) {
		g_create_error = std::string("vgsdf_create: no HIP device (") +
		                 (e != hipSuccess ? hipGetErrorString(e) : "device count 0") +
		                 "); this library has no CPU fallback";
		return VGSDF_E_HIP;
	}
	if (device_ordinal < 0 || device_ordinal >= n) {
		g_create_error = "vgsdf_create: device ordinal out of range";
		return VGSDF_E_ARG;
	}
	vgsdf_ctx *ctx = new (std::nothrow) vgsdf_ctx();
	if (!ctx) {
		g_create_error = "vgsdf_create: out of host memory";
		return VGSDF_E_OOM;
	}
	ctx->device = device_ordinal;
	if ((e = hipSetDevice(device_ordinal)) != hipSuccess ||
	    (e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess ||
	    (e = hipEventCreateWithFlags(&ctx->ev_plan, hipEventDisableTiming)) != hipSuccess ||
	    (e = hipEventCreateWithFlags(&ctx->ev_rects, hipEventDisableTiming)) != hipSuccess ||
	    (e = hipEventCreate(&ctx->ev0)) != hipSuccess || (e = hipEventCreate(&ctx->ev1)) != hipSuccess) {
		g_create_error = std::string("vgsdf_create: ") + hipGetErrorString(e);
		vgsdf_destroy(ctx);
		return VGSDF_E_HIP;
	}
	*out = ctx;
	return VGSDF_OK;
}

void vgsdf_destroy(vgsdf_ctx *ctx)
{
	if (!ctx)
		return;
	(void)hipSetDevice(ctx->device);
	if (ctx->stream) {
		(void)hipStreamSynchronize(ctx->stream);
		(void)hipStreamDestroy(ctx->stream);
	}
	if (ctx->copy_stream) {
		(void)hipStreamSynchronize(ctx->copy_stream);
		(void)hipStreamDestroy(ctx->copy_stream);
	}
	if (ctx->ev_plan)
		(void)hipEventDestroy(ctx->ev_plan);
	if (ctx->ev_rects)
		(void)hipEventDestroy(ctx->ev_rects);
	if (ctx->ev0)
		(void)hipEventDestroy(ctx->ev0);
	if (ctx->ev1)
		(void)hipEventDestroy(ctx->ev1);
	fe_destroy(ctx->fe);
	if (ctx->d_counters)
		(void)hipFree(ctx->d_counters);
	ctx->d_scratch.release();
	ctx->h_scratch.release();
	if (ctx->charstring_spill)
		(void)hipFree(ctx->charstring_spill);
	ctx->gvar_scratch.release();
	ctx->gvar_advance.release();
	delete ctx;
}

const char *vgsdf_last_error(const vgsdf_ctx *ctx)
{
	return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int vgsdf_set_variant(vgsdf_ctx *ctx, int variant)
{
	if (!ctx)
		return VGSDF_E_ARG;
	// the product build knows 0 (default) and 1 (brute force); development builds (-DVGSDF_DEV_VARIANTS)
	// add the earlier generations and the timing-only ablations
	if (!vgsdf_kernel_known(kernel_id(variant)) || variant == 50) {
		ctx->err = "vgsdf_set_variant: unknown kernel variant " + std::to_string(variant);
		return VGSDF_E_ARG;
	}
	ctx->variant = variant;
	return VGSDF_OK;
}

int vgsdf_sync(vgsdf_ctx *ctx)
{
	if (!ctx)
		return VGSDF_E_ARG;
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return VGSDF_OK;
}

int vgsdf_batch_free(vgsdf_ctx *ctx, vgsdf_dbatch *b)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!b)
		return VGSDF_OK;
	(void)hipSetDevice(ctx->device);
	(void)hipStreamSynchronize(ctx->stream);
	if (!b->borrowed) {
		if (b->d_arena)
			(void)hipFree(b->d_arena);
		if (b->h_stage)
			(void)hipHostFree(b->h_stage);
	}
	delete b;
	return VGSDF_OK;
}

// Argument and shape checks of a batch, on the host BEFORE anything is launched: the kernels index with the shapes.
// Fills the counts of `stats` (all but alg_bytes)
static int check_batch(vgsdf_ctx *ctx, const vgsdf_batch *in, vgsdf_stats &stats)
{
	const uint32_t n = in->n_glyphs;
	if (n && (!in->seg_off || !in->x0 || !in->y0 || !in->w || !in->h || !in->out_off)) {
		ctx->err = "vgsdf_batch_upload: NULL array in batch";
		return VGSDF_E_ARG;
	}
	const uint64_t n_seg = n ? in->seg_off[n] : 0;
	if (n_seg && (!in->seg_sx || !in->seg_sy || !in->seg_ex || !in->seg_ey)) {
		ctx->err = "vgsdf_batch_upload: NULL segment array";
		return VGSDF_E_ARG;
	}
	stats = vgsdf_stats{};
	stats.n_glyphs = n;
	stats.n_segments = n_seg;
	if (n && in->seg_off[0] != 0) {
		ctx->err = "vgsdf_batch_upload: seg_off[0] must be 0";
		return VGSDF_E_ARG;
	}
	for (uint32_t g = 0; g < n; g++) {
		if (in->seg_off[g + 1] < in->seg_off[g]) {
			ctx->err = "vgsdf_batch_upload: seg_off not monotone";
			return VGSDF_E_ARG;
		}
		const uint64_t px = (uint64_t)in->w[g] * in->h[g];
		if (px > 0xFFFFFFFFull - VGSDF_TILE_PIXELS || in->out_off[g + 1] < in->out_off[g] || in->out_off[g + 1] - in->out_off[g] < px) {
			ctx->err = "vgsdf_batch_upload: out_off inconsistent with w*h (bitmap g needs out_off[g] + w*h <= out_off[g+1])";
			return VGSDF_E_ARG;
		}
		stats.n_tiles += (px + VGSDF_TILE_PIXELS - 1) / VGSDF_TILE_PIXELS;
		stats.n_pairs += px * (in->seg_off[g + 1] - in->seg_off[g]);
		stats.n_pixels += px;
	}
	if (stats.n_tiles > 0x7FFFFFFFull) {
		ctx->err = "vgsdf_batch_upload: batch too large (tile count exceeds 2^31-1); split it";
		return VGSDF_E_ARG;
	}
	return VGSDF_OK;
}

static int upload_impl(vgsdf_ctx *ctx, const vgsdf_batch *in, vgsdf_dbatch **out, bool use_ctx_scratch)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out) {
		ctx->err = "vgsdf_batch_upload: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	vgsdf_stats stats;
	if (int rc = check_batch(ctx, in, stats); rc != VGSDF_OK)
		return rc;
	const uint32_t n = in->n_glyphs;
	const uint64_t n_seg = stats.n_segments, n_tiles = stats.n_tiles, n_pixels = stats.n_pixels;
	const uint64_t n_pix = n ? in->out_off[n] : 0; // size of the output buffer (>= the pixels: gaps are allowed)

	vgsdf_dbatch *b = new (std::nothrow) vgsdf_dbatch();
	if (!b) {
		ctx->err = "vgsdf_batch_upload: out of host memory";
		return VGSDF_E_OOM;
	}
	b->stats = stats;
	b->stats.alg_bytes = 32 * n_seg + 32 * (uint64_t)n + n_pixels;
	b->out_bytes = n_pix;

	const BatchArena at(n, n_tiles, n_seg, n_pix);
	const size_t off_desc = at.desc, off_tiles = at.tiles, off_sx = at.sx, off_sy = at.sy, off_ex = at.ex, off_ey = at.ey, off_out = at.out,
	             off_boxes = at.boxes;
	b->input_bytes = at.input_bytes;
	b->arena_bytes = at.bytes;

	(void)hipSetDevice(ctx->device);
	hipError_t e = hipSuccess;
	// segment arrays already page-locked: DMA them directly, stage only descriptors + tiles
	const size_t seg_nb = sizeof(double) * (size_t)n_seg;
	const bool direct = n_seg && is_pinned(in->seg_sx, seg_nb) && is_pinned(in->seg_sy, seg_nb) &&
	                    is_pinned(in->seg_ex, seg_nb) && is_pinned(in->seg_ey, seg_nb);
	const size_t stage_bytes = direct ? off_sx : b->input_bytes;
	if (use_ctx_scratch) {
		b->borrowed = true;
		if (ctx->d_scratch.cap < b->arena_bytes || ctx->h_scratch.cap < stage_bytes)
			(void)hipStreamSynchronize(ctx->stream); // a buffer is about to be freed: nothing in flight may still use it
		const char *what = "hipMalloc";
		if ((e = ctx->d_scratch.ensure(b->arena_bytes)) == hipSuccess) {
			what = "hipHostMalloc";
			e = ctx->h_scratch.ensure(stage_bytes);
		}
		if (e != hipSuccess) {
			ctx->err = std::string("vgsdf_render_batch: ") + what + ": " + hipGetErrorString(e);
			delete b;
			return VGSDF_E_OOM;
		}
		b->d_arena = ctx->d_scratch.p;
		b->h_stage = ctx->h_scratch.p;
	} else {
		e = hipMalloc(&b->d_arena, b->arena_bytes);
		if (e != hipSuccess) {
			ctx->err = std::string("vgsdf_batch_upload: hipMalloc: ") + hipGetErrorString(e);
			delete b;
			return VGSDF_E_OOM;
		}
		if (stage_bytes) {
			e = hipHostMalloc(&b->h_stage, stage_bytes, hipHostMallocDefault);
			if (e != hipSuccess) {
				ctx->err = std::string("vgsdf_batch_upload: hipHostMalloc: ") + hipGetErrorString(e);
				vgsdf_batch_free(ctx, b);
				return VGSDF_E_OOM;
			}
		}
	}
	uint8_t *hs = (uint8_t *)b->h_stage, *da = (uint8_t *)b->d_arena;
	b->d_glyphs = (vgsdf::GlyphDesc *)(da + off_desc);
	b->d_tiles = (vgsdf::SpanRec *)(da + off_tiles);
	b->d_sx = (double *)(da + off_sx);
	b->d_sy = (double *)(da + off_sy);
	b->d_ex = (double *)(da + off_ex);
	b->d_ey = (double *)(da + off_ey);
	b->d_out = da + off_out;
	b->d_boxes = da + off_boxes;

	if (n) {
		vgsdf::GlyphDesc *hd = (vgsdf::GlyphDesc *)(hs + off_desc);
		vgsdf::SpanRec *ht = (vgsdf::SpanRec *)(hs + off_tiles);
		build_descs_and_tiles(in, hd, ht, b, uses_span_list(ctx->variant));
		if (n_seg && !direct) {
			std::memcpy(hs + off_sx, in->seg_sx, sizeof(double) * n_seg);
			std::memcpy(hs + off_sy, in->seg_sy, sizeof(double) * n_seg);
			std::memcpy(hs + off_ex, in->seg_ex, sizeof(double) * n_seg);
			std::memcpy(hs + off_ey, in->seg_ey, sizeof(double) * n_seg);
		}
		e = hipMemcpyAsync(b->d_arena, b->h_stage, stage_bytes, hipMemcpyHostToDevice, ctx->stream);
		if (e == hipSuccess && direct) {
			const size_t nb = sizeof(double) * n_seg;
			e = hipMemcpyAsync(b->d_sx, in->seg_sx, nb, hipMemcpyHostToDevice, ctx->stream);
			if (e == hipSuccess)
				e = hipMemcpyAsync(b->d_sy, in->seg_sy, nb, hipMemcpyHostToDevice, ctx->stream);
			if (e == hipSuccess)
				e = hipMemcpyAsync(b->d_ex, in->seg_ex, nb, hipMemcpyHostToDevice, ctx->stream);
			if (e == hipSuccess)
				e = hipMemcpyAsync(b->d_ey, in->seg_ey, nb, hipMemcpyHostToDevice, ctx->stream);
		}
		if (e == hipSuccess && b->span_list)
			e = (hipError_t)vgsdf_launch_chunk_boxes(b->d_glyphs, n, b->d_sx, b->d_sy, b->d_ex, b->d_ey, 1, b->d_boxes, nullptr, 0, ctx->stream);
		// page-locked caller arrays are DMA'd in place: the copies must be over before the caller may
		// touch them again (vgsdf.h: the batch is read-only "for the call")
		if (e == hipSuccess && direct)
			e = hipStreamSynchronize(ctx->stream);
		if (e != hipSuccess) {
			ctx->err = std::string("vgsdf_batch_upload: H2D: ") + hipGetErrorString(e);
			vgsdf_batch_free(ctx, b);
			return VGSDF_E_HIP;
		}
	}
	*out = b;
	return VGSDF_OK;
}

int vgsdf_batch_upload(vgsdf_ctx *ctx, const vgsdf_batch *in, vgsdf_dbatch **out)
{
	return upload_impl(ctx, in, out, false);
}

void *vgsdf_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { // every device of the process may read / write it
		(void)hipGetLastError();
		return nullptr;
	}
	return p;
}

void vgsdf_host_free(void *p)
{
	if (p)
		(void)hipHostFree(p);
}

int vgsdf_batch_launch(vgsdf_ctx *ctx, vgsdf_dbatch *b)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!b) {
		ctx->err = "vgsdf_batch_launch: NULL batch";
		return VGSDF_E_ARG;
	}
	(void)hipSetDevice(ctx->device);
	const uint32_t n_all = (uint32_t)b->stats.n_tiles;
	const int v = ctx->variant;
	const uint32_t n_main = v == 1 ? 0 : b->n_main;
	const int k_main = kernel_id(v);
	if (b->stats.n_tiles != 0 && uses_span_list(v) != b->span_list) {
		ctx->err = "vgsdf_batch_launch: the batch was uploaded for a different kernel variant (tile list layout)";
		return VGSDF_E_ARG;
	}
	const int list_order = b->tile_order == 1;
	int e = vgsdf_launch_tiles(k_main, list_order, b->d_tiles, n_main, b->d_sx, b->d_sy, b->d_ex, b->d_ey,
	                           b->seg_stride, b->d_out, b->span_list ? b->d_boxes : nullptr, ctx->stream);
	if (e == 0)
		e = vgsdf_launch_tiles(1, list_order, b->d_tiles + n_main, n_all - n_main, b->d_sx, b->d_sy, b->d_ex,
		                       b->d_ey, b->seg_stride, b->d_out, nullptr, ctx->stream);
	if (e != 0) {
		ctx->err = std::string("vgsdf_batch_launch: ") + hipGetErrorString((hipError_t)e);
		return VGSDF_E_HIP;
	}
	return VGSDF_OK;
}

int vgsdf_batch_download(vgsdf_ctx *ctx, vgsdf_dbatch *b, uint8_t *out_bitmaps)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!b || (!out_bitmaps && b->out_bytes)) {
		ctx->err = "vgsdf_batch_download: NULL argument";
		return VGSDF_E_ARG;
	}
	(void)hipSetDevice(ctx->device);
	if (b->out_bytes)
		HIP_TRY(ctx, hipMemcpyAsync(out_bitmaps, b->d_out, b->out_bytes, hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return VGSDF_OK;
}

int vgsdf_batch_stats(const vgsdf_dbatch *b, vgsdf_stats *out)
{
	if (!b || !out)
		return VGSDF_E_ARG;
	*out = b->stats;
	return VGSDF_OK;
}

void *vgsdf_batch_device_output(const vgsdf_dbatch *b) { return b ? b->d_out : nullptr; }

int vgsdf_batch_time(vgsdf_ctx *ctx, vgsdf_dbatch *b, int iters, float *total_ms)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!b || !total_ms || iters < 1) {
		ctx->err = "vgsdf_batch_time: bad argument";
		return VGSDF_E_ARG;
	}
	(void)hipSetDevice(ctx->device);
	HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
	for (int i = 0; i < iters; i++) {
		int rc = vgsdf_batch_launch(ctx, b);
		if (rc != VGSDF_OK)
			return rc;
	}
	HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
	HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
	HIP_TRY(ctx, hipEventElapsedTime(total_ms, ctx->ev0, ctx->ev1));
	return VGSDF_OK;
}

int vgsdf_render_batch(vgsdf_ctx *ctx, const vgsdf_batch *in, uint8_t *out_bitmaps)
{
	if (!ctx)
		return VGSDF_E_ARG;
	vgsdf_dbatch *b = nullptr;
	int rc = upload_impl(ctx, in, &b, true);
	if (rc != VGSDF_OK)
		return rc;
	rc = vgsdf_batch_launch(ctx, b);
	if (rc == VGSDF_OK)
		rc = vgsdf_batch_download(ctx, b, out_bitmaps);
	vgsdf_batch_free(ctx, b);
	return rc;
}

} // extern "C"
