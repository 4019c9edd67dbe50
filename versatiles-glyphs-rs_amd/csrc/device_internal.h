// device_internal.h — what the translation units of the C-ABI layer (include/vgsdf.h) share: the context, the resident
// batch, grow-only buffers and the error macro.
//   vgsdf_device.cpp        contexts, resident batches, transfers and launches
//   work_list.cpp           the host's planner of a resident batch's work list
//   outline_front_end.cpp   outline commands in, rects and bitmaps out
//   resident_fonts.cpp      fonts uploaded once and named by glyph id (resident_fonts.h: what the front-end reads of them)
//   resident_glyf_tables.cpp, resident_charstrings.cpp, resident_gvar.cpp
//                           the fonts the device builds: from loca and glyf, from charstrings, from loca, glyf and gvar
//                           (resident_command_store.h: what the builders of command stores share)
//   resident_families.cpp   the families over them, named by code-point range (resident_build.h: what all of these share)
//   outline_union.cpp       union outlines: a resident batch's segments -> the boundary of its filled sets
//   run_counters.cpp        run counters and their RCCL reduction
// The kernels they launch are translation units of their own, each with a header of its name: sdf_kernels (raster),
// input_form_kernels, outline_kernels, outline_plan_kernels (the device front-end: input forms, flattening, plan),
// charstring_kernels, family_table_kernels, glyf_table_kernels (the constructors of resident stores), outline_union_kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>

#include "../../include/vgsdf.h"
#include "sdf_kernels.h"

// grow-only device / pinned-host buffer.  ensure() frees the old block at once: the caller sees to it that nothing in
// flight still uses it
struct DevBuf {
	void *p = nullptr;
	size_t cap = 0;
	bool host = false;
	hipError_t ensure(size_t bytes)
	{
		if (bytes <= cap)
			return hipSuccess;
		release();
		const size_t want = bytes + bytes / 4 + 256;
		hipError_t e = host ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
		if (e != hipSuccess) {
			p = nullptr;
			return e;
		}
		cap = want;
		return hipSuccess;
	}
	void release()
	{
		if (p)
			(void)(host ? hipHostFree(p) : hipFree(p));
		p = nullptr;
		cap = 0;
	}
};

struct vgsdf_ctx {
	int device = 0;
	hipStream_t stream = nullptr;
	hipStream_t copy_stream = nullptr;                 // the front-end's read-back, beside the kernels that follow the plan
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	hipEvent_t ev_plan = nullptr, ev_rects = nullptr;   // plan done (kernel stream) / rects on the host (copy stream)
	int variant = 0;
	std::string err;
	// arena and pinned staging of vgsdf_render_batch: no hipMalloc / hipHostMalloc in steady state
	DevBuf d_scratch, h_scratch{nullptr, 0, true};
	struct FrontEnd *fe = nullptr; // device outline front-end state (lazy; outline_front_end.cpp)
	// run counters {blocks, glyphs, pixels} of the work this context did (vgsdf_add_counters), summed over the
	// contexts of a run by vgsdf_reduce_counters; d_counters: 24 bytes on the device for the collective
	uint64_t counters[3] = {0, 0, 0};
	uint64_t *d_counters = nullptr;
	void *comm = nullptr; // ncclComm_t of the communicator this context last reduced in (owned by run_counters.cpp's cache)
	float charstring_ms[2] = {0.0f, 0.0f}; // count / emit kernels of the last vgsdf_font_create_charstrings / _charstrings2 (resident_charstrings.cpp)
	float charstring_batch_ms[2] = {0.0f, 0.0f}; // the same of the last vgsdf_fonts_create_charstrings2: one face at all its positions
	// vgsdf_font_create_charstrings2: operand slots past the decoder's LDS window, for one launch (at most 16384 glyph ids); grows
	// to exactly what the largest launch so far needed and belongs to no font
	void *charstring_spill = nullptr;
	size_t charstring_spill_bytes = 0;
	float family_tables_ms[2] = {0.0f, 0.0f}; // count / emit kernels of the last vgsdf_family_create_tables (resident_families.cpp)
	float family_census_ms = 0.0f;            // the kernel of the last vgsdf_family_tables_census (resident_families.cpp)
	float glyf_tables_ms[2] = {0.0f, 0.0f};   // count / emit kernels of the last vgsdf_font_create_tables (resident_glyf_tables.cpp)
	float glyf_batch_ms[2] = {0.0f, 0.0f};    // the same of the last vgsdf_fonts_create_tables: one launch each over all its faces
	float gvar_ms[3] = {0.0f, 0.0f, 0.0f};    // count / deltas / emit kernels of the last vgsdf_font_create_gvar (resident_gvar.cpp)
	float gvar_batch_ms[3] = {0.0f, 0.0f, 0.0f}; // the same of the last vgsdf_fonts_create_gvar: one face at all its positions
	// the phantom pass (all its launches) of the last vgsdf_gvar_advance_deltas or vgsdf_family_create_tables_gvar (resident_gvar.cpp)
	float gvar_advance_ms = 0.0f;
	// vgsdf_family_create_tables_gvar: the phantom pass's output for the call's faces, read by its emit pass; grown on demand,
	// belongs to no family (the call ends with a synchronisation)
	DevBuf gvar_advance;
	// phantom / count / emit kernels of the last vgsdf_families_create_tables (one face at many positions: 5 bytes per glyph id and
	// position of gvar_advance above); [0] alone of the last vgsdf_gvar_advance_deltas_batch
	float families_tables_ms[3] = {0.0f, 0.0f, 0.0f};
	// vgsdf_font_create_gvar, vgsdf_fonts_create_gvar: the deltas pass's scratch for one launch (GvarScratch: 13 bytes per point of
	// at most 2^17 points — points x positions in the batched call —, or of one glyph id at one position); grown on demand, belongs
	// to no font
	DevBuf gvar_scratch;
	float union_ms[2] = {0.0f, 0.0f}; // count / emit kernels of the last vgsdf_batch_union or vgsdf_outlines_union (outline_union.cpp)
	std::string reduce_path; // how the last vgsdf_reduce_counters with this context first took its sum (vgsdf_reduce_path)
};

struct vgsdf_dbatch {
	vgsdf_stats stats{};
	// one device arena: [descs | tiles | sx | sy | ex | ey | out]
	void *d_arena = nullptr;
	size_t arena_bytes = 0, input_bytes = 0;
	void *h_stage = nullptr; // pinned staging of the input part
	vgsdf::GlyphDesc *d_glyphs = nullptr;
	vgsdf::SpanRec *d_tiles = nullptr;
	void *d_boxes = nullptr; // chunk boxes (span kernel); NULL: none
	double *d_sx = nullptr, *d_sy = nullptr, *d_ex = nullptr, *d_ey = nullptr;
	uint32_t seg_stride = 1; // 1: four SoA arrays (C ABI batches); 4: 32-byte records (device front-end)
	uint8_t *d_out = nullptr;
	size_t out_bytes = 0;
	// work list = [main kernel | brute force]
	uint32_t n_main = 0; // entries [0, n_main): main kernel; the rest: brute-force tiles
	int tile_order = 1;
	bool span_list = false; // main-class entries say first pixel | tile count: sdf_tiles_span only
	bool borrowed = false; // arena + staging belong to the context (vgsdf_render_batch)
};

// kernel id understood by vgsdf_launch_tiles.  Variant 0 (default) = kernel 50: bounded groups over spans of tiles;
// misfits: brute force.  1: everything brute.  Other ids exist only in development builds (vgsdf_set_variant rejects
// them otherwise): earlier generations and timing-only ablations, see vgsdf_launch_tiles; 60..84 only in `make margins`
// builds: the margin instances of the span kernel (sdf_margin_kernels.hip).
inline int kernel_id(int variant) { return variant == 0 ? 50 : (variant == 13 ? 10 : variant); }
// the variant's main-class entries are spans: first pixel | tile count
inline bool uses_span_list(int variant) { return variant == 0 || (variant >= 50 && variant <= 99); }

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// the one device arena of a resident batch: [descs | tiles | sx | sy | ex | ey | out | chunk boxes], every part aligned to 256
// bytes; input_bytes: what the host stages (everything in front of `out`)
struct BatchArena {
	size_t desc = 0, tiles, sx, sy, ex, ey, input_bytes, out, boxes, bytes;
	BatchArena(uint32_t n_glyphs, uint64_t n_tiles, uint64_t n_seg, uint64_t n_pix)
	{
		const size_t A = 256;
		tiles = align_up(sizeof(vgsdf::GlyphDesc) * (size_t)n_glyphs, A);
		sx = align_up(tiles + sizeof(vgsdf::SpanRec) * (size_t)n_tiles, A);
		const size_t seg_bytes = align_up(sizeof(double) * (size_t)n_seg, A);
		sy = sx + seg_bytes, ex = sx + 2 * seg_bytes, ey = sx + 3 * seg_bytes;
		input_bytes = out = sx + 4 * seg_bytes;
		boxes = align_up(out + (size_t)n_pix, A);
		const size_t end = align_up(boxes + vgsdf_chunk_box_bytes(n_seg, n_glyphs), A);
		bytes = end ? end : A;
	}
};

inline double fe_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// (functions shared between the translation units stay out of the library's exported symbols)
#define VGSDF_INTERNAL __attribute__((visibility("hidden")))

// true when p is page-locked host memory known to HIP (hipHostMalloc / vgsdf_host_alloc):
// such arrays are DMA'd straight from/to the caller without a staging copy
VGSDF_INTERNAL bool is_pinned(const void *p, size_t bytes);
// The address a KERNEL may use for page-locked host memory: the mapping the runtime reports for it (equal to the host
// address for hipHostMalloc memory on this platform, but not guaranteed for memory the caller registered itself with
// hipHostRegister).  NULL when p is not page-locked host memory known to HIP, or has no device mapping.
VGSDF_INTERNAL void *pinned_device_ptr(void *p, size_t bytes);

// Fills the glyph descriptors and the tile list (routing + order) of a batch, and b->n_main, b->stats.n_tiles,
// b->span_list, b->tile_order.  `ht` must hold one entry per 256-pixel tile of the batch.  (work_list.cpp)
VGSDF_INTERNAL void build_descs_and_tiles(const vgsdf_batch *in, vgsdf::GlyphDesc *hd, vgsdf::SpanRec *ht, vgsdf_dbatch *b, bool span);

// Rule U over a resident batch (outline_union.cpp): a NEW batch with src's glyphs, rects and out_off whose segments are the
// boundary of the filled sets, with descriptors, work list and chunk boxes over them; complete on the device when the call
// returns.  own_output false: without an output buffer of its own (d_out NULL: the caller points it at one of out_bytes).
// state_out: [n_glyphs] or NULL.  `entry`: the exported function's name for the error text
VGSDF_INTERNAL int union_resident(vgsdf_ctx *ctx, const char *entry, const vgsdf_dbatch *src, vgsdf_dbatch **out, uint8_t *state_out,
                                  bool own_output);

// frees the front-end state of a context that is being destroyed (outline_front_end.cpp)
VGSDF_INTERNAL void fe_destroy(struct FrontEnd *fe);

// a failed HIP call ends the entry point: `what` (the text of the call, behind the caller's prefix if it has one) goes
// into the context's error string
#define HIP_TRY_AS(ctx, what, expr)                                                            \
	do {                                                                                       \
		hipError_t e__ = (expr);                                                               \
		if (e__ != hipSuccess) {                                                               \
			(ctx)->err = std::string(what ": ") + hipGetErrorString(e__);                      \
			return e__ == hipErrorOutOfMemory ? VGSDF_E_OOM : VGSDF_E_HIP;                     \
		}                                                                                      \
	} while (0)
#define HIP_TRY(ctx, expr) HIP_TRY_AS(ctx, #expr, expr)
