/*
 * vgsdf.h — C ABI of the MI355X SDF raster (libvgsdf.so).
 *
 * Drop-in boundary for the per-glyph hot loop of versatiles-glyphs-rs: one call renders
 * the signed-distance bitmaps of a whole batch of glyphs on the GPU, bit-exact with
 *   renderer_precise()               src/render/renderer_precise.rs:8-84
 *   min_distance_to_line_segment()   src/render/rtree_segments.rs:40-68
 *   Segment::squared_distance_to_point / project_point_on   src/geometry/segment.rs:54-99
 * which the reference runs once per glyph from Renderer::render_glyph
 * (src/render/renderer.rs:140-143, the `match self.mode` arm a new back-end slots into).
 * The caller is the GPU batch dispatcher that replaces the rayon block loop of
 * FontManager::render_glyphs (src/font/manager.rs:104-121); see vgfont.h.
 *
 * Plain C: pointers + sizes, no C++/torch types, no exceptions across the boundary.
 * Every entry point returns VGSDF_OK (0) or a negative vgsdf_status; the message is
 * available from vgsdf_last_error().  There is NO CPU fallback: without a usable HIP
 * device vgsdf_create() fails with VGSDF_E_HIP.
 *
 * Reference-side binding (Rust `extern "C"` block, untested here — no rustc in this
 * image): INTEGRATION.md.
 */
#ifndef VGSDF_H
#define VGSDF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
	VGSDF_OK = 0,
	VGSDF_E_ARG = -1, /* NULL / inconsistent batch */
	VGSDF_E_HIP = -2, /* HIP runtime error (no device, launch failure, ...) */
	VGSDF_E_OOM = -3, /* device or pinned-host allocation failed */
	VGSDF_E_GLYF = -4 /* vgsdf_outlines_submit_glyf: a malformed `glyf` entry in the batch — record it with a host reader instead */
} vgsdf_status;

/* One context per (host thread, GPU): owns a HIP stream, device buffers and pinned
 * staging.  Not thread-safe; use one per thread. */
typedef struct vgsdf_ctx vgsdf_ctx;
/* A batch resident in HBM (segments, descriptors, tile list, output bitmaps). */
typedef struct vgsdf_dbatch vgsdf_dbatch;

/*
 * Host-side SoA batch, caller-owned, read-only during the call.
 *
 * Segments are what Rings::get_segments() yields (src/geometry/rings.rs:75-81) AFTER
 * rings.scale() and rings.translate() (renderer.rs:122,131): consecutive point pairs per
 * ring, rings in order, f64 pixel units.  Glyph g owns segments
 * [seg_off[g], seg_off[g+1]).  (x0,y0,w,h) is RenderResult{x0,y0,width,height}
 * (src/render/result.rs:7-29), i.e. including the 3 px buffer on every side.
 * Output bitmap of glyph g: out[out_off[g] + (h-1-y)*w + x], row-major, top row first —
 * exactly renderer_precise.rs:78.  out_off is ascending with out_off[g] + w[g]*h[g] <= out_off[g+1]: normally the prefix
 * sums of w*h (bitmaps packed back to back); a caller that assembles its output in place (the host façade lays the
 * bitmaps out where the finished PBF blocks have them) leaves gaps, whose bytes are not written.  out_off[n_glyphs] is
 * the size of the output buffer.
 */
typedef struct {
	uint32_t n_glyphs;
	const uint32_t *seg_off; /* [n_glyphs+1] prefix sums */
	const double *seg_sx;    /* [seg_off[n_glyphs]] */
	const double *seg_sy;
	const double *seg_ex;
	const double *seg_ey;
	const int32_t *x0; /* [n_glyphs] */
	const int32_t *y0;
	const uint32_t *w;
	const uint32_t *h;
	const uint64_t *out_off; /* [n_glyphs+1] ascending, see above */
} vgsdf_batch;

/* Per-launch statistics (filled by vgsdf_batch_stats). */
typedef struct {
	uint64_t n_glyphs;
	uint64_t n_segments;
	uint64_t n_pixels;
	uint64_t n_pairs;   /* sum over glyphs of w*h*n_segments (pixel x segment evaluations) */
	uint64_t n_tiles;   /* workgroups launched */
	uint64_t alg_bytes; /* 32*segments + 32*glyphs + pixels   */
} vgsdf_stats;

int vgsdf_device_count(void);
int vgsdf_create(int device_ordinal, vgsdf_ctx **out);
void vgsdf_destroy(vgsdf_ctx *ctx);
const char *vgsdf_last_error(const vgsdf_ctx *ctx); /* ctx may be NULL: last create error */

/* Page-locked host memory (hipHostMalloc).  Batch arrays / output buffers allocated with it
 * are DMA'd directly by vgsdf_render_batch / vgsdf_batch_upload / _download (no staging
 * copy).  Returns NULL when HIP is unavailable.  Optional: plain memory works too. */
void *vgsdf_host_alloc(size_t bytes);
void vgsdf_host_free(void *p);

/* Synchronous whole-batch render: H2D, kernel, D2H; out_bitmaps is host memory of
 * out_off[n_glyphs] bytes. */
int vgsdf_render_batch(vgsdf_ctx *ctx, const vgsdf_batch *in, uint8_t *out_bitmaps);

/* Split form, for callers that keep batches resident / overlap transfers:
 *   upload   : validates, builds the tile list, copies everything to HBM (async on the
 *              context stream, staged through pinned memory).
 *   launch   : enqueues the SDF kernel on the context stream (asynchronous).
 *   download : enqueues D2H of all bitmaps and waits for it.
 *   sync     : waits for the context stream. */
int vgsdf_batch_upload(vgsdf_ctx *ctx, const vgsdf_batch *in, vgsdf_dbatch **out);
int vgsdf_batch_launch(vgsdf_ctx *ctx, vgsdf_dbatch *b);
int vgsdf_batch_download(vgsdf_ctx *ctx, vgsdf_dbatch *b, uint8_t *out_bitmaps);
int vgsdf_batch_free(vgsdf_ctx *ctx, vgsdf_dbatch *b);
int vgsdf_sync(vgsdf_ctx *ctx);
int vgsdf_batch_stats(const vgsdf_dbatch *b, vgsdf_stats *out);

/* Times `iters` back-to-back launches of the SDF kernel with HIP events recorded on the
 * context stream (the stream the kernel runs on); *total_ms = elapsed for all of them. */
int vgsdf_batch_time(vgsdf_ctx *ctx, vgsdf_dbatch *b, int iters, float *total_ms);

/* Selects the kernel variant: 0 = default (bounded-group span kernel), 1 = brute force (every pixel
 * against every segment in f64; A/B reference).  Both are bit-exact with the reference.  Any other
 * value fails with VGSDF_E_ARG (development builds of the library, `make dev`, accept more ids for
 * kernel experiments; those are not part of the product).  Set it BEFORE uploading / preparing a
 * batch: the work list layout depends on it, and launching a resident batch under a different
 * variant fails with VGSDF_E_ARG. */
int vgsdf_set_variant(vgsdf_ctx *ctx, int variant);

/*
 * Device front-end: the host only records the OutlineBuilder callbacks of
 * every glyph (f32 font units); flattening (ring_builder.rs:62-110, ring.rs:119-187), ring
 * closing (ring.rs:53-63), scale / shift (renderer.rs:122-131), bbox + buffer
 * (renderer.rs:64-91) and Rings::get_segments run on the GPU, bit-exact with the host path.
 *   prepare : commands in -> per-glyph rects out (needed for the PBF metrics and to size the
 *             output); leaves segments, descriptors and tiles resident on the device.
 *   render  : SDF raster of the prepared batch; bitmaps of the glyphs with has_raster != 0
 *             are packed back to back in glyph order (w*h bytes each).
 */
typedef struct {
	float x1, y1;  /* quad control / first cubic control */
	float x2, y2;  /* second cubic control */
	float x, y;    /* end point */
	uint32_t kind; /* 0 move_to, 1 line_to, 2 quad_to, 3 curve_to, 4 close */
} vgsdf_outline_cmd;

typedef struct {
	uint32_t n_glyphs;
	const uint32_t *cmd_off;       /* [n_glyphs+1] prefix sums */
	const vgsdf_outline_cmd *cmds; /* [cmd_off[n_glyphs]] */
	const double *scale;           /* [n_glyphs] GLYPH_SIZE / units_per_em (renderer.rs:107) */
	const double *shift_x;         /* [n_glyphs] (advance - advance_float) / 2 (renderer.rs:130) */
} vgsdf_outlines;

typedef struct {
	int32_t x0, y0;      /* RenderResult.x0 / y0 (incl. -3 buffer) */
	uint32_t w, h;       /* RenderResult.width / height (incl. +6) */
	uint32_t n_segments;
	uint32_t has_raster; /* 0 => PbfGlyph::empty (no ring survived, or empty bbox) */
} vgsdf_rect;

int vgsdf_outlines_prepare(vgsdf_ctx *ctx, const vgsdf_outlines *in, vgsdf_rect *rects_out, uint64_t *out_bytes,
                           uint64_t *n_segments);
int vgsdf_outlines_render(vgsdf_ctx *ctx, uint8_t *out_bitmaps);
/* prepare + render as ONE submission: the raster is enqueued right behind the front-end kernels, before the host
 * has seen the sizes; the device checks the grid and every capacity it was launched against.  `out_bitmaps` holds
 * `out_capacity` bytes (from earlier batches, or a guess).  If it comes from vgsdf_host_alloc() the raster writes
 * the bitmaps straight into it (no copy, one synchronisation per call).  On return *out_bytes is the size needed;
 * *rendered = 1: the bitmaps are in out_bitmaps (packed in glyph order, as vgsdf_outlines_render leaves them);
 * *rendered = 0 (only when *out_bytes > out_capacity): the batch stays prepared — grow the buffer and call
 * vgsdf_outlines_render().  Results are identical to prepare + render. */
int vgsdf_outlines_render_into(vgsdf_ctx *ctx, const vgsdf_outlines *in, vgsdf_rect *rects_out, uint8_t *out_bitmaps,
                               size_t out_capacity, uint64_t *out_bytes, uint64_t *n_segments, int *rendered);
/* The same in two halves, for callers that overlap their own work with the device (one batch in flight per context;
 * use two contexts to keep the GPU busy while the host prepares the next batch and encodes the previous one):
 * submit enqueues the upload, the front-end and the raster and returns at once; wait synchronises and reports as
 * vgsdf_outlines_render_into does.  in->cmds and out_bitmaps must stay valid and untouched in between
 * (out_bitmaps may be NULL: no raster is enqueued, wait then equals vgsdf_outlines_prepare).
 * A submit that fails — this one or any of the vgsdf_outlines_submit_* forms below — leaves nothing to wait for, and nothing
 * of the caller's memory in use: whatever it had enqueued before the failing step (the upload of a page-locked block, which a
 * kernel reads in place and under which the block's offsets are validated; a raster storing through out_bitmaps) has
 * finished when the call returns.  Input and output buffers may be freed or reused at once. */
int vgsdf_outlines_submit(vgsdf_ctx *ctx, const vgsdf_outlines *in, uint8_t *out_bitmaps, size_t out_capacity);
/* The same commands in their compact form for the upload: one kind byte per command and only the coordinates the kind
 * carries, in callback order (move_to / line_to: x y; quad_to: x1 y1 x y; curve_to: x1 y1 x2 y2 x y; close: none) —
 * about 12 bytes per command of a TrueType font instead of 28.  dat_off[g] .. dat_off[g + 1] is glyph g's range of
 * `coords` (dat_off[0] = 0); it must match the kinds (VGSDF_E_ARG otherwise).  Everything else as
 * vgsdf_outlines_submit; collect with vgsdf_outlines_wait.  When the arrays sit back to back in ONE block from
 * vgsdf_host_alloc() in the order scale | shift_x | cmd_off | dat_off | (pad to a multiple of 8 bytes) | coords | kinds
 * the library uploads them with a single copy. */
typedef struct {
	uint32_t n_glyphs;
	const uint32_t *cmd_off; /* [n_glyphs + 1] into kinds */
	const uint32_t *dat_off; /* [n_glyphs + 1] into coords */
	const uint8_t *kinds;    /* [cmd_off[n_glyphs]] 0..4 = move / line / quad / curve / close */
	const float *coords;     /* [dat_off[n_glyphs]] */
	const double *scale;     /* [n_glyphs] */
	const double *shift_x;   /* [n_glyphs] */
	/* In-place PBF assembly (both NULL: the bitmaps are packed back to back).  The output buffer becomes an ARENA of
	 * finished glyphs-PBF blocks (src/protobuf/glyphs.rs:66-70): the device lays the glyphs out as the `glyphs` entries
	 * of their fontstack message —
	 *   0x1A varint(len) | 0x08 varint(id) | [0x12 varint(w h) BITMAP] | 0x18 width 0x20 height 0x28 left 0x30 top 0x38 advance
	 * (glyph.rs:10-41; width = w - 6, height = h - 6, left = x0 + 3, top = y0 + h - 27: result.rs:66-76 after
	 * renderer.rs:146; a glyph without a raster is PbfGlyph::empty, glyph.rs:60-70) — one after the other, and the raster
	 * stores every BITMAP where the finished file has it; all other bytes are left for the caller, who knows id, advance and
	 * the block headers and gets w, h, x0, y0 back in the rects (the host façade writes them: csrc/host/pbf.hpp,
	 * write_pbf_entry_headers).  Glyph g starts at the running sum of what the glyphs before it occupy plus pbf_pre[g]:
	 *   pbf_pre[g]  bytes reserved in front of glyph g's entry (the file + fontstack header of the block it opens, else 0)
	 *   pbf_fix[g]  (1 + varint_len(id)) | (1 + varint_len(advance)) << 4
	 * *out_bytes of vgsdf_outlines_wait is the size of the arena.  In the single-copy block of vgsdf_host_alloc() the two
	 * arrays follow `kinds`: ... | kinds | (pad to a multiple of 4 bytes) | pbf_pre | pbf_fix. */
	const uint32_t *pbf_pre; /* [n_glyphs] or NULL */
	const uint8_t *pbf_fix;  /* [n_glyphs] or NULL */
} vgsdf_outlines_packed;
int vgsdf_outlines_submit_packed(vgsdf_ctx *ctx, const vgsdf_outlines_packed *in, uint8_t *out_bitmaps, size_t out_capacity);
/* The same front-end fed with the glyphs' `glyf` entries themselves: the host only looks glyphs up (cmap, loca, the
 * component records of composite glyphs) and copies bytes; the device replays ttf-parser's walk of every simple glyph
 * (glyf.rs parse_simple_outline + Builder: flag runs, short / repeated coordinates, wrapping i16 sums, implied on-curve
 * midpoints, the closing curve of a contour) and produces the callbacks Face::outline_glyph would deliver
 * (/root/reference/src/render/renderer.rs:110), then runs on as above.  One PART per simple glyph:
 *   bytes[byte_off .. +byte_len)  endPtsOfContours[n_contours] (big-endian u16, as in the font) followed by the entry's
 *                                 flags / xCoordinates / yCoordinates exactly as they stand in the font (the bytes from behind
 *                                 the instructions to the end of the entry); byte_off a multiple of 4
 *   a b c d e f                   the transform ttf-parser has accumulated for the component (x' = a x + c y + e,
 *                                 y' = b x + d y + f, in f32); plain = 1 for the identity (a simple glyph drawn as itself)
 *   cmd_at, cmd_cap               its command slots: cmd_cap >= points + 2 * contours of the entry (what its end points say);
 *                                 the parts tile [0, cmd_off[n_glyphs]) in order, glyph g owns [cmd_off[g], cmd_off[g + 1])
 * A glyph without outline has no part and no slots.  Slots a part does not need are filled with close() callbacks, which
 * do nothing on the empty ring behind a contour's own close().  An entry whose arrays do not fit its bytes or its slots
 * (ttf-parser returns None for such a glyph and, in a composite, skips the components behind it) fails the whole batch with
 * VGSDF_E_GLYF in vgsdf_outlines_wait: the caller records that batch with its host reader and submits commands instead.
 * The decoder has two limits of its own per part, and a well-formed entry beyond either fails the batch the same way: an entry
 * of more than 6144 points, or a byte_len above 30720 (30 KB: end points + arrays, whatever lies behind them included).
 * In ONE block from vgsdf_host_alloc() in the order scale | shift_x | cmd_off | (pad to a multiple of 8 bytes) | parts | bytes
 * [| pbf_pre | pbf_fix] the batch is uploaded with a single copy — by a kernel reading the block itself (it is device-mapped), so no
 * copy-engine hand-over sits in front of the decoder — and its offsets are validated under that copy.  When every scale is positive
 * and finite and no part's slots straddle two glyphs the decoder also notes the ring state in front of every callback (what
 * ring_builder.rs:83-85,99-101 ask) and the separate context pass is skipped.  pbf_pre / pbf_fix as in vgsdf_outlines_packed. */
typedef struct {
	uint32_t byte_off, byte_len;
	uint32_t cmd_at, cmd_cap;
	uint32_t n_contours; /* > 0 */
	uint32_t plain;
	float a, b, c, d, e, f;
} vgsdf_glyf_part;
typedef struct {
	uint32_t n_glyphs, n_parts, n_bytes; /* n_bytes a multiple of 4 */
	const uint32_t *cmd_off;      /* [n_glyphs + 1] command slots, cmd_off[0] = 0 */
	const vgsdf_glyf_part *parts; /* [n_parts] */
	const uint8_t *bytes;         /* [n_bytes] */
	const double *scale;          /* [n_glyphs] */
	const double *shift_x;        /* [n_glyphs] */
	const uint32_t *pbf_pre;      /* [n_glyphs] or NULL */
	const uint8_t *pbf_fix;       /* [n_glyphs] or NULL */
} vgsdf_outlines_glyf;
int vgsdf_outlines_submit_glyf(vgsdf_ctx *ctx, const vgsdf_outlines_glyf *in, uint8_t *out_bitmaps, size_t out_capacity);
/*
 * Resident fonts: a font's outlines are uploaded ONCE and live in HBM; a submission then names glyphs by (font, glyph id)
 * and carries 33 bytes per glyph instead of the parts and a copy of the `glyf` arrays.  Output is the glyf form's, byte for byte.
 *
 * vgsdf_font_desc describes a face: for every glyph id its LEAVES — the simple glyphs it is drawn from, records as the parts of
 * vgsdf_outlines_glyf, except that cmd_at counts from the glyph's FIRST slot (the leaves of one glyph tile [0, its slot count)
 * in order) and byte_off points into `bytes`, where every simple glyph's endPtsOfContours + flag / x / y arrays are stored
 * once, 4-aligned, however many composites name it.
 * vgsdf_font_create validates the description on the host (leaf_off ascending from 0 to n_leaves, every leaf's byte range
 * 4-aligned inside `bytes`, the leaves tiling their glyph's slots, n_contours > 0, plain 0 or 1; VGSDF_E_ARG otherwise), copies
 * the three arrays to the device and returns when they are there: the description may be freed at once.  The font belongs to the
 * context's DEVICE, not to the context: every context of that device may name it from then on (a font of another device is
 * VGSDF_E_ARG in a submission).  vgsdf_font_free is the caller's to time: no submission that names the font may be in
 * flight (submitted and not yet waited for) on any context.  vgsdf_font_device_bytes: what the font occupies on the device.
 */
typedef struct vgsdf_font vgsdf_font;
typedef struct {
	uint32_t n_glyph_ids;          /* numGlyphs of the face */
	uint32_t n_leaves, n_bytes;    /* n_bytes a multiple of 4 */
	const uint32_t *leaf_off;      /* [n_glyph_ids + 1] glyph id -> its leaves; ascending, leaf_off[0] = 0 */
	const vgsdf_glyf_part *leaves; /* [n_leaves] */
	const uint8_t *bytes;          /* [n_bytes] */
} vgsdf_font_desc;
int vgsdf_font_create(vgsdf_ctx *ctx, const vgsdf_font_desc *in, vgsdf_font **out);
int vgsdf_font_free(vgsdf_ctx *ctx, vgsdf_font *font);
uint64_t vgsdf_font_device_bytes(const vgsdf_font *font);
/* A submission that names its glyphs: glyph g is glyph id glyph_id[g] of fonts[font_of[g]].  A glyph id past the face or a
 * font_of past n_fonts is VGSDF_E_ARG before anything runs; a glyph id without leaves is a glyph without outline (no slots,
 * has_raster = 0); glyph ids may repeat and come in any order.  The host's share is two table reads and two additions per
 * glyph (the running sums of leaves and command slots); it gathers the arrays below into one page-locked block of its own
 *   scale f64[n] | shift_x f64[n] | cmd_off u32[n + 1] | part_off u32[n + 1] | glyph_id u16[n] | font_of u16[n] | pbf_pre u32[n] | pbf_fix u8[n]
 * followed by 32 bytes of device addresses per font, which ONE kernel reads: it copies the per-glyph arrays and expands the
 * leaves into this submission's parts on the device (leaf k of glyph g becomes part part_off[g] + k with
 * cmd_at = cmd_off[g] + leaf.cmd_at).  The decoder then reads every part's bytes from the resident store of its font and the
 * front-end runs on as in the glyf form — the same number of launches.  The caller's arrays need not outlive the call.
 * A malformed entry fails the batch with VGSDF_E_GLYF in vgsdf_outlines_wait, as in the glyf form.  Collected with
 * vgsdf_outlines_wait; _peek, _pbf_positions and _segments work behind it as behind any other form.
 * vgsdf_outlines_resident_upload_bytes: the size of the block the last resident submission of the context uploaded. */
typedef struct {
	uint32_t n_glyphs, n_fonts;
	const vgsdf_font *const *fonts; /* [n_fonts] */
	const uint16_t *font_of;        /* [n_glyphs] index into fonts */
	const uint16_t *glyph_id;       /* [n_glyphs] */
	const double *scale;            /* [n_glyphs] as in vgsdf_outlines_glyf */
	const double *shift_x;          /* [n_glyphs] */
	const uint32_t *pbf_pre;        /* [n_glyphs] or NULL, as in vgsdf_outlines_packed */
	const uint8_t *pbf_fix;         /* [n_glyphs] or NULL */
} vgsdf_outlines_resident;
int vgsdf_outlines_submit_resident(vgsdf_ctx *ctx, const vgsdf_outlines_resident *in, uint8_t *out_bitmaps, size_t out_capacity);
uint64_t vgsdf_outlines_resident_upload_bytes(const vgsdf_ctx *ctx);
/*
 * Command fonts: the resident form for every face whose outlines the caller can read, whatever table they come from (CFF,
 * CFF2, a `glyf` face the decoder refuses).  vgsdf_font_cmds_desc gives, for every glyph id, the callbacks of its outline in
 * the arrays of vgsdf_outlines_packed: glyph id g owns kinds[cmd_off[g] .. cmd_off[g + 1]) and
 * coords[dat_off[g] .. dat_off[g + 1]).  vgsdf_font_create_commands validates on the host everything a packed submission
 * is checked for per render — at most 65536 glyph ids, a store and coordinates that 32-bit offsets address (29 bytes per command + 4 per glyph id, and
 * 4 n_floats, below 2^32), both offset arrays ascending from 0 to n_cmds /
 * n_floats, every kind <= 4, every glyph's dat_off range exactly what its kinds carry (2 floats for a move or a line, 4 for a
 * quad, 6 for a curve, none for a close) — and refuses with VGSDF_E_ARG, nothing left allocated, the context sound.  It then
 * expands the commands ONCE on the device (the context pass of the packed form over the whole face) and keeps the 28-byte
 * records and the byte per command that says whether a ring is open in front of it: 29 bytes per command and 4 per glyph id.
 * The result is a vgsdf_font like any other: vgsdf_font_free and vgsdf_font_device_bytes work on it, it belongs to the
 * context's device, and vgsdf_outlines_submit_resident names it — but ONE submission names fonts of one kind (fonts from
 * vgsdf_font_create and from vgsdf_font_create_commands in one list: VGSDF_E_ARG before anything runs).
 * Against command fonts the host's share per glyph is one table read and one addition (the running sum of command counts;
 * more than 2^31 - 1 commands in one submission: VGSDF_E_ARG); the block is
 *   scale f64[n] | shift_x f64[n] | cmd_off u32[n + 1] | glyph_id u16[n] | font_of u16[n] | pbf_pre u32[n] | pbf_fix u8[n]
 * followed by 32 bytes of device addresses per font, and ONE kernel copies it and gathers every named glyph's records and
 * context bytes from the stores.  No decoder runs and, when every scale is positive and finite, no context pass either: one
 * launch fewer than the packed and the glyf-resident forms.  Output is the packed form's of the same commands, byte for byte.
 * A glyph id without commands is a glyph without outline (no slots, has_raster = 0).
 */
typedef struct {
	uint32_t n_glyph_ids, n_cmds, n_floats;
	const uint32_t *cmd_off; /* [n_glyph_ids + 1] into kinds, ascending, cmd_off[0] = 0, last = n_cmds */
	const uint32_t *dat_off; /* [n_glyph_ids + 1] into coords, likewise, last = n_floats */
	const uint8_t *kinds;    /* [n_cmds] as in vgsdf_outlines_packed */
	const float *coords;     /* [n_floats] */
} vgsdf_font_cmds_desc;
int vgsdf_font_create_commands(vgsdf_ctx *ctx, const vgsdf_font_cmds_desc *in, vgsdf_font **out);
/*
 * Fonts of BOTH kinds in one submission: the same description and the same validation as vgsdf_outlines_submit_resident, except
 * that `fonts` may hold fonts from vgsdf_font_create (and _create_tables) and command fonts in any order; a list of one kind is
 * accepted too.  Every glyph gives, byte for byte, what it gives in a submission of its own kind: rects, segments, bitmaps.
 * The block is the one vgsdf_outlines_submit_resident gathers for glyf fonts,
 *   scale f64[n] | shift_x f64[n] | cmd_off u32[n + 1] | part_off u32[n + 1] | glyph_id u16[n] | font_of u16[n] | pbf_pre u32[n] | pbf_fix u8[n]
 * with cmd_off the running sum of command slots (glyf fonts) and commands (command fonts) over all glyphs, part_off standing
 * still over a glyph of a command font, and 32 bytes of device addresses per font that also say the font's kind.  ONE kernel
 * copies it, expands the leaves of the glyf fonts' glyphs into parts and gathers the records and context bytes of the command
 * fonts' glyphs; the decoder then runs over the parts.  With pbf_pre / pbf_fix the arena is laid out as vgsdf_outlines_packed
 * states it, whatever the kinds.  More than 2^31 - 1 slots and commands together: VGSDF_E_ARG.
 */
int vgsdf_outlines_submit_resident_mixed(vgsdf_ctx *ctx, const vgsdf_outlines_resident *in, uint8_t *out_bitmaps, size_t out_capacity);
/*
 * The same command font made from a `CFF ` (version 1) face's own bytes: the DEVICE interprets the Type 2 charstrings of every
 * glyph id (csrc/charstring_kernels.hip: the operator set and the rules of the host reader, csrc/host/cff.cpp, whose callbacks it
 * equals bit for bit), so the host's share is to locate the INDEX tables and resolve their offsets.  The description:
 *   bytes        every charstring and subroutine body of the face, back to back in any order, padded to a multiple of 4
 *   cs_off       glyph id g's charstring is bytes[cs_off[g] .. cs_off[g + 1]) (an empty range: a glyph without outline)
 *   gsubr_off    global subroutine k is bytes[gsubr_off[k] .. gsubr_off[k + 1])
 *   lsubr_first  Font DICT d owns the local subroutines [lsubr_first[d], lsubr_first[d + 1]) of lsubr_off (lsubr_first[0] = 0;
 *                name-keyed fonts have one Font DICT), subroutine j of it being bytes[lsubr_off[lsubr_first[d] + j] .. the next entry)
 *   fd_of        FDSelect expanded to one byte per glyph id; NULL when n_fds == 1
 * vgsdf_font_create_charstrings validates on the host, before anything runs, every range the device will read: 1 .. 65536 glyph
 * ids, n_bytes a multiple of 4, 1 .. 256 Font DICTs, at most 65535 subroutines per set, every offset array ascending and ending inside
 * `bytes`, every fd_of below n_fds — VGSDF_E_ARG otherwise, nothing left allocated, the context sound.  The device never reads
 * outside a validated range.  It then runs a count pass (commands and coordinates per glyph id), reads the counts back, lays
 * the store out, runs an emit pass that writes kinds | coords on the device, and the context pass of vgsdf_font_create_commands
 * over them: the result is the font vgsdf_font_create_commands makes from the host reader's callbacks of the same face — the same
 * records, cmd_off and context bytes, the same vgsdf_font_device_bytes — and is used and freed like it.  Synchronous like it.
 * Refused with VGSDF_E_GLYF, nothing left allocated, the context sound (the caller then describes the face with its host reader
 * and calls vgsdf_font_create_commands):
 *   - a glyph whose `endchar` takes the seac form (it needs the charset and two further charstrings);
 *   - a glyph that executes more than VGSDF_CHARSTRING_MAX_TOKENS tokens, operands and operators alike (ten nested calls of
 *     fan-out k are k^10 tokens: the bound keeps a crafted font from holding the device; real glyphs stay below a few thousand);
 *   - a store or coordinates past the bounds vgsdf_font_create_commands states.
 * A `CFF2` face goes to vgsdf_font_create_charstrings2 below.
 */
#define VGSDF_CHARSTRING_MAX_TOKENS (1u << 20)
typedef struct {
	uint32_t n_glyph_ids;        /* 1 .. 65536 */
	uint32_t n_bytes;            /* multiple of 4 */
	const uint8_t *bytes;        /* [n_bytes] */
	const uint32_t *cs_off;      /* [n_glyph_ids + 1] */
	uint32_t n_gsubrs;           /* <= 65535 */
	const uint32_t *gsubr_off;   /* [n_gsubrs + 1] */
	uint32_t n_fds;              /* 1 .. 256 */
	const uint32_t *lsubr_first; /* [n_fds + 1] */
	const uint32_t *lsubr_off;   /* [lsubr_first[n_fds] + 1] */
	const uint8_t *fd_of;        /* [n_glyph_ids] or NULL (n_fds == 1) */
} vgsdf_font_charstrings_desc;
int vgsdf_font_create_charstrings(vgsdf_ctx *ctx, const vgsdf_font_charstrings_desc *in, vgsdf_font **out);
/* The same under a limit on the store, for callers that keep a budget of device memory: behind the count pass, and before
 * the store is allocated, *store_bytes (may be NULL) is what the store will hold (29 bytes per command + 4 per glyph id + 4); when
 * that exceeds max_store_bytes the call returns VGSDF_OK with *out = NULL and nothing allocated.  Refusals as above. */
int vgsdf_font_create_charstrings_within(vgsdf_ctx *ctx, const vgsdf_font_charstrings_desc *in, uint64_t max_store_bytes,
                                         vgsdf_font **out, uint64_t *store_bytes);
/*
 * The same for a `CFF2` face: the device interprets its charstrings by the rules of the host reader's CFF2 mode (no width operand,
 * an operand stack of 513, `return` and `endchar` fail the glyph, a glyph ends with its data and its last contour is not closed,
 * `vsindex` and `blend`), and equals its callbacks bit for bit.  The description is the one above with n_fds == 1 and fd_of == NULL
 * (one set of local subroutines serves every glyph) plus the BLEND SETS, one per ItemVariationData of the face's variation store:
 *   n_sets     their count; 0 is legal: no glyph has an outline (set 0 is selected before a glyph's first operator, and a glyph
 *              whose selected set does not exist or is not usable delivers nothing from there on)
 *   set_ok     one byte per set, 0 = not usable
 *   set_off    set s owns factors[set_off[s] .. set_off[s + 1]), one factor per region (set_off[0] = 0)
 *   factors    f32; `blend` adds to each of its values delta x factor for every region, last region first, one product and one
 *              sum per delta in f32
 * The factors are plain data: the entry point neither knows nor checks which position of the design space they stand for (the
 * host reader's are those of the face's position: the default one, or where vg_manager_add_font_instance put it).  Validated on the host before anything runs, VGSDF_E_ARG otherwise: all the
 * above validates, n_fds == 1, fd_of == NULL, at most 65536 sets, set_off ascending from 0 and ending at or below n_factors, at
 * most 64 factors per set, every factor finite.  Count pass, store, emit pass, refusals (no seac form exists in CFF2), budget
 * form, result and vgsdf_font_device_bytes are those of vgsdf_font_create_charstrings.  The passes run in launches of at most
 * 16384 glyph ids; operand slots past the first 48 live in a workspace the CONTEXT owns (at most 465 x 4 x 16384 bytes, grown on
 * demand, freed with the context, not counted by vgsdf_font_device_bytes).
 */
typedef struct {
	vgsdf_font_charstrings_desc charstrings; /* n_fds == 1, fd_of == NULL */
	uint32_t n_sets;                         /* <= 65536 */
	uint32_t n_factors;
	const uint8_t *set_ok;                   /* [n_sets] (may be NULL when n_sets == 0) */
	const uint32_t *set_off;                 /* [n_sets + 1] (may be NULL when n_sets == 0) */
	const float *factors;                    /* [n_factors] (may be NULL when n_factors == 0) */
} vgsdf_font_charstrings2_desc;
int vgsdf_font_create_charstrings2(vgsdf_ctx *ctx, const vgsdf_font_charstrings2_desc *in, vgsdf_font **out);
int vgsdf_font_create_charstrings2_within(vgsdf_ctx *ctx, const vgsdf_font_charstrings2_desc *in, uint64_t max_store_bytes,
                                          vgsdf_font **out, uint64_t *store_bytes);
/* test / inspection (tools/charstrings_ab.py): milliseconds the count and the emit pass of the context's last
 * vgsdf_font_create_charstrings or vgsdf_font_create_charstrings2 took (HIP events around the pass, all its launches; 0 0 before
 * the first, and for a pass that did not run) */
void vgsdf_font_charstrings_kernel_ms(const vgsdf_ctx *ctx, float ms[2]);
/*
 * The same for ONE CFF2 FACE AT MANY POSITIONS in one call — the named instances of a variable file, say.  The description goes
 * up once, with the factors of all positions: face.factors holds n_positions x face.n_factors of them, position after position,
 * each position's laid out by face.set_off.  Both passes run over (glyph id, position) pairs, the lanes of one glyph id at
 * different positions side by side (csrc/charstring_batch_kernels.hip: the single call's device text).  The COUNT pass runs over
 * pairs too: the operand a `callsubr` / `callgsubr` takes as its index, or a `blend` as its count, may itself be blended, so two
 * positions may deliver different numbers of commands; counts, layout and store size are each position's own.  One read-back of
 * all counts and all flag words, the context pass per store, two synchronisations for the whole call.  A launch covers
 * max(1, 16384 / n_positions) glyph ids with all their positions, so the context's workspace grows no further than under the
 * single call.  Each position that is built is a vgsdf_font of its own, with its own store: it cannot be told from what
 * vgsdf_font_create_charstrings2 makes of the same face with that position's factors alone (vgsdf_font_commands_read,
 * vgsdf_font_device_bytes), and is read, named by submissions and families, and freed like it, each alone (the same position
 * given twice: two fonts).  Per position p:
 *   built                                      status[p] VGSDF_OK      out[p] the font
 *   over the limit (_within)                   status[p] VGSDF_OK      out[p] NULL, needed[p] its store's bytes
 *   refused: a glyph past VGSDF_CHARSTRING_MAX_TOKENS AT p, or a store past the command store's bounds AT p
 *                                              status[p] VGSDF_E_GLYF  out[p] NULL, no room taken, the other positions untouched
 * _within takes the positions in order: one that is not refused is built when its store fits into what the positions built
 * before it have left of max_store_bytes; one that does not fit is passed over and does not stop those behind it.  needed (may
 * be NULL): [n_positions], 0 for a refused position.
 * The whole call fails with VGSDF_E_ARG, before anything runs and with nothing allocated, for a NULL argument, more than
 * VGSDF_CHARSTRING2_MAX_POSITIONS positions, anything vgsdf_font_create_charstrings2 validates, or a factor of any position
 * that is not finite; a HIP error or an exhausted host fails it too: nothing is left allocated, every out[p] is NULL and the
 * context stays sound.  n_positions == 0: VGSDF_OK, nothing is touched.
 */
#define VGSDF_CHARSTRING2_MAX_POSITIONS 64u
typedef struct {
	vgsdf_font_charstrings2_desc face; /* face.factors: [n_positions * face.n_factors], position after position */
	uint32_t n_positions;              /* 0 .. VGSDF_CHARSTRING2_MAX_POSITIONS */
} vgsdf_fonts_charstrings2_desc;
int vgsdf_fonts_create_charstrings2(vgsdf_ctx *ctx, const vgsdf_fonts_charstrings2_desc *in, vgsdf_font **out /* [n_positions] */,
                                    int *status /* [n_positions] */);
int vgsdf_fonts_create_charstrings2_within(vgsdf_ctx *ctx, const vgsdf_fonts_charstrings2_desc *in, uint64_t max_store_bytes,
                                           vgsdf_font **out, int *status, uint64_t *needed /* [n_positions], may be NULL */);
/* test / inspection (tools/charstrings2_batch_ab.py): the count and the emit pass of the context's last
 * vgsdf_fonts_create_charstrings2 */
void vgsdf_fonts_charstrings2_kernel_ms(const vgsdf_ctx *ctx, float ms[2]);
/* test / inspection: download a command font's store.  *n_glyph_ids / *n_cmds: its counts (either may be NULL); cmd_off
 * [n_glyph_ids + 1], records [28 * n_cmds bytes: x1 y1 x2 y2 x y as f32, kind as u32], context [n_cmds]: each NULL or filled.
 * A font from vgsdf_font_create: VGSDF_E_ARG. */
int vgsdf_font_commands_read(vgsdf_ctx *ctx, const vgsdf_font *font, uint32_t *n_glyph_ids, uint32_t *n_cmds, uint32_t *cmd_off,
                             void *records, uint8_t *context);
/*
 * A `glyf` face's resident font built on the DEVICE from its `loca` and `glyf` tables: the host says where the tables are and
 * looks at no glyph.  One lane per glyph id walks the glyph's component tree by the rules of the host reader (ttf-parser 0.25:
 * the loca rules of both formats, a child that does not resolve is skipped, anchor-point arguments are not consumed, a
 * truncated record ends its composite, a depth of 32 fails the glyph and keeps the leaves delivered so far, transforms composed
 * in f32); a count pass sizes the arrays, the host lays them out, an emit pass writes them.  The result is the font
 * vgsdf_font_create makes of
 *   leaves    the host reader's, in its order; byte_off = byte_at[the simple glyph's id]
 *   bytes     in GLYPH-ID order: for every glyph id whose own entry is a simple glyph of more than one point, its
 *             endPtsOfContours followed by the bytes from behind its instructions to the end of the entry (nothing for an entry
 *             whose two ranges pass 32 KB: byte_len 0), zero-padded to a multiple of 4; byte_at is the running sum
 * and is used and freed like it.  Validated on the host, VGSDF_E_ARG, nothing allocated: a NULL argument (a table of length 0
 * may be NULL), num_glyphs > 65535, loca_long > 1, loca_entries past what the loca bytes hold or past num_glyphs + 1 (a component could
 * otherwise resolve to a glyph id the font has no place for).  Refused with VGSDF_E_GLYF,
 * nothing left allocated, the context sound (the caller then describes the face with its host reader and calls
 * vgsdf_font_create): a glyph id that reads more than 2^20 component records (a record counts when its four leading bytes have
 * been read; the library's VGSDF_GLYF_MAX_COMPONENTS), more than 2^22 leaves, a glyph id of more than 2^26 command slots, a store past 2^32 - 4 bytes, command slots that sum past 2^32 - 1.
 * _within: the budget form of vgsdf_font_create_charstrings_within; *needed is leaves + bytes + 4 per glyph id.
 */
typedef struct {
	uint32_t num_glyphs;                 /* maxp */
	uint32_t loca_entries;               /* min(num_glyphs + 1 (0xFFFF when num_glyphs == 0xFFFF), loca bytes / entry size) */
	uint32_t loca_long;                  /* 0 or 1 */
	uint32_t n_loca_bytes, n_glyf_bytes;
	const uint8_t *loca, *glyf;          /* the whole tables as they stand in the file */
} vgsdf_font_tables_desc;
int vgsdf_font_create_tables(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *in, vgsdf_font **out);
int vgsdf_font_create_tables_within(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                    uint64_t *needed);
/* test / inspection: download a glyf-kind font's store, whichever call made it.  *n_glyph_ids / *n_leaves / *n_bytes: its counts
 * (each may be NULL); leaf_off [n_glyph_ids + 1], leaves [n_leaves], bytes [n_bytes]: each NULL or filled.  A command font:
 * VGSDF_E_ARG. */
int vgsdf_font_read(vgsdf_ctx *ctx, const vgsdf_font *font, uint32_t *n_glyph_ids, uint32_t *n_leaves, uint32_t *n_bytes,
                    uint32_t *leaf_off, vgsdf_glyf_part *leaves, uint8_t *bytes);
/* test / inspection (tools/glyf_tables_ab.py): milliseconds the count pass and the emit pass (with its copy of the bytes) of the
 * context's last vgsdf_font_create_tables took (HIP events around the pass; 0 0 before the first, and for a pass that did not run) */
void vgsdf_font_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2]);
/*
 * The same for ALL FACES OF A FONT ID in one call: one count launch, one read-back, one emit launch, so that what a call costs
 * beside its two passes (its synchronisations, events, scratch allocation) is paid once and not once per face.  Each face that
 * is built is a vgsdf_font of its own, with its own store: it cannot be told from what vgsdf_font_create_tables makes of that
 * face alone, and is read, named by submissions and families, and freed like it, each alone.  Per face f:
 *   built                                      status[f] VGSDF_OK      out[f] the font
 *   over the limit (_within)                   status[f] VGSDF_OK      out[f] NULL, needed[f] its store's bytes
 *   badly described (the single call's VGSDF_E_ARG conditions)   status[f] VGSDF_E_ARG   out[f] NULL
 *   refused (its VGSDF_E_GLYF conditions)      status[f] VGSDF_E_GLYF  out[f] NULL
 * and a bad or refused face leaves the others untouched.  _within takes the faces in order: a face is built when its store fits
 * into what the faces built before it have left of max_store_bytes; one that does not fit is passed over and does not stop the
 * faces behind it.  needed (may be NULL): [n_faces], 0 for a face that was badly described or refused.
 * The whole call fails with VGSDF_E_ARG, before anything runs, for a NULL argument, more than 65536 faces or well-described
 * faces of more than 2^22 glyph ids together; a HIP error or an exhausted host fails it too: nothing is left allocated, every
 * out[f] is NULL and the context stays sound.  n_faces == 0: VGSDF_OK, nothing is touched.
 */
int vgsdf_fonts_create_tables(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *faces, uint32_t n_faces, vgsdf_font **out /* [n_faces] */,
                              int *status /* [n_faces] */);
int vgsdf_fonts_create_tables_within(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *faces, uint32_t n_faces, uint64_t max_store_bytes,
                                     vgsdf_font **out, int *status, uint64_t *needed /* [n_faces], may be NULL */);
/* test / inspection (tools/glyf_tables_ab.py): the count and the emit pass of the context's last vgsdf_fonts_create_tables */
void vgsdf_fonts_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2]);
/*
 * The command font of a `glyf` face PLACED BY `gvar` at a position of its design space, built on the DEVICE from the face's
 * `loca`, `glyf` and `gvar` tables: the host says where the tables are and looks at no glyph.  The description: the tables of
 * vgsdf_font_tables_desc, the whole `gvar` table, and the position as n_axes normalised coordinates (F2Dot14 as int16, behind
 * `avar`).  Validated on the host, VGSDF_E_ARG, nothing allocated: what vgsdf_font_create_tables validates; 1 .. 64 axes; a
 * `gvar` that is not version 1.0, whose axisCount is not n_axes, or whose header, shared tuples or offset array leave gvar_len.
 * Three passes, one lane per glyph id (csrc/gvar_kernels.hip), every read bounded by the table lengths:
 *   count   the points of the glyph id's own entry, and over its component tree the commands and coordinates it delivers
 *   deltas  rules G1 to G6 of the host reader (csrc/host/ttf_face.hpp) over the own entry: per point the f32 sums of its tuples
 *   emit    the tree again: component offsets take the composite's sums, a leaf's points those of the leaf's glyph id
 * and the context pass of vgsdf_font_create_commands over the result, which is the font that call makes of the host reader's
 * command table of the same face at the same position — the same records, cmd_off and context bytes, the same
 * vgsdf_font_device_bytes — used and freed like it.  Synchronous like it.  The deltas pass works in a scratch the CONTEXT owns
 * (13 bytes per point of a launch; launches of at most 2^17 points, or one glyph id; grown on demand, freed with the context, not
 * counted by vgsdf_font_device_bytes).  Refused with VGSDF_E_GLYF, nothing left allocated, the context sound (the caller then
 * takes the host reader's table to vgsdf_font_create_commands):
 *   - a glyph id whose variation data is malformed (the host reader delivers nothing for it from there on);
 *   - a glyph id whose own entry has more than VGSDF_GVAR_MAX_DELTAS tuples x points (phantom points included), whatever the
 *     tuples' scalars: one lane works through them, and the bound keeps a crafted table from holding the device;
 *   - a glyph id that reads more than 2^20 component records, or a composite entry of more than 65535; a glyph id of more than 2^26
 *     commands;
 *   - a store or coordinates past the bounds vgsdf_font_create_commands states.
 * _within: the budget form of vgsdf_font_create_charstrings_within.
 */
#define VGSDF_GVAR_MAX_DELTAS (1u << 20)
typedef struct {
	vgsdf_font_tables_desc tables; /* loca, glyf */
	const uint8_t *gvar;           /* the whole table as it stands in the file */
	uint32_t gvar_len;
	uint32_t n_axes;               /* 1 .. 64, the table's axisCount */
	const int16_t *coords;         /* [n_axes] */
} vgsdf_font_gvar_desc;
int vgsdf_font_create_gvar(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *in, vgsdf_font **out);
int vgsdf_font_create_gvar_within(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                  uint64_t *store_bytes);
/* test / inspection (tools/gvar_instances_ab.py): milliseconds the count, the deltas and the emit pass of the context's last
 * vgsdf_font_create_gvar took (HIP events around the pass, all its launches; 0 before the first, and for a pass that did not run) */
void vgsdf_font_gvar_kernel_ms(const vgsdf_ctx *ctx, float ms[3]);
/*
 * The same for ONE FACE AT MANY POSITIONS in one call — the named instances of a variable file, say.  The tables are uploaded
 * once; the count pass (it looks at no coordinate), its read-back and the layout are done once and serve every position, whose
 * stores all have the same sizes; the deltas pass and the emit pass run over (glyph id, position) pairs, the lanes of one glyph
 * id at different positions side by side (csrc/gvar_batch_kernels.hip: the single call's device text); the context pass runs
 * per store; three synchronisations for the whole call.  The deltas pass's launches cover glyph ids x positions of at most 2^17
 * points x positions (or one glyph id at one position), so the context's scratch grows no further than under the single call.
 * coords: n_positions x n_axes, position after position.  Each position that is built is a vgsdf_font of its own, with its own
 * store: it cannot be told from what vgsdf_font_create_gvar makes of the same tables at that position alone, and is read, named
 * by submissions and families, and freed like it, each alone (the same position given twice: two fonts).  Per position p:
 *   built                                      status[p] VGSDF_OK      out[p] the font
 *   over the limit (_within)                   status[p] VGSDF_OK      out[p] NULL, needed[p] its store's bytes
 *   refused where the position decides: a glyph id whose variation data is malformed AT p (a tuple of scalar 0 is not read)
 *                                              status[p] VGSDF_E_GLYF  out[p] NULL, the other positions untouched
 *   refused whatever the position: the single call's other VGSDF_E_GLYF conditions — component records, a composite of more
 *   than 65535, 2^26 commands, the store's bounds, and VGSDF_GVAR_MAX_DELTAS (tuples x points, whatever the scalars)
 *                                              status[p] VGSDF_E_GLYF at every p (the call itself returns VGSDF_OK)
 * _within takes the positions in order: one that is not refused is built when its store fits into what the positions built
 * before it have left of max_store_bytes; one that does not fit is passed over and does not stop those behind it.  needed (may
 * be NULL): [n_positions], 0 for a refused position.  When not even one store fits, no position is looked at (needed[p] is set,
 * status[p] VGSDF_OK), as the single call returns before its deltas pass.
 * The whole call fails with VGSDF_E_ARG, before anything runs, for a NULL argument, more than VGSDF_GVAR_MAX_POSITIONS
 * positions or anything vgsdf_font_create_gvar validates; a HIP error or an exhausted host fails it too: nothing is left
 * allocated, every out[p] is NULL and the context stays sound.  n_positions == 0: VGSDF_OK, nothing is touched.
 */
#define VGSDF_GVAR_MAX_POSITIONS 64u
typedef struct {
	vgsdf_font_tables_desc tables; /* loca, glyf */
	const uint8_t *gvar;           /* the whole table as it stands in the file */
	uint32_t gvar_len;
	uint32_t n_axes;               /* 1 .. 64, the table's axisCount */
	const int16_t *coords;         /* [n_positions * n_axes], normalised, behind avar */
	uint32_t n_positions;          /* 0 .. VGSDF_GVAR_MAX_POSITIONS */
} vgsdf_fonts_gvar_desc;
int vgsdf_fonts_create_gvar(vgsdf_ctx *ctx, const vgsdf_fonts_gvar_desc *in, vgsdf_font **out /* [n_positions] */,
                            int *status /* [n_positions] */);
int vgsdf_fonts_create_gvar_within(vgsdf_ctx *ctx, const vgsdf_fonts_gvar_desc *in, uint64_t max_store_bytes, vgsdf_font **out, int *status,
                                   uint64_t *needed /* [n_positions], may be NULL */);
/* test / inspection (tools/gvar_batch_ab.py): the count, the deltas and the emit pass of the context's last vgsdf_fonts_create_gvar */
void vgsdf_fonts_gvar_kernel_ms(const vgsdf_ctx *ctx, float ms[3]);
/*
 * The PHANTOM PASS (csrc/gvar_advance_kernels.hip): what the advances of a placed `glyf` face whose file has no `HVAR` take from
 * `gvar`, rule G7 of csrc/host/ttf_face.hpp, computed on the device from the description vgsdf_font_create_gvar takes.  One lane
 * per glyph id, one pass, no scratch: the lane reads the point count n of its glyph id's OWN entry (a simple entry's last end
 * point + 1, a composite's component records, 0 for a glyph id without an entry or with an entry of no contours) and streams the
 * glyph id's tuples, taking from every applied one the x deltas of the phantom points n (l) and n + 1 (r) — += f32(delta) *
 * scalar each, in tuple order — while walking its point numbers and all 2 x count of its deltas to their end.  delta[g] = r - l
 * in f32, and state[g]: 0, no variation data (a glyph id at or past glyphCount, an empty range, tuple count 0; delta 0);
 * 1, a delta; 2, malformed — the entry (its count cannot be read) or the data, by the meaning the outline's rules G1 to G5 give
 * the word at that position (delta 0: the `hmtx` advance stands).  Both arrays hold tables.num_glyphs elements and equal, bit for
 * bit, what the host reader gives (vg_manager_font_gvar_advance_deltas of vgfont.h).  Every read is bounded by loca_entries,
 * n_glyf_bytes and gvar_len.  Test / inspection: the pass alone, read back.  Synchronous; nothing stays allocated.
 * Validated on the host as vgsdf_font_create_gvar validates its description (VGSDF_E_ARG).  Refused with VGSDF_E_GLYF, delta and
 * state untouched, the context sound: a glyph id of more than VGSDF_GVAR_MAX_DELTAS tuples x (n + 4), whatever the scalars —
 * refused by the count, its tuples are not walked.
 */
int vgsdf_gvar_advance_deltas(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *in, float *delta /* [num_glyphs] */, uint8_t *state /* [num_glyphs] */);
/* test / inspection (tools/gvar_advances_ab.py): milliseconds the phantom pass of the context's last vgsdf_gvar_advance_deltas or
 * vgsdf_family_create_tables_gvar took (HIP events around the pass, summed over the faces it ran for; 0 before the first, and
 * when it did not run) */
float vgsdf_gvar_advance_kernel_ms(const vgsdf_ctx *ctx);
/*
 * Resident families: the table code point -> (font, glyph id, advance, scale, shift_x) of a font id lives on the device
 * beside its fonts, and a submission names CODE-POINT RANGES of families instead of glyphs.  The host's share per submission
 * is O(tasks): the block it uploads holds 32 bytes per task that maps a glyph, per family and per font, and no per-glyph byte.
 *
 * vgsdf_family_create validates the description on the host (code points strictly ascending, font_of < n_fonts, every glyph id
 * inside its face, every font on the context's device and of ONE kind; VGSDF_E_ARG otherwise, nothing left allocated, the
 * context sound), keeps per entry its fields, pbf_fix (from code point and advance, as vgsdf_outlines_packed states it) and the
 * prefix sums over the entries of the glyphs' command slots (glyf fonts: and of their leaves), copies the table to the device and
 * returns when it is there.  A family owns no font: the fonts must outlive it.  vgsdf_family_free follows the timing rule of
 * vgsdf_font_free.  vgsdf_family_count: the mapped code points in [first, last].
 */
typedef struct vgsdf_family vgsdf_family;
typedef struct {
	uint32_t n_fonts;               /* 1 .. 65536 */
	const vgsdf_font *const *fonts; /* one device, ONE kind (all from vgsdf_font_create or all from _create_commands) */
	uint32_t n_entries;             /* mapped code points, <= 65536 */
	const uint16_t *code_point;     /* [n_entries] strictly ascending */
	const uint16_t *font_of;        /* [n_entries] index into fonts */
	const uint16_t *glyph_id;       /* [n_entries] */
	const uint32_t *advance;        /* [n_entries] PbfGlyph.advance */
	const double *scale, *shift_x;  /* [n_entries] as in vgsdf_outlines_resident */
} vgsdf_family_desc;
int vgsdf_family_create(vgsdf_ctx *ctx, const vgsdf_family_desc *in, vgsdf_family **out);
int vgsdf_family_free(vgsdf_ctx *ctx, vgsdf_family *family);
uint64_t vgsdf_family_device_bytes(const vgsdf_family *family);
uint32_t vgsdf_family_count(const vgsdf_family *family, uint32_t first, uint32_t last);
/* The same description with fonts of EITHER kind in `fonts`.  The family is of a third kind, MIXED, even when its fonts happen to
 * be of one kind: the prefix sum of command slots runs over every font's glyphs (slots of a glyf font, commands of a command
 * font), the prefix sum of leaves over the glyf fonts' and stands still over an entry of a command font.  vgsdf_family_free,
 * _device_bytes, _count and _read work on it as on any family. */
int vgsdf_family_create_mixed(vgsdf_ctx *ctx, const vgsdf_family_desc *in, vgsdf_family **out);
/*
 * The same family from its faces' `cmap` and `hmtx` TABLES: no code point is looked up on the host.  The host says where the
 * unicode subtables are (vg_manager_family_tables_desc of vgfont.h builds such a description), the device looks every code point
 * of [0, 0xFFFF] outside the surrogates up in the faces in order and writes the table in place: a count pass sizes it, an
 * emit pass places every entry at its rank.  A face MAPS a code point when one of its subtables enumerates it and that
 * subtable's lookup has a value; the entry belongs to the first face that maps it, its glyph id is the first value any of
 * that face's subtables has, and advance, scale and shift_x are those of the packed form's recorder in f64:
 * scale = 24 / units_per_em, advance = round(hmtx advance * scale * 0.95), shift_x = (advance - that product) / 2.  The lookups
 * are bounded by cmap_len / hmtx_len throughout, whatever the tables' own length fields say.
 * Validated on the host (VGSDF_E_ARG): pointers that are NULL beside a length that is not 0, subtable_off < cmap_len, formats
 * from the list, units_per_em in 16 .. 16384, fonts on the context's device and of one kind.  A glyph id at or past its font's
 * glyph ids is found by the count pass: VGSDF_E_ARG, nothing left allocated, the context sound.  The family is
 * indistinguishable from one vgsdf_family_create makes of the same entries.
 */
typedef struct { /* one face, as vg_manager_family_tables_desc states it */
	const uint8_t *cmap;
	uint32_t cmap_len;
	const uint8_t *hmtx;
	uint32_t hmtx_len;
	uint16_t units_per_em, num_glyphs, num_hmetrics, n_subtables;
	const uint32_t *subtable_off;    /* [n_subtables] into cmap */
	const uint16_t *subtable_format; /* [n_subtables] 0 4 6 10 12 13 */
} vgsdf_face_tables;
typedef struct {
	uint32_t n_fonts;                /* 1 .. 65536, provider order: the first face that maps a code point wins */
	const vgsdf_font *const *fonts;  /* one device, one kind */
	const vgsdf_face_tables *tables; /* [n_fonts] */
} vgsdf_family_tables_desc;
int vgsdf_family_create_tables(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, vgsdf_family **out);
/* The same with fonts of either kind: a mixed family, indistinguishable from one vgsdf_family_create_mixed makes of the same
 * entries.  (vgsdf_family_tables_kernel_ms reports its passes as well.) */
int vgsdf_family_create_tables_mixed(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, vgsdf_family **out);
/*
 * A family belongs to a PLANE p, 0 .. 16: its 16-bit code_point entries, and the first / last of a task that names it, are the
 * low halves of (p << 16) | x.  Every constructor above and below makes plane 0; these two make any plane, and plane 0 through
 * them is the family the old entry point makes.  `kind` chooses what the pair of constructors chooses: VGSDF_FAMILY_ONE_KIND
 * (vgsdf_family_create / _create_tables) or VGSDF_FAMILY_MIXED (_create_mixed / _create_tables_mixed); validation is theirs, and a
 * plane above 16 or another kind is VGSDF_E_ARG.  pbf_fix counts the varint of the FULL code point (3 bytes in planes 1 .. 16), and
 * the device writes the full value as the id of an entry's PBF bytes.  vgsdf_family_create_at takes any face, placed ones included
 * (the host states the advances).  vgsdf_family_create_tables_at is the device build over the code points (p << 16) + 0 .. 0xFFFF
 * with the surrogates taken from the full value — static faces only — and its result is indistinguishable from
 * vgsdf_family_create_at of the same entries (vgsdf_family_read).  The lookup answers any code point: a format 0, 4 or 6 subtable
 * has nothing above 0xFFFF, formats 10, 12 and 13 are followed, a format 12 group whose id + (c - start) passes 0xFFFF has no
 * value from there on.  One vgsdf_outlines_submit_ranges may name families of different planes (of one kind, as ever); its
 * output is that of vgsdf_outlines_submit_resident of the sequence with pbf_fix from the full ids.  vgsdf_family_count keeps its
 * meaning on low halves; vgsdf_family_plane reads the plane back (0 for NULL).
 */
#define VGSDF_FAMILY_ONE_KIND 0
#define VGSDF_FAMILY_MIXED 1
int vgsdf_family_create_at(vgsdf_ctx *ctx, const vgsdf_family_desc *in, int kind, uint32_t plane, vgsdf_family **out);
int vgsdf_family_create_tables_at(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, int kind, uint32_t plane, vgsdf_family **out);
uint32_t vgsdf_family_plane(const vgsdf_family *family);
/*
 * Which planes are worth a family: a CENSUS of the faces' cmap tables on the device, for the caller of
 * vgsdf_family_create_tables_at, who has not parsed cmap.  bits is a bitmap over the 4352 blocks [256 b, 256 b + 255] up to
 * 0x10FFFF, bit b at bits[b / 32] >> (b % 32).  Bit b is set exactly when some face's subtable of the description LISTS a code
 * point c of the block that is no surrogate and at most 0x10FFFF, where a subtable lists
 *   format 0: c < 256, when the table has its 262 bytes;   format 4: its segments [start, end], less a closing segment
 *   0xFFFF - 0xFFFF;   formats 6 and 10: [first, first + count - 1];   formats 12 and 13: its groups.
 * A span that ends past 0x10FFFF is cut there; a span that straddles the surrogates sets what lies on either side of them.  A
 * listed code point may have no value, so the census is a SUPERSET of the blocks that map something: it promises only that a
 * clear bit maps nothing (on the regular tables vg_manager_family_tables_desc describes).  One workgroup per subtable, its lanes
 * over the segments / groups, each ORing its span into the bitmap with atomics, whole words where the span covers them
 * (csrc/family_census_kernels.hip); every read is bounded by cmap_len.  The tables are validated as vgsdf_family_create_tables
 * validates them (VGSDF_E_ARG, bits untouched, the context sound); the description's fonts are not looked at and may be NULL.
 * vgsdf_family_census_kernel_ms: milliseconds the kernel of the context's last census took (HIP events; 0 before the first).
 */
#define VGSDF_CENSUS_WORDS 136u
int vgsdf_family_tables_census(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, uint32_t bits[VGSDF_CENSUS_WORDS]);
float vgsdf_family_census_kernel_ms(const vgsdf_ctx *ctx);
/*
 * The same with faces AT A POSITION of their design space, whose advances follow `HVAR` (vg_manager_add_font_instance of
 * vgfont.h): var[k] beside tables[k] says where face k's HVAR is and what factor every region of its ItemVariationStore has at
 * the face's position (the host evaluates the regions, once; the device takes the factors as data, as the CFF2 decoder takes
 * its own).  A record with hvar NULL and hvar_len 0 is a static face; var NULL: every face is (the call is then
 * vgsdf_family_create_tables).  A family may mix both.  Where the emit pass has a glyph's `hmtx` advance it adds, in f32,
 * what the host's reader adds (Face::glyph_hor_advance of a face at a position):
 *   (outer, inner) = the advance map's entry of min(glyph id, mapCount - 1) (DeltaSetIndexMap format 0 or 1, entry size
 *   ((entryFormat >> 4) & 3) + 1 bytes, inner bits (entryFormat & 15) + 1), or (0, glyph id) without a map (map_off 0);
 *   delta = sum over the columns of row `inner` of ItemVariationData[outer] of delta * factor(regionIndex), one f32 product and
 *   one f32 sum per column in column order, the first wordDeltaCount columns i16 and the rest i8, a region index at or past
 *   n_regions with factor 0;  advance = trunc((f32)hmtx advance + delta + 0.5), 0 when that leaves 0 .. 65535.
 * No delta — the `hmtx` advance stands — for a map without entries or of another format, outer past the store's list, inner at
 * or past itemCount, more word deltas than columns, and whenever a byte of the walk would lie at or past hvar_len: every read is
 * bounded by hvar_len, whatever the table's own fields say.  Everything else is as in vgsdf_family_create_tables; the count
 * pass is the same.  Validated on the host in addition (VGSDF_E_ARG, nothing left allocated, the context sound): hvar NULL
 * beside a length, region_scalars NULL beside n_regions, store_off + 8 past hvar_len, map_off at or past hvar_len, a store
 * whose format is not 1, an ItemVariationData (its header inside the table) with the LONG_WORDS bit, a factor that is not finite.
 * The family is indistinguishable from one vgsdf_family_create makes of the same entries with the reader's advances.
 */
typedef struct { /* one face's variation, as vg_manager_family_variation_desc states it */
	const uint8_t *hvar;         /* the whole table as it stands in the file; NULL: a static face */
	uint32_t hvar_len;
	uint32_t store_off, map_off; /* into hvar: the ItemVariationStore, the advance-width map (0: none) */
	const float *region_scalars; /* [n_regions] */
	uint32_t n_regions;
} vgsdf_face_variation;
int vgsdf_family_create_tables_var(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var /* [n_fonts] or NULL */,
                                   vgsdf_family **out);
int vgsdf_family_create_tables_var_mixed(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var,
                                         vgsdf_family **out);
/*
 * The same with placed `glyf` faces whose file has NO `HVAR` and whose advances follow gvar's phantom points instead (rule G7 of
 * csrc/host/ttf_face.hpp; vg_manager_set_gvar_advances of vgfont.h): gvar is [n_fonts] pointers, gvar[k] the description
 * vgsdf_font_create_gvar takes of face k (vg_manager_family_gvar_desc states it), or NULL for a face that takes nothing from
 * gvar.  gvar NULL: the call is vgsdf_family_create_tables_var.  For face k with gvar[k] and without var[k].hvar (var may be NULL)
 * the call uploads the three tables and runs the PHANTOM PASS (vgsdf_gvar_advance_deltas above: the same pass) into an array the
 * CONTEXT owns (5 bytes per glyph id; grown on demand, freed with the context, counted by no family); where the emit pass has a
 * glyph's `hmtx` advance of such a face it adds, unless the glyph id's state is "malformed" or the glyph id lies at or past the
 * description's num_glyphs, the pass's delta where the `HVAR` form adds HVAR's:  advance = trunc((f32)hmtx advance + (delta +
 * 0.5)), 0 when that leaves 0 .. 65535.  A face with both descriptions uses its HVAR, as the host's reader does; its gvar
 * description is validated and otherwise not looked at.  Validated on the host in addition (VGSDF_E_ARG): every gvar[k] as
 * vgsdf_font_create_gvar validates its description.  Refused with VGSDF_E_GLYF, nothing left allocated, the context sound: a
 * glyph id past VGSDF_GVAR_MAX_DELTAS (tuples x (points + 4)) in a face the pass runs over.  The count pass and everything else
 * are vgsdf_family_create_tables'; the family is indistinguishable from one vgsdf_family_create makes of the same entries with
 * the reader's advances.  Existing structs and entry points are as they were.
 */
int vgsdf_family_create_tables_gvar(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var /* [n_fonts] or NULL */,
                                    const vgsdf_font_gvar_desc *const *gvar /* [n_fonts] or NULL */, vgsdf_family **out);
int vgsdf_family_create_tables_gvar_mixed(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var,
                                          const vgsdf_font_gvar_desc *const *gvar, vgsdf_family **out);
/* test / inspection: download the DEVICE's copy of a family's table, whichever call made it; *n_entries: its entries; code_point,
 * font_of, glyph_id, advance, scale, shift_x, pbf_fix [n_entries], cmd_pre, leaf_pre [n_entries + 1] (mod 2^32): each NULL or filled */
int vgsdf_family_read(vgsdf_ctx *ctx, const vgsdf_family *family, uint32_t *n_entries, uint16_t *code_point, uint16_t *font_of,
                      uint16_t *glyph_id, uint32_t *advance, double *scale, double *shift_x, uint32_t *cmd_pre, uint32_t *leaf_pre,
                      uint8_t *pbf_fix);
/* test / inspection (tools/family_tables_ab.py): milliseconds the count and the emit pass of the context's last
 * vgsdf_family_create_tables took (HIP events around the pass; 0 0 before the first, and for a pass that did not run) */
void vgsdf_family_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2]);
/*
 * The family tables of ONE FACE AT MANY POSITIONS in one call — the named instances of a variable file, whose stores
 * vgsdf_fonts_create_gvar (or vgsdf_fonts_create_charstrings2 for a CFF2 file) has made.  Position p is a family of one face over
 * fonts[p]: `tables` is the one face's cmap and hmtx, var[p] its HVAR with the region factors of position p (every record names
 * the same hvar, hvar_len, store_off, map_off and n_regions: one file has one HVAR or none), gvar the description
 * vgsdf_fonts_create_gvar takes, with the coordinates of all positions.  What runs once for the call: the tables' upload; the
 * PHANTOM PASS — only with gvar given and no HVAR described, HVAR wins as in the single call — over (glyph id, position) pairs,
 * pair index glyph id x n_positions + position, a lane doing for its pair what a lane of vgsdf_gvar_advance_deltas does for its
 * glyph id (csrc/gvar_advance_batch_kernels.hip: the same device text), into the context's array (now 5 bytes per glyph id AND
 * position, grown on demand, freed with the context); the count pass, its read-back, the layout and the emit pass, each over a
 * second grid dimension, the position (csrc/family_table_kernels.hip: the single call's text).  Counts are taken per position:
 * the command-slot sums come from font p, and the call does not assume the fonts are alike.
 * out[p] is a family of its own, freed alone: its vgsdf_family_read arrays, vgsdf_family_device_bytes and vgsdf_family_count
 * cannot be told from what vgsdf_family_create_tables_gvar (_mixed: _gvar_mixed) makes of the one face with fonts[p], var[p]
 * and the single description at position p.  The same position given twice: two families.
 *   VGSDF_E_ARG before anything runs, nothing allocated: a NULL argument, more than VGSDF_FAMILY_MAX_POSITIONS positions,
 *     anything the single calls validate, var records that do not name one HVAR, gvar->n_positions other than n_positions.
 *   VGSDF_E_GLYF for the whole call, every out[p] NULL, the context sound: a glyph id past VGSDF_GVAR_MAX_DELTAS (the count
 *     decides before a tuple is walked, whatever the position).
 *   status[p] VGSDF_E_ARG, out[p] NULL, the other positions built: a code point that maps to a glyph id at or past font p's.
 *   A HIP error or an exhausted host fails the whole call: nothing left allocated, every out[p] NULL, the context sound.
 *   n_positions == 0: VGSDF_OK, nothing is touched.
 */
#define VGSDF_FAMILY_MAX_POSITIONS 64u
typedef struct {
	uint32_t n_positions;              /* 0 .. VGSDF_FAMILY_MAX_POSITIONS */
	const vgsdf_font *const *fonts;    /* [n_positions]: the face's font at position p; one device, one kind */
	vgsdf_face_tables tables;          /* the ONE face */
	const vgsdf_face_variation *var;   /* [n_positions] or NULL; region_scalars differ per position */
	const vgsdf_fonts_gvar_desc *gvar; /* or NULL; its n_positions must equal n_positions above */
} vgsdf_families_tables_desc;
int vgsdf_families_create_tables(vgsdf_ctx *ctx, const vgsdf_families_tables_desc *in, vgsdf_family **out /* [n_positions] */,
                                 int *status /* [n_positions] */);
int vgsdf_families_create_tables_mixed(vgsdf_ctx *ctx, const vgsdf_families_tables_desc *in, vgsdf_family **out, int *status);
/* test / inspection: the batched phantom pass alone, read back.  delta, state: [n_positions * num_glyphs] each, position after
 * position; bit for bit what vgsdf_gvar_advance_deltas gives at each position.  Validation and VGSDF_E_GLYF as there; more than
 * VGSDF_FAMILY_MAX_POSITIONS positions: VGSDF_E_ARG; none: VGSDF_OK, nothing touched. */
int vgsdf_gvar_advance_deltas_batch(vgsdf_ctx *ctx, const vgsdf_fonts_gvar_desc *in, float *delta, uint8_t *state);
/* test / inspection (tools/family_batch_ab.py): milliseconds the phantom, the count and the emit pass of the context's last
 * vgsdf_families_create_tables took (0 for a pass that did not run; vgsdf_gvar_advance_deltas_batch sets [0] alone) */
void vgsdf_families_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[3]);
/*
 * The glyph sequence of a ranges submission: the tasks in order, and inside a task the mapped code points of
 * [first, last] of its family, ascending.  The output is, byte for byte, that of vgsdf_outlines_submit_resident given that
 * sequence with the families' fonts, the entries' scale and shift_x, pbf_pre[g] = the task's value on its first glyph and 0
 * elsewhere, and pbf_fix[g] from the entries' code points (the ids) and advances: rects, segments, bitmaps and
 * vgsdf_outlines_pbf_positions alike.  With pbf_pre NULL the bitmaps are packed back to back.  With pbf_pre given the device
 * also WRITES every glyph's entry bytes around its bitmap (0x1A varint(len) 0x08 varint(id) [0x12 varint(w h)] in front,
 * 0x18 width 0x20 height 0x28 left 0x30 top 0x38 advance behind), wherever the raster stores the bitmaps, so the arena comes
 * back as finished entries; only the bytes a task reserved with pbf_pre are left for the caller.
 * Tasks may come in any order, repeat and overlap; a task that maps nothing occupies nothing.  Refused with VGSDF_E_ARG before
 * anything runs: a family of another device, families of more than one kind (there are three: glyf, commands, mixed — a
 * submission of mixed families is, byte for byte, vgsdf_outlines_submit_resident_mixed of its sequence; a mixed family beside a
 * family of glyf or of command fonts is refused like glyf beside commands), more than 65536 fonts over the families, first > last,
 * family_of past n_families, more than 2^31 - 1 command slots (or glyphs).  n_tasks == 0, or tasks that map nothing, make an
 * empty submission that waits cleanly.  Collected with vgsdf_outlines_wait; _peek, _pbf_positions and _segments work behind it
 * as behind any other form, and rects_out of _wait / _peek may be NULL.  The fonts of the block are the families' lists in the
 * order of `families`, whether or not a task names the family: all of them count towards the 65536 fonts and the upload.  vgsdf_outlines_resident_upload_bytes reports the block.
 * vgsdf_outlines_task_extents (after _peek or _wait of a ranges submission with pbf_pre): begin[t] = where task t's reserved room
 * starts in the arena, begin[n_tasks] = the arena's size; a task without glyphs has begin[t] == begin[t + 1].
 */
typedef struct {
	uint32_t n_tasks, n_families;
	const vgsdf_family *const *families;
	const uint16_t *family_of;    /* [n_tasks] */
	const uint16_t *first, *last; /* [n_tasks] inclusive code-point range, first <= last */
	const uint32_t *pbf_pre;      /* [n_tasks] or NULL: bytes reserved in front of the task's FIRST glyph entry */
} vgsdf_outlines_ranges;
int vgsdf_outlines_submit_ranges(vgsdf_ctx *ctx, const vgsdf_outlines_ranges *in, uint8_t *out_bitmaps, size_t out_capacity);
int vgsdf_outlines_task_extents(vgsdf_ctx *ctx, uint64_t *begin /* [n_tasks + 1] */);
int vgsdf_outlines_wait(vgsdf_ctx *ctx, vgsdf_rect *rects_out, uint64_t *out_bytes, uint64_t *n_segments, int *rendered);
/* Between submit and wait: blocks until the front-end's results are on the host — they leave the device right behind the
 * plan kernel, on a stream of their own, while flattening and raster are still running — and reports the rects and
 * *out_bytes as vgsdf_outlines_wait will.  *in_place = 1: the raster enqueued with the submission is storing the bitmaps
 * straight into the caller's page-locked out_bitmaps and nothing else will touch that buffer, so the caller may write the
 * bytes BETWEEN the bitmaps (in-place PBF assembly: the headers) while it runs; 0: the bitmaps arrive only in
 * vgsdf_outlines_wait (pageable destination, a capacity guess that did not hold, a batch in error).  Optional. */
int vgsdf_outlines_peek(vgsdf_ctx *ctx, vgsdf_rect *rects_out, uint64_t *out_bytes, int *in_place);
/* after vgsdf_outlines_wait (or _peek) on a batch submitted with pbf_pre / pbf_fix: bitmap_at[g] = where in the arena the device placed
 * glyph g's bitmap (for a glyph without a raster: the byte behind its id field, where the `width` tag goes) */
int vgsdf_outlines_pbf_positions(vgsdf_ctx *ctx, uint64_t *bitmap_at);
/* test / inspection: download the segments the front-end produced (seg_off[n_glyphs+1]) */
int vgsdf_outlines_segments(vgsdf_ctx *ctx, uint32_t *seg_off, double *sx, double *sy, double *ex, double *ey);

/*
 * Union outlines (rule U): a glyph's segments rewritten on the device into the boundary of its filled
 * set { p : winding number != 0 }, so that the edges of one contour inside another no longer take part in the distance.  With
 * it the output is deliberately NOT the reference's.  state: per glyph 0 = nothing to do (the input less its zero-length
 * segments), 1 = rebuilt, 2 = more than 6144 segments, passed through unchanged, 3 = a non-finite coordinate, passed through.
 */
/* b's segments -> the boundary of its filled sets (rule U).  A NEW resident batch with the same
 * glyphs, rects and out_off; b is untouched and both may be launched.  state: [n_glyphs] or NULL. */
int vgsdf_batch_union(vgsdf_ctx *ctx, const vgsdf_dbatch *b, vgsdf_dbatch **out, uint8_t *state);
/* read a resident batch's segments back (seg_off[n_glyphs+1], then four arrays or NULL to size) */
int vgsdf_batch_segments_read(vgsdf_ctx *ctx, const vgsdf_dbatch *b, uint32_t *seg_off, double *sx, double *sy, double *ex, double *ey);
/* the same step for the batch vgsdf_outlines_prepare (or submit with out_bitmaps NULL + wait) left on the
 * context: replaces its segments, descriptors, work list and chunk boxes; vgsdf_outlines_render then
 * renders the union.  In-place PBF positions are kept.  n_segments (may be NULL): the union's. */
int vgsdf_outlines_union(vgsdf_ctx *ctx, uint8_t *state, uint64_t *n_segments);
/* test / inspection (tools/outline_union_ab.py): milliseconds the count and the emit pass of the context's last
 * vgsdf_batch_union or vgsdf_outlines_union took (HIP events around the pass; 0 0 before the first) */
void vgsdf_union_kernel_ms(const vgsdf_ctx *ctx, float ms[2]);

/*
 * Multi-GPU: ONE process drives N devices, one context (+ its own host thread) per device; glyph batches
 * are independent (renderer.rs:103 has no shared state), so results need no exchange and the only collective of the
 * path is the sum of the run counters {blocks, glyphs, pixels} over the contexts.
 *   vgsdf_add_counters    : the dispatcher credits a context with the work it rendered there
 *   vgsdf_reduce_counters : counters[3] = sum over ctxs[0..n).  n >= 2 contexts on DISTINCT devices: an RCCL all-reduce
 *                           (sum, 3 x u64) over a communicator of exactly those devices, on the contexts' streams; every
 *                           rank's result is checked against the others.  RCCL is loaded at first use (dlopen of
 *                           librccl.so.1: no link-time dependency, shared with a host that already mapped it).  The
 *                           payload is 24 bytes the host already holds, so a finished render is never lost to the
 *                           collective: if RCCL cannot be loaded, cannot form the communicator or fails, the sum is taken
 *                           on the host, a line goes to stderr and vgsdf_reduce_path() says so.  One context, and contexts
 *                           that share a device (n lanes rehearsed on one GPU: RCCL refuses two ranks on one device), are
 *                           summed on the host.
 *   vgsdf_reduce_counters_rccl : the same through RCCL or not at all (n >= 1 distinct devices; VGSDF_E_HIP when the
 *                           collective is unavailable or fails, VGSDF_E_ARG when two contexts share a device) — for
 *                           callers and tests that want the failure instead of the fallback.
 *   vgsdf_reduce_path     : how the last reduce whose FIRST context was `ctx` took its sum: "rccl", "host: one context",
 *                           "host: contexts share a device" or "host: RCCL fallback: <reason>".
 * The all-reduce over distinct devices has not run on hardware yet (rounds 1-4 had one-GPU boxes; a one-rank communicator
 * has).  Replaces nothing in the reference (single process, rayon threads: src/font/manager.rs:81-125 counts nothing); it is
 * the north star's "RCCL only for the final block-count reduce".
 */
void vgsdf_add_counters(vgsdf_ctx *ctx, uint64_t blocks, uint64_t glyphs, uint64_t pixels);
void vgsdf_reset_counters(vgsdf_ctx *ctx);
int vgsdf_reduce_counters(vgsdf_ctx **ctxs, int n, uint64_t counters[3]);
int vgsdf_reduce_counters_rccl(vgsdf_ctx **ctxs, int n, uint64_t counters[3]);
const char *vgsdf_reduce_path(const vgsdf_ctx *ctx);

/* Raw device pointer of the resident output bitmaps (for zero-copy consumers on the same
 * device, e.g. a torch tensor wrapping it); valid until vgsdf_batch_free. */
void *vgsdf_batch_device_output(const vgsdf_dbatch *b);

#ifdef __cplusplus
}
#endif
#endif
