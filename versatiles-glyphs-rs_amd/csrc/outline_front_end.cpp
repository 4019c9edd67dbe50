// outline_front_end.cpp — the device outline front-end behind the vgsdf_outlines_* entry points: outline commands (or
// packed commands, or `glyf` bytes) in, rects out (prepare); bitmaps out (render).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <variant>
#include <vector>

#include "device_internal.h"
#include "input_form_kernels.h"
#include "outline_kernels.h"
#include "outline_plan_kernels.h"
#include "resident_fonts.h"
#include "upload_layout.h"
#include "work_plan.h"

// a submission between vgsdf_outlines_submit and vgsdf_outlines_wait
struct FePending {
	bool active = false;
	uint32_t n = 0, n_cmds = 0;
	size_t hdr_off = 0, rh_bytes = 0, at_off = 0; // rects | PlanHeader | (in-place PBF assembly) bitmap positions u64[n]
	bool span = false, spec = false;
	bool copy_stream_waits = false; // the read-back's wait for the plan has been enqueued on the copy stream
	bool spec_direct = false; // the raster stores through the device mapping of the caller's page-locked buffer
	const uint32_t *d_pbf_pre = nullptr; // device copies of the in-place PBF inputs (NULL: bitmaps packed back to back)
	const uint8_t *d_pbf_fix = nullptr;
	uint8_t *spec_out = nullptr, *d_spec = nullptr; // destination of the raster enqueued behind the front-end
	size_t spec_cap = 0;
	uint32_t launch_spans = 0, span_max = 4, span_budget = 16;
	double t0 = 0, t1 = 0;
	// a submission of code-point ranges (vgsdf_outlines_submit_ranges)
	bool by_ranges = false;
	uint32_t n_tasks = 0, n_live = 0;    // the caller's tasks; of which map a glyph (the block's)
	std::vector<uint32_t> task_live;     // [n_tasks] the first task of the block at or behind the caller's task t
	size_t begin_off = 0;                // in the read-back block, with pbf_pre: u64[n_live + 1] where the tasks' reserved rooms begin
	const void *d_names = nullptr;       // with pbf_pre: vgsdf::EntryName[n] of the device (pbf_entries)
};

struct FrontEnd {
	// device: inputs, per-command / per-ring intermediates, results of measure + plan, the resident batch
	DevBuf cmds, kinds, coords, meta, cmd_open, counts, pt_local, cmd_box, cmd_mask, rings, cmd_ring, rects_hdr, descs, tiles, flag;
	DevBuf seg, out, boxes, pbf_in; // seg: records {sx, sy, ex, ey}
	DevBuf h_rects, h_stage; // pinned
	size_t seg_cap = 0, tile_cap = 0; // elements the segment arrays / the work list hold
	uint32_t last_spans = 0;          // work-list length of the previous batch (grid guess of the one-submission form)
	// error words of the submissions: two 16-byte slots used alternately; the plan kernel of a submission zeroes the other
	// slot for its successor (no memset launch per submission).  flags_clean: both slots are known to be in that state
	uint32_t flag_slot = 0;
	bool flags_clean = false;
	uint32_t *flag_word() const { return (uint32_t *)((uint8_t *)flag.p + 16 * (size_t)flag_slot); }
	uint32_t *next_flag_word() const { return (uint32_t *)((uint8_t *)flag.p + 16 * (size_t)(flag_slot ^ 1u)); }
	FePending pend;
	uint64_t resident_upload_bytes = 0; // block of the last vgsdf_outlines_resident submission
	uint32_t n_glyphs = 0, n_cmds = 0, n_segs = 0;
	uint64_t out_bytes = 0;
	vgsdf_dbatch batch; // borrowed view over the buffers above
	bool prepared = false;
	bool peeked = false; // vgsdf_outlines_peek has waited for the read-back of the pending submission
	// vgsdf_outlines_union: the arena `batch` views instead of the buffers above, until the next submission is waited for
	vgsdf_dbatch *unioned = nullptr;
	void drop_union() // (nothing in flight uses it: the callers stand behind a synchronisation)
	{
		if (!unioned)
			return;
		(void)hipFree(unioned->d_arena);
		(void)hipHostFree(unioned->h_stage);
		delete unioned;
		unioned = nullptr;
	}
	FrontEnd()
	{
		h_rects.host = true;
		h_stage.host = true;
		batch.borrowed = true;
	}
	void release_all()
	{
		for (DevBuf *b : {&cmds, &kinds, &coords, &meta, &cmd_open, &counts, &pt_local, &cmd_box, &cmd_mask, &rings, &cmd_ring, &rects_hdr, &descs, &tiles, &flag, &seg, &out, &boxes, &pbf_in,
		                  &h_rects, &h_stage})
			b->release();
		drop_union();
	}
};

void fe_destroy(FrontEnd *fe)
{
	if (!fe)
		return;
	fe->release_all();
	delete fe;
}

#define FE_TRY(expr) HIP_TRY_AS(ctx, "vgsdf_outlines: " #expr, expr)
// (a launch: its failure is never reported as VGSDF_E_OOM)
#define FE_KERNEL(expr)                                                                         \
	do {                                                                                        \
		int e__ = (expr);                                                                       \
		if (e__ != 0) {                                                                         \
			ctx->err = std::string("vgsdf_outlines: " #expr ": ") + hipGetErrorString((hipError_t)e__); \
			return VGSDF_E_HIP;                                                                 \
		}                                                                                       \
	} while (0)

// ---- the front-end as two halves: submit (everything enqueued, nothing waited for) and wait (the one
// synchronisation, the read-back, second launches if a guess was too small).  With a destination (`spec_out`,
// `spec_cap` bytes) the raster is enqueued right behind the front-end kernels, before the host has seen the plan: its
// grid and every capacity are guesses the plan kernel checks on the device (PlanHeader::ok).  When they hold, the
// bitmaps are in `spec_out` after the wait (written there by the kernel itself if the buffer is page-locked).
namespace {
struct FeDev { // device views of a submitted batch
	const vgsdf::OutlineCmd *cmds;
	const double *scale, *shift;
	const uint32_t *cmd_off;
	vgsdf::OutlineRect *rects;
	vgsdf::PlanHeader *hdr;
	vgsdf::GlyphDesc *descs;
};
FeDev fe_dev(FrontEnd &fe)
{
	const FePending &p = fe.pend;
	const vgsdf::GlyphArraysLayout at(p.n); // (the head of fe.meta in every input form)
	FeDev d;
	d.cmds = (const vgsdf::OutlineCmd *)fe.cmds.p;
	d.scale = (const double *)((const uint8_t *)fe.meta.p + at.scale);
	d.shift = (const double *)((const uint8_t *)fe.meta.p + at.shift_x);
	d.cmd_off = (const uint32_t *)((const uint8_t *)fe.meta.p + at.cmd_off);
	d.rects = (vgsdf::OutlineRect *)fe.rects_hdr.p;
	d.hdr = (vgsdf::PlanHeader *)((uint8_t *)fe.rects_hdr.p + p.hdr_off);
	d.descs = (vgsdf::GlyphDesc *)fe.descs.p;
	return d;
}
int fe_launch_plan(vgsdf_ctx *ctx, FrontEnd &fe, uint32_t spans_launched)
{
	const FePending &p = fe.pend;
	const FeDev d = fe_dev(fe);
	return vgsdf_outline_plan(d.rects, p.n, p.span ? 1 : 0, (uint32_t)vgsdf_filtered_delta_cap(), p.span_max, p.span_budget,
	                          (uint32_t)std::min<size_t>(fe.tile_cap, 0x7FFFFFFFu), d.descs, (vgsdf::SpanRec *)fe.tiles.p, d.hdr,
	                          fe.flag_word(), (unsigned long long)fe.seg_cap, (unsigned long long)p.spec_cap,
	                          spans_launched, p.d_pbf_pre, p.d_pbf_fix,
	                          p.d_pbf_fix ? (unsigned long long *)((uint8_t *)fe.rects_hdr.p + p.at_off) : nullptr, fe.next_flag_word(), ctx->stream);
}
// The second flattening pass and the raster's chunk boxes.  Boxes: by default the first workgroups of the pass's own grid take
// them from the commands' boxes (outline_kernels.hip, chunk_boxes_of_glyph: supersets of the exact boxes, no launch of their
// own); VGSDF_CMD_BOXES=0 (measurement switch): from the segments, by sdf_chunk_boxes behind the pass
int fe_launch_emit(vgsdf_ctx *ctx, FrontEnd &fe)
{
	const FePending &p = fe.pend;
	const FeDev d = fe_dev(fe);
	static const char *cb_env = std::getenv("VGSDF_CMD_BOXES");
	const bool cmd_boxes = p.span && !(cb_env && cb_env[0] == '0');
	int e = vgsdf_outline_emit_segments(d.cmds, p.n_cmds, (const uint8_t *)fe.cmd_open.p, d.scale, d.shift, (const uint32_t *)fe.pt_local.p,
	                                    (const vgsdf::RingRec *)fe.rings.p, (const uint32_t *)fe.cmd_ring.p, d.descs, d.hdr,
	                                    (unsigned long long)fe.seg_cap, (double *)fe.seg.p, (const unsigned long long *)fe.cmd_mask.p,
	                                    cmd_boxes ? p.n : 0u, d.cmd_off, fe.cmd_box.p, fe.boxes.p, ctx->stream);
	if (e == 0 && p.span && !cmd_boxes)
		e = vgsdf_launch_chunk_boxes(d.descs, p.n, (const double *)fe.seg.p, (const double *)fe.seg.p + 1, (const double *)fe.seg.p + 2,
		                             (const double *)fe.seg.p + 3, 4, fe.boxes.p, d.hdr, (unsigned long long)fe.seg_cap, ctx->stream);
	return e;
}
// pbf_entries of a ranges submission with pbf_pre: into `out` (NULL: the tasks' extents only); need_ok: under PlanHeader::ok, as
// the raster enqueued behind the plan — the launches the host repeats after a guess that did not hold pass false
int fe_launch_entries(vgsdf_ctx *ctx, FrontEnd &fe, uint8_t *out, size_t out_cap, bool need_ok)
{
	const FePending &p = fe.pend;
	const FeDev d = fe_dev(fe);
	uint8_t *const rh = (uint8_t *)fe.rects_hdr.p;
	return vgsdf_pbf_entries(d.rects, (const unsigned long long *)(rh + p.at_off), p.d_pbf_pre, p.d_names, p.n, p.n_live, d.hdr, need_ok,
	                         (unsigned long long)out_cap, out, (unsigned long long *)(rh + p.begin_off), ctx->stream);
}
hipError_t fe_ensure_tiles(FrontEnd &fe, size_t want)
{
	if (want <= fe.tile_cap)
		return hipSuccess;
	hipError_t e = fe.tiles.ensure(sizeof(vgsdf::SpanRec) * want);
	if (e == hipSuccess)
		fe.tile_cap = fe.tiles.cap / sizeof(vgsdf::SpanRec);
	return e;
}
hipError_t fe_ensure_segs(FrontEnd &fe, size_t want, uint32_t n_glyphs)
{
	if (want > fe.seg_cap) {
		if (hipError_t e = fe.seg.ensure(32 * want + 32); e != hipSuccess)
			return e;
		fe.seg_cap = fe.seg.cap / 32 - 1;
	}
	return fe.boxes.ensure(vgsdf_chunk_box_bytes(fe.seg_cap, n_glyphs) + 16);
}
} // namespace

// The input forms of a submission.  A FeInput has exactly one; the legal states are the enumerators
enum class FeForm {
	Records,          // 28-byte command records (vgsdf_outlines)
	Packed,           // kinds + the coordinates they carry (vgsdf_outlines_packed)
	Glyf,             // the glyphs' `glyf` arrays as parts; cmd_off counts command SLOTS (vgsdf_outlines_glyf)
	ResidentGlyf,     // glyphs named by (font, glyph id) of fonts from vgsdf_font_create: the upload kernel expands their leaves into parts
	ResidentCommands, // ... of fonts from vgsdf_font_create_commands: the upload kernel gathers their records and context bytes
	ResidentMixed,    // ... of fonts of both kinds in one list: the upload kernel does both, glyph by glyph, and the decoder runs over the parts
};
struct FeInput {
	FeForm form = FeForm::Records;
	uint32_t n_glyphs = 0;
	const uint32_t *cmd_off = nullptr;
	const double *scale = nullptr, *shift_x = nullptr;
	const vgsdf_outline_cmd *cmds = nullptr; // Records
	const uint32_t *dat_off = nullptr;       // Packed
	const uint8_t *kinds = nullptr;
	const float *coords = nullptr;
	const uint32_t *pbf_pre = nullptr; // in-place PBF assembly (every form but Records): both or neither
	const uint8_t *pbf_fix = nullptr;
	const vgsdf_glyf_part *parts = nullptr; // Glyf (ResidentGlyf: n_parts only — the parts come to be on the device)
	uint32_t n_parts = 0;
	const uint8_t *bytes = nullptr;
	uint32_t n_bytes = 0;
	// the named forms: the arrays above point into the block the library gathered in the context's page-locked staging buffer
	uint32_t n_fonts = 0;
	uint32_t res_max_cap = 0, res_max_len = 0; // over the fonts the submission names
	bool res_scales_plain = true;
	// code-point ranges of families: no per-glyph array exists on the host (the ones above stay NULL but for pbf_pre / pbf_fix,
	// which only SAY that the submission assembles PBF in place); the block lies in the context's staging buffer
	const struct FeRanges *ranges = nullptr;

	// the glyphs are named, not sent: the library validated the names, summed the offsets itself and gathered the block
	bool names_glyphs() const { return form == FeForm::ResidentGlyf || form == FeForm::ResidentCommands || form == FeForm::ResidentMixed; }
	// ... and some of them have leaves that the upload kernel expands into parts behind the device's copy of the block
	bool expands_leaves() const { return form == FeForm::ResidentGlyf || form == FeForm::ResidentMixed; }
	// ... and some of them have records that the upload kernel gathers from their fonts' stores
	bool gathers_records() const { return form == FeForm::ResidentCommands || form == FeForm::ResidentMixed; }
	// the command records come out of the device's glyf decoder, which runs on parts
	bool decodes_glyf() const { return form == FeForm::Glyf || expands_leaves(); }
	// the form may bring pbf_pre / pbf_fix
	bool takes_pbf() const { return form != FeForm::Records; }
};

struct FeRanges {
	uint32_t n_cmds = 0, n_families = 0;
	uint32_t n_tasks = 0, n_live = 0;
	std::vector<uint32_t> task_live;
	const uint8_t *block = nullptr; // RangesBlockLayout(n_live, n_families, n_fonts)
	size_t block_bytes = 0;
};

// ---- submit, step by step (fe_submit below keeps their order: it is part of the contract with the device) ----

// 1. argument checks: nothing is touched on a bad call.  Sets the command and coordinate counts of the batch
static int fe_check_args(vgsdf_ctx *ctx, const FeInput *in, uint32_t &n_cmds, uint32_t &n_floats)
{
	if (in && in->ranges) { // (laid out by the library itself from validated families)
		n_cmds = in->ranges->n_cmds;
		n_floats = 0;
		return VGSDF_OK;
	}
	if (!in || (in->n_glyphs && (!in->cmd_off || !in->scale || !in->shift_x || (in->form == FeForm::Packed && !in->dat_off)))) {
		ctx->err = "vgsdf_outlines: NULL argument";
		return VGSDF_E_ARG;
	}
	if ((in->pbf_pre == nullptr) != (in->pbf_fix == nullptr) || (in->pbf_fix && !in->takes_pbf())) {
		ctx->err = "vgsdf_outlines: pbf_pre and pbf_fix come together (packed and glyf forms only)";
		return VGSDF_E_ARG;
	}
	static_assert(sizeof(vgsdf_glyf_part) == 48, "ABI struct mirrors the kernel struct");
	static_assert(sizeof(vgsdf_outline_cmd) == sizeof(vgsdf::OutlineCmd), "ABI struct mirrors the kernel struct");
	static_assert(sizeof(vgsdf_rect) == sizeof(vgsdf::OutlineRect), "ABI struct mirrors the kernel struct");
	const uint32_t n = in->n_glyphs;
	if (n && in->cmd_off[0] != 0) {
		ctx->err = "vgsdf_outlines: cmd_off[0] must be 0";
		return VGSDF_E_ARG;
	}
	n_cmds = n ? in->cmd_off[n] : 0;
	if (n_cmds && ((in->form == FeForm::Packed && !in->kinds) || (in->form == FeForm::Records && !in->cmds))) {
		ctx->err = "vgsdf_outlines: NULL command array";
		return VGSDF_E_ARG;
	}
	if (in->form == FeForm::Glyf && ((in->n_parts && (!in->parts || !in->bytes)) || (in->n_bytes & 3u))) {
		ctx->err = "vgsdf_outlines_glyf: NULL parts / bytes, or n_bytes not a multiple of 4";
		return VGSDF_E_ARG;
	}
	if (in->form == FeForm::Packed && n && (in->dat_off[0] != 0 || (in->dat_off[n] && !in->coords))) {
		ctx->err = in->dat_off[0] != 0 ? "vgsdf_outlines: dat_off[0] must be 0" : "vgsdf_outlines: NULL coordinate array";
		return VGSDF_E_ARG;
	}
	n_floats = in->form == FeForm::Packed && n ? in->dat_off[n] : 0u;
	return VGSDF_OK;
}

// 2. The walks over the input — offsets monotone, parts tiling the command slots inside their glyphs and inside `bytes`, scales —
// are what every kernel's indexing rests on, so they come before the first kernel that reads the input; but not before the
// UPLOAD, which reads nothing of it: a single-block submission starts its copy first and validates under it (25 k entries
// of a 21-font group: ~45 us of this thread that the device used to wait for).
// (the command kinds are checked on the device: the kernels treat an unknown kind as a no-op and the context
// pass raises the batch's error flag, so nothing unsafe runs and the host need not walk the commands)
struct FeFacts { // what the walks note on their way, for the launches
	uint32_t glyf_max_cap = 0, glyf_max_len = 0; // the largest cmd_cap / byte_len among the parts
	bool parts_inside_glyphs = true;             // every part's slots lie inside ONE glyph's range (what a sound caller sends)
	bool scales_plain = true;                    // every scale positive and finite
};
static int fe_validate(vgsdf_ctx *ctx, const FeInput *in, uint32_t n_cmds, FeFacts &facts)
{
	const uint32_t n = in->n_glyphs;
	FeFacts &f = facts;
	uint32_t bad = 0;
	for (uint32_t g = 0; g < n; g++) {
		bad |= in->cmd_off[g + 1] < in->cmd_off[g];
		f.scales_plain = f.scales_plain && in->scale[g] > 0.0 && in->scale[g] < HUGE_VAL;
	}
	if (bad) {
		ctx->err = "vgsdf_outlines: cmd_off not monotone";
		return VGSDF_E_ARG;
	}
	if (in->form == FeForm::Glyf) {
		// the parts tile the command slots in order, and their bytes lie inside `bytes` (what the bytes SAY is checked on
		// the device, entry by entry)
		uint64_t slots = 0;
		uint32_t gi = 0;
		for (uint32_t i = 0; i < in->n_parts; i++) {
			const vgsdf_glyf_part &pt = in->parts[i];
			while (gi < n && in->cmd_off[gi + 1] <= pt.cmd_at)
				gi++;
			f.parts_inside_glyphs = f.parts_inside_glyphs && gi < n && pt.cmd_at >= in->cmd_off[gi] && (uint64_t)pt.cmd_at + pt.cmd_cap <= in->cmd_off[gi + 1];
			f.glyf_max_cap = std::max(f.glyf_max_cap, pt.cmd_cap);
			f.glyf_max_len = std::max(f.glyf_max_len, pt.byte_len);
			if (pt.cmd_at != slots || (pt.byte_off & 3u) || pt.byte_off > in->n_bytes || pt.byte_len > in->n_bytes - pt.byte_off ||
			    pt.n_contours == 0) {
				ctx->err = "vgsdf_outlines_glyf: parts must tile the command slots in order, with 4-aligned byte ranges inside `bytes`";
				return VGSDF_E_ARG;
			}
			slots += pt.cmd_cap;
		}
		if (slots != n_cmds) {
			ctx->err = "vgsdf_outlines_glyf: cmd_off[n_glyphs] differs from the parts' command slots";
			return VGSDF_E_ARG;
		}
	}
	if (in->form == FeForm::Packed) {
		for (uint32_t g = 0; g < n; g++)
			bad |= in->dat_off[g + 1] < in->dat_off[g];
		if (bad) {
			ctx->err = "vgsdf_outlines: dat_off not monotone";
			return VGSDF_E_ARG;
		}
	}
	return VGSDF_OK;
}

// How the input of a submission travels.  The device keeps the glyf form, and a packed single block, in fe.meta in the
// single-block layout (upload_layout.h) whether the arrays arrive as one block or one by one; otherwise fe.meta holds
// the per-glyph arrays only (staged as one block) and kinds / coords / cmds have buffers of their own.
using FeLayout = std::variant<vgsdf::PackedBlockLayout, vgsdf::GlyfBlockLayout, vgsdf::ResidentBlockLayout, vgsdf::CommandBlockLayout>;
struct FeUpload {
	FeLayout layout; // that of the submission's own form (Records: the head of the packed one)
	// what every form's layout shares
	size_t block_bytes = 0;          // the arrays as ONE block
	size_t pbf_pre = 0, pbf_fix = 0; // where the PBF arrays lie in it
	size_t arrays_bytes = 0;         // scale | shift_x | cmd_off [| dat_off]
	size_t meta_bytes = 0;           // what the device keeps in fe.meta
	const uint8_t *block = nullptr; // the caller's arrays are ONE page-locked block in their form's layout: one copy
	const void *mapped = nullptr; // ... that the device can address: uploaded by a kernel (input_form_kernels.hip, copy_in)
	// set by fe_upload: device views of what the form brings besides the per-glyph arrays (those: fe_dev)
	const uint8_t *d_kinds = nullptr, *d_parts = nullptr, *d_bytes = nullptr;
	const float *d_coords = nullptr;
	const uint32_t *d_dat_off = nullptr;
};
static FeLayout fe_layout(const FeInput *in, uint32_t n_cmds, uint32_t n_floats)
{
	const uint32_t n = in->n_glyphs;
	const bool pbf = in->pbf_fix != nullptr;
	switch (in->form) {
	case FeForm::Glyf:
		return vgsdf::GlyfBlockLayout(n, in->n_parts, in->n_bytes, pbf);
	case FeForm::ResidentGlyf:
	case FeForm::ResidentMixed: // (the glyf form's block: a glyph of a command font has no parts)
		return vgsdf::ResidentBlockLayout(n, in->n_fonts, pbf);
	case FeForm::ResidentCommands:
		return vgsdf::CommandBlockLayout(n, in->n_fonts, pbf);
	case FeForm::Records:
	case FeForm::Packed:
		break;
	}
	return vgsdf::PackedBlockLayout(n, n_cmds, n_floats, pbf);
}
static FeUpload fe_upload_form(const FeInput *in, uint32_t n_cmds, uint32_t n_floats)
{
	const bool pbf = in->pbf_fix != nullptr;
	FeUpload up{fe_layout(in, n_cmds, n_floats)};
	std::visit([&up](const auto &l) { up.block_bytes = l.bytes, up.pbf_pre = l.pbf_pre, up.pbf_fix = l.pbf_fix, up.arrays_bytes = l.end; }, up.layout);
	// the block is recognised by the caller's pointers: every array where the layout has it, counted from `scale`
	const uint8_t *hb = in->ranges ? in->ranges->block : (const uint8_t *)in->scale;
	const size_t layout_bytes = up.block_bytes; // (what the device keeps of a named form, whatever was uploaded)
	if (in->ranges)
		up.block_bytes = in->ranges->block_bytes;
	auto at = [hb](const void *array, size_t off) { return (const uint8_t *)array == hb + off; };
	bool single = false;
	switch (in->form) {
	case FeForm::ResidentGlyf:
	case FeForm::ResidentMixed:
	case FeForm::ResidentCommands: // (gathered by the library itself, in the context's page-locked staging buffer)
		single = true;
		break;
	case FeForm::Glyf: {
		const auto &gl = std::get<vgsdf::GlyfBlockLayout>(up.layout);
		single = at(in->shift_x, gl.shift_x) && at(in->cmd_off, gl.cmd_off) && at(in->parts, gl.parts) && at(in->bytes, gl.glyf_bytes) &&
		         (!pbf || (at(in->pbf_pre, gl.pbf_pre) && at(in->pbf_fix, gl.pbf_fix)));
		break;
	}
	case FeForm::Packed: {
		const auto &pk = std::get<vgsdf::PackedBlockLayout>(up.layout);
		up.arrays_bytes = pk.arrays_end;
		single = at(in->shift_x, pk.shift_x) && at(in->cmd_off, pk.cmd_off) && at(in->dat_off, pk.dat_off) && at(in->coords, pk.coords) &&
		         at(in->kinds, pk.kinds) && (!pbf || (at(in->pbf_pre, pk.pbf_pre) && at(in->pbf_fix, pk.pbf_fix)));
		break;
	}
	case FeForm::Records: // (its command records never travel with the per-glyph arrays)
		break;
	}
	if (single && is_pinned(hb, up.block_bytes))
		up.block = hb;
	static const char *ck_env = std::getenv("VGSDF_COPY_KERNEL"); // (0: measurement switch, the copy engine takes the block)
	if (up.block && !(ck_env && ck_env[0] == '0') && ((uintptr_t)hb & 15u) == 0)
		up.mapped = pinned_device_ptr(const_cast<uint8_t *>(hb), up.block_bytes);
	// the device's copy: the block as it stands (ResidentGlyf: and the parts its leaves expand into behind it); the
	// per-glyph arrays alone where commands or kinds / coords arrive one by one and have buffers of their own
	const bool arrays_only = in->form == FeForm::Records || (in->form == FeForm::Packed && !up.block);
	up.meta_bytes = arrays_only ? up.arrays_bytes : layout_bytes;
	if (in->expands_leaves())
		up.meta_bytes += sizeof(vgsdf_glyf_part) * (size_t)in->n_parts;
	return up;
}

// 3. buffer reservation: everything a submission of this size writes.  Sets the layout of the read-back block in fe.pend
static int fe_reserve(vgsdf_ctx *ctx, FrontEnd &fe, const FeInput *in, uint32_t n_cmds, const FeUpload &up)
{
	FePending &p = fe.pend;
	const uint32_t n = in->n_glyphs;
	FE_TRY(fe.cmds.ensure(sizeof(vgsdf::OutlineCmd) * (size_t)(n_cmds + 1)));
	FE_TRY(fe.meta.ensure(up.meta_bytes + 16));
	if (!in->names_glyphs()) // (a submission that names its glyphs: its block lies there already)
		FE_TRY(fe.h_stage.ensure(up.arrays_bytes + 16));
	FE_TRY(fe.cmd_open.ensure((size_t)n_cmds + 1));
	FE_TRY(fe.counts.ensure(4 * (size_t)(n_cmds + 1)));
	FE_TRY(fe.pt_local.ensure(4 * ((size_t)n_cmds + n + 2)));
	FE_TRY(fe.cmd_box.ensure(32 * (size_t)(n_cmds + 1)));
	FE_TRY(fe.cmd_mask.ensure(8 * (size_t)(n_cmds + 1)));
	FE_TRY(fe.rings.ensure(sizeof(vgsdf::RingRec) * (size_t)(n_cmds + 1)));
	FE_TRY(fe.cmd_ring.ensure(4 * (size_t)(n_cmds + 1)));
	p.hdr_off = align_up(sizeof(vgsdf::OutlineRect) * (size_t)n, 16); // rects and totals: one block, one read-back
	p.at_off = align_up(p.hdr_off + sizeof(vgsdf::PlanHeader), 16);
	p.rh_bytes = in->pbf_fix ? p.at_off + 8 * (size_t)n : p.hdr_off + sizeof(vgsdf::PlanHeader);
	if (in->ranges && in->pbf_fix) { // the tasks' extents travel back with the positions; the entries' names stay on the device
		p.begin_off = p.rh_bytes;
		p.rh_bytes += 8 * ((size_t)p.n_live + 1);
		FE_TRY(fe.pbf_in.ensure(sizeof(vgsdf::EntryName) * (size_t)n + 16));
		p.d_names = fe.pbf_in.p;
	}
	FE_TRY(fe.rects_hdr.ensure(p.rh_bytes));
	FE_TRY(fe.h_rects.ensure(p.rh_bytes));
	FE_TRY(fe.descs.ensure(sizeof(vgsdf::GlyphDesc) * (size_t)n + 16));
	FE_TRY(fe.flag.ensure(32));
	// capacities of what only the device knows the size of: the work list and the segment arrays.  Guessed from
	// the input (and kept from earlier batches); the plan / emit kernels write nothing past them and the totals
	// that come back with the rects say whether a second launch is needed.
	FE_TRY(fe_ensure_tiles(fe, 2 * (size_t)n + 1024));
	FE_TRY(fe_ensure_segs(fe, 12 * (size_t)n_cmds + 4096, n));
	return VGSDF_OK;
}

// 4. upload, per input form
static hipError_t fe_copy_in(hipStream_t st, void *dst, const void *src, size_t bytes)
{
	return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
}
// The block of a named form as its ONE upload kernel can read it: the page-locked block itself; without a device mapping
// (or with VGSDF_COPY_KERNEL=0) the copy engine brings the block into fe.coords first and the kernel reads that copy
static int fe_kernel_readable_block(vgsdf_ctx *ctx, FrontEnd &fe, const FeUpload &up, const void *&src)
{
	src = up.mapped;
	if (src)
		return VGSDF_OK;
	FE_TRY(fe.coords.ensure(up.block_bytes + 16));
	FE_TRY(fe_copy_in(ctx->stream, fe.coords.p, up.block, up.block_bytes));
	src = fe.coords.p;
	return VGSDF_OK;
}
// per-glyph inputs (scale, shift, command offsets [, coordinate offsets]) of a form whose arrays arrive one by one: they
// travel as ONE block through pinned staging
static int fe_stage_arrays(vgsdf_ctx *ctx, FrontEnd &fe, const FeInput *in, const FeUpload &up)
{
	const auto &pk = std::get<vgsdf::PackedBlockLayout>(up.layout);
	const size_t n = in->n_glyphs;
	uint8_t *hm = (uint8_t *)fe.h_stage.p;
	std::memcpy(hm + pk.scale, in->scale, 8 * n);
	std::memcpy(hm + pk.shift_x, in->shift_x, 8 * n);
	std::memcpy(hm + pk.cmd_off, in->cmd_off, 4 * (n + 1));
	if (in->form == FeForm::Packed)
		std::memcpy(hm + pk.dat_off, in->dat_off, 4 * (n + 1));
	FE_TRY(fe_copy_in(ctx->stream, fe.meta.p, hm, up.arrays_bytes));
	return VGSDF_OK;
}
static int fe_upload(vgsdf_ctx *ctx, FrontEnd &fe, const FeInput *in, uint32_t n_cmds, uint32_t n_floats, FeUpload &up)
{
	FePending &p = fe.pend;
	hipStream_t st = ctx->stream;
	const size_t n = in->n_glyphs;
	const bool pbf = in->pbf_fix != nullptr;
	uint8_t *dm = (uint8_t *)fe.meta.p;
	auto copy = [st](void *dst, const void *src, size_t bytes) { return fe_copy_in(st, dst, src, bytes); };
	// a block the caller built (Glyf, Packed): one kernel or one copy brings it over as it stands
	auto copy_block = [&]() -> int {
		if (up.mapped)
			FE_KERNEL(vgsdf_copy_in(up.mapped, dm, up.block_bytes, st));
		else if (up.block)
			FE_TRY(copy(dm, up.block, up.block_bytes));
		return VGSDF_OK;
	};
	if (in->ranges) { // ONE kernel: it names the glyphs from the families' tables, then expands / gathers as the cases below
		const bool commands = in->form == FeForm::ResidentCommands;
		const int kind = commands ? VGSDF_FONTS_COMMANDS : in->form == FeForm::ResidentMixed ? VGSDF_FONTS_MIXED : VGSDF_FONTS_GLYF;
		const void *src = nullptr;
		if (int rc = fe_kernel_readable_block(ctx, fe, up, src); rc != VGSDF_OK)
			return rc;
		// (the device's copy is laid out as that of the form that names its glyphs one by one)
		const size_t fonts_at = commands ? std::get<vgsdf::CommandBlockLayout>(up.layout).fonts : std::get<vgsdf::ResidentBlockLayout>(up.layout).fonts;
		const size_t parts_at = commands ? 0 : std::get<vgsdf::ResidentBlockLayout>(up.layout).bytes;
		FE_KERNEL(vgsdf_family_upload(kind, src, dm, (uint32_t)n, n_cmds, in->n_parts, in->n_fonts, in->ranges->n_live, in->ranges->n_families,
		                              pbf, dm + parts_at, (vgsdf::OutlineCmd *)fe.cmds.p, (uint8_t *)fe.cmd_open.p, const_cast<void *>(p.d_names),
		                              fe.flag_word(), st));
		if (!commands) {
			up.d_parts = dm + parts_at;
			up.d_bytes = dm + fonts_at;
		}
		fe.resident_upload_bytes = up.block_bytes;
	} else
	switch (in->form) {
	case FeForm::ResidentGlyf: { // ONE kernel: the copy of the block and the expansion of the glyphs' leaves into parts behind it
		const auto &rs = std::get<vgsdf::ResidentBlockLayout>(up.layout);
		const void *src = nullptr;
		if (int rc = fe_kernel_readable_block(ctx, fe, up, src); rc != VGSDF_OK)
			return rc;
		FE_KERNEL(vgsdf_resident_expand(src, dm, rs.bytes, (uint32_t)n, in->n_parts, in->n_fonts, pbf, dm + rs.bytes, st));
		up.d_parts = dm + rs.bytes;
		up.d_bytes = dm + rs.fonts; // (the fonts' stores: vgsdf_glyf_decode_resident)
		fe.resident_upload_bytes = rs.bytes;
		break;
	}
	case FeForm::ResidentMixed: { // ONE kernel here too: the copy of the block, the expansion for the glyphs of glyf fonts and the
		                          // gather for those of command fonts
		const auto &rs = std::get<vgsdf::ResidentBlockLayout>(up.layout);
		const void *src = nullptr;
		if (int rc = fe_kernel_readable_block(ctx, fe, up, src); rc != VGSDF_OK)
			return rc;
		FE_KERNEL(vgsdf_resident_mixed(src, dm, rs.bytes, (uint32_t)n, n_cmds, in->n_parts, in->n_fonts, pbf, dm + rs.bytes,
		                               (vgsdf::OutlineCmd *)fe.cmds.p, (uint8_t *)fe.cmd_open.p, st));
		up.d_parts = dm + rs.bytes;
		up.d_bytes = dm + rs.fonts; // (the decoder follows a part's font index: parts name glyf fonts only)
		fe.resident_upload_bytes = rs.bytes;
		break;
	}
	case FeForm::ResidentCommands: { // ONE kernel again: the copy of the block and the gather of the named glyphs' records and
		                             // context bytes from the fonts' stores
		const void *src = nullptr;
		if (int rc = fe_kernel_readable_block(ctx, fe, up, src); rc != VGSDF_OK)
			return rc;
		FE_KERNEL(vgsdf_resident_gather(src, dm, up.block_bytes, (uint32_t)n, n_cmds, in->n_fonts, pbf, (vgsdf::OutlineCmd *)fe.cmds.p,
		                                (uint8_t *)fe.cmd_open.p, st));
		fe.resident_upload_bytes = up.block_bytes;
		break;
	}
	case FeForm::Glyf: {
		const auto &gl = std::get<vgsdf::GlyfBlockLayout>(up.layout);
		if (int rc = copy_block(); rc != VGSDF_OK)
			return rc;
		if (!up.block) { // (array by array, to where the block would have put them)
			FE_TRY(copy(dm + gl.scale, in->scale, 8 * n));
			FE_TRY(copy(dm + gl.shift_x, in->shift_x, 8 * n));
			FE_TRY(copy(dm + gl.cmd_off, in->cmd_off, 4 * (n + 1)));
			FE_TRY(copy(dm + gl.parts, in->parts, sizeof(vgsdf_glyf_part) * (size_t)in->n_parts));
			FE_TRY(copy(dm + gl.glyf_bytes, in->bytes, in->n_bytes));
			FE_TRY(copy(dm + gl.pbf_pre, in->pbf_pre, pbf ? 4 * n : 0));
			FE_TRY(copy(dm + gl.pbf_fix, in->pbf_fix, pbf ? n : 0));
		}
		up.d_parts = dm + gl.parts;
		up.d_bytes = dm + gl.glyf_bytes;
		break;
	}
	case FeForm::Packed: {
		const auto &pk = std::get<vgsdf::PackedBlockLayout>(up.layout);
		up.d_dat_off = (const uint32_t *)(dm + pk.dat_off);
		if (up.block) {
			if (int rc = copy_block(); rc != VGSDF_OK)
				return rc;
			up.d_coords = (const float *)(dm + pk.coords);
			up.d_kinds = dm + pk.kinds;
			break;
		}
		FE_TRY(fe.kinds.ensure((size_t)n_cmds + 16));
		FE_TRY(fe.coords.ensure(4 * (size_t)n_floats + 16));
		FE_TRY(copy(fe.kinds.p, in->kinds, (size_t)n_cmds));
		FE_TRY(copy(fe.coords.p, in->coords, 4 * (size_t)n_floats));
		up.d_kinds = (const uint8_t *)fe.kinds.p;
		up.d_coords = (const float *)fe.coords.p;
		if (int rc = fe_stage_arrays(ctx, fe, in, up); rc != VGSDF_OK)
			return rc;
		if (pbf) { // the one exception to the rule below: arrays that did not travel in a block get copies of their own
			FE_TRY(fe.pbf_in.ensure(5 * n + 16));
			FE_TRY(copy(fe.pbf_in.p, in->pbf_pre, 4 * n));
			FE_TRY(copy((uint8_t *)fe.pbf_in.p + 4 * n, in->pbf_fix, n));
			p.d_pbf_pre = (const uint32_t *)fe.pbf_in.p;
			p.d_pbf_fix = (const uint8_t *)fe.pbf_in.p + 4 * n;
		}
		break;
	}
	case FeForm::Records:
		FE_TRY(copy(fe.cmds.p, in->cmds, sizeof(vgsdf::OutlineCmd) * (size_t)n_cmds));
		if (int rc = fe_stage_arrays(ctx, fe, in, up); rc != VGSDF_OK)
			return rc;
		break;
	}
	// the PBF arrays: the block travelled as one (or was laid out as one on the device), so they sit at the layout's offsets in fe.meta
	if (pbf && !p.d_pbf_fix) {
		p.d_pbf_pre = (const uint32_t *)(dm + up.pbf_pre);
		p.d_pbf_fix = dm + up.pbf_fix;
	}
	return VGSDF_OK;
}

// the raster launch enqueued behind the front-end: default kernel only, destination the caller's page-locked
// buffer itself or, for pageable memory, the context's device buffer
static int fe_place_raster(vgsdf_ctx *ctx, FrontEnd &fe)
{
	FePending &p = fe.pend;
	p.spec = p.spec_out != nullptr && p.spec_cap != 0 && ctx->variant == 0;
	if (!p.spec)
		return VGSDF_OK;
	if (void *mapped = pinned_device_ptr(p.spec_out, p.spec_cap)) {
		p.d_spec = (uint8_t *)mapped;
		p.spec_direct = true;
	} else {
		FE_TRY(fe.out.ensure(p.spec_cap + 16));
		p.d_spec = (uint8_t *)fe.out.p;
	}
	const size_t guess = fe.last_spans ? (size_t)fe.last_spans + fe.last_spans / 2 + 256 : fe.tile_cap;
	p.launch_spans = (uint32_t)std::min<size_t>(std::min(guess, fe.tile_cap), 0x7FFFFFFFu);
	return VGSDF_OK;
}

// 5. the kernels and the read-back of their results
static int fe_enqueue(vgsdf_ctx *ctx, FrontEnd &fe, const FeInput *in, const FeUpload &up, const FeFacts &facts)
{
	const FePending &p = fe.pend;
	hipStream_t st = ctx->stream;
	const uint32_t n = p.n, n_cmds = p.n_cmds;
	const FeDev d = fe_dev(fe);
	uint32_t *const flagw = fe.flag_word();
	// glyf form: the decoder writes the context bytes itself (the ring state follows from the contour rules) when no glyph
	// of the batch has an odd scale (not positive and finite: bit 1 of the context byte, which only the context pass forms)
	// and no part straddles two glyphs (the decoder's rule is per part; the ring pass trusts the context bytes to be those of
	// the glyph's own command sequence — a byte that says "open" in front of a glyph's first command would index a ring
	// that does not exist)
	bool decode_makes_context = in->decodes_glyf() && facts.parts_inside_glyphs && facts.scales_plain;
	static const char *fuse_env = std::getenv("VGSDF_FUSE_CONTEXT"); // (measurement switch)
	if (fuse_env && fuse_env[0] == '0')
		decode_makes_context = false;
	// command fonts: the gathered context bytes are the context pass's own for positive finite scales; a batch with an odd scale
	// takes the pass over the gathered records, as the glyf form does
	const bool gather_makes_context = in->gathers_records() && facts.scales_plain;
	// fonts of both kinds: the decoder writes the bytes of its parts' slots and the gather has copied those of its records, so no
	// pass runs when BOTH hold; otherwise the pass runs over the whole batch
	const bool context_made = in->form == FeForm::ResidentMixed ? decode_makes_context && gather_makes_context
	                                                           : decode_makes_context || gather_makes_context;
	if (in->expands_leaves())
		FE_KERNEL(vgsdf_glyf_decode_resident(up.d_parts, in->n_parts, up.d_bytes, (vgsdf::OutlineCmd *)fe.cmds.p, flagw, facts.glyf_max_cap,
		                                     facts.glyf_max_len, decode_makes_context ? (uint8_t *)fe.cmd_open.p : nullptr, st));
	else if (in->form == FeForm::Glyf)
		FE_KERNEL(vgsdf_glyf_decode(up.d_parts, in->n_parts, up.d_bytes, (vgsdf::OutlineCmd *)fe.cmds.p, flagw, facts.glyf_max_cap, facts.glyf_max_len,
		                            decode_makes_context ? (uint8_t *)fe.cmd_open.p : nullptr, st));
	if (in->form == FeForm::Packed)
		FE_KERNEL(vgsdf_outline_context_packed(up.d_kinds, up.d_coords, up.d_dat_off, d.cmd_off, d.scale, n, (vgsdf::OutlineCmd *)fe.cmds.p,
		                                       (uint8_t *)fe.cmd_open.p, flagw, st));
	else if (!context_made)
		FE_KERNEL(vgsdf_outline_context(d.cmds, d.cmd_off, d.scale, n, (uint8_t *)fe.cmd_open.p, flagw, st));
	FE_KERNEL(vgsdf_outline_count(d.cmds, (const uint8_t *)fe.cmd_open.p, n_cmds, d.cmd_off, n, d.scale, d.shift,
	                              (uint32_t *)fe.counts.p, fe.cmd_box.p, (unsigned long long *)fe.cmd_mask.p, flagw, st));
	FE_KERNEL(vgsdf_outline_rings(d.cmds, d.cmd_off, (const uint8_t *)fe.cmd_open.p, d.scale, d.shift, n,
	                              (const uint32_t *)fe.counts.p, (uint32_t *)fe.pt_local.p,
	                              fe.cmd_box.p, (vgsdf::RingRec *)fe.rings.p, (uint32_t *)fe.cmd_ring.p, d.rects,
	                              flagw, st));
	FE_KERNEL(fe_launch_plan(ctx, fe, p.launch_spans));
	if (p.d_names) // ranges with pbf_pre: the entry bytes, where the raster below stores the bitmaps, and the tasks' extents
		FE_KERNEL(fe_launch_entries(ctx, fe, p.spec ? p.d_spec : nullptr, p.spec_cap, true));
	// The front-end's results (rects, totals, positions of the bitmaps) are final once the plan has run: they travel back
	// on a stream of their own, beside the flattening and the raster instead of behind them — the host can have them a
	// good 100 us before the bitmaps (vgsdf_outlines_peek), and the end of the submission loses a copy and its hand-over.
	static const char *early_env = std::getenv("VGSDF_EARLY_COPY"); // (measurement switch: 0 = read-back behind the raster, as in round 2)
	const bool early_copy = !(early_env && early_env[0] == '0');
	if (early_copy) {
		FE_TRY(hipEventRecord(ctx->ev_plan, st));
		FE_TRY(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_plan, 0));
		fe.pend.copy_stream_waits = true;
		FE_TRY(hipMemcpyAsync(fe.h_rects.p, fe.rects_hdr.p, p.rh_bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
		FE_TRY(hipEventRecord(ctx->ev_rects, ctx->copy_stream));
	}
	FE_KERNEL(fe_launch_emit(ctx, fe));
	if (p.spec)
		FE_KERNEL(vgsdf_launch_span_planned((const vgsdf::SpanRec *)fe.tiles.p, p.launch_spans, (const double *)fe.seg.p,
		                                    (const double *)fe.seg.p + 1, (const double *)fe.seg.p + 2, (const double *)fe.seg.p + 3, 4,
		                                    p.d_spec, fe.boxes.p, d.hdr, st));
	if (!early_copy) {
		FE_TRY(hipMemcpyAsync(fe.h_rects.p, fe.rects_hdr.p, p.rh_bytes, hipMemcpyDeviceToHost, st));
		FE_TRY(hipEventRecord(ctx->ev_rects, st));
	}
	static const bool trace_span = std::getenv("VGSDF_TRACE") != nullptr;
	if (trace_span)
		FE_TRY(hipEventRecord(ctx->ev1, st));
	return VGSDF_OK;
}

// The context's front-end state for a new submission: its device made current, the state created on first use, and refused
// while a submission is pending (its kernels may still be reading their input, the staging buffer included)
static int fe_acquire(vgsdf_ctx *ctx, FrontEnd *&fe)
{
	(void)hipSetDevice(ctx->device);
	if (!ctx->fe)
		ctx->fe = new (std::nothrow) FrontEnd();
	if (!ctx->fe) {
		ctx->err = "vgsdf_outlines: out of host memory";
		return VGSDF_E_OOM;
	}
	if (ctx->fe->pend.active) {
		ctx->err = "vgsdf_outlines_submit: the previous submission of this context has not been waited for";
		return VGSDF_E_ARG;
	}
	fe = ctx->fe;
	return VGSDF_OK;
}

// Steps 4 and 5 with the error word's handling around them: everything of a submission that enqueues work.  When a step in
// here fails, what the steps before it enqueued is still running: fe_submit, the one caller, drains it
static int fe_upload_and_enqueue(vgsdf_ctx *ctx, FrontEnd &fe, const FeInput *in, uint32_t n_cmds, uint32_t n_floats, FeUpload &up, FeFacts &facts,
                                 bool validate_under_upload)
{
	// error word of this submission (FrontEnd::flag_slot)
	if (!fe.flags_clean)
		FE_TRY(hipMemsetAsync(fe.flag.p, 0, 32, ctx->stream));
	fe.flags_clean = false; // (until everything below is enqueued: its plan kernel zeroes the other slot)
	fe.flag_slot ^= 1u;
	if (int rc = fe_upload(ctx, fe, in, n_cmds, n_floats, up); rc != VGSDF_OK)
		return rc;
	if (int rc = fe_place_raster(ctx, fe); rc != VGSDF_OK)
		return rc;
	if (validate_under_upload) // the upload is under way: now the walks over the input, before the first kernel that reads it
		if (int rc = fe_validate(ctx, in, n_cmds, facts); rc != VGSDF_OK)
			return rc;
	if (int rc = fe_enqueue(ctx, fe, in, up, facts); rc != VGSDF_OK)
		return rc;
	fe.flags_clean = true; // the plan kernel enqueued above leaves the other slot zeroed for the next submission
	return VGSDF_OK;
}

static int fe_submit(vgsdf_ctx *ctx, const FeInput *in, uint8_t *spec_out, size_t spec_cap)
{
	const double tr0 = fe_now();
	if (!ctx)
		return VGSDF_E_ARG;
	uint32_t n_cmds = 0, n_floats = 0;
	if (int rc = fe_check_args(ctx, in, n_cmds, n_floats); rc != VGSDF_OK)
		return rc;
	const uint32_t n = in->n_glyphs;
	FrontEnd *fe_p = nullptr;
	if (int rc = fe_acquire(ctx, fe_p); rc != VGSDF_OK)
		return rc;
	FrontEnd &fe = *fe_p;
	fe.prepared = false;
	fe.peeked = false;
	fe.n_glyphs = n;
	fe.n_cmds = n_cmds;
	fe.n_segs = 0;
	fe.out_bytes = 0;
	FePending &p = fe.pend;
	p = FePending{};
	p.n = n;
	p.n_cmds = n_cmds;
	p.spec_out = spec_out;
	p.spec_cap = spec_out ? spec_cap : 0;
	p.t0 = tr0;
	if (in->ranges) {
		p.by_ranges = true;
		p.n_tasks = in->ranges->n_tasks;
		p.n_live = in->ranges->n_live;
		p.task_live = in->ranges->task_live;
	}
	if (n == 0) {
		fe.batch.stats = vgsdf_stats{};
		p.active = true;
		p.t1 = fe_now();
		return VGSDF_OK;
	}
	p.t1 = fe_now();
	p.span = uses_span_list(ctx->variant);
	vgsdf::span_policy_from_env(n, p.span_max, p.span_budget);
	FeUpload up = fe_upload_form(in, n_cmds, n_floats);
	if (int rc = fe_reserve(ctx, fe, in, n_cmds, up); rc != VGSDF_OK)
		return rc;
	if (std::getenv("VGSDF_TRACE") != nullptr)
		FE_TRY(hipEventRecord(ctx->ev0, ctx->stream));
	FeFacts facts;
	// (a submission that names its glyphs was validated before its block was gathered, and its offsets are the library's own sums)
	const bool named = in->names_glyphs();
	if (named) {
		facts.glyf_max_cap = in->res_max_cap;
		facts.glyf_max_len = in->res_max_len;
		facts.scales_plain = in->res_scales_plain;
	}
	const bool validate_under_upload = up.mapped != nullptr && !named; // (not one block uploaded by a kernel: validate first, as ever)
	if (!validate_under_upload && !named)
		if (int rc = fe_validate(ctx, in, n_cmds, facts); rc != VGSDF_OK)
			return rc;
	if (int rc = fe_upload_and_enqueue(ctx, fe, in, n_cmds, n_floats, up, facts, validate_under_upload); rc != VGSDF_OK) {
		// A failed submit leaves the caller nothing to wait on (pend stays inactive), so nothing of the caller's memory may
		// be in use when it returns: what was enqueued — the upload kernel reading a page-locked block, a raster storing through
		// the output buffer — is drained here.  The code and the message are those of the step that failed
		(void)hipStreamSynchronize(ctx->stream);
		if (p.copy_stream_waits)
			(void)hipStreamSynchronize(ctx->copy_stream);
		return rc;
	}
	p.active = true;
	return VGSDF_OK;
}

static int fe_wait(vgsdf_ctx *ctx, vgsdf_rect *rects_out, uint64_t *out_bytes, uint64_t *n_segments, int *rendered)
{
	static const bool trace = std::getenv("VGSDF_TRACE") != nullptr;
	if (rendered)
		*rendered = 0;
	if (out_bytes)
		*out_bytes = 0;
	if (n_segments)
		*n_segments = 0;
	if (!ctx)
		return VGSDF_E_ARG;
	if (!ctx->fe || !ctx->fe->pend.active) {
		ctx->err = "vgsdf_outlines_wait: nothing was submitted";
		return VGSDF_E_ARG;
	}
	FrontEnd &fe = *ctx->fe;
	FePending &p = fe.pend;
	const uint32_t n = p.n;
	if (n && !rects_out && !p.by_ranges) { // (a ranges submission's entries come back finished: its caller may not want the rects)
		ctx->err = "vgsdf_outlines: NULL argument";
		return VGSDF_E_ARG;
	}
	p.active = false;
	if (n == 0) {
		fe.drop_union(); // (the batch it belonged to is gone; the union and every render of it ended with a synchronisation)
		fe.prepared = true;
		if (rendered && p.spec_out)
			*rendered = 1;
		return VGSDF_OK;
	}
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	FE_TRY(hipStreamSynchronize(st)); // the one synchronisation of the submission
	FE_TRY(hipEventSynchronize(ctx->ev_rects)); // (the read-back finished long ago: it left right behind the plan)
	fe.drop_union();
	const double tr2 = fe_now();
	if (rects_out)
		std::memcpy(rects_out, fe.h_rects.p, sizeof(vgsdf_rect) * (size_t)n);
	const vgsdf_rect *const rects = (const vgsdf_rect *)fe.h_rects.p;
	vgsdf::PlanHeader hdr;
	std::memcpy(&hdr, (const uint8_t *)fe.h_rects.p + p.hdr_off, sizeof hdr);
	if (hdr.error & 32u) {
		ctx->err = "vgsdf_outlines_ranges: internal error (an index of the block outside what its upload kernel was launched with)";
		return VGSDF_E_HIP;
	}
	if (hdr.error & 16u) {
		ctx->err = "vgsdf_outlines_glyf: a `glyf` entry whose arrays do not fit its bytes (ttf-parser drops such a glyph): record this batch "
		           "with the host's reader";
		return VGSDF_E_GLYF;
	}
	if (hdr.error & 2u) {
		ctx->err = "vgsdf_outlines_prepare: unknown command kind";
		return VGSDF_E_ARG;
	}
	if (hdr.error & 8u) {
		ctx->err = "vgsdf_outlines: dat_off does not match the command kinds";
		return VGSDF_E_ARG;
	}
	if (hdr.error & 4u) {
		ctx->err = "vgsdf_outlines_prepare: internal error (a cubic exceeded its subdivision depth bound)";
		return VGSDF_E_HIP;
	}
	if (hdr.error) {
		ctx->err = "vgsdf_outlines_prepare: a glyph flattens to more than 2^28 points, the batch to more than 2^32 - 1 segments, or a "
		           "bitmap exceeds 2^32 pixels (non-finite or absurd control points?)";
		return VGSDF_E_ARG;
	}
	if (hdr.n_spans > 0x7FFFFFFFu) {
		ctx->err = "vgsdf_outlines_prepare: batch too large (tile count exceeds 2^31-1); split it";
		return VGSDF_E_ARG;
	}
	// second launches when a capacity guess was too small (first batches of a context, unusual fonts)
	const bool replan = hdr.n_spans > fe.tile_cap, reemit = hdr.n_segments > fe.seg_cap;
	if (replan) {
		FE_TRY(fe_ensure_tiles(fe, (size_t)hdr.n_spans + hdr.n_spans / 4 + 1024));
		FE_KERNEL(fe_launch_plan(ctx, fe, 0));
	}
	if (reemit) {
		FE_TRY(fe_ensure_segs(fe, (size_t)hdr.n_segments + hdr.n_segments / 4 + 4096, n));
		FE_KERNEL(fe_launch_emit(ctx, fe));
	}
	const double tr3 = fe_now();

	uint64_t n_pairs = 0, n_pixels = 0;
	for (uint32_t g = 0; g < n; g++) {
		const vgsdf_rect &r = rects[g];
		if (r.has_raster) {
			n_pairs += (uint64_t)r.w * r.h * r.n_segments;
			n_pixels += (uint64_t)r.w * r.h;
		}
	}
	const FeDev d = fe_dev(fe);
	fe.n_segs = (uint32_t)hdr.n_segments;
	fe.out_bytes = hdr.out_bytes;
	vgsdf_dbatch &b = fe.batch;
	b.stats.n_glyphs = n;
	b.stats.n_segments = fe.n_segs;
	b.stats.n_pixels = n_pixels; // (out_bytes is larger with in-place PBF assembly: headers and gaps)
	b.stats.n_pairs = n_pairs;
	b.stats.n_tiles = hdr.n_spans;
	b.stats.alg_bytes = 32 * (uint64_t)fe.n_segs + 32 * (uint64_t)n + n_pixels;
	b.out_bytes = (size_t)fe.out_bytes;
	b.n_main = hdr.n_main;
	b.span_list = p.span;
	b.tile_order = 1; // the device-built list is dispatched in list order
	fe.last_spans = hdr.n_spans;
	const bool done = p.spec && hdr.ok != 0; // the raster behind the plan ran over the whole list
	if (!(done && p.spec_direct))
		FE_TRY(fe.out.ensure(std::max((size_t)fe.out_bytes, done ? p.spec_cap : (size_t)0) + 16));
	b.d_glyphs = d.descs;
	b.d_tiles = (vgsdf::SpanRec *)fe.tiles.p;
	b.d_sx = (double *)fe.seg.p;
	b.d_sy = (double *)fe.seg.p + 1;
	b.d_ex = (double *)fe.seg.p + 2;
	b.d_ey = (double *)fe.seg.p + 3;
	b.seg_stride = 4;
	b.d_out = (uint8_t *)fe.out.p;
	b.d_boxes = p.span ? fe.boxes.p : nullptr;
	fe.prepared = true;
	if (out_bytes)
		*out_bytes = fe.out_bytes;
	if (n_segments)
		*n_segments = fe.n_segs;
	if (p.spec_out && fe.out_bytes <= p.spec_cap) {
		int rc = VGSDF_OK;
		if (done) {
			if (!p.spec_direct && fe.out_bytes) { // pageable destination: the raster wrote the device buffer
				FE_TRY(hipMemcpyAsync(p.spec_out, p.d_spec, (size_t)fe.out_bytes, hipMemcpyDeviceToHost, st));
				FE_TRY(hipStreamSynchronize(st));
			}
		} else if (fe.out_bytes) { // a guess was too small (first batch of a context, a batch unlike the last one)
			if (p.d_names) // (the entries with the raster, into the device buffer the download takes them from)
				FE_KERNEL(fe_launch_entries(ctx, fe, b.d_out, (size_t)fe.out_bytes, false));
			rc = vgsdf_batch_launch(ctx, &fe.batch);
			if (rc == VGSDF_OK)
				rc = vgsdf_batch_download(ctx, &fe.batch, p.spec_out);
		}
		if (rc != VGSDF_OK)
			return rc;
		if (rendered)
			*rendered = 1;
	}
	if (trace) {
		float span_ms = 0;
		if (hipEventElapsedTime(&span_ms, ctx->ev0, ctx->ev1) == hipSuccess)
			std::fprintf(stderr, "[vgsdf] device span of the submission (upload ... last kernel, events on the kernel stream): %.1f us\n", span_ms * 1e3);
		else
			(void)hipGetLastError();
	}
	if (trace && p.spec_out)
		std::fprintf(stderr, "[vgsdf] one submission%s, %s destination\n", done ? "" : " (guess too small: second launches)",
		             p.spec_direct ? "page-locked" : "pageable");
	if (trace)
		std::fprintf(stderr, "[vgsdf] prepare: validate %.3f ms, submit ... read-back %.3f ms, second launches%s%s %.3f ms, host %.3f ms\n",
		             (p.t1 - p.t0) * 1e3, (tr2 - p.t1) * 1e3, replan ? " (plan)" : "", reemit ? " (emit)" : "", (tr3 - tr2) * 1e3,
		             (fe_now() - tr3) * 1e3);
	return VGSDF_OK;
}

// The block of a submission that names its glyphs, gathered in the context's page-locked staging buffer in the layout of
// its kind of font: the caller's arrays, the running sum(s), the fonts' device addresses.  Points `f` into it
// Mixed: fonts of both kinds in the list (ResidentBlockLayout): per glyph the slots of either kind, leaves of the glyf kind alone
template <class Layout, bool Mixed = false>
static int fe_gather_named(vgsdf_ctx *ctx, FrontEnd &fe, const vgsdf_outlines_resident *in, FeInput &f)
{
	constexpr bool glyf = std::is_same_v<Layout, vgsdf::ResidentBlockLayout>; // (else: command fonts, CommandBlockLayout)
	static_assert(glyf || !Mixed, "a list of both kinds takes the glyf form's block");
	const uint32_t n = in->n_glyphs;
	const bool pbf = in->pbf_fix != nullptr;
	const Layout at(n, in->n_fonts, pbf);
	FE_TRY(fe.h_stage.ensure(at.bytes + 16));
	uint8_t *hb = (uint8_t *)fe.h_stage.p;
	std::memcpy(hb + at.scale, in->scale, 8 * (size_t)n);
	std::memcpy(hb + at.shift_x, in->shift_x, 8 * (size_t)n);
	std::memcpy(hb + at.glyph_id, in->glyph_id, 2 * (size_t)n);
	std::memcpy(hb + at.font_of, in->font_of, 2 * (size_t)n);
	if (pbf) {
		std::memcpy(hb + at.pbf_pre, in->pbf_pre, 4 * (size_t)n);
		std::memcpy(hb + at.pbf_fix, in->pbf_fix, n);
	}
	std::memset(hb + at.arrays_end, 0, at.fonts - at.arrays_end);
	// per glyph one table read and one addition: the running sum of command slots (command fonts: of commands) — and, for
	// glyf fonts, the same again for the leaves that become the submission's parts
	uint32_t *cmd_off = (uint32_t *)(hb + at.cmd_off), *part_off = nullptr;
	if constexpr (glyf)
		part_off = (uint32_t *)(hb + at.part_off);
	uint64_t cmds = 0, parts = 0;
	for (uint32_t g = 0; g < n; g++) {
		const vgsdf_font &ft = *in->fonts[in->font_of[g]];
		const uint32_t id = in->glyph_id[g];
		cmd_off[g] = (uint32_t)cmds;
		cmds += ft.slots[id];
		if constexpr (glyf) {
			part_off[g] = (uint32_t)parts;
			if (!Mixed || !ft.commands)
				parts += ft.leaf_off[id + 1] - ft.leaf_off[id];
		}
		if (cmds > 0x7FFFFFFFull) {
			ctx->err = Mixed  ? "vgsdf_outlines_resident_mixed: more than 2^31 - 1 command slots and commands in one submission; split it"
			           : glyf ? "vgsdf_outlines_resident: more than 2^31 - 1 command slots in one submission; split it"
			                : "vgsdf_outlines_resident: more than 2^31 - 1 commands in one submission; split it";
			return VGSDF_E_ARG;
		}
		f.res_scales_plain = f.res_scales_plain && in->scale[g] > 0.0 && in->scale[g] < HUGE_VAL;
	}
	cmd_off[n] = (uint32_t)cmds;
	if constexpr (Mixed) {
		part_off[n] = (uint32_t)parts;
		vgsdf::MixedFontRef *refs = (vgsdf::MixedFontRef *)(hb + at.fonts);
		for (uint32_t k = 0; k < in->n_fonts; k++) {
			const vgsdf_font &ft = *in->fonts[k];
			refs[k] = mixed_font_ref(ft);
			if (!ft.commands) { // (the decoder's LDS: from the fonts it reads)
				f.res_max_cap = std::max(f.res_max_cap, ft.max_cap);
				f.res_max_len = std::max(f.res_max_len, ft.max_len);
			}
		}
	} else if constexpr (glyf) {
		part_off[n] = (uint32_t)parts;
		vgsdf::ResidentFontRef *refs = (vgsdf::ResidentFontRef *)(hb + at.fonts);
		for (uint32_t k = 0; k < in->n_fonts; k++) {
			refs[k] = in->fonts[k]->ref;
			f.res_max_cap = std::max(f.res_max_cap, in->fonts[k]->max_cap);
			f.res_max_len = std::max(f.res_max_len, in->fonts[k]->max_len);
		}
	} else {
		vgsdf::CommandFontRef *refs = (vgsdf::CommandFontRef *)(hb + at.fonts);
		for (uint32_t k = 0; k < in->n_fonts; k++)
			refs[k] = in->fonts[k]->cref;
	}
	f.form = Mixed ? FeForm::ResidentMixed : glyf ? FeForm::ResidentGlyf : FeForm::ResidentCommands;
	f.cmd_off = cmd_off;
	f.scale = (const double *)(hb + at.scale);
	f.shift_x = (const double *)(hb + at.shift_x);
	f.pbf_pre = pbf ? (const uint32_t *)(hb + at.pbf_pre) : nullptr;
	f.pbf_fix = pbf ? hb + at.pbf_fix : nullptr;
	f.n_parts = (uint32_t)parts;
	f.n_fonts = in->n_fonts;
	return VGSDF_OK;
}

static FeInput fe_input(const vgsdf_outlines *in)
{
	FeInput f;
	f.n_glyphs = in->n_glyphs;
	f.cmd_off = in->cmd_off;
	f.scale = in->scale;
	f.shift_x = in->shift_x;
	f.cmds = in->cmds;
	return f;
}

extern "C" {

int vgsdf_outlines_prepare(vgsdf_ctx *ctx, const vgsdf_outlines *in, vgsdf_rect *rects_out, uint64_t *out_bytes,
                           uint64_t *n_segments)
{
	if (ctx && in && in->n_glyphs && !rects_out) {
		ctx->err = "vgsdf_outlines_prepare: NULL argument";
		return VGSDF_E_ARG;
	}
	if (ctx && !in) {
		ctx->err = "vgsdf_outlines: NULL argument";
		return VGSDF_E_ARG;
	}
	FeInput f;
	if (in)
		f = fe_input(in);
	const int rc = fe_submit(ctx, in ? &f : nullptr, nullptr, 0);
	return rc != VGSDF_OK ? rc : fe_wait(ctx, rects_out, out_bytes, n_segments, nullptr);
}

int vgsdf_outlines_submit(vgsdf_ctx *ctx, const vgsdf_outlines *in, uint8_t *out_bitmaps, size_t out_capacity)
{
	FeInput f;
	if (in)
		f = fe_input(in);
	return fe_submit(ctx, in ? &f : nullptr, out_bitmaps, out_bitmaps ? out_capacity : 0);
}

int vgsdf_outlines_submit_packed(vgsdf_ctx *ctx, const vgsdf_outlines_packed *in, uint8_t *out_bitmaps, size_t out_capacity)
{
	FeInput f;
	if (in) {
		f.n_glyphs = in->n_glyphs;
		f.cmd_off = in->cmd_off;
		f.scale = in->scale;
		f.shift_x = in->shift_x;
		f.dat_off = in->dat_off;
		f.kinds = in->kinds;
		f.coords = in->coords;
		f.pbf_pre = in->pbf_pre;
		f.pbf_fix = in->pbf_fix;
		f.form = FeForm::Packed;
	}
	return fe_submit(ctx, in ? &f : nullptr, out_bitmaps, out_bitmaps ? out_capacity : 0);
}

int vgsdf_outlines_submit_glyf(vgsdf_ctx *ctx, const vgsdf_outlines_glyf *in, uint8_t *out_bitmaps, size_t out_capacity)
{
	FeInput f;
	if (in) {
		f.n_glyphs = in->n_glyphs;
		f.cmd_off = in->cmd_off;
		f.scale = in->scale;
		f.shift_x = in->shift_x;
		f.pbf_pre = in->pbf_pre;
		f.pbf_fix = in->pbf_fix;
		f.form = FeForm::Glyf;
		f.parts = in->parts;
		f.n_parts = in->n_parts;
		f.bytes = in->bytes;
		f.n_bytes = in->n_bytes;
	}
	return fe_submit(ctx, in ? &f : nullptr, out_bitmaps, out_bitmaps ? out_capacity : 0);
}

// ---- glyphs named by (font, glyph id) of resident fonts (resident_fonts.cpp) ----

uint64_t vgsdf_outlines_resident_upload_bytes(const vgsdf_ctx *ctx) { return ctx && ctx->fe ? ctx->fe->resident_upload_bytes : 0; }

// both entry points of the form; mixed: fonts of both kinds may stand in the list (vgsdf_outlines_submit_resident_mixed)
static int fe_submit_named(vgsdf_ctx *ctx, const vgsdf_outlines_resident *in, uint8_t *out_bitmaps, size_t out_capacity, bool mixed)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || (in->n_glyphs && (!in->fonts || !in->font_of || !in->glyph_id || !in->scale || !in->shift_x))) {
		ctx->err = "vgsdf_outlines_resident: NULL argument";
		return VGSDF_E_ARG;
	}
	if ((in->pbf_pre == nullptr) != (in->pbf_fix == nullptr)) {
		ctx->err = "vgsdf_outlines: pbf_pre and pbf_fix come together (packed and glyf forms only)";
		return VGSDF_E_ARG;
	}
	const uint32_t n = in->n_glyphs;
	FeInput f;
	f.form = mixed ? FeForm::ResidentMixed : FeForm::ResidentGlyf;
	f.n_glyphs = n;
	if (n == 0)
		return fe_submit(ctx, &f, out_bitmaps, out_bitmaps ? out_capacity : 0);
	if (in->n_fonts == 0 || in->n_fonts > 0x10000u) {
		ctx->err = "vgsdf_outlines_resident: n_fonts must be 1 .. 65536";
		return VGSDF_E_ARG;
	}
	for (uint32_t k = 0; k < in->n_fonts; k++)
		if (!in->fonts[k] || in->fonts[k]->device != ctx->device) {
			ctx->err = "vgsdf_outlines_resident: a NULL font, or a font of another device than the context's";
			return VGSDF_E_ARG;
		}
	const bool commands = in->fonts[0]->commands;
	for (uint32_t k = 1; k < in->n_fonts && !mixed; k++)
		if (in->fonts[k]->commands != commands) {
			ctx->err = "vgsdf_outlines_resident: fonts of both kinds (vgsdf_font_create and vgsdf_font_create_commands) in one submission";
			return VGSDF_E_ARG;
		}
	// every name before anything is touched
	for (uint32_t g = 0; g < n; g++)
		if (in->font_of[g] >= in->n_fonts || in->glyph_id[g] >= in->fonts[in->font_of[g]]->n_glyph_ids) {
			ctx->err = "vgsdf_outlines_resident: font_of past n_fonts, or a glyph id past its face";
			return VGSDF_E_ARG;
		}
	FrontEnd *fe = nullptr; // (pending: its upload kernel may still be reading the staging block)
	if (int rc = fe_acquire(ctx, fe); rc != VGSDF_OK)
		return rc;
	if (int rc = mixed      ? fe_gather_named<vgsdf::ResidentBlockLayout, true>(ctx, *fe, in, f)
	             : commands ? fe_gather_named<vgsdf::CommandBlockLayout>(ctx, *fe, in, f)
	                        : fe_gather_named<vgsdf::ResidentBlockLayout>(ctx, *fe, in, f);
	    rc != VGSDF_OK)
		return rc;
	return fe_submit(ctx, &f, out_bitmaps, out_bitmaps ? out_capacity : 0);
}

int vgsdf_outlines_submit_resident(vgsdf_ctx *ctx, const vgsdf_outlines_resident *in, uint8_t *out_bitmaps, size_t out_capacity)
{
	return fe_submit_named(ctx, in, out_bitmaps, out_capacity, false);
}

int vgsdf_outlines_submit_resident_mixed(vgsdf_ctx *ctx, const vgsdf_outlines_resident *in, uint8_t *out_bitmaps, size_t out_capacity)
{
	return fe_submit_named(ctx, in, out_bitmaps, out_capacity, true);
}

// ---- code-point ranges of resident families (resident_families.cpp, vgsdf_family_create) ----

// The host's share is O(tasks): per task two bisections of its family's code points and two reads of each prefix sum; per
// submission the totals that size buffers and grids.  The block it uploads (upload_layout.h, RangesBlockLayout) holds a record
// per task that maps a glyph, per family and per font; the upload kernel names the glyphs (family_upload_kernel.inc)
int vgsdf_outlines_submit_ranges(vgsdf_ctx *ctx, const vgsdf_outlines_ranges *in, uint8_t *out_bitmaps, size_t out_capacity)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || (in->n_families && !in->families) || (in->n_tasks && (!in->family_of || !in->first || !in->last))) {
		ctx->err = "vgsdf_outlines_ranges: NULL argument";
		return VGSDF_E_ARG;
	}
	// the families: one device, one kind; their fonts, list after list, are the block's fonts
	uint64_t n_fonts = 0;
	uint32_t max_cap = 0, max_len = 0;
	bool scales_plain = true;
	for (uint32_t k = 0; k < in->n_families; k++) {
		const vgsdf_family *fm = in->families[k];
		if (!fm || fm->device != ctx->device || fm->commands != in->families[0]->commands || fm->mixed != in->families[0]->mixed) {
			ctx->err = "vgsdf_outlines_ranges: a NULL family, a family of another device than the context's, or families of more than one "
			           "kind (over fonts from vgsdf_font_create, from vgsdf_font_create_commands, mixed) in one submission";
			return VGSDF_E_ARG;
		}
		n_fonts += fm->fonts.size();
		max_cap = std::max(max_cap, fm->max_cap);
		max_len = std::max(max_len, fm->max_len);
		scales_plain = scales_plain && fm->scales_plain;
	}
	if (n_fonts > 0x10000u) {
		ctx->err = "vgsdf_outlines_ranges: more than 65536 fonts over the families";
		return VGSDF_E_ARG;
	}
	for (uint32_t t = 0; t < in->n_tasks; t++)
		if (in->family_of[t] >= in->n_families || in->first[t] > in->last[t]) {
			ctx->err = "vgsdf_outlines_ranges: family_of past n_families, or first > last";
			return VGSDF_E_ARG;
		}
	const bool commands = in->n_families ? in->families[0]->commands : false;
	const bool mixed = in->n_families ? in->families[0]->mixed : false; // (a third kind: its font lists hold both, reference by reference)
	const bool pbf = in->pbf_pre != nullptr;
	FrontEnd *fe = nullptr; // (pending: its upload kernel may still be reading the staging block)
	if (int rc = fe_acquire(ctx, fe); rc != VGSDF_OK)
		return rc;
	// the tasks: entry range, glyph base, command base, part base
	FeRanges rg;
	rg.n_tasks = in->n_tasks;
	rg.n_families = in->n_families;
	rg.task_live.resize(in->n_tasks);
	std::vector<vgsdf::RangeTask> tasks;
	tasks.reserve(in->n_tasks);
	uint64_t glyphs = 0, cmds = 0, parts = 0;
	for (uint32_t t = 0; t < in->n_tasks; t++) {
		const vgsdf_family &fm = *in->families[in->family_of[t]];
		const auto e0 = std::lower_bound(fm.code_point.begin(), fm.code_point.end(), in->first[t]) - fm.code_point.begin();
		const auto e1 = std::upper_bound(fm.code_point.begin(), fm.code_point.end(), in->last[t]) - fm.code_point.begin();
		rg.task_live[t] = (uint32_t)tasks.size();
		if (e1 <= e0)
			continue; // (maps nothing: not in the block; its extent is empty, at the next task's begin)
		vgsdf::RangeTask rt{};
		rt.glyph_base = (uint32_t)glyphs;
		rt.n_glyphs = (uint32_t)(e1 - e0);
		rt.entry_first = (uint32_t)e0;
		rt.family = in->family_of[t];
		rt.cmd_rel = (uint32_t)cmds - (uint32_t)fm.cmd_pre[e0];
		rt.part_rel = (uint32_t)parts - (uint32_t)fm.leaf_pre[e0];
		rt.pbf_pre = pbf ? in->pbf_pre[t] : 0u;
		tasks.push_back(rt);
		glyphs += rt.n_glyphs;
		cmds += fm.cmd_pre[e1] - fm.cmd_pre[e0];
		parts += fm.leaf_pre[e1] - fm.leaf_pre[e0];
		if (cmds > 0x7FFFFFFFull || glyphs > 0x7FFFFFFFull) {
			ctx->err = "vgsdf_outlines_ranges: more than 2^31 - 1 command slots (or glyphs) in one submission; split it";
			return VGSDF_E_ARG;
		}
	}
	rg.n_live = (uint32_t)tasks.size();
	rg.n_cmds = (uint32_t)cmds;
	// the block, in the context's page-locked staging buffer
	const vgsdf::RangesBlockLayout at(rg.n_live, in->n_families, (size_t)n_fonts);
	FE_TRY(fe->h_stage.ensure(at.bytes + 16));
	uint8_t *hb = (uint8_t *)fe->h_stage.p;
	if (!tasks.empty())
		std::memcpy(hb + at.tasks, tasks.data(), sizeof(vgsdf::RangeTask) * tasks.size());
	vgsdf::FamilyRef *frefs = (vgsdf::FamilyRef *)(hb + at.families);
	uint32_t font_base = 0;
	for (uint32_t k = 0; k < in->n_families; k++) {
		const vgsdf_family &fm = *in->families[k];
		vgsdf::FamilyRef r{};
		r.table = (uint64_t)(uintptr_t)fm.table.p;
		r.n_entries = (uint32_t)fm.code_point.size();
		r.font_base = font_base;
		r.n_fonts = (uint32_t)fm.fonts.size();
		r.cp_base = fm.plane << 16;
		frefs[k] = r;
		for (const vgsdf_font *ft : fm.fonts) { // (both references are 32 bytes)
			if (mixed)
				((vgsdf::MixedFontRef *)(hb + at.fonts))[font_base++] = mixed_font_ref(*ft);
			else if (commands)
				((vgsdf::CommandFontRef *)(hb + at.fonts))[font_base++] = ft->cref;
			else
				((vgsdf::ResidentFontRef *)(hb + at.fonts))[font_base++] = ft->ref;
		}
	}
	rg.block = hb;
	rg.block_bytes = at.bytes;
	FeInput f;
	f.form = mixed ? FeForm::ResidentMixed : commands ? FeForm::ResidentCommands : FeForm::ResidentGlyf;
	f.n_glyphs = (uint32_t)glyphs;
	f.n_parts = (uint32_t)parts;
	f.n_fonts = (uint32_t)n_fonts;
	f.res_max_cap = max_cap;
	f.res_max_len = max_len;
	f.res_scales_plain = scales_plain;
	f.ranges = &rg;
	if (pbf) { // (never read on the host in a named form: they say that the submission assembles PBF in place)
		f.pbf_pre = (const uint32_t *)hb;
		f.pbf_fix = hb;
	}
	fe->resident_upload_bytes = at.bytes;
	return fe_submit(ctx, &f, out_bitmaps, out_bitmaps ? out_capacity : 0);
}

int vgsdf_outlines_task_extents(vgsdf_ctx *ctx, uint64_t *begin)
{
	if (!ctx || !begin)
		return VGSDF_E_ARG;
	FrontEnd *fe = ctx->fe;
	if (!fe || !(fe->prepared || (fe->pend.active && fe->peeked)) || !fe->pend.by_ranges || (fe->pend.n && !fe->pend.d_names)) {
		ctx->err = "vgsdf_outlines_task_extents: the last batch was not a ranges submission with pbf_pre that has been peeked at or waited for";
		return VGSDF_E_ARG;
	}
	const FePending &p = fe->pend;
	if (p.n) { // (peeked at, not yet waited for: a batch in error has no extents, and says so in wait)
		vgsdf::PlanHeader hdr;
		std::memcpy(&hdr, (const uint8_t *)fe->h_rects.p + p.hdr_off, sizeof hdr);
		if (hdr.error) {
			ctx->err = "vgsdf_outlines_task_extents: the batch is in error (vgsdf_outlines_wait reports it)";
			return VGSDF_E_ARG;
		}
	}
	const uint64_t *live = p.n ? (const uint64_t *)((const uint8_t *)fe->h_rects.p + p.begin_off) : nullptr;
	for (uint32_t t = 0; t <= p.n_tasks; t++)
		begin[t] = live ? live[t < p.n_tasks ? p.task_live[t] : p.n_live] : 0;
	return VGSDF_OK;
}

int vgsdf_outlines_wait(vgsdf_ctx *ctx, vgsdf_rect *rects_out, uint64_t *out_bytes, uint64_t *n_segments, int *rendered)
{
	return fe_wait(ctx, rects_out, out_bytes, n_segments, rendered);
}

int vgsdf_outlines_peek(vgsdf_ctx *ctx, vgsdf_rect *rects_out, uint64_t *out_bytes, int *in_place)
{
	if (out_bytes)
		*out_bytes = 0;
	if (in_place)
		*in_place = 0;
	if (!ctx)
		return VGSDF_E_ARG;
	if (!ctx->fe || !ctx->fe->pend.active) {
		ctx->err = "vgsdf_outlines_peek: nothing was submitted";
		return VGSDF_E_ARG;
	}
	FrontEnd &fe = *ctx->fe;
	const FePending &p = fe.pend;
	if (p.n == 0)
		return VGSDF_OK;
	if (!rects_out && !p.by_ranges) {
		ctx->err = "vgsdf_outlines: NULL argument";
		return VGSDF_E_ARG;
	}
	(void)hipSetDevice(ctx->device);
	FE_TRY(hipEventSynchronize(ctx->ev_rects));
	if (rects_out)
		std::memcpy(rects_out, fe.h_rects.p, sizeof(vgsdf_rect) * (size_t)p.n);
	vgsdf::PlanHeader hdr;
	std::memcpy(&hdr, (const uint8_t *)fe.h_rects.p + p.hdr_off, sizeof hdr);
	if (out_bytes)
		*out_bytes = hdr.out_bytes;
	// the raster behind the plan runs over the whole list and stores through the caller's own (page-locked) buffer
	if (in_place)
		*in_place = p.spec && p.spec_direct && hdr.ok != 0 && hdr.error == 0;
	fe.peeked = true;
	return VGSDF_OK;
}

int vgsdf_outlines_pbf_positions(vgsdf_ctx *ctx, uint64_t *bitmap_at)
{
	if (!ctx || !bitmap_at)
		return VGSDF_E_ARG;
	if (!ctx->fe || !(ctx->fe->prepared || (ctx->fe->pend.active && ctx->fe->peeked)) || ctx->fe->pend.d_pbf_fix == nullptr) {
		ctx->err = "vgsdf_outlines_pbf_positions: the last batch was not submitted with pbf_pre / pbf_fix";
		return VGSDF_E_ARG;
	}
	const FePending &p = ctx->fe->pend;
	std::memcpy(bitmap_at, (const uint8_t *)ctx->fe->h_rects.p + p.at_off, 8 * (size_t)p.n);
	return VGSDF_OK;
}

int vgsdf_outlines_render_into(vgsdf_ctx *ctx, const vgsdf_outlines *in, vgsdf_rect *rects_out, uint8_t *out_bitmaps,
                               size_t out_capacity, uint64_t *out_bytes, uint64_t *n_segments, int *rendered)
{
	if (ctx && (!rendered || (in && in->n_glyphs && !rects_out))) {
		ctx->err = "vgsdf_outlines_render_into: NULL argument";
		return VGSDF_E_ARG;
	}
	FeInput f;
	if (in)
		f = fe_input(in);
	const int rc = fe_submit(ctx, in ? &f : nullptr, out_bitmaps, out_bitmaps ? out_capacity : 0);
	return rc != VGSDF_OK ? rc : fe_wait(ctx, rects_out, out_bytes, n_segments, rendered);
}

int vgsdf_outlines_render(vgsdf_ctx *ctx, uint8_t *out_bitmaps)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!ctx->fe || !ctx->fe->prepared) {
		ctx->err = "vgsdf_outlines_render: call vgsdf_outlines_prepare first";
		return VGSDF_E_ARG;
	}
	FrontEnd &fe = *ctx->fe;
	if (fe.n_glyphs == 0 || fe.out_bytes == 0)
		return VGSDF_OK;
	if (!out_bitmaps) {
		ctx->err = "vgsdf_outlines_render: NULL output";
		return VGSDF_E_ARG;
	}
	static const bool trace = std::getenv("VGSDF_TRACE") != nullptr;
	const double t0 = fe_now();
	(void)hipSetDevice(ctx->device);
	FE_TRY(fe.out.ensure((size_t)fe.out_bytes + 16)); // (the one-submission form may have rendered elsewhere)
	fe.batch.d_out = (uint8_t *)fe.out.p;
	if (fe.pend.d_names) // (a ranges submission with pbf_pre: its entries with its bitmaps)
		FE_KERNEL(fe_launch_entries(ctx, fe, fe.batch.d_out, (size_t)fe.out_bytes, false));
	int rc = vgsdf_batch_launch(ctx, &fe.batch);
	if (rc != VGSDF_OK)
		return rc;
	rc = vgsdf_batch_download(ctx, &fe.batch, out_bitmaps);
	if (trace)
		std::fprintf(stderr, "[vgsdf] render: launch+D2H+sync %.3f ms\n", (fe_now() - t0) * 1e3);
	return rc;
}

int vgsdf_outlines_union(vgsdf_ctx *ctx, uint8_t *state, uint64_t *n_segments)
{
	if (n_segments)
		*n_segments = 0;
	if (!ctx)
		return VGSDF_E_ARG;
	if (!ctx->fe || !ctx->fe->prepared) {
		ctx->err = "vgsdf_outlines_union: call vgsdf_outlines_prepare first";
		return VGSDF_E_ARG;
	}
	FrontEnd &fe = *ctx->fe;
	if (fe.n_glyphs == 0)
		return VGSDF_OK;
	// the prepared batch's segments, descriptors, work list and chunk boxes are replaced; its output buffer and, with in-place
	// PBF assembly, the bitmap positions in the descriptors' out_off stay
	vgsdf_dbatch *u = nullptr;
	if (int rc = union_resident(ctx, "vgsdf_outlines_union", &fe.batch, &u, state, /*own_output=*/false); rc != VGSDF_OK)
		return rc;
	fe.drop_union(); // (a second union of the same batch read the first one's arena)
	fe.unioned = u;
	vgsdf_dbatch &b = fe.batch;
	b.stats = u->stats;
	b.d_glyphs = u->d_glyphs, b.d_tiles = u->d_tiles;
	b.d_sx = u->d_sx, b.d_sy = u->d_sy, b.d_ex = u->d_ex, b.d_ey = u->d_ey;
	b.seg_stride = u->seg_stride;
	b.d_boxes = u->span_list ? u->d_boxes : nullptr;
	b.n_main = u->n_main, b.span_list = u->span_list, b.tile_order = u->tile_order;
	fe.n_segs = (uint32_t)u->stats.n_segments;
	if (n_segments)
		*n_segments = fe.n_segs;
	return VGSDF_OK;
}

int vgsdf_outlines_segments(vgsdf_ctx *ctx, uint32_t *seg_off, double *sx, double *sy, double *ex, double *ey)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!ctx->fe || !ctx->fe->prepared) {
		ctx->err = "vgsdf_outlines_segments: call vgsdf_outlines_prepare first";
		return VGSDF_E_ARG;
	}
	FrontEnd &fe = *ctx->fe;
	if (fe.unioned && seg_off) // (after vgsdf_outlines_union: the union's segments)
		return vgsdf_batch_segments_read(ctx, fe.unioned, seg_off, sx, sy, ex, ey);
	(void)hipSetDevice(ctx->device);
	std::vector<vgsdf::GlyphDesc> hd;
	if (fe.n_glyphs && seg_off) {
		hd.resize(fe.n_glyphs);
		FE_TRY(hipMemcpyAsync(hd.data(), fe.descs.p, sizeof(vgsdf::GlyphDesc) * (size_t)fe.n_glyphs, hipMemcpyDeviceToHost, ctx->stream));
	}
	std::vector<double> rec;
	if (fe.n_segs && sx && sy && ex && ey) {
		rec.resize(4 * (size_t)fe.n_segs);
		FE_TRY(hipMemcpyAsync(rec.data(), fe.seg.p, 32 * (size_t)fe.n_segs, hipMemcpyDeviceToHost, ctx->stream));
	}
	FE_TRY(hipStreamSynchronize(ctx->stream));
	for (uint32_t g = 0; g < (uint32_t)hd.size(); g++) {
		seg_off[g] = hd[g].seg_off;
		seg_off[g + 1] = hd[g].seg_off + hd[g].n_seg;
	}
	for (size_t i = 0; i * 4 < rec.size(); i++) { // records -> the four arrays of the C ABI
		sx[i] = rec[4 * i];
		sy[i] = rec[4 * i + 1];
		ex[i] = rec[4 * i + 2];
		ey[i] = rec[4 * i + 3];
	}
	return VGSDF_OK;
}

} // extern "C"
