// resident_fonts.cpp — the stores behind vgsdf_font: a face's outlines uploaded once, as `glyf` leaves (vgsdf_font_create)
// (vgsdf_font_create_tables: walked on the device from a face's loca and glyf) or as expanded commands (vgsdf_font_create_commands; vgsdf_font_create_charstrings: decoded on the device from a CFF face's charstrings).  Submissions that name their glyphs read them
// (outline_front_end.cpp, vgsdf_outlines_submit_resident).  And the families over them (vgsdf_family_create): a font id's table
// code point -> (font, glyph id, advance, scale, shift_x) on host and device, for submissions that name code-point ranges
// (vgsdf_outlines_submit_ranges).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>

#include "charstring_kernels.h"
#include "charstring_limits.h"
#include "family_table_kernels.h"
#include "glyf_table_kernels.h"
#include "glyf_table_limits.h"
#include "outline_kernels.h"
#include "resident_fonts.h"
#include "work_plan.h"

namespace {
// a failed HIP call of a constructor: the entry point's name, what it was doing and the runtime's words
int font_hip_error(vgsdf_ctx *ctx, const char *entry, const char *what, hipError_t e)
{
	ctx->err = std::string(entry) + ": " + what + ": " + hipGetErrorString(e);
	return e == hipErrorOutOfMemory ? VGSDF_E_OOM : VGSDF_E_HIP;
}
struct ScratchBuf : DevBuf { // device memory for the duration of one call
	~ScratchBuf() { release(); }
};
} // namespace

extern "C" {

int vgsdf_font_create(vgsdf_ctx *ctx, const vgsdf_font_desc *in, vgsdf_font **out)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || !in->leaf_off || (in->n_leaves && !in->leaves) || (in->n_bytes && !in->bytes)) {
		ctx->err = "vgsdf_font_create: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	const uint32_t n = in->n_glyph_ids;
	if (n > 0x10000u || (in->n_bytes & 3u) || in->leaf_off[0] != 0 || in->leaf_off[n] != in->n_leaves) {
		ctx->err = "vgsdf_font_create: more than 65536 glyph ids, n_bytes not a multiple of 4, or leaf_off does not run from 0 to n_leaves";
		return VGSDF_E_ARG;
	}
	std::unique_ptr<vgsdf_font> f(new (std::nothrow) vgsdf_font());
	if (!f) {
		ctx->err = "vgsdf_font_create: out of host memory";
		return VGSDF_E_OOM;
	}
	f->slots.assign(n, 0);
	for (uint32_t g = 0; g < n; g++) {
		const uint32_t l0 = in->leaf_off[g], l1 = in->leaf_off[g + 1];
		if (l1 < l0 || l1 > in->n_leaves) {
			ctx->err = "vgsdf_font_create: leaf_off not ascending";
			return VGSDF_E_ARG;
		}
		uint64_t slots = 0;
		for (uint32_t i = l0; i < l1; i++) {
			const vgsdf_glyf_part &lf = in->leaves[i];
			if (lf.cmd_at != slots || (lf.byte_off & 3u) || lf.byte_off > in->n_bytes || lf.byte_len > in->n_bytes - lf.byte_off ||
			    lf.n_contours == 0 || lf.plain > 1u) {
				ctx->err = "vgsdf_font_create: the leaves of a glyph must tile its command slots from 0 in order, with 4-aligned byte ranges "
				           "inside `bytes`, n_contours > 0 and plain 0 or 1";
				return VGSDF_E_ARG;
			}
			slots += lf.cmd_cap;
			if (slots > 0x7FFFFFFFull) {
				ctx->err = "vgsdf_font_create: a glyph of more than 2^31 - 1 command slots";
				return VGSDF_E_ARG;
			}
			f->max_cap = std::max(f->max_cap, lf.cmd_cap);
			f->max_len = std::max(f->max_len, lf.byte_len);
		}
		f->slots[g] = (uint32_t)slots;
	}
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->n_leaves = in->n_leaves;
	f->n_bytes = in->n_bytes;
	f->leaf_off.assign(in->leaf_off, in->leaf_off + n + 1);
	(void)hipSetDevice(ctx->device);
	const size_t leaves_bytes = sizeof(vgsdf_glyf_part) * (size_t)in->n_leaves; // (a multiple of 16)
	const size_t bytes_at = leaves_bytes, off_at = align_up(bytes_at + in->n_bytes, 16), total = off_at + 4 * ((size_t)n + 1);
	if (hipError_t e = f->store.ensure(total + 16); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create", "hipMalloc", e);
	uint8_t *d = (uint8_t *)f->store.p;
	hipError_t e = leaves_bytes ? hipMemcpyAsync(d, in->leaves, leaves_bytes, hipMemcpyHostToDevice, ctx->stream) : hipSuccess;
	if (e == hipSuccess && in->n_bytes)
		e = hipMemcpyAsync(d + bytes_at, in->bytes, in->n_bytes, hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(d + off_at, in->leaf_off, 4 * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess)
		e = hipStreamSynchronize(ctx->stream); // the arrays are on the device when the call returns: every context may name the font
	if (e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create", "upload", e);
	f->ref.leaves = (uint64_t)(uintptr_t)d;
	f->ref.bytes = (uint64_t)(uintptr_t)(d + bytes_at);
	f->ref.leaf_off = (uint64_t)(uintptr_t)(d + off_at);
	*out = f.release();
	return VGSDF_OK;
}

int vgsdf_font_create_commands(vgsdf_ctx *ctx, const vgsdf_font_cmds_desc *in, vgsdf_font **out)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || !in->cmd_off || !in->dat_off || (in->n_cmds && !in->kinds) || (in->n_floats && !in->coords)) {
		ctx->err = "vgsdf_font_create_commands: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	const uint32_t n = in->n_glyph_ids, n_cmds = in->n_cmds;
	// (the store: 28-byte records | cmd_off | a context byte per record)
	if (n > 0x10000u || 29ull * n_cmds + 4ull * (n + 1) > 0xFFFFFFFCull || 4ull * in->n_floats > 0xFFFFFFFCull) {
		ctx->err = "vgsdf_font_create_commands: more than 65536 glyph ids, or a store (29 bytes per command, 4 per glyph id) or "
		           "coordinates past what 32-bit offsets address";
		return VGSDF_E_ARG;
	}
	if (in->cmd_off[0] != 0 || in->cmd_off[n] != n_cmds || in->dat_off[0] != 0 || in->dat_off[n] != in->n_floats) {
		ctx->err = "vgsdf_font_create_commands: cmd_off / dat_off do not run from 0 to n_cmds / n_floats";
		return VGSDF_E_ARG;
	}
	std::unique_ptr<vgsdf_font> f(new (std::nothrow) vgsdf_font());
	if (!f) {
		ctx->err = "vgsdf_font_create_commands: out of host memory";
		return VGSDF_E_OOM;
	}
	// everything a submission of these commands would be checked for per render, once: the offsets (they bound every read of
	// the loop below), the kinds, and the coordinates every glyph's kinds carry against its dat_off range
	f->slots.assign(n, 0);
	for (uint32_t g = 0; g < n; g++) {
		const uint32_t c0 = in->cmd_off[g], c1 = in->cmd_off[g + 1], d0 = in->dat_off[g], d1 = in->dat_off[g + 1];
		if (c1 < c0 || c1 > n_cmds || d1 < d0 || d1 > in->n_floats) {
			ctx->err = "vgsdf_font_create_commands: cmd_off / dat_off not ascending";
			return VGSDF_E_ARG;
		}
		uint64_t floats = 0;
		uint32_t bad_kind = 0;
		for (uint32_t c = c0; c < c1; c++) {
			const uint32_t k = in->kinds[c];
			bad_kind |= k > vgsdf::CMD_CLOSE;
			floats += k <= vgsdf::CMD_LINE ? 2u : (k == vgsdf::CMD_QUAD ? 4u : (k == vgsdf::CMD_CURVE ? 6u : 0u));
		}
		if (bad_kind || floats != (uint64_t)(d1 - d0)) {
			ctx->err = bad_kind ? "vgsdf_font_create_commands: unknown command kind"
			                    : "vgsdf_font_create_commands: a glyph's dat_off range does not match its command kinds";
			return VGSDF_E_ARG;
		}
		f->slots[g] = c1 - c0;
	}
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->commands = true;
	(void)hipSetDevice(ctx->device);
	// the store: records | cmd_off | context bytes.  Beside it, for the duration of this call, what the packed form's context
	// pass reads: scale (1: the bytes then say "ring open" and nothing else) | dat_off | coords | kinds | its error word
	const size_t off_at = sizeof(vgsdf::OutlineCmd) * (size_t)n_cmds, open_at = off_at + 4 * ((size_t)n + 1), total = open_at + n_cmds;
	const size_t t_dat = 8 * (size_t)n, t_coords = t_dat + 4 * ((size_t)n + 1), t_kinds = t_coords + 4 * (size_t)in->n_floats,
	             t_flag = align_up(t_kinds + n_cmds, 16), t_total = t_flag + 16;
	ScratchBuf tmp;
	if (hipError_t e = f->store.ensure(total + 16); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_commands", "hipMalloc", e);
	if (hipError_t e = tmp.ensure(t_total); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_commands", "hipMalloc", e);
	uint8_t *d = (uint8_t *)f->store.p, *t = (uint8_t *)tmp.p;
	hipStream_t st = ctx->stream;
	const std::vector<double> ones(n, 1.0);
	auto copy = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
	hipError_t e = copy(d + off_at, in->cmd_off, 4 * ((size_t)n + 1));
	if (e == hipSuccess)
		e = copy(t, ones.data(), 8 * (size_t)n);
	if (e == hipSuccess)
		e = copy(t + t_dat, in->dat_off, 4 * ((size_t)n + 1));
	if (e == hipSuccess)
		e = copy(t + t_coords, in->coords, 4 * (size_t)in->n_floats);
	if (e == hipSuccess)
		e = copy(t + t_kinds, in->kinds, n_cmds);
	if (e == hipSuccess)
		e = hipMemsetAsync(t + t_flag, 0, 16, st);
	if (e == hipSuccess && n_cmds)
		e = (hipError_t)vgsdf_outline_context_packed(t + t_kinds, (const float *)(t + t_coords), (const uint32_t *)(t + t_dat),
		                                             (const uint32_t *)(d + off_at), (const double *)t, n, (vgsdf::OutlineCmd *)d, d + open_at,
		                                             (uint32_t *)(t + t_flag), st);
	uint32_t flag = 0;
	if (e == hipSuccess)
		e = hipMemcpyAsync(&flag, t + t_flag, 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st); // the store is complete when the call returns: every context may name the font
	if (e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_commands", "upload", e);
	if (flag) { // (what the walk above has ruled out, said by the pass itself)
		ctx->err = "vgsdf_font_create_commands: the device's context pass refused the commands";
		return VGSDF_E_ARG;
	}
	f->n_cmds = n_cmds;
	f->cref.cmds = (uint64_t)(uintptr_t)d;
	f->cref.cmd_off = (uint64_t)(uintptr_t)(d + off_at);
	f->cref.open = (uint64_t)(uintptr_t)(d + open_at);
	*out = f.release();
	return VGSDF_OK;
}

} // extern "C"

namespace {
// the blend sets of a CFF2 description (vgsdf_font_charstrings2_desc)
struct BlendSets {
	uint32_t n_sets, n_factors;
	const uint8_t *set_ok;
	const uint32_t *set_off;
	const float *factors;
};
constexpr uint32_t kChunkGlyphIds = 16384; // CFF2: glyph ids per launch, which bounds the workspace of the operand stack

// vgsdf_font_create_charstrings_within (blend == nullptr) and vgsdf_font_create_charstrings2_within: one sequence
int create_charstrings(vgsdf_ctx *ctx, const vgsdf_font_charstrings_desc *in, const BlendSets *blend, uint64_t max_store_bytes,
                       vgsdf_font **out, uint64_t *store_bytes)
{
	const char *name = blend ? "vgsdf_font_create_charstrings2" : "vgsdf_font_create_charstrings";
	const std::string entry = std::string(name) + ": ";
	if (!in || !out || !in->cs_off || !in->gsubr_off || !in->lsubr_first || !in->lsubr_off || (in->n_bytes && !in->bytes) ||
	    (in->n_fds > 1 && !in->fd_of)) {
		ctx->err = entry + "NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (store_bytes)
		*store_bytes = 0;
	const uint32_t n = in->n_glyph_ids, n_bytes = in->n_bytes;
	if (blend) {
		if (in->n_fds != 1 || in->fd_of) {
			ctx->err = entry + "n_fds must be 1 and fd_of NULL";
			return VGSDF_E_ARG;
		}
		if (blend->n_sets > 0x10000u || (blend->n_sets && (!blend->set_ok || !blend->set_off)) || (blend->n_factors && !blend->factors)) {
			ctx->err = entry + "more than 65536 blend sets, or a NULL array of them";
			return VGSDF_E_ARG;
		}
		if (blend->n_sets && blend->set_off[0] != 0) {
			ctx->err = entry + "set_off does not start at 0";
			return VGSDF_E_ARG;
		}
		for (uint32_t s = 0; s < blend->n_sets; s++)
			if (blend->set_off[s + 1] < blend->set_off[s] || blend->set_off[s + 1] - blend->set_off[s] > (uint32_t)vg::kCharstringMaxRegions ||
			    blend->set_off[s + 1] > blend->n_factors) {
				ctx->err = entry + "set_off not ascending, a set of more than 64 factors, or one ending past n_factors";
				return VGSDF_E_ARG;
			}
		for (uint32_t i = 0; i < blend->n_factors; i++)
			if (!std::isfinite(blend->factors[i])) {
				ctx->err = entry + "a factor that is not finite";
				return VGSDF_E_ARG;
			}
	}
	if (n == 0 || n > 0x10000u || (n_bytes & 3u) || n_bytes > 0xFFFFFFF0u || in->n_gsubrs > 0xFFFFu || in->n_fds == 0 || in->n_fds > 256u) {
		ctx->err = entry + "glyph ids not 1 .. 65536, n_bytes not a multiple of 4 (or past 2^32 - 16), more than "
		           "65535 global subroutines, or Font DICTs not 1 .. 256";
		return VGSDF_E_ARG;
	}
	// every range the device will read, before anything runs
	auto ascends_inside = [&](const uint32_t *off, size_t count) {
		for (size_t i = 0; i < count; i++)
			if (off[i + 1] < off[i])
				return false;
		return off[count] <= n_bytes;
	};
	if (in->lsubr_first[0] != 0) {
		ctx->err = entry + "lsubr_first does not start at 0";
		return VGSDF_E_ARG;
	}
	for (uint32_t k = 0; k < in->n_fds; k++)
		if (in->lsubr_first[k + 1] < in->lsubr_first[k] || in->lsubr_first[k + 1] - in->lsubr_first[k] > 0xFFFFu) {
			ctx->err = entry + "lsubr_first not ascending, or a Font DICT of more than 65535 local subroutines";
			return VGSDF_E_ARG;
		}
	const uint32_t n_lsubrs = in->lsubr_first[in->n_fds];
	if (!ascends_inside(in->cs_off, n) || !ascends_inside(in->gsubr_off, in->n_gsubrs) || !ascends_inside(in->lsubr_off, n_lsubrs)) {
		ctx->err = entry + "cs_off, gsubr_off or lsubr_off not ascending, or ending past n_bytes";
		return VGSDF_E_ARG;
	}
	if (in->fd_of)
		for (uint32_t g = 0; g < n; g++)
			if (in->fd_of[g] >= in->n_fds) {
				ctx->err = entry + "an fd_of past n_fds";
				return VGSDF_E_ARG;
			}
	std::unique_ptr<vgsdf_font> f(new (std::nothrow) vgsdf_font());
	if (!f) {
		ctx->err = entry + "out of host memory";
		return VGSDF_E_OOM;
	}
	ctx->charstring_ms[0] = ctx->charstring_ms[1] = 0.0f;
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	// the description on the device, for the duration of this call:
	// bytes | cs_off | gsubr_off | lsubr_first | lsubr_off | counts (commands, coordinates per glyph id) | flags | fd_of
	// CFF2, behind them: set_off | factors | set_ok
	const size_t a_cs = align_up(n_bytes, 16), a_gs = a_cs + 4 * ((size_t)n + 1), a_lf = a_gs + 4 * ((size_t)in->n_gsubrs + 1),
	             a_lo = a_lf + 4 * ((size_t)in->n_fds + 1), a_counts = a_lo + 4 * ((size_t)n_lsubrs + 1), a_flags = a_counts + 8 * (size_t)n,
	             a_fd = a_flags + 16, a_fd_end = a_fd + (in->fd_of ? n : 0);
	const uint32_t n_sets = blend ? blend->n_sets : 0, n_factors = blend ? blend->n_factors : 0;
	const size_t a_so = align_up(a_fd_end, 16), a_fac = a_so + 4 * ((size_t)n_sets + 1), a_ok = a_fac + 4 * (size_t)n_factors,
	             a_total = blend ? a_ok + n_sets : a_fd_end;
	ScratchBuf face_buf, tmp;
	struct Events {
		hipEvent_t e[3] = {nullptr, nullptr, nullptr};
		~Events()
		{
			for (hipEvent_t ev : e)
				if (ev)
					(void)hipEventDestroy(ev);
		}
	} ev;
	for (hipEvent_t &e : ev.e)
		if (hipError_t err = hipEventCreate(&e); err != hipSuccess)
			return font_hip_error(ctx, name, "hipEventCreate", err);
	if (hipError_t e = face_buf.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)face_buf.p;
	auto copy = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
	hipError_t e = copy(a, in->bytes, n_bytes);
	if (e == hipSuccess)
		e = copy(a + a_cs, in->cs_off, 4 * ((size_t)n + 1));
	if (e == hipSuccess)
		e = copy(a + a_gs, in->gsubr_off, 4 * ((size_t)in->n_gsubrs + 1));
	if (e == hipSuccess)
		e = copy(a + a_lf, in->lsubr_first, 4 * ((size_t)in->n_fds + 1));
	if (e == hipSuccess)
		e = copy(a + a_lo, in->lsubr_off, 4 * ((size_t)n_lsubrs + 1));
	if (e == hipSuccess && in->fd_of)
		e = copy(a + a_fd, in->fd_of, n);
	if (e == hipSuccess && n_sets)
		e = copy(a + a_so, blend->set_off, 4 * ((size_t)n_sets + 1));
	if (e == hipSuccess && n_factors)
		e = copy(a + a_fac, blend->factors, 4 * (size_t)n_factors);
	if (e == hipSuccess && n_sets)
		e = copy(a + a_ok, blend->set_ok, n_sets);
	if (e == hipSuccess)
		e = hipMemsetAsync(a + a_flags, 0, 16, st);
	vgsdf::Charstrings2Ref face{}; // (a version 1 face: its CharstringsRef part)
	face.words = (const uint32_t *)a;
	face.cs_off = (const uint32_t *)(a + a_cs);
	face.gsubr_off = (const uint32_t *)(a + a_gs);
	face.lsubr_first = (const uint32_t *)(a + a_lf);
	face.lsubr_off = (const uint32_t *)(a + a_lo);
	face.fd_of = in->fd_of ? a + a_fd : nullptr;
	face.n_glyph_ids = n;
	face.n_gsubrs = in->n_gsubrs;
	if (blend) {
		face.set_ok = a + a_ok;
		face.set_off = (const uint32_t *)(a + a_so);
		face.factors = (const float *)(a + a_fac);
		face.n_sets = n_sets;
		face.spill_stride = (std::min(kChunkGlyphIds, n) + 63u) & ~63u;
		// the context's workspace: the operand slots past the decoder's LDS window, for one launch (at most 465 x 4 x 16384 B)
		const size_t want = 4 * (size_t)(vg::kCharstringMaxOperands2 - vg::kCharstringWindow) * face.spill_stride;
		if (want > ctx->charstring_spill_bytes) {
			if (ctx->charstring_spill)
				(void)hipFree(ctx->charstring_spill); // (nothing in flight reads it: every call ends synchronised)
			ctx->charstring_spill = nullptr;
			ctx->charstring_spill_bytes = 0;
			if (hipError_t err = hipMalloc(&ctx->charstring_spill, want); err != hipSuccess) {
				ctx->charstring_spill = nullptr;
				return font_hip_error(ctx, name, "hipMalloc", err);
			}
			ctx->charstring_spill_bytes = want;
		}
		face.spill = (float *)ctx->charstring_spill;
	}
	// the two passes; CFF2: in launches of at most kChunkGlyphIds glyph ids, one after the other over the workspace
	auto run_pass = [&](bool emit, const uint32_t *cmd_off, const uint32_t *dat_off, uint8_t *kinds, float *coords) -> hipError_t {
		uint32_t *counts = (uint32_t *)(a + a_counts), *flags = (uint32_t *)(a + a_flags);
		if (!blend)
			return (hipError_t)(emit ? vgsdf_charstring_emit(&face, cmd_off, dat_off, kinds, coords, flags, st)
			                         : vgsdf_charstring_count(&face, counts, flags, st));
		for (uint32_t g0 = 0; g0 < n; g0 += kChunkGlyphIds) {
			vgsdf::Charstrings2Ref part = face;
			part.cs_off = face.cs_off + g0;
			part.n_glyph_ids = std::min(kChunkGlyphIds, n - g0);
			const hipError_t err = (hipError_t)(emit ? vgsdf_charstring2_emit(&part, cmd_off + g0, dat_off + g0, kinds, coords, flags, st)
			                                         : vgsdf_charstring2_count(&part, counts + 2 * (size_t)g0, flags, st));
			if (err != hipSuccess)
				return err;
		}
		return hipSuccess;
	};
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[0], st);
	if (e == hipSuccess)
		e = run_pass(false, nullptr, nullptr, nullptr, nullptr);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[1], st);
	std::vector<uint32_t> counts(2 * (size_t)n);
	uint32_t flags = 0;
	if (e == hipSuccess)
		e = hipMemcpyAsync(counts.data(), a + a_counts, 8 * (size_t)n, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipMemcpyAsync(&flags, a + a_flags, 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st);
	if (e != hipSuccess)
		return font_hip_error(ctx, name, "count pass", e);
	(void)hipEventElapsedTime(&ctx->charstring_ms[0], ev.e[0], ev.e[1]);
	if (flags) {
		ctx->err = entry + (flags & vgsdf::CS_FLAG_SEAC ? "a glyph whose endchar takes the seac form" : "a glyph past VGSDF_CHARSTRING_MAX_TOKENS");
		return VGSDF_E_GLYF;
	}
	// the store's layout from the counts: what vgsdf_font_create_commands is given by its caller
	std::vector<uint32_t> cmd_off((size_t)n + 1), dat_off((size_t)n + 1);
	uint64_t cmds = 0, floats = 0;
	f->slots.assign(n, 0);
	for (uint32_t g = 0; g < n; g++) {
		cmd_off[g] = (uint32_t)cmds, dat_off[g] = (uint32_t)floats;
		f->slots[g] = counts[2 * (size_t)g];
		cmds += counts[2 * (size_t)g], floats += counts[2 * (size_t)g + 1];
		if (29ull * cmds + 4ull * (n + 1) > 0xFFFFFFFCull || 4ull * floats > 0xFFFFFFFCull) {
			ctx->err = entry + "a store (29 bytes per command, 4 per glyph id) or coordinates past what 32-bit "
			           "offsets address";
			return VGSDF_E_GLYF;
		}
	}
	const uint32_t n_cmds = (uint32_t)cmds, n_floats = (uint32_t)floats;
	cmd_off[n] = n_cmds, dat_off[n] = n_floats;
	if (store_bytes)
		*store_bytes = 29ull * n_cmds + 4ull * (n + 1);
	if (29ull * n_cmds + 4ull * (n + 1) > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->commands = true;
	f->n_cmds = n_cmds;
	// store and temporaries as vgsdf_font_create_commands lays them out (the same sizes: the same vgsdf_font_device_bytes)
	const size_t off_at = sizeof(vgsdf::OutlineCmd) * (size_t)n_cmds, open_at = off_at + 4 * ((size_t)n + 1), total = open_at + n_cmds;
	const size_t t_dat = 8 * (size_t)n, t_coords = t_dat + 4 * ((size_t)n + 1), t_kinds = t_coords + 4 * (size_t)n_floats,
	             t_flag = align_up(t_kinds + n_cmds, 16), t_total = t_flag + 16;
	if (hipError_t err = f->store.ensure(total + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	if (hipError_t err = tmp.ensure(t_total); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	uint8_t *d = (uint8_t *)f->store.p, *t = (uint8_t *)tmp.p;
	const std::vector<double> ones(n, 1.0);
	e = copy(d + off_at, cmd_off.data(), 4 * ((size_t)n + 1));
	if (e == hipSuccess)
		e = copy(t, ones.data(), 8 * (size_t)n);
	if (e == hipSuccess)
		e = copy(t + t_dat, dat_off.data(), 4 * ((size_t)n + 1));
	if (e == hipSuccess)
		e = hipMemsetAsync(t + t_flag, 0, 16, st);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[1], st);
	// (cmd_off is read from the store, where it stays; dat_off from the temporaries, as the context pass below reads them)
	if (e == hipSuccess && n_cmds)
		e = run_pass(true, (const uint32_t *)(d + off_at), (const uint32_t *)(t + t_dat), t + t_kinds, (float *)(t + t_coords));
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[2], st);
	if (e == hipSuccess && n_cmds)
		e = (hipError_t)vgsdf_outline_context_packed(t + t_kinds, (const float *)(t + t_coords), (const uint32_t *)(t + t_dat),
		                                             (const uint32_t *)(d + off_at), (const double *)t, n, (vgsdf::OutlineCmd *)d, d + open_at,
		                                             (uint32_t *)(t + t_flag), st);
	uint32_t flag = 0;
	if (e == hipSuccess)
		e = hipMemcpyAsync(&flag, t + t_flag, 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipMemcpyAsync(&flags, a + a_flags, 4, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st); // the store is complete when the call returns: every context may name the font
	if (e != hipSuccess)
		return font_hip_error(ctx, name, "emit pass", e);
	if (n_cmds)
		(void)hipEventElapsedTime(&ctx->charstring_ms[1], ev.e[1], ev.e[2]);
	if (flag || flags) { // (the two passes walk one text over the same bytes: said by the passes themselves)
		ctx->err = entry + "the emit pass did not match the count pass, or the context pass refused the commands";
		return VGSDF_E_HIP;
	}
	f->cref.cmds = (uint64_t)(uintptr_t)d;
	f->cref.cmd_off = (uint64_t)(uintptr_t)(d + off_at);
	f->cref.open = (uint64_t)(uintptr_t)(d + open_at);
	*out = f.release();
	return VGSDF_OK;
}

} // namespace

extern "C" {

int vgsdf_font_create_charstrings(vgsdf_ctx *ctx, const vgsdf_font_charstrings_desc *in, vgsdf_font **out)
{
	return vgsdf_font_create_charstrings_within(ctx, in, ~0ull, out, nullptr);
}

int vgsdf_font_create_charstrings_within(vgsdf_ctx *ctx, const vgsdf_font_charstrings_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                         uint64_t *store_bytes)
{
	if (!ctx)
		return VGSDF_E_ARG;
	return create_charstrings(ctx, in, nullptr, max_store_bytes, out, store_bytes);
}

int vgsdf_font_create_charstrings2(vgsdf_ctx *ctx, const vgsdf_font_charstrings2_desc *in, vgsdf_font **out)
{
	return vgsdf_font_create_charstrings2_within(ctx, in, ~0ull, out, nullptr);
}

int vgsdf_font_create_charstrings2_within(vgsdf_ctx *ctx, const vgsdf_font_charstrings2_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                          uint64_t *store_bytes)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in) {
		ctx->err = "vgsdf_font_create_charstrings2: NULL argument";
		return VGSDF_E_ARG;
	}
	const BlendSets blend{in->n_sets, in->n_factors, in->set_ok, in->set_off, in->factors};
	return create_charstrings(ctx, &in->charstrings, &blend, max_store_bytes, out, store_bytes);
}

void vgsdf_font_charstrings_kernel_ms(const vgsdf_ctx *ctx, float ms[2])
{
	if (ms)
		ms[0] = ctx ? ctx->charstring_ms[0] : 0.0f, ms[1] = ctx ? ctx->charstring_ms[1] : 0.0f;
}

int vgsdf_font_commands_read(vgsdf_ctx *ctx, const vgsdf_font *font, uint32_t *n_glyph_ids, uint32_t *n_cmds, uint32_t *cmd_off,
                             void *records, uint8_t *context)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!font || !font->commands || font->device != ctx->device) {
		ctx->err = "vgsdf_font_commands_read: no font, a font from vgsdf_font_create, or a font of another device than the context's";
		return VGSDF_E_ARG;
	}
	if (n_glyph_ids)
		*n_glyph_ids = font->n_glyph_ids;
	if (n_cmds)
		*n_cmds = font->n_cmds;
	(void)hipSetDevice(ctx->device);
	const size_t n = font->n_cmds;
	if (cmd_off)
		HIP_TRY(ctx, hipMemcpy(cmd_off, (const void *)(uintptr_t)font->cref.cmd_off, 4 * ((size_t)font->n_glyph_ids + 1), hipMemcpyDeviceToHost));
	if (records && n)
		HIP_TRY(ctx, hipMemcpy(records, (const void *)(uintptr_t)font->cref.cmds, sizeof(vgsdf::OutlineCmd) * n, hipMemcpyDeviceToHost));
	if (context && n)
		HIP_TRY(ctx, hipMemcpy(context, (const void *)(uintptr_t)font->cref.open, n, hipMemcpyDeviceToHost));
	return VGSDF_OK;
}

int vgsdf_font_create_tables(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *in, vgsdf_font **out)
{
	return vgsdf_font_create_tables_within(ctx, in, ~0ull, out, nullptr);
}

int vgsdf_font_create_tables_within(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                    uint64_t *needed)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || (in->n_loca_bytes && !in->loca) || (in->n_glyf_bytes && !in->glyf)) {
		ctx->err = "vgsdf_font_create_tables: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (needed)
		*needed = 0;
	ctx->glyf_tables_ms[0] = ctx->glyf_tables_ms[1] = 0.0f;
	const uint32_t n = in->num_glyphs;
	// (tables of 4 GiB or more cannot be stated: the lengths are 32-bit)
	// (loca_entries <= num_glyphs + 1: every glyph id a component can resolve to is then one of the face's, with a place in the store)
	if (n > 0xFFFFu || in->loca_long > 1u || (uint64_t)in->loca_entries * (in->loca_long ? 4u : 2u) > in->n_loca_bytes || in->loca_entries > n + 1) {
		ctx->err = "vgsdf_font_create_tables: more than 65535 glyphs, loca_long not 0 or 1, or more loca entries than the loca bytes hold or than num_glyphs + 1";
		return VGSDF_E_ARG;
	}
	std::unique_ptr<vgsdf_font> f(new (std::nothrow) vgsdf_font());
	if (!f) {
		ctx->err = "vgsdf_font_create_tables: out of host memory";
		return VGSDF_E_OOM;
	}
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	struct Events {
		hipEvent_t e[3] = {nullptr, nullptr, nullptr};
		~Events()
		{
			for (hipEvent_t ev : e)
				if (ev)
					(void)hipEventDestroy(ev);
		}
	} ev;
	for (hipEvent_t &e : ev.e)
		if (hipError_t err = hipEventCreate(&e); err != hipSuccess)
			return font_hip_error(ctx, "vgsdf_font_create_tables", "hipEventCreate", err);
	// the description on the device, for the duration of this call: loca | glyf | counts (4 per glyph id) | flags | byte_at
	const size_t a_glyf = align_up(in->n_loca_bytes, 16), a_counts = align_up(a_glyf + in->n_glyf_bytes, 16),
	             a_flags = a_counts + 4 * (size_t)vgsdf::kGlyfTableCounts * n, a_at = a_flags + 4 * (size_t)vgsdf::GLYF_FLAG_WORDS,
	             a_total = a_at + 4 * ((size_t)n + 1);
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_tables", "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	auto copy = [&](void *dst, const void *src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess; };
	hipError_t e = copy(a, in->loca, in->n_loca_bytes);
	if (e == hipSuccess)
		e = copy(a + a_glyf, in->glyf, in->n_glyf_bytes);
	if (e == hipSuccess)
		e = hipMemsetAsync(a + a_flags, 0, 4 * (size_t)vgsdf::GLYF_FLAG_WORDS, st);
	vgsdf::GlyfTablesRef face{};
	face.loca = a, face.glyf = a + a_glyf;
	face.glyf_len = in->n_glyf_bytes, face.loca_entries = in->loca_entries, face.loca_long = in->loca_long, face.n_glyph_ids = n;
	uint32_t *d_counts = (uint32_t *)(a + a_counts), *d_flags = (uint32_t *)(a + a_flags), *d_at = (uint32_t *)(a + a_at);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[0], st);
	if (e == hipSuccess && n)
		e = (hipError_t)vgsdf_glyf_tables_count(&face, d_counts, d_flags, st);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[1], st);
	// the counts and, behind them, the flag words: one read-back
	std::vector<uint32_t> got((size_t)vgsdf::kGlyfTableCounts * n + vgsdf::GLYF_FLAG_WORDS);
	if (e == hipSuccess)
		e = hipMemcpyAsync(got.data(), d_counts, 4 * got.size(), hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st);
	if (e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_tables", "count pass", e);
	(void)hipEventElapsedTime(&ctx->glyf_tables_ms[0], ev.e[0], ev.e[1]);
	const uint32_t *fl = got.data() + (size_t)vgsdf::kGlyfTableCounts * n;
	if (fl[vgsdf::GLYF_FLAG_BUDGET] || fl[vgsdf::GLYF_FLAG_SLOTS]) {
		ctx->err = fl[vgsdf::GLYF_FLAG_BUDGET] ? "vgsdf_font_create_tables: a glyph past VGSDF_GLYF_MAX_COMPONENTS"
		                                       : "vgsdf_font_create_tables: a glyph of more than 2^26 command slots";
		return VGSDF_E_GLYF;
	}
	// the running sums, and the bounds of the host's table (glyf_table_limits.h)
	std::vector<uint32_t> byte_at((size_t)n + 1);
	f->leaf_off.assign((size_t)n + 1, 0);
	f->slots.assign(n, 0);
	uint64_t n_bytes = 0, n_leaves = 0, slot_sum = 0;
	for (uint32_t g = 0; g < n; g++) {
		const uint32_t *c = got.data() + (size_t)vgsdf::kGlyfTableCounts * g;
		byte_at[g] = (uint32_t)n_bytes, f->leaf_off[g] = (uint32_t)n_leaves;
		f->slots[g] = c[2];
		n_bytes += align_up(c[0], 4), n_leaves += c[1], slot_sum += c[2];
		if (n_bytes > vg::kResidentMaxBytes || n_leaves > vg::kResidentMaxLeaves || slot_sum > vg::kResidentMaxSlotSum) {
			ctx->err = "vgsdf_font_create_tables: more than 2^22 leaves, a store past 2^32 - 4 bytes, or command slots that sum past 2^32 - 1";
			return VGSDF_E_GLYF;
		}
		f->max_cap = std::max(f->max_cap, c[3]); // (every simple entry a leaf names is some glyph id's own)
		f->max_len = std::max(f->max_len, c[0]);
	}
	byte_at[n] = (uint32_t)n_bytes, f->leaf_off[n] = (uint32_t)n_leaves;
	// the store as vgsdf_font_create lays it out (the same size: the same vgsdf_font_device_bytes)
	const size_t leaves_bytes = sizeof(vgsdf_glyf_part) * (size_t)n_leaves;
	const size_t bytes_at = leaves_bytes, off_at = align_up(bytes_at + n_bytes, 16), total = off_at + 4 * ((size_t)n + 1);
	if (needed)
		*needed = total;
	if (total > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->n_leaves = (uint32_t)n_leaves;
	f->n_bytes = (uint32_t)n_bytes;
	if (hipError_t err = f->store.ensure(total + 16); err != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_tables", "hipMalloc", err);
	uint8_t *d = (uint8_t *)f->store.p;
	e = copy(d + off_at, f->leaf_off.data(), 4 * ((size_t)n + 1));
	if (e == hipSuccess)
		e = copy(d_at, byte_at.data(), 4 * ((size_t)n + 1));
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[1], st);
	if (e == hipSuccess && n)
		e = (hipError_t)vgsdf_glyf_tables_emit(&face, (const uint32_t *)(d + off_at), d_at, d, d + bytes_at, d_flags, st);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[2], st);
	uint32_t flags[vgsdf::GLYF_FLAG_WORDS] = {};
	if (e == hipSuccess)
		e = hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st); // the store is complete when the call returns: every context may name the font
	if (e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_tables", "emit pass", e);
	(void)hipEventElapsedTime(&ctx->glyf_tables_ms[1], ev.e[1], ev.e[2]);
	if (flags[vgsdf::GLYF_FLAG_EMIT]) { // (the two passes walk one text over the same bytes: said by the pass itself)
		ctx->err = "vgsdf_font_create_tables: the emit pass did not match the count pass";
		return VGSDF_E_HIP;
	}
	f->ref.leaves = (uint64_t)(uintptr_t)d;
	f->ref.bytes = (uint64_t)(uintptr_t)(d + bytes_at);
	f->ref.leaf_off = (uint64_t)(uintptr_t)(d + off_at);
	*out = f.release();
	return VGSDF_OK;
}

void vgsdf_font_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2])
{
	if (ms)
		ms[0] = ctx ? ctx->glyf_tables_ms[0] : 0.0f, ms[1] = ctx ? ctx->glyf_tables_ms[1] : 0.0f;
}

int vgsdf_font_read(vgsdf_ctx *ctx, const vgsdf_font *font, uint32_t *n_glyph_ids, uint32_t *n_leaves, uint32_t *n_bytes,
                    uint32_t *leaf_off, vgsdf_glyf_part *leaves, uint8_t *bytes)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!font || font->commands || font->device != ctx->device) {
		ctx->err = "vgsdf_font_read: no font, a command font, or a font of another device than the context's";
		return VGSDF_E_ARG;
	}
	if (n_glyph_ids)
		*n_glyph_ids = font->n_glyph_ids;
	if (n_leaves)
		*n_leaves = font->n_leaves;
	if (n_bytes)
		*n_bytes = font->n_bytes;
	(void)hipSetDevice(ctx->device);
	if (leaf_off)
		HIP_TRY(ctx, hipMemcpy(leaf_off, (const void *)(uintptr_t)font->ref.leaf_off, 4 * ((size_t)font->n_glyph_ids + 1), hipMemcpyDeviceToHost));
	if (leaves && font->n_leaves)
		HIP_TRY(ctx, hipMemcpy(leaves, (const void *)(uintptr_t)font->ref.leaves, sizeof(vgsdf_glyf_part) * (size_t)font->n_leaves, hipMemcpyDeviceToHost));
	if (bytes && font->n_bytes)
		HIP_TRY(ctx, hipMemcpy(bytes, (const void *)(uintptr_t)font->ref.bytes, font->n_bytes, hipMemcpyDeviceToHost));
	return VGSDF_OK;
}

int vgsdf_font_free(vgsdf_ctx *ctx, vgsdf_font *font)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!font)
		return VGSDF_OK;
	if (font->device != ctx->device) {
		ctx->err = "vgsdf_font_free: the font lives on another device than the context";
		return VGSDF_E_ARG;
	}
	(void)hipSetDevice(ctx->device);
	delete font;
	return VGSDF_OK;
}

uint64_t vgsdf_font_device_bytes(const vgsdf_font *font) { return font ? (uint64_t)font->store.cap : 0; }

int vgsdf_family_create(vgsdf_ctx *ctx, const vgsdf_family_desc *in, vgsdf_family **out)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || !in->fonts ||
	    (in->n_entries && (!in->code_point || !in->font_of || !in->glyph_id || !in->advance || !in->scale || !in->shift_x))) {
		ctx->err = "vgsdf_family_create: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	const uint32_t n = in->n_entries;
	if (in->n_fonts == 0 || in->n_fonts > 0x10000u || n > 0x10000u) {
		ctx->err = "vgsdf_family_create: n_fonts must be 1 .. 65536 and n_entries at most 65536";
		return VGSDF_E_ARG;
	}
	for (uint32_t k = 0; k < in->n_fonts; k++)
		if (!in->fonts[k] || in->fonts[k]->device != ctx->device || in->fonts[k]->commands != in->fonts[0]->commands) {
			ctx->err = "vgsdf_family_create: a NULL font, a font of another device than the context's, or fonts of both kinds";
			return VGSDF_E_ARG;
		}
	for (uint32_t i = 0; i < n; i++)
		if ((i && in->code_point[i] <= in->code_point[i - 1]) || in->font_of[i] >= in->n_fonts ||
		    in->glyph_id[i] >= in->fonts[in->font_of[i]]->n_glyph_ids) {
			ctx->err = "vgsdf_family_create: code points not strictly ascending, font_of past n_fonts, or a glyph id past its face";
			return VGSDF_E_ARG;
		}
	std::unique_ptr<vgsdf_family> f(new (std::nothrow) vgsdf_family());
	if (!f) {
		ctx->err = "vgsdf_family_create: out of host memory";
		return VGSDF_E_OOM;
	}
	f->device = ctx->device;
	f->commands = in->fonts[0]->commands;
	f->fonts.assign(in->fonts, in->fonts + in->n_fonts);
	for (const vgsdf_font *ft : f->fonts) {
		f->max_cap = std::max(f->max_cap, ft->max_cap);
		f->max_len = std::max(f->max_len, ft->max_len);
	}
	f->code_point.assign(in->code_point, in->code_point + n);
	f->font_of.assign(in->font_of, in->font_of + n);
	f->glyph_id.assign(in->glyph_id, in->glyph_id + n);
	f->advance.assign(in->advance, in->advance + n);
	f->scale.assign(in->scale, in->scale + n);
	f->shift_x.assign(in->shift_x, in->shift_x + n);
	f->pbf_fix.resize(n);
	f->cmd_pre.assign((size_t)n + 1, 0);
	f->leaf_pre.assign((size_t)n + 1, 0);
	auto varint_len = [](uint32_t v) { return v < 0x80u ? 1u : v < 0x4000u ? 2u : v < 0x200000u ? 3u : v < 0x10000000u ? 4u : 5u; };
	for (uint32_t i = 0; i < n; i++) {
		const vgsdf_font &ft = *f->fonts[f->font_of[i]];
		const uint32_t id = f->glyph_id[i];
		f->cmd_pre[i + 1] = f->cmd_pre[i] + ft.slots[id];
		f->leaf_pre[i + 1] = f->leaf_pre[i] + (ft.commands ? 0u : ft.leaf_off[id + 1] - ft.leaf_off[id]);
		f->pbf_fix[i] = (uint8_t)((1u + varint_len(f->code_point[i])) | ((1u + varint_len(f->advance[i])) << 4));
		f->scales_plain = f->scales_plain && f->scale[i] > 0.0 && f->scale[i] < HUGE_VAL;
	}
	// the device's copy: one block in FamilyTableLayout, staged on the host and copied once
	const vgsdf::FamilyTableLayout at(n);
	std::vector<uint8_t> h(at.bytes + 16, 0);
	std::memcpy(h.data() + at.scale, f->scale.data(), 8 * (size_t)n);
	std::memcpy(h.data() + at.shift_x, f->shift_x.data(), 8 * (size_t)n);
	for (uint32_t i = 0; i <= n; i++) {
		((uint32_t *)(h.data() + at.cmd_pre))[i] = (uint32_t)f->cmd_pre[i];
		((uint32_t *)(h.data() + at.leaf_pre))[i] = (uint32_t)f->leaf_pre[i];
	}
	std::memcpy(h.data() + at.advance, f->advance.data(), 4 * (size_t)n);
	std::memcpy(h.data() + at.code_point, f->code_point.data(), 2 * (size_t)n);
	std::memcpy(h.data() + at.font_of, f->font_of.data(), 2 * (size_t)n);
	std::memcpy(h.data() + at.glyph_id, f->glyph_id.data(), 2 * (size_t)n);
	std::memcpy(h.data() + at.pbf_fix, f->pbf_fix.data(), n);
	(void)hipSetDevice(ctx->device);
	if (hipError_t e = f->table.ensure(h.size()); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_family_create", "hipMalloc", e);
	hipError_t e = hipMemcpyAsync(f->table.p, h.data(), h.size(), hipMemcpyHostToDevice, ctx->stream);
	if (e == hipSuccess)
		e = hipStreamSynchronize(ctx->stream); // the table is on the device when the call returns: every context may name the family
	if (e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_family_create", "upload", e);
	*out = f.release();
	return VGSDF_OK;
}

int vgsdf_family_create_tables(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, vgsdf_family **out)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || !in->fonts || !in->tables) {
		ctx->err = "vgsdf_family_create_tables: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	ctx->family_tables_ms[0] = ctx->family_tables_ms[1] = 0.0f;
	const uint32_t n_fonts = in->n_fonts;
	if (n_fonts == 0 || n_fonts > 0x10000u) {
		ctx->err = "vgsdf_family_create_tables: n_fonts must be 1 .. 65536";
		return VGSDF_E_ARG;
	}
	// what can be said without a lookup; the staging block's layout on the way:
	// FamilyFaceRef[n_fonts] | FamilySubtable[all] | per face cmap, hmtx (4-aligned) | counts | flags
	size_t n_subtables = 0, table_bytes = 0;
	for (uint32_t k = 0; k < n_fonts; k++) {
		const vgsdf_font *ft = in->fonts[k];
		const vgsdf_face_tables &t = in->tables[k];
		if (!ft || ft->device != ctx->device || ft->commands != in->fonts[0]->commands) {
			ctx->err = "vgsdf_family_create_tables: a NULL font, a font of another device than the context's, or fonts of both kinds";
			return VGSDF_E_ARG;
		}
		if ((t.cmap_len && !t.cmap) || (t.hmtx_len && !t.hmtx) || (t.n_subtables && (!t.subtable_off || !t.subtable_format))) {
			ctx->err = "vgsdf_family_create_tables: a NULL table or subtable array of a length that is not 0";
			return VGSDF_E_ARG;
		}
		if (t.units_per_em < 16 || t.units_per_em > 16384) {
			ctx->err = "vgsdf_family_create_tables: units_per_em not 16 .. 16384";
			return VGSDF_E_ARG;
		}
		for (uint32_t s = 0; s < t.n_subtables; s++) {
			const uint16_t fm = t.subtable_format[s];
			if (t.subtable_off[s] >= t.cmap_len || !(fm == 0 || fm == 4 || fm == 6 || fm == 10 || fm == 12 || fm == 13)) {
				ctx->err = "vgsdf_family_create_tables: a subtable offset at or past cmap_len, or a format that is not 0, 4, 6, 10, 12 or 13";
				return VGSDF_E_ARG;
			}
		}
		n_subtables += t.n_subtables;
		table_bytes += align_up(t.cmap_len, 4) + align_up(t.hmtx_len, 4);
	}
	std::unique_ptr<vgsdf_family> f(new (std::nothrow) vgsdf_family());
	if (!f) {
		ctx->err = "vgsdf_family_create_tables: out of host memory";
		return VGSDF_E_OOM;
	}
	f->device = ctx->device;
	f->commands = in->fonts[0]->commands;
	f->fonts.assign(in->fonts, in->fonts + n_fonts);
	for (const vgsdf_font *ft : f->fonts) {
		f->max_cap = std::max(f->max_cap, ft->max_cap);
		f->max_len = std::max(f->max_len, ft->max_len);
	}
	const size_t a_subs = sizeof(vgsdf::FamilyFaceRef) * (size_t)n_fonts, a_bytes = a_subs + sizeof(vgsdf::FamilySubtable) * n_subtables,
	             a_counts = align_up(a_bytes + table_bytes, 16), a_flags = a_counts + 4 * (size_t)vgsdf::kFamilyCounts * vgsdf::kFamilyGroups,
	             a_total = a_flags + 16;
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(a_total); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_family_create_tables", "hipMalloc", e);
	uint8_t *d = (uint8_t *)dev.p;
	std::vector<uint8_t> h(a_counts, 0);
	{
		vgsdf::FamilyFaceRef *faces = (vgsdf::FamilyFaceRef *)h.data();
		vgsdf::FamilySubtable *subs = (vgsdf::FamilySubtable *)(h.data() + a_subs);
		size_t at_sub = 0, at_byte = a_bytes;
		for (uint32_t k = 0; k < n_fonts; k++) {
			const vgsdf_font &ft = *in->fonts[k];
			const vgsdf_face_tables &t = in->tables[k];
			vgsdf::FamilyFaceRef &r = faces[k];
			r.subtables = (uint64_t)(uintptr_t)(d + a_subs + sizeof(vgsdf::FamilySubtable) * at_sub);
			for (uint32_t s = 0; s < t.n_subtables; s++)
				subs[at_sub++] = vgsdf::FamilySubtable{t.subtable_off[s], t.subtable_format[s]};
			r.cmap = (uint64_t)(uintptr_t)(d + at_byte);
			if (t.cmap_len)
				std::memcpy(h.data() + at_byte, t.cmap, t.cmap_len);
			at_byte += align_up(t.cmap_len, 4);
			r.hmtx = t.hmtx_len ? (uint64_t)(uintptr_t)(d + at_byte) : 0;
			if (t.hmtx_len)
				std::memcpy(h.data() + at_byte, t.hmtx, t.hmtx_len);
			at_byte += align_up(t.hmtx_len, 4);
			r.off = ft.commands ? ft.cref.cmd_off : ft.ref.leaf_off;
			r.leaves = ft.commands ? 0 : ft.ref.leaves;
			r.cmap_len = t.cmap_len, r.hmtx_len = t.hmtx_len;
			r.n_glyph_ids = ft.n_glyph_ids;
			r.units_per_em = t.units_per_em, r.num_glyphs = t.num_glyphs, r.num_hmetrics = t.num_hmetrics, r.n_subtables = t.n_subtables;
			r.commands = ft.commands ? 1u : 0u;
		}
	}
	struct Events {
		hipEvent_t e[3] = {nullptr, nullptr, nullptr};
		~Events()
		{
			for (hipEvent_t ev : e)
				if (ev)
					(void)hipEventDestroy(ev);
		}
	} ev;
	for (hipEvent_t &e : ev.e)
		if (hipError_t err = hipEventCreate(&e); err != hipSuccess)
			return font_hip_error(ctx, "vgsdf_family_create_tables", "hipEventCreate", err);
	const vgsdf::FamilyFaceRef *faces = (const vgsdf::FamilyFaceRef *)d;
	uint32_t *counts = (uint32_t *)(d + a_counts), *flags = (uint32_t *)(d + a_flags);
	hipError_t e = hipMemcpyAsync(d, h.data(), h.size(), hipMemcpyHostToDevice, st);
	if (e == hipSuccess)
		e = hipMemsetAsync(d + a_flags, 0, 16, st);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[0], st);
	if (e == hipSuccess)
		e = (hipError_t)vgsdf_family_tables_count(faces, n_fonts, counts, flags, st);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[1], st);
	uint32_t got[vgsdf::kFamilyCounts * vgsdf::kFamilyGroups + 1]; // the counts and, behind them, the flag word
	if (e == hipSuccess)
		e = hipMemcpyAsync(got, counts, sizeof got, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st);
	if (e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_family_create_tables", "count pass", e);
	(void)hipEventElapsedTime(&ctx->family_tables_ms[0], ev.e[0], ev.e[1]);
	if (got[vgsdf::kFamilyCounts * vgsdf::kFamilyGroups]) {
		ctx->err = "vgsdf_family_create_tables: a glyph id past its face";
		return VGSDF_E_ARG;
	}
	uint32_t n = 0;
	for (uint32_t w = 0; w < vgsdf::kFamilyGroups; w++)
		n += got[vgsdf::kFamilyCounts * w];
	// the table as vgsdf_family_create allocates it (the same size: the same vgsdf_family_device_bytes)
	const vgsdf::FamilyTableLayout at(n);
	if (hipError_t err = f->table.ensure(at.bytes + 16); err != hipSuccess)
		return font_hip_error(ctx, "vgsdf_family_create_tables", "hipMalloc", err);
	std::vector<uint8_t> back(at.bytes);
	e = hipEventRecord(ev.e[1], st);
	if (e == hipSuccess)
		e = (hipError_t)vgsdf_family_tables_emit(faces, n_fonts, counts, n, (uint8_t *)f->table.p, st);
	if (e == hipSuccess)
		e = hipEventRecord(ev.e[2], st);
	if (e == hipSuccess)
		e = hipMemcpyAsync(back.data(), f->table.p, at.bytes, hipMemcpyDeviceToHost, st);
	if (e == hipSuccess)
		e = hipStreamSynchronize(st); // the table is complete when the call returns: every context may name the family
	if (e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_family_create_tables", "emit pass", e);
	(void)hipEventElapsedTime(&ctx->family_tables_ms[1], ev.e[1], ev.e[2]);
	// the host's copy from the one read-back; the 64-bit running sums from the table's differences (exact: a glyph holds fewer
	// than 2^31 slots and fewer than 2^32 leaves)
	auto slice = [&](auto &v, size_t off, size_t count) {
		v.resize(count);
		if (count)
			std::memcpy(v.data(), back.data() + off, sizeof(v[0]) * count);
	};
	slice(f->scale, at.scale, n), slice(f->shift_x, at.shift_x, n), slice(f->advance, at.advance, n), slice(f->code_point, at.code_point, n);
	slice(f->font_of, at.font_of, n), slice(f->glyph_id, at.glyph_id, n), slice(f->pbf_fix, at.pbf_fix, n);
	f->cmd_pre.assign((size_t)n + 1, 0);
	f->leaf_pre.assign((size_t)n + 1, 0);
	const uint32_t *cp32 = (const uint32_t *)(back.data() + at.cmd_pre), *lp32 = (const uint32_t *)(back.data() + at.leaf_pre);
	for (uint32_t i = 0; i < n; i++) {
		f->cmd_pre[i + 1] = f->cmd_pre[i] + (uint32_t)(cp32[i + 1] - cp32[i]);
		f->leaf_pre[i + 1] = f->leaf_pre[i] + (uint32_t)(lp32[i + 1] - lp32[i]);
	}
	// (scales_plain stays true: every scale is 24 / units_per_em of a checked units_per_em)
	*out = f.release();
	return VGSDF_OK;
}

void vgsdf_family_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2])
{
	if (ms)
		ms[0] = ctx ? ctx->family_tables_ms[0] : 0.0f, ms[1] = ctx ? ctx->family_tables_ms[1] : 0.0f;
}

int vgsdf_family_read(vgsdf_ctx *ctx, const vgsdf_family *family, uint32_t *n_entries, uint16_t *code_point, uint16_t *font_of,
                      uint16_t *glyph_id, uint32_t *advance, double *scale, double *shift_x, uint32_t *cmd_pre, uint32_t *leaf_pre,
                      uint8_t *pbf_fix)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!family || family->device != ctx->device) {
		ctx->err = "vgsdf_family_read: no family, or a family of another device than the context's";
		return VGSDF_E_ARG;
	}
	const size_t n = family->code_point.size();
	if (n_entries)
		*n_entries = (uint32_t)n;
	(void)hipSetDevice(ctx->device);
	const vgsdf::FamilyTableLayout at(n);
	const uint8_t *t = (const uint8_t *)family->table.p;
	auto read = [&](void *dst, size_t off, size_t bytes) { return dst && bytes ? hipMemcpy(dst, t + off, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
	HIP_TRY(ctx, read(code_point, at.code_point, 2 * n));
	HIP_TRY(ctx, read(font_of, at.font_of, 2 * n));
	HIP_TRY(ctx, read(glyph_id, at.glyph_id, 2 * n));
	HIP_TRY(ctx, read(advance, at.advance, 4 * n));
	HIP_TRY(ctx, read(scale, at.scale, 8 * n));
	HIP_TRY(ctx, read(shift_x, at.shift_x, 8 * n));
	HIP_TRY(ctx, read(cmd_pre, at.cmd_pre, 4 * (n + 1)));
	HIP_TRY(ctx, read(leaf_pre, at.leaf_pre, 4 * (n + 1)));
	HIP_TRY(ctx, read(pbf_fix, at.pbf_fix, n));
	return VGSDF_OK;
}

int vgsdf_family_free(vgsdf_ctx *ctx, vgsdf_family *family)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!family)
		return VGSDF_OK;
	if (family->device != ctx->device) {
		ctx->err = "vgsdf_family_free: the family lives on another device than the context";
		return VGSDF_E_ARG;
	}
	(void)hipSetDevice(ctx->device);
	delete family;
	return VGSDF_OK;
}

uint64_t vgsdf_family_device_bytes(const vgsdf_family *family) { return family ? (uint64_t)family->table.cap : 0; }

uint32_t vgsdf_family_count(const vgsdf_family *family, uint32_t first, uint32_t last)
{
	if (!family || first > last)
		return 0;
	const auto &cp = family->code_point;
	const auto lo = std::lower_bound(cp.begin(), cp.end(), (uint16_t)std::min(first, 0xFFFFu));
	if (first > 0xFFFFu)
		return 0;
	const auto hi = std::upper_bound(cp.begin(), cp.end(), (uint16_t)std::min(last, 0xFFFFu));
	return (uint32_t)(hi - lo);
}

} // extern "C"
