// resident_fonts.cpp — the stores behind vgsdf_font: a face's outlines uploaded once, as `glyf` leaves (vgsdf_font_create;
// vgsdf_font_create_tables: walked on the device from a face's loca and glyf) or as expanded commands (vgsdf_font_create_commands;
// vgsdf_font_create_charstrings: decoded on the device from a CFF face's charstrings).  Submissions that name their glyphs read them
// (outline_front_end.cpp, vgsdf_outlines_submit_resident).  Each kind has one layout (upload_layout.h: GlyfStoreLayout,
// CommandStoreLayout) and one function that finishes a store in it; the families over the fonts: resident_families.cpp.
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "charstring_kernels.h"
#include "charstring_limits.h"
#include "glyf_table_kernels.h"
#include "glyf_table_limits.h"
#include "gvar_kernels.h"
#include "gvar_limits.h"
#include "outline_kernels.h"
#include "resident_build.h"

namespace {
static_assert(sizeof(vgsdf::OutlineCmd) == 28, "the records of CommandStoreLayout");

// a glyf font's three arrays, once its store is allocated
void name_glyf_store(vgsdf_font &f, const vgsdf::GlyfStoreLayout &at)
{
	const uintptr_t d = (uintptr_t)f.store.p;
	f.ref.leaves = d + at.leaves, f.ref.bytes = d + at.bytes, f.ref.leaf_off = d + at.leaf_off;
}

// a command font's three arrays, once its store is allocated
void name_command_store(vgsdf_font &f, const vgsdf::CommandStoreLayout &at, uint32_t n_cmds)
{
	uint8_t *d = (uint8_t *)f.store.p;
	f.n_cmds = n_cmds;
	f.cref.cmds = (uintptr_t)d, f.cref.cmd_off = (uintptr_t)(d + at.cmd_off), f.cref.open = (uintptr_t)(d + at.open);
}

// what the packed form's context pass reads beside a command store, for the duration of the call that builds it:
// scale f64[n] (1: the bytes then say "ring open" and nothing else) | dat_off u32[n + 1] | coords | kinds | pad to 16 | its error word
struct ContextStagingLayout {
	size_t scale = 0, dat_off, coords, kinds, flag, total;
	constexpr ContextStagingLayout(size_t n, size_t n_cmds, size_t n_floats)
	    : dat_off(8 * n), coords(dat_off + 4 * (n + 1)), kinds(coords + 4 * n_floats), flag((kinds + n_cmds + 15) / 16 * 16), total(flag + 16)
	{
	}
};
static_assert(ContextStagingLayout(3, 5, 14).kinds == 24 + 16 + 56 && ContextStagingLayout(3, 5, 14).flag == 112 &&
                  ContextStagingLayout(3, 16, 14).flag == 112 && ContextStagingLayout(1, 0, 0).flag == 16 && ContextStagingLayout(1, 0, 0).total == 32,
              "scale | dat_off | coords | kinds | pad to 16 | flag");

// Both command constructors, once store (`at`) and staging (t, `tat`) are allocated: uploads cmd_off into the store and the unit
// scales and dat_off into the staging, lets `fill` put kinds and coordinates there (a copy, or the emit pass), runs the context
// pass over them and ends the call's work on the device.  Returns the pass's error word (0 also when q has failed); more_flags (may
// be NULL): a word of the emit pass's to read back with it, from d_more_flags
template <class Fill>
uint32_t finish_command_store(Calls &q, vgsdf_font &f, const vgsdf::CommandStoreLayout &at, uint8_t *t, const ContextStagingLayout &tat,
                              uint32_t n_cmds, const uint32_t *cmd_off, const uint32_t *dat_off, Fill fill, uint32_t *more_flags = nullptr,
                              const void *d_more_flags = nullptr)
{
	const uint32_t n = f.n_glyph_ids;
	uint8_t *d = (uint8_t *)f.store.p;
	const std::vector<double> ones(n, 1.0);
	q.copy(d + at.cmd_off, cmd_off, 4 * ((size_t)n + 1));
	q.copy(t + tat.scale, ones.data(), 8 * (size_t)n);
	q.copy(t + tat.dat_off, dat_off, 4 * ((size_t)n + 1));
	q.zero(t + tat.flag, 16);
	fill();
	if (n_cmds)
		q.launch([&] {
			return vgsdf_outline_context_packed(t + tat.kinds, (const float *)(t + tat.coords), (const uint32_t *)(t + tat.dat_off),
			                                    (const uint32_t *)(d + at.cmd_off), (const double *)(t + tat.scale), n, (vgsdf::OutlineCmd *)d,
			                                    d + at.open, (uint32_t *)(t + tat.flag), q.st);
		});
	uint32_t flag = 0;
	q.read_back(&flag, t + tat.flag, 4);
	if (more_flags)
		q.read_back(more_flags, d_more_flags, 4);
	q.sync();
	name_command_store(f, at, n_cmds);
	return flag;
}
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
	const vgsdf::GlyfStoreLayout at(n, in->n_leaves, in->n_bytes);
	if (hipError_t e = f->store.ensure(at.total + 16); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create", "hipMalloc", e);
	uint8_t *d = (uint8_t *)f->store.p;
	Calls q(ctx->stream);
	q.copy(d + at.leaves, in->leaves, at.bytes - at.leaves);
	q.copy(d + at.bytes, in->bytes, in->n_bytes);
	q.copy(d + at.leaf_off, in->leaf_off, 4 * ((size_t)n + 1));
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, "vgsdf_font_create", "upload", q.e);
	name_glyf_store(*f, at);
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
	const vgsdf::CommandStoreLayout at(n, n_cmds);
	if (n > 0x10000u || at.total > 0xFFFFFFFCull || 4ull * in->n_floats > 0xFFFFFFFCull) {
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
	const ContextStagingLayout tat(n, n_cmds, in->n_floats);
	ScratchBuf tmp;
	if (hipError_t e = f->store.ensure(at.total + 16); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_commands", "hipMalloc", e);
	if (hipError_t e = tmp.ensure(tat.total); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_commands", "hipMalloc", e);
	uint8_t *t = (uint8_t *)tmp.p;
	Calls q(ctx->stream);
	const uint32_t flag = finish_command_store(q, *f, at, t, tat, n_cmds, in->cmd_off, in->dat_off, [&] {
		q.copy(t + tat.coords, in->coords, 4 * (size_t)in->n_floats);
		q.copy(t + tat.kinds, in->kinds, n_cmds);
	});
	if (q.failed())
		return font_hip_error(ctx, "vgsdf_font_create_commands", "upload", q.e);
	if (flag) { // (what the walk above has ruled out, said by the pass itself)
		ctx->err = "vgsdf_font_create_commands: the device's context pass refused the commands";
		return VGSDF_E_ARG;
	}
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
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	if (hipError_t e = face_buf.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)face_buf.p;
	Calls q(st);
	q.copy(a, in->bytes, n_bytes);
	q.copy(a + a_cs, in->cs_off, 4 * ((size_t)n + 1));
	q.copy(a + a_gs, in->gsubr_off, 4 * ((size_t)in->n_gsubrs + 1));
	q.copy(a + a_lf, in->lsubr_first, 4 * ((size_t)in->n_fds + 1));
	q.copy(a + a_lo, in->lsubr_off, 4 * ((size_t)n_lsubrs + 1));
	if (in->fd_of)
		q.copy(a + a_fd, in->fd_of, n);
	if (n_sets)
		q.copy(a + a_so, blend->set_off, 4 * ((size_t)n_sets + 1));
	if (n_factors)
		q.copy(a + a_fac, blend->factors, 4 * (size_t)n_factors);
	if (n_sets)
		q.copy(a + a_ok, blend->set_ok, n_sets);
	q.zero(a + a_flags, 16);
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
	q.record(ev.at[0]);
	q.launch([&] { return run_pass(false, nullptr, nullptr, nullptr, nullptr); });
	q.record(ev.at[1]);
	std::vector<uint32_t> counts(2 * (size_t)n);
	uint32_t flags = 0;
	q.read_back(counts.data(), a + a_counts, 8 * (size_t)n);
	q.read_back(&flags, a + a_flags, 4);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "count pass", q.e);
	ev.elapsed(ctx->charstring_ms, 0);
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
		if (vgsdf::CommandStoreLayout(n, cmds).total > 0xFFFFFFFCull || 4ull * floats > 0xFFFFFFFCull) {
			ctx->err = entry + "a store (29 bytes per command, 4 per glyph id) or coordinates past what 32-bit "
			           "offsets address";
			return VGSDF_E_GLYF;
		}
	}
	const uint32_t n_cmds = (uint32_t)cmds, n_floats = (uint32_t)floats;
	cmd_off[n] = n_cmds, dat_off[n] = n_floats;
	const vgsdf::CommandStoreLayout at(n, n_cmds);
	if (store_bytes)
		*store_bytes = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->commands = true;
	const ContextStagingLayout tat(n, n_cmds, n_floats);
	if (hipError_t err = f->store.ensure(at.total + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	if (hipError_t err = tmp.ensure(tat.total); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	uint8_t *d = (uint8_t *)f->store.p, *t = (uint8_t *)tmp.p;
	// (the emit pass reads cmd_off from the store, where it stays, and dat_off from the staging, as the context pass behind it does)
	const uint32_t flag = finish_command_store(q, *f, at, t, tat, n_cmds, cmd_off.data(), dat_off.data(), [&] {
		q.record(ev.at[1]);
		if (n_cmds)
			q.launch([&] {
				return run_pass(true, (const uint32_t *)(d + at.cmd_off), (const uint32_t *)(t + tat.dat_off), t + tat.kinds, (float *)(t + tat.coords));
			});
		q.record(ev.at[2]);
	}, &flags, a + a_flags);
	if (q.failed())
		return font_hip_error(ctx, name, "emit pass", q.e);
	if (n_cmds)
		ev.elapsed(ctx->charstring_ms, 1);
	if (flag || flags) { // (the two passes walk one text over the same bytes: said by the passes themselves)
		ctx->err = entry + "the emit pass did not match the count pass, or the context pass refused the commands";
		return VGSDF_E_HIP;
	}
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

void vgsdf_font_charstrings_kernel_ms(const vgsdf_ctx *ctx, float ms[2]) { pass_ms_out(ctx ? ctx->charstring_ms : nullptr, ms); }

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
	// (the arrays' sizes as CommandStoreLayout states them; spelled out because HIP_TRY's error text is the call's own)
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
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_tables", "hipEventCreate", err);
	// the description on the device, for the duration of this call: loca | glyf | counts (4 per glyph id) | flags | byte_at
	const size_t a_glyf = align_up(in->n_loca_bytes, 16), a_counts = align_up(a_glyf + in->n_glyf_bytes, 16),
	             a_flags = a_counts + 4 * (size_t)vgsdf::kGlyfTableCounts * n, a_at = a_flags + 4 * (size_t)vgsdf::GLYF_FLAG_WORDS,
	             a_total = a_at + 4 * ((size_t)n + 1);
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_tables", "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	Calls q(st);
	q.copy(a, in->loca, in->n_loca_bytes);
	q.copy(a + a_glyf, in->glyf, in->n_glyf_bytes);
	q.zero(a + a_flags, 4 * (size_t)vgsdf::GLYF_FLAG_WORDS);
	vgsdf::GlyfTablesRef face{};
	face.loca = a, face.glyf = a + a_glyf;
	face.glyf_len = in->n_glyf_bytes, face.loca_entries = in->loca_entries, face.loca_long = in->loca_long, face.n_glyph_ids = n;
	uint32_t *d_counts = (uint32_t *)(a + a_counts), *d_flags = (uint32_t *)(a + a_flags), *d_at = (uint32_t *)(a + a_at);
	q.record(ev.at[0]);
	if (n)
		q.launch([&] { return vgsdf_glyf_tables_count(&face, d_counts, d_flags, st); });
	q.record(ev.at[1]);
	// the counts and, behind them, the flag words: one read-back
	std::vector<uint32_t> got((size_t)vgsdf::kGlyfTableCounts * n + vgsdf::GLYF_FLAG_WORDS);
	q.read_back(got.data(), d_counts, 4 * got.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, "vgsdf_font_create_tables", "count pass", q.e);
	ev.elapsed(ctx->glyf_tables_ms, 0);
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
	const vgsdf::GlyfStoreLayout at(n, n_leaves, n_bytes);
	if (needed)
		*needed = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->n_leaves = (uint32_t)n_leaves;
	f->n_bytes = (uint32_t)n_bytes;
	if (hipError_t err = f->store.ensure(at.total + 16); err != hipSuccess)
		return font_hip_error(ctx, "vgsdf_font_create_tables", "hipMalloc", err);
	uint8_t *d = (uint8_t *)f->store.p;
	q.copy(d + at.leaf_off, f->leaf_off.data(), 4 * ((size_t)n + 1));
	q.copy(d_at, byte_at.data(), 4 * ((size_t)n + 1));
	q.record(ev.at[1]);
	if (n)
		q.launch([&] { return vgsdf_glyf_tables_emit(&face, (const uint32_t *)(d + at.leaf_off), d_at, d + at.leaves, d + at.bytes, d_flags, st); });
	q.record(ev.at[2]);
	uint32_t flags[vgsdf::GLYF_FLAG_WORDS] = {};
	q.read_back(flags, d_flags, sizeof flags);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, "vgsdf_font_create_tables", "emit pass", q.e);
	ev.elapsed(ctx->glyf_tables_ms, 1);
	if (flags[vgsdf::GLYF_FLAG_EMIT]) { // (the two passes walk one text over the same bytes: said by the pass itself)
		ctx->err = "vgsdf_font_create_tables: the emit pass did not match the count pass";
		return VGSDF_E_HIP;
	}
	name_glyf_store(*f, at);
	*out = f.release();
	return VGSDF_OK;
}

void vgsdf_font_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2]) { pass_ms_out(ctx ? ctx->glyf_tables_ms : nullptr, ms); }

} // extern "C"

namespace {
uint32_t be16_at(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
uint32_t be32_at(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// what both gvar constructors validate of the tables and the gvar header before anything runs; fills the header's fields of `face`
bool gvar_face_described(vgsdf_ctx *ctx, const char *entry, const vgsdf_font_tables_desc &in, const uint8_t *g, uint64_t gvar_len, uint32_t n_axes,
                         vgsdf::GvarRef &face)
{
	const uint32_t n = in.num_glyphs;
	if (n > 0xFFFFu || in.loca_long > 1u || (uint64_t)in.loca_entries * (in.loca_long ? 4u : 2u) > in.n_loca_bytes || in.loca_entries > n + 1) {
		ctx->err = std::string(entry) + ": more than 65535 glyphs, loca_long not 0 or 1, or more loca entries than the loca bytes hold or than num_glyphs + 1";
		return false;
	}
	// GvarTable::parse: majorVersion, minorVersion, axisCount, sharedTupleCount, sharedTuplesOffset, glyphCount, flags,
	// glyphVariationDataArrayOffset; the shared tuples and the offset array inside the table
	bool readable = n_axes >= 1 && n_axes <= vg::kGvarMaxAxes && gvar_len >= 20 && be32_at(g) == 0x00010000u && be16_at(g + 4) == n_axes;
	if (readable) {
		face.shared_count = be16_at(g + 6), face.shared_at = be32_at(g + 8), face.glyph_count = be16_at(g + 12);
		face.long_offsets = be16_at(g + 14) & 1u, face.data_at = be32_at(g + 16);
		const uint64_t tuples = (uint64_t)face.shared_count * n_axes * 2, offsets = ((uint64_t)face.glyph_count + 1) * (face.long_offsets ? 4u : 2u);
		readable = face.shared_at <= gvar_len && tuples <= gvar_len - face.shared_at && offsets <= gvar_len - 20;
	}
	if (!readable) {
		ctx->err = std::string(entry) + ": axes not 1 .. 64, a gvar that is not version 1.0 or has another axisCount, or a header, shared tuples "
		                                "or offset array outside gvar_len";
		return false;
	}
	return true;
}

struct EventGuard { // an event beside PassEvents' three, destroyed with the call
	hipEvent_t &e;
	~EventGuard()
	{
		if (e)
			(void)hipEventDestroy(e);
	}
};

// vgsdf_font_create_gvar_within: count pass, read-back and layout, deltas pass in slices over the context's scratch, emit pass,
// context pass (gvar_kernels.h)
int create_gvar(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *desc, uint64_t max_store_bytes, vgsdf_font **out, uint64_t *store_bytes)
{
	const char *name = "vgsdf_font_create_gvar";
	if (!desc || !out || (desc->tables.n_loca_bytes && !desc->tables.loca) || (desc->tables.n_glyf_bytes && !desc->tables.glyf) || !desc->gvar ||
	    !desc->coords) {
		ctx->err = "vgsdf_font_create_gvar: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (store_bytes)
		*store_bytes = 0;
	ctx->gvar_ms[0] = ctx->gvar_ms[1] = ctx->gvar_ms[2] = 0.0f;
	const vgsdf_font_tables_desc &in = desc->tables;
	const uint32_t n = in.num_glyphs;
	const uint64_t gvar_len = desc->gvar_len;
	vgsdf::GvarRef face{};
	if (!gvar_face_described(ctx, name, in, desc->gvar, desc->gvar_len, desc->n_axes, face))
		return VGSDF_E_ARG;
	std::unique_ptr<vgsdf_font> f(new (std::nothrow) vgsdf_font());
	if (!f) {
		ctx->err = "vgsdf_font_create_gvar: out of host memory";
		return VGSDF_E_OOM;
	}
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	PassEvents ev;
	hipEvent_t ev_deltas = nullptr; // (the deltas pass ends here; PassEvents has the other three)
	EventGuard guard{ev_deltas};
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	if (hipError_t err = hipEventCreate(&ev_deltas); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	// the description on the device, for the duration of this call: loca | glyf | gvar | coords | counts (4 per glyph id) | flags | pt_at
	const size_t a_glyf = align_up(in.n_loca_bytes, 16), a_gvar = align_up(a_glyf + in.n_glyf_bytes, 16), a_coords = align_up(a_gvar + (size_t)gvar_len, 16),
	             a_counts = align_up(a_coords + 2 * (size_t)desc->n_axes, 16), a_flags = a_counts + 4 * (size_t)vgsdf::kGvarCounts * n,
	             a_at = a_flags + 4 * (size_t)vgsdf::GVAR_FLAG_WORDS, a_total = a_at + 4 * ((size_t)n + 1);
	ScratchBuf dev, sums, tmp;
	if (hipError_t e = dev.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	Calls q(st);
	q.copy(a, in.loca, in.n_loca_bytes);
	q.copy(a + a_glyf, in.glyf, in.n_glyf_bytes);
	q.copy(a + a_gvar, desc->gvar, (size_t)gvar_len);
	q.copy(a + a_coords, desc->coords, 2 * (size_t)desc->n_axes);
	q.zero(a + a_flags, 4 * (size_t)vgsdf::GVAR_FLAG_WORDS);
	face.loca = a, face.glyf = a + a_glyf, face.gvar = a + a_gvar, face.coords = (const int16_t *)(a + a_coords);
	face.glyf_len = in.n_glyf_bytes, face.loca_entries = in.loca_entries, face.loca_long = in.loca_long, face.n_glyph_ids = n;
	face.gvar_len = (uint32_t)gvar_len, face.n_axes = desc->n_axes;
	uint32_t *d_counts = (uint32_t *)(a + a_counts), *d_flags = (uint32_t *)(a + a_flags), *d_at = (uint32_t *)(a + a_at);
	q.record(ev.at[0]);
	if (n)
		q.launch([&] { return vgsdf_gvar_count(&face, d_counts, d_flags, st); });
	q.record(ev.at[1]);
	// the counts and, behind them, the flag words: one read-back
	std::vector<uint32_t> got((size_t)vgsdf::kGvarCounts * n + vgsdf::GVAR_FLAG_WORDS);
	q.read_back(got.data(), d_counts, 4 * got.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "count pass", q.e);
	ev.elapsed(ctx->gvar_ms, 0);
	const uint32_t *fl = got.data() + (size_t)vgsdf::kGvarCounts * n;
	if (fl[vgsdf::GVAR_FLAG_RECORDS] || fl[vgsdf::GVAR_FLAG_CMDS]) {
		ctx->err = fl[vgsdf::GVAR_FLAG_RECORDS]
		               ? "vgsdf_font_create_gvar: a glyph past VGSDF_GLYF_MAX_COMPONENTS, or a composite of more than 65535 component records"
		               : "vgsdf_font_create_gvar: a glyph of more than 2^26 commands";
		return VGSDF_E_GLYF;
	}
	// the running sums: the points of the deltas pass, the store's layout (what vgsdf_font_create_commands is given by its caller)
	std::vector<uint32_t> pt_at((size_t)n + 1), cmd_off((size_t)n + 1), dat_off((size_t)n + 1);
	uint64_t points = 0, cmds = 0, floats = 0;
	f->slots.assign(n, 0);
	for (uint32_t gid = 0; gid < n; gid++) {
		const uint32_t *c = got.data() + (size_t)vgsdf::kGvarCounts * gid;
		pt_at[gid] = (uint32_t)points, cmd_off[gid] = (uint32_t)cmds, dat_off[gid] = (uint32_t)floats;
		f->slots[gid] = c[1];
		points += c[0], cmds += c[1], floats += c[2];
		if (vgsdf::CommandStoreLayout(n, cmds).total > 0xFFFFFFFCull || 4ull * floats > 0xFFFFFFFCull) {
			ctx->err = "vgsdf_font_create_gvar: a store (29 bytes per command, 4 per glyph id) or coordinates past what 32-bit offsets address";
			return VGSDF_E_GLYF;
		}
	}
	// (65535 glyph ids of at most 65539 points: below 2^32)
	const uint32_t n_cmds = (uint32_t)cmds, n_floats = (uint32_t)floats;
	pt_at[n] = (uint32_t)points, cmd_off[n] = n_cmds, dat_off[n] = n_floats;
	const vgsdf::CommandStoreLayout at(n, n_cmds);
	if (store_bytes)
		*store_bytes = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	// the deltas pass, in slices of glyph ids over the context's scratch
	if (hipError_t err = sums.ensure(8 * (size_t)points + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	float *d_acc = (float *)sums.p;
	q.copy(d_at, pt_at.data(), 4 * ((size_t)n + 1));
	q.record(ev.at[1]);
	for (uint32_t g0 = 0; g0 < n && !q.failed();) {
		uint32_t g1 = g0 + 1;
		while (g1 < n && pt_at[g1 + 1] - pt_at[g0] <= vg::kGvarSlicePoints)
			g1++;
		const size_t slice = pt_at[g1] - pt_at[g0];
		if (slice) {
			// sx | sy | x | y | mark, each 16-aligned
			const size_t s_sy = align_up(4 * slice, 16), s_x = s_sy + s_sy, s_y = s_x + align_up(2 * slice, 16), s_mark = s_y + align_up(2 * slice, 16),
			             s_total = s_mark + slice;
			if (hipError_t err = ctx->gvar_scratch.ensure(s_total + 16); err != hipSuccess) // (nothing in flight reads it: see below)
				return font_hip_error(ctx, name, "hipMalloc", err);
			uint8_t *s = (uint8_t *)ctx->gvar_scratch.p;
			const vgsdf::GvarScratch scratch{(float *)s, (float *)(s + s_sy), (int16_t *)(s + s_x), (int16_t *)(s + s_y), s + s_mark};
			q.launch([&] { return vgsdf_gvar_deltas(&face, g0, g1, d_counts, d_at, d_acc, &scratch, d_flags, st); });
			// (the launches follow one another on one stream over one scratch; it grows only between them, so the stream is drained
			// before the next slice may replace it)
			if (g1 < n)
				q.sync();
		}
		g0 = g1;
	}
	q.record(ev_deltas);
	uint32_t flags[vgsdf::GVAR_FLAG_WORDS] = {};
	q.read_back(flags, d_flags, sizeof flags);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "deltas pass", q.e);
	(void)hipEventElapsedTime(&ctx->gvar_ms[1], ev.at[1], ev_deltas);
	if (flags[vgsdf::GVAR_FLAG_MALFORMED] || flags[vgsdf::GVAR_FLAG_DELTAS]) {
		ctx->err = flags[vgsdf::GVAR_FLAG_MALFORMED] ? "vgsdf_font_create_gvar: a glyph with malformed variation data"
		                                             : "vgsdf_font_create_gvar: a glyph past VGSDF_GVAR_MAX_DELTAS";
		return VGSDF_E_GLYF;
	}
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->commands = true;
	const ContextStagingLayout tat(n, n_cmds, n_floats);
	if (hipError_t err = f->store.ensure(at.total + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	if (hipError_t err = tmp.ensure(tat.total); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	uint8_t *d = (uint8_t *)f->store.p, *t = (uint8_t *)tmp.p;
	uint32_t emit_flag = 0;
	// (the emit pass reads cmd_off from the store, where it stays, and dat_off from the staging, as the context pass behind it does)
	const uint32_t flag = finish_command_store(q, *f, at, t, tat, n_cmds, cmd_off.data(), dat_off.data(), [&] {
		q.record(ev.at[1]);
		if (n)
			q.launch([&] {
				return vgsdf_gvar_emit(&face, d_counts, d_at, d_acc, (const uint32_t *)(d + at.cmd_off), (const uint32_t *)(t + tat.dat_off), t + tat.kinds,
				                       (float *)(t + tat.coords), d_flags, st);
			});
		q.record(ev.at[2]);
	}, &emit_flag, d_flags + vgsdf::GVAR_FLAG_EMIT);
	if (q.failed())
		return font_hip_error(ctx, name, "emit pass", q.e);
	(void)hipEventElapsedTime(&ctx->gvar_ms[2], ev.at[1], ev.at[2]);
	if (flag || emit_flag) { // (the two passes walk one text over the same bytes: said by the passes themselves)
		ctx->err = "vgsdf_font_create_gvar: the emit pass did not match the count pass, or the context pass refused the commands";
		return VGSDF_E_HIP;
	}
	*out = f.release();
	return VGSDF_OK;
}
} // namespace

extern "C" {

int vgsdf_font_create_gvar(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *in, vgsdf_font **out)
{
	return vgsdf_font_create_gvar_within(ctx, in, ~0ull, out, nullptr);
}

int vgsdf_font_create_gvar_within(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                  uint64_t *store_bytes)
{
	if (!ctx)
		return VGSDF_E_ARG;
	try {
		return create_gvar(ctx, in, max_store_bytes, out, store_bytes);
	} catch (const std::bad_alloc &) {
		ctx->err = "vgsdf_font_create_gvar: out of host memory";
		return VGSDF_E_OOM;
	}
}

void vgsdf_font_gvar_kernel_ms(const vgsdf_ctx *ctx, float ms[3])
{
	if (ms)
		for (int i = 0; i < 3; i++)
			ms[i] = ctx ? ctx->gvar_ms[i] : 0.0f;
}

} // extern "C"

namespace {
// vgsdf_fonts_create_gvar_within: create_gvar for one face at all its positions.  The tables go up once; the count pass, its
// read-back and the layout are the single call's and serve every position; the deltas pass and the emit pass run over (glyph id,
// position) pairs (gvar_batch_kernels.hip), the context pass once per store; two more read-backs (the positions' flag words
// behind the deltas pass and behind the emit pass) and three synchronisations for the whole call
int create_gvar_batch(vgsdf_ctx *ctx, const vgsdf_fonts_gvar_desc *desc, uint64_t max_store_bytes, vgsdf_font **out, int *status, uint64_t *needed)
{
	const char *name = "vgsdf_fonts_create_gvar";
	if (!desc) {
		ctx->err = "vgsdf_fonts_create_gvar: NULL argument";
		return VGSDF_E_ARG;
	}
	const uint32_t n_pos = desc->n_positions;
	if (n_pos == 0)
		return VGSDF_OK;
	if (!out || !status || (desc->tables.n_loca_bytes && !desc->tables.loca) || (desc->tables.n_glyf_bytes && !desc->tables.glyf) || !desc->gvar ||
	    !desc->coords) {
		ctx->err = "vgsdf_fonts_create_gvar: NULL argument";
		return VGSDF_E_ARG;
	}
	if (n_pos > VGSDF_GVAR_MAX_POSITIONS) {
		ctx->err = "vgsdf_fonts_create_gvar: more than 64 positions in one call";
		return VGSDF_E_ARG;
	}
	for (uint32_t p = 0; p < n_pos; p++) {
		out[p] = nullptr, status[p] = VGSDF_OK;
		if (needed)
			needed[p] = 0;
	}
	ctx->gvar_batch_ms[0] = ctx->gvar_batch_ms[1] = ctx->gvar_batch_ms[2] = 0.0f;
	const vgsdf_font_tables_desc &in = desc->tables;
	const uint32_t n = in.num_glyphs, n_axes = desc->n_axes;
	const uint64_t gvar_len = desc->gvar_len;
	vgsdf::GvarRef face{};
	if (!gvar_face_described(ctx, name, in, desc->gvar, gvar_len, n_axes, face))
		return VGSDF_E_ARG;
	auto refuse_all = [&](const char *why) { // a refusal that no position can change
		ctx->err = std::string(name) + ": " + why;
		for (uint32_t p = 0; p < n_pos; p++)
			status[p] = VGSDF_E_GLYF;
		return VGSDF_OK;
	};
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	PassEvents ev;
	hipEvent_t ev_deltas = nullptr;
	EventGuard guard{ev_deltas};
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	if (hipError_t err = hipEventCreate(&ev_deltas); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	// the description on the device, for the duration of this call:
	// loca | glyf | gvar | coords (n_axes per position) | counts (4 per glyph id) | flags (8 per position) | pt_at | position records
	const size_t a_glyf = align_up(in.n_loca_bytes, 16), a_gvar = align_up(a_glyf + in.n_glyf_bytes, 16), a_coords = align_up(a_gvar + (size_t)gvar_len, 16),
	             a_counts = align_up(a_coords + 2 * (size_t)n_axes * n_pos, 16), a_flags = a_counts + 4 * (size_t)vgsdf::kGvarCounts * n,
	             a_at = a_flags + 4 * (size_t)vgsdf::GVAR_FLAG_WORDS * n_pos, a_rec = align_up(a_at + 4 * ((size_t)n + 1), 16),
	             a_total = a_rec + sizeof(vgsdf::GvarPositionRef) * (size_t)n_pos;
	ScratchBuf dev, sums, tmp;
	if (hipError_t e = dev.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	Calls q(st);
	q.copy(a, in.loca, in.n_loca_bytes);
	q.copy(a + a_glyf, in.glyf, in.n_glyf_bytes);
	q.copy(a + a_gvar, desc->gvar, (size_t)gvar_len);
	q.copy(a + a_coords, desc->coords, 2 * (size_t)n_axes * n_pos);
	q.zero(a + a_flags, 4 * (size_t)vgsdf::GVAR_FLAG_WORDS * n_pos);
	const int16_t *d_coords = (const int16_t *)(a + a_coords);
	face.loca = a, face.glyf = a + a_glyf, face.gvar = a + a_gvar, face.coords = d_coords; // (the batched kernels take each lane's own)
	face.glyf_len = in.n_glyf_bytes, face.loca_entries = in.loca_entries, face.loca_long = in.loca_long, face.n_glyph_ids = n;
	face.gvar_len = (uint32_t)gvar_len, face.n_axes = n_axes;
	uint32_t *d_counts = (uint32_t *)(a + a_counts), *d_flags = (uint32_t *)(a + a_flags), *d_at = (uint32_t *)(a + a_at);
	vgsdf::GvarPositionRef *d_rec = (vgsdf::GvarPositionRef *)(a + a_rec);
	// the count pass looks at no coordinate: one launch for all positions; its two flag words land among those of position 0
	q.record(ev.at[0]);
	if (n)
		q.launch([&] { return vgsdf_gvar_count(&face, d_counts, d_flags, st); });
	q.record(ev.at[1]);
	std::vector<uint32_t> got((size_t)vgsdf::kGvarCounts * n + vgsdf::GVAR_FLAG_WORDS);
	q.read_back(got.data(), d_counts, 4 * got.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "count pass", q.e);
	ev.elapsed(ctx->gvar_batch_ms, 0);
	const uint32_t *fl = got.data() + (size_t)vgsdf::kGvarCounts * n;
	if (fl[vgsdf::GVAR_FLAG_RECORDS])
		return refuse_all("a glyph past VGSDF_GLYF_MAX_COMPONENTS, or a composite of more than 65535 component records");
	if (fl[vgsdf::GVAR_FLAG_CMDS])
		return refuse_all("a glyph of more than 2^26 commands");
	// the running sums, the same for every position: the points of the deltas pass, the stores' layout
	std::vector<uint32_t> pt_at((size_t)n + 1), cmd_off((size_t)n + 1), dat_off((size_t)n + 1), slots(n, 0);
	uint64_t points = 0, cmds = 0, floats = 0;
	for (uint32_t gid = 0; gid < n; gid++) {
		const uint32_t *c = got.data() + (size_t)vgsdf::kGvarCounts * gid;
		pt_at[gid] = (uint32_t)points, cmd_off[gid] = (uint32_t)cmds, dat_off[gid] = (uint32_t)floats;
		slots[gid] = c[1];
		points += c[0], cmds += c[1], floats += c[2];
		if (vgsdf::CommandStoreLayout(n, cmds).total > 0xFFFFFFFCull || 4ull * floats > 0xFFFFFFFCull)
			return refuse_all("a store (29 bytes per command, 4 per glyph id) or coordinates past what 32-bit offsets address");
	}
	const uint32_t n_cmds = (uint32_t)cmds, n_floats = (uint32_t)floats;
	pt_at[n] = (uint32_t)points, cmd_off[n] = n_cmds, dat_off[n] = n_floats;
	const vgsdf::CommandStoreLayout at(n, n_cmds);
	if (needed)
		for (uint32_t p = 0; p < n_pos; p++)
			needed[p] = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (not one store fits: nothing allocated, no position looked at, as the single call)
	// the deltas pass: launches of glyph ids x positions whose points x positions stay within the single call's slice; a glyph id
	// that passes it with all positions goes alone, in runs of positions (at least one)
	struct Launch {
		uint32_t g0, g1, p0, p1;
	};
	std::vector<Launch> launches;
	size_t most = 0;
	for (uint32_t g0 = 0; g0 < n;) {
		uint32_t g1 = g0 + 1;
		const uint64_t own = pt_at[g1] - pt_at[g0];
		uint32_t step = n_pos;
		if (own * n_pos > vg::kGvarSlicePoints)
			step = (uint32_t)std::max<uint64_t>(1, vg::kGvarSlicePoints / own);
		else
			while (g1 < n && (uint64_t)(pt_at[g1 + 1] - pt_at[g0]) * n_pos <= vg::kGvarSlicePoints)
				g1++;
		const size_t slice = pt_at[g1] - pt_at[g0];
		for (uint32_t p0 = 0; slice && p0 < n_pos; p0 += step) {
			const uint32_t p1 = std::min(n_pos, p0 + step);
			launches.push_back(Launch{g0, g1, p0, p1});
			most = std::max(most, slice * (p1 - p0));
		}
		g0 = g1;
	}
	const size_t acc_stride = 2 * (size_t)points; // floats of one position's sums
	if (hipError_t err = sums.ensure(4 * acc_stride * n_pos + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	float *d_acc = (float *)sums.p;
	// sx | sy | x | y | mark, each 16-aligned, for the points x positions of a launch (nothing in flight reads the scratch: every
	// call that uses it ends with a synchronisation)
	auto scratch_bytes = [](size_t e, size_t *sy, size_t *x, size_t *y, size_t *mark) {
		*sy = align_up(4 * e, 16), *x = 2 * *sy, *y = *x + align_up(2 * e, 16), *mark = *y + align_up(2 * e, 16);
		return *mark + e;
	};
	size_t s_sy = 0, s_x = 0, s_y = 0, s_mark = 0;
	if (most)
		if (hipError_t err = ctx->gvar_scratch.ensure(scratch_bytes(most, &s_sy, &s_x, &s_y, &s_mark) + 16); err != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", err);
	q.copy(d_at, pt_at.data(), 4 * ((size_t)n + 1));
	q.record(ev.at[1]);
	for (const Launch &l : launches) {
		const uint32_t slice = pt_at[l.g1] - pt_at[l.g0];
		(void)scratch_bytes((size_t)slice * (l.p1 - l.p0), &s_sy, &s_x, &s_y, &s_mark);
		uint8_t *s = (uint8_t *)ctx->gvar_scratch.p;
		const vgsdf::GvarScratch scratch{(float *)s, (float *)(s + s_sy), (int16_t *)(s + s_x), (int16_t *)(s + s_y), s + s_mark};
		q.launch([&] {
			return vgsdf_gvar_batch_deltas(&face, l.g0, l.g1, l.p0, l.p1, d_coords, d_counts, d_at, d_acc, acc_stride, &scratch, slice, d_flags, st);
		});
	}
	q.record(ev_deltas);
	std::vector<uint32_t> flags((size_t)vgsdf::GVAR_FLAG_WORDS * n_pos, 0);
	q.read_back(flags.data(), d_flags, 4 * flags.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "deltas pass", q.e);
	(void)hipEventElapsedTime(&ctx->gvar_batch_ms[1], ev.at[1], ev_deltas);
	// per position: refused, passed over, or a font with its store
	std::vector<std::unique_ptr<vgsdf_font>> made(n_pos); // freed on every way out but the last
	std::vector<uint32_t> built;
	uint64_t room = max_store_bytes;
	for (uint32_t p = 0; p < n_pos; p++) {
		const uint32_t *f = flags.data() + (size_t)vgsdf::GVAR_FLAG_WORDS * p;
		if (f[vgsdf::GVAR_FLAG_MALFORMED] || f[vgsdf::GVAR_FLAG_DELTAS]) {
			ctx->err = std::string(name) + ": position " + std::to_string(p) +
			           (f[vgsdf::GVAR_FLAG_MALFORMED] ? ": a glyph with malformed variation data" : ": a glyph past VGSDF_GVAR_MAX_DELTAS");
			status[p] = VGSDF_E_GLYF;
			if (needed)
				needed[p] = 0;
			continue;
		}
		if (at.total > room)
			continue; // (out[p] stays NULL: passed over, the positions behind it go on with the same room)
		room -= at.total;
		std::unique_ptr<vgsdf_font> font(new vgsdf_font());
		font->slots = slots;
		font->device = ctx->device;
		font->n_glyph_ids = n;
		font->commands = true;
		if (hipError_t err = font->store.ensure(at.total + 16); err != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", err);
		made[p] = std::move(font);
		built.push_back(p);
	}
	if (built.empty())
		return VGSDF_OK;
	// what the context passes read, for the duration of this call: scale | dat_off (one for all: ContextStagingLayout's) | the
	// context passes' error words | per built position coords | kinds | pad to 16
	const uint32_t n_built = (uint32_t)built.size();
	const size_t t_dat = 8 * (size_t)n, t_flags = align_up(t_dat + 4 * ((size_t)n + 1), 16), t_first = t_flags + align_up(4 * (size_t)n_built, 16),
	             t_each = align_up(4 * (size_t)n_floats + n_cmds, 16);
	if (hipError_t err = tmp.ensure(t_first + t_each * n_built + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	uint8_t *t = (uint8_t *)tmp.p;
	const std::vector<double> ones(n, 1.0);
	q.copy(t, ones.data(), 8 * (size_t)n);
	q.copy(t + t_dat, dat_off.data(), 4 * ((size_t)n + 1));
	q.zero(t + t_flags, 4 * (size_t)n_built);
	std::vector<vgsdf::GvarPositionRef> rec(n_built);
	for (uint32_t k = 0; k < n_built; k++) {
		const uint32_t p = built[k];
		uint8_t *d = (uint8_t *)made[p]->store.p, *tp = t + t_first + t_each * k;
		q.copy(d + at.cmd_off, cmd_off.data(), 4 * ((size_t)n + 1));
		rec[k] = vgsdf::GvarPositionRef{d_acc + acc_stride * p, (const uint32_t *)(d + at.cmd_off), (const uint32_t *)(t + t_dat),
		                                tp + 4 * (size_t)n_floats, (float *)tp, d_flags + (size_t)vgsdf::GVAR_FLAG_WORDS * p};
	}
	q.copy(d_rec, rec.data(), sizeof(vgsdf::GvarPositionRef) * (size_t)n_built);
	q.record(ev.at[1]);
	if (n)
		q.launch([&] { return vgsdf_gvar_batch_emit(&face, d_rec, n_built, d_counts, d_at, st); });
	q.record(ev.at[2]);
	if (n_cmds)
		for (uint32_t k = 0; k < n_built; k++) {
			uint8_t *d = (uint8_t *)made[built[k]]->store.p;
			q.launch([&] {
				return vgsdf_outline_context_packed(rec[k].kinds, rec[k].coords, rec[k].dat_off, rec[k].cmd_off, (const double *)t, n, (vgsdf::OutlineCmd *)d,
				                                    d + at.open, (uint32_t *)(t + t_flags) + k, q.st);
			});
		}
	std::vector<uint32_t> context_flags(n_built, 0);
	q.read_back(context_flags.data(), t + t_flags, 4 * (size_t)n_built);
	q.read_back(flags.data(), d_flags, 4 * flags.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "emit pass", q.e);
	(void)hipEventElapsedTime(&ctx->gvar_batch_ms[2], ev.at[1], ev.at[2]);
	for (uint32_t k = 0; k < n_built; k++)
		if (context_flags[k] || flags[(size_t)vgsdf::GVAR_FLAG_WORDS * built[k] + vgsdf::GVAR_FLAG_EMIT]) { // (one text over the same bytes)
			ctx->err = "vgsdf_fonts_create_gvar: the emit pass did not match the count pass, or the context pass refused the commands";
			return VGSDF_E_HIP;
		}
	for (uint32_t p : built) {
		name_command_store(*made[p], at, n_cmds);
		out[p] = made[p].release();
	}
	return VGSDF_OK;
}
} // namespace

extern "C" {

int vgsdf_fonts_create_gvar_within(vgsdf_ctx *ctx, const vgsdf_fonts_gvar_desc *in, uint64_t max_store_bytes, vgsdf_font **out, int *status,
                                   uint64_t *needed)
{
	if (!ctx)
		return VGSDF_E_ARG;
	try {
		return create_gvar_batch(ctx, in, max_store_bytes, out, status, needed);
	} catch (const std::bad_alloc &) { // (the fonts made so far are freed on the way here; out[] holds none of them)
		ctx->err = "vgsdf_fonts_create_gvar: out of host memory";
		return VGSDF_E_OOM;
	}
}

int vgsdf_fonts_create_gvar(vgsdf_ctx *ctx, const vgsdf_fonts_gvar_desc *in, vgsdf_font **out, int *status)
{
	return vgsdf_fonts_create_gvar_within(ctx, in, ~0ull, out, status, nullptr);
}

void vgsdf_fonts_gvar_kernel_ms(const vgsdf_ctx *ctx, float ms[3])
{
	if (ms)
		for (int i = 0; i < 3; i++)
			ms[i] = ctx ? ctx->gvar_batch_ms[i] : 0.0f;
}

} // extern "C"

namespace {
// vgsdf_font_create_tables_within over all faces at once: its checks, sums and layout per face, its two passes and its
// synchronisations once per call (glyf_table_kernels.h, GlyfFaceRecord)
int create_tables_batch(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *faces, uint32_t n_faces, uint64_t max_store_bytes, vgsdf_font **out,
                        int *status, uint64_t *needed)
{
	const char *name = "vgsdf_fonts_create_tables";
	if (!ctx)
		return VGSDF_E_ARG;
	ctx->glyf_batch_ms[0] = ctx->glyf_batch_ms[1] = 0.0f;
	if (n_faces == 0)
		return VGSDF_OK;
	if (!faces || !out || !status) {
		ctx->err = "vgsdf_fonts_create_tables: NULL argument";
		return VGSDF_E_ARG;
	}
	if (n_faces > vgsdf::kGlyfBatchMaxFaces) {
		ctx->err = "vgsdf_fonts_create_tables: more than 65536 faces in one call";
		return VGSDF_E_ARG;
	}
	// the descriptions, each by the single call's rules: a bad one fails its own face; the good ones' glyph ids bound the call
	std::vector<uint8_t> described(n_faces, 0);
	uint64_t sum_glyphs = 0;
	for (uint32_t f = 0; f < n_faces; f++) {
		const vgsdf_font_tables_desc &in = faces[f];
		described[f] = !((in.n_loca_bytes && !in.loca) || (in.n_glyf_bytes && !in.glyf) || in.num_glyphs > 0xFFFFu || in.loca_long > 1u ||
		                 (uint64_t)in.loca_entries * (in.loca_long ? 4u : 2u) > in.n_loca_bytes || in.loca_entries > in.num_glyphs + 1);
		if (described[f])
			sum_glyphs += in.num_glyphs;
	}
	if (sum_glyphs > vgsdf::kGlyfBatchMaxGlyphIds) {
		ctx->err = "vgsdf_fonts_create_tables: more than 2^22 glyph ids in one call";
		return VGSDF_E_ARG;
	}
	for (uint32_t f = 0; f < n_faces; f++) {
		out[f] = nullptr, status[f] = described[f] ? VGSDF_OK : VGSDF_E_ARG;
		if (needed)
			needed[f] = 0;
		if (!described[f])
			ctx->err = "vgsdf_fonts_create_tables: face " + std::to_string(f) + ": a NULL table, more than 65535 glyphs, loca_long not 0 or 1, or more loca entries than the loca bytes hold or than num_glyphs + 1";
	}
	std::vector<std::unique_ptr<vgsdf_font>> made(n_faces); // freed on every way out but the last
	{
		(void)hipSetDevice(ctx->device);
		hipStream_t st = ctx->stream;
		PassEvents ev;
		if (hipError_t err = ev.create(); err != hipSuccess)
			return font_hip_error(ctx, name, "hipEventCreate", err);
		// the batch on the device, for the duration of this call:
		// every face's loca, glyf (each 16-aligned) | counts (4 per glyph id) | flags (4 per face) | face records | byte_at (n + 1 per face)
		// and the last three on the host in that order: the count pass takes zeroed flags and the records in one copy, the emit pass
		// the records and byte_at in one, the read-backs counts and flags in one
		const size_t total = (size_t)sum_glyphs;
		const size_t flag_bytes = 4 * (size_t)vgsdf::GLYF_FLAG_WORDS * n_faces, rec_bytes = sizeof(vgsdf::GlyfFaceRecord) * (size_t)n_faces;
		std::vector<uint64_t> up((flag_bytes + rec_bytes + 4 * (total + n_faces) + 7) / 8, 0);
		vgsdf::GlyfFaceRecord *rec = (vgsdf::GlyfFaceRecord *)((uint8_t *)up.data() + flag_bytes);
		uint32_t *byte_at = (uint32_t *)((uint8_t *)up.data() + flag_bytes + rec_bytes);
		std::vector<size_t> a_loca(n_faces, 0);
		size_t at_end = 0;
		uint32_t n_blocks = 0, glyph_base = 0;
		for (uint32_t f = 0; f < n_faces; f++) {
			vgsdf::GlyfFaceRecord &r = rec[f];
			r = vgsdf::GlyfFaceRecord{};
			r.first_block = n_blocks, r.glyph_base = glyph_base;
			if (!described[f])
				continue;
			const vgsdf_font_tables_desc &in = faces[f];
			a_loca[f] = at_end;
			at_end = align_up(align_up(at_end + in.n_loca_bytes, 16) + in.n_glyf_bytes, 16);
			r.glyf_len = in.n_glyf_bytes, r.loca_entries = in.loca_entries, r.loca_long = in.loca_long, r.n_glyph_ids = in.num_glyphs;
			r.takes_part = 1;
			n_blocks += (in.num_glyphs + vgsdf::kGlyfTableLanes - 1) / vgsdf::kGlyfTableLanes;
			glyph_base += in.num_glyphs;
		}
		const size_t a_counts = at_end, a_flags = a_counts + 4 * (size_t)vgsdf::kGlyfTableCounts * total, a_rec = a_flags + flag_bytes,
		             a_at = a_rec + rec_bytes, a_total = a_at + 4 * (total + n_faces);
		ScratchBuf dev;
		if (hipError_t e = dev.ensure(a_total + 16); e != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", e);
		uint8_t *a = (uint8_t *)dev.p;
		Calls q(st);
		for (uint32_t f = 0; f < n_faces; f++)
			if (described[f]) {
				const size_t a_glyf = align_up(a_loca[f] + faces[f].n_loca_bytes, 16);
				q.copy(a + a_loca[f], faces[f].loca, faces[f].n_loca_bytes);
				q.copy(a + a_glyf, faces[f].glyf, faces[f].n_glyf_bytes);
				rec[f].loca = (uintptr_t)(a + a_loca[f]), rec[f].glyf = (uintptr_t)(a + a_glyf);
			}
		q.copy(a + a_flags, up.data(), flag_bytes + rec_bytes);
		const vgsdf::GlyfFaceRecord *d_rec = (const vgsdf::GlyfFaceRecord *)(a + a_rec);
		uint32_t *d_counts = (uint32_t *)(a + a_counts), *d_flags = (uint32_t *)(a + a_flags), *d_at = (uint32_t *)(a + a_at);
		q.record(ev.at[0]);
		if (n_blocks)
			q.launch([&] { return vgsdf_glyf_tables_batch_count(d_rec, n_faces, n_blocks, d_counts, d_flags, st); });
		q.record(ev.at[1]);
		// all counts and, behind them, all flag words: one read-back
		std::vector<uint32_t> got((size_t)vgsdf::kGlyfTableCounts * total + (size_t)vgsdf::GLYF_FLAG_WORDS * n_faces);
		q.read_back(got.data(), d_counts, 4 * got.size());
		q.sync();
		if (q.failed())
			return font_hip_error(ctx, name, "count pass", q.e);
		ev.elapsed(ctx->glyf_batch_ms, 0);
		// per face: the running sums and the bounds of the host's table (glyf_table_limits.h), the limit, the store
		uint64_t room = max_store_bytes;
		uint32_t emit_blocks = 0;
		for (uint32_t f = 0; f < n_faces; f++) {
			vgsdf::GlyfFaceRecord &r = rec[f];
			r.first_block = emit_blocks, r.takes_part = 0;
			if (!described[f])
				continue;
			const uint32_t n = r.n_glyph_ids;
			const uint32_t *fl = got.data() + (size_t)vgsdf::kGlyfTableCounts * total + (size_t)vgsdf::GLYF_FLAG_WORDS * f;
			const std::string face = "vgsdf_fonts_create_tables: face " + std::to_string(f) + ": ";
			if (fl[vgsdf::GLYF_FLAG_BUDGET] || fl[vgsdf::GLYF_FLAG_SLOTS]) {
				ctx->err = face + (fl[vgsdf::GLYF_FLAG_BUDGET] ? "a glyph past VGSDF_GLYF_MAX_COMPONENTS" : "a glyph of more than 2^26 command slots");
				status[f] = VGSDF_E_GLYF;
				continue;
			}
			std::unique_ptr<vgsdf_font> font(new vgsdf_font());
			uint32_t *at_f = byte_at + r.glyph_base + f;
			font->leaf_off.assign((size_t)n + 1, 0);
			font->slots.assign(n, 0);
			uint64_t n_bytes = 0, n_leaves = 0, slot_sum = 0;
			bool inside = true;
			for (uint32_t g = 0; g < n && inside; g++) {
				const uint32_t *c = got.data() + (size_t)vgsdf::kGlyfTableCounts * (r.glyph_base + g);
				at_f[g] = (uint32_t)n_bytes, font->leaf_off[g] = (uint32_t)n_leaves;
				font->slots[g] = c[2];
				n_bytes += align_up(c[0], 4), n_leaves += c[1], slot_sum += c[2];
				inside = n_bytes <= vg::kResidentMaxBytes && n_leaves <= vg::kResidentMaxLeaves && slot_sum <= vg::kResidentMaxSlotSum;
				font->max_cap = std::max(font->max_cap, c[3]); // (every simple entry a leaf names is some glyph id's own)
				font->max_len = std::max(font->max_len, c[0]);
			}
			if (!inside) {
				ctx->err = face + "more than 2^22 leaves, a store past 2^32 - 4 bytes, or command slots that sum past 2^32 - 1";
				status[f] = VGSDF_E_GLYF;
				continue;
			}
			at_f[n] = (uint32_t)n_bytes, font->leaf_off[n] = (uint32_t)n_leaves;
			const vgsdf::GlyfStoreLayout at(n, n_leaves, n_bytes);
			if (needed)
				needed[f] = at.total;
			if (at.total > room)
				continue; // (out[f] stays NULL: passed over, the faces behind it go on with the same room)
			room -= at.total;
			font->device = ctx->device;
			font->n_glyph_ids = n;
			font->n_leaves = (uint32_t)n_leaves;
			font->n_bytes = (uint32_t)n_bytes;
			if (hipError_t err = font->store.ensure(at.total + 16); err != hipSuccess)
				return font_hip_error(ctx, name, "hipMalloc", err);
			name_glyf_store(*font, at);
			r.store = (uintptr_t)font->store.p, r.bytes_at = (uint32_t)at.bytes, r.leaf_off_at16 = (uint32_t)(at.leaf_off / 16);
			r.takes_part = 1;
			emit_blocks += (n + vgsdf::kGlyfTableLanes - 1) / vgsdf::kGlyfTableLanes;
			made[f] = std::move(font);
		}
		// the stores' leaf_off (one copy each: every font owns its allocation); the records of the emit pass and all byte_at (one copy)
		for (uint32_t f = 0; f < n_faces; f++)
			if (made[f])
				q.copy((void *)(uintptr_t)made[f]->ref.leaf_off, made[f]->leaf_off.data(), 4 * ((size_t)made[f]->n_glyph_ids + 1));
		q.copy(a + a_rec, rec, rec_bytes + 4 * (total + n_faces));
		q.record(ev.at[1]);
		if (emit_blocks)
			q.launch([&] { return vgsdf_glyf_tables_batch_emit(d_rec, n_faces, emit_blocks, d_at, d_flags, st); });
		q.record(ev.at[2]);
		std::vector<uint32_t> flags((size_t)vgsdf::GLYF_FLAG_WORDS * n_faces);
		q.read_back(flags.data(), d_flags, 4 * flags.size());
		q.sync();
		if (q.failed())
			return font_hip_error(ctx, name, "emit pass", q.e);
		if (emit_blocks)
			ev.elapsed(ctx->glyf_batch_ms, 1);
		for (uint32_t f = 0; f < n_faces; f++)
			if (made[f] && flags[(size_t)vgsdf::GLYF_FLAG_WORDS * f + vgsdf::GLYF_FLAG_EMIT]) { // (the two passes walk one text over the same bytes)
				ctx->err = "vgsdf_fonts_create_tables: the emit pass did not match the count pass";
				return VGSDF_E_HIP;
			}
	}
	for (uint32_t f = 0; f < n_faces; f++)
		out[f] = made[f].release();
	return VGSDF_OK;
}
} // namespace

extern "C" {

int vgsdf_fonts_create_tables_within(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *faces, uint32_t n_faces, uint64_t max_store_bytes,
                                     vgsdf_font **out, int *status, uint64_t *needed)
{
	try {
		return create_tables_batch(ctx, faces, n_faces, max_store_bytes, out, status, needed);
	} catch (const std::bad_alloc &) { // (the fonts made so far are freed on the way here; out[] holds none of them)
		ctx->err = "vgsdf_fonts_create_tables: out of host memory";
		return VGSDF_E_OOM;
	}
}

int vgsdf_fonts_create_tables(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *faces, uint32_t n_faces, vgsdf_font **out, int *status)
{
	return vgsdf_fonts_create_tables_within(ctx, faces, n_faces, ~0ull, out, status, nullptr);
}

void vgsdf_fonts_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2]) { pass_ms_out(ctx ? ctx->glyf_batch_ms : nullptr, ms); }

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
	// (the arrays' sizes as GlyfStoreLayout states them; spelled out because HIP_TRY's error text is the call's own)
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

} // extern "C"
