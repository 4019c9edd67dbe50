// resident_charstrings.cpp — command stores the device decodes from a CFF or CFF2 face's charstrings (vgsdf_font_create_charstrings,
// _charstrings2 and their _within forms; charstring_kernels.h): count pass, the store's layout from its counts, emit pass, context
// pass (resident_command_store.h).
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "charstring_kernels.h"
#include "charstring_limits.h"
#include "resident_command_store.h"

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
	CommandSums sums; // (commands, coordinates per glyph id)
	if (!sums.fill(counts.data(), n, 2, 0, 1)) {
		ctx->err = entry + kCommandStorePast;
		return VGSDF_E_GLYF;
	}
	const uint32_t n_cmds = sums.n_cmds, n_floats = sums.n_floats;
	const std::vector<uint32_t> &cmd_off = sums.cmd_off, &dat_off = sums.dat_off;
	const vgsdf::CommandStoreLayout at(n, n_cmds);
	if (store_bytes)
		*store_bytes = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->commands = true;
	f->slots.swap(sums.slots);
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

} // extern "C"
