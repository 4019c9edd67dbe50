// resident_charstrings.cpp — command stores the device decodes from a CFF or CFF2 face's charstrings (vgsdf_font_create_charstrings,
// _charstrings2 and their _within forms; charstring_kernels.h): count pass, the store's layout from its counts, emit pass, context
// pass (resident_command_store.h).  vgsdf_fonts_create_charstrings2 builds the stores of one CFF2 face at many positions in one
// call, both passes over (glyph id, position) pairs (charstring_batch_kernels.h); validation, arena and workspace are one text for
// all of them.
#include <algorithm>
#include <cmath>
#include <memory>
#include <new>

#include "charstring_batch_kernels.h"
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

// what both CFF2 calls and the version 1 call are given of a face: every array there
bool charstrings_given(const vgsdf_font_charstrings_desc &in)
{
	return in.cs_off && in.gsubr_off && in.lsubr_first && in.lsubr_off && !(in.n_bytes && !in.bytes) && !(in.n_fds > 1 && !in.fd_of);
}

// What every constructor validates of a description before anything runs: every range the device will read (blend == nullptr: a
// version 1 face; n_positions: how many times n_factors factors stand at blend->factors).  false: ctx->err says why, behind `entry`
bool charstrings_described(vgsdf_ctx *ctx, const std::string &entry, const vgsdf_font_charstrings_desc *in, const BlendSets *blend,
                           uint32_t n_positions)
{
	const uint32_t n = in->n_glyph_ids, n_bytes = in->n_bytes;
	if (blend) {
		if (in->n_fds != 1 || in->fd_of) {
			ctx->err = entry + "n_fds must be 1 and fd_of NULL";
			return false;
		}
		if (blend->n_sets > 0x10000u || (blend->n_sets && (!blend->set_ok || !blend->set_off)) || (blend->n_factors && !blend->factors)) {
			ctx->err = entry + "more than 65536 blend sets, or a NULL array of them";
			return false;
		}
		if (blend->n_sets && blend->set_off[0] != 0) {
			ctx->err = entry + "set_off does not start at 0";
			return false;
		}
		for (uint32_t s = 0; s < blend->n_sets; s++)
			if (blend->set_off[s + 1] < blend->set_off[s] || blend->set_off[s + 1] - blend->set_off[s] > (uint32_t)vg::kCharstringMaxRegions ||
			    blend->set_off[s + 1] > blend->n_factors) {
				ctx->err = entry + "set_off not ascending, a set of more than 64 factors, or one ending past n_factors";
				return false;
			}
		for (size_t i = 0; i < (size_t)blend->n_factors * n_positions; i++)
			if (!std::isfinite(blend->factors[i])) {
				ctx->err = entry + "a factor that is not finite";
				return false;
			}
	}
	if (n == 0 || n > 0x10000u || (n_bytes & 3u) || n_bytes > 0xFFFFFFF0u || in->n_gsubrs > 0xFFFFu || in->n_fds == 0 || in->n_fds > 256u) {
		ctx->err = entry + "glyph ids not 1 .. 65536, n_bytes not a multiple of 4 (or past 2^32 - 16), more than "
		           "65535 global subroutines, or Font DICTs not 1 .. 256";
		return false;
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
		return false;
	}
	for (uint32_t k = 0; k < in->n_fds; k++)
		if (in->lsubr_first[k + 1] < in->lsubr_first[k] || in->lsubr_first[k + 1] - in->lsubr_first[k] > 0xFFFFu) {
			ctx->err = entry + "lsubr_first not ascending, or a Font DICT of more than 65535 local subroutines";
			return false;
		}
	const uint32_t n_lsubrs = in->lsubr_first[in->n_fds];
	if (!ascends_inside(in->cs_off, n) || !ascends_inside(in->gsubr_off, in->n_gsubrs) || !ascends_inside(in->lsubr_off, n_lsubrs)) {
		ctx->err = entry + "cs_off, gsubr_off or lsubr_off not ascending, or ending past n_bytes";
		return false;
	}
	if (in->fd_of)
		for (uint32_t g = 0; g < n; g++)
			if (in->fd_of[g] >= in->n_fds) {
				ctx->err = entry + "an fd_of past n_fds";
				return false;
			}
	return true;
}

// The description on the device, for the duration of a call:
// bytes | cs_off | gsubr_off | lsubr_first | lsubr_off | counts (commands, coordinates per glyph id and position) | flags (a word
// per position, padded to 16) | fd_of
// CFF2, behind them: set_off | factors (n_factors per position) | set_ok | the batched call's position records, 16-aligned
struct CharstringArenaLayout {
	size_t bytes = 0, cs, gs, lf, lo, counts, flags, fd, so, fac, ok, records, total;
	constexpr CharstringArenaLayout(size_t n_bytes, size_t n, size_t n_gsubrs, size_t n_fds, size_t n_lsubrs, bool fd_of, bool cff2, size_t n_sets,
	                                size_t n_factors, size_t n_pos, size_t record_bytes)
	    : cs(align_up(n_bytes, 16)), gs(cs + 4 * (n + 1)), lf(gs + 4 * (n_gsubrs + 1)), lo(lf + 4 * (n_fds + 1)), counts(lo + 4 * (n_lsubrs + 1)),
	      flags(counts + 8 * n * n_pos), fd(flags + align_up(4 * n_pos, 16)), so(align_up(fd + (fd_of ? n : 0), 16)), fac(so + 4 * (n_sets + 1)),
	      ok(fac + 4 * n_factors * n_pos), records(record_bytes ? align_up(ok + n_sets, 16) : ok + n_sets),
	      total(cff2 ? records + record_bytes * n_pos : fd + (fd_of ? n : 0))
	{
	}
};
static_assert(CharstringArenaLayout(10, 3, 1, 2, 4, true, false, 0, 0, 1, 0).counts == 16 + 16 + 8 + 12 + 20 &&
                  CharstringArenaLayout(10, 3, 1, 2, 4, true, false, 0, 0, 1, 0).fd == 72 + 24 + 16 &&
                  CharstringArenaLayout(10, 3, 1, 2, 4, true, false, 0, 0, 1, 0).total == 115 &&
                  CharstringArenaLayout(10, 3, 1, 1, 4, false, true, 2, 5, 1, 0).so == 112 && CharstringArenaLayout(10, 3, 1, 1, 4, false, true, 2, 5, 1, 0).total == 112 + 12 + 20 + 2,
              "one position: the arena as the single calls have always laid it out");
static_assert(CharstringArenaLayout(10, 3, 1, 1, 4, false, true, 2, 5, 5, 48).flags == 68 + 120 && CharstringArenaLayout(10, 3, 1, 1, 4, false, true, 2, 5, 5, 48).fd == 188 + 32 &&
                  CharstringArenaLayout(10, 3, 1, 1, 4, false, true, 2, 5, 5, 48).ok == 224 + 12 + 100 && CharstringArenaLayout(10, 3, 1, 1, 4, false, true, 2, 5, 5, 48).records == 352,
              "counts, flag words and factors per position, the records 16-aligned behind set_ok");

// uploads the face and the positions' factors, zeroes the flag words and names it all in `face` (a version 1 face: its
// CharstringsRef part; face.factors: the first position's)
void upload_charstring_face(Calls &q, uint8_t *a, const CharstringArenaLayout &at, const vgsdf_font_charstrings_desc &in, const BlendSets *blend,
                            uint32_t n_pos, vgsdf::Charstrings2Ref &face)
{
	const uint32_t n = in.n_glyph_ids, n_lsubrs = in.lsubr_first[in.n_fds];
	const uint32_t n_sets = blend ? blend->n_sets : 0, n_factors = blend ? blend->n_factors : 0;
	q.copy(a, in.bytes, in.n_bytes);
	q.copy(a + at.cs, in.cs_off, 4 * ((size_t)n + 1));
	q.copy(a + at.gs, in.gsubr_off, 4 * ((size_t)in.n_gsubrs + 1));
	q.copy(a + at.lf, in.lsubr_first, 4 * ((size_t)in.n_fds + 1));
	q.copy(a + at.lo, in.lsubr_off, 4 * ((size_t)n_lsubrs + 1));
	if (in.fd_of)
		q.copy(a + at.fd, in.fd_of, n);
	if (n_sets)
		q.copy(a + at.so, blend->set_off, 4 * ((size_t)n_sets + 1));
	if (n_factors)
		q.copy(a + at.fac, blend->factors, 4 * (size_t)n_factors * n_pos);
	if (n_sets)
		q.copy(a + at.ok, blend->set_ok, n_sets);
	q.zero(a + at.flags, at.fd - at.flags);
	face.words = (const uint32_t *)a;
	face.cs_off = (const uint32_t *)(a + at.cs);
	face.gsubr_off = (const uint32_t *)(a + at.gs);
	face.lsubr_first = (const uint32_t *)(a + at.lf);
	face.lsubr_off = (const uint32_t *)(a + at.lo);
	face.fd_of = in.fd_of ? a + at.fd : nullptr;
	face.n_glyph_ids = n;
	face.n_gsubrs = in.n_gsubrs;
	if (blend) {
		face.set_ok = a + at.ok;
		face.set_off = (const uint32_t *)(a + at.so);
		face.factors = (const float *)(a + at.fac);
		face.n_sets = n_sets;
	}
}

// the context's workspace: the operand slots past the decoder's LDS window, for one launch of `lanes` lanes (at most 465 x 4 x
// 16384 B); names it in `face`
hipError_t charstring_workspace(vgsdf_ctx *ctx, uint32_t lanes, vgsdf::Charstrings2Ref &face)
{
	face.spill_stride = (lanes + 63u) & ~63u;
	const size_t want = 4 * (size_t)(vg::kCharstringMaxOperands2 - vg::kCharstringWindow) * face.spill_stride;
	if (want > ctx->charstring_spill_bytes) {
		if (ctx->charstring_spill)
			(void)hipFree(ctx->charstring_spill); // (nothing in flight reads it: every call ends synchronised)
		ctx->charstring_spill = nullptr;
		ctx->charstring_spill_bytes = 0;
		if (hipError_t err = hipMalloc(&ctx->charstring_spill, want); err != hipSuccess) {
			ctx->charstring_spill = nullptr;
			return err;
		}
		ctx->charstring_spill_bytes = want;
	}
	face.spill = (float *)ctx->charstring_spill;
	return hipSuccess;
}

// vgsdf_font_create_charstrings_within (blend == nullptr) and vgsdf_font_create_charstrings2_within: one sequence
int create_charstrings(vgsdf_ctx *ctx, const vgsdf_font_charstrings_desc *in, const BlendSets *blend, uint64_t max_store_bytes,
                       vgsdf_font **out, uint64_t *store_bytes)
{
	const char *name = blend ? "vgsdf_font_create_charstrings2" : "vgsdf_font_create_charstrings";
	const std::string entry = std::string(name) + ": ";
	if (!in || !out || !charstrings_given(*in)) {
		ctx->err = entry + "NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (store_bytes)
		*store_bytes = 0;
	if (!charstrings_described(ctx, entry, in, blend, 1))
		return VGSDF_E_ARG;
	const uint32_t n = in->n_glyph_ids;
	std::unique_ptr<vgsdf_font> f(new (std::nothrow) vgsdf_font());
	if (!f) {
		ctx->err = entry + "out of host memory";
		return VGSDF_E_OOM;
	}
	ctx->charstring_ms[0] = ctx->charstring_ms[1] = 0.0f;
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	const CharstringArenaLayout arena(in->n_bytes, n, in->n_gsubrs, in->n_fds, in->lsubr_first[in->n_fds], in->fd_of != nullptr, blend != nullptr,
	                                  blend ? blend->n_sets : 0, blend ? blend->n_factors : 0, 1, 0);
	const size_t a_counts = arena.counts, a_flags = arena.flags;
	ScratchBuf face_buf, tmp;
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	if (hipError_t e = face_buf.ensure(arena.total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)face_buf.p;
	Calls q(st);
	vgsdf::Charstrings2Ref face{}; // (a version 1 face: its CharstringsRef part)
	upload_charstring_face(q, a, arena, *in, blend, 1, face);
	if (blend)
		if (hipError_t err = charstring_workspace(ctx, std::min(kChunkGlyphIds, n), face); err != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", err);
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

// vgsdf_fonts_create_charstrings2_within: create_charstrings for one CFF2 face at all the positions of a call.  The description
// goes up once; both passes run over (glyph id, position) pairs (charstring_batch_kernels.hip), because what a glyph delivers may
// depend on the position: counts, running sums, layout and store size are each position's own.  One read-back of all counts and
// flag words behind the count pass, the context pass once per store, two synchronisations for the whole call
int create_charstrings2_batch(vgsdf_ctx *ctx, const vgsdf_fonts_charstrings2_desc *desc, uint64_t max_store_bytes, vgsdf_font **out, int *status,
                              uint64_t *needed)
{
	const char *name = "vgsdf_fonts_create_charstrings2";
	const std::string entry = std::string(name) + ": ";
	if (!desc) {
		ctx->err = entry + "NULL argument";
		return VGSDF_E_ARG;
	}
	const uint32_t n_pos = desc->n_positions;
	if (n_pos == 0)
		return VGSDF_OK;
	const vgsdf_font_charstrings_desc *in = &desc->face.charstrings;
	if (!out || !status || !charstrings_given(*in)) {
		ctx->err = entry + "NULL argument";
		return VGSDF_E_ARG;
	}
	if (n_pos > VGSDF_CHARSTRING2_MAX_POSITIONS) {
		ctx->err = entry + "more than 64 positions in one call";
		return VGSDF_E_ARG;
	}
	for (uint32_t p = 0; p < n_pos; p++) {
		out[p] = nullptr, status[p] = VGSDF_OK;
		if (needed)
			needed[p] = 0;
	}
	ctx->charstring_batch_ms[0] = ctx->charstring_batch_ms[1] = 0.0f;
	const BlendSets blend{desc->face.n_sets, desc->face.n_factors, desc->face.set_ok, desc->face.set_off, desc->face.factors};
	if (!charstrings_described(ctx, entry, in, &blend, n_pos))
		return VGSDF_E_ARG;
	const uint32_t n = in->n_glyph_ids;
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	const CharstringArenaLayout arena(in->n_bytes, n, in->n_gsubrs, 1, in->lsubr_first[1], false, true, blend.n_sets, blend.n_factors, n_pos,
	                                  sizeof(vgsdf::Charstrings2PositionRef));
	ScratchBuf face_buf, tmp;
	if (hipError_t e = face_buf.ensure(arena.total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)face_buf.p;
	Calls q(st);
	vgsdf::Charstrings2Ref face{};
	upload_charstring_face(q, a, arena, *in, &blend, n_pos, face);
	// a launch: the glyph ids whose pairs stay within kChunkGlyphIds lanes (at least one glyph id), one after the other over the workspace
	const uint32_t per_launch = std::max(1u, kChunkGlyphIds / n_pos);
	if (hipError_t err = charstring_workspace(ctx, std::min(per_launch, n) * n_pos, face); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	uint32_t *d_counts = (uint32_t *)(a + arena.counts), *d_flags = (uint32_t *)(a + arena.flags);
	vgsdf::Charstrings2PositionRef *d_rec = (vgsdf::Charstrings2PositionRef *)(a + arena.records);
	auto run_pass = [&](bool emit, uint32_t n_rec) -> hipError_t {
		for (uint32_t g0 = 0; g0 < n; g0 += per_launch) {
			vgsdf::Charstrings2Ref part = face;
			part.n_glyph_ids = std::min(n, g0 + per_launch); // (the launch's last glyph id: the arrays stay the face's)
			const hipError_t err = (hipError_t)(emit ? vgsdf_charstring2_batch_emit(&part, g0, d_rec, n_rec, st)
			                                         : vgsdf_charstring2_batch_count(&part, g0, d_rec, n_rec, d_counts, st));
			if (err != hipSuccess)
				return err;
		}
		return hipSuccess;
	};
	// the count pass: of every position its factors and its flag word
	std::vector<vgsdf::Charstrings2PositionRef> rec(n_pos);
	for (uint32_t p = 0; p < n_pos; p++)
		rec[p] = vgsdf::Charstrings2PositionRef{face.factors + (size_t)blend.n_factors * p, nullptr, nullptr, nullptr, nullptr, d_flags + p};
	q.copy(d_rec, rec.data(), sizeof(vgsdf::Charstrings2PositionRef) * (size_t)n_pos);
	q.record(ev.at[0]);
	q.launch([&] { return run_pass(false, n_pos); });
	q.record(ev.at[1]);
	std::vector<uint32_t> counts(2 * (size_t)n * n_pos), flags(n_pos, 0);
	q.read_back(counts.data(), d_counts, 4 * counts.size());
	q.read_back(flags.data(), d_flags, 4 * (size_t)n_pos);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "count pass", q.e);
	ev.elapsed(ctx->charstring_batch_ms, 0);
	// per position: refused, passed over, or a font with its store
	struct Built {
		uint32_t p;
		CommandSums sums;
		size_t t_at; // its staging in tmp
	};
	std::vector<std::unique_ptr<vgsdf_font>> made(n_pos); // freed on every way out but the last
	std::vector<Built> built;
	uint64_t room = max_store_bytes;
	size_t t_total = 0;
	for (uint32_t p = 0; p < n_pos; p++) {
		CommandSums sums; // (commands, coordinates per glyph id, at this position)
		const char *refused = flags[p] ? "a glyph past VGSDF_CHARSTRING_MAX_TOKENS" : nullptr;
		if (!refused && !sums.fill(counts.data() + 2 * (size_t)p, n, 2 * n_pos, 0, 1))
			refused = kCommandStorePast;
		if (refused) {
			ctx->err = entry + "position " + std::to_string(p) + ": " + refused;
			status[p] = VGSDF_E_GLYF;
			continue;
		}
		const vgsdf::CommandStoreLayout at(n, sums.n_cmds);
		if (needed)
			needed[p] = at.total;
		if (at.total > room)
			continue; // (out[p] stays NULL: passed over, the positions behind it go on with the same room)
		room -= at.total;
		std::unique_ptr<vgsdf_font> font(new vgsdf_font());
		font->device = ctx->device;
		font->n_glyph_ids = n;
		font->commands = true;
		font->slots = sums.slots;
		if (hipError_t err = font->store.ensure(at.total + 16); err != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", err);
		made[p] = std::move(font);
		built.push_back(Built{p, std::move(sums), t_total});
		t_total += ContextStagingLayout(n, built.back().sums.n_cmds, built.back().sums.n_floats).total;
	}
	if (built.empty())
		return VGSDF_OK;
	// the emit pass over the built positions' pairs, into each store's staging (ContextStagingLayout, one behind the other)
	const uint32_t n_built = (uint32_t)built.size();
	if (hipError_t err = tmp.ensure(t_total + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	uint8_t *t0 = (uint8_t *)tmp.p;
	const std::vector<double> ones(n, 1.0);
	uint64_t all_cmds = 0;
	for (uint32_t k = 0; k < n_built; k++) {
		const Built &b = built[k];
		const vgsdf::CommandStoreLayout at(n, b.sums.n_cmds);
		const ContextStagingLayout tat(n, b.sums.n_cmds, b.sums.n_floats);
		uint8_t *d = (uint8_t *)made[b.p]->store.p, *t = t0 + b.t_at;
		q.copy(d + at.cmd_off, b.sums.cmd_off.data(), 4 * ((size_t)n + 1));
		q.copy(t + tat.scale, ones.data(), 8 * (size_t)n);
		q.copy(t + tat.dat_off, b.sums.dat_off.data(), 4 * ((size_t)n + 1));
		q.zero(t + tat.flag, 16);
		rec[k] = vgsdf::Charstrings2PositionRef{face.factors + (size_t)blend.n_factors * b.p, (const uint32_t *)(d + at.cmd_off),
		                                        (const uint32_t *)(t + tat.dat_off), t + tat.kinds, (float *)(t + tat.coords), d_flags + b.p};
		all_cmds += b.sums.n_cmds;
	}
	q.copy(d_rec, rec.data(), sizeof(vgsdf::Charstrings2PositionRef) * (size_t)n_built);
	q.record(ev.at[1]);
	if (all_cmds)
		q.launch([&] { return run_pass(true, n_built); });
	q.record(ev.at[2]);
	std::vector<uint32_t> context_flags(n_built, 0);
	for (uint32_t k = 0; k < n_built; k++) {
		const Built &b = built[k];
		const vgsdf::CommandStoreLayout at(n, b.sums.n_cmds);
		const ContextStagingLayout tat(n, b.sums.n_cmds, b.sums.n_floats);
		uint8_t *d = (uint8_t *)made[b.p]->store.p, *t = t0 + b.t_at;
		if (b.sums.n_cmds)
			q.launch([&] {
				return vgsdf_outline_context_packed(t + tat.kinds, (const float *)(t + tat.coords), (const uint32_t *)(t + tat.dat_off),
				                                    (const uint32_t *)(d + at.cmd_off), (const double *)(t + tat.scale), n, (vgsdf::OutlineCmd *)d,
				                                    d + at.open, (uint32_t *)(t + tat.flag), q.st);
			});
		q.read_back(&context_flags[k], t + tat.flag, 4);
	}
	q.read_back(flags.data(), d_flags, 4 * (size_t)n_pos);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "emit pass", q.e);
	if (all_cmds)
		ev.elapsed(ctx->charstring_batch_ms, 1);
	for (uint32_t k = 0; k < n_built; k++)
		if (context_flags[k] || flags[built[k].p]) { // (the two passes walk one text over the same bytes)
			ctx->err = entry + "the emit pass did not match the count pass, or the context pass refused the commands";
			return VGSDF_E_HIP;
		}
	for (const Built &b : built) {
		name_command_store(*made[b.p], vgsdf::CommandStoreLayout(n, b.sums.n_cmds), b.sums.n_cmds);
		out[b.p] = made[b.p].release();
	}
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

int vgsdf_fonts_create_charstrings2_within(vgsdf_ctx *ctx, const vgsdf_fonts_charstrings2_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                           int *status, uint64_t *needed)
{
	if (!ctx)
		return VGSDF_E_ARG;
	try {
		return create_charstrings2_batch(ctx, in, max_store_bytes, out, status, needed);
	} catch (const std::bad_alloc &) { // (the fonts made so far are freed on the way here; out[] holds none of them)
		ctx->err = "vgsdf_fonts_create_charstrings2: out of host memory";
		return VGSDF_E_OOM;
	}
}

int vgsdf_fonts_create_charstrings2(vgsdf_ctx *ctx, const vgsdf_fonts_charstrings2_desc *in, vgsdf_font **out, int *status)
{
	return vgsdf_fonts_create_charstrings2_within(ctx, in, ~0ull, out, status, nullptr);
}

void vgsdf_fonts_charstrings2_kernel_ms(const vgsdf_ctx *ctx, float ms[2]) { pass_ms_out(ctx ? ctx->charstring_batch_ms : nullptr, ms); }

void vgsdf_font_charstrings_kernel_ms(const vgsdf_ctx *ctx, float ms[2]) { pass_ms_out(ctx ? ctx->charstring_ms : nullptr, ms); }

} // extern "C"
