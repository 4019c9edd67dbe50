// resident_gvar.cpp — command stores of a placed `glyf` face the device builds from loca, glyf and gvar (gvar_kernels.h): at one
// position (vgsdf_font_create_gvar, _within) or at all positions of a call (vgsdf_fonts_create_gvar, _within: the deltas and the
// emit pass over (glyph id, position) pairs, gvar_batch_kernels.hip).  Up to the deltas pass both are one sequence of the steps
// below — description, arena, count pass, running sums, launch plan — each over its own kernels; behind it the single call
// finishes one store (resident_command_store.h) and the batched call one per position.
#include <algorithm>
#include <memory>
#include <new>

#include "gvar_advance_batch_kernels.h"
#include "gvar_advance_kernels.h"
#include "gvar_kernels.h"
#include "gvar_limits.h"
#include "resident_command_store.h"

namespace {
uint32_t be16_at(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
uint32_t be32_at(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// what both constructors validate of the tables and the gvar header before anything runs; fills the header's fields of `face`
bool gvar_face_described(vgsdf_ctx *ctx, const char *entry, const vgsdf_font_tables_desc &in, const uint8_t *g, uint64_t gvar_len, uint32_t n_axes,
                         vgsdf::GvarRef &face)
{
	if (!tables_stateable(in)) {
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

struct GvarEvents : PassEvents { // and one event more, where the deltas pass ends
	hipEvent_t deltas = nullptr;
	hipError_t create()
	{
		const hipError_t err = PassEvents::create();
		return err != hipSuccess ? err : hipEventCreate(&deltas);
	}
	~GvarEvents()
	{
		if (deltas)
			(void)hipEventDestroy(deltas);
	}
};

// The description on the device, for the duration of a call:
// loca | glyf | gvar | coords (n_axes per position) | counts (4 per glyph id) | flags (8 per position) | pt_at | position records
// (the batched call's, 16-aligned; the single call has none)
struct GvarArenaLayout {
	size_t loca = 0, glyf, gvar, coords, counts, flags, pt_at, records, total;
	constexpr GvarArenaLayout(size_t loca_bytes, size_t glyf_bytes, size_t gvar_len, size_t n_axes, size_t n, size_t n_pos, bool with_records)
	    : glyf(align_up(loca_bytes, 16)), gvar(align_up(glyf + glyf_bytes, 16)), coords(align_up(gvar + gvar_len, 16)),
	      counts(align_up(coords + 2 * n_axes * n_pos, 16)), flags(counts + 4 * vgsdf::kGvarCounts * n),
	      pt_at(flags + 4 * vgsdf::GVAR_FLAG_WORDS * n_pos), records(with_records ? align_up(pt_at + 4 * (n + 1), 16) : pt_at + 4 * (n + 1)),
	      total(records + (with_records ? sizeof(vgsdf::GvarPositionRef) * n_pos : 0))
	{
	}
};
static_assert(GvarArenaLayout(10, 20, 30, 2, 3, 1, false).gvar == 48 && GvarArenaLayout(10, 20, 30, 2, 3, 1, false).coords == 80 &&
                  GvarArenaLayout(10, 20, 30, 2, 3, 1, false).counts == 96 && GvarArenaLayout(10, 20, 30, 2, 3, 1, false).flags == 144 &&
                  GvarArenaLayout(10, 20, 30, 2, 3, 1, false).pt_at == 176 && GvarArenaLayout(10, 20, 30, 2, 3, 1, false).total == 192,
              "one position: loca | glyf | gvar | coords | counts | flags | pt_at, as the single call has always laid them out");
static_assert(GvarArenaLayout(10, 20, 30, 2, 3, 5, true).counts == 112 && GvarArenaLayout(10, 20, 30, 2, 3, 5, true).pt_at == 160 + 160 &&
                  GvarArenaLayout(10, 20, 30, 2, 3, 5, true).records == 336 &&
                  GvarArenaLayout(10, 20, 30, 2, 3, 5, true).total == 336 + 5 * sizeof(vgsdf::GvarPositionRef),
              "coordinates and flag words per position, the records 16-aligned behind pt_at");

// uploads the tables and the positions' coordinates, zeroes the flag words and names it all in `face`
void upload_gvar_face(Calls &q, uint8_t *a, const GvarArenaLayout &at, const vgsdf_font_tables_desc &in, const uint8_t *gvar, uint32_t gvar_len,
                      uint32_t n_axes, const int16_t *coords, uint32_t n_pos, vgsdf::GvarRef &face)
{
	q.copy(a, in.loca, in.n_loca_bytes);
	q.copy(a + at.glyf, in.glyf, in.n_glyf_bytes);
	q.copy(a + at.gvar, gvar, gvar_len);
	q.copy(a + at.coords, coords, 2 * (size_t)n_axes * n_pos);
	q.zero(a + at.flags, at.pt_at - at.flags);
	face.loca = a, face.glyf = a + at.glyf, face.gvar = a + at.gvar;
	face.coords = (const int16_t *)(a + at.coords); // (the first position's: the batched kernels take each lane's own)
	face.glyf_len = in.n_glyf_bytes, face.loca_entries = in.loca_entries, face.loca_long = in.loca_long, face.n_glyph_ids = in.num_glyphs;
	face.gvar_len = gvar_len, face.n_axes = n_axes;
}

// The count pass.  It looks at no coordinate: one launch whatever the positions, and its two flag words land among those of the
// first.  Launch, the counts and, behind them, those flag words in one read-back into `got`, synchronisation.  -> what the pass
// refuses the face for, behind the caller's name; NULL: nothing (or q has failed)
const char *gvar_count_pass(Calls &q, const PassEvents &ev, const vgsdf::GvarRef &face, uint32_t *d_counts, uint32_t *d_flags,
                            std::vector<uint32_t> &got)
{
	const uint32_t n = face.n_glyph_ids;
	q.record(ev.at[0]);
	if (n)
		q.launch([&] { return vgsdf_gvar_count(&face, d_counts, d_flags, q.st); });
	q.record(ev.at[1]);
	got.assign((size_t)vgsdf::kGvarCounts * n + vgsdf::GVAR_FLAG_WORDS, 0);
	q.read_back(got.data(), d_counts, 4 * got.size());
	q.sync();
	if (q.failed())
		return nullptr;
	const uint32_t *fl = got.data() + (size_t)vgsdf::kGvarCounts * n;
	if (fl[vgsdf::GVAR_FLAG_RECORDS])
		return "a glyph past VGSDF_GLYF_MAX_COMPONENTS, or a composite of more than 65535 component records";
	return fl[vgsdf::GVAR_FLAG_CMDS] ? "a glyph of more than 2^26 commands" : nullptr;
}

// what the deltas pass refuses a position for, from its flag words; NULL: nothing
const char *gvar_deltas_refusal(const uint32_t *fl)
{
	if (fl[vgsdf::GVAR_FLAG_MALFORMED])
		return "a glyph with malformed variation data";
	return fl[vgsdf::GVAR_FLAG_DELTAS] ? "a glyph past VGSDF_GVAR_MAX_DELTAS" : nullptr;
}

// the running sums over the counts, the same at every position: the points of the deltas pass and the store's layout
struct GvarSums {
	std::vector<uint32_t> pt_at; // [n + 1]  (65535 glyph ids of at most 65539 points: below 2^32)
	CommandSums store;
	// false: a store past what 32-bit offsets address (kCommandStorePast)
	bool fill(const uint32_t *counts, uint32_t n)
	{
		pt_at.assign((size_t)n + 1, 0);
		for (uint32_t g = 0; g < n; g++)
			pt_at[g + 1] = pt_at[g] + counts[(size_t)vgsdf::kGvarCounts * g];
		return store.fill(counts, n, vgsdf::kGvarCounts, 1, 2);
	}
};

// the deltas pass's scratch for the e points (x positions) of one launch: sx | sy | x | y | mark, each 16-aligned
struct GvarScratchLayout {
	size_t sx = 0, sy, x, y, mark, total;
	constexpr explicit GvarScratchLayout(size_t e)
	    : sy(align_up(4 * e, 16)), x(2 * sy), y(x + align_up(2 * e, 16)), mark(y + align_up(2 * e, 16)), total(mark + e)
	{
	}
	vgsdf::GvarScratch in(void *scratch) const
	{
		uint8_t *s = (uint8_t *)scratch;
		return vgsdf::GvarScratch{(float *)s, (float *)(s + sy), (int16_t *)(s + x), (int16_t *)(s + y), s + mark};
	}
};
static_assert(GvarScratchLayout(5).sy == 32 && GvarScratchLayout(5).x == 64 && GvarScratchLayout(5).y == 80 && GvarScratchLayout(5).mark == 96 &&
                  GvarScratchLayout(5).total == 101 && GvarScratchLayout(8).y == 64 + 16 && GvarScratchLayout(8).total == 96 + 8,
              "sx | sy | x | y | mark");

// The launches of the deltas pass: glyph ids x positions whose points x positions stay within kGvarSlicePoints; a glyph id that
// passes it with all positions goes alone, in runs of positions (at least one).  With one position these are the slices of glyph
// ids of the single call.  *most: the points x positions of the largest launch (0: none), which sizes the context's scratch once
// for all of them — nothing in flight reads it: every call that uses it ends with a synchronisation
struct GvarLaunch {
	uint32_t g0, g1, p0, p1;
};
std::vector<GvarLaunch> plan_gvar_deltas(const std::vector<uint32_t> &pt_at, uint32_t n_pos, size_t *most)
{
	const uint32_t n = (uint32_t)pt_at.size() - 1;
	std::vector<GvarLaunch> launches;
	*most = 0;
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
			launches.push_back(GvarLaunch{g0, g1, p0, p1});
			*most = std::max(*most, slice * (p1 - p0));
		}
		g0 = g1;
	}
	return launches;
}

// vgsdf_font_create_gvar_within: count pass, read-back and layout, deltas pass in slices over the context's scratch, emit pass,
// context pass (gvar_kernels.h)
int create_gvar(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *desc, uint64_t max_store_bytes, vgsdf_font **out, uint64_t *store_bytes)
{
	const char *name = "vgsdf_font_create_gvar";
	if (!desc || !out || !tables_given(desc->tables) || !desc->gvar || !desc->coords) {
		ctx->err = "vgsdf_font_create_gvar: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (store_bytes)
		*store_bytes = 0;
	ctx->gvar_ms[0] = ctx->gvar_ms[1] = ctx->gvar_ms[2] = 0.0f;
	const vgsdf_font_tables_desc &in = desc->tables;
	const uint32_t n = in.num_glyphs;
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
	GvarEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	const GvarArenaLayout arena(in.n_loca_bytes, in.n_glyf_bytes, desc->gvar_len, desc->n_axes, n, 1, false);
	ScratchBuf dev, acc, tmp;
	if (hipError_t e = dev.ensure(arena.total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	Calls q(st);
	upload_gvar_face(q, a, arena, in, desc->gvar, desc->gvar_len, desc->n_axes, desc->coords, 1, face);
	uint32_t *d_counts = (uint32_t *)(a + arena.counts), *d_flags = (uint32_t *)(a + arena.flags), *d_at = (uint32_t *)(a + arena.pt_at);
	std::vector<uint32_t> got;
	const char *why = gvar_count_pass(q, ev, face, d_counts, d_flags, got);
	if (q.failed())
		return font_hip_error(ctx, name, "count pass", q.e);
	ev.elapsed(ctx->gvar_ms, 0);
	GvarSums sums;
	if (why || !sums.fill(got.data(), n)) {
		ctx->err = std::string(name) + ": " + (why ? why : kCommandStorePast);
		return VGSDF_E_GLYF;
	}
	const uint32_t n_cmds = sums.store.n_cmds, n_floats = sums.store.n_floats;
	const vgsdf::CommandStoreLayout at(n, n_cmds);
	if (store_bytes)
		*store_bytes = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	// the deltas pass, in slices of glyph ids over the context's scratch
	size_t most = 0;
	const std::vector<GvarLaunch> launches = plan_gvar_deltas(sums.pt_at, 1, &most);
	if (hipError_t err = acc.ensure(8 * (size_t)sums.pt_at[n] + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	float *d_acc = (float *)acc.p;
	if (most)
		if (hipError_t err = ctx->gvar_scratch.ensure(GvarScratchLayout(most).total + 16); err != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", err);
	q.copy(d_at, sums.pt_at.data(), 4 * ((size_t)n + 1));
	q.record(ev.at[1]);
	for (const GvarLaunch &l : launches) {
		const vgsdf::GvarScratch scratch = GvarScratchLayout(sums.pt_at[l.g1] - sums.pt_at[l.g0]).in(ctx->gvar_scratch.p);
		q.launch([&] { return vgsdf_gvar_deltas(&face, l.g0, l.g1, d_counts, d_at, d_acc, &scratch, d_flags, st); });
	}
	q.record(ev.deltas);
	uint32_t flags[vgsdf::GVAR_FLAG_WORDS] = {};
	q.read_back(flags, d_flags, sizeof flags);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "deltas pass", q.e);
	(void)hipEventElapsedTime(&ctx->gvar_ms[1], ev.at[1], ev.deltas);
	if (const char *refused = gvar_deltas_refusal(flags)) {
		ctx->err = std::string(name) + ": " + refused;
		return VGSDF_E_GLYF;
	}
	f->device = ctx->device;
	f->n_glyph_ids = n;
	f->commands = true;
	f->slots.swap(sums.store.slots);
	const ContextStagingLayout tat(n, n_cmds, n_floats);
	if (hipError_t err = f->store.ensure(at.total + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	if (hipError_t err = tmp.ensure(tat.total); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	uint8_t *d = (uint8_t *)f->store.p, *t = (uint8_t *)tmp.p;
	uint32_t emit_flag = 0;
	// (the emit pass reads cmd_off from the store, where it stays, and dat_off from the staging, as the context pass behind it does)
	const uint32_t flag = finish_command_store(q, *f, at, t, tat, n_cmds, sums.store.cmd_off.data(), sums.store.dat_off.data(), [&] {
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

// vgsdf_fonts_create_gvar_within: create_gvar for one face at all its positions.  The tables go up once; the count pass, its
// read-back and the layout serve every position; the deltas pass and the emit pass run over (glyph id, position) pairs
// (gvar_batch_kernels.hip), the context pass once per store; two more read-backs (the positions' flag words behind the deltas pass
// and behind the emit pass) and three synchronisations for the whole call
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
	if (!out || !status || !tables_given(desc->tables) || !desc->gvar || !desc->coords) {
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
	vgsdf::GvarRef face{};
	if (!gvar_face_described(ctx, name, in, desc->gvar, desc->gvar_len, n_axes, face))
		return VGSDF_E_ARG;
	auto refuse_all = [&](const char *why) { // a refusal that no position can change
		ctx->err = std::string(name) + ": " + why;
		for (uint32_t p = 0; p < n_pos; p++)
			status[p] = VGSDF_E_GLYF;
		return VGSDF_OK;
	};
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	GvarEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	const GvarArenaLayout arena(in.n_loca_bytes, in.n_glyf_bytes, desc->gvar_len, n_axes, n, n_pos, true);
	ScratchBuf dev, acc, tmp;
	if (hipError_t e = dev.ensure(arena.total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	Calls q(st);
	upload_gvar_face(q, a, arena, in, desc->gvar, desc->gvar_len, n_axes, desc->coords, n_pos, face);
	const int16_t *d_coords = (const int16_t *)(a + arena.coords);
	uint32_t *d_counts = (uint32_t *)(a + arena.counts), *d_flags = (uint32_t *)(a + arena.flags), *d_at = (uint32_t *)(a + arena.pt_at);
	vgsdf::GvarPositionRef *d_rec = (vgsdf::GvarPositionRef *)(a + arena.records);
	std::vector<uint32_t> got;
	const char *why = gvar_count_pass(q, ev, face, d_counts, d_flags, got);
	if (q.failed())
		return font_hip_error(ctx, name, "count pass", q.e);
	ev.elapsed(ctx->gvar_batch_ms, 0);
	GvarSums sums;
	if (why || !sums.fill(got.data(), n))
		return refuse_all(why ? why : kCommandStorePast);
	const std::vector<uint32_t> &pt_at = sums.pt_at;
	const uint32_t n_cmds = sums.store.n_cmds, n_floats = sums.store.n_floats;
	const vgsdf::CommandStoreLayout at(n, n_cmds);
	if (needed)
		for (uint32_t p = 0; p < n_pos; p++)
			needed[p] = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (not one store fits: nothing allocated, no position looked at, as the single call)
	// the deltas pass over (glyph id, position) pairs
	size_t most = 0;
	const std::vector<GvarLaunch> launches = plan_gvar_deltas(pt_at, n_pos, &most);
	const size_t acc_stride = 2 * (size_t)pt_at[n]; // floats of one position's sums
	if (hipError_t err = acc.ensure(4 * acc_stride * n_pos + 16); err != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", err);
	float *d_acc = (float *)acc.p;
	if (most)
		if (hipError_t err = ctx->gvar_scratch.ensure(GvarScratchLayout(most).total + 16); err != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", err);
	q.copy(d_at, pt_at.data(), 4 * ((size_t)n + 1));
	q.record(ev.at[1]);
	for (const GvarLaunch &l : launches) {
		const uint32_t slice = pt_at[l.g1] - pt_at[l.g0];
		const vgsdf::GvarScratch scratch = GvarScratchLayout((size_t)slice * (l.p1 - l.p0)).in(ctx->gvar_scratch.p);
		q.launch([&] {
			return vgsdf_gvar_batch_deltas(&face, l.g0, l.g1, l.p0, l.p1, d_coords, d_counts, d_at, d_acc, acc_stride, &scratch, slice, d_flags, st);
		});
	}
	q.record(ev.deltas);
	std::vector<uint32_t> flags((size_t)vgsdf::GVAR_FLAG_WORDS * n_pos, 0);
	q.read_back(flags.data(), d_flags, 4 * flags.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "deltas pass", q.e);
	(void)hipEventElapsedTime(&ctx->gvar_batch_ms[1], ev.at[1], ev.deltas);
	// per position: refused, passed over, or a font with its store
	std::vector<std::unique_ptr<vgsdf_font>> made(n_pos); // freed on every way out but the last
	std::vector<uint32_t> built;
	uint64_t room = max_store_bytes;
	for (uint32_t p = 0; p < n_pos; p++) {
		if (const char *refused = gvar_deltas_refusal(flags.data() + (size_t)vgsdf::GVAR_FLAG_WORDS * p)) {
			ctx->err = std::string(name) + ": position " + std::to_string(p) + ": " + refused;
			status[p] = VGSDF_E_GLYF;
			if (needed)
				needed[p] = 0;
			continue;
		}
		if (at.total > room)
			continue; // (out[p] stays NULL: passed over, the positions behind it go on with the same room)
		room -= at.total;
		std::unique_ptr<vgsdf_font> font(new vgsdf_font());
		font->slots = sums.store.slots;
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
	q.copy(t + t_dat, sums.store.dat_off.data(), 4 * ((size_t)n + 1));
	q.zero(t + t_flags, 4 * (size_t)n_built);
	std::vector<vgsdf::GvarPositionRef> rec(n_built);
	for (uint32_t k = 0; k < n_built; k++) {
		const uint32_t p = built[k];
		uint8_t *d = (uint8_t *)made[p]->store.p, *tp = t + t_first + t_each * k;
		q.copy(d + at.cmd_off, sums.store.cmd_off.data(), 4 * ((size_t)n + 1));
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

// the phantom pass's output on the device: delta (f32 per glyph id) | state (a byte per glyph id) | flags, each 16-aligned
struct GvarAdvanceLayout {
	size_t delta = 0, state, flags, total;
	constexpr explicit GvarAdvanceLayout(size_t n) : state(align_up(4 * n, 16)), flags(align_up(state + n, 16)), total(flags + 4 * vgsdf::GVAR_ADVANCE_FLAG_WORDS) {}
};
static_assert(GvarAdvanceLayout(5).state == 32 && GvarAdvanceLayout(5).flags == 48 && GvarAdvanceLayout(5).total == 64, "delta | state | flags");
} // namespace

// The phantom pass over one face (gvar_advance_kernels.h).  _described: the description validated as create_gvar validates it
// (VGSDF_E_ARG).  _bytes / _state_at: what the pass writes for n glyph ids, delta at 0 | state (GvarAdvanceLayout).  _on_device,
// over a description that passed _described: the tables uploaded into an arena of the call's own, the pass into `out` (device
// memory of _bytes(num_glyphs)), its flag word read back, synchronisation; *ms: the pass's milliseconds.
int gvar_advance_described(vgsdf_ctx *ctx, const char *name, const vgsdf_font_gvar_desc *desc)
{
	if (!desc || !tables_given(desc->tables) || !desc->gvar || !desc->coords) {
		ctx->err = std::string(name) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	vgsdf::GvarRef face{};
	return gvar_face_described(ctx, name, desc->tables, desc->gvar, desc->gvar_len, desc->n_axes, face) ? VGSDF_OK : VGSDF_E_ARG;
}
size_t gvar_advance_bytes(uint32_t n) { return GvarAdvanceLayout(n).total; }
size_t gvar_advance_state_at(uint32_t n) { return GvarAdvanceLayout(n).state; }

int gvar_advance_on_device(vgsdf_ctx *ctx, const char *name, const vgsdf_font_gvar_desc *desc, uint8_t *o, float *ms)
{
	*ms = 0.0f;
	const vgsdf_font_tables_desc &in = desc->tables;
	const uint32_t n = in.num_glyphs;
	vgsdf::GvarRef face{};
	if (!gvar_face_described(ctx, name, in, desc->gvar, desc->gvar_len, desc->n_axes, face))
		return VGSDF_E_ARG;
	(void)hipSetDevice(ctx->device);
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	const GvarArenaLayout arena(in.n_loca_bytes, in.n_glyf_bytes, desc->gvar_len, desc->n_axes, 0, 1, false);
	const GvarAdvanceLayout at(n);
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(arena.total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	Calls q(ctx->stream);
	upload_gvar_face(q, a, arena, in, desc->gvar, desc->gvar_len, desc->n_axes, desc->coords, 1, face);
	q.zero(o + at.flags, 4 * vgsdf::GVAR_ADVANCE_FLAG_WORDS);
	q.record(ev.at[0]);
	if (n)
		q.launch([&] { return vgsdf_gvar_advance_pass(&face, (float *)(o + at.delta), o + at.state, (uint32_t *)(o + at.flags), q.st); });
	q.record(ev.at[1]);
	uint32_t flags[vgsdf::GVAR_ADVANCE_FLAG_WORDS] = {};
	q.read_back(flags, o + at.flags, sizeof flags);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "phantom pass", q.e);
	(void)hipEventElapsedTime(ms, ev.at[0], ev.at[1]);
	if (flags[vgsdf::GVAR_ADVANCE_FLAG_DELTAS]) {
		ctx->err = std::string(name) + ": a glyph past VGSDF_GVAR_MAX_DELTAS";
		return VGSDF_E_GLYF;
	}
	return VGSDF_OK;
}

// The phantom pass over one face at MANY positions (gvar_advance_batch_kernels.h), for vgsdf_gvar_advance_deltas_batch and
// vgsdf_families_create_tables.  _described: n_positions 1 .. VGSDF_FAMILY_MAX_POSITIONS and the description validated as
// create_gvar_batch validates it (VGSDF_E_ARG).  _bytes / _state_at: what the pass writes for n glyph ids at n_pos positions,
// delta [n_pos x n] f32 at 0 | state [n_pos x n] bytes | flags, each 16-aligned, position-major.  _on_device, over a description
// that passed _described: the tables and all coordinates uploaded once into an arena of the call's own, ONE launch over all
// pairs into `o`, its flag word read back, synchronisation; *ms: the pass's milliseconds.
namespace {
struct GvarAdvanceBatchLayout {
	size_t delta = 0, state, flags, total;
	constexpr GvarAdvanceBatchLayout(size_t n, size_t n_pos)
	    : state(align_up(4 * n * n_pos, 16)), flags(align_up(state + n * n_pos, 16)), total(flags + 4 * vgsdf::GVAR_ADVANCE_FLAG_WORDS)
	{
	}
};
static_assert(GvarAdvanceBatchLayout(5, 1).state == GvarAdvanceLayout(5).state && GvarAdvanceBatchLayout(5, 1).total == GvarAdvanceLayout(5).total &&
                  GvarAdvanceBatchLayout(5, 3).state == 64 && GvarAdvanceBatchLayout(5, 3).flags == 80,
              "delta | state | flags over glyph ids x positions; one position: the single pass's layout");
} // namespace
int gvar_advance_batch_described(vgsdf_ctx *ctx, const char *name, const vgsdf_fonts_gvar_desc *desc)
{
	if (!desc || !tables_given(desc->tables) || !desc->gvar || !desc->coords) {
		ctx->err = std::string(name) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	if (desc->n_positions == 0 || desc->n_positions > VGSDF_FAMILY_MAX_POSITIONS) {
		ctx->err = std::string(name) + ": a gvar description of no position or of more than 64";
		return VGSDF_E_ARG;
	}
	vgsdf::GvarRef face{};
	return gvar_face_described(ctx, name, desc->tables, desc->gvar, desc->gvar_len, desc->n_axes, face) ? VGSDF_OK : VGSDF_E_ARG;
}
size_t gvar_advance_batch_bytes(uint32_t n, uint32_t n_pos) { return GvarAdvanceBatchLayout(n, n_pos).total; }
size_t gvar_advance_batch_state_at(uint32_t n, uint32_t n_pos) { return GvarAdvanceBatchLayout(n, n_pos).state; }

int gvar_advance_batch_on_device(vgsdf_ctx *ctx, const char *name, const vgsdf_fonts_gvar_desc *desc, uint8_t *o, float *ms)
{
	*ms = 0.0f;
	const vgsdf_font_tables_desc &in = desc->tables;
	const uint32_t n = in.num_glyphs, n_pos = desc->n_positions;
	vgsdf::GvarRef face{};
	if (!gvar_face_described(ctx, name, in, desc->gvar, desc->gvar_len, desc->n_axes, face))
		return VGSDF_E_ARG;
	(void)hipSetDevice(ctx->device);
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, name, "hipEventCreate", err);
	const GvarArenaLayout arena(in.n_loca_bytes, in.n_glyf_bytes, desc->gvar_len, desc->n_axes, 0, n_pos, false);
	const GvarAdvanceBatchLayout at(n, n_pos);
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(arena.total + 16); e != hipSuccess)
		return font_hip_error(ctx, name, "hipMalloc", e);
	uint8_t *a = (uint8_t *)dev.p;
	Calls q(ctx->stream);
	upload_gvar_face(q, a, arena, in, desc->gvar, desc->gvar_len, desc->n_axes, desc->coords, n_pos, face);
	q.zero(o + at.flags, 4 * vgsdf::GVAR_ADVANCE_FLAG_WORDS);
	q.record(ev.at[0]);
	if (n)
		q.launch([&] {
			return vgsdf_gvar_advance_batch_pass(&face, (const int16_t *)(a + arena.coords), n_pos, (float *)(o + at.delta), o + at.state,
			                                     (uint32_t *)(o + at.flags), q.st);
		});
	q.record(ev.at[1]);
	uint32_t flags[vgsdf::GVAR_ADVANCE_FLAG_WORDS] = {};
	q.read_back(flags, o + at.flags, sizeof flags);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, name, "phantom pass", q.e);
	(void)hipEventElapsedTime(ms, ev.at[0], ev.at[1]);
	if (flags[vgsdf::GVAR_ADVANCE_FLAG_DELTAS]) {
		ctx->err = std::string(name) + ": a glyph past VGSDF_GVAR_MAX_DELTAS";
		return VGSDF_E_GLYF;
	}
	return VGSDF_OK;
}

namespace {
// what both `…_kernel_ms` getters answer: the context's count / deltas / emit triple of the last call, zeros without a context
void gvar_ms_out(const float *triple, float ms[3])
{
	if (ms)
		for (int i = 0; i < 3; i++)
			ms[i] = triple ? triple[i] : 0.0f;
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

void vgsdf_font_gvar_kernel_ms(const vgsdf_ctx *ctx, float ms[3]) { gvar_ms_out(ctx ? ctx->gvar_ms : nullptr, ms); }

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

void vgsdf_fonts_gvar_kernel_ms(const vgsdf_ctx *ctx, float ms[3]) { gvar_ms_out(ctx ? ctx->gvar_batch_ms : nullptr, ms); }

int vgsdf_gvar_advance_deltas(vgsdf_ctx *ctx, const vgsdf_font_gvar_desc *in, float *delta, uint8_t *state)
{
	if (!ctx)
		return VGSDF_E_ARG;
	const char *name = "vgsdf_gvar_advance_deltas";
	ctx->gvar_advance_ms = 0.0f;
	if (!delta || !state) {
		ctx->err = std::string(name) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	try {
		if (const int rc = gvar_advance_described(ctx, name, in); rc != VGSDF_OK)
			return rc;
		const uint32_t n = in->tables.num_glyphs;
		ScratchBuf out;
		if (hipError_t e = out.ensure(gvar_advance_bytes(n) + 16); e != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", e);
		if (const int rc = gvar_advance_on_device(ctx, name, in, (uint8_t *)out.p, &ctx->gvar_advance_ms); rc != VGSDF_OK)
			return rc;
		if (n) {
			HIP_TRY(ctx, hipMemcpy(delta, out.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
			HIP_TRY(ctx, hipMemcpy(state, (const uint8_t *)out.p + gvar_advance_state_at(n), n, hipMemcpyDeviceToHost));
		}
		return VGSDF_OK;
	} catch (const std::bad_alloc &) {
		ctx->err = std::string(name) + ": out of host memory";
		return VGSDF_E_OOM;
	}
}

float vgsdf_gvar_advance_kernel_ms(const vgsdf_ctx *ctx) { return ctx ? ctx->gvar_advance_ms : 0.0f; }

int vgsdf_gvar_advance_deltas_batch(vgsdf_ctx *ctx, const vgsdf_fonts_gvar_desc *in, float *delta, uint8_t *state)
{
	if (!ctx)
		return VGSDF_E_ARG;
	const char *name = "vgsdf_gvar_advance_deltas_batch";
	if (!in) {
		ctx->err = std::string(name) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	if (in->n_positions == 0)
		return VGSDF_OK;
	ctx->families_tables_ms[0] = ctx->families_tables_ms[1] = ctx->families_tables_ms[2] = 0.0f;
	if (!delta || !state) {
		ctx->err = std::string(name) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	try {
		if (const int rc = gvar_advance_batch_described(ctx, name, in); rc != VGSDF_OK)
			return rc;
		const size_t pairs = (size_t)in->tables.num_glyphs * in->n_positions;
		ScratchBuf out;
		if (hipError_t e = out.ensure(gvar_advance_batch_bytes(in->tables.num_glyphs, in->n_positions) + 16); e != hipSuccess)
			return font_hip_error(ctx, name, "hipMalloc", e);
		if (const int rc = gvar_advance_batch_on_device(ctx, name, in, (uint8_t *)out.p, &ctx->families_tables_ms[0]); rc != VGSDF_OK)
			return rc;
		if (pairs) {
			HIP_TRY(ctx, hipMemcpy(delta, out.p, 4 * pairs, hipMemcpyDeviceToHost));
			HIP_TRY(ctx, hipMemcpy(state, (const uint8_t *)out.p + gvar_advance_batch_state_at(in->tables.num_glyphs, in->n_positions), pairs,
			                       hipMemcpyDeviceToHost));
		}
		return VGSDF_OK;
	} catch (const std::bad_alloc &) {
		ctx->err = std::string(name) + ": out of host memory";
		return VGSDF_E_OOM;
	}
}

} // extern "C"
