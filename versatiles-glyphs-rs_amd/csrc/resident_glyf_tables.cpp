// resident_glyf_tables.cpp — glyf-kind stores the device walks from a face's loca and glyf (glyf_table_kernels.h): one face
// (vgsdf_font_create_tables, _within) or all faces of a call in one count and one emit launch (vgsdf_fonts_create_tables, _within).
// The two share what a description must hold (resident_build.h), what the count pass's flags say and one face's running sums.
#include <algorithm>
#include <memory>
#include <new>

#include "glyf_table_kernels.h"
#include "glyf_table_limits.h"
#include "resident_build.h"

namespace {
// what the count pass refused a face for, behind the caller's "entry: " or "entry: face N: "; NULL: nothing
const char *glyf_count_refusal(const uint32_t *fl)
{
	if (fl[vgsdf::GLYF_FLAG_BUDGET])
		return "a glyph past VGSDF_GLYF_MAX_COMPONENTS";
	return fl[vgsdf::GLYF_FLAG_SLOTS] ? "a glyph of more than 2^26 command slots" : nullptr;
}

// One face's running sums from its counts (kGlyfTableCounts per glyph id): byte_at[n + 1] for the emit pass and, of the font,
// leaf_off, slots, its sizes and its largest leaf.  false: outside the bounds of the host's table (glyf_table_limits.h), which
// kGlyfStorePast says
constexpr const char *kGlyfStorePast = "more than 2^22 leaves, a store past 2^32 - 4 bytes, or command slots that sum past 2^32 - 1";
bool glyf_running_sums(const uint32_t *counts, uint32_t n, uint32_t *byte_at, vgsdf_font &f)
{
	f.leaf_off.assign((size_t)n + 1, 0);
	f.slots.assign(n, 0);
	uint64_t n_bytes = 0, n_leaves = 0, slot_sum = 0;
	for (uint32_t g = 0; g < n; g++) {
		const uint32_t *c = counts + (size_t)vgsdf::kGlyfTableCounts * g;
		byte_at[g] = (uint32_t)n_bytes, f.leaf_off[g] = (uint32_t)n_leaves;
		f.slots[g] = c[2];
		n_bytes += align_up(c[0], 4), n_leaves += c[1], slot_sum += c[2];
		if (n_bytes > vg::kResidentMaxBytes || n_leaves > vg::kResidentMaxLeaves || slot_sum > vg::kResidentMaxSlotSum)
			return false;
		f.max_cap = std::max(f.max_cap, c[3]); // (every simple entry a leaf names is some glyph id's own)
		f.max_len = std::max(f.max_len, c[0]);
	}
	byte_at[n] = (uint32_t)n_bytes, f.leaf_off[n] = (uint32_t)n_leaves;
	f.n_glyph_ids = n, f.n_leaves = (uint32_t)n_leaves, f.n_bytes = (uint32_t)n_bytes;
	return true;
}
} // namespace

extern "C" {

int vgsdf_font_create_tables(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *in, vgsdf_font **out)
{
	return vgsdf_font_create_tables_within(ctx, in, ~0ull, out, nullptr);
}

int vgsdf_font_create_tables_within(vgsdf_ctx *ctx, const vgsdf_font_tables_desc *in, uint64_t max_store_bytes, vgsdf_font **out,
                                    uint64_t *needed)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || !tables_given(*in)) {
		ctx->err = "vgsdf_font_create_tables: NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (needed)
		*needed = 0;
	ctx->glyf_tables_ms[0] = ctx->glyf_tables_ms[1] = 0.0f;
	const uint32_t n = in->num_glyphs;
	if (!tables_stateable(*in)) {
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
	if (const char *why = glyf_count_refusal(got.data() + (size_t)vgsdf::kGlyfTableCounts * n)) {
		ctx->err = std::string("vgsdf_font_create_tables: ") + why;
		return VGSDF_E_GLYF;
	}
	std::vector<uint32_t> byte_at((size_t)n + 1);
	if (!glyf_running_sums(got.data(), n, byte_at.data(), *f)) {
		ctx->err = std::string("vgsdf_font_create_tables: ") + kGlyfStorePast;
		return VGSDF_E_GLYF;
	}
	const vgsdf::GlyfStoreLayout at(n, f->n_leaves, f->n_bytes);
	if (needed)
		*needed = at.total;
	if (at.total > max_store_bytes)
		return VGSDF_OK; // (*out stays NULL: the caller's limit, nothing allocated)
	f->device = ctx->device;
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
		described[f] = tables_given(in) && tables_stateable(in);
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
			std::unique_ptr<vgsdf_font> font(new vgsdf_font());
			const char *why = glyf_count_refusal(fl);
			if (!why && !glyf_running_sums(got.data() + (size_t)vgsdf::kGlyfTableCounts * r.glyph_base, n, byte_at + r.glyph_base + f, *font))
				why = kGlyfStorePast;
			if (why) {
				ctx->err = face + why;
				status[f] = VGSDF_E_GLYF;
				continue;
			}
			const vgsdf::GlyfStoreLayout at(n, font->n_leaves, font->n_bytes);
			if (needed)
				needed[f] = at.total;
			if (at.total > room)
				continue; // (out[f] stays NULL: passed over, the faces behind it go on with the same room)
			room -= at.total;
			font->device = ctx->device;
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

} // extern "C"
