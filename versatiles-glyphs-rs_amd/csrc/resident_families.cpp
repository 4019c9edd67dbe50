// resident_families.cpp — the families over resident fonts (resident_fonts.cpp): a font id's table
// code point -> (font, glyph id, advance, scale, shift_x) on host and device (upload_layout.h, FamilyTableLayout), stated by the
// host (vgsdf_family_create) or built by the device from the faces' cmap and hmtx (vgsdf_family_create_tables; for one face at
// many positions, a family each, by one call: vgsdf_families_create_tables), for submissions
// that name code-point ranges (vgsdf_outlines_submit_ranges).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "family_census_kernels.h"
#include "family_table_kernels.h"
#include "resident_build.h"

namespace {
// font k of a family: there, on the context's device and of the kind of font 0 (a mixed family: of either kind)
bool family_font_fits(const vgsdf_ctx *ctx, const vgsdf_font *const *fonts, uint32_t k, bool mixed)
{
	return fonts[k] && fonts[k]->device == ctx->device && (mixed || (fonts[0] && fonts[k]->commands == fonts[0]->commands));
}
// what a family keeps of its (checked) fonts
void adopt_fonts(vgsdf_family &f, const vgsdf_ctx *ctx, const vgsdf_font *const *fonts, uint32_t n_fonts, bool mixed)
{
	f.device = ctx->device;
	f.mixed = mixed;
	f.commands = !mixed && fonts[0]->commands;
	f.fonts.assign(fonts, fonts + n_fonts);
	for (const vgsdf_font *ft : f.fonts)
		if (!ft->commands) { // (what the decoder's LDS is sized from: the leaves of glyf fonts)
			f.max_cap = std::max(f.max_cap, ft->max_cap);
			f.max_len = std::max(f.max_len, ft->max_len);
		}
}
const char *const kFontsRefused[2] = {"a NULL font, a font of another device than the context's, or fonts of both kinds",
                                      "a NULL font, or a font of another device than the context's"};

// vgsdf_family_create, vgsdf_family_create_mixed and, with a plane, vgsdf_family_create_at: `me` names the call in its messages
int family_create(vgsdf_ctx *ctx, const vgsdf_family_desc *in, vgsdf_family **out, bool mixed, const char *me, uint32_t plane = 0)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || !in->fonts ||
	    (in->n_entries && (!in->code_point || !in->font_of || !in->glyph_id || !in->advance || !in->scale || !in->shift_x))) {
		ctx->err = std::string(me) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (plane > 16) {
		ctx->err = std::string(me) + ": plane must be 0 .. 16";
		return VGSDF_E_ARG;
	}
	const uint32_t n = in->n_entries;
	if (in->n_fonts == 0 || in->n_fonts > 0x10000u || n > 0x10000u) {
		ctx->err = std::string(me) + ": n_fonts must be 1 .. 65536 and n_entries at most 65536";
		return VGSDF_E_ARG;
	}
	for (uint32_t k = 0; k < in->n_fonts; k++)
		if (!family_font_fits(ctx, in->fonts, k, mixed)) {
			ctx->err = std::string(me) + ": " + kFontsRefused[mixed];
			return VGSDF_E_ARG;
		}
	for (uint32_t i = 0; i < n; i++)
		if ((i && in->code_point[i] <= in->code_point[i - 1]) || in->font_of[i] >= in->n_fonts ||
		    in->glyph_id[i] >= in->fonts[in->font_of[i]]->n_glyph_ids) {
			ctx->err = std::string(me) + ": code points not strictly ascending, font_of past n_fonts, or a glyph id past its face";
			return VGSDF_E_ARG;
		}
	std::unique_ptr<vgsdf_family> f(new (std::nothrow) vgsdf_family());
	if (!f) {
		ctx->err = std::string(me) + ": out of host memory";
		return VGSDF_E_OOM;
	}
	adopt_fonts(*f, ctx, in->fonts, in->n_fonts, mixed);
	f->plane = plane;
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
		f->pbf_fix[i] = (uint8_t)((1u + varint_len((plane << 16) | f->code_point[i])) | ((1u + varint_len(f->advance[i])) << 4));
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
		return font_hip_error(ctx, me, "hipMalloc", e);
	Calls q(ctx->stream);
	q.copy(f->table.p, h.data(), h.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, me, "upload", q.e);
	*out = f.release();
	return VGSDF_OK;
}

// what can be said of a face's variation record without walking a glyph's row (vgsdf.h); nullptr: nothing against it
const char *variation_refused(const vgsdf_face_variation &v)
{
	if ((v.hvar_len && !v.hvar) || (v.n_regions && !v.region_scalars))
		return "a NULL HVAR table or factor array of a length that is not 0";
	if (!v.hvar)
		return v.hvar_len || v.n_regions ? "factors or a length without an HVAR table" : nullptr;
	if ((uint64_t)v.store_off + 8 > v.hvar_len || v.map_off >= v.hvar_len)
		return "an HVAR store or advance-map offset outside the table";
	const uint8_t *st = v.hvar + v.store_off;
	const uint64_t room = v.hvar_len - v.store_off;
	auto be16 = [](const uint8_t *p) { return (uint32_t)((p[0] << 8) | p[1]); };
	auto be32 = [](const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3]; };
	if (be16(st) != 1)
		return "an HVAR store of a format other than 1";
	for (uint64_t d = 0, n = be16(st + 6); d < n && 8 + 4 * d + 4 <= room; d++) {
		const uint64_t at = be32(st + 8 + 4 * d);
		if (at <= room && 6 <= room - at && (be16(st + at + 2) & 0x8000u))
			return "an HVAR ItemVariationData with 32-bit deltas (LONG_WORDS)";
	}
	for (uint32_t r = 0; r < v.n_regions; r++)
		if (!std::isfinite(v.region_scalars[r]))
			return "a region factor that is not finite";
	return nullptr;
}

// the host's copy of a table the device built, from its one read-back (FamilyTableLayout(n)); the 64-bit running sums from the
// table's differences (exact: a glyph holds fewer than 2^31 slots and fewer than 2^32 leaves)
void adopt_table(vgsdf_family &f, const uint8_t *back, uint32_t n)
{
	const vgsdf::FamilyTableLayout at(n);
	auto slice = [&](auto &v, size_t off, size_t count) {
		v.resize(count);
		if (count)
			std::memcpy(v.data(), back + off, sizeof(v[0]) * count);
	};
	slice(f.scale, at.scale, n), slice(f.shift_x, at.shift_x, n), slice(f.advance, at.advance, n), slice(f.code_point, at.code_point, n);
	slice(f.font_of, at.font_of, n), slice(f.glyph_id, at.glyph_id, n), slice(f.pbf_fix, at.pbf_fix, n);
	f.cmd_pre.assign((size_t)n + 1, 0);
	f.leaf_pre.assign((size_t)n + 1, 0);
	const uint32_t *cp32 = (const uint32_t *)(back + at.cmd_pre), *lp32 = (const uint32_t *)(back + at.leaf_pre);
	for (uint32_t i = 0; i < n; i++) {
		f.cmd_pre[i + 1] = f.cmd_pre[i] + (uint32_t)(cp32[i + 1] - cp32[i]);
		f.leaf_pre[i + 1] = f.leaf_pre[i] + (uint32_t)(lp32[i + 1] - lp32[i]);
	}
}

// what vgsdf_family_create_tables validates of one face's tables; nullptr: nothing against them
const char *face_tables_refused(const vgsdf_face_tables &t)
{
	if ((t.cmap_len && !t.cmap) || (t.hmtx_len && !t.hmtx) || (t.n_subtables && (!t.subtable_off || !t.subtable_format)))
		return "a NULL table or subtable array of a length that is not 0";
	if (t.units_per_em < 16 || t.units_per_em > 16384)
		return "units_per_em not 16 .. 16384";
	for (uint32_t s = 0; s < t.n_subtables; s++) {
		const uint16_t fm = t.subtable_format[s];
		if (t.subtable_off[s] >= t.cmap_len || !(fm == 0 || fm == 4 || fm == 6 || fm == 10 || fm == 12 || fm == 13))
			return "a subtable offset at or past cmap_len, or a format that is not 0, 4, 6, 10, 12 or 13";
	}
	return nullptr;
}

// vgsdf_family_create_tables and vgsdf_family_create_tables_mixed (the kernels take the kind face by face: FamilyFaceRef::commands)
// and their _var forms (var: NULL, or a record per face) and _gvar forms (gvar: NULL, or per face a description or NULL)
int family_create_tables(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var, vgsdf_family **out, bool mixed,
                         const char *me, const vgsdf_font_gvar_desc *const *gvar = nullptr, uint32_t plane = 0)
{
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !out || !in->fonts || !in->tables) {
		ctx->err = std::string(me) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	*out = nullptr;
	if (plane > 16) {
		ctx->err = std::string(me) + ": plane must be 0 .. 16";
		return VGSDF_E_ARG;
	}
	ctx->family_tables_ms[0] = ctx->family_tables_ms[1] = 0.0f;
	if (gvar)
		ctx->gvar_advance_ms = 0.0f;
	const uint32_t n_fonts = in->n_fonts;
	if (n_fonts == 0 || n_fonts > 0x10000u) {
		ctx->err = std::string(me) + ": n_fonts must be 1 .. 65536";
		return VGSDF_E_ARG;
	}
	// what can be said without a lookup; the staging block's layout on the way:
	// FamilyFaceRef[n_fonts] | FamilySubtable[all] | per face cmap, hmtx (4-aligned) |
	// with a variation: FamilyFaceVar[n_fonts] | per face HVAR, factors (4-aligned) | then, 16-aligned: counts | flags
	// with faces that take their advances' deltas from gvar (a description and no HVAR): FamilyFaceVar[n_fonts] as well (zeroed
	// for such a face), FamilyFaceGvar[n_fonts] behind the variation's bytes; the phantom pass's output lies in the context's array
	size_t n_subtables = 0, table_bytes = 0, var_bytes = 0, advance_bytes = 0;
	bool any_var = false, any_gvar = false;
	for (uint32_t k = 0; k < n_fonts; k++) {
		const vgsdf_face_tables &t = in->tables[k];
		if (!family_font_fits(ctx, in->fonts, k, mixed)) {
			ctx->err = std::string(me) + ": " + kFontsRefused[mixed];
			return VGSDF_E_ARG;
		}
		if (const char *why = face_tables_refused(t)) {
			ctx->err = std::string(me) + ": " + why;
			return VGSDF_E_ARG;
		}
		n_subtables += t.n_subtables;
		table_bytes += align_up(t.cmap_len, 4) + align_up(t.hmtx_len, 4);
		if (var) {
			if (const char *why = variation_refused(var[k])) {
				ctx->err = std::string(me) + ": " + why;
				return VGSDF_E_ARG;
			}
			if (var[k].hvar) {
				any_var = true;
				var_bytes += align_up(var[k].hvar_len, 4) + 4 * (size_t)var[k].n_regions;
			}
		}
		if (gvar && gvar[k]) {
			if (const int rc = gvar_advance_described(ctx, me, gvar[k]); rc != VGSDF_OK)
				return rc;
			if (!(var && var[k].hvar)) { // (a face with both descriptions uses HVAR)
				any_gvar = true;
				advance_bytes += gvar_advance_bytes(gvar[k]->tables.num_glyphs);
			}
		}
	}
	const bool with_var = any_var || any_gvar;
	if (with_var)
		var_bytes += sizeof(vgsdf::FamilyFaceVar) * (size_t)n_fonts;
	const size_t gvar_records = any_gvar ? sizeof(vgsdf::FamilyFaceGvar) * (size_t)n_fonts : 0;
	std::unique_ptr<vgsdf_family> f(new (std::nothrow) vgsdf_family());
	if (!f) {
		ctx->err = std::string(me) + ": out of host memory";
		return VGSDF_E_OOM;
	}
	adopt_fonts(*f, ctx, in->fonts, n_fonts, mixed);
	f->plane = plane; // (other than 0 only from vgsdf_family_create_tables_at: static faces, var and gvar NULL)
	const size_t a_subs = sizeof(vgsdf::FamilyFaceRef) * (size_t)n_fonts, a_bytes = a_subs + sizeof(vgsdf::FamilySubtable) * n_subtables,
	             a_var = align_up(a_bytes + table_bytes, 8), a_gvar = align_up(a_var + var_bytes, 8), a_counts = align_up(a_gvar + gvar_records, 16), a_flags = a_counts + 4 * (size_t)vgsdf::kFamilyCounts * vgsdf::kFamilyGroups,
	             a_total = a_flags + 16;
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(a_total); e != hipSuccess)
		return font_hip_error(ctx, me, "hipMalloc", e);
	uint8_t *d = (uint8_t *)dev.p;
	if (any_gvar) { // the phantom pass, face by face, into the context's array (nothing in flight reads it: every call that does ends synchronised)
		if (hipError_t e = ctx->gvar_advance.ensure(advance_bytes + 16); e != hipSuccess)
			return font_hip_error(ctx, me, "hipMalloc", e);
		size_t at = 0;
		for (uint32_t k = 0; k < n_fonts; k++) {
			if (!gvar[k] || (var && var[k].hvar))
				continue;
			float ms = 0.0f;
			const int rc = gvar_advance_on_device(ctx, me, gvar[k], (uint8_t *)ctx->gvar_advance.p + at, &ms);
			ctx->gvar_advance_ms += ms;
			if (rc != VGSDF_OK)
				return rc;
			at += gvar_advance_bytes(gvar[k]->tables.num_glyphs);
		}
	}
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
		if (any_gvar) {
			vgsdf::FamilyFaceGvar *recs = (vgsdf::FamilyFaceGvar *)(h.data() + a_gvar);
			size_t at = 0;
			for (uint32_t k = 0; k < n_fonts; k++) {
				if (!gvar[k] || (var && var[k].hvar))
					continue; // (zeroed: the face takes none)
				const uint32_t n_ids = gvar[k]->tables.num_glyphs;
				const uint64_t base = (uint64_t)(uintptr_t)((uint8_t *)ctx->gvar_advance.p + at);
				recs[k] = vgsdf::FamilyFaceGvar{base, base + gvar_advance_state_at(n_ids), n_ids, 0};
				at += gvar_advance_bytes(n_ids);
			}
		}
		if (any_var) {
			vgsdf::FamilyFaceVar *vars = (vgsdf::FamilyFaceVar *)(h.data() + a_var);
			size_t at = a_var + sizeof(vgsdf::FamilyFaceVar) * (size_t)n_fonts;
			for (uint32_t k = 0; k < n_fonts; k++) {
				const vgsdf_face_variation &v = var[k];
				vgsdf::FamilyFaceVar &r = vars[k]; // (zeroed: a static face)
				if (!v.hvar)
					continue;
				r.hvar = (uint64_t)(uintptr_t)(d + at);
				std::memcpy(h.data() + at, v.hvar, v.hvar_len);
				at += align_up(v.hvar_len, 4);
				r.scalars = (uint64_t)(uintptr_t)(d + at);
				if (v.n_regions)
					std::memcpy(h.data() + at, v.region_scalars, 4 * (size_t)v.n_regions);
				at += 4 * (size_t)v.n_regions;
				r.hvar_len = v.hvar_len, r.store_off = v.store_off, r.map_off = v.map_off, r.n_regions = v.n_regions;
			}
		}
	}
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, me, "hipEventCreate", err);
	const vgsdf::FamilyFaceRef *faces = (const vgsdf::FamilyFaceRef *)d;
	uint32_t *counts = (uint32_t *)(d + a_counts), *flags = (uint32_t *)(d + a_flags);
	Calls q(st);
	q.copy(d, h.data(), h.size());
	q.zero(d + a_flags, 16);
	q.record(ev.at[0]);
	q.launch([&] { return vgsdf_family_tables_count(faces, n_fonts, plane, counts, flags, st); });
	q.record(ev.at[1]);
	uint32_t got[vgsdf::kFamilyCounts * vgsdf::kFamilyGroups + 1]; // the counts and, behind them, the flag word
	q.read_back(got, counts, sizeof got);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, me, "count pass", q.e);
	ev.elapsed(ctx->family_tables_ms, 0);
	if (got[vgsdf::kFamilyCounts * vgsdf::kFamilyGroups]) {
		ctx->err = std::string(me) + ": a glyph id past its face";
		return VGSDF_E_ARG;
	}
	uint32_t n = 0;
	for (uint32_t w = 0; w < vgsdf::kFamilyGroups; w++)
		n += got[vgsdf::kFamilyCounts * w];
	// the table as vgsdf_family_create allocates it (the same size: the same vgsdf_family_device_bytes)
	const vgsdf::FamilyTableLayout at(n);
	if (hipError_t err = f->table.ensure(at.bytes + 16); err != hipSuccess)
		return font_hip_error(ctx, me, "hipMalloc", err);
	std::vector<uint8_t> back(at.bytes);
	q.record(ev.at[1]);
	q.launch([&] {
		if (any_gvar)
			return vgsdf_family_tables_emit_gvar(faces, (const vgsdf::FamilyFaceVar *)(d + a_var), (const vgsdf::FamilyFaceGvar *)(d + a_gvar), n_fonts,
			                                     counts, n, (uint8_t *)f->table.p, st);
		return any_var ? vgsdf_family_tables_emit_var(faces, (const vgsdf::FamilyFaceVar *)(d + a_var), n_fonts, counts, n, (uint8_t *)f->table.p, st)
		               : vgsdf_family_tables_emit(faces, n_fonts, plane, counts, n, (uint8_t *)f->table.p, st);
	});
	q.record(ev.at[2]);
	q.read_back(back.data(), f->table.p, at.bytes);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, me, "emit pass", q.e);
	ev.elapsed(ctx->family_tables_ms, 1);
	adopt_table(*f, back.data(), n);
	// (scales_plain stays true: every scale is 24 / units_per_em of a checked units_per_em)
	*out = f.release();
	return VGSDF_OK;
}

// vgsdf_families_create_tables and _mixed: family_create_tables for ONE face at all positions of a call, position p a family of one
// face over fonts[p].  The tables go up once; the phantom pass (a gvar description and no HVAR) runs once over (glyph id,
// position) pairs into the context's array; the count pass, its read-back, the layout and the emit pass run once each with the
// position as the grid's second dimension; two synchronisations behind the phantom pass's
int families_create_tables(vgsdf_ctx *ctx, const vgsdf_families_tables_desc *in, vgsdf_family **out, int *status, bool mixed, const char *me)
{
	if (!in) {
		ctx->err = std::string(me) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	const uint32_t n_pos = in->n_positions;
	if (n_pos == 0)
		return VGSDF_OK;
	if (!out || !status || !in->fonts) {
		ctx->err = std::string(me) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	if (n_pos > VGSDF_FAMILY_MAX_POSITIONS) {
		ctx->err = std::string(me) + ": more than 64 positions in one call";
		return VGSDF_E_ARG;
	}
	for (uint32_t p = 0; p < n_pos; p++)
		out[p] = nullptr, status[p] = VGSDF_OK;
	ctx->families_tables_ms[0] = ctx->families_tables_ms[1] = ctx->families_tables_ms[2] = 0.0f;
	const vgsdf_face_tables &t = in->tables;
	const vgsdf_face_variation *var = in->var;
	const vgsdf_fonts_gvar_desc *gvar = in->gvar;
	for (uint32_t p = 0; p < n_pos; p++)
		if (!family_font_fits(ctx, in->fonts, p, mixed)) {
			ctx->err = std::string(me) + ": " + kFontsRefused[mixed];
			return VGSDF_E_ARG;
		}
	if (const char *why = face_tables_refused(t)) {
		ctx->err = std::string(me) + ": " + why;
		return VGSDF_E_ARG;
	}
	if (var)
		for (uint32_t p = 0; p < n_pos; p++) {
			if (const char *why = variation_refused(var[p])) {
				ctx->err = std::string(me) + ": " + why;
				return VGSDF_E_ARG;
			}
			if (var[p].hvar != var[0].hvar || var[p].hvar_len != var[0].hvar_len || var[p].store_off != var[0].store_off ||
			    var[p].map_off != var[0].map_off || var[p].n_regions != var[0].n_regions) {
				ctx->err = std::string(me) + ": variation records that do not name one HVAR table (hvar, hvar_len, store_off, map_off, n_regions)";
				return VGSDF_E_ARG;
			}
		}
	if (gvar) {
		if (const int rc = gvar_advance_batch_described(ctx, me, gvar); rc != VGSDF_OK)
			return rc;
		if (gvar->n_positions != n_pos) {
			ctx->err = std::string(me) + ": a gvar description of another number of positions";
			return VGSDF_E_ARG;
		}
	}
	const bool any_var = var && var[0].hvar, any_gvar = gvar && !any_var; // (a face with both descriptions uses HVAR)
	const bool with_var = any_var || any_gvar;
	const uint32_t n_regions = any_var ? var[0].n_regions : 0, hvar_len = any_var ? var[0].hvar_len : 0;
	std::vector<std::unique_ptr<vgsdf_family>> made(n_pos); // freed on every way out but the last
	for (uint32_t p = 0; p < n_pos; p++) {
		made[p].reset(new vgsdf_family());
		adopt_fonts(*made[p], ctx, in->fonts + p, 1, mixed);
	}
	// the staging block: FamilyFaceRef[n_pos] | FamilySubtable[all] | cmap, hmtx (4-aligned) | with a variation: FamilyFaceVar[n_pos]
	// (zeroed without HVAR) | HVAR | factors [n_pos x n_regions] | FamilyFaceGvar[n_pos] | then, 16-aligned: FamilyBatchTable[n_pos]
	// (uploaded behind the count pass) | counts [n_pos x 4 x kFamilyGroups] | flags [n_pos]
	const size_t per_counts = (size_t)vgsdf::kFamilyCounts * vgsdf::kFamilyGroups;
	const size_t a_subs = sizeof(vgsdf::FamilyFaceRef) * (size_t)n_pos, a_bytes = a_subs + sizeof(vgsdf::FamilySubtable) * (size_t)t.n_subtables,
	             a_var = align_up(a_bytes + align_up(t.cmap_len, 4) + align_up(t.hmtx_len, 4), 8), a_hvar = a_var + (with_var ? sizeof(vgsdf::FamilyFaceVar) * (size_t)n_pos : 0),
	             a_scalars = a_hvar + align_up(hvar_len, 4), a_gvar = align_up(a_scalars + 4 * (size_t)n_regions * n_pos, 8),
	             a_tables = align_up(a_gvar + (any_gvar ? sizeof(vgsdf::FamilyFaceGvar) * (size_t)n_pos : 0), 16),
	             a_counts = a_tables + sizeof(vgsdf::FamilyBatchTable) * (size_t)n_pos, a_flags = a_counts + 4 * per_counts * n_pos,
	             a_total = align_up(a_flags + 4 * (size_t)n_pos, 16);
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, me, "hipMalloc", e);
	uint8_t *d = (uint8_t *)dev.p;
	const uint32_t n_ids = any_gvar ? gvar->tables.num_glyphs : 0;
	if (any_gvar) { // the phantom pass, once (nothing in flight reads the context's array: every call that does ends synchronised)
		if (hipError_t e = ctx->gvar_advance.ensure(gvar_advance_batch_bytes(n_ids, n_pos) + 16); e != hipSuccess)
			return font_hip_error(ctx, me, "hipMalloc", e);
		if (const int rc = gvar_advance_batch_on_device(ctx, me, gvar, (uint8_t *)ctx->gvar_advance.p, &ctx->families_tables_ms[0]); rc != VGSDF_OK)
			return rc;
	}
	std::vector<uint8_t> h(a_tables, 0);
	{
		vgsdf::FamilyFaceRef *faces = (vgsdf::FamilyFaceRef *)h.data();
		vgsdf::FamilySubtable *subs = (vgsdf::FamilySubtable *)(h.data() + a_subs);
		for (uint32_t s = 0; s < t.n_subtables; s++)
			subs[s] = vgsdf::FamilySubtable{t.subtable_off[s], t.subtable_format[s]};
		const size_t at_hmtx = a_bytes + align_up(t.cmap_len, 4);
		if (t.cmap_len)
			std::memcpy(h.data() + a_bytes, t.cmap, t.cmap_len);
		if (t.hmtx_len)
			std::memcpy(h.data() + at_hmtx, t.hmtx, t.hmtx_len);
		if (any_var)
			std::memcpy(h.data() + a_hvar, var[0].hvar, hvar_len);
		for (uint32_t p = 0; p < n_pos; p++) {
			const vgsdf_font &ft = *in->fonts[p];
			vgsdf::FamilyFaceRef &r = faces[p];
			r.subtables = (uint64_t)(uintptr_t)(d + a_subs);
			r.cmap = (uint64_t)(uintptr_t)(d + a_bytes);
			r.hmtx = t.hmtx_len ? (uint64_t)(uintptr_t)(d + at_hmtx) : 0;
			r.off = ft.commands ? ft.cref.cmd_off : ft.ref.leaf_off;
			r.leaves = ft.commands ? 0 : ft.ref.leaves;
			r.cmap_len = t.cmap_len, r.hmtx_len = t.hmtx_len;
			r.n_glyph_ids = ft.n_glyph_ids;
			r.units_per_em = t.units_per_em, r.num_glyphs = t.num_glyphs, r.num_hmetrics = t.num_hmetrics, r.n_subtables = t.n_subtables;
			r.commands = ft.commands ? 1u : 0u;
			if (any_var) {
				vgsdf::FamilyFaceVar &v = ((vgsdf::FamilyFaceVar *)(h.data() + a_var))[p];
				const size_t at = a_scalars + 4 * (size_t)n_regions * p;
				v.hvar = (uint64_t)(uintptr_t)(d + a_hvar);
				v.scalars = (uint64_t)(uintptr_t)(d + at);
				if (n_regions)
					std::memcpy(h.data() + at, var[p].region_scalars, 4 * (size_t)n_regions);
				v.hvar_len = hvar_len, v.store_off = var[0].store_off, v.map_off = var[0].map_off, v.n_regions = n_regions;
			}
			if (any_gvar) { // position p's slices of the batched phantom pass
				const uint8_t *o = (const uint8_t *)ctx->gvar_advance.p;
				((vgsdf::FamilyFaceGvar *)(h.data() + a_gvar))[p] =
				    vgsdf::FamilyFaceGvar{(uint64_t)(uintptr_t)(o + 4 * (size_t)n_ids * p),
				                          (uint64_t)(uintptr_t)(o + gvar_advance_batch_state_at(n_ids, n_pos) + (size_t)n_ids * p), n_ids, 0};
			}
		}
	}
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, me, "hipEventCreate", err);
	const vgsdf::FamilyFaceRef *faces = (const vgsdf::FamilyFaceRef *)d;
	uint32_t *counts = (uint32_t *)(d + a_counts), *flags = (uint32_t *)(d + a_flags);
	Calls q(st);
	q.copy(d, h.data(), h.size());
	q.zero(d + a_flags, 4 * (size_t)n_pos);
	q.record(ev.at[0]);
	q.launch([&] { return vgsdf_family_tables_batch_count(faces, n_pos, counts, flags, st); });
	q.record(ev.at[1]);
	std::vector<uint32_t> got((per_counts + 1) * n_pos); // the counts and, behind them, the positions' flag words
	q.read_back(got.data(), counts, 4 * got.size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, me, "count pass", q.e);
	ev.elapsed(ctx->families_tables_ms + 1, 0);
	// per position: refused, or a table as vgsdf_family_create allocates it (the same size: the same vgsdf_family_device_bytes)
	std::vector<vgsdf::FamilyBatchTable> tables(n_pos, vgsdf::FamilyBatchTable{0, 0, 0});
	std::vector<std::vector<uint8_t>> back(n_pos);
	uint32_t n_built = 0;
	for (uint32_t p = 0; p < n_pos; p++) {
		if (got[per_counts * n_pos + p]) {
			ctx->err = std::string(me) + ": position " + std::to_string(p) + ": a glyph id past its face";
			status[p] = VGSDF_E_ARG;
			made[p].reset();
			continue;
		}
		uint32_t n = 0;
		for (uint32_t w = 0; w < vgsdf::kFamilyGroups; w++)
			n += got[per_counts * p + vgsdf::kFamilyCounts * w];
		const vgsdf::FamilyTableLayout at(n);
		if (hipError_t err = made[p]->table.ensure(at.bytes + 16); err != hipSuccess)
			return font_hip_error(ctx, me, "hipMalloc", err);
		tables[p] = vgsdf::FamilyBatchTable{(uint64_t)(uintptr_t)made[p]->table.p, n, 0};
		back[p].resize(at.bytes);
		n_built++;
	}
	if (n_built == 0)
		return VGSDF_OK;
	q.copy(d + a_tables, tables.data(), sizeof(vgsdf::FamilyBatchTable) * (size_t)n_pos);
	q.record(ev.at[1]);
	q.launch([&] {
		return vgsdf_family_tables_batch_emit(faces, with_var ? (const vgsdf::FamilyFaceVar *)(d + a_var) : nullptr,
		                                      any_gvar ? (const vgsdf::FamilyFaceGvar *)(d + a_gvar) : nullptr, n_pos, counts,
		                                      (const vgsdf::FamilyBatchTable *)(d + a_tables), st);
	});
	q.record(ev.at[2]);
	for (uint32_t p = 0; p < n_pos; p++)
		if (made[p] && !back[p].empty())
			q.read_back(back[p].data(), made[p]->table.p, back[p].size());
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, me, "emit pass", q.e);
	ev.elapsed(ctx->families_tables_ms + 1, 1);
	for (uint32_t p = 0; p < n_pos; p++)
		if (made[p])
			adopt_table(*made[p], back[p].data(), tables[p].n_entries);
	for (uint32_t p = 0; p < n_pos; p++)
		out[p] = made[p].release();
	return VGSDF_OK;
}

// the exported pair: no context, no call; an exhausted host fails the call whole (the families made so far are freed on the way)
int families_create_tables_guarded(vgsdf_ctx *ctx, const vgsdf_families_tables_desc *in, vgsdf_family **out, int *status, bool mixed, const char *me)
{
	if (!ctx)
		return VGSDF_E_ARG;
	try {
		return families_create_tables(ctx, in, out, status, mixed, me);
	} catch (const std::bad_alloc &) {
		ctx->err = std::string(me) + ": out of host memory";
		return VGSDF_E_OOM;
	}
}

} // namespace

extern "C" {

int vgsdf_family_create(vgsdf_ctx *ctx, const vgsdf_family_desc *in, vgsdf_family **out)
{
	return family_create(ctx, in, out, false, "vgsdf_family_create");
}
int vgsdf_family_create_mixed(vgsdf_ctx *ctx, const vgsdf_family_desc *in, vgsdf_family **out)
{
	return family_create(ctx, in, out, true, "vgsdf_family_create_mixed");
}
int vgsdf_family_create_tables(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, vgsdf_family **out)
{
	return family_create_tables(ctx, in, nullptr, out, false, "vgsdf_family_create_tables");
}
int vgsdf_family_create_tables_mixed(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, vgsdf_family **out)
{
	return family_create_tables(ctx, in, nullptr, out, true, "vgsdf_family_create_tables_mixed");
}
// the planes' entry points: `kind` chooses between the two constructors of each pair
int vgsdf_family_create_at(vgsdf_ctx *ctx, const vgsdf_family_desc *in, int kind, uint32_t plane, vgsdf_family **out)
{
	if (ctx && kind != VGSDF_FAMILY_ONE_KIND && kind != VGSDF_FAMILY_MIXED) {
		ctx->err = "vgsdf_family_create_at: kind must be VGSDF_FAMILY_ONE_KIND or VGSDF_FAMILY_MIXED";
		return VGSDF_E_ARG;
	}
	return family_create(ctx, in, out, kind == VGSDF_FAMILY_MIXED, "vgsdf_family_create_at", plane);
}
int vgsdf_family_create_tables_at(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, int kind, uint32_t plane, vgsdf_family **out)
{
	if (ctx && kind != VGSDF_FAMILY_ONE_KIND && kind != VGSDF_FAMILY_MIXED) {
		ctx->err = "vgsdf_family_create_tables_at: kind must be VGSDF_FAMILY_ONE_KIND or VGSDF_FAMILY_MIXED";
		return VGSDF_E_ARG;
	}
	return family_create_tables(ctx, in, nullptr, out, kind == VGSDF_FAMILY_MIXED, "vgsdf_family_create_tables_at", nullptr, plane);
}
uint32_t vgsdf_family_plane(const vgsdf_family *family) { return family ? family->plane : 0; }

// the census of the faces' cmap tables (family_census_kernels.hip): the tables go up, one workgroup per subtable ORs what it lists
// into 136 zeroed words, the words come back; one synchronisation.  The fonts of the description are not looked at
int vgsdf_family_tables_census(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, uint32_t bits[VGSDF_CENSUS_WORDS])
{
	const char *me = "vgsdf_family_tables_census";
	if (!ctx)
		return VGSDF_E_ARG;
	if (!in || !bits || !in->tables) {
		ctx->err = std::string(me) + ": NULL argument";
		return VGSDF_E_ARG;
	}
	if (in->n_fonts == 0 || in->n_fonts > 0x10000u) {
		ctx->err = std::string(me) + ": n_fonts must be 1 .. 65536";
		return VGSDF_E_ARG;
	}
	size_t n_subtables = 0, table_bytes = 0;
	for (uint32_t k = 0; k < in->n_fonts; k++) {
		if (const char *why = face_tables_refused(in->tables[k])) {
			ctx->err = std::string(me) + ": " + why;
			return VGSDF_E_ARG;
		}
		n_subtables += in->tables[k].n_subtables;
		table_bytes += align_up(in->tables[k].cmap_len, 4);
	}
	if (n_subtables > 0x7FFFFFFFu) {
		ctx->err = std::string(me) + ": more than 2^31 - 1 subtables over the faces";
		return VGSDF_E_ARG;
	}
	ctx->family_census_ms = 0.0f;
	// the staging block: CensusSubtable[all] | per face cmap (4-aligned) | then, 16-aligned: the bitmap
	const size_t a_bytes = sizeof(vgsdf::CensusSubtable) * n_subtables, a_bits = align_up(a_bytes + table_bytes, 16),
	             a_total = a_bits + 4 * (size_t)vgsdf::kCensusWords;
	static_assert(VGSDF_CENSUS_WORDS == vgsdf::kCensusWords, "the bitmap of the header is the kernel's");
	(void)hipSetDevice(ctx->device);
	hipStream_t st = ctx->stream;
	ScratchBuf dev;
	if (hipError_t e = dev.ensure(a_total + 16); e != hipSuccess)
		return font_hip_error(ctx, me, "hipMalloc", e);
	uint8_t *d = (uint8_t *)dev.p;
	std::vector<uint8_t> h(a_bits, 0);
	{
		vgsdf::CensusSubtable *subs = (vgsdf::CensusSubtable *)h.data();
		size_t at_sub = 0, at_byte = a_bytes;
		for (uint32_t k = 0; k < in->n_fonts; k++) {
			const vgsdf_face_tables &t = in->tables[k];
			for (uint32_t s = 0; s < t.n_subtables; s++) // (subtable_off < cmap_len: face_tables_refused)
				subs[at_sub++] = vgsdf::CensusSubtable{(uint64_t)(uintptr_t)(d + at_byte + t.subtable_off[s]), t.cmap_len - t.subtable_off[s], t.subtable_format[s]};
			if (t.cmap_len)
				std::memcpy(h.data() + at_byte, t.cmap, t.cmap_len);
			at_byte += align_up(t.cmap_len, 4);
		}
	}
	PassEvents ev;
	if (hipError_t err = ev.create(); err != hipSuccess)
		return font_hip_error(ctx, me, "hipEventCreate", err);
	uint32_t got[vgsdf::kCensusWords];
	Calls q(st);
	q.copy(d, h.data(), h.size());
	q.zero(d + a_bits, 4 * (size_t)vgsdf::kCensusWords);
	q.record(ev.at[0]);
	q.launch([&] { return vgsdf_family_census_launch((const vgsdf::CensusSubtable *)d, (uint32_t)n_subtables, (uint32_t *)(d + a_bits), st); });
	q.record(ev.at[1]);
	q.read_back(got, d + a_bits, sizeof got);
	q.sync();
	if (q.failed())
		return font_hip_error(ctx, me, "census", q.e);
	(void)hipEventElapsedTime(&ctx->family_census_ms, ev.at[0], ev.at[1]);
	std::memcpy(bits, got, sizeof got);
	return VGSDF_OK;
}
float vgsdf_family_census_kernel_ms(const vgsdf_ctx *ctx) { return ctx ? ctx->family_census_ms : 0.0f; }
int vgsdf_family_create_tables_var(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var, vgsdf_family **out)
{
	return family_create_tables(ctx, in, var, out, false, "vgsdf_family_create_tables_var");
}
int vgsdf_family_create_tables_var_mixed(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var, vgsdf_family **out)
{
	return family_create_tables(ctx, in, var, out, true, "vgsdf_family_create_tables_var_mixed");
}

int vgsdf_family_create_tables_gvar(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var,
                                    const vgsdf_font_gvar_desc *const *gvar, vgsdf_family **out)
{
	return family_create_tables(ctx, in, var, out, false, "vgsdf_family_create_tables_gvar", gvar);
}
int vgsdf_family_create_tables_gvar_mixed(vgsdf_ctx *ctx, const vgsdf_family_tables_desc *in, const vgsdf_face_variation *var,
                                          const vgsdf_font_gvar_desc *const *gvar, vgsdf_family **out)
{
	return family_create_tables(ctx, in, var, out, true, "vgsdf_family_create_tables_gvar_mixed", gvar);
}

int vgsdf_families_create_tables(vgsdf_ctx *ctx, const vgsdf_families_tables_desc *in, vgsdf_family **out, int *status)
{
	return families_create_tables_guarded(ctx, in, out, status, false, "vgsdf_families_create_tables");
}
int vgsdf_families_create_tables_mixed(vgsdf_ctx *ctx, const vgsdf_families_tables_desc *in, vgsdf_family **out, int *status)
{
	return families_create_tables_guarded(ctx, in, out, status, true, "vgsdf_families_create_tables_mixed");
}
void vgsdf_families_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[3])
{
	if (ms)
		for (int i = 0; i < 3; i++)
			ms[i] = ctx ? ctx->families_tables_ms[i] : 0.0f;
}

void vgsdf_family_tables_kernel_ms(const vgsdf_ctx *ctx, float ms[2]) { pass_ms_out(ctx ? ctx->family_tables_ms : nullptr, ms); }

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
