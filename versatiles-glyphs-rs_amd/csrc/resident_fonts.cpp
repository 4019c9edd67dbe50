// resident_fonts.cpp — the stores behind vgsdf_font that the host hands over ready: a face's outlines uploaded once, as `glyf`
// leaves (vgsdf_font_create) or as expanded commands (vgsdf_font_create_commands), and what every font answers whichever call made
// it (vgsdf_font_read, _commands_read, _free, _device_bytes).  The stores the DEVICE builds: resident_glyf_tables.cpp (from loca and
// glyf), resident_charstrings.cpp (from a CFF face's charstrings), resident_gvar.cpp (a placed glyf face, from loca, glyf and gvar).
// Submissions that name their glyphs read them (outline_front_end.cpp, vgsdf_outlines_submit_resident).  Each kind has one layout
// (upload_layout.h: GlyfStoreLayout, CommandStoreLayout) and one function that finishes a store in it (resident_build.h,
// resident_command_store.h); the families over the fonts: resident_families.cpp.
#include <algorithm>
#include <memory>
#include <new>

#include "resident_command_store.h"

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
	if (n > 0x10000u || !command_store_addressable(n, n_cmds, in->n_floats)) {
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
