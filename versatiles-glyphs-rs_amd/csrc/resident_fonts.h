// resident_fonts.h — a font resident on a device, as its constructor (resident_*.cpp) fills it and the front-end
// (outline_front_end.cpp) reads it when a submission names glyphs by (font, glyph id).
#pragma once
#include <vector>

#include "device_internal.h"
#include "upload_layout.h"

// vgsdf_font_create: one allocation leaves | bytes | leaf_off, and what the host needs per glyph id to lay a submission
// out without looking at a leaf
struct vgsdf_font {
	int device = 0;
	uint32_t n_glyph_ids = 0, n_leaves = 0, n_bytes = 0;
	DevBuf store;
	vgsdf::ResidentFontRef ref{};       // device addresses of the three arrays
	std::vector<uint32_t> leaf_off;     // [n_glyph_ids + 1]
	std::vector<uint32_t> slots;        // [n_glyph_ids] command slots of the glyph's leaves
	uint32_t max_cap = 0, max_len = 0;  // the largest cmd_cap / byte_len among the leaves (the decoder's LDS is sized from them)
	// a command font (vgsdf_font_create_commands): one allocation records | cmd_off | context bytes; `slots` holds the glyph
	// ids' command counts and nothing of the leaves above is used
	bool commands = false;
	uint32_t n_cmds = 0; // of the store
	vgsdf::CommandFontRef cref{};
	vgsdf_font() = default;
	vgsdf_font(const vgsdf_font &) = delete;
	vgsdf_font &operator=(const vgsdf_font &) = delete;
	~vgsdf_font() { store.release(); } // (the owner has made the font's device current)
};

// a font's reference in a list that holds fonts of both kinds (upload_layout.h): its three addresses and its kind
inline vgsdf::MixedFontRef mixed_font_ref(const vgsdf_font &ft)
{
	return ft.commands ? vgsdf::MixedFontRef{ft.cref.cmd_off, ft.cref.cmds, ft.cref.open, vgsdf::kFontRefCommands}
	                   : vgsdf::MixedFontRef{ft.ref.leaf_off, ft.ref.leaves, ft.ref.bytes, vgsdf::kFontRefGlyf};
}

// vgsdf_family_create: the table code point -> (font, glyph id, advance, scale, shift_x) of a font id, on the host (what a
// ranges submission is laid out from in O(tasks)) and on the device (upload_layout.h, FamilyTableLayout: what its upload
// kernel names the glyphs from).  Owns no font
struct vgsdf_family {
	int device = 0;
	bool commands = false;    // the kind of its fonts
	bool mixed = false;       // a third kind (vgsdf_family_create_mixed): fonts of either kind, font by font; `commands` stays false
	bool scales_plain = true; // every scale positive and finite
	uint32_t plane = 0;       // 0 .. 16: code_point holds the low halves of (plane << 16) | x (vgsdf_family_create_at)
	uint32_t max_cap = 0, max_len = 0; // over its fonts (vgsdf_font); a mixed family: over its glyf fonts
	std::vector<const vgsdf_font *> fonts;
	std::vector<uint16_t> code_point, font_of, glyph_id;
	std::vector<uint32_t> advance;
	std::vector<double> scale, shift_x;
	std::vector<uint8_t> pbf_fix;
	std::vector<uint64_t> cmd_pre, leaf_pre; // [n_entries + 1] prefix sums of command slots / leaves (leaves: glyf fonts only)
	DevBuf table;
	vgsdf_family() = default;
	vgsdf_family(const vgsdf_family &) = delete;
	vgsdf_family &operator=(const vgsdf_family &) = delete;
	~vgsdf_family() { table.release(); }
};
