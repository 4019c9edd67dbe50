// resident_fonts.h — a font resident on a device, as its store (resident_fonts.cpp) fills it and the front-end
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
	vgsdf::CommandFontRef cref{};
	vgsdf_font() = default;
	vgsdf_font(const vgsdf_font &) = delete;
	vgsdf_font &operator=(const vgsdf_font &) = delete;
	~vgsdf_font() { store.release(); } // (the owner has made the font's device current)
};
