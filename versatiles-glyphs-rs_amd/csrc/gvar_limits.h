// gvar_limits.h — the bounds of the device's builder of a placed `glyf` face's command store (gvar_kernels.hip,
// vgsdf_font_create_gvar) that its kernels and its entry point share.  The host reader (host/ttf_face.cpp, GvarWalker and
// GvarTable::accumulate: the statement of behaviour) has none of them: a face past one is refused and built from the reader.
#pragma once
#include <cstdint>

#include "../../include/vgsdf.h"

// VGSDF_GVAR_MAX_DELTAS (vgsdf.h): a glyph id's own entry applies at most that many deltas, its tuples x its points (the 4
// phantom points included), whatever the tuples' scalars.  One lane works through them alone (4095 tuples over 65539 points
// would be 2.7e8); real glyphs stay below a few thousand.

namespace vg {

constexpr uint32_t kGvarMaxAxes = 64;            // fvar axes of a face (the instance interface's bound)
constexpr uint32_t kGvarMaxRecords = 0xFFFF;     // component records of ONE composite entry (its points are numbered in 16 bits)
constexpr uint32_t kGvarMaxGlyphCmds = 1u << 26; // commands of one glyph id (kResidentMaxGlyphSlots of glyf_table_limits.h)
constexpr uint32_t kGvarSlicePoints = 1u << 17;  // points of one launch of the deltas pass: a slice of glyph ids ends before the
                                                 // glyph id that would pass it (a slice of one glyph id may: at most 65539).
                                                 // vgsdf_fonts_create_gvar: points x positions of one launch, by the same rule
                                                 // (a glyph id that passes it with all positions goes in runs of positions)

} // namespace vg
