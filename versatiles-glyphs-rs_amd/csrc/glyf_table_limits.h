// glyf_table_limits.h — the bounds of a `glyf` face's resident form that its two statements share: the host reader
// (host/ttf_face.cpp, Face::resident_table: the statement of behaviour) and the device's table builder
// (glyf_table_kernels.hip, vgsdf_font_create_tables), which must equal it byte for byte.
#pragma once
#include <cstdint>

// A glyph id visits at most this many component records (a record counts when its four leading bytes have been read);
// the device refuses a face with a glyph past it, whatever the font says about itself: termination does not depend on it.
#define VGSDF_GLYF_MAX_COMPONENTS (1u << 20)

namespace vg {

constexpr int kGlyfMaxComponentDepth = 32;        // ttf-parser: MAX_COMPONENTS (a glyph at this depth fails)
constexpr uint32_t kGlyfMaxEntry = 32 * 1024;     // end points + arrays of a simple entry that are copied; a longer one holds nothing
constexpr uint64_t kResidentMaxLeaves = 1ull << 22;      // leaves of a face
constexpr uint64_t kResidentMaxGlyphSlots = 1ull << 26;  // command slots of one glyph id
constexpr uint64_t kResidentMaxBytes = (1ull << 32) - 4; // the store of the simple entries
constexpr uint64_t kResidentMaxSlotSum = 0xFFFFFFFFull;  // the running sum of the glyph ids' command slots

} // namespace vg
