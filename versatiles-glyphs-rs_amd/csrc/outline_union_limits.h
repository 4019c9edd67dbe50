// outline_union_limits.h — the limits of the union pass (outline_union_kernels.hip), mirrored by tests/union_outline_kit.py.
#pragma once

// The partners of a glyph's segments pass through a window in LDS: four f64 arrays of this many segments, 32 KiB; with the
// lanes' counts and the votes a workgroup takes 34048 B (count) / 33024 B (emit), so four fit a CU's 160 KiB: 4 waves per SIMD.
// A glyph of up to one window is staged once; a larger one is swept window by window.
#define VGSDF_UNION_WINDOW 1024
// A glyph of more segments is passed through unchanged (state 2): the pair loop is O(N^2) in ONE workgroup, and this bounds
// it to 36 windows' worth of pairs.  The largest glyph of the 21 fixture fonts has 5341 segments (Noto Sans Arabic, U+FDFD).
#define VGSDF_UNION_MAX_SEGMENTS 6144

// a glyph's state byte after the count pass
#define VGSDF_UNION_IDENTITY 0   // no cut point, no interior piece: the input less its zero-length segments
#define VGSDF_UNION_REBUILT 1
#define VGSDF_UNION_OVER_LIMIT 2 // more than VGSDF_UNION_MAX_SEGMENTS: passed through unchanged
#define VGSDF_UNION_NON_FINITE 3 // a coordinate that is not finite: passed through unchanged
