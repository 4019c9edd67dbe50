// outline_union_kernels.h — the union pass: a glyph's segments rewritten into the boundary of its filled set (rule U,
// DESIGN.md §7).  One workgroup per glyph, two passes of one text (outline_union_pass.inc).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "outline_union_limits.h"
#include "sdf_kernels.h"

// The segments are read in either layout of a resident batch (seg_stride 1 or 4, sdf_kernels.h).
// Count pass: per glyph its number of pieces and its state byte; per INPUT segment (indexed as the segments themselves, without
// the stride) the place of its first piece among the glyph's pieces, which the emit pass reads back.
extern "C" int vgsdf_outline_union_count(const vgsdf::GlyphDesc *glyphs, uint32_t n_glyphs, const double *sx, const double *sy,
                                         const double *ex, const double *ey, uint32_t seg_stride, uint32_t *piece_count,
                                         uint8_t *state, uint32_t *seg_first, hipStream_t stream);
// Emit pass: the same walk; glyph g's pieces go to [piece_off[g], piece_off[g + 1]) of the output arrays (layout out_stride),
// a glyph of state 2 or 3 is copied.  Nothing is stored outside a glyph's own range.
extern "C" int vgsdf_outline_union_emit(const vgsdf::GlyphDesc *glyphs, uint32_t n_glyphs, const double *sx, const double *sy,
                                        const double *ex, const double *ey, uint32_t seg_stride, const uint8_t *state,
                                        const uint32_t *seg_first, const uint32_t *piece_off, double *out_sx, double *out_sy,
                                        double *out_ex, double *out_ey, uint32_t out_stride, hipStream_t stream);
