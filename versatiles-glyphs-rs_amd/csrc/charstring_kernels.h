// charstring_kernels.h — the device's Type 2 charstring decoder (charstring_kernels.hip): a CFF face's charstrings in, the
// callbacks of every glyph id out, in the arrays of the packed upload form (kinds | coords).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vgsdf {

// what the decoder reads of a face, all device addresses (vgsdf_font_charstrings_desc of include/vgsdf.h, validated by
// vgsdf_font_create_charstrings: every offset array ascends and ends inside `bytes`, every fd_of is below n_fds)
struct CharstringsRef {
	const uint32_t *words;       // `bytes`, 4-aligned, a multiple of 4 long: read a word at a time
	const uint32_t *cs_off;      // [n_glyph_ids + 1]
	const uint32_t *gsubr_off;   // [n_gsubrs + 1]
	const uint32_t *lsubr_first; // [n_fds + 1]
	const uint32_t *lsubr_off;   // [lsubr_first[n_fds] + 1]
	const uint8_t *fd_of;        // [n_glyph_ids] or NULL (every glyph id: FD 0)
	uint32_t n_glyph_ids, n_gsubrs;
};

// bits of the decoder's flag word
enum : uint32_t {
	CS_FLAG_SEAC = 1u,   // a glyph whose endchar takes the seac form
	CS_FLAG_BUDGET = 2u, // a glyph past VGSDF_CHARSTRING_MAX_TOKENS
	CS_FLAG_RANGE = 4u,  // emit only: a glyph delivered more than its counted range holds (never, by construction)
};

} // namespace vgsdf

extern "C" {
// count pass: counts[2 g] / counts[2 g + 1] = the commands / coordinates glyph id g delivers; flags: one zeroed word
int vgsdf_charstring_count(const vgsdf::CharstringsRef *face, uint32_t *counts, uint32_t *flags, hipStream_t stream);
// emit pass: glyph id g's kinds into kinds[cmd_off[g] .. cmd_off[g + 1]) and its coordinates into
// coords[dat_off[g] .. dat_off[g + 1]), the offsets being the running sums of the count pass
int vgsdf_charstring_emit(const vgsdf::CharstringsRef *face, const uint32_t *cmd_off, const uint32_t *dat_off, uint8_t *kinds,
                          float *coords, uint32_t *flags, hipStream_t stream);
}
