// charstring_kernels.h — the device's Type 2 charstring decoder (charstring_kernels.hip): a CFF or CFF2 face's charstrings in, the
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

// the same of a `CFF2` face (vgsdf_font_charstrings2_desc, validated by vgsdf_font_create_charstrings2), with its blend sets and
// the launch's workspace.  lsubr_first is {0, n}; fd_of is NULL.  A launch decodes the glyph ids [0, n_glyph_ids) of cs_off: a
// chunk of a face is given by offsetting cs_off (and counts / cmd_off / dat_off) to its first glyph id.
struct Charstrings2Ref : CharstringsRef {
	const uint8_t *set_ok;   // [n_sets]: 0 = the set is not usable (a glyph that selects it ends there)
	const uint32_t *set_off; // [n_sets + 1] into factors: set s has set_off[s + 1] - set_off[s] <= 64 regions
	const float *factors;    // one factor per region of every set
	float *spill;            // operand slots past the LDS window: [kCharstringMaxOperands2 - kCharstringWindow][spill_stride]
	uint32_t n_sets;
	uint32_t spill_stride;   // lanes of the launch: n_glyph_ids rounded up to the wave
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
// the CFF2 stamping of the two passes (hipErrorInvalidValue: spill_stride below the lanes of the launch)
int vgsdf_charstring2_count(const vgsdf::Charstrings2Ref *face, uint32_t *counts, uint32_t *flags, hipStream_t stream);
int vgsdf_charstring2_emit(const vgsdf::Charstrings2Ref *face, const uint32_t *cmd_off, const uint32_t *dat_off, uint8_t *kinds,
                           float *coords, uint32_t *flags, hipStream_t stream);
}
