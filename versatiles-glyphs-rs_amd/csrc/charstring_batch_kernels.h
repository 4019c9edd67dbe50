// charstring_batch_kernels.h — the CFF2 stamping of the charstring decoder over (glyph id, position) pairs
// (charstring_batch_kernels.hip), for vgsdf_fonts_create_charstrings2: one face's charstrings at many positions of the design
// space, the stores of all of them in one count pass and one emit pass.
#pragma once
#include "charstring_kernels.h"

namespace vgsdf {

// what differs between the positions of a launch, all device addresses.  The count pass reads factors and flags of every
// position of the call; the emit pass every field, of the positions whose stores are built
struct Charstrings2PositionRef {
	const float *factors;    // [n_factors]: the position's factor of every region of every set (Charstrings2Ref::set_off into it)
	const uint32_t *cmd_off; // [n_glyph_ids + 1]: the position's store's
	const uint32_t *dat_off; // [n_glyph_ids + 1]
	uint8_t *kinds;
	float *coords;
	uint32_t *flags; // the position's flag word (CS_FLAG_*)
};

} // namespace vgsdf

extern "C" {
// Both passes decode the glyph ids [g0, face->n_glyph_ids) of `face` (the whole face's arrays; face->factors is not read) at the
// n_positions positions of `positions`, lane = (glyph id - g0) x n_positions + position: the lanes of one glyph id are neighbours.
// hipErrorInvalidValue: no position, g0 not below n_glyph_ids, more than 2^24 lanes, or face->spill_stride below the lanes of the
// launch rounded up to the wave.
// count pass: counts[2 pair] / counts[2 pair + 1] = the commands / coordinates of pair = glyph id x n_positions + position
int vgsdf_charstring2_batch_count(const vgsdf::Charstrings2Ref *face, uint32_t g0, const vgsdf::Charstrings2PositionRef *positions,
                                  uint32_t n_positions, uint32_t *counts, hipStream_t stream);
// emit pass: glyph id g at position p into p's kinds[cmd_off[g] .. cmd_off[g + 1]) and coords[dat_off[g] .. dat_off[g + 1])
int vgsdf_charstring2_batch_emit(const vgsdf::Charstrings2Ref *face, uint32_t g0, const vgsdf::Charstrings2PositionRef *positions,
                                 uint32_t n_positions, hipStream_t stream);
}
