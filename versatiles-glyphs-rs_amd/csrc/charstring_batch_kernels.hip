// charstring_batch_kernels.hip — CFF2 charstrings decoded at many positions of the design space in one launch: the CFF2 stamping
// of charstring_decode.inc (the text of charstring_kernels.hip, which states its rules and bounds) over (glyph id, position)
// pairs.  A position is data: its factors, its store's ranges and its flag word come from a record in device memory
// (Charstrings2PositionRef); the bytes, the offset arrays and the sets' usability are the face's and stand once.
//
// lane = (glyph id - g0) x n_positions + position, so the lanes of one glyph id are neighbours: they read the same words of the
// same stream and part only where the factors make them part (a blended subroutine index or blend count).  Both passes run over
// pairs, because what a glyph delivers may depend on the position.  The operand slots past the LDS window lie in the launch's
// workspace at the lane's index in the launch, [slot - window][lane of the launch]: every index is below
// (513 - window) x spill_stride, and spill_stride is checked against the launch's lanes before it starts.  LDS per workgroup is
// that of the single stamping; workgroups are one wave.
#include "charstring_batch_kernels.h"

#include "../../include/vgsdf.h"
#include "charstring_limits.h"
#include "outline_kernels.h"

namespace {

using vgsdf::Charstrings2PositionRef;
using vgsdf::Charstrings2Ref;

#include "charstring_decode_support.inc"

constexpr bool CFF2 = true;
constexpr uint32_t kMaxLanes = 1u << 24;

template <bool EMIT>
__global__ __launch_bounds__(kLanes) void charstring2_batch_decode(const Charstrings2Ref face, uint32_t g0,
                                                                    const Charstrings2PositionRef *__restrict__ positions, uint32_t n_positions,
                                                                    uint32_t *__restrict__ counts)
{
	const uint32_t lane = threadIdx.x, column = blockIdx.x * kLanes + lane;
	if (column >= (face.n_glyph_ids - g0) * n_positions)
		return; // (no barrier below: a lane's slots of the stacks are its own)
	const uint32_t g_in = column / n_positions, position = column - g_in * n_positions, gid = g0 + g_in;
	const uint32_t slot = EMIT ? gid : g0 * n_positions + column;
	const Charstrings2PositionRef at = positions[position];
	const float *factors_all = at.factors;
	const uint32_t *cmd_off = at.cmd_off, *dat_off = at.dat_off;
	uint8_t *kinds = at.kinds;
	float *coords = at.coords;
	uint32_t *flags = at.flags;
#include "charstring_decode.inc"
}

// the lanes of a launch; 0: not a launch these kernels take
uint32_t lanes_of(const Charstrings2Ref &face, uint32_t g0, uint32_t n_positions)
{
	if (n_positions == 0 || g0 >= face.n_glyph_ids)
		return 0;
	const uint64_t lanes = (uint64_t)(face.n_glyph_ids - g0) * n_positions;
	if (lanes > kMaxLanes || face.spill_stride < ((lanes + kLanes - 1) / kLanes) * kLanes)
		return 0;
	return (uint32_t)lanes;
}

} // namespace

extern "C" {

int vgsdf_charstring2_batch_count(const Charstrings2Ref *face, uint32_t g0, const Charstrings2PositionRef *positions, uint32_t n_positions,
                                  uint32_t *counts, hipStream_t stream)
{
	const uint32_t lanes = lanes_of(*face, g0, n_positions);
	if (!lanes)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL((charstring2_batch_decode<false>), dim3((lanes + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, *face, g0, positions,
	                   n_positions, counts);
	return (int)hipGetLastError();
}

int vgsdf_charstring2_batch_emit(const Charstrings2Ref *face, uint32_t g0, const Charstrings2PositionRef *positions, uint32_t n_positions,
                                 hipStream_t stream)
{
	const uint32_t lanes = lanes_of(*face, g0, n_positions);
	if (!lanes)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL((charstring2_batch_decode<true>), dim3((lanes + kLanes - 1) / kLanes), dim3(kLanes), 0, stream, *face, g0, positions,
	                   n_positions, nullptr);
	return (int)hipGetLastError();
}
}
