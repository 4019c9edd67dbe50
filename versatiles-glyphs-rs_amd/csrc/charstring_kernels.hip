// charstring_kernels.hip — Type 2 charstrings (`CFF ` version 1, and `CFF2` with its `vsindex` / `blend`) decoded on the device:
// the operator set and the rules of host/cff.cpp's CharStringRun, restated for one lane per glyph id.  The host reader is the
// statement of behaviour; what this kernel delivers equals its callbacks bit for bit (f32, one addition per coordinate in
// operand order, -ffp-contract=off).
//
// A charstring is sequential (variable-length tokens, a hintmask whose length depends on the stems counted so far,
// subroutine calls), so a lane walks one glyph id's program from its first byte to its end.  The walk runs twice from one
// text: COUNT notes how many commands and coordinates the glyph delivers, EMIT writes them behind the running sums of the
// counts.  Workgroups are one wave, so a face of a few thousand glyph ids spreads over the CUs.
//
// Operand stack and call stack are indexed at run time and live in LDS, slot-major ([slot][lane]: the lanes of a wave at
// one depth touch 64 consecutive words), 48 x 64 x 4 B + 2 x 10 x 64 x 4 B = 17 KB per workgroup; nothing is in scratch.
// Every byte read lies inside the current stream's [pos, end), a range of an offset array the host has validated; every
// subroutine index is checked against its set's count after the bias; every stack index against its limit.  Termination
// does not depend on the font: a glyph executes at most VGSDF_CHARSTRING_MAX_TOKENS tokens (ten call levels of fan-out k are
// k^10 of them), then sets CS_FLAG_BUDGET and stops.
//
// The CFF2 stamping (second template parameter) is the same text with CharStringRun's cff2 rules: no width operand, `return` and
// `endchar` fail the glyph, a mask past the end ends the stream, the glyph ends with its data, `vsindex` selects a set of blend
// factors and `blend` folds each value's deltas into it (f32, one product and one sum per delta, in the host's order).  The
// factors are data in device memory: a position in the design space is another array, not another kernel.  Its operand stack
// holds 513 values: the first kCharstringWindow slots are the LDS array of the version 1 stamping (the same LDS per workgroup,
// the same waves per SIMD), slots past it live in a global workspace laid out like the LDS array, [slot - window][lane of the
// launch], so the lanes of a wave at one depth touch consecutive words.  Every workspace index is below
// (513 - window) x spill_stride, which the launch allocates.
//
// The walk itself is charstring_decode.inc over charstring_decode_support.inc: charstring_batch_kernels.hip stamps the same text
// over (glyph id, position) pairs.
#include "charstring_kernels.h"

#include "../../include/vgsdf.h"
#include "charstring_limits.h"
#include "outline_kernels.h"

namespace {

using vgsdf::Charstrings2Ref;
using vgsdf::CharstringsRef;

#include "charstring_decode_support.inc"

template <bool CFF2> struct FaceOf {
	using type = CharstringsRef;
};
template <> struct FaceOf<true> {
	using type = Charstrings2Ref;
};

template <bool EMIT, bool CFF2>
__global__ __launch_bounds__(kLanes) void charstring_decode(const typename FaceOf<CFF2>::type face, uint32_t *__restrict__ counts,
                                                             const uint32_t *__restrict__ cmd_off, const uint32_t *__restrict__ dat_off,
                                                             uint8_t *__restrict__ kinds, float *__restrict__ coords, uint32_t *flags)
{
	const uint32_t lane = threadIdx.x, gid = blockIdx.x * kLanes + lane;
	if (gid >= face.n_glyph_ids)
		return; // (no barrier below: a lane's slots of the stacks are its own)
	const uint32_t column = gid, slot = gid; // (a launch of one face at one position: every index is the glyph id)
	const float *factors_all = nullptr;
	if constexpr (CFF2)
		factors_all = face.factors;
#include "charstring_decode.inc"
}

} // namespace

namespace {
uint32_t groups_of(const CharstringsRef &face) { return (face.n_glyph_ids + kLanes - 1) / kLanes; }
} // namespace

extern "C" {

int vgsdf_charstring_count(const CharstringsRef *face, uint32_t *counts, uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids + kLanes - 1) / kLanes;
	hipLaunchKernelGGL((charstring_decode<false, false>), dim3(groups), dim3(kLanes), 0, stream, *face, counts, nullptr, nullptr, nullptr, nullptr, flags);
	return (int)hipGetLastError();
}

int vgsdf_charstring_emit(const CharstringsRef *face, const uint32_t *cmd_off, const uint32_t *dat_off, uint8_t *kinds, float *coords,
                          uint32_t *flags, hipStream_t stream)
{
	const uint32_t groups = (face->n_glyph_ids + kLanes - 1) / kLanes;
	hipLaunchKernelGGL((charstring_decode<true, false>), dim3(groups), dim3(kLanes), 0, stream, *face, nullptr, cmd_off, dat_off, kinds, coords, flags);
	return (int)hipGetLastError();
}

int vgsdf_charstring2_count(const Charstrings2Ref *face, uint32_t *counts, uint32_t *flags, hipStream_t stream)
{
	if (face->spill_stride < groups_of(*face) * kLanes)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL((charstring_decode<false, true>), dim3(groups_of(*face)), dim3(kLanes), 0, stream, *face, counts, nullptr, nullptr,
	                   nullptr, nullptr, flags);
	return (int)hipGetLastError();
}

int vgsdf_charstring2_emit(const Charstrings2Ref *face, const uint32_t *cmd_off, const uint32_t *dat_off, uint8_t *kinds, float *coords,
                           uint32_t *flags, hipStream_t stream)
{
	if (face->spill_stride < groups_of(*face) * kLanes)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL((charstring_decode<true, true>), dim3(groups_of(*face)), dim3(kLanes), 0, stream, *face, nullptr, cmd_off, dat_off,
	                   kinds, coords, flags);
	return (int)hipGetLastError();
}
}
