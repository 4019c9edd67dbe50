// charstring_limits.h — the limits of the Type 2 charstring interpreter that its two statements share: the host reader
// (host/cff.cpp, CharStringRun: the statement of behaviour) and the device decoder (charstring_kernels.hip), which must
// equal it bit for bit.
#pragma once
#include <cstdint>

namespace vg {

constexpr int kCharstringMaxOperands = 48; // ttf-parser: MAX_ARGUMENTS_STACK_LEN of cff1
constexpr int kCharstringMaxOperands2 = 513; // ttf-parser: MAX_ARGUMENTS_STACK_LEN of cff2
constexpr int kCharstringWindow = 48; // device: slots of the operand stack kept in LDS; CFF2's further slots live in global memory
constexpr int kCharstringMaxRegions = 64; // ttf-parser: scalars of one ItemVariationData (cff2), the factors of one blend set
constexpr int kCharstringMaxDepth = 10;    // ttf-parser: STACK_LIMIT (nested subroutine calls)
// Technical Note #5176, section 16: the bias added to a subroutine operand, by the number of subroutines of the set
constexpr uint32_t charstring_subr_bias(uint32_t n) { return n < 1240 ? 107 : (n < 33900 ? 1131 : 32768); }

} // namespace vg
