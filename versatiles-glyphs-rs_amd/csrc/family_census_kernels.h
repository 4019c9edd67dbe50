// family_census_kernels.h — the census of a font id's cmap tables on the device (family_census_kernels.hip;
// vgsdf_family_tables_census of include/vgsdf.h): a bitmap over the 4352 blocks of 256 code points up to 0x10FFFF, a bit set
// where some unicode subtable lists a code point of the block that is no surrogate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vgsdf {

// one unicode subtable of one face: from its first byte to the END OF THE CMAP TABLE, on the device
struct CensusSubtable {
	uint64_t p;
	uint32_t n;      // bytes from p to the end of the table: the bound of every read
	uint32_t format; // 0 4 6 10 12 13
};
static_assert(sizeof(CensusSubtable) == 16, "one 16-byte record per subtable");

constexpr uint32_t kCensusThreads = 256;
constexpr uint32_t kCensusBlocks = 0x110000u / 256u; // 4352
constexpr uint32_t kCensusWords = kCensusBlocks / 32u; // 136

} // namespace vgsdf

// one workgroup per subtable; bits: kCensusWords zeroed words on the device
extern "C" int vgsdf_family_census_launch(const vgsdf::CensusSubtable *subs, uint32_t n_subtables, uint32_t *bits, hipStream_t stream);
