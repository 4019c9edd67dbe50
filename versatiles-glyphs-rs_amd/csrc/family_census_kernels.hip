// family_census_kernels.hip — which of the 4352 blocks of 256 code points a font id's faces LIST (family_census_kernels.h;
// vgsdf_family_tables_census of include/vgsdf.h): the caller of vgsdf_family_create_tables_at has not parsed cmap and learns
// here which planes are worth a family.  Bit b of the bitmap is set exactly when some unicode subtable lists a code point c of
// [256 b, 256 b + 255] that is no surrogate and at most 0x10FFFF, where a subtable lists
//   format 0        c < 256, when the table has its 262 bytes
//   format 4        its segments [start, end], less a closing segment 0xFFFF - 0xFFFF
//   formats 6, 10   [first, first + count - 1]
//   formats 12, 13  its groups
// A listed code point may have no value: a set bit promises nothing, a clear bit that the block maps nothing.
// One workgroup per subtable; its lanes stride over the segments / groups, and a lane ORs its span into the bitmap with atomics
// on global memory, whole 32-bit words where the span covers them.  Every read is bounded by the bytes from the subtable to the end
// of the cmap table, as in the lookup of family_table_kernels.hip; every word index is at most 135 by the cut at 0x10FFFF.
#include "family_census_kernels.h"

namespace vgsdf {
namespace {

__device__ inline bool has(const CensusSubtable &d, uint64_t off, uint64_t len) { return off <= d.n && len <= d.n - off; }
__device__ inline uint32_t be16(const uint8_t *p) { return ((uint32_t)p[0] << 8) | p[1]; }
__device__ inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// the blocks of [a, b], a <= b <= 0x10FFFF, none of it a surrogate
__device__ void or_blocks(uint32_t *bits, uint32_t a, uint32_t b)
{
	const uint32_t lo = a >> 8, hi = min(b >> 8, kCensusBlocks - 1u);
	if (lo > hi)
		return;
	const uint32_t w0 = lo >> 5, w1 = hi >> 5;
	const uint32_t head = 0xFFFFFFFFu << (lo & 31u), tail = 0xFFFFFFFFu >> (31u - (hi & 31u));
	if (w0 == w1) {
		atomicOr(bits + w0, head & tail);
		return;
	}
	atomicOr(bits + w0, head);
	for (uint32_t w = w0 + 1; w < w1; w++)
		atomicOr(bits + w, 0xFFFFFFFFu);
	atomicOr(bits + w1, tail);
}

// a listed span [a, b] as the table states it: cut at 0x10FFFF, and what lies on either side of the surrogates
__device__ void or_span(uint32_t *bits, uint64_t a, uint64_t b)
{
	if (a > b || a > 0x10FFFFull)
		return;
	const uint32_t lo = (uint32_t)a, hi = (uint32_t)(b < 0x10FFFFull ? b : 0x10FFFFull);
	if (lo < 0xD800u)
		or_blocks(bits, lo, hi < 0xD7FFu ? hi : 0xD7FFu);
	if (hi > 0xDFFFu)
		or_blocks(bits, lo > 0xE000u ? lo : 0xE000u, hi);
}

__global__ __launch_bounds__(kCensusThreads) void family_census(const CensusSubtable *subs, uint32_t *bits)
{
	const CensusSubtable d = subs[blockIdx.x];
	const uint8_t *p = (const uint8_t *)(uintptr_t)d.p;
	const uint32_t tid = threadIdx.x;
	switch (d.format) {
	case 0:
		if (tid == 0 && has(d, 6, 256))
			or_span(bits, 0, 255);
		break;
	case 4: {
		if (!has(d, 0, 14))
			break;
		const uint32_t x2 = be16(p + 6);
		if (x2 < 2)
			break;
		const uint32_t segs = x2 / 2, ends = 14, starts = ends + segs * 2 + 2, offsets = starts + segs * 4;
		if (!has(d, offsets, segs * 2))
			break;
		for (uint32_t s = tid; s < segs; s += kCensusThreads) {
			const uint32_t a = be16(p + starts + s * 2), b = be16(p + ends + s * 2);
			if (!(a == 0xFFFFu && b == 0xFFFFu))
				or_span(bits, a, b);
		}
		break;
	}
	case 6:
		if (tid == 0 && has(d, 0, 10) && be16(p + 8) != 0)
			or_span(bits, be16(p + 6), (uint64_t)be16(p + 6) + be16(p + 8) - 1u);
		break;
	case 10:
		if (tid == 0 && has(d, 0, 20) && be32(p + 16) != 0)
			or_span(bits, be32(p + 12), (uint64_t)be32(p + 12) + be32(p + 16) - 1u);
		break;
	case 12:
	case 13: {
		if (!has(d, 0, 16))
			break;
		const uint32_t n = be32(p + 12);
		if (!has(d, 16, (uint64_t)n * 12))
			break;
		for (uint32_t k = tid; k < n; k += kCensusThreads) {
			const uint8_t *g = p + 16 + (size_t)k * 12;
			or_span(bits, be32(g), be32(g + 4));
		}
		break;
	}
	default:
		break;
	}
}

} // namespace
} // namespace vgsdf

extern "C" int vgsdf_family_census_launch(const vgsdf::CensusSubtable *subs, uint32_t n_subtables, uint32_t *bits, hipStream_t stream)
{
	if (n_subtables == 0)
		return (int)hipSuccess;
	hipLaunchKernelGGL(vgsdf::family_census, dim3(n_subtables), dim3(vgsdf::kCensusThreads), 0, stream, subs, bits);
	return (int)hipGetLastError();
}
