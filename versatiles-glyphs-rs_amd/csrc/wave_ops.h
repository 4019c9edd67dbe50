// wave_ops.h — the two wave-wide scans that more than one kernel file of the front-end uses (outline_kernels.hip,
// input_form_kernels.hip).  The raster's scans (sdf_span_support.h) are a different family and stay there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vgsdf {

// exclusive prefix sum over the wave (DPP row shifts + row broadcasts); total = sum over all lanes
__device__ __forceinline__ uint32_t wave_exclusive_sum(uint32_t v, uint32_t &total)
{
	uint32_t incl = v;
	incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xF, 0xF, false); // row_shr:1
	incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xF, 0xF, false); // row_shr:2
	incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xF, 0xF, false); // row_shr:4
	incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xF, 0xF, false); // row_shr:8
	incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1, 3
	incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2, 3
	total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
	return incl - v;
}

// inclusive running maximum over the wave
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v)
{
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = (uint32_t)__shfl_up((int)v, d);
		if ((int)(threadIdx.x & 63u) >= d)
			v = max(v, o);
	}
	return v;
}

} // namespace vgsdf
