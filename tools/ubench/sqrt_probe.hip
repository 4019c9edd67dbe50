// sqrt_probe: the raw v_sqrt_f32 (__builtin_amdgcn_sqrtf) against the correctly rounded __builtin_sqrtf over EVERY non-negative
// finite f32 bit pattern (0 .. 0x7F7FFFFF, 2^31 - 2^23 inputs), as the span kernel's bounds use it (U, the
// group radius and the decide step's sq take the raw instruction; each feeds a bound with an explicit margin).
// Build with the product's floating-point flags (-O3 -ffp-contract=off -fno-fast-math): they decide what __builtin_sqrtf is.
// Prints, for the normal inputs: how many results differ and the largest distance in ulps (units of the correctly rounded
// result's last place), its sign split (raw below / above) and one input where it occurs; for the denormal inputs
// (0x00000001 .. 0x007FFFFF): how many return exactly 0, and the largest ulp distance among the others; and sqrt(+0).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

struct Result {
	unsigned long long differ, below, above, den_zero, den_differ;
	unsigned int max_ulp, max_at, den_max_ulp, den_max_at, zero_bits, pad;
};

__global__ __launch_bounds__(256) void probe(Result *out)
{
	const uint32_t n_threads = gridDim.x * blockDim.x, t = blockIdx.x * blockDim.x + threadIdx.x;
	unsigned long long differ = 0, below = 0, above = 0, den_zero = 0, den_differ = 0;
	uint32_t max_ulp = 0, max_at = 0, den_max_ulp = 0, den_max_at = 0;
	for (uint64_t b = t; b <= 0x7F7FFFFFull; b += n_threads) {
		const float x = __uint_as_float((uint32_t)b);
		const uint32_t raw = __float_as_uint(__builtin_amdgcn_sqrtf(x)), ref = __float_as_uint(__builtin_sqrtf(x));
		// both results are non-negative floats (or the raw one a NaN, which then counts as a huge distance): bits order like values
		const uint32_t d = raw > ref ? raw - ref : ref - raw;
		if (b == 0) {
			out->zero_bits = raw;
		} else if (b < 0x00800000ull) {
			if (raw == 0)
				den_zero++;
			else {
				den_differ += d != 0;
				if (d > den_max_ulp) {
					den_max_ulp = d;
					den_max_at = (uint32_t)b;
				}
			}
		} else {
			differ += d != 0;
			below += raw < ref;
			above += raw > ref;
			if (d > max_ulp) {
				max_ulp = d;
				max_at = (uint32_t)b;
			}
		}
	}
	atomicAdd(&out->differ, differ);
	atomicAdd(&out->below, below);
	atomicAdd(&out->above, above);
	atomicAdd(&out->den_zero, den_zero);
	atomicAdd(&out->den_differ, den_differ);
	if (atomicMax(&out->max_ulp, max_ulp) < max_ulp)
		out->max_at = max_at; // (any input at the largest distance will do)
	if (atomicMax(&out->den_max_ulp, den_max_ulp) < den_max_ulp)
		out->den_max_at = den_max_at;
}

int main()
{
	Result *d = nullptr, h = {};
	if (hipMalloc(&d, sizeof(Result)) != hipSuccess || hipMemset(d, 0, sizeof(Result)) != hipSuccess) {
		std::fprintf(stderr, "sqrt_probe: no device memory\n");
		return 2;
	}
	probe<<<256 * 16, 256>>>(d);
	if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&h, d, sizeof(Result), hipMemcpyDeviceToHost) != hipSuccess) {
		std::fprintf(stderr, "sqrt_probe: the kernel failed\n");
		return 2;
	}
	std::printf("inputs: every f32 bit pattern 0x00000000 .. 0x7F7FFFFF; raw = v_sqrt_f32, ref = correctly rounded sqrtf\n");
	std::printf("normal inputs: %llu of %llu differ (raw below ref: %llu, above: %llu); max distance %u ulp (at input 0x%08X)\n", h.differ,
	            0x7F7FFFFFull - 0x00800000ull + 1, h.below, h.above, h.max_ulp, h.max_at);
	std::printf("denormal inputs: %llu of %llu return exactly 0; of the others %llu differ, max distance %u ulp (at input 0x%08X)\n", h.den_zero,
	            0x007FFFFFull, h.den_differ, h.den_max_ulp, h.den_max_at);
	std::printf("sqrt(+0): raw bits 0x%08X\n", h.zero_bits);
	std::printf("RESULT max_ulp=%u differ=%llu den_zero=%llu den_max_ulp=%u zero_bits=0x%08X\n", h.max_ulp, h.differ, h.den_zero, h.den_max_ulp,
	            h.zero_bits);
	(void)hipFree(d);
	return 0;
}
