// simd_probe: on which SIMD of its CU does wave i of a 256-thread workgroup run?  The span kernel's sweep gives the four waves
// of a workgroup unequal work by wave index (tools/model_wave_shares.py); that matters only if wave i of every workgroup
// lands on the same SIMD.  The probe launches workgroups shaped like the product kernel's (256 threads, 4 waves per SIMD,
// 4 workgroups per CU, a grid of 3023, a few microseconds of VALU work each so that several generations of workgroups pass
// through every CU) and lane 0 of every wave records HW_REG_HW_ID and HW_REG_XCC_ID.
// Output: the 4 x 4 table wave index x SIMD id, the SIMD of wave 0 (over the grid and per CU), the order in which a workgroup's
// waves are placed, and the share of workgroups whose four waves sit on four distinct SIMDs (profiles/simd_placement.txt).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

constexpr int GRID = 3023, TPB = 256, WAVES = TPB / 64;
constexpr int LDS_WORDS = 33 * 256; // 33 KiB: 4 workgroups per CU, as the product (31 KB of LDS, but 4 by its 125 VGPRs: this kernel needs few)

__global__ __launch_bounds__(TPB, 4) void probe(uint2 *rec, float *sink, int iters, float a, float b)
{
	__shared__ float lds[LDS_WORDS];
	const uint32_t hw = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_REG_HW_ID, all 32 bits
	const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20); // HW_REG_XCC_ID
	for (int i = threadIdx.x; i < LDS_WORDS; i += TPB)
		lds[i] = (float)i;
	__syncthreads();
	float x = lds[(threadIdx.x * 31) % LDS_WORDS];
	for (int i = 0; i < iters; i++)
		x = __builtin_fmaf(x, a, b);
	if (x == 12345.678f) // never: keeps the loop and the LDS alive
		sink[threadIdx.x] = x;
	if ((threadIdx.x & 63) == 0)
		rec[blockIdx.x * WAVES + (threadIdx.x >> 6)] = make_uint2(hw, xcc);
}

int main()
{
	uint2 *d;
	float *sink;
	if (hipMalloc(&d, sizeof(uint2) * GRID * WAVES) != hipSuccess || hipMalloc(&sink, sizeof(float) * TPB) != hipSuccess) {
		std::fprintf(stderr, "simd_probe: no device memory\n");
		return 1;
	}
	std::vector<uint2> h(GRID * WAVES);
	for (int rep = 0; rep < 3; rep++) { // the last launch is reported (the first loads the code object)
		hipLaunchKernelGGL(probe, dim3(GRID), dim3(TPB), 0, 0, d, sink, 2000, 1.0001f, 0.5f);
		if (hipDeviceSynchronize() != hipSuccess) {
			std::fprintf(stderr, "simd_probe: launch failed\n");
			return 1;
		}
	}
	if (hipMemcpy(h.data(), d, sizeof(uint2) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
		return 1;

	// HW_ID (gfx9): wave_id [3:0], simd_id [5:4], pipe_id [7:6], cu_id [11:8], sh_id [12], se_id [15:13]
	auto simd = [](uint32_t hw) { return (hw >> 4) & 3u; };
	auto cu = [](uint2 r) { return ((r.y & 15u) << 8) | ((r.x >> 8) & 0xFFu); }; // XCC : SE : SH : CU
	unsigned table[WAVES][4] = {}, start[4] = {}, distinct = 0, same_cu = 0;
	std::map<uint32_t, unsigned> orders;
	std::map<uint32_t, std::vector<unsigned>> wg_of_cu;
	for (int b = 0; b < GRID; b++) {
		uint32_t seen = 0, order = 0;
		bool one_cu = true;
		for (int w = 0; w < WAVES; w++) {
			const uint2 r = h[b * WAVES + w];
			table[w][simd(r.x)]++;
			seen |= 1u << simd(r.x);
			order = order * 10 + ((simd(r.x) - simd(h[b * WAVES].x)) & 3u); // SIMDs relative to wave 0's
			one_cu = one_cu && cu(r) == cu(h[b * WAVES]);
		}
		start[simd(h[b * WAVES].x)]++;
		distinct += seen == 0xFu;
		same_cu += one_cu;
		orders[order]++;
		wg_of_cu[cu(h[b * WAVES])].push_back((unsigned)b);
	}
	std::printf("simd_probe: %d workgroups of %d threads, __launch_bounds__(%d, 4), %d B of static LDS\n", GRID, TPB, TPB, LDS_WORDS * 4);
	std::printf("waves by wave index (rows) and SIMD id (columns)\n          SIMD0  SIMD1  SIMD2  SIMD3\n");
	for (int w = 0; w < WAVES; w++)
		std::printf("  wave %d  %5u  %5u  %5u  %5u\n", w, table[w][0], table[w][1], table[w][2], table[w][3]);
	std::printf("workgroups whose four waves sit on four distinct SIMDs: %u of %d (%.1f %%); on one CU: %u\n", distinct, GRID,
	            100.0 * distinct / GRID, same_cu);
	std::printf("SIMD of wave 0: %u %u %u %u\n", start[0], start[1], start[2], start[3]);
	std::printf("SIMDs of waves 0..3 relative to wave 0's (digits), workgroups:");
	for (auto &o : orders)
		std::printf("  %04u: %u", o.first, o.second);
	std::printf("\n");
	// the workgroups one CU ran, in index order: do their indices share low bits (of b / 8, the index inside the XCD)?
	unsigned n_cu = 0, eq2 = 0, pairs = 0;
	for (auto &c : wg_of_cu) {
		n_cu++;
		for (size_t i = 1; i < c.second.size(); i++) {
			pairs++;
			eq2 += ((c.second[i] >> 3) & 3u) == ((c.second[i - 1] >> 3) & 3u);
		}
	}
	// per CU: is the SIMD of wave 0 the same for all the workgroups the CU ran (then wave i WOULD share a SIMD per CU)?
	unsigned by_distinct[5] = {};
	double top_share = 0;
	for (auto &c : wg_of_cu) {
		unsigned n[4] = {}, top = 0, kinds = 0;
		for (unsigned b : c.second)
			n[simd(h[b * WAVES].x)]++;
		for (int i = 0; i < 4; i++) {
			kinds += n[i] != 0;
			top = n[i] > top ? n[i] : top;
		}
		by_distinct[kinds]++;
		top_share += (double)top / c.second.size();
	}
	std::printf("CUs by the number of distinct SIMDs their workgroups' wave 0 ran on: 1: %u  2: %u  3: %u  4: %u; commonest SIMD of a CU: "
	            "%.1f %% of its workgroups (25 %% = even)\n", by_distinct[1], by_distinct[2], by_distinct[3], by_distinct[4], 100.0 * top_share / n_cu);
	std::printf("CUs seen: %u (%.1f workgroups each); consecutive workgroups of one CU with equal bits [4:3] of blockIdx: %u of %u (%.1f %%)\n",
	            n_cu, (double)GRID / n_cu, eq2, pairs, pairs ? 100.0 * eq2 / pairs : 0.0);
	(void)hipFree(d);
	(void)hipFree(sink);
	return 0;
}
