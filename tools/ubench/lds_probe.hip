// lds_probe: what an LDS round trip costs a wave, and what the LDS counters count.  The span kernel's sweep (csrc/sdf_span_kernel.inc)
// issues ds_read_b128 whose results the next instructions need; DESIGN.md §4.1 "What the wave waits for" uses these figures.
//   chain     ONE wave follows a dependent chain of ds_read_b128 (every address comes out of the read before it) on an otherwise
//             idle CU: shader cycles per round trip
//   loaded    the same chain while the other 15 waves of its 1024-thread workgroup (16 waves on the CU, as the product kernel
//             keeps) stream independent conflict-free ds_read_b128
//   stream S  16 waves stream independent ds_read_b128 with a lane stride of S = 16, 32, 64 bytes (conflict-free, 2-way, 4-way):
//             cycles per instruction and CU, and, under `rocprofv3 --pmc SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT`
//             (counters only, a run of its own), what the counters show per instruction: the probe prints every kernel's
//             instruction count for that division
// One workgroup on one CU throughout; times are d(s_memtime) in shader cycles, the clock from d(s_memrealtime) (100 MHz).
// Output: profiles/lds_probe.txt.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

constexpr int WORDS4 = 2048;      // 32 KiB of uint4
constexpr int CHAIN = 4096;       // dependent reads of the chain wave
constexpr int STREAM_ITERS = 2048; // x 8 independent reads per streaming wave

// stamps: per wave (cycles, realtime ticks, start, end)
template <int STRIDE, bool WITH_CHAIN, bool WITH_STREAM>
__global__ __launch_bounds__(1024) void probe(unsigned long long *stamps, uint32_t *sink)
{
	__shared__ uint4 lds[WORDS4];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	// element i holds the byte address of element (i + 64) % WORDS4: a lane's chain visits every 64th element, the 64 lanes of
	// a step read 64 consecutive elements (conflict-free)
	for (uint32_t i = threadIdx.x; i < WORDS4; i += blockDim.x)
		lds[i] = make_uint4(((i + 64) % WORDS4) * 16u, i, i * 3u, i * 5u);
	__syncthreads();
	uint32_t acc = 0;
	const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
	if (WITH_CHAIN && wave == 0) {
		uint32_t addr = lane * 16u;
#pragma unroll 8
		for (int i = 0; i < CHAIN; i++) {
			const uint4 v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(lds) + addr);
			addr = v.x;
			acc += v.y ^ v.z ^ v.w; // (all four words are used: the read stays a ds_read_b128)
		}
	} else if (WITH_STREAM) {
		// 8 independent reads per trip; lane stride STRIDE bytes, the window moved every trip (mask keeps it inside the array)
		uint32_t base = (lane * (uint32_t)STRIDE + wave * 1024u) & (WORDS4 * 16u - 1u);
		for (int i = 0; i < STREAM_ITERS; i++) {
			uint4 v[8];
#pragma unroll
			for (int j = 0; j < 8; j++)
				v[j] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(lds) + ((base + (uint32_t)j * 4096u) & (WORDS4 * 16u - 1u)));
#pragma unroll
			for (int j = 0; j < 8; j++)
				acc += v[j].x ^ v[j].y ^ v[j].z ^ v[j].w;
			base = (base + 16u * 64u) & (WORDS4 * 16u - 1u);
			asm volatile("" : "+v"(base)); // (the addresses stay a run-time value: the reads are issued every trip)
		}
	}
	const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
	if (acc == 0xDEADBEEFu)
		sink[threadIdx.x] = acc;
	if (lane == 0) {
		stamps[4 * wave] = t1 - t0;
		stamps[4 * wave + 1] = r1 - r0;
		stamps[4 * wave + 2] = t0;
		stamps[4 * wave + 3] = t1;
	}
}

template <typename K> static bool run(const char *name, K kernel, int threads, unsigned long long *d, uint32_t *sink, bool chain, bool stream)
{
	std::vector<unsigned long long> h(4 * 16);
	for (int rep = 0; rep < 3; rep++) { // the last launch is reported (the first loads the code object)
		hipLaunchKernelGGL(kernel, dim3(1), dim3(threads), 0, 0, d, sink);
		if (hipDeviceSynchronize() != hipSuccess) {
			std::fprintf(stderr, "lds_probe: launch failed (%s)\n", name);
			return false;
		}
	}
	if (hipMemcpy(h.data(), d, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
		return false;
	const int waves = threads / 64;
	const double mhz = h[1] ? (double)h[0] / (double)h[1] * 100.0 : 0.0;
	std::printf("%-10s %2d waves, shader clock %.0f MHz:", name, waves, mhz);
	if (chain)
		std::printf("  chain wave: %d dependent ds_read_b128 in %llu cycles = %.1f cycles per round trip", CHAIN, h[0], (double)h[0] / CHAIN);
	if (stream) {
		unsigned long long first_end = ~0ull, last_end = 0, first_start = ~0ull;
		const int w0 = chain ? 1 : 0;
		for (int w = w0; w < waves; w++) {
			first_start = h[4 * w + 2] < first_start ? h[4 * w + 2] : first_start;
			first_end = h[4 * w + 3] < first_end ? h[4 * w + 3] : first_end;
			last_end = h[4 * w + 3] > last_end ? h[4 * w + 3] : last_end;
		}
		const double n = (double)(waves - w0) * STREAM_ITERS * 8;
		std::printf("  %d streaming waves: %.0f ds_read_b128 in %llu cycles = %.2f cycles per instruction and CU", waves - w0, n,
		            last_end - first_start, (double)(last_end - first_start) / n);
		if (chain)
			std::printf("  (the chain ended %s the first streaming wave did)", h[3] <= first_end ? "before" : "AFTER");
	}
	std::printf("\n            LDS instructions of the launch (wave64): %.0f ds_read_b128 + %d ds_write_b128\n",
	            (chain ? (double)CHAIN : 0.0) + (stream ? (double)(waves - (chain ? 1 : 0)) * STREAM_ITERS * 8 : 0.0), WORDS4 / 64);
	return true;
}

int main()
{
	unsigned long long *d;
	uint32_t *sink;
	if (hipMalloc(&d, sizeof(unsigned long long) * 4 * 16) != hipSuccess || hipMalloc(&sink, sizeof(uint32_t) * 1024) != hipSuccess) {
		std::fprintf(stderr, "lds_probe: no device memory\n");
		return 1;
	}
	bool ok = run("chain", probe<16, true, false>, 64, d, sink, true, false);
	ok = ok && run("loaded", probe<16, true, true>, 1024, d, sink, true, true);
	ok = ok && run("stream 16", probe<16, false, true>, 1024, d, sink, false, true);
	ok = ok && run("stream 32", probe<32, false, true>, 1024, d, sink, false, true);
	ok = ok && run("stream 64", probe<64, false, true>, 1024, d, sink, false, true);
	(void)hipFree(d);
	(void)hipFree(sink);
	return ok ? 0 : 1;
}
