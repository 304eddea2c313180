// Microbenchmark (tuning aid): the rate at which this GPU issues v_mfma_f32_32x32x16_bf16 from registers, the ceiling that
// DESIGN.md sections 11 and 12 hold the split kernels against.  Every wave runs ITER rounds of 8 independent accumulator tiles (the
// reuse distance of conv_split_kernel's products), operands in registers; 1 or 2 waves per SIMD on every CU; operands all zero or
// pseudo-random bf16 (the matrix cores' power, and with it the clock, depends on the data).  Prints TFLOP/s per case.
//   hipcc --offload-arch=gfx950 -O3 -o mfma_bf16_rate mfma_bf16_rate.hip && ./mfma_bf16_rate
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__global__ void __launch_bounds__(256) mfma_loop(float *out, int iters, uint32_t seed)
{
	const uint32_t id = blockIdx.x * 256 + threadIdx.x;
	uint4 a[2], b[4];
	uint32_t s = seed ? seed * 2654435761u + id * 40503u + 1u : 0u;
	auto next = [&]() -> uint32_t {     // xorshift; the exponent bits are forced into a small range so that nothing overflows
		if (!seed) return 0u;
		s ^= s << 13; s ^= s >> 17; s ^= s << 5;
		return (s & 0x807f807fu) | 0x3c003c00u;
	};
	for (int i = 0; i < 2; ++i) a[i] = make_uint4(next(), next(), next(), next());
	for (int i = 0; i < 4; ++i) b[i] = make_uint4(next(), next(), next(), next());
	floatx16 acc[8];
	for (int t = 0; t < 8; ++t)
		for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
	for (int it = 0; it < iters; ++it) {
#pragma unroll
		for (int t = 0; t < 8; ++t)
			acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[t & 1]), __builtin_bit_cast(bf16x8, b[t >> 1]), acc[t], 0, 0, 0);
	}
	float r = 0.0f;
	for (int t = 0; t < 8; ++t)
		for (int i = 0; i < 16; ++i) r += acc[t][i];
	out[id] = r;
}

int main()
{
	int cus = 0;
	CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
	float *out;
	CK(hipMalloc(&out, (size_t)cus * 2 * 256 * sizeof(float)));
	hipEvent_t e0, e1;
	CK(hipEventCreate(&e0));
	CK(hipEventCreate(&e1));
	const int iters = 20000;
	for (int waves = 1; waves <= 2; ++waves)
		for (uint32_t seed = 0; seed <= 1; ++seed) {
			const int blocks = cus * waves;
			hipLaunchKernelGGL(mfma_loop, dim3(blocks), dim3(256), 0, 0, out, 200, seed);    // warm-up
			float best = 1e30f;
			for (int rep = 0; rep < 3; ++rep) {
				CK(hipEventRecord(e0, 0));
				hipLaunchKernelGGL(mfma_loop, dim3(blocks), dim3(256), 0, 0, out, iters, seed);
				CK(hipEventRecord(e1, 0));
				CK(hipEventSynchronize(e1));
				float ms;
				CK(hipEventElapsedTime(&ms, e0, e1));
				if (ms < best) best = ms;
			}
			const double flop = (double)blocks * 4 * iters * 8 * 32768.0;
			printf("%d CUs, %d wave(s) per SIMD, %s operands: %.3f ms, %.1f TFLOP/s, %.1f cycles per MFMA and SIMD at 2.4 GHz\n", cus, waves,
			       seed ? "pseudo-random" : "zero", best, flop / (best * 1e-3) / 1e12, best * 1e-3 * 2.4e9 / ((double)waves * iters * 8));
		}
	CK(hipFree(out));
	return 0;
}
