// libmcops.so (include/mc_ops.h): Normalize_backward_input (adcensus.cu:1335-1377).
//
// Every expression is the reference's, operation for operation, with fmaf() where the reference's build contracts
// (`norm - x * x`, `sum += x * g`, `deriv - q` whose deriv is a product) and nowhere else.  THIS FILE ALONE IS BUILT WITH
// -ffp-contract=fast (FLAGS_ops_normalize in the Makefile), for powf: the compiler inlines the device library's powf and, where
// fusion is allowed, contracts multiply-add pairs inside it, so powf(norm, 1.5f) of a -ffp-contract=off build differs from the
// reference's in the last bits (seen on the GPU: 115 of 192 results of the training shape).  Fusion is a per-file switch.  Outside
// powf the file has no floating-point product that feeds a sum or difference except through fmaf(): `sum * x / denom` feeds a
// division, so the switch changes nothing else.  -fno-slp-vectorize as the reference's build, so that powf's body meets the
// same instruction selection.
//
// The sum of an element leaves out the element's own channel, so the C channels of a pixel need C different sums of C - 1 terms
// in ascending order; no sum can be derived from another without changing its rounding.  The reference re-reads both tensors
// from global memory for each of them.  Here a workgroup of NB_WAVES waves takes NB_TP pixels (one per lane), stages all C
// channels of `input` and `grad_output` of those pixels in LDS once, and each wave then walks the channels for NB_CH outputs at
// a time: two LDS reads feed NB_CH fused multiply-adds.  Lanes are consecutive pixels, so the global accesses coalesce wherever
// H * W > 1 and the LDS accesses are conflict-free.
#include "mc_common.h"
#include "../../include/mc_ops.h"

namespace mc {

constexpr int NB_TP = 64;                  // pixels of a normalize-backward workgroup: one per lane
constexpr int NB_WAVES = 8;                // C = 64 is one sweep per wave
constexpr int NB_CH = 8;                   // output channels per wave and sweep over the staged channels
static_assert(2 * MC_OPS_MAX_C * NB_TP * sizeof(float) <= 65536, "a tile of both tensors has to fit in 64 KiB of LDS");

__global__ __launch_bounds__(NB_TP *NB_WAVES) void normalize_backward_kernel(const float *__restrict__ go, const float *__restrict__ in,
                                                                             const float *__restrict__ norm, float *__restrict__ gi, int C,
                                                                             int64_t HW, int64_t NP)
{
	extern __shared__ float tile[];          // [2][C][NB_TP]
	float *sx = tile, *sg = tile + C * NB_TP;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t q = (int64_t)blockIdx.x * NB_TP + lane;   // pixel (n, p) = n * HW + p
	const bool live = q < NP;
	const int64_t n = live ? q / HW : 0;
	const int64_t base = n * C * HW + (live ? q - n * HW : 0);   // element (n, 0, p); channel c lies c * HW further
	for (int c = wave; c < C; c += NB_WAVES) {
		float x = 0.f, g = 0.f;
		if (live) {
			x = in[base + c * HW];
			g = go[base + c * HW];
		}
		sx[c * NB_TP + lane] = x;
		sg[c * NB_TP + lane] = g;
	}
	const float nrm = live ? norm[q] : 1.f;  // requested before the barrier, so that its latency passes behind the staging
	__syncthreads();                         // the only barrier: a lane without a pixel may leave now
	if (!live) return;
	const float denom = powf(nrm, 1.5f);
	for (int cb = wave * NB_CH; cb < C; cb += NB_WAVES * NB_CH) {
		const int ce = min(cb + NB_CH, C);
		float sum[NB_CH];
#pragma unroll
		for (int k = 0; k < NB_CH; ++k) sum[k] = 0.f;
#pragma unroll 4
		for (int c = 0; c < cb; ++c) {       // channels below this sweep's outputs: a term of every sum (unrolled: LDS reads in batches)
			const float x = sx[c * NB_TP + lane], g = sg[c * NB_TP + lane];
#pragma unroll
			for (int k = 0; k < NB_CH; ++k) sum[k] = fmaf(x, g, sum[k]);
		}
		for (int c = cb; c < ce; ++c) {      // the outputs' own channels: each sum skips its own
			const float x = sx[c * NB_TP + lane], g = sg[c * NB_TP + lane];
#pragma unroll
			for (int k = 0; k < NB_CH; ++k) sum[k] = c == cb + k ? sum[k] : fmaf(x, g, sum[k]);
		}
#pragma unroll 4
		for (int c = ce; c < C; ++c) {
			const float x = sx[c * NB_TP + lane], g = sg[c * NB_TP + lane];
#pragma unroll
			for (int k = 0; k < NB_CH; ++k) sum[k] = fmaf(x, g, sum[k]);
		}
#pragma unroll
		for (int k = 0; k < NB_CH; ++k) {
			const int c = cb + k;
			if (c < C) {
				const float x = sx[c * NB_TP + lane], g = sg[c * NB_TP + lane];
				const float d = fmaf(-x, x, nrm) / denom;        // (norm - input * input) / denom, to be multiplied by grad_output
				const float s = sum[k] * x / denom;
				gi[base + c * HW] = fmaf(d, g, -s);              // deriv - sum * input / denom
			}
		}
	}
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_normalize_backward_input(const float *grad_output, const float *input, const float *norm, float *grad_input, int N, int C, int H, int W,
                                void *stream)
{
	MC_REQUIRE(grad_output && input && norm && grad_input, "mc_normalize_backward_input: null pointer (grad_output %p, input %p, norm %p, grad_input %p)",
	           (const void *)grad_output, (const void *)input, (const void *)norm, (void *)grad_input);
	MC_REQUIRE(C >= 1 && C <= MC_OPS_MAX_C, "mc_normalize_backward_input: C %d outside [1, %d]", C, MC_OPS_MAX_C);
	MC_REQUIRE(N >= 1 && H >= 1 && W >= 1, "mc_normalize_backward_input: bad dims %d x %d x %d x %d", N, C, H, W);
	MC_REQUIRE((int64_t)N * H * W < ((int64_t)1 << 40) / C, "mc_normalize_backward_input: %d x %d x %d x %d is 2^40 elements or more", N, C, H, W);
	const int64_t HW = (int64_t)H * W, NP = (int64_t)N * HW;
	MC_REQUIRE((NP + NB_TP - 1) / NB_TP < ((int64_t)1 << 31), "mc_normalize_backward_input: %lld pixels are too many for one launch", (long long)NP);
	const size_t lds = 2 * (size_t)C * NB_TP * sizeof(float);
	hipLaunchKernelGGL(normalize_backward_kernel, dim3((unsigned)((NP + NB_TP - 1) / NB_TP)), dim3(NB_TP * NB_WAVES), lds, as_stream(stream),
	                   grad_output, input, norm, grad_input, C, HW, NP);
	return check_launch("mc_normalize_backward_input");
}

}  // extern "C"
