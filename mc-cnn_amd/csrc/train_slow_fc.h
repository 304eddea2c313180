// The FC stack of the accurate architecture's training step, shared by train_slow.hip (Linear 224 -> 384 x 4 -> 1) and
// train_mb_slow.hip (Linear 224 -> 384 x 3 -> 1): batch GEMMs over the R = 2 * n_pairs rows on v_mfma_f32_16x16x4_f32, one wave
// per 16 x 16 tile; the head (last Linear, Sigmoid, BCECriterion2 and their backward passes); the SGD update.  The kernels
// take their layer by pointer, so the number of hidden Linears is the host's loop count.
// The including file defines MC_FC_HEAD_MAX_ROWS, the most rows (2 * its MAX_PAIRS) the head kernel keeps in LDS.
#pragma once
#include "train_slow_conv.h"

#ifndef MC_FC_HEAD_MAX_ROWS
#error "define MC_FC_HEAD_MAX_ROWS (2 * the library's MAX_PAIRS) before including train_slow_fc.h"
#endif

namespace mc {

constexpr int NH = 384;                  // units per hidden Linear (-nh2)
constexpr int FC_WAVES = 4;              // tiles per workgroup
static_assert(NH % 16 == 0 && NH % 64 == 0, "16 x 16 tiles, 64 bias columns per wave");

// out (R, 384) = ReLU(in (R, K) w (384, K)^T + b).  Both operands are contiguous along K: a lane loads four
// consecutive k as one float4, so K step 4c + j of the instruction sequence is k = 16c + 4 * (lane>>4) + j.
__global__ void __launch_bounds__(FC_WAVES * 64) fc_forward_kernel(const float *__restrict__ in, int K, const float *__restrict__ w,
                                                                   const float *__restrict__ b, float *__restrict__ out, int R)
{
	const int lane = threadIdx.x & 63, kg = lane >> 4, l = lane & 15;
	const int task = blockIdx.x * FC_WAVES + (threadIdx.x >> 6);
	const int ntn = NH / 16;
	if (task >= (R + 15) / 16 * ntn) return;
	const int mt = task / ntn, nt = task - mt * ntn;
	const int row = mt * 16 + l, col = nt * 16 + l;
	const float *pa = in + (int64_t)(row < R ? row : R - 1) * K + 4 * kg;
	const float *pb = w + (int64_t)col * K + 4 * kg;
	floatx4 acc = {0.f, 0.f, 0.f, 0.f};
	for (int c = 0; c < K; c += 16) {
		const float4 a = *(const float4 *)(pa + c), v = *(const float4 *)(pb + c);
		acc = mfma(a.x, v.x, acc);
		acc = mfma(a.y, v.y, acc);
		acc = mfma(a.z, v.z, acc);
		acc = mfma(a.w, v.w, acc);
	}
	const float bias = b[col];
	for (int r = 0; r < 4; ++r) {
		const int orow = mt * 16 + 4 * kg + r;
		if (orow < R) out[(int64_t)orow * NH + col] = fmaxf(acc[r] + bias, 0.f);
	}
}

__device__ __forceinline__ float wave_sum(float v)
{
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// One workgroup, for the last Linear wo (1, 384), bo on the last hidden activations ah (R, 384): z = ah wo + bo,
// o = Sigmoid(z), BCECriterion2 with target r & 1 and its gradient in the reference's operation order (BCECriterion2.lua),
// Sigmoid's backward, then dwo, dbo, the loss and gh = (go wo) masked by ah.
constexpr int HEAD_NT = 1024;
__global__ void __launch_bounds__(HEAD_NT) fc_head_kernel(const float *__restrict__ ah, const float *__restrict__ wo, const float *__restrict__ bo,
                                                          int R, float *__restrict__ gh, float *__restrict__ dwo, float *__restrict__ dbo,
                                                          float *__restrict__ loss_out)
{
	__shared__ float go_[MC_FC_HEAD_MAX_ROWS], term[MC_FC_HEAD_MAX_ROWS];
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const float eps = 1e-12f, n = (float)R;
	for (int r = wave; r < R; r += HEAD_NT / 64) {
		float z = 0.f;
		for (int c = lane; c < NH; c += 64) z += ah[(int64_t)r * NH + c] * wo[c];
		z = wave_sum(z) + bo[0];
		const float o = 1.f / (1.f + expf(-z));
		const float tg = (float)(r & 1);
		const float t1 = 1.f - tg;
		const float t2 = (1.f - o) + eps;
		const float t3 = o + eps;
		if (lane == 0) {
			term[r] = (logf(t3) * tg + logf(t2) * t1) / n;
			const float go = -((tg / t3 - t1 / t2) / n);
			go_[r] = go * ((1.f - o) * o);
		}
	}
	__syncthreads();
	if (t < NH) {
		float s = 0.f;
		for (int r = 0; r < R; ++r) s += go_[r] * ah[(int64_t)r * NH + t];
		dwo[t] = s;
	} else if (t == NH) {
		float s = 0.f;
		for (int r = 0; r < R; ++r) s += go_[r];
		dbo[0] = s;
	} else if (t == NH + 64) {
		float s = 0.f;
		for (int r = 0; r < R; ++r) s += term[r];
		loss_out[0] = -s;
	}
	for (int e = t; e < R * NH; e += HEAD_NT) {
		const int r = e / NH, c = e - r * NH;
		gh[e] = ah[e] > 0.f ? go_[r] * wo[c] : 0.f;
	}
}

// For the hidden Linear w (384, K) with input ap (R, K) and output gradient g (R, 384).  A wave's task is one of
//   data    gp[r, k]  = sum_c g[r, c] w[c, k], masked by ap[r, k] > 0 where MASK   (R x K, summed over c in order)
//   weight  dw[c, k]  = sum_r g[r, c] ap[r, k]                                      (384 x K, summed over the rows in order)
//   bias    db[c]     = sum_r g[r, c]                                               (64 columns per wave)
template <bool MASK>
__global__ void __launch_bounds__(FC_WAVES * 64) fc_backward_kernel(const float *__restrict__ g, const float *__restrict__ ap, int K,
                                                                    const float *__restrict__ w, int R, float *__restrict__ gp,
                                                                    float *__restrict__ dw, float *__restrict__ db)
{
	const int lane = threadIdx.x & 63, kg = lane >> 4, l = lane & 15;
	int task = blockIdx.x * FC_WAVES + (threadIdx.x >> 6);
	const int nkt = K / 16, n_data = (R + 15) / 16 * nkt, n_weight = NH / 16 * nkt, n_bias = NH / 64;
	if (task < n_data) {
		const int mt = task / nkt, nt = task - mt * nkt;
		const int row = mt * 16 + l, col = nt * 16 + l;
		const float *pa = g + (int64_t)(row < R ? row : R - 1) * NH + 4 * kg;
		const float *pb = w + (int64_t)(4 * kg) * K + col;
		floatx4 acc = {0.f, 0.f, 0.f, 0.f};
		for (int c = 0; c < NH; c += 16, pb += 16 * K) {
			const float4 a = *(const float4 *)(pa + c);
			acc = mfma(a.x, pb[0], acc);
			acc = mfma(a.y, pb[K], acc);
			acc = mfma(a.z, pb[2 * K], acc);
			acc = mfma(a.w, pb[3 * K], acc);
		}
		for (int r = 0; r < 4; ++r) {
			const int orow = mt * 16 + 4 * kg + r;
			if (orow < R) {
				const int64_t e = (int64_t)orow * K + col;
				gp[e] = !MASK || ap[e] > 0.f ? acc[r] : 0.f;
			}
		}
		return;
	}
	task -= n_data;
	if (task < n_weight) {
		const int mt = task / nkt, nt = task - mt * nkt;
		const int m = mt * 16 + l, col = nt * 16 + l;
		floatx4 acc = {0.f, 0.f, 0.f, 0.f};
		for (int r0 = 0; r0 < R; r0 += 4) {
			const int r = r0 + kg;
			const float a = r < R ? g[(int64_t)r * NH + m] : 0.f;
			const float v = r < R ? ap[(int64_t)r * K + col] : 0.f;
			acc = mfma(a, v, acc);
		}
		for (int r = 0; r < 4; ++r) dw[(int64_t)(mt * 16 + 4 * kg + r) * K + col] = acc[r];
		return;
	}
	task -= n_weight;
	if (task < n_bias) {
		const int c = task * 64 + lane;
		float s = 0.f;
		for (int r = 0; r < R; ++r) s += g[(int64_t)r * NH + c];
		db[c] = s;
	}
}

// Parameter j's update: the convolutions' gradient is the slab's n_rows rows of n_conv floats summed in row order, the FC
// stack's is gfc as it is; v = mom * v - lr * g; w += v.
__device__ __forceinline__ void sgd_update(int j, const float *__restrict__ slab, const float *__restrict__ gfc, int n_rows, int n_conv,
                                           float *__restrict__ params, float *__restrict__ moms, float lr, float mom)
{
	float g;
	if (j < n_conv) {
		g = 0.f;
		for (int p = 0; p < n_rows; ++p) g += slab[(int64_t)p * n_conv + j];
	} else {
		g = gfc[j - n_conv];
	}
	const float v = moms[j] * mom - lr * g;
	moms[j] = v;
	params[j] = params[j] + v;
}

}  // namespace mc
