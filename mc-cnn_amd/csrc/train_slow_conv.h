// The convolution GEMMs of the accurate architecture's training step on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate;
// 112 = 7 x 16 rows fill its tiles exactly), shared by train_slow.hip (four layers on 9 x 9 patches, a PAIR's three patches per
// workgroup: NP = 3) and train_mb_slow.hip (five layers on 11 x 11 patches, ONE patch per workgroup: NP = 1).  112 feature
// maps, every activation of the workgroup's NP patches in LDS as [NP][112][pixels], one workgroup of eight waves.  Then the
// towers' layer chain over a net N of train_net.h, and where a patch's features sit in the FC stack's input.
#pragma once
#include "mc_common.h"
#include "train_net.h"

namespace mc {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int FM = 112;                  // feature maps per convolution (MC_TRAIN_SLOW_FM, MC_TRAIN_MB_SLOW_FM)
constexpr int NW = 8;                    // waves per tower workgroup (two per SIMD)
constexpr int NT = NW * 64;
static_assert(FM % 16 == 0, "16 x 16 tiles");

__device__ __forceinline__ floatx4 mfma(float a, float b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---- the tower: block GEMMs of (M = 112) x N over the workgroup's waves ------------------------------------------------
// Tiles of 16 x 16; a lane holds A[row lane&15][k = lane>>4] and B[k = lane>>4][col lane&15]; its result register r is row
// 4 * (lane>>4) + r of column lane&15.
// mac(acc, i, j, kg): every K step for output row i / column j on lane group kg.  out(row, col, v): one element's epilogue.
template <class Mac, class Out>
__device__ __forceinline__ void block_gemm(int N, Mac mac, Out out)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kg = lane >> 4, l = lane & 15;
	const int ntile = (FM / 16) * ((N + 15) / 16);
	for (int task = wave; task < ntile; task += NW) {
		const int mt = task % (FM / 16), nt = task / (FM / 16);
		floatx4 acc = {0.f, 0.f, 0.f, 0.f};
		mac(acc, mt * 16 + l, nt * 16 + l, kg);
		const int col = nt * 16 + l;
		if (col < N)
			for (int r = 0; r < 4; ++r) out(mt * 16 + 4 * kg + r, col, acc[r]);
	}
}

// forward of a layer with CIN input maps of SI x SI per patch into FM maps of (SI-2)^2: out = ReLU(b + W * in)
template <int NP, int CIN, int SI>
__device__ void conv_forward(const float *__restrict__ w, const float *__restrict__ bias, const float *in, float *out)
{
	constexpr int SO = SI - 2, PO = SO * SO, PI = SI * SI, N = NP * PO;
	auto mac = [&](floatx4 &acc, int i, int j, int kg) {
		const int jc = j < N ? j : N - 1;
		const int patch = jc / PO, pix = jc - patch * PO, py = pix / SO, px = pix - py * SO;
		const float *pb = in + patch * CIN * PI + py * SI + px;
		if constexpr (CIN == 1) {
			for (int s = 0; s < 3; ++s) {
				const int tap = 4 * s + kg;
				const float a = tap < 9 ? w[i * 9 + tap] : 0.f;
				const float b = tap < 9 ? pb[(tap / 3) * SI + tap % 3] : 0.f;
				acc = mfma(a, b, acc);
			}
		} else {
			const float *pa = w + i * CIN * 9 + kg * 9;
			pb += kg * PI;
			for (int s = 0; s < CIN / 4; ++s, pa += 36, pb += 4 * PI) {
				float a[9];
#pragma unroll
				for (int t = 0; t < 9; ++t) a[t] = pa[t];
#pragma unroll
				for (int t = 0; t < 9; ++t) acc = mfma(a[t], pb[(t / 3) * SI + t % 3], acc);
			}
		}
	};
	auto put = [&](int co, int j, float v) {
		const int patch = j / PO, pix = j - patch * PO;
		out[(patch * FM + co) * PO + pix] = fmaxf(v + bias[co], 0.f);
	};
	block_gemm(N, mac, put);
}

// weight and bias gradients of a layer: dW[co, ci, tap] = sum_p g[co, p] in[ci, p + tap] into the workgroup's slab row
template <int NP, int CIN, int SI>
__device__ void conv_weight_grad(const float *g, const float *in, float *__restrict__ dw, float *__restrict__ db)
{
	constexpr int SO = SI - 2, PO = SO * SO, PI = SI * SI, P = NP * PO, KN = CIN * 9;
	auto mac = [&](floatx4 &acc, int i, int j, int kg) {
		const int jc = j < KN ? j : KN - 1;
		const int ci = jc / 9, tap = jc - ci * 9;
		const float *pb = in + ci * PI + (tap / 3) * SI + tap % 3;
		const float *pa = g + i * PO;
		for (int s = 0; s < (P + 3) / 4; ++s) {
			const int p = 4 * s + kg;
			const int pc = p < P ? p : P - 1;
			const int patch = pc / PO, pix = pc - patch * PO, py = pix / SO, px = pix - py * SO;
			const float a = p < P ? pa[patch * FM * PO + pix] : 0.f;
			const float b = p < P ? pb[patch * CIN * PI + py * SI + px] : 0.f;
			acc = mfma(a, b, acc);
		}
	};
	auto put = [&](int co, int j, float v) { dw[co * KN + j] = v; };
	block_gemm(KN, mac, put);
	if (threadIdx.x < FM) {
		const int co = threadIdx.x;
		float s = 0.f;
		for (int patch = 0; patch < NP; ++patch)
			for (int pix = 0; pix < PO; ++pix) s += g[(patch * FM + co) * PO + pix];
		db[co] = s;
	}
}

// data gradient of a layer into its input activations, in place, masked by their ReLU: in[ci, q] = in > 0 ? dX : 0
template <int NP, int SI>
__device__ void conv_data_grad(const float *__restrict__ w, const float *g, float *in)
{
	constexpr int SO = SI - 2, PO = SO * SO, PI = SI * SI, N = NP * PI;
	auto mac = [&](floatx4 &acc, int i, int j, int kg) {
		const int jc = j < N ? j : N - 1;
		const int patch = jc / PI, q = jc - patch * PI, qy = q / SI, qx = q - qy * SI;
		bool ok[9];
#pragma unroll
		for (int t = 0; t < 9; ++t) {
			const int y = qy - t / 3, x = qx - t % 3;
			ok[t] = y >= 0 && y < SO && x >= 0 && x < SO;
		}
		// g[patch][co = 4s + kg][qy - ky][qx - kx]; out-of-range taps read 0 (the offsets are only formed where valid)
		const int gb = patch * FM * PO + kg * PO + qy * SO + qx;
		const float *pa = w + kg * FM * 9 + i * 9;
		for (int s = 0; s < FM / 4; ++s, pa += 4 * FM * 9) {
			float a[9];
#pragma unroll
			for (int t = 0; t < 9; ++t) a[t] = pa[t];
			const int base = gb + s * 4 * PO;
#pragma unroll
			for (int t = 0; t < 9; ++t) acc = mfma(a[t], ok[t] ? g[base - (t / 3) * SO - t % 3] : 0.f, acc);
		}
	};
	auto put = [&](int ci, int j, float v) {
		const int patch = j / PI, q = j - patch * PI;
		float *p = in + (patch * FM + ci) * PI + q;
		*p = *p > 0.f ? v : 0.f;
	};
	block_gemm(N, mac, put);
}

// ---- the tower of a net N ------------------------------------------------------------------------------------------------
template <class N> constexpr int TOWER_LDS_FLOATS = lds_act<N>(N::NL + 1);
template <class N> constexpr size_t TOWER_LDS_BYTES = (size_t)TOWER_LDS_FLOATS<N> * sizeof(float);

// the convolutions L .. NL of the workgroup's patches X into A_1 .. A_NL, all in LDS; a barrier after each
template <class N, int L = 1>
__device__ __forceinline__ void tower_forward(const float *__restrict__ params, float *lds)
{
	static_assert(N::FM == FM, "this family's feature maps");
	conv_forward<N::NP, L == 1 ? 1 : FM, side<N>(L - 1)>(params + off_w<N>(L), params + off_b<N>(L), lds + lds_act<N>(L - 1), lds + lds_act<N>(L));
	__syncthreads();
	if constexpr (L < N::NL) tower_forward<N, L + 1>(params, lds);
}

// layers L .. 1 of the backward pass, A_L holding its gradient: layer l's weight and bias gradients into g (the workgroup's
// slab row), then its data gradient over A_{l-1} in place; a barrier between any two GEMMs
template <class N, int L = N::NL>
__device__ __forceinline__ void tower_backward(const float *__restrict__ params, float *__restrict__ g, float *lds)
{
	constexpr int SI = side<N>(L - 1);
	conv_weight_grad<N::NP, L == 1 ? 1 : FM, SI>(lds + lds_act<N>(L), lds + lds_act<N>(L - 1), g + off_w<N>(L), g + off_b<N>(L));
	if constexpr (L > 1) {
		__syncthreads();
		conv_data_grad<N::NP, SI>(params + off_w<N>(L), lds + lds_act<N>(L), lds + lds_act<N>(L - 1));
		__syncthreads();
		tower_backward<N, L - 1>(params, g, lds);
	}
}

// The FC stack's input a0 (2n, 2 * FM) has two rows per pair: [feat(left) | feat(positive)], [feat(left) | feat(negative)].
// Feature c of patch (0 left, 1 positive, 2 negative) of a pair goes there ...
__device__ __forceinline__ void scatter_feature(float *__restrict__ a0, int pair, int patch, int c, float v)
{
	float *r0 = a0 + (int64_t)(2 * pair) * (2 * FM), *r1 = r0 + 2 * FM;
	if (patch == 0) {
		r0[c] = v;
		r1[c] = v;
	} else if (patch == 1) {
		r0[FM + c] = v;
	} else {
		r1[FM + c] = v;
	}
}

// ... and its gradient comes back from dfeat, laid out as a0: the left patch gets the positive's, then the negative's sample
__device__ __forceinline__ float gather_feature_grad(const float *__restrict__ dfeat, int pair, int patch, int c)
{
	const float *r0 = dfeat + (int64_t)(2 * pair) * (2 * FM), *r1 = r0 + 2 * FM;
	return patch == 0 ? r0[c] + r1[c] : patch == 1 ? r0[FM + c] : r1[FM + c];
}

}  // namespace mc
