// The fast architecture's training step on v_mfma_f32_32x32x2_f32, shared by train.hip (four layers on 9 x 9 patches) and
// train_mb.hip (five layers on 11 x 11 patches): 64 feature maps, a pair's three patches in LDS, one workgroup of eight waves.
// The block GEMM, the three convolution GEMMs (see train.hip's head), the Normalize2 / StereoJoin1 / Margin2 tail, then the
// step itself over a net N of train_net.h -- the LDS layout, the layer chain, the update -- and the step's argument check.
#pragma once
#include "mc_common.h"
#include "train_net.h"

namespace mc {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int FM = 64;                   // feature maps per layer (MC_TRAIN_FM, MC_TRAIN_MB_FM)
constexpr int NW = 8;                    // waves per workgroup (two per SIMD)
constexpr int NT = NW * 64;
constexpr int SPLIT_FLOATS = NW * 16 * 64;   // LDS floats of the split-K partial tiles: [8][16][64]

// ---- block GEMM on the matrix cores --------------------------------------------------------------------------------
// Tiles of 32 x 32 over (M = 64) x N; a lane holds A[row lane&31][k = lane>>5] and B[k = lane>>5][col lane&31] and its
// result registers r are rows (r&3) + 8*(r>>2) + 4*(lane>>5) of column lane&31.  KS > 1 splits the K steps into KS
// slices over the waves; the partial tiles meet in LDS and are added in slice order.
// mac(acc, i, j, h, s0, s1): run K steps [s0, s1) for output row i / column j on lane half h.
// out(row, col, v): the epilogue of one element.
// A GEMM of N <= 32 columns has only two output tiles for eight waves: split_k(N) slices its K over four waves each.  N is
// 3 * (output pixels) in the forward pass and 3 * (input pixels) in the data gradient; the weight gradient's 576 columns never split.
__host__ __device__ constexpr int split_k(int N) { return N <= 32 ? 4 : 1; }

template <int KS, class Mac, class Out>
__device__ __forceinline__ void block_gemm(int N, int ksteps, float *split, Mac mac, Out out)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5;
	const int ntile = 2 * ((N + 31) / 32);
	for (int task = wave; task < ntile * KS; task += NW) {
		const int tile = task / KS, ks = task - tile * KS;
		const int m0 = (tile & 1) * 32, n0 = (tile >> 1) * 32;
		floatx16 acc;
		for (int r = 0; r < 16; ++r) acc[r] = 0.f;
		mac(acc, m0 + (lane & 31), n0 + (lane & 31), h, ksteps * ks / KS, ksteps * (ks + 1) / KS);
		if (KS == 1) {
			const int col = n0 + (lane & 31);
			if (col < N)
				for (int r = 0; r < 16; ++r) out(m0 + (r & 3) + 8 * (r >> 2) + 4 * h, col, acc[r]);
		} else {
			for (int r = 0; r < 16; ++r) split[(task * 16 + r) * 64 + lane] = acc[r];
		}
	}
	if (KS > 1) {
		__syncthreads();
		for (int e = threadIdx.x; e < ntile * 16 * 64; e += NT) {
			const int tile = e >> 10, r = (e >> 6) & 15, l = e & 63;
			const int m0 = (tile & 1) * 32, n0 = (tile >> 1) * 32, col = n0 + (l & 31);
			float v = split[((tile * KS) * 16 + r) * 64 + l];
			for (int ks = 1; ks < KS; ++ks) v += split[((tile * KS + ks) * 16 + r) * 64 + l];
			if (col < N) out(m0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col, v);
		}
	}
}

__device__ __forceinline__ floatx16 mfma(float a, float b, floatx16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// forward of layer with CIN input maps of SI x SI per patch into FM maps of (SI-2)^2: out = b + W * in (+ ReLU)
template <int CIN, int SI, int KS>
__device__ void conv_forward(const float *__restrict__ w, const float *__restrict__ bias, const float *in, float *out, bool relu, float *split)
{
	constexpr int SO = SI - 2, PO = SO * SO, PI = SI * SI, N = 3 * PO;
	auto mac = [&](floatx16 &acc, int i, int j, int h, int s0, int s1) {
		const int jc = j < N ? j : N - 1;
		const int patch = jc / PO, pix = jc - patch * PO, py = pix / SO, px = pix - py * SO;
		const float *pb = in + patch * CIN * PI + py * SI + px;
		if constexpr (CIN == 1) {
			for (int s = s0; s < s1; ++s) {
				const int tap = 2 * s + h;
				const float a = tap < 9 ? w[i * 9 + tap] : 0.f;
				const float b = tap < 9 ? pb[(tap / 3) * SI + tap % 3] : 0.f;
				acc = mfma(a, b, acc);
			}
		} else {
			const float *pa = w + i * CIN * 9 + h * 9 + s0 * 18;
			pb += h * PI + s0 * 2 * PI;
			for (int s = s0; s < s1; ++s, pa += 18, pb += 2 * PI) {
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
		v = v + bias[co];
		out[(patch * FM + co) * PO + pix] = relu ? fmaxf(v, 0.f) : v;
	};
	block_gemm<KS>(N, CIN == 1 ? 5 : CIN / 2, split, mac, put);
}

// weight and bias gradients of a layer: dW[co, ci, tap] = sum_p g[co, p] in[ci, p + tap] into slab (no atomics)
template <int CIN, int SI>
__device__ void conv_weight_grad(const float *g, const float *in, float *__restrict__ dw, float *__restrict__ db, float *split)
{
	constexpr int SO = SI - 2, PO = SO * SO, PI = SI * SI, P = 3 * PO, KN = CIN * 9;
	auto mac = [&](floatx16 &acc, int i, int j, int h, int s0, int s1) {
		const int jc = j < KN ? j : KN - 1;
		const int ci = jc / 9, tap = jc - ci * 9;
		const float *pb = in + ci * PI + (tap / 3) * SI + tap % 3;
		const float *pa = g + i * PO;
		for (int s = s0; s < s1; ++s) {
			const int p = 2 * s + h;
			const int pc = p < P ? p : P - 1;
			const int patch = pc / PO, pix = pc - patch * PO, py = pix / SO, px = pix - py * SO;
			const float a = p < P ? pa[patch * FM * PO + pix] : 0.f;
			const float b = p < P ? pb[patch * CIN * PI + py * SI + px] : 0.f;
			acc = mfma(a, b, acc);
		}
	};
	auto put = [&](int co, int j, float v) { dw[co * KN + j] = v; };
	block_gemm<1>(KN, (P + 1) / 2, split, mac, put);
	if (threadIdx.x < FM) {
		const int co = threadIdx.x;
		float s = 0.f;
		for (int patch = 0; patch < 3; ++patch)
			for (int pix = 0; pix < PO; ++pix) s += g[(patch * FM + co) * PO + pix];
		db[co] = s;
	}
}

// data gradient of a layer into its input activations, in place, masked by their ReLU: in[ci, q] = in > 0 ? dX : 0
template <int SI, int KS>
__device__ void conv_data_grad(const float *__restrict__ w, const float *g, float *in, float *split)
{
	constexpr int SO = SI - 2, PO = SO * SO, PI = SI * SI, N = 3 * PI;
	auto mac = [&](floatx16 &acc, int i, int j, int h, int s0, int s1) {
		const int jc = j < N ? j : N - 1;
		const int patch = jc / PI, q = jc - patch * PI, qy = q / SI, qx = q - qy * SI;
		bool ok[9];
#pragma unroll
		for (int t = 0; t < 9; ++t) {
			const int y = qy - t / 3, x = qx - t % 3;
			ok[t] = y >= 0 && y < SO && x >= 0 && x < SO;
		}
		// g[patch][co = 2s + h][qy - ky][qx - kx]; out-of-range taps read 0 (the offsets are only formed where valid)
		const int gb = patch * FM * PO + h * PO + qy * SO + qx;
		const float *pa = w + h * FM * 9 + i * 9 + s0 * 2 * FM * 9;
		for (int s = s0; s < s1; ++s, pa += 2 * FM * 9) {
			float a[9];
#pragma unroll
			for (int t = 0; t < 9; ++t) a[t] = pa[t];
			const int base = gb + s * 2 * PO;
#pragma unroll
			for (int t = 0; t < 9; ++t) acc = mfma(a[t], ok[t] ? g[base - (t / 3) * SO - t % 3] : 0.f, acc);
		}
	};
	auto put = [&](int ci, int j, float v) {
		const int patch = j / PI, q = j - patch * PI;
		float *p = in + (patch * FM + ci) * PI + q;
		*p = *p > 0.f ? v : 0.f;
	};
	block_gemm<KS>(N, FM / 2, split, mac, put);
}

__device__ __forceinline__ float wave_sum(float v)
{
	for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
	return v;
}

// Normalize2 (adcensus.cu:1284-1333), StereoJoin1, Margin2 (adcensus.cu:1379-1451) and their backward passes on the last
// layer's features A [3][64] of a pair (left, positive, negative), run by the first wave with channel c = lane: A becomes
// the gradient with respect to the features, the pair's loss is returned.
__device__ __forceinline__ float hinge_tail(float *A, int c, float margin, int pow, float inv_pairs)
{
	float x[3], n[3], y[3];
	for (int p = 0; p < 3; ++p) {
		x[p] = A[p * FM + c];
		n[p] = wave_sum(x[p] * x[p]) + 1e-5f;
		y[p] = x[p] / sqrtf(n[p]);
	}
	const float pos = wave_sum(y[0] * y[1]), neg = wave_sum(y[0] * y[2]);
	const float f = neg - pos + margin;
	float loss, gp, gn;
	if (pow == 1) {
		loss = fmaxf(0.f, f);
		gp = -1.f * (f > 0);
		gn = (float)(f > 0);
	} else {
		const float d = fmaxf(0.f, f);
		loss = d * d * 0.5f;
		gp = -f * (f > 0);
		gn = f * (f > 0);
	}
	gp *= inv_pairs;
	gn *= inv_pairs;
	// StereoJoin1 backward; the left patch gets both pairs' contributions
	float go[3] = {y[1] * gp + y[2] * gn, y[0] * gp, y[0] * gn};
	for (int p = 0; p < 3; ++p) {
		const float denom = powf(n[p], 1.5f);
		const float dot = wave_sum(x[p] * go[p]);
		const float others = dot - x[p] * go[p];
		A[p * FM + c] = (n[p] - x[p] * x[p]) / denom * go[p] - others * x[p] / denom;
	}
	return loss;
}

// ---- the step of a net N -----------------------------------------------------------------------------------------------
// LDS (floats): the activations of train_net.h, then the split-K partial tiles [8][16][64]
template <class N> constexpr int STEP_LDS_FLOATS = lds_act<N>(N::NL + 1) + SPLIT_FLOATS;
template <class N> constexpr size_t STEP_LDS_BYTES = (size_t)STEP_LDS_FLOATS<N> * sizeof(float);

// layers L .. NL of the forward pass: A_l = ReLU(b_l + W_l * A_{l-1}), the last without ReLU; a barrier after each
template <class N, int L = 1>
__device__ __forceinline__ void chain_forward(const float *__restrict__ params, float *lds, float *split)
{
	constexpr int SI = side<N>(L - 1), SO = SI - 2;
	conv_forward<L == 1 ? 1 : FM, SI, split_k(3 * SO * SO)>(params + off_w<N>(L), params + off_b<N>(L), lds + lds_act<N>(L - 1), lds + lds_act<N>(L),
	                                                         L < N::NL, split);
	__syncthreads();
	if constexpr (L < N::NL) chain_forward<N, L + 1>(params, lds, split);
}

// layers L .. 1 of the backward pass, A_L holding its gradient: layer l's weight and bias gradients into g, then its data
// gradient over A_{l-1} in place; a barrier between any two GEMMs
template <class N, int L = N::NL>
__device__ __forceinline__ void chain_backward(const float *__restrict__ params, float *__restrict__ g, float *lds, float *split)
{
	constexpr int SI = side<N>(L - 1);
	conv_weight_grad<L == 1 ? 1 : FM, SI>(lds + lds_act<N>(L), lds + lds_act<N>(L - 1), g + off_w<N>(L), g + off_b<N>(L), split);
	if constexpr (L > 1) {
		__syncthreads();
		conv_data_grad<SI, split_k(3 * SI * SI)>(params + off_w<N>(L), lds + lds_act<N>(L), lds + lds_act<N>(L - 1), split);
		__syncthreads();
		chain_backward<N, L - 1>(params, g, lds, split);
	}
}

// One pair's step, its patches already in LDS behind a barrier: forward, Normalize2 / StereoJoin1 / Margin2 and their
// backward passes, backward; the gradients go to g (the pair's slab row), the loss to *loss.
template <class N>
__device__ __forceinline__ void pair_step(const float *__restrict__ params, float margin, int pow, float inv_pairs, float *lds,
                                          float *__restrict__ g, float *__restrict__ loss)
{
	static_assert(N::FM == FM && N::NP == 3 && 3 * N::PS * N::PS <= NT, "this family's feature maps; one thread per pixel of the pair's patches");
	float *split = lds + lds_act<N>(N::NL + 1);
	chain_forward<N>(params, lds, split);
	if (threadIdx.x < 64) {
		const float l = hinge_tail(lds + lds_act<N>(N::NL), threadIdx.x, margin, pow, inv_pairs);
		if (threadIdx.x == 0) *loss = l;
	}
	__syncthreads();
	chain_backward<N>(params, g, lds, split);
}

// The update: g = the slab's rows summed in pair order; v = mom * v - lr * g; w += v.  Block 0 also writes the mean loss.
__device__ __forceinline__ void slab_sgd(const float *__restrict__ slab, const float *__restrict__ pair_losses, int n_pairs, int n_params,
                                         float *__restrict__ params, float *__restrict__ moms, float lr, float mom, float *__restrict__ loss_out)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j < n_params) {
		float g = 0.f;
		for (int p = 0; p < n_pairs; ++p) g += slab[(int64_t)p * n_params + j];
		const float v = moms[j] * mom - lr * g;
		moms[j] = v;
		params[j] = params[j] + v;
	}
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		float s = 0.f;
		for (int p = 0; p < n_pairs; ++p) s += pair_losses[p];
		*loss_out = s / (float)n_pairs;
	}
}

// the workspace: a slab row and a loss per pair
template <class N> static size_t step_workspace_bytes(int n_pairs)
{
	if (n_pairs < 1 || n_pairs > N::MAX_PAIRS) return 0;
	return (size_t)n_pairs * (n_conv<N>() + 1) * sizeof(float);
}

template <class N>
static int check_step_args(int n_pairs, const float *params, const float *moms, float margin, int pow, void *ws, size_t ws_bytes)
{
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= N::MAX_PAIRS, "%s: n_pairs %d outside [1, %d]", N::PREFIX, n_pairs, N::MAX_PAIRS);
	MC_REQUIRE(params && moms, "%s: null params / momenta", N::PREFIX);
	MC_REQUIRE(pow == 1 || pow == 2, "%s: pow %d (Margin2 has pow 1 and 2, adcensus.cu:1427-1447)", N::PREFIX, pow);
	MC_REQUIRE(isfinite(margin), "%s: margin not finite", N::PREFIX);
	MC_REQUIRE(ws && ws_bytes >= step_workspace_bytes<N>(n_pairs), "%s: workspace of %zu bytes, %zu needed", N::PREFIX, ws_bytes,
	           step_workspace_bytes<N>(n_pairs));
	return 0;
}

}  // namespace mc
