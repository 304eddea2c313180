// The FC stack of the accurate architecture's training step, shared by train_slow.hip (Linear 224 -> 384 x 4 -> 1),
// train_mb_slow.hip (Linear 224 -> 384 x 3 -> 1) and train_slow_depth.hip (Linear 224 -> 384 x l2 -> 1, l2 = 1..7): batch GEMMs over the R = 2 * n_pairs rows on v_mfma_f32_16x16x4_f32, one wave
// per 16 x 16 tile; the head (last Linear, Sigmoid, BCECriterion2 and their backward passes); the SGD update.  The kernels
// take their layer by pointer, so the number of hidden Linears is the host's loop count.  Then, over a StepShape (a value:
// that of a net N of train_net.h, or train_slow_depth.hip's with l2 given at run time), the FC parameters' offsets, the step's
// workspace, the launches of the FC stack and the step's argument check.
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

// ---- the FC stack of a step: the flat parameter buffer goes on  | fw1 fb1 .. fw(L2) fb(L2) fw(L2+1) fb(L2+1) ------------------
constexpr int NIN = 2 * FM;              // columns of the FC stack's input
static_assert(NIN % 16 == 0, "16 x 16 tiles");
constexpr int MAX_L2 = 7;                // the most hidden Linears a step takes: prediction's mc_fc_stack serves 8 layers
__host__ __device__ constexpr int fc_in(int l) { return l == 1 ? NIN : NH; }

// What the host side of a step knows of its net: the tower through its patch side, patches per workgroup and floats of
// convolution parameters, and the number of hidden Linears.  A VALUE: train_slow.hip and train_mb_slow.hip make theirs from a
// net N of train_net.h at compile time (step_shape<N>()), train_slow_depth.hip takes l2 from its caller.  Every offset, the
// workspace, the FC launches and the argument check below are stated once, over this value.
struct StepShape {
	const char *prefix;    // what every message starts with
	int ps, np, n_conv;    // N::PS, N::NP, n_conv<N>()
	int l2;                // hidden Linears, 1 .. MAX_L2
	int max_pairs;         // pairs per batch
	constexpr int off_fw(int l) const { return n_conv + (l == 1 ? 0 : NH * NIN + NH + (l - 2) * (NH * NH + NH)); }
	constexpr int off_fb(int l) const { return off_fw(l) + (l == l2 + 1 ? NH : NH * fc_in(l)); }
	constexpr int n_params() const { return off_fb(l2 + 1) + 1; }
	constexpr int n_fc() const { return n_params() - n_conv; }
	constexpr bool fc_weights_aligned() const   // the float4 loads of fc_forward_kernel and fc_backward_kernel
	{
		for (int l = 1; l <= l2; ++l)
			if (off_fw(l) % 4 != 0) return false;
		return true;
	}
};
template <class N> constexpr StepShape step_shape() { return {N::PREFIX, N::PS, N::NP, n_conv<N>(), N::L2, N::MAX_PAIRS}; }
template <class N> __host__ __device__ constexpr int off_fw(int l) { return step_shape<N>().off_fw(l); }
template <class N> __host__ __device__ constexpr int off_fb(int l) { return step_shape<N>().off_fb(l); }
template <class N> __host__ __device__ constexpr int n_params() { return step_shape<N>().n_params(); }
template <class N> constexpr bool fc_weights_aligned() { return step_shape<N>().fc_weights_aligned(); }

// the workspace of a step over n pairs; R = 2 n rows of the FC stack
struct StepWorkspace {
	float *xs;             // (n, 3, PS, PS) sampled patches
	float *a[MAX_L2 + 1];  // a[0] (R, 224) the FC input; a[1..L2] (R, 384) the hidden Linears' outputs
	float *g[2];           // (R, 384) output gradients of two consecutive Linears
	float *dfeat;          // (R, 224) gradient of a[0]
	float *gfc;            // (NFC) gradient of the FC parameters
	float *slab;           // (3 n / NP, NCONV) the tower workgroups' gradients of the convolutions
	size_t floats;
};
template <class N> struct Workspace : StepWorkspace {};   // that of a compiled net

static StepWorkspace carve(const StepShape &s, float *base, int n_pairs)
{
	StepWorkspace ws = {};
	size_t o = 0;
	const size_t R = 2 * (size_t)n_pairs;
	auto take = [&](size_t n) {
		float *p = base + o;
		o += align_up(n, 64);
		return p;
	};
	ws.xs = take((size_t)n_pairs * 3 * s.ps * s.ps);
	ws.a[0] = take(R * NIN);
	for (int l = 1; l <= s.l2; ++l) ws.a[l] = take(R * NH);
	ws.g[0] = take(R * NH);
	ws.g[1] = take(R * NH);
	ws.dfeat = take(R * NIN);
	ws.gfc = take(s.n_fc());
	ws.slab = take((size_t)(3 / s.np) * n_pairs * s.n_conv);
	ws.floats = o;
	return ws;
}

template <class N> static Workspace<N> carve(float *base, int n_pairs)
{
	static_assert(N::L2 >= 1 && N::L2 <= MAX_L2, "StepWorkspace's activations");
	Workspace<N> ws;
	static_cast<StepWorkspace &>(ws) = carve(step_shape<N>(), base, n_pairs);
	return ws;
}

static size_t step_workspace_bytes(const StepShape &s, int n_pairs)
{
	if (n_pairs < 1 || n_pairs > s.max_pairs) return 0;
	return carve(s, nullptr, n_pairs).floats * sizeof(float);
}

template <class N> static size_t step_workspace_bytes(int n_pairs) { return step_workspace_bytes(step_shape<N>(), n_pairs); }

// The launches between the two tower kernels: ws.a[0] -> the hidden Linears, the head (the step's loss), the backward passes
// -> ws.gfc and ws.dfeat.  The head writes ws.g[0]; Linear l reads g[(L2 - l) & 1] and writes the other, so at L2 = 1 the one
// hidden Linear, which is also the first, reads what the head wrote.
static int enqueue_fc(const StepShape &s, const StepWorkspace &ws, const float *params, int n_pairs, float *loss_out, hipStream_t st)
{
	const int L2 = s.l2, NCONV = s.n_conv;
	const int R = 2 * n_pairs, mtr = (R + 15) / 16;
	for (int l = 1; l <= L2; ++l) {
		fc_forward_kernel<<<cdiv(mtr * (NH / 16), FC_WAVES), FC_WAVES * 64, 0, st>>>(ws.a[l - 1], fc_in(l), params + s.off_fw(l), params + s.off_fb(l),
		                                                                            ws.a[l], R);
		if (int rc = check_launch(s.prefix, "fc_forward")) return rc;
	}
	fc_head_kernel<<<1, HEAD_NT, 0, st>>>(ws.a[L2], params + s.off_fw(L2 + 1), params + s.off_fb(L2 + 1), R, ws.g[0],
	                                      ws.gfc + (s.off_fw(L2 + 1) - NCONV), ws.gfc + (s.off_fb(L2 + 1) - NCONV), loss_out);
	if (int rc = check_launch(s.prefix, "fc_head")) return rc;
	for (int l = L2; l >= 1; --l) {
		const int K = fc_in(l), tasks = (mtr + NH / 16) * (K / 16) + NH / 64;
		const float *g = ws.g[(L2 - l) & 1];
		float *dw = ws.gfc + (s.off_fw(l) - NCONV), *db = ws.gfc + (s.off_fb(l) - NCONV);
		if (l > 1)
			fc_backward_kernel<true><<<cdiv(tasks, FC_WAVES), FC_WAVES * 64, 0, st>>>(g, ws.a[l - 1], K, params + s.off_fw(l), R, ws.g[(L2 + 1 - l) & 1],
			                                                                         dw, db);
		else   // a[0]'s ReLU mask is applied by the tower, which has the activations
			fc_backward_kernel<false><<<cdiv(tasks, FC_WAVES), FC_WAVES * 64, 0, st>>>(g, ws.a[0], K, params + s.off_fw(l), R, ws.dfeat, dw, db);
		if (int rc = check_launch(s.prefix, "fc_backward")) return rc;
	}
	return 0;
}

template <class N>
static int enqueue_fc(const Workspace<N> &ws, const float *params, int n_pairs, float *loss_out, hipStream_t st)
{
	return enqueue_fc(step_shape<N>(), ws, params, n_pairs, loss_out, st);
}

static int check_step_args(const StepShape &s, int n_pairs, const float *params, const float *moms, void *ws, size_t ws_bytes)
{
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= s.max_pairs, "%s: n_pairs %d outside [1, %d]", s.prefix, n_pairs, s.max_pairs);
	MC_REQUIRE(params && moms, "%s: null params / momenta", s.prefix);
	MC_REQUIRE(((uintptr_t)params & 15) == 0, "%s: params not 16-byte aligned", s.prefix);
	MC_REQUIRE(ws && ws_bytes >= step_workspace_bytes(s, n_pairs), "%s: workspace of %zu bytes, %zu needed", s.prefix, ws_bytes,
	           step_workspace_bytes(s, n_pairs));
	MC_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: workspace not 16-byte aligned", s.prefix);
	return 0;
}

template <class N>
static int check_step_args(int n_pairs, const float *params, const float *moms, void *ws, size_t ws_bytes)
{
	static_assert(MC_FC_HEAD_MAX_ROWS == 2 * N::MAX_PAIRS, "the head kernel's rows");
	return check_step_args(step_shape<N>(), n_pairs, params, moms, ws, ws_bytes);
}

}  // namespace mc
