// Training of the accurate architecture on Middlebury (main.lua:116-130, 602-890, `mb slow`: -l1 5 -fm 112 -l2 3 -nh2 384) on
// gfx950: libmctrainmbslow.so (include/mc_train_mb_slow.h).
//
// The step is train_slow.hip's, restated for five valid 3x3 convolutions on 11 x 11 patches, three hidden Linears and the
// ragged image store of train_mb.hip.  A pair's activations are 221 KB and do not fit a CU's LDS; ONE PATCH's are 74 KB, so
// the tower kernels run one workgroup of 8 waves per PATCH: block 3 * pair + p handles patch p of (left, positive, negative),
// and two workgroups fit a CU.  A step is TEN launches, all on v_mfma_f32_16x16x4_f32:
//    1  mb_tower_forward_kernel   the patch's 121 pixels (sampled from its plane and kept for launch 9, or given) through the
//                                 five convolutions with every activation in LDS (74 432 bytes); writes the patch's 112 features
//                                 into rows 2 * pair, 2 * pair + 1 of the FC input: [feat(left) | feat(positive)],
//                                 [feat(left) | feat(negative)]
//  2-4  fc_forward_kernel         A_l = ReLU(A_{l-1} W_l^T + b_l) over the 2 * n_pairs rows
//    5  fc_head_kernel            Linear 384 -> 1, Sigmoid, BCECriterion2, their backward passes, dW_4, db_4, the loss, G_3
//  6-8  fc_backward_kernel        per hidden Linear: data, weight and bias gradients
//    9  mb_tower_backward_kernel  RECOMPUTES the patch's forward pass, takes the gradient of its features (the left patch:
//                                 positive's sample, then negative's, added in that order), then the backward pass; the
//                                 convolutions' gradients go to the PATCH's row of a slab of 3 * n_pairs rows
//   10  mb_slow_sgd_kernel        sums the slab's rows in the order 3 * pair + p, takes the FC gradients as they are,
//                                 v = mom * v - lr * g;  w += v  on all 835 617 parameters
// The GEMMs are train_slow_conv.h's with one patch per workgroup, the FC kernels and the update train_slow_fc.h's, the sampler
// train_mb_sampler.h's: this file holds the layer chain, the LDS layout, the workspace and the entry points.
#include "mc_common.h"
#include "../../include/mc_train_mb_slow.h"
#include "train_mb_sampler.h"
#include "train_slow_conv.h"
#include "train_range.h"
#define MC_FC_HEAD_MAX_ROWS (2 * MC_TRAIN_MB_SLOW_MAX_PAIRS)
#include "train_slow_fc.h"

namespace mc {

constexpr int PS = MC_TRAIN_MB_SLOW_WS;
constexpr int NL = MC_TRAIN_MB_SLOW_L1;
constexpr int L2 = MC_TRAIN_MB_SLOW_L2;
constexpr int NIN = 2 * FM;              // columns of the FC stack's input
constexpr int NPRM = MC_TRAIN_MB_SLOW_NPRM;
constexpr int NCONV = MC_TRAIN_MB_SLOW_NCONV;
constexpr int NFC = MC_TRAIN_MB_SLOW_NFC;
constexpr int NPARAMS = MC_TRAIN_MB_SLOW_NPARAMS;
constexpr int PPIX = PS * PS;            // floats of a patch
constexpr int NPIX = 3 * PPIX;           // floats of a pair's patches
static_assert(MC_TRAIN_MB_SLOW_WS == MC_TRAIN_MB_WS && NPRM == MC_TRAIN_MB_NPRM && NPRM == MC_TRAIN_NPRM, "the sampler's patch and parameter layout");
static_assert(FM == MC_TRAIN_MB_SLOW_FM && NH == MC_TRAIN_MB_SLOW_NH2, "train_slow_conv.h's feature maps, train_slow_fc.h's hidden units");
static_assert(NIN % 16 == 0 && PPIX <= NT && FM <= NT, "16 x 16 tiles; one thread per patch pixel and per feature");

// offsets of the flat parameter buffer: w1 b1 .. w5 b5 | fw1 fb1 fw2 fb2 fw3 fb3 fw4 fb4
constexpr int LAYER_STRIDE = FM * FM * 9 + FM;
__host__ __device__ constexpr int off_w(int l) { return l == 1 ? 0 : FM * 9 + FM + (l - 2) * LAYER_STRIDE; }
__host__ __device__ constexpr int off_b(int l) { return l == 1 ? FM * 9 : off_w(l) + FM * FM * 9; }
__host__ __device__ constexpr int fc_in(int l) { return l == 1 ? NIN : NH; }
__host__ __device__ constexpr int off_fw(int l) { return l == 1 ? NCONV : NCONV + NH * NIN + NH + (l - 2) * (NH * NH + NH); }
__host__ __device__ constexpr int off_fb(int l) { return off_fw(l) + (l == L2 + 1 ? NH : NH * fc_in(l)); }
static_assert(off_b(NL) + FM == NCONV && NCONV == 453152, "convolution parameter layout");
static_assert(off_fb(L2 + 1) + 1 == NPARAMS && NCONV + NFC == NPARAMS && NPARAMS == 835617, "parameter layout");
static_assert(off_fw(1) % 4 == 0 && off_fw(2) % 4 == 0 && off_fw(3) % 4 == 0, "float4 loads of the FC weights");

// LDS layout of the tower kernels (floats): ONE patch's activations of every layer
constexpr int S0 = 11, S1 = 9, S2 = 7, S3 = 5, S4 = 3;
constexpr int L_X = 0;                                  // [121], padded to 128
constexpr int L_A1 = 128;                               // [112][81]
constexpr int L_A2 = L_A1 + FM * S1 * S1;               // [112][49]
constexpr int L_A3 = L_A2 + FM * S2 * S2;               // [112][25]
constexpr int L_A4 = L_A3 + FM * S3 * S3;               // [112][9]
constexpr int L_A5 = L_A4 + FM * S4 * S4;               // [112]
constexpr int L_TOTAL = L_A5 + FM;
constexpr size_t TOWER_LDS_BYTES = (size_t)L_TOTAL * sizeof(float);
static_assert(L_TOTAL == 18608 && TOWER_LDS_BYTES == 74432 && 2 * TOWER_LDS_BYTES <= 160 * 1024, "two patches' workgroups fit a CU's 160 KiB of LDS");

// the five convolutions of the workgroup's patch X into A1 .. A5, all in LDS
__device__ __forceinline__ void tower_forward(const float *__restrict__ params, float *lds)
{
	float *X = lds + L_X, *A1 = lds + L_A1, *A2 = lds + L_A2, *A3 = lds + L_A3, *A4 = lds + L_A4, *A5 = lds + L_A5;
	conv_forward<1, 1, S0>(params + off_w(1), params + off_b(1), X, A1);
	__syncthreads();
	conv_forward<1, FM, S1>(params + off_w(2), params + off_b(2), A1, A2);
	__syncthreads();
	conv_forward<1, FM, S2>(params + off_w(3), params + off_b(3), A2, A3);
	__syncthreads();
	conv_forward<1, FM, S3>(params + off_w(4), params + off_b(4), A3, A4);
	__syncthreads();
	conv_forward<1, FM, S4>(params + off_w(5), params + off_b(5), A4, A5);
	__syncthreads();
}

// Launch 1, block 3 * pair + p.  SAMPLE: pixels 121 * p .. 121 * p + 120 of the pair come from the planes (rows[pair] of nnz,
// src and prm of the pair) and are kept in xs for the backward kernel; otherwise from patches (n_pairs, 3, 11, 11).  Writes
// the patch's half-rows of rows 2 * pair and 2 * pair + 1 of a0 (2n, 224), as train_slow.hip's tower_forward_kernel lays them out.
template <bool SAMPLE>
__global__ void __launch_bounds__(NT) mb_tower_forward_kernel(const float *__restrict__ patches, const float *__restrict__ planes,
                                                              const mc_train_mb_plane *__restrict__ table, int n_planes,
                                                              const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                              const int32_t *__restrict__ src, const float *__restrict__ prm,
                                                              const float *__restrict__ params, float *__restrict__ xs, float *__restrict__ a0)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x / 3, patch = blockIdx.x - 3 * pair, t = threadIdx.x;
	if (t < PPIX) {
		const int64_t e = (int64_t)blockIdx.x * PPIX + t;   // (pair, patch, pixel) of (n, 3, 11, 11)
		if (SAMPLE) {
			const float v = sample_mb_pixel<PS>(planes, table, n_planes, nnz, n_nnz, rows[pair], src + 2 * (int64_t)pair,
			                                    prm + (int64_t)pair * NPRM, PPIX * patch + t);
			lds[L_X + t] = v;
			xs[e] = v;
		} else {
			lds[L_X + t] = patches[e];
		}
	}
	__syncthreads();
	tower_forward(params, lds);
	if (t < FM) {
		const float v = lds[L_A5 + t];
		float *r0 = a0 + (int64_t)(2 * pair) * NIN, *r1 = r0 + NIN;
		if (patch == 0) {
			r0[t] = v;
			r1[t] = v;
		} else if (patch == 1) {
			r0[FM + t] = v;
		} else {
			r1[FM + t] = v;
		}
	}
}

// Launch 9, block 3 * pair + p.  patches (n_pairs, 3, 11, 11): the given batch, or what launch 1 sampled.  dfeat (2n, 224):
// the gradient of a0.  slab (3n, NCONV): row 3 * pair + p receives the patch's gradients of the convolutions.
__global__ void __launch_bounds__(NT) mb_tower_backward_kernel(const float *__restrict__ patches, const float *__restrict__ params,
                                                               const float *__restrict__ dfeat, float *__restrict__ slab)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x / 3, patch = blockIdx.x - 3 * pair, t = threadIdx.x;
	float *X = lds + L_X, *A1 = lds + L_A1, *A2 = lds + L_A2, *A3 = lds + L_A3, *A4 = lds + L_A4, *A5 = lds + L_A5;
	if (t < PPIX) X[t] = patches[(int64_t)blockIdx.x * PPIX + t];
	__syncthreads();
	tower_forward(params, lds);
	if (t < FM) {   // the gradient of A5, masked by its ReLU; the left patch gets the positive's, then the negative's sample
		const float *r0 = dfeat + (int64_t)(2 * pair) * NIN, *r1 = r0 + NIN;
		const float d = patch == 0 ? r0[t] + r1[t] : patch == 1 ? r0[FM + t] : r1[FM + t];
		A5[t] = A5[t] > 0.f ? d : 0.f;
	}
	__syncthreads();
	float *g = slab + (int64_t)blockIdx.x * NCONV;
	conv_weight_grad<1, FM, S4>(A5, A4, g + off_w(5), g + off_b(5));
	__syncthreads();
	conv_data_grad<1, S4>(params + off_w(5), A5, A4);
	__syncthreads();
	conv_weight_grad<1, FM, S3>(A4, A3, g + off_w(4), g + off_b(4));
	__syncthreads();
	conv_data_grad<1, S3>(params + off_w(4), A4, A3);
	__syncthreads();
	conv_weight_grad<1, FM, S2>(A3, A2, g + off_w(3), g + off_b(3));
	__syncthreads();
	conv_data_grad<1, S2>(params + off_w(3), A3, A2);
	__syncthreads();
	conv_weight_grad<1, FM, S1>(A2, A1, g + off_w(2), g + off_b(2));
	__syncthreads();
	conv_data_grad<1, S1>(params + off_w(2), A2, A1);
	__syncthreads();
	conv_weight_grad<1, 1, S0>(A1, X, g + off_w(1), g + off_b(1));
}

// Launch 10: the convolutions' gradient is the slab's 3 * n_pairs rows summed in the order 3 * pair + p.
__global__ void __launch_bounds__(256) mb_slow_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ gfc, int n_rows,
                                                          float *__restrict__ params, float *__restrict__ moms, float lr, float mom)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NPARAMS) return;
	sgd_update(j, slab, gfc, n_rows, NCONV, params, moms, lr, mom);
}

// ---- the workspace ---------------------------------------------------------------------------------------------------
struct Workspace {
	float *xs;          // (n, 3, 11, 11) sampled patches
	float *a[L2 + 1];   // a[0] (R, 224) the FC input; a[1..3] (R, 384) the hidden Linears' outputs
	float *g[2];        // (R, 384) output gradients of two consecutive Linears
	float *dfeat;       // (R, 224) gradient of a[0]
	float *gfc;         // (NFC) gradient of the FC parameters
	float *slab;        // (3n, NCONV) per-patch gradients of the convolutions
	size_t floats;
};

static Workspace carve(float *base, int n_pairs)
{
	Workspace ws;
	size_t o = 0;
	const size_t R = 2 * (size_t)n_pairs;
	auto take = [&](size_t n) {
		float *p = base + o;
		o += align_up(n, 64);
		return p;
	};
	ws.xs = take((size_t)n_pairs * NPIX);
	ws.a[0] = take(R * NIN);
	for (int l = 1; l <= L2; ++l) ws.a[l] = take(R * NH);
	ws.g[0] = take(R * NH);
	ws.g[1] = take(R * NH);
	ws.dfeat = take(R * NIN);
	ws.gfc = take(NFC);
	ws.slab = take(3 * (size_t)n_pairs * NCONV);
	ws.floats = o;
	return ws;
}

static int prepare_kernels()
{
	static int rc = -1;
	if (rc >= 0) return rc;
	const void *ks[3] = {(const void *)mb_tower_forward_kernel<true>, (const void *)mb_tower_forward_kernel<false>,
	                     (const void *)mb_tower_backward_kernel};
	for (const void *k : ks) {
		const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOWER_LDS_BYTES);
		if (e != hipSuccess) {
			set_error("train_mb_slow: hipFuncSetAttribute(%zu bytes of LDS): %s", TOWER_LDS_BYTES, hipGetErrorString(e));
			return (int)e;
		}
	}
	rc = 0;
	return rc;
}

static int check_step_args(int n_pairs, const float *params, const float *moms, void *ws, size_t ws_bytes)
{
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= MC_TRAIN_MB_SLOW_MAX_PAIRS, "train_mb_slow: n_pairs %d outside [1, %d]", n_pairs,
	           MC_TRAIN_MB_SLOW_MAX_PAIRS);
	MC_REQUIRE(params && moms, "train_mb_slow: null params / momenta");
	MC_REQUIRE(((uintptr_t)params & 15) == 0, "train_mb_slow: params not 16-byte aligned");
	MC_REQUIRE(ws && ws_bytes >= mc_train_mb_slow_workspace_bytes(n_pairs), "train_mb_slow: workspace of %zu bytes, %zu needed", ws_bytes,
	           mc_train_mb_slow_workspace_bytes(n_pairs));
	MC_REQUIRE(((uintptr_t)ws & 15) == 0, "train_mb_slow: workspace not 16-byte aligned");
	return 0;
}

static int check_store_args(const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz)
{
	MC_REQUIRE(planes && table && nnz, "train_mb_slow: null planes / table / nnz pointer");
	MC_REQUIRE(n_planes >= 1, "train_mb_slow: n_planes %d", n_planes);
	MC_REQUIRE(n_nnz >= 1, "train_mb_slow: empty nnz");
	return 0;
}

// one step: patches given (rows == nullptr) or sampled
static int enqueue_step(const float *patches, const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz,
                        int64_t n_nnz, const int32_t *rows, const int32_t *src, const float *prm, int n_pairs, float *params, float *moms,
                        float lr, float mom, float *loss_out, void *workspace, hipStream_t st)
{
	const Workspace ws = carve((float *)workspace, n_pairs);
	const int R = 2 * n_pairs, mtr = (R + 15) / 16, n_blocks = 3 * n_pairs;
	if (patches)
		mb_tower_forward_kernel<false><<<n_blocks, NT, TOWER_LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
		                                                                      ws.xs, ws.a[0]);
	else
		mb_tower_forward_kernel<true><<<n_blocks, NT, TOWER_LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
		                                                                     ws.xs, ws.a[0]);
	if (int rc = check_launch("train_mb_slow tower_forward")) return rc;
	for (int l = 1; l <= L2; ++l) {
		fc_forward_kernel<<<cdiv(mtr * (NH / 16), FC_WAVES), FC_WAVES * 64, 0, st>>>(ws.a[l - 1], fc_in(l), params + off_fw(l), params + off_fb(l),
		                                                                            ws.a[l], R);
		if (int rc = check_launch("train_mb_slow fc_forward")) return rc;
	}
	fc_head_kernel<<<1, HEAD_NT, 0, st>>>(ws.a[L2], params + off_fw(L2 + 1), params + off_fb(L2 + 1), R, ws.g[0],
	                                      ws.gfc + (off_fw(L2 + 1) - NCONV), ws.gfc + (off_fb(L2 + 1) - NCONV), loss_out);
	if (int rc = check_launch("train_mb_slow fc_head")) return rc;
	for (int l = L2; l >= 1; --l) {
		const int K = fc_in(l), tasks = (mtr + NH / 16) * (K / 16) + NH / 64;
		const float *g = ws.g[(L2 - l) & 1];
		float *dw = ws.gfc + (off_fw(l) - NCONV), *db = ws.gfc + (off_fb(l) - NCONV);
		if (l > 1)
			fc_backward_kernel<true><<<cdiv(tasks, FC_WAVES), FC_WAVES * 64, 0, st>>>(g, ws.a[l - 1], K, params + off_fw(l), R, ws.g[(L2 + 1 - l) & 1],
			                                                                         dw, db);
		else   // a[0]'s ReLU mask is applied by the tower, which has the activations
			fc_backward_kernel<false><<<cdiv(tasks, FC_WAVES), FC_WAVES * 64, 0, st>>>(g, ws.a[0], K, params + off_fw(l), R, ws.dfeat, dw, db);
		if (int rc = check_launch("train_mb_slow fc_backward")) return rc;
	}
	mb_tower_backward_kernel<<<n_blocks, NT, TOWER_LDS_BYTES, st>>>(patches ? patches : ws.xs, params, ws.dfeat, ws.slab);
	if (int rc = check_launch("train_mb_slow tower_backward")) return rc;
	mb_slow_sgd_kernel<<<cdiv(NPARAMS, 256), 256, 0, st>>>(ws.slab, ws.gfc, n_blocks, params, moms, lr, mom);
	return check_launch("train_mb_slow sgd");
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_mb_slow_version(void) { return MC_TRAIN_MB_SLOW_ABI_VERSION; }

const char *mc_train_mb_slow_last_error(void) { return last_error(); }

size_t mc_train_mb_slow_workspace_bytes(int n_pairs)
{
	if (n_pairs < 1 || n_pairs > MC_TRAIN_MB_SLOW_MAX_PAIRS) return 0;
	return carve(nullptr, n_pairs).floats * sizeof(float);
}

int mc_train_mb_slow_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float *loss_out,
                                void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_step_args(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "train_mb_slow_step_batch: null pointer");
	if (int rc = prepare_kernels()) return rc;
	return enqueue_step(patches, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, n_pairs, params, moms, lr, mom, loss_out,
	                    workspace, as_stream(stream));
}

int mc_train_mb_slow_run(const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                         const int32_t *perm, int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const int32_t *src, const float *prm,
                         float *params, float *moms, float lr, float mom, float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_store_args(planes, table, n_planes, nnz, n_nnz)) return rc;
	if (int rc = check_step_args(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(perm && src && prm && losses, "train_mb_slow_run: null pointer");
	MC_REQUIRE(n_steps >= 0, "train_mb_slow_run: n_steps %d", n_steps);
	int64_t end;   // t0 + n_steps * n_pairs, saturated: train_range.h
	MC_REQUIRE(train_steps_fit(t0, n_steps, n_pairs, n_perm, &end), "train_mb_slow_run: steps [%lld, %lld) of the permutation exceed its %lld rows",
	           (long long)t0, (long long)end, (long long)n_perm);
	if (int rc = prepare_kernels()) return rc;
	const hipStream_t st = as_stream(stream);
	for (int s = 0; s < n_steps; ++s) {
		const int64_t first = (int64_t)s * n_pairs;
		if (int rc = enqueue_step(nullptr, planes, table, n_planes, nnz, n_nnz, perm + t0 + first, src + 2 * first, prm + first * NPRM, n_pairs,
		                          params, moms, lr, mom, losses + s, workspace, st))
			return rc;
	}
	return 0;
}

}  // extern "C"
