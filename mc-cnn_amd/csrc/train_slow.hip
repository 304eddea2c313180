// Training of the accurate architecture (main.lua:663-677, 753-875, arch slow on kitti / kitti2015) on gfx950:
// libmctrainslow.so (include/mc_train_slow.h).
//
// A step is TWELVE launches, all on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate; 112 = 7 x 16 rows fill its tiles
// exactly, where 32x32x2 would pad M to 128):
//    1  tower_forward_kernel   one workgroup per pair: the pair's three patches (sampled from the images, or given)
//                              through the four convolutions with every activation in LDS (113 920 bytes); writes the two
//                              rows [feat(left) | feat(positive)], [feat(left) | feat(negative)] of the FC stack's input
//  2-5  fc_forward_kernel      A_l = ReLU(A_{l-1} W_l^T + b_l) over the 2 * n_pairs rows, one wave per 16 x 16 tile
//    6  fc_head_kernel         the last Linear (384 -> 1), Sigmoid, BCECriterion2, their backward passes, the last Linear's
//                              gradients and the gradient of A_4
// 7-10  fc_backward_kernel     per hidden Linear, in one launch: the data gradient G_{l-1} = (G_l W_l) masked by ReLU, the
//                              weight gradient dW_l = G_l^T A_{l-1} (the batch is K, summed in row order inside one wave) and
//                              the bias gradient (column sums in row order)
//   11  tower_backward_kernel  one workgroup per pair: RECOMPUTES the forward pass from the pair's patches (24 MFLOP; saving
//                              the activations instead would write and read back 111 KB per pair and need the same LDS
//                              layout anyway), then the backward pass as in train.hip; the convolutions' gradients go to
//                              the pair's row of a slab (no float atomics)
//   12  sgd_kernel             sums the slab's rows in pair order, takes the FC gradients as they are, applies
//                              v = mom * v - lr * g;  w += v  to all 870 449 parameters
// The launch count is above the ~10 the design aimed for: the four hidden Linears' forward and backward GEMMs each need
// the whole previous layer, and a device-wide barrier inside one kernel was not worth its risk.
// The GEMMs of the towers are train_slow_conv.h's, the FC kernels and the update train_slow_fc.h's: both are shared with
// train_mb_slow.hip (Middlebury's accurate net, one patch per workgroup).  This file holds the layer chain, the LDS layout, the
// workspace and the entry points.
#include "mc_common.h"
#include "../../include/mc_train_slow.h"
#include "train_sampler.h"
#include "train_range.h"
#include "train_slow_conv.h"   // block_gemm and the three convolution GEMMs, here with a pair's three patches per workgroup
#define MC_FC_HEAD_MAX_ROWS (2 * MC_TRAIN_SLOW_MAX_PAIRS)
#include "train_slow_fc.h"     // fc_forward_kernel, fc_head_kernel, fc_backward_kernel, sgd_update

namespace mc {

constexpr int NIN = 2 * FM;              // columns of the FC stack's input
constexpr int NPRM = MC_TRAIN_SLOW_NPRM;
constexpr int NCONV = MC_TRAIN_SLOW_NCONV;
constexpr int NFC = MC_TRAIN_SLOW_NFC;
constexpr int NPARAMS = MC_TRAIN_SLOW_NPARAMS;
constexpr int NP = 3;                    // patches per tower workgroup: a pair's
constexpr int NPIX = 3 * WS * WS;        // floats of a pair's patches
static_assert(MC_TRAIN_SLOW_WS == WS && MC_TRAIN_SLOW_NPRM == MC_TRAIN_NPRM, "the sampler's patch and parameter layout");
static_assert(FM == MC_TRAIN_SLOW_FM && NH == MC_TRAIN_SLOW_NH2, "train_slow_conv.h's feature maps, train_slow_fc.h's hidden units");
static_assert(FM % 16 == 0 && NH % 16 == 0 && NIN % 16 == 0, "16 x 16 tiles");

// offsets of the flat parameter buffer: w1 b1 w2 b2 w3 b3 w4 b4 | fw1 fb1 .. fw4 fb4 fw5 fb5
constexpr int LAYER_STRIDE = FM * FM * 9 + FM;
__host__ __device__ constexpr int off_w(int l) { return l == 1 ? 0 : FM * 9 + FM + (l - 2) * LAYER_STRIDE; }
__host__ __device__ constexpr int off_b(int l) { return l == 1 ? FM * 9 : off_w(l) + FM * FM * 9; }
__host__ __device__ constexpr int fc_in(int l) { return l == 1 ? NIN : NH; }
__host__ __device__ constexpr int off_fw(int l) { return l == 1 ? NCONV : NCONV + NH * NIN + NH + (l - 2) * (NH * NH + NH); }
__host__ __device__ constexpr int off_fb(int l) { return off_fw(l) + (l == 5 ? NH : NH * fc_in(l)); }
static_assert(off_b(4) + FM == NCONV, "convolution parameter layout");
static_assert(off_fb(5) + 1 == NPARAMS && NCONV + NFC == NPARAMS && NPARAMS == 870449, "parameter layout");
static_assert(off_fw(1) % 4 == 0 && off_fw(2) % 4 == 0 && off_fw(3) % 4 == 0 && off_fw(4) % 4 == 0, "float4 loads of the FC weights");

// LDS layout of the tower kernels (floats): three patches' activations of every layer
constexpr int S0 = 9, S1 = 7, S2 = 5, S3 = 3;
constexpr int L_X = 0;                                  // [3][81]
constexpr int L_A1 = 256;                               // [3][112][49]
constexpr int L_A2 = L_A1 + 3 * FM * S1 * S1;           // [3][112][25]
constexpr int L_A3 = L_A2 + 3 * FM * S2 * S2;           // [3][112][9]
constexpr int L_A4 = L_A3 + 3 * FM * S3 * S3;           // [3][112]
constexpr int L_TOTAL = L_A4 + 3 * FM;
constexpr size_t TOWER_LDS_BYTES = (size_t)L_TOTAL * sizeof(float);
static_assert(TOWER_LDS_BYTES <= 160 * 1024, "one pair's activations fit a CU's LDS");

// the four convolutions of a pair's patches X into A1 .. A4, all in LDS
__device__ __forceinline__ void tower_forward(const float *__restrict__ params, float *lds)
{
	float *X = lds + L_X, *A1 = lds + L_A1, *A2 = lds + L_A2, *A3 = lds + L_A3, *A4 = lds + L_A4;
	conv_forward<NP, 1, S0>(params + off_w(1), params + off_b(1), X, A1);
	__syncthreads();
	conv_forward<NP, FM, S1>(params + off_w(2), params + off_b(2), A1, A2);
	__syncthreads();
	conv_forward<NP, FM, S2>(params + off_w(3), params + off_b(3), A2, A3);
	__syncthreads();
	conv_forward<NP, FM, S3>(params + off_w(4), params + off_b(4), A3, A4);
	__syncthreads();
}

// Launch 1.  SAMPLE: the patches come from the images (rows[pair] of nnz, prm of the pair) and are kept in xs for the
// backward kernel; otherwise from patches (n_pairs, 3, 9, 9).  Writes rows 2 * pair and 2 * pair + 1 of a0 (2n, 224).
template <bool SAMPLE>
__global__ void __launch_bounds__(NT) tower_forward_kernel(const float *__restrict__ patches,
                                                           const float *__restrict__ x0, const float *__restrict__ x1, int n_img, int H, int W,
                                                           const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                           const float *__restrict__ prm, const float *__restrict__ params,
                                                           float *__restrict__ xs, float *__restrict__ a0)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x, t = threadIdx.x;
	if (t < NPIX) {
		if (SAMPLE) {
			const float v = sample_pair_pixel<WS>(x0, x1, n_img, H, W, nnz, n_nnz, rows[pair], prm + (int64_t)pair * NPRM, t);
			lds[L_X + t] = v;
			xs[(int64_t)pair * NPIX + t] = v;
		} else {
			lds[L_X + t] = patches[(int64_t)pair * NPIX + t];
		}
	}
	__syncthreads();
	tower_forward(params, lds);
	if (t < 3 * FM) {
		const int patch = t / FM, c = t - patch * FM;
		const float v = lds[L_A4 + t];
		float *r0 = a0 + (int64_t)(2 * pair) * NIN, *r1 = r0 + NIN;
		if (patch == 0) {
			r0[c] = v;
			r1[c] = v;
		} else if (patch == 1) {
			r0[FM + c] = v;
		} else {
			r1[FM + c] = v;
		}
	}
}

// Launch 11.  patches (n_pairs, 3, 9, 9): the given batch, or what launch 1 sampled.  dfeat (2n, 224): the gradient of a0.
__global__ void __launch_bounds__(NT) tower_backward_kernel(const float *__restrict__ patches, const float *__restrict__ params,
                                                            const float *__restrict__ dfeat, float *__restrict__ slab)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x, t = threadIdx.x;
	float *X = lds + L_X, *A1 = lds + L_A1, *A2 = lds + L_A2, *A3 = lds + L_A3, *A4 = lds + L_A4;
	if (t < NPIX) X[t] = patches[(int64_t)pair * NPIX + t];
	__syncthreads();
	tower_forward(params, lds);
	if (t < 3 * FM) {   // the gradient of A4, masked by its ReLU; the left patch gets the positive's, then the negative's sample
		const int patch = t / FM, c = t - patch * FM;
		const float *r0 = dfeat + (int64_t)(2 * pair) * NIN, *r1 = r0 + NIN;
		const float d = patch == 0 ? r0[c] + r1[c] : patch == 1 ? r0[FM + c] : r1[FM + c];
		A4[t] = A4[t] > 0.f ? d : 0.f;
	}
	__syncthreads();
	float *g = slab + (int64_t)pair * NCONV;
	conv_weight_grad<NP, FM, S3>(A4, A3, g + off_w(4), g + off_b(4));
	__syncthreads();
	conv_data_grad<NP, S3>(params + off_w(4), A4, A3);
	__syncthreads();
	conv_weight_grad<NP, FM, S2>(A3, A2, g + off_w(3), g + off_b(3));
	__syncthreads();
	conv_data_grad<NP, S2>(params + off_w(3), A3, A2);
	__syncthreads();
	conv_weight_grad<NP, FM, S1>(A2, A1, g + off_w(2), g + off_b(2));
	__syncthreads();
	conv_data_grad<NP, S1>(params + off_w(2), A2, A1);
	__syncthreads();
	conv_weight_grad<NP, 1, S0>(A1, X, g + off_w(1), g + off_b(1));
}

// Launch 12: the convolutions' gradient is the slab's rows summed in pair order, the FC stack's is gfc as it is;
// v = mom * v - lr * g; w += v.
__global__ void __launch_bounds__(256) sgd_kernel(const float *__restrict__ slab, const float *__restrict__ gfc, int n_pairs,
                                                  float *__restrict__ params, float *__restrict__ moms, float lr, float mom)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NPARAMS) return;
	sgd_update(j, slab, gfc, n_pairs, NCONV, params, moms, lr, mom);
}

// ---- the workspace ---------------------------------------------------------------------------------------------------
struct Workspace {
	float *xs;        // (n, 3, 9, 9) sampled patches
	float *a[5];      // a[0] (R, 224) the FC input; a[1..4] (R, 384) the hidden Linears' outputs
	float *g[2];      // (R, 384) output gradients of two consecutive Linears
	float *dfeat;     // (R, 224) gradient of a[0]
	float *gfc;       // (NFC) gradient of the FC parameters
	float *slab;      // (n, NCONV) per-pair gradients of the convolutions
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
	for (int l = 1; l <= 4; ++l) ws.a[l] = take(R * NH);
	ws.g[0] = take(R * NH);
	ws.g[1] = take(R * NH);
	ws.dfeat = take(R * NIN);
	ws.gfc = take(NFC);
	ws.slab = take((size_t)n_pairs * NCONV);
	ws.floats = o;
	return ws;
}

static int prepare_kernels()
{
	static int rc = -1;
	if (rc >= 0) return rc;
	const void *ks[3] = {(const void *)tower_forward_kernel<true>, (const void *)tower_forward_kernel<false>, (const void *)tower_backward_kernel};
	for (const void *k : ks) {
		const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOWER_LDS_BYTES);
		if (e != hipSuccess) {
			set_error("train_slow: hipFuncSetAttribute(%zu bytes of LDS): %s", TOWER_LDS_BYTES, hipGetErrorString(e));
			return (int)e;
		}
	}
	rc = 0;
	return rc;
}

static int check_step_args(int n_pairs, const float *params, const float *moms, void *ws, size_t ws_bytes)
{
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= MC_TRAIN_SLOW_MAX_PAIRS, "train_slow: n_pairs %d outside [1, %d]", n_pairs, MC_TRAIN_SLOW_MAX_PAIRS);
	MC_REQUIRE(params && moms, "train_slow: null params / momenta");
	MC_REQUIRE(((uintptr_t)params & 15) == 0, "train_slow: params not 16-byte aligned");
	MC_REQUIRE(ws && ws_bytes >= mc_train_slow_workspace_bytes(n_pairs), "train_slow: workspace of %zu bytes, %zu needed", ws_bytes,
	           mc_train_slow_workspace_bytes(n_pairs));
	MC_REQUIRE(((uintptr_t)ws & 15) == 0, "train_slow: workspace not 16-byte aligned");
	return 0;
}

static int check_image_args(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz)
{
	MC_REQUIRE(x0 && x1 && nnz, "train_slow: null image / nnz pointer");
	MC_REQUIRE(n_img >= 1 && H >= 4 && W >= 4 && (int64_t)n_img * H * W < ((int64_t)1 << 40), "train_slow: bad image dims %d x %d x %d", n_img, H, W);
	MC_REQUIRE(H < 32768 && W < 32768, "train_slow: images of %d x %d exceed the warp's 16-bit coordinates", H, W);
	MC_REQUIRE(n_nnz >= 1, "train_slow: empty nnz");
	return 0;
}

// one step: patches given (rows == nullptr) or sampled
static int enqueue_step(const float *patches, const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz,
                        const int32_t *rows, const float *prm, int n_pairs, float *params, float *moms, float lr, float mom, float *loss_out,
                        void *workspace, hipStream_t st)
{
	const Workspace ws = carve((float *)workspace, n_pairs);
	const int R = 2 * n_pairs, mtr = (R + 15) / 16;
	if (patches)
		tower_forward_kernel<false><<<n_pairs, NT, TOWER_LDS_BYTES, st>>>(patches, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, params, ws.xs, ws.a[0]);
	else
		tower_forward_kernel<true><<<n_pairs, NT, TOWER_LDS_BYTES, st>>>(patches, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, params, ws.xs, ws.a[0]);
	if (int rc = check_launch("train_slow tower_forward")) return rc;
	for (int l = 1; l <= 4; ++l) {
		fc_forward_kernel<<<cdiv(mtr * (NH / 16), FC_WAVES), FC_WAVES * 64, 0, st>>>(ws.a[l - 1], fc_in(l), params + off_fw(l), params + off_fb(l),
		                                                                            ws.a[l], R);
		if (int rc = check_launch("train_slow fc_forward")) return rc;
	}
	fc_head_kernel<<<1, HEAD_NT, 0, st>>>(ws.a[4], params + off_fw(5), params + off_fb(5), R, ws.g[0], ws.gfc + (off_fw(5) - NCONV),
	                                      ws.gfc + (off_fb(5) - NCONV), loss_out);
	if (int rc = check_launch("train_slow fc_head")) return rc;
	for (int l = 4; l >= 1; --l) {
		const int K = fc_in(l), tasks = (mtr + NH / 16) * (K / 16) + NH / 64;
		const float *g = ws.g[(4 - l) & 1];
		float *dw = ws.gfc + (off_fw(l) - NCONV), *db = ws.gfc + (off_fb(l) - NCONV);
		if (l > 1)
			fc_backward_kernel<true><<<cdiv(tasks, FC_WAVES), FC_WAVES * 64, 0, st>>>(g, ws.a[l - 1], K, params + off_fw(l), R, ws.g[(5 - l) & 1], dw, db);
		else   // a[0]'s ReLU mask is applied by the tower, which has the activations
			fc_backward_kernel<false><<<cdiv(tasks, FC_WAVES), FC_WAVES * 64, 0, st>>>(g, ws.a[0], K, params + off_fw(l), R, ws.dfeat, dw, db);
		if (int rc = check_launch("train_slow fc_backward")) return rc;
	}
	tower_backward_kernel<<<n_pairs, NT, TOWER_LDS_BYTES, st>>>(patches ? patches : ws.xs, params, ws.dfeat, ws.slab);
	if (int rc = check_launch("train_slow tower_backward")) return rc;
	sgd_kernel<<<cdiv(NPARAMS, 256), 256, 0, st>>>(ws.slab, ws.gfc, n_pairs, params, moms, lr, mom);
	return check_launch("train_slow sgd");
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_slow_version(void) { return MC_TRAIN_SLOW_ABI_VERSION; }

const char *mc_train_slow_last_error(void) { return last_error(); }

size_t mc_train_slow_workspace_bytes(int n_pairs)
{
	if (n_pairs < 1 || n_pairs > MC_TRAIN_SLOW_MAX_PAIRS) return 0;
	return carve(nullptr, n_pairs).floats * sizeof(float);
}

int mc_train_slow_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float *loss_out,
                             void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_step_args(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "train_slow_step_batch: null pointer");
	if (int rc = prepare_kernels()) return rc;
	return enqueue_step(patches, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr, n_pairs, params, moms, lr, mom, loss_out, workspace,
	                    as_stream(stream));
}

int mc_train_slow_run(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *perm,
                      int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const float *prm, float *params, float *moms, float lr, float mom,
                      float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_image_args(x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
	if (int rc = check_step_args(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(perm && prm && losses, "train_slow_run: null pointer");
	MC_REQUIRE(n_steps >= 0, "train_slow_run: n_steps %d", n_steps);
	int64_t end;   // t0 + n_steps * n_pairs, saturated: train_range.h
	MC_REQUIRE(train_steps_fit(t0, n_steps, n_pairs, n_perm, &end), "train_slow_run: steps [%lld, %lld) of the permutation exceed its %lld rows",
	           (long long)t0, (long long)end, (long long)n_perm);
	if (int rc = prepare_kernels()) return rc;
	const hipStream_t st = as_stream(stream);
	for (int s = 0; s < n_steps; ++s) {
		const int64_t first = t0 + (int64_t)s * n_pairs;
		if (int rc = enqueue_step(nullptr, x0, x1, n_img, H, W, nnz, n_nnz, perm + first, prm + (int64_t)s * n_pairs * NPRM, n_pairs, params, moms,
		                          lr, mom, losses + s, workspace, st))
			return rc;
	}
	return 0;
}

}  // extern "C"
