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
// train_mb_slow.hip (Middlebury's accurate net, one patch per workgroup), and so are the layer chain, the LDS layout, the
// workspace and the FC launches, which those two headers derive from the net described below.  This file holds the net, its
// tower and update kernels and the entry points.
#include "mc_common.h"
#include "../../include/mc_train_slow.h"
#include "train_sampler.h"
#include "train_slow_conv.h"   // block_gemm, the three convolution GEMMs and the towers' layer chain, here with a pair's three patches per workgroup
#define MC_FC_HEAD_MAX_ROWS (2 * MC_TRAIN_SLOW_MAX_PAIRS)
#include "train_slow_fc.h"     // fc_forward_kernel, fc_head_kernel, fc_backward_kernel, sgd_update, the workspace, the FC launches

namespace mc {

struct Net {
	static constexpr int FM = MC_TRAIN_SLOW_FM, PS = MC_TRAIN_SLOW_WS, NL = MC_TRAIN_SLOW_L1, NP = 3, L2 = MC_TRAIN_SLOW_L2, MAX_PAIRS = MC_TRAIN_SLOW_MAX_PAIRS;
	static constexpr const char *PREFIX = "train_slow";
};
constexpr int NPRM = MC_TRAIN_SLOW_NPRM;
constexpr int NCONV = MC_TRAIN_SLOW_NCONV;
constexpr int NFC = MC_TRAIN_SLOW_NFC;
constexpr int NPARAMS = MC_TRAIN_SLOW_NPARAMS;
constexpr int NPIX = 3 * WS * WS;        // floats of a pair's patches
static_assert(MC_TRAIN_SLOW_WS == WS && MC_TRAIN_SLOW_NPRM == MC_TRAIN_NPRM, "the sampler's patch and parameter layout");
static_assert(NH == MC_TRAIN_SLOW_NH2 && FM % 16 == 0 && NH % 16 == 0, "train_slow_fc.h's hidden units; 16 x 16 tiles");

// the flat parameter buffer: w1 b1 w2 b2 w3 b3 w4 b4 | fw1 fb1 .. fw4 fb4 fw5 fb5
static_assert(n_conv<Net>() == NCONV && off_b<Net>(4) + FM == NCONV, "convolution parameter layout");
static_assert(off_fb<Net>(5) + 1 == NPARAMS && n_params<Net>() == NPARAMS && NCONV + NFC == NPARAMS && NPARAMS == 870449, "parameter layout");
static_assert(fc_weights_aligned<Net>(), "float4 loads of the FC weights");

// LDS of the tower kernels: X [3][81] in 256 floats, A1 [3][112][49], A2 [3][112][25], A3 [3][112][9], A4 [3][112]
constexpr int L_A4 = lds_act<Net>(Net::NL);
constexpr size_t LDS_BYTES = TOWER_LDS_BYTES<Net>;
static_assert(LDS_BYTES == 113920 && LDS_BYTES <= 160 * 1024 && lds_act<Net>(1) == 256, "one pair's activations fit a CU's LDS");

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
			lds[t] = v;
			xs[(int64_t)pair * NPIX + t] = v;
		} else {
			lds[t] = patches[(int64_t)pair * NPIX + t];
		}
	}
	__syncthreads();
	tower_forward<Net>(params, lds);
	if (t < 3 * FM) scatter_feature(a0, pair, t / FM, t % FM, lds[L_A4 + t]);
}

// Launch 11.  patches (n_pairs, 3, 9, 9): the given batch, or what launch 1 sampled.  dfeat (2n, 224): the gradient of a0.
__global__ void __launch_bounds__(NT) tower_backward_kernel(const float *__restrict__ patches, const float *__restrict__ params,
                                                            const float *__restrict__ dfeat, float *__restrict__ slab)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x, t = threadIdx.x;
	float *A4 = lds + L_A4;
	if (t < NPIX) lds[t] = patches[(int64_t)pair * NPIX + t];
	__syncthreads();
	tower_forward<Net>(params, lds);
	if (t < 3 * FM) {   // the gradient of A4, masked by its ReLU
		const float d = gather_feature_grad(dfeat, pair, t / FM, t % FM);
		A4[t] = A4[t] > 0.f ? d : 0.f;
	}
	__syncthreads();
	tower_backward<Net>(params, slab + (int64_t)pair * NCONV, lds);
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

static int prepare_tower_kernels()
{
	return prepare_kernels(Net::PREFIX, {(const void *)tower_forward_kernel<true>, (const void *)tower_forward_kernel<false>,
	                                     (const void *)tower_backward_kernel}, LDS_BYTES);
}

// one step: patches given (rows == nullptr) or sampled
static int enqueue_step(const float *patches, const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz,
                        const int32_t *rows, const float *prm, int n_pairs, float *params, float *moms, float lr, float mom, float *loss_out,
                        void *workspace, hipStream_t st)
{
	const Workspace<Net> ws = carve<Net>((float *)workspace, n_pairs);
	if (patches)
		tower_forward_kernel<false><<<n_pairs, NT, LDS_BYTES, st>>>(patches, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, params, ws.xs, ws.a[0]);
	else
		tower_forward_kernel<true><<<n_pairs, NT, LDS_BYTES, st>>>(patches, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, params, ws.xs, ws.a[0]);
	if (int rc = check_launch("train_slow tower_forward")) return rc;
	if (int rc = enqueue_fc(ws, params, n_pairs, loss_out, st)) return rc;
	tower_backward_kernel<<<n_pairs, NT, LDS_BYTES, st>>>(patches ? patches : ws.xs, params, ws.dfeat, ws.slab);
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
	return step_workspace_bytes<Net>(n_pairs);
}

int mc_train_slow_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float *loss_out,
                             void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_step_args<Net>(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "train_slow_step_batch: null pointer");
	if (int rc = prepare_tower_kernels()) return rc;
	return enqueue_step(patches, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr, n_pairs, params, moms, lr, mom, loss_out, workspace,
	                    as_stream(stream));
}

int mc_train_slow_run(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *perm,
                      int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const float *prm, float *params, float *moms, float lr, float mom,
                      float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_image_args(Net::PREFIX, x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
	if (int rc = check_step_args<Net>(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	const hipStream_t st = as_stream(stream);
	return run_steps(Net::PREFIX, perm && prm && losses, t0, n_steps, n_pairs, n_perm, prepare_tower_kernels, [&](int s, int64_t first) {
		return enqueue_step(nullptr, x0, x1, n_img, H, W, nnz, n_nnz, perm + t0 + first, prm + first * NPRM, n_pairs, params, moms, lr, mom,
		                    losses + s, workspace, st);
	});
}

}  // extern "C"
