// Training of the accurate architecture on Middlebury (main.lua:116-130, 602-890, `mb slow`: -l1 5 -fm 112 -l2 3 -nh2 384) on
// gfx950: libmctrainmbslow.so (include/mc_train_mb_slow.h).
//
// The step is train_slow.hip's (train_slow_conv.h and train_slow_fc.h state it once for both) with five valid 3x3
// convolutions on 11 x 11 patches, three hidden Linears and the ragged image store of train_mb.hip.  A pair's activations are 221 KB and do not fit a CU's LDS; ONE PATCH's are 74 KB, so
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
// The GEMMs and the layer chain are train_slow_conv.h's with one patch per workgroup, the FC kernels, the update, the workspace
// and the FC launches train_slow_fc.h's, the sampler train_mb_sampler.h's: this file holds the net, its tower and update
// kernels and the entry points.
#include "mc_common.h"
#include "../../include/mc_train_mb_slow.h"
#include "train_mb_sampler.h"
#include "train_slow_conv.h"
#define MC_FC_HEAD_MAX_ROWS (2 * MC_TRAIN_MB_SLOW_MAX_PAIRS)
#include "train_slow_fc.h"

namespace mc {

struct Net {
	static constexpr int FM = MC_TRAIN_MB_SLOW_FM, PS = MC_TRAIN_MB_SLOW_WS, NL = MC_TRAIN_MB_SLOW_L1, NP = 1, L2 = MC_TRAIN_MB_SLOW_L2,
	                     MAX_PAIRS = MC_TRAIN_MB_SLOW_MAX_PAIRS;
	static constexpr const char *PREFIX = "train_mb_slow";
};
constexpr int PS = Net::PS;
constexpr int NPRM = MC_TRAIN_MB_SLOW_NPRM;
constexpr int NCONV = MC_TRAIN_MB_SLOW_NCONV;
constexpr int NFC = MC_TRAIN_MB_SLOW_NFC;
constexpr int NPARAMS = MC_TRAIN_MB_SLOW_NPARAMS;
constexpr int PPIX = PS * PS;            // floats of a patch
static_assert(MC_TRAIN_MB_SLOW_WS == MC_TRAIN_MB_WS && NPRM == MC_TRAIN_MB_NPRM && NPRM == MC_TRAIN_NPRM, "the sampler's patch and parameter layout");
static_assert(NH == MC_TRAIN_MB_SLOW_NH2 && PPIX <= NT && FM <= NT, "train_slow_fc.h's hidden units; one thread per patch pixel and per feature");

// the flat parameter buffer: w1 b1 .. w5 b5 | fw1 fb1 fw2 fb2 fw3 fb3 fw4 fb4
static_assert(off_b<Net>(Net::NL) + FM == NCONV && n_conv<Net>() == NCONV && NCONV == 453152, "convolution parameter layout");
static_assert(off_fb<Net>(Net::L2 + 1) + 1 == NPARAMS && n_params<Net>() == NPARAMS && NCONV + NFC == NPARAMS && NPARAMS == 835617, "parameter layout");
static_assert(fc_weights_aligned<Net>(), "float4 loads of the FC weights");

// LDS of the tower kernels, ONE patch's activations: X [121] in 128 floats, A1 [112][81], A2 [112][49], A3 [112][25], A4 [112][9], A5 [112]
constexpr int L_A5 = lds_act<Net>(Net::NL);
constexpr size_t LDS_BYTES = TOWER_LDS_BYTES<Net>;
static_assert(TOWER_LDS_FLOATS<Net> == 18608 && LDS_BYTES == 74432 && 2 * LDS_BYTES <= 160 * 1024 && lds_act<Net>(1) == 128,
              "two patches' workgroups fit a CU's 160 KiB of LDS");

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
			lds[t] = v;
			xs[e] = v;
		} else {
			lds[t] = patches[e];
		}
	}
	__syncthreads();
	tower_forward<Net>(params, lds);
	if (t < FM) scatter_feature(a0, pair, patch, t, lds[L_A5 + t]);
}

// Launch 9, block 3 * pair + p.  patches (n_pairs, 3, 11, 11): the given batch, or what launch 1 sampled.  dfeat (2n, 224):
// the gradient of a0.  slab (3n, NCONV): row 3 * pair + p receives the patch's gradients of the convolutions.
__global__ void __launch_bounds__(NT) mb_tower_backward_kernel(const float *__restrict__ patches, const float *__restrict__ params,
                                                               const float *__restrict__ dfeat, float *__restrict__ slab)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x / 3, patch = blockIdx.x - 3 * pair, t = threadIdx.x;
	float *A5 = lds + L_A5;
	if (t < PPIX) lds[t] = patches[(int64_t)blockIdx.x * PPIX + t];
	__syncthreads();
	tower_forward<Net>(params, lds);
	if (t < FM) {   // the gradient of A5, masked by its ReLU
		const float d = gather_feature_grad(dfeat, pair, patch, t);
		A5[t] = A5[t] > 0.f ? d : 0.f;
	}
	__syncthreads();
	tower_backward<Net>(params, slab + (int64_t)blockIdx.x * NCONV, lds);
}

// Launch 10: the convolutions' gradient is the slab's 3 * n_pairs rows summed in the order 3 * pair + p.
__global__ void __launch_bounds__(256) mb_slow_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ gfc, int n_rows,
                                                          float *__restrict__ params, float *__restrict__ moms, float lr, float mom)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= NPARAMS) return;
	sgd_update(j, slab, gfc, n_rows, NCONV, params, moms, lr, mom);
}

static int prepare_tower_kernels()
{
	return prepare_kernels(Net::PREFIX, {(const void *)mb_tower_forward_kernel<true>, (const void *)mb_tower_forward_kernel<false>,
	                                     (const void *)mb_tower_backward_kernel}, LDS_BYTES);
}

// one step: patches given (rows == nullptr) or sampled
static int enqueue_step(const float *patches, const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz,
                        int64_t n_nnz, const int32_t *rows, const int32_t *src, const float *prm, int n_pairs, float *params, float *moms,
                        float lr, float mom, float *loss_out, void *workspace, hipStream_t st)
{
	const Workspace<Net> ws = carve<Net>((float *)workspace, n_pairs);
	const int n_blocks = 3 * n_pairs;
	if (patches)
		mb_tower_forward_kernel<false><<<n_blocks, NT, LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
		                                                                ws.xs, ws.a[0]);
	else
		mb_tower_forward_kernel<true><<<n_blocks, NT, LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
		                                                               ws.xs, ws.a[0]);
	if (int rc = check_launch("train_mb_slow tower_forward")) return rc;
	if (int rc = enqueue_fc(ws, params, n_pairs, loss_out, st)) return rc;
	mb_tower_backward_kernel<<<n_blocks, NT, LDS_BYTES, st>>>(patches ? patches : ws.xs, params, ws.dfeat, ws.slab);
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
	return step_workspace_bytes<Net>(n_pairs);
}

int mc_train_mb_slow_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float *loss_out,
                                void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_step_args<Net>(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "train_mb_slow_step_batch: null pointer");
	if (int rc = prepare_tower_kernels()) return rc;
	return enqueue_step(patches, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, n_pairs, params, moms, lr, mom, loss_out,
	                    workspace, as_stream(stream));
}

int mc_train_mb_slow_run(const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                         const int32_t *perm, int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const int32_t *src, const float *prm,
                         float *params, float *moms, float lr, float mom, float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_store_args(Net::PREFIX, planes, table, n_planes, nnz, n_nnz)) return rc;
	if (int rc = check_step_args<Net>(n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	const hipStream_t st = as_stream(stream);
	return run_steps(Net::PREFIX, perm && src && prm && losses, t0, n_steps, n_pairs, n_perm, prepare_tower_kernels, [&](int s, int64_t first) {
		return enqueue_step(nullptr, planes, table, n_planes, nnz, n_nnz, perm + t0 + first, src + 2 * first, prm + first * NPRM, n_pairs, params,
		                    moms, lr, mom, losses + s, workspace, st);
	});
}

}  // extern "C"
