// Training of the fast architecture (main.lua:602-890, arch fast on kitti / kitti2015) on gfx950: libmctrain.so.
//
// A step of the reference is ~15 cuDNN / THC launches (make_patch on the host, copy, forward of 4 convolutions, 3 ReLUs,
// Normalize2, StereoJoin1, Margin2, and their backward passes, then 16 tensor updates).  The work is tiny (~2 GFLOP for
// bs = 128), so here a step is TWO kernels:
//   (a) train_step_kernel: one workgroup per training pair.  It samples the pair's three distinct patches (left,
//       positive, negative; patches 4i-3 and 4i-1 of the reference's batch are drawn with identical arguments,
//       main.lua:843,845) straight from the device-resident images into LDS, runs the forward pass, Normalize2,
//       StereoJoin1, Margin2 and the whole backward pass with every activation in LDS, and writes the pair's weight and
//       bias gradients to its own row of a slab (no float atomics).
//   (b) train_sgd_kernel: sums the slab's rows in a fixed order (pair 0, 1, ...), applies  v = mom * v - lr * g;
//       w += v  (main.lua:870-874) and writes the step's mean loss.  The fixed order makes a run bitwise reproducible.
// The convolution GEMMs run on v_mfma_f32_32x32x2_f32 (fp32 in, fp32 accumulate -- the reference's precision):
//   forward  out[co, p]      = sum_{ci,tap} W[co, ci, tap] * in[ci, p + tap]          (M = 64, N = pixels, K = 576)
//   weights  dW[co, ci, tap] = sum_p g[co, p] * in[ci, p + tap]                        (M = 64, N = 576, K = pixels)
//   data     dX[ci, q]       = sum_{co,tap} W[co, ci, tap] * g[co, q - tap]  (masked by ReLU)  (M = 64, N = pixels, K = 576)
// The weights are read from global memory (L2-resident: 445 KB), the activations from LDS.  dX overwrites the
// activation it is masked by, in place: a layer's activations are dead once its weight gradient is taken.
// GEMMs with only two 32 x 32 output tiles (layer 3 / 4 forward, layer 4 data gradient) split K over four waves and
// add the partial tiles in a fixed order.
// The GEMMs, the layer chain, the LDS layout and the update are train_conv.h's; the net, the kernels' bodies, the launches of a
// step and the checks of the entry points are train_fast.h's, which states them once for this library, libmctrainmb.so and
// libmctraindepth.so; the run driver is train_net.h's.  This file holds the library's tag, its pinned layout, its kernels'
// entries and its entry points.
#include "mc_common.h"
#include "../../include/mc_train.h"
#include "train_fast.h"   // the fast net, its kernels' bodies, the host side of a step

namespace mc {

struct Lib {
	static constexpr const char *PREFIX = "train";
	static constexpr int MAX_PAIRS = MC_TRAIN_MAX_PAIRS;
};
using Net = FastNet<MC_TRAIN_L1, Lib>;
static_assert(Net::FM == MC_TRAIN_FM && Net::PS == MC_TRAIN_WS && NPRM == MC_TRAIN_NPRM && Net::SAMPLE_NT == 256, "the net of mc_train.h");
static_assert(Net::NPARAMS == MC_TRAIN_NPARAMS && off_b<Net>(4) + FM == Net::NPARAMS, "parameter layout: w1 b1 w2 b2 w3 b3 w4 b4");
// LDS: X [3][81] in 256 floats, A1 [3][64][49], A2 [3][64][25], A3 [3][64][9], A4 [3][64], the partial tiles [8][16][64]
static_assert(Net::LDS_BYTES == 98304 && lds_act<Net>(1) == 256, "the LDS layout");

__global__ void __launch_bounds__(256) train_sample_kernel(const float *__restrict__ x0, const float *__restrict__ x1, int n_img, int H, int W,
                                                           const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                           const float *__restrict__ prm, float *__restrict__ out)
{
	write_patches<Net, ImageStore>(out, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm);
}

// Kernel (a): one workgroup per pair.  SAMPLE: the patches come from the images (rows[pair] of nnz, prm of the pair);
// otherwise from patches (n_pairs, 3, 9, 9).  Writes the pair's gradients to slab[pair] and its loss to losses[pair].
template <bool SAMPLE>
__global__ void __launch_bounds__(NT) train_step_kernel(const float *__restrict__ patches,
                                                        const float *__restrict__ x0, const float *__restrict__ x1, int n_img, int H, int W,
                                                        const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                        const float *__restrict__ prm, const float *__restrict__ params,
                                                        float margin, int pow, float inv_pairs, float *__restrict__ slab, float *__restrict__ losses)
{
	step_of_pair<Net, SAMPLE, ImageStore>(patches, params, margin, pow, inv_pairs, slab, losses, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm);
}

// Kernel (b): g = sum over pairs in order; v = mom * v - lr * g; w += v.  Block 0 also writes the mean loss.
__global__ void __launch_bounds__(256) train_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ pair_losses, int n_pairs,
                                                        float *__restrict__ params, float *__restrict__ moms, float lr, float mom,
                                                        float *__restrict__ loss_out)
{
	slab_sgd(slab, pair_losses, n_pairs, Net::NPARAMS, params, moms, lr, mom, loss_out);
}

static int prepare_step_kernels()
{
	return raise_lds_limit<Net>({(const void *)train_step_kernel<true>, (const void *)train_step_kernel<false>});
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_version(void) { return MC_TRAIN_ABI_VERSION; }

const char *mc_train_last_error(void) { return last_error(); }

size_t mc_train_workspace_bytes(int n_pairs)
{
	return step_workspace_bytes<Net>(n_pairs);
}

int mc_train_sample(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *rows,
                    const float *prm, int n_pairs, float *out, void *stream)
{
	if (int rc = check_image_args(Net::PREFIX, x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
	return sample_patches<Net, train_sample_kernel>("train_sample", n_pairs, rows && prm && out, stream, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm,
	                                                out);
}

int mc_train_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow,
                        float *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
	return step_batch<Net, train_step_kernel<false>, train_sgd_kernel>(prepare_step_kernels, patches, n_pairs, params, moms, lr, mom, margin, pow,
	                                                                    loss_out, workspace, workspace_bytes, stream, nullptr, nullptr, 0, 0, 0,
	                                                                    nullptr, 0, nullptr, nullptr);
}

int mc_train_run(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *perm,
                 int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const float *prm, float *params, float *moms, float lr, float mom,
                 float margin, int pow, float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_image_args(Net::PREFIX, x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
	if (int rc = check_step_args<Net>(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
	const hipStream_t st = as_stream(stream);
	return run_steps(Net::PREFIX, perm && prm && losses, t0, n_steps, n_pairs, n_perm, prepare_step_kernels, [&](int s, int64_t first) {
		return enqueue_step<Net, train_step_kernel<true>, train_sgd_kernel>(n_pairs, params, moms, lr, mom, margin, pow, losses + s, workspace, st,
		                                                                     nullptr, x0, x1, n_img, H, W, nnz, n_nnz, perm + t0 + first,
		                                                                     prm + first * NPRM);
	});
}

}  // extern "C"
