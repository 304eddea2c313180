// Training of the fast architecture on Middlebury (main.lua:602-890, `mb fast`: -l1 5 -fm 64) on gfx950: libmctrainmb.so.
//
// The step is the fast net's of train_fast.h, which states the net, the kernels' bodies and the host side of a step once for
// libmctrain.so, this library and libmctraindepth.so, with five valid 3x3 convolutions on 11 x 11 patches
// (11 -> 9 -> 7 -> 5 -> 3 -> 1) and a ragged image store (include/mc_train_mb.h).  TWO kernels:
//   (a) train_mb_step_kernel: one workgroup of 8 waves per pair; the pair's three patches are sampled from their planes into
//       LDS (or copied from given patches), forward, Normalize2 / StereoJoin1 / Margin2, backward with every activation in
//       LDS; the pair's gradients go to its own slab row.
//   (b) train_mb_sgd_kernel: sums the slab in pair order, v = mom * v - lr * g; w += v, and the mean loss.
// The GEMMs are train_conv.h's (fp32 v_mfma_f32_32x32x2_f32), the sampler is train_sampler.h's with patch size 11.
//
// LDS: all three patches' activations of all five layers plus the split-K area, 40 256 floats = 161 024 bytes (157.25 KiB)
// of the CU's 163 840: one workgroup per CU.  The split area cannot alias an activation: it is used in the forward pass of
// layers 4 and 5, where every earlier activation is still needed by the backward pass.
//
// Tiles: output columns N per GEMM, padded to 32 (this file) or to 16 (the 16x16x4 tiles of train_slow.hip):
//   forward  layer 1..5:   N = 243 147 75 27 3  -> 256 160 96 32 32  |  256 160 80 32 16
//   data     layer 5..2:   N = 27 75 147 243    -> 32 96 160 256     |  32 80 160 256
//   weights  every layer:  N = 576 = 18 * 32, no padding either way; K = 3 * pixels pads to 2 or 4, the same 4 28 76 148 244.
// The narrow tiles save 16 of 96 columns in two GEMMs (layer 3 forward, layer 4 data gradient) and 16 of 32 in layer 5's
// forward (3 columns; 0.4 % of the step's multiply-adds), at the same FLOPs per cycle but twice the operand loads per FLOP -- and the
// operands (weights from L2, activations from LDS) are what these GEMMs wait for.  So every GEMM uses the 32 x 32 x 2 tile.
// K is split over four waves where a GEMM has only two output tiles: forward of layers 4 and 5, data gradient of layer 5.
#include "mc_common.h"
#include "../../include/mc_train_mb.h"
#include "train_fast.h"   // the fast net, its kernels' bodies (the sampler is train_mb_sampler.h's), the host side of a step

namespace mc {

struct Lib {
	static constexpr const char *PREFIX = "train_mb";
	static constexpr int MAX_PAIRS = MC_TRAIN_MB_MAX_PAIRS;
};
using Net = FastNet<MC_TRAIN_MB_L1, Lib>;
static_assert(Net::FM == MC_TRAIN_MB_FM && Net::PS == MC_TRAIN_MB_WS && NPRM == MC_TRAIN_MB_NPRM && Net::SAMPLE_NT == 384, "the net of mc_train_mb.h");
static_assert(Net::NPARAMS == MC_TRAIN_MB_NPARAMS && off_b<Net>(Net::NL) + FM == Net::NPARAMS, "parameter layout: w1 b1 w2 b2 ... w5 b5");
// LDS: X [3][121] in 384 floats, A1 [3][64][81], A2 [3][64][49], A3 [3][64][25], A4 [3][64][9], A5 [3][64], the partial tiles
static_assert(Net::NPIX <= lds_act<Net>(1) && lds_act<Net>(1) == 384 && Net::NPIX <= NT, "the patches' slot, one thread per patch pixel");
static_assert(Net::LDS_BYTES == 161024 && Net::LDS_BYTES <= 160 * 1024, "a CU has 160 KiB of LDS");

__global__ void __launch_bounds__(384) train_mb_sample_kernel(const float *__restrict__ planes, const mc_train_mb_plane *__restrict__ table,
                                                              int n_planes, const float *__restrict__ nnz, int64_t n_nnz,
                                                              const int32_t *__restrict__ rows, const int32_t *__restrict__ src,
                                                              const float *__restrict__ prm, float *__restrict__ out)
{
	write_patches<Net, RaggedStore>(out, planes, table, n_planes, nnz, n_nnz, rows, src, prm);
}

// Kernel (a): one workgroup per pair.  SAMPLE: the patches come from the planes (rows[pair] of nnz, src and prm of the
// pair); otherwise from patches (n_pairs, 3, 11, 11).  Writes the pair's gradients to slab[pair], its loss to losses[pair].
template <bool SAMPLE>
__global__ void __launch_bounds__(NT) train_mb_step_kernel(const float *__restrict__ patches, const float *__restrict__ planes,
                                                           const mc_train_mb_plane *__restrict__ table, int n_planes,
                                                           const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                           const int32_t *__restrict__ src, const float *__restrict__ prm,
                                                           const float *__restrict__ params, float margin, int pow, float inv_pairs,
                                                           float *__restrict__ slab, float *__restrict__ losses)
{
	step_of_pair<Net, SAMPLE, RaggedStore>(patches, params, margin, pow, inv_pairs, slab, losses, planes, table, n_planes, nnz, n_nnz, rows, src, prm);
}

// Kernel (b): g = sum over pairs in order; v = mom * v - lr * g; w += v.  Block 0 also writes the mean loss.
__global__ void __launch_bounds__(256) train_mb_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ pair_losses, int n_pairs,
                                                           float *__restrict__ params, float *__restrict__ moms, float lr, float mom,
                                                           float *__restrict__ loss_out)
{
	slab_sgd(slab, pair_losses, n_pairs, Net::NPARAMS, params, moms, lr, mom, loss_out);
}

static int prepare_step_kernels()
{
	return raise_lds_limit<Net>({(const void *)train_mb_step_kernel<true>, (const void *)train_mb_step_kernel<false>});
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_mb_version(void) { return MC_TRAIN_MB_ABI_VERSION; }

const char *mc_train_mb_last_error(void) { return last_error(); }

size_t mc_train_mb_workspace_bytes(int n_pairs)
{
	return step_workspace_bytes<Net>(n_pairs);
}

int mc_train_mb_sample(const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                       const int32_t *rows, const int32_t *src, const float *prm, int n_pairs, float *out, void *stream)
{
	if (int rc = check_store_args(Net::PREFIX, planes, table, n_planes, nnz, n_nnz)) return rc;
	return sample_patches<Net, train_mb_sample_kernel>("train_mb_sample", n_pairs, rows && src && prm && out, stream, planes, table, n_planes, nnz,
	                                                   n_nnz, rows, src, prm, out);
}

int mc_train_mb_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow,
                           float *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
	return step_batch<Net, train_mb_step_kernel<false>, train_mb_sgd_kernel>(prepare_step_kernels, patches, n_pairs, params, moms, lr, mom, margin,
	                                                                          pow, loss_out, workspace, workspace_bytes, stream, nullptr, nullptr, 0,
	                                                                          nullptr, 0, nullptr, nullptr, nullptr);
}

int mc_train_mb_run(const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                    const int32_t *perm, int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const int32_t *src, const float *prm,
                    float *params, float *moms, float lr, float mom, float margin, int pow, float *losses, void *workspace,
                    size_t workspace_bytes, void *stream)
{
	if (int rc = check_store_args(Net::PREFIX, planes, table, n_planes, nnz, n_nnz)) return rc;
	if (int rc = check_step_args<Net>(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
	const hipStream_t st = as_stream(stream);
	return run_steps(Net::PREFIX, perm && src && prm && losses, t0, n_steps, n_pairs, n_perm, prepare_step_kernels, [&](int s, int64_t first) {
		return enqueue_step<Net, train_mb_step_kernel<true>, train_mb_sgd_kernel>(n_pairs, params, moms, lr, mom, margin, pow, losses + s, workspace, st,
		                                                                           nullptr, planes, table, n_planes, nnz, n_nnz, perm + t0 + first,
		                                                                           src + 2 * first, prm + first * NPRM);
	});
}

}  // extern "C"
