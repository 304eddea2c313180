// Training of the fast architecture on Middlebury (main.lua:602-890, `mb fast`: -l1 5 -fm 64) on gfx950: libmctrainmb.so.
//
// The step is train.hip's (train_conv.h states it once for both) with five valid 3x3 convolutions on 11 x 11 patches
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
#include "train_mb_sampler.h"   // sample_mb_pixel: a pair's patches from the ragged store, shared with train_mb_slow.hip
#include "train_conv.h"         // the GEMMs, the step of a net, the update

namespace mc {

struct Net {
	static constexpr int FM = MC_TRAIN_MB_FM, PS = MC_TRAIN_MB_WS, NL = MC_TRAIN_MB_L1, NP = 3, L2 = 0, MAX_PAIRS = MC_TRAIN_MB_MAX_PAIRS;
	static constexpr const char *PREFIX = "train_mb";
};
static_assert(MC_TRAIN_MB_NPRM == MC_TRAIN_NPRM, "the sampler's parameter layout");
constexpr int PS = Net::PS;
constexpr int NPIX = 3 * PS * PS;        // floats of a pair's patches
constexpr int NPRM = MC_TRAIN_MB_NPRM;
constexpr int NPARAMS = MC_TRAIN_MB_NPARAMS;
static_assert(n_conv<Net>() == NPARAMS && off_b<Net>(Net::NL) + FM == NPARAMS, "parameter layout: w1 b1 w2 b2 ... w5 b5");
// LDS: X [3][121] in 384 floats, A1 [3][64][81], A2 [3][64][49], A3 [3][64][25], A4 [3][64][9], A5 [3][64], the partial tiles
constexpr size_t LDS_BYTES = STEP_LDS_BYTES<Net>;
static_assert(NPIX <= lds_act<Net>(1) && lds_act<Net>(1) == 384 && NPIX <= NT, "the patches' slot, one thread per patch pixel");
static_assert(LDS_BYTES == 161024 && LDS_BYTES <= 160 * 1024, "a CU has 160 KiB of LDS");

__global__ void __launch_bounds__(384) train_mb_sample_kernel(const float *__restrict__ planes, const mc_train_mb_plane *__restrict__ table,
                                                              int n_planes, const float *__restrict__ nnz, int64_t n_nnz,
                                                              const int32_t *__restrict__ rows, const int32_t *__restrict__ src,
                                                              const float *__restrict__ prm, float *__restrict__ out)
{
	const int pair = blockIdx.x, t = threadIdx.x;
	if (t < NPIX)
		out[(int64_t)pair * NPIX + t] = sample_mb_pixel<PS>(planes, table, n_planes, nnz, n_nnz, rows[pair], src + 2 * (int64_t)pair,
		                                                    prm + (int64_t)pair * NPRM, t);
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
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x, t = threadIdx.x;
	if (t < NPIX) {
		if (SAMPLE)
			lds[t] = sample_mb_pixel<PS>(planes, table, n_planes, nnz, n_nnz, rows[pair], src + 2 * (int64_t)pair, prm + (int64_t)pair * NPRM, t);
		else
			lds[t] = patches[(int64_t)pair * NPIX + t];
	}
	__syncthreads();
	pair_step<Net>(params, margin, pow, inv_pairs, lds, slab + (int64_t)pair * NPARAMS, losses + pair);
}

// Kernel (b): g = sum over pairs in order; v = mom * v - lr * g; w += v.  Block 0 also writes the mean loss.
__global__ void __launch_bounds__(256) train_mb_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ pair_losses, int n_pairs,
                                                           float *__restrict__ params, float *__restrict__ moms, float lr, float mom,
                                                           float *__restrict__ loss_out)
{
	slab_sgd(slab, pair_losses, n_pairs, NPARAMS, params, moms, lr, mom, loss_out);
}

static int prepare_step_kernels()
{
	return prepare_kernels(Net::PREFIX, {(const void *)train_mb_step_kernel<true>, (const void *)train_mb_step_kernel<false>}, LDS_BYTES);
}

static int enqueue_step(const float *patches, const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz,
                        int64_t n_nnz, const int32_t *rows, const int32_t *src, const float *prm, int n_pairs, float *params, float *moms,
                        float lr, float mom, float margin, int pow, float *loss_out, void *ws, hipStream_t st)
{
	float *slab = (float *)ws;
	float *pair_losses = slab + (size_t)n_pairs * NPARAMS;
	if (patches)
		train_mb_step_kernel<false><<<n_pairs, NT, LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
		                                                                  margin, pow, 1.f / (float)n_pairs, slab, pair_losses);
	else
		train_mb_step_kernel<true><<<n_pairs, NT, LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
		                                                                 margin, pow, 1.f / (float)n_pairs, slab, pair_losses);
	if (int rc = check_launch("train_mb_step")) return rc;
	train_mb_sgd_kernel<<<cdiv(NPARAMS, 256), 256, 0, st>>>(slab, pair_losses, n_pairs, params, moms, lr, mom, loss_out);
	return check_launch("train_mb_sgd");
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
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 24), "train_mb_sample: n_pairs %d", n_pairs);
	MC_REQUIRE(rows && src && prm && out, "train_mb_sample: null pointer");
	train_mb_sample_kernel<<<n_pairs, 384, 0, as_stream(stream)>>>(planes, table, n_planes, nnz, n_nnz, rows, src, prm, out);
	return check_launch("train_mb_sample");
}

int mc_train_mb_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow,
                           float *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_step_args<Net>(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "train_mb_step_batch: null pointer");
	if (int rc = prepare_step_kernels()) return rc;
	return enqueue_step(patches, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, n_pairs, params, moms, lr, mom, margin, pow,
	                    loss_out, workspace, as_stream(stream));
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
		return enqueue_step(nullptr, planes, table, n_planes, nnz, n_nnz, perm + t0 + first, src + 2 * first, prm + first * NPRM, n_pairs, params,
		                    moms, lr, mom, margin, pow, losses + s, workspace, st);
	});
}

}  // extern "C"
