// Training of the fast architecture on Middlebury (main.lua:602-890, `mb fast`: -l1 5 -fm 64) on gfx950: libmctrainmb.so.
//
// The step is train.hip's, restated for five valid 3x3 convolutions on 11 x 11 patches (11 -> 9 -> 7 -> 5 -> 3 -> 1) and a
// ragged image store (include/mc_train_mb.h).  TWO kernels:
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
#include "train_conv.h"
#include "train_range.h"

namespace mc {

static_assert(FM == MC_TRAIN_MB_FM && MC_TRAIN_MB_NPRM == MC_TRAIN_NPRM, "train_conv.h's feature maps, the sampler's parameter layout");
constexpr int PS = MC_TRAIN_MB_WS;
constexpr int NPIX = 3 * PS * PS;        // floats of a pair's patches
constexpr int NPRM = MC_TRAIN_MB_NPRM;
constexpr int NPARAMS = MC_TRAIN_MB_NPARAMS;
constexpr int NL = MC_TRAIN_MB_L1;

// offsets of the flat parameter buffer: w1 b1 w2 b2 ... w5 b5
constexpr int LAYER_STRIDE = FM * FM * 9 + FM;
__host__ __device__ constexpr int off_w(int l) { return l == 1 ? 0 : FM * 9 + FM + (l - 2) * LAYER_STRIDE; }
__host__ __device__ constexpr int off_b(int l) { return l == 1 ? FM * 9 : off_w(l) + FM * FM * 9; }
static_assert(off_b(NL) + FM == NPARAMS, "parameter layout");

// LDS layout (floats): three patches' activations of every layer, then split-K partial tiles
constexpr int S0 = 11, S1 = 9, S2 = 7, S3 = 5, S4 = 3;
constexpr int L_X = 0;                                  // [3][121]
constexpr int L_A1 = 384;                               // [3][64][81]
constexpr int L_A2 = L_A1 + 3 * FM * S1 * S1;           // [3][64][49]
constexpr int L_A3 = L_A2 + 3 * FM * S2 * S2;           // [3][64][25]
constexpr int L_A4 = L_A3 + 3 * FM * S3 * S3;           // [3][64][9]
constexpr int L_A5 = L_A4 + 3 * FM * S4 * S4;           // [3][64]
constexpr int L_SPLIT = L_A5 + 3 * FM;                  // [8][16][64] partial tiles
constexpr int L_TOTAL = L_SPLIT + SPLIT_FLOATS;
constexpr size_t STEP_LDS_BYTES = (size_t)L_TOTAL * sizeof(float);
static_assert(NPIX <= L_A1 && NPIX <= NT, "the patches' slot, one thread per patch pixel");
static_assert(STEP_LDS_BYTES == 161024 && STEP_LDS_BYTES <= 160 * 1024, "a CU has 160 KiB of LDS");

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
	float *X = lds + L_X, *A1 = lds + L_A1, *A2 = lds + L_A2, *A3 = lds + L_A3, *A4 = lds + L_A4, *A5 = lds + L_A5, *split = lds + L_SPLIT;
	if (t < NPIX) {
		if (SAMPLE)
			X[t] = sample_mb_pixel<PS>(planes, table, n_planes, nnz, n_nnz, rows[pair], src + 2 * (int64_t)pair, prm + (int64_t)pair * NPRM, t);
		else
			X[t] = patches[(int64_t)pair * NPIX + t];
	}
	__syncthreads();
	conv_forward<1, S0, 1>(params + off_w(1), params + off_b(1), X, A1, true, split);
	__syncthreads();
	conv_forward<FM, S1, 1>(params + off_w(2), params + off_b(2), A1, A2, true, split);
	__syncthreads();
	conv_forward<FM, S2, 1>(params + off_w(3), params + off_b(3), A2, A3, true, split);
	__syncthreads();
	conv_forward<FM, S3, 4>(params + off_w(4), params + off_b(4), A3, A4, true, split);
	__syncthreads();
	conv_forward<FM, S4, 4>(params + off_w(5), params + off_b(5), A4, A5, false, split);
	__syncthreads();
	// Normalize2, StereoJoin1, Margin2 and their backward passes (train_conv.h): exactly those of train_step_kernel
	if (t < 64) {
		const float loss = hinge_tail(A5, t, margin, pow, inv_pairs);
		if (t == 0) losses[pair] = loss;
	}
	__syncthreads();
	float *g = slab + (int64_t)pair * NPARAMS;
	conv_weight_grad<FM, S4>(A5, A4, g + off_w(5), g + off_b(5), split);
	__syncthreads();
	conv_data_grad<S4, 4>(params + off_w(5), A5, A4, split);
	__syncthreads();
	conv_weight_grad<FM, S3>(A4, A3, g + off_w(4), g + off_b(4), split);
	__syncthreads();
	conv_data_grad<S3, 1>(params + off_w(4), A4, A3, split);
	__syncthreads();
	conv_weight_grad<FM, S2>(A3, A2, g + off_w(3), g + off_b(3), split);
	__syncthreads();
	conv_data_grad<S2, 1>(params + off_w(3), A3, A2, split);
	__syncthreads();
	conv_weight_grad<FM, S1>(A2, A1, g + off_w(2), g + off_b(2), split);
	__syncthreads();
	conv_data_grad<S1, 1>(params + off_w(2), A2, A1, split);
	__syncthreads();
	conv_weight_grad<1, S0>(A1, X, g + off_w(1), g + off_b(1), split);
}

// Kernel (b): g = sum over pairs in order; v = mom * v - lr * g; w += v.  Block 0 also writes the mean loss.
__global__ void __launch_bounds__(256) train_mb_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ pair_losses, int n_pairs,
                                                           float *__restrict__ params, float *__restrict__ moms, float lr, float mom,
                                                           float *__restrict__ loss_out)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j < NPARAMS) {
		float g = 0.f;
		for (int p = 0; p < n_pairs; ++p) g += slab[(int64_t)p * NPARAMS + j];
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

static size_t slab_bytes(int n_pairs) { return (size_t)n_pairs * NPARAMS * sizeof(float); }

static int prepare_step_kernels()
{
	static int rc = -1;
	if (rc >= 0) return rc;
	hipError_t e = hipFuncSetAttribute((const void *)train_mb_step_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STEP_LDS_BYTES);
	if (e == hipSuccess)
		e = hipFuncSetAttribute((const void *)train_mb_step_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STEP_LDS_BYTES);
	if (e != hipSuccess) {
		set_error("train_mb: hipFuncSetAttribute(%zu bytes of LDS): %s", STEP_LDS_BYTES, hipGetErrorString(e));
		return (int)e;
	}
	rc = 0;
	return rc;
}

static int check_step_args(int n_pairs, const float *params, const float *moms, float margin, int pow, void *ws, size_t ws_bytes)
{
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= MC_TRAIN_MB_MAX_PAIRS, "train_mb: n_pairs %d outside [1, %d]", n_pairs, MC_TRAIN_MB_MAX_PAIRS);
	MC_REQUIRE(params && moms, "train_mb: null params / momenta");
	MC_REQUIRE(pow == 1 || pow == 2, "train_mb: pow %d (Margin2 has pow 1 and 2, adcensus.cu:1427-1447)", pow);
	MC_REQUIRE(isfinite(margin), "train_mb: margin not finite");
	MC_REQUIRE(ws && ws_bytes >= mc_train_mb_workspace_bytes(n_pairs), "train_mb: workspace of %zu bytes, %zu needed", ws_bytes,
	           mc_train_mb_workspace_bytes(n_pairs));
	return 0;
}

static int check_store_args(const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz)
{
	MC_REQUIRE(planes && table && nnz, "train_mb: null planes / table / nnz pointer");
	MC_REQUIRE(n_planes >= 1, "train_mb: n_planes %d", n_planes);
	MC_REQUIRE(n_nnz >= 1, "train_mb: empty nnz");
	return 0;
}

static int enqueue_step(const float *patches, const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz,
                        int64_t n_nnz, const int32_t *rows, const int32_t *src, const float *prm, int n_pairs, float *params, float *moms,
                        float lr, float mom, float margin, int pow, float *loss_out, void *ws, hipStream_t st)
{
	float *slab = (float *)ws;
	float *pair_losses = slab + (size_t)n_pairs * NPARAMS;
	if (patches)
		train_mb_step_kernel<false><<<n_pairs, NT, STEP_LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
		                                                                  margin, pow, 1.f / (float)n_pairs, slab, pair_losses);
	else
		train_mb_step_kernel<true><<<n_pairs, NT, STEP_LDS_BYTES, st>>>(patches, planes, table, n_planes, nnz, n_nnz, rows, src, prm, params,
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
	if (n_pairs < 1 || n_pairs > MC_TRAIN_MB_MAX_PAIRS) return 0;
	return slab_bytes(n_pairs) + (size_t)n_pairs * sizeof(float);
}

int mc_train_mb_sample(const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                       const int32_t *rows, const int32_t *src, const float *prm, int n_pairs, float *out, void *stream)
{
	if (int rc = check_store_args(planes, table, n_planes, nnz, n_nnz)) return rc;
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 24), "train_mb_sample: n_pairs %d", n_pairs);
	MC_REQUIRE(rows && src && prm && out, "train_mb_sample: null pointer");
	train_mb_sample_kernel<<<n_pairs, 384, 0, as_stream(stream)>>>(planes, table, n_planes, nnz, n_nnz, rows, src, prm, out);
	return check_launch("train_mb_sample");
}

int mc_train_mb_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow,
                           float *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_step_args(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
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
	if (int rc = check_store_args(planes, table, n_planes, nnz, n_nnz)) return rc;
	if (int rc = check_step_args(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(perm && src && prm && losses, "train_mb_run: null pointer");
	MC_REQUIRE(n_steps >= 0, "train_mb_run: n_steps %d", n_steps);
	int64_t end;   // t0 + n_steps * n_pairs, saturated: train_range.h
	MC_REQUIRE(train_steps_fit(t0, n_steps, n_pairs, n_perm, &end), "train_mb_run: steps [%lld, %lld) of the permutation exceed its %lld rows",
	           (long long)t0, (long long)end, (long long)n_perm);
	if (int rc = prepare_step_kernels()) return rc;
	const hipStream_t st = as_stream(stream);
	for (int s = 0; s < n_steps; ++s) {
		const int64_t first = (int64_t)s * n_pairs;
		if (int rc = enqueue_step(nullptr, planes, table, n_planes, nnz, n_nnz, perm + t0 + first, src + 2 * first, prm + first * NPRM, n_pairs,
		                          params, moms, lr, mom, margin, pow, losses + s, workspace, st))
			return rc;
	}
	return 0;
}

}  // extern "C"
