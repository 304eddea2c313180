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
#include "mc_common.h"
#include "../../include/mc_train.h"
#include "train_sampler.h"
#include "train_conv.h"
#include "train_range.h"

namespace mc {

static_assert(FM == MC_TRAIN_FM, "train_conv.h's feature maps");
constexpr int NPRM = MC_TRAIN_NPRM;
constexpr int NPARAMS = MC_TRAIN_NPARAMS;

// offsets of the flat parameter buffer: w1 b1 w2 b2 w3 b3 w4 b4
constexpr int OFF_W1 = 0, OFF_B1 = FM * 9;
constexpr int OFF_W2 = OFF_B1 + FM;
constexpr int LAYER_STRIDE = FM * FM * 9 + FM;
__host__ __device__ constexpr int off_w(int l) { return l == 1 ? OFF_W1 : OFF_W2 + (l - 2) * LAYER_STRIDE; }
__host__ __device__ constexpr int off_b(int l) { return l == 1 ? OFF_B1 : off_w(l) + FM * FM * 9; }
static_assert(off_b(4) + FM == NPARAMS, "parameter layout");

// LDS layout (floats): three patches' activations of every layer, then split-K partial tiles
constexpr int S0 = 9, S1 = 7, S2 = 5, S3 = 3;
constexpr int L_X = 0;                                  // [3][81]
constexpr int L_A1 = 256;                               // [3][64][49]
constexpr int L_A2 = L_A1 + 3 * FM * S1 * S1;           // [3][64][25]
constexpr int L_A3 = L_A2 + 3 * FM * S2 * S2;           // [3][64][9]
constexpr int L_A4 = L_A3 + 3 * FM * S3 * S3;           // [3][64]
constexpr int L_SPLIT = L_A4 + 3 * FM;                  // [8][16][64] partial tiles
constexpr int L_TOTAL = L_SPLIT + SPLIT_FLOATS;
constexpr size_t STEP_LDS_BYTES = (size_t)L_TOTAL * sizeof(float);

__global__ void __launch_bounds__(256) train_sample_kernel(const float *__restrict__ x0, const float *__restrict__ x1, int n_img, int H, int W,
                                                           const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                           const float *__restrict__ prm, float *__restrict__ out)
{
	const int pair = blockIdx.x, t = threadIdx.x;
	if (t < 3 * WS * WS)
		out[(int64_t)pair * 3 * WS * WS + t] = sample_pair_pixel<WS>(x0, x1, n_img, H, W, nnz, n_nnz, rows[pair], prm + (int64_t)pair * NPRM, t);
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
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x, t = threadIdx.x;
	float *X = lds + L_X, *A1 = lds + L_A1, *A2 = lds + L_A2, *A3 = lds + L_A3, *A4 = lds + L_A4, *split = lds + L_SPLIT;
	if (t < 3 * WS * WS) {
		if (SAMPLE)
			X[t] = sample_pair_pixel<WS>(x0, x1, n_img, H, W, nnz, n_nnz, rows[pair], prm + (int64_t)pair * NPRM, t);
		else
			X[t] = patches[(int64_t)pair * 3 * WS * WS + t];
	}
	__syncthreads();
	conv_forward<1, S0, 1>(params + off_w(1), params + off_b(1), X, A1, true, split);
	__syncthreads();
	conv_forward<FM, S1, 1>(params + off_w(2), params + off_b(2), A1, A2, true, split);
	__syncthreads();
	conv_forward<FM, S2, 4>(params + off_w(3), params + off_b(3), A2, A3, true, split);
	__syncthreads();
	conv_forward<FM, S3, 4>(params + off_w(4), params + off_b(4), A3, A4, false, split);
	__syncthreads();
	// Normalize2, StereoJoin1, Margin2 and their backward passes (train_conv.h)
	if (t < 64) {
		const float loss = hinge_tail(A4, t, margin, pow, inv_pairs);
		if (t == 0) losses[pair] = loss;
	}
	__syncthreads();
	float *g = slab + (int64_t)pair * NPARAMS;
	conv_weight_grad<FM, S3>(A4, A3, g + off_w(4), g + off_b(4), split);
	__syncthreads();
	conv_data_grad<S3, 4>(params + off_w(4), A4, A3, split);
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
__global__ void __launch_bounds__(256) train_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ pair_losses, int n_pairs,
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
	hipError_t e = hipFuncSetAttribute((const void *)train_step_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STEP_LDS_BYTES);
	if (e == hipSuccess)
		e = hipFuncSetAttribute((const void *)train_step_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)STEP_LDS_BYTES);
	if (e != hipSuccess) {
		set_error("train: hipFuncSetAttribute(%zu bytes of LDS): %s", STEP_LDS_BYTES, hipGetErrorString(e));
		return (int)e;
	}
	rc = 0;
	return rc;
}

static int check_step_args(int n_pairs, const float *params, const float *moms, float margin, int pow, void *ws, size_t ws_bytes)
{
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= MC_TRAIN_MAX_PAIRS, "train: n_pairs %d outside [1, %d]", n_pairs, MC_TRAIN_MAX_PAIRS);
	MC_REQUIRE(params && moms, "train: null params / momenta");
	MC_REQUIRE(pow == 1 || pow == 2, "train: pow %d (Margin2 has pow 1 and 2, adcensus.cu:1427-1447)", pow);
	MC_REQUIRE(isfinite(margin), "train: margin not finite");
	MC_REQUIRE(ws && ws_bytes >= mc_train_workspace_bytes(n_pairs), "train: workspace of %zu bytes, %zu needed", ws_bytes,
	           mc_train_workspace_bytes(n_pairs));
	return 0;
}

static int check_image_args(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz)
{
	MC_REQUIRE(x0 && x1 && nnz, "train: null image / nnz pointer");
	MC_REQUIRE(n_img >= 1 && H >= 4 && W >= 4 && (int64_t)n_img * H * W < ((int64_t)1 << 40), "train: bad image dims %d x %d x %d", n_img, H, W);
	MC_REQUIRE(H < 32768 && W < 32768, "train: images of %d x %d exceed the warp's 16-bit coordinates", H, W);
	MC_REQUIRE(n_nnz >= 1, "train: empty nnz");
	return 0;
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_version(void) { return MC_TRAIN_ABI_VERSION; }

const char *mc_train_last_error(void) { return last_error(); }

size_t mc_train_workspace_bytes(int n_pairs)
{
	if (n_pairs < 1 || n_pairs > MC_TRAIN_MAX_PAIRS) return 0;
	return slab_bytes(n_pairs) + (size_t)n_pairs * sizeof(float);
}

int mc_train_sample(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *rows,
                    const float *prm, int n_pairs, float *out, void *stream)
{
	if (int rc = check_image_args(x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 24), "train_sample: n_pairs %d", n_pairs);
	MC_REQUIRE(rows && prm && out, "train_sample: null pointer");
	train_sample_kernel<<<n_pairs, 256, 0, as_stream(stream)>>>(x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, out);
	return check_launch("train_sample");
}

static int enqueue_step(const float *patches, const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz,
                        const int32_t *rows, const float *prm, int n_pairs, float *params, float *moms, float lr, float mom, float margin,
                        int pow, float *loss_out, void *ws, hipStream_t st)
{
	float *slab = (float *)ws;
	float *pair_losses = slab + (size_t)n_pairs * NPARAMS;
	if (patches)
		train_step_kernel<false><<<n_pairs, NT, STEP_LDS_BYTES, st>>>(patches, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, params, margin,
		                                                               pow, 1.f / (float)n_pairs, slab, pair_losses);
	else
		train_step_kernel<true><<<n_pairs, NT, STEP_LDS_BYTES, st>>>(patches, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, params, margin,
		                                                              pow, 1.f / (float)n_pairs, slab, pair_losses);
	if (int rc = check_launch("train_step")) return rc;
	train_sgd_kernel<<<cdiv(NPARAMS, 256), 256, 0, st>>>(slab, pair_losses, n_pairs, params, moms, lr, mom, loss_out);
	return check_launch("train_sgd");
}

int mc_train_step_batch(const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow,
                        float *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_step_args(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "train_step_batch: null pointer");
	if (int rc = prepare_step_kernels()) return rc;
	return enqueue_step(patches, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr, n_pairs, params, moms, lr, mom, margin, pow,
	                    loss_out, workspace, as_stream(stream));
}

int mc_train_run(const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *perm,
                 int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const float *prm, float *params, float *moms, float lr, float mom,
                 float margin, int pow, float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_image_args(x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
	if (int rc = check_step_args(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(perm && prm && losses, "train_run: null pointer");
	MC_REQUIRE(n_steps >= 0, "train_run: n_steps %d", n_steps);
	int64_t end;   // t0 + n_steps * n_pairs, saturated: train_range.h
	MC_REQUIRE(train_steps_fit(t0, n_steps, n_pairs, n_perm, &end), "train_run: steps [%lld, %lld) of the permutation exceed its %lld rows",
	           (long long)t0, (long long)end, (long long)n_perm);
	if (int rc = prepare_step_kernels()) return rc;
	const hipStream_t st = as_stream(stream);
	for (int s = 0; s < n_steps; ++s) {
		const int64_t first = t0 + (int64_t)s * n_pairs;
		if (int rc = enqueue_step(nullptr, x0, x1, n_img, H, W, nnz, n_nnz, perm + first, prm + (int64_t)s * n_pairs * NPRM, n_pairs, params,
		                          moms, lr, mom, margin, pow, losses + s, workspace, st))
			return rc;
	}
	return 0;
}

}  // extern "C"
