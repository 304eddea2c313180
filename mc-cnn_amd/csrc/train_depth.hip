// Training of the fast architecture at -l1 1..5 (main.lua:212-214, 240-242, 271-273, 726-746) on gfx950: libmctraindepth.so.
//
// The step is the fast net's of train_fast.h, which states the net, the kernels' bodies and the host side of a step once for
// libmctrain.so, libmctrainmb.so and this library: l1 valid 3x3 convolutions of 64 maps on patches of side 2 l1 + 1, one
// workgroup of eight waves per pair with every activation in LDS, the pair's gradients into its own slab row, then the update
// that sums the slab in pair order.  A depth is an instantiation: the kernels below are templates of L and each entry point
// switches on l1 (with_depth); at l1 4 and 5 they instantiate what libmctrain.so and libmctrainmb.so instantiate, so the three
// libraries compute the same bits where they overlap.  Both image stores are served: x0 / x1 of a KITTI set (train_sampler.h)
// and Middlebury's ragged planes (train_mb_sampler.h).
//
// What a depth changes in the GEMMs (N columns, padded to 32; split_k(N) slices K over four waves where N <= 32):
//   l1 = 1: one forward GEMM of N = 3 (K = 9 taps in 5 steps, split 1 1 1 2), one weight gradient of K = 3, no data gradient;
//   l1 = 2: forward N = 27 (the first layer split for once: 5 steps again), 3; data gradient N = 27;
//   l1 = 3: forward N = 75, 27, 3; data gradient N = 27, 75.
// Every kernel's dynamic-LDS limit is raised to its own depth's size (train_fast.h's raise_lds_limit), once per depth.
#include "mc_common.h"
#include "../../include/mc_train_depth.h"
#include "train_fast.h"   // the fast net, its kernels' bodies over either store, the host side of a step

namespace mc {

struct Lib {
	static constexpr const char *PREFIX = "train_depth";
	static constexpr int MAX_PAIRS = MC_TRAIN_DEPTH_MAX_PAIRS;
};
template <int L> using Net = FastNet<L, Lib>;
constexpr int MIN_L1 = MC_TRAIN_DEPTH_MIN_L1, MAX_L1 = MC_TRAIN_DEPTH_MAX_L1;
static_assert(Net<1>::FM == MC_TRAIN_DEPTH_FM && NPRM == MC_TRAIN_DEPTH_NPRM, "the net of mc_train_depth.h");
static_assert(Net<1>::NPARAMS == 640 && Net<2>::NPARAMS == 37568 && Net<3>::NPARAMS == 74496, "640 + (l1 - 1) * 36 928");
static_assert(Net<4>::NPARAMS == MC_TRAIN_NPARAMS && Net<5>::NPARAMS == MC_TRAIN_MB_NPARAMS, "the layouts of mc_train.h and mc_train_mb.h");
static_assert(Net<1>::LDS_BYTES == 34048 && Net<2>::LDS_BYTES == 40960 && Net<3>::LDS_BYTES == 60672, "the LDS layout");
static_assert(Net<4>::LDS_BYTES == 98304 && Net<5>::LDS_BYTES == 161024, "train.hip's and train_mb.hip's");
static_assert(Net<MAX_L1>::LDS_BYTES <= 160 * 1024 && Net<MAX_L1>::NPIX <= NT, "a CU has 160 KiB of LDS; one thread per patch pixel");
// what refuses l1 = 6: its step's LDS, of which the activations alone are 221 696 bytes
constexpr long DEEPER_LDS_BYTES = (long)Net<MAX_L1 + 1>::LDS_BYTES;
static_assert(DEEPER_LDS_BYTES == 254464 && DEEPER_LDS_BYTES - SPLIT_FLOATS * (long)sizeof(float) > 160 * 1024, "l1 = 6 does not fit");

// ---- the KITTI store: x0, x1 (n_img, H, W) -----------------------------------------------------------------------------------
template <int L>
__global__ void __launch_bounds__(Net<L>::SAMPLE_NT) train_depth_sample_kernel(const float *__restrict__ x0, const float *__restrict__ x1, int n_img,
                                                                              int H, int W, const float *__restrict__ nnz, int64_t n_nnz,
                                                                              const int32_t *__restrict__ rows, const float *__restrict__ prm,
                                                                              float *__restrict__ out)
{
	write_patches<Net<L>, ImageStore>(out, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm);
}

// One workgroup per pair.  SAMPLE: the patches come from the images (rows[pair] of nnz, prm of the pair); otherwise from patches
// (n_pairs, 3, PS, PS).  Writes the pair's gradients to slab[pair] and its loss to losses[pair].
template <int L, bool SAMPLE>
__global__ void __launch_bounds__(NT) train_depth_step_kernel(const float *__restrict__ patches, const float *__restrict__ x0,
                                                              const float *__restrict__ x1, int n_img, int H, int W,
                                                              const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                              const float *__restrict__ prm, const float *__restrict__ params, float margin,
                                                              int pow, float inv_pairs, float *__restrict__ slab, float *__restrict__ losses)
{
	step_of_pair<Net<L>, SAMPLE, ImageStore>(patches, params, margin, pow, inv_pairs, slab, losses, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm);
}

// ---- the ragged store: planes, table, src ------------------------------------------------------------------------------------
template <int L>
__global__ void __launch_bounds__(Net<L>::SAMPLE_NT) train_depth_mb_sample_kernel(const float *__restrict__ planes,
                                                                                 const mc_train_mb_plane *__restrict__ table, int n_planes,
                                                                                 const float *__restrict__ nnz, int64_t n_nnz,
                                                                                 const int32_t *__restrict__ rows, const int32_t *__restrict__ src,
                                                                                 const float *__restrict__ prm, float *__restrict__ out)
{
	write_patches<Net<L>, RaggedStore>(out, planes, table, n_planes, nnz, n_nnz, rows, src, prm);
}

// The step on the ragged store; it takes given patches only through train_depth_step_kernel<L, false>.
template <int L>
__global__ void __launch_bounds__(NT) train_depth_mb_step_kernel(const float *__restrict__ planes, const mc_train_mb_plane *__restrict__ table,
                                                                 int n_planes, const float *__restrict__ nnz, int64_t n_nnz,
                                                                 const int32_t *__restrict__ rows, const int32_t *__restrict__ src,
                                                                 const float *__restrict__ prm, const float *__restrict__ params, float margin,
                                                                 int pow, float inv_pairs, float *__restrict__ slab, float *__restrict__ losses)
{
	step_of_pair<Net<L>, true, RaggedStore>(nullptr, params, margin, pow, inv_pairs, slab, losses, planes, table, n_planes, nnz, n_nnz, rows, src, prm);
}

// g = sum over pairs in order; v = mom * v - lr * g; w += v.  Block 0 also writes the mean loss.  One kernel for every depth.
__global__ void __launch_bounds__(256) train_depth_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ pair_losses, int n_pairs,
                                                              int n_params, float *__restrict__ params, float *__restrict__ moms, float lr, float mom,
                                                              float *__restrict__ loss_out)
{
	slab_sgd(slab, pair_losses, n_pairs, n_params, params, moms, lr, mom, loss_out);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <class N> static int prepare()
{
	return raise_lds_limit<N>({(const void *)train_depth_step_kernel<N::L, true>, (const void *)train_depth_step_kernel<N::L, false>,
	                           (const void *)train_depth_mb_step_kernel<N::L>});
}

// f(Net<l1>{}) for l1 in [1, 5]; refuses every other depth
template <class F> static int with_depth(int l1, F f)
{
	switch (l1) {
	case 1: return f(Net<1>{});
	case 2: return f(Net<2>{});
	case 3: return f(Net<3>{});
	case 4: return f(Net<4>{});
	case 5: return f(Net<5>{});
	}
	if (l1 > MAX_L1)
		set_error("train_depth: l1 %d outside [%d, %d]: the step of six layers keeps %ld bytes in LDS, a CU has %d", l1, MIN_L1, MAX_L1,
		          DEEPER_LDS_BYTES, 160 * 1024);
	else
		set_error("train_depth: l1 %d outside [%d, %d]", l1, MIN_L1, MAX_L1);
	return MC_EINVAL;
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_depth_version(void) { return MC_TRAIN_DEPTH_ABI_VERSION; }

const char *mc_train_depth_last_error(void) { return last_error(); }

int mc_train_depth_ws(int l1) { return l1 >= MIN_L1 && l1 <= MAX_L1 ? 2 * l1 + 1 : 0; }

int mc_train_depth_nparams(int l1)
{
	return l1 >= MIN_L1 && l1 <= MAX_L1 ? with_depth(l1, [](auto n) { return decltype(n)::NPARAMS; }) : 0;
}

size_t mc_train_depth_workspace_bytes(int l1, int n_pairs)
{
	const int n_params = mc_train_depth_nparams(l1);
	if (n_params == 0 || n_pairs < 1 || n_pairs > MC_TRAIN_DEPTH_MAX_PAIRS) return 0;
	return (size_t)n_pairs * ((size_t)n_params + 1) * sizeof(float);   // step_workspace_bytes<Net<l1>>(n_pairs)
}

int mc_train_depth_step_batch(int l1, const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow,
                              float *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
	return with_depth(l1, [&](auto n) {
		using N = decltype(n);
		return step_batch<N, train_depth_step_kernel<N::L, false>, train_depth_sgd_kernel>(prepare<N>, patches, n_pairs, params, moms, lr, mom, margin,
		                                                                                    pow, loss_out, workspace, workspace_bytes, stream, nullptr,
		                                                                                    nullptr, 0, 0, 0, nullptr, 0, nullptr, nullptr);
	});
}

int mc_train_depth_sample(int l1, const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *rows,
                          const float *prm, int n_pairs, float *out, void *stream)
{
	return with_depth(l1, [&](auto n) {
		using N = decltype(n);
		if (int rc = check_image_args(N::PREFIX, x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
		return sample_patches<N, train_depth_sample_kernel<N::L>>("train_depth_sample", n_pairs, rows && prm && out, stream, x0, x1, n_img, H, W, nnz,
		                                                          n_nnz, rows, prm, out);
	});
}

int mc_train_depth_run(int l1, const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz, const int32_t *perm,
                       int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const float *prm, float *params, float *moms, float lr, float mom,
                       float margin, int pow, float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	return with_depth(l1, [&](auto n) {
		using N = decltype(n);
		if (int rc = check_image_args(N::PREFIX, x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
		if (int rc = check_step_args<N>(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
		const hipStream_t st = as_stream(stream);
		return run_steps(N::PREFIX, perm && prm && losses, t0, n_steps, n_pairs, n_perm, prepare<N>, [&](int s, int64_t first) {
			return enqueue_step<N, train_depth_step_kernel<N::L, true>, train_depth_sgd_kernel>(n_pairs, params, moms, lr, mom, margin, pow, losses + s,
			                                                                                     workspace, st, nullptr, x0, x1, n_img, H, W, nnz, n_nnz,
			                                                                                     perm + t0 + first, prm + first * NPRM);
		});
	});
}

int mc_train_depth_mb_sample(int l1, const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                             const int32_t *rows, const int32_t *src, const float *prm, int n_pairs, float *out, void *stream)
{
	return with_depth(l1, [&](auto n) {
		using N = decltype(n);
		if (int rc = check_store_args(N::PREFIX, planes, table, n_planes, nnz, n_nnz)) return rc;
		return sample_patches<N, train_depth_mb_sample_kernel<N::L>>("train_depth_mb_sample", n_pairs, rows && src && prm && out, stream, planes, table,
		                                                             n_planes, nnz, n_nnz, rows, src, prm, out);
	});
}

int mc_train_depth_mb_run(int l1, const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                          const int32_t *perm, int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const int32_t *src, const float *prm,
                          float *params, float *moms, float lr, float mom, float margin, int pow, float *losses, void *workspace,
                          size_t workspace_bytes, void *stream)
{
	return with_depth(l1, [&](auto n) {
		using N = decltype(n);
		if (int rc = check_store_args(N::PREFIX, planes, table, n_planes, nnz, n_nnz)) return rc;
		if (int rc = check_step_args<N>(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
		const hipStream_t st = as_stream(stream);
		return run_steps(N::PREFIX, perm && src && prm && losses, t0, n_steps, n_pairs, n_perm, prepare<N>, [&](int s, int64_t first) {
			return enqueue_step<N, train_depth_mb_step_kernel<N::L>, train_depth_sgd_kernel>(n_pairs, params, moms, lr, mom, margin, pow, losses + s,
			                                                                                  workspace, st, planes, table, n_planes, nnz, n_nnz,
			                                                                                  perm + t0 + first, src + 2 * first, prm + first * NPRM);
		});
	});
}

}  // extern "C"
