// The fast architecture's trainer, stated once for its three libraries: train.hip (libmctrain.so, l1 4, KITTI's image store),
// train_mb.hip (libmctrainmb.so, l1 5, Middlebury's ragged store) and train_depth.hip (libmctraindepth.so, l1 1..5, both).
//   the net      FastNet<L, Lib>: train_net.h's description of l1 = L valid 3x3 convolutions of 64 maps on patches of side 2 L + 1,
//                with what a library's kernels and entry points need of it; Lib is the library's tag (PREFIX, MAX_PAIRS).
//   the device   where a pair's patches come from (ImageStore, RaggedStore), the sampler kernels' body (write_patches) and
//                the step kernels' (step_of_pair: patches into LDS, a barrier, train_conv.h's pair_step).
//   the host     raise_lds_limit, enqueue_step (step kernel, update kernel and their checks), step_batch and sample_patches with
//                their argument checks.  A library hands its own kernels in as template arguments and keeps its __global__
//                entries, its entry points and the offsets of a run (rows, src and prm arrive here already offset).
#pragma once
#include "mc_common.h"
#include "train_mb_sampler.h"   // sample_mb_pixel, and train_sampler.h's sample_pair_pixel
#include "train_conv.h"         // the GEMMs, the step of a net, the update

#include <initializer_list>
#include <type_traits>

namespace mc {

template <int L_, class Lib>
struct FastNet {
	static constexpr int L = L_;
	static constexpr int FM = mc::FM, PS = 2 * L + 1, NL = L, NP = 3, L2 = 0, MAX_PAIRS = Lib::MAX_PAIRS;
	static constexpr const char *PREFIX = Lib::PREFIX;
	static constexpr int NPIX = 3 * PS * PS;                  // floats of a pair's patches
	static constexpr int SAMPLE_NT = (NPIX + 63) / 64 * 64;   // the sample kernel's block: a thread per patch pixel, whole waves
	static constexpr int NPARAMS = n_conv<FastNet>();
	static constexpr size_t LDS_BYTES = STEP_LDS_BYTES<FastNet>;
};
constexpr int NPRM = MC_TRAIN_NPRM;
static_assert(NPRM == MC_TRAIN_MB_NPRM, "the sampler's parameter layout");

// ---- device ------------------------------------------------------------------------------------------------------------------
// F(a...) as a function of its own.  The sampler's warp is a few thousand instructions of double arithmetic.  While every sample
// and step kernel wrote its own call of it, the compiler's cost model left it a function that a library's kernels share; called
// from the one place below it would be inlined into each of them.  This states what the cost model chose: the kernels' code
// stays instruction for instruction what it was.
template <auto F, class... A> __device__ __noinline__ float out_of_line(A... a) { return F(a...); }

// Where a pair's patches come from: pixel<N>(pair, t, the store's kernel arguments) is float t of the pair's three patches.
struct ImageStore {    // x0, x1 (n_img, H, W), sampled by rows[pair] of nnz and the pair's prm
	template <class N>
	static __device__ __forceinline__ float pixel(int pair, int t, const float *__restrict__ x0, const float *__restrict__ x1, int n_img, int H, int W,
	                                              const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
	                                              const float *__restrict__ prm)
	{
		return out_of_line<sample_pair_pixel<N::PS>>(x0, x1, n_img, H, W, nnz, n_nnz, rows[pair], prm + (int64_t)pair * NPRM, t);
	}
};
struct RaggedStore {   // planes, table (n_planes), sampled by the pair's src as well
	template <class N>
	static __device__ __forceinline__ float pixel(int pair, int t, const float *__restrict__ planes, const mc_train_mb_plane *__restrict__ table,
	                                              int n_planes, const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
	                                              const int32_t *__restrict__ src, const float *__restrict__ prm)
	{
		return out_of_line<sample_mb_pixel<N::PS>>(planes, table, n_planes, nnz, n_nnz, rows[pair], src + 2 * (int64_t)pair, prm + (int64_t)pair * NPRM, t);
	}
};

// A sample kernel: one workgroup per pair writes its patches to out (n_pairs, 3, PS, PS).
template <class N, class Store, class... A>
__device__ __forceinline__ void write_patches(float *__restrict__ out, A... store)
{
	const int pair = blockIdx.x, t = threadIdx.x;
	if (t < N::NPIX) out[(int64_t)pair * N::NPIX + t] = Store::template pixel<N>(pair, t, store...);
}

// A step kernel: one workgroup per pair.  SAMPLE: the patches are sampled from the store; otherwise they are patches
// (n_pairs, 3, PS, PS).  Writes the pair's gradients to slab[pair] and its loss to losses[pair].
template <class N, bool SAMPLE, class Store, class... A>
__device__ __forceinline__ void step_of_pair(const float *__restrict__ patches, const float *__restrict__ params, float margin, int pow,
                                             float inv_pairs, float *__restrict__ slab, float *__restrict__ losses, A... store)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	const int pair = blockIdx.x, t = threadIdx.x;
	if (t < N::NPIX) {
		if (SAMPLE)
			lds[t] = Store::template pixel<N>(pair, t, store...);
		else
			lds[t] = patches[(int64_t)pair * N::NPIX + t];
	}
	__syncthreads();
	pair_step<N>(params, margin, pow, inv_pairs, lds, slab + (int64_t)pair * N::NPARAMS, losses + pair);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// check_launch("<prefix>_<what>")
static int check_launch_of(const char *prefix, const char *what)
{
	char name[64];
	snprintf(name, sizeof(name), "%s_%s", prefix, what);
	return check_launch(name);
}

// Lets net N's step kernels ks take its LDS; once per net, so that every depth of libmctraindepth.so keeps its own limit.
template <class N> static int raise_lds_limit(std::initializer_list<const void *> ks)
{
	static int rc = -1;
	if (rc >= 0) return rc;
	for (const void *k : ks) {
		const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)N::LDS_BYTES);
		if (e != hipSuccess) {
			set_error("%s: hipFuncSetAttribute(l1 %d, %zu bytes of LDS): %s", N::PREFIX, N::L, N::LDS_BYTES, hipGetErrorString(e));
			return (int)e;
		}
	}
	rc = 0;
	return rc;
}

// One step of net N: the step kernel Step on what it takes before `params` (given patches and / or a store with rows, src and prm
// of this step), then the update kernel Sgd, which sums the slab in pair order.  libmctraindepth.so's one update kernel for
// every depth takes the number of parameters as well.
template <class N, auto Step, auto Sgd, class... Store>
static int enqueue_step(int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow, float *loss_out, void *ws,
                        hipStream_t st, Store... store)
{
	float *slab = (float *)ws;
	float *pair_losses = slab + (size_t)n_pairs * N::NPARAMS;
	Step<<<n_pairs, NT, N::LDS_BYTES, st>>>(store..., params, margin, pow, 1.f / (float)n_pairs, slab, pair_losses);
	if (int rc = check_launch_of(N::PREFIX, "step")) return rc;
	if constexpr (std::is_invocable_v<decltype(Sgd), const float *, const float *, int, int, float *, float *, float, float, float *>)
		Sgd<<<cdiv(N::NPARAMS, 256), 256, 0, st>>>(slab, pair_losses, n_pairs, N::NPARAMS, params, moms, lr, mom, loss_out);
	else
		Sgd<<<cdiv(N::NPARAMS, 256), 256, 0, st>>>(slab, pair_losses, n_pairs, params, moms, lr, mom, loss_out);
	return check_launch_of(N::PREFIX, "sgd");
}

// mc_train*_step_batch: Step is the library's step kernel for given patches, no_store what it takes between them and `params`
// (a store that is not read: null pointers and zeros); prepare() raises the net's LDS limit.
template <class N, auto Step, auto Sgd, class Prepare, class... Store>
static int step_batch(Prepare prepare, const float *patches, int n_pairs, float *params, float *moms, float lr, float mom, float margin, int pow,
                      float *loss_out, void *workspace, size_t workspace_bytes, void *stream, Store... no_store)
{
	if (int rc = check_step_args<N>(n_pairs, params, moms, margin, pow, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "%s_step_batch: null pointer", N::PREFIX);
	if (int rc = prepare()) return rc;
	return enqueue_step<N, Step, Sgd>(n_pairs, params, moms, lr, mom, margin, pow, loss_out, workspace, as_stream(stream), patches, no_store...);
}

// mc_train*_sample after the check of its store: `who` names the entry point, args are the sample kernel Sample's
template <class N, auto Sample, class... Args>
static int sample_patches(const char *who, int n_pairs, bool pointers_given, void *stream, Args... args)
{
	MC_REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 24), "%s: n_pairs %d", who, n_pairs);
	MC_REQUIRE(pointers_given, "%s: null pointer", who);
	Sample<<<n_pairs, N::SAMPLE_NT, 0, as_stream(stream)>>>(args...);
	return check_launch(who);
}

}  // namespace mc
