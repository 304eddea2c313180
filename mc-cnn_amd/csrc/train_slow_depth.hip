// Training of the accurate architecture at -l2 1..7 (main.lua:73-78, 120-124, 663-695) on gfx950: libmctrainslowdepth.so
// (include/mc_train_slow_depth.h).
//
// The step is the one of train_slow.hip (KITTI's store, four convolutions on 9 x 9 patches, a PAIR per tower workgroup, l2 4) and
// train_mb_slow.hip (the ragged store, five convolutions on 11 x 11 patches, a PATCH per tower workgroup, l2 3) with the number of
// hidden Linears given at run time.  What a depth changes is on the host alone: train_slow_fc.h's kernels take their layer by
// pointer, and its offsets, workspace and FC launches are stated over a StepShape, which here carries the caller's l2.  So
//   * the tower kernels are instantiated once per TOWER (they read n_conv, the LDS layout, PS, NL, NP, never l2): two forward
//     kernels per store (patches sampled / given) and one backward kernel per tower, SIX in all;
//   * fc_forward_kernel, fc_head_kernel and fc_backward_kernel<true / false> are the parents' FOUR;
//   * ONE update kernel takes n_conv and n_params as arguments.
// ELEVEN kernels serve the fourteen nets.  A step is 2 l2 + 4 launches: tower forward, l2 fc_forward, the head, l2 fc_backward
// (the first Linear's unmasked: the tower applies its ReLU), tower backward, the update.  At (KITTI, 4) and (Middlebury, 3) every
// launch computes what the parent library's does, in the same order: the results are the parents' bit for bit.
//
// MC_FC_HEAD_MAX_ROWS is 2048 for both stores (one translation unit), where libmctrainmbslow.so has 512: it sizes the head kernel's
// static LDS, 8 bytes per row, so 16 KiB here.  The head is ONE workgroup of a launch of its own: no other workgroup shares its CU's
// LDS, its arithmetic does not read the size, and the ragged store's 512 rows are checked on the host against its own MAX_PAIRS.
#include "mc_common.h"
#include "../../include/mc_train_slow_depth.h"
#include "../../include/mc_train_slow.h"
#include "../../include/mc_train_mb_slow.h"
#include "train_mb_sampler.h"   // sample_mb_pixel, and train_sampler.h's sample_pair_pixel
#include "train_slow_conv.h"    // block_gemm, the convolution GEMMs, the towers' layer chain
#define MC_FC_HEAD_MAX_ROWS (2 * MC_TRAIN_SLOW_DEPTH_MAX_PAIRS)
#include "train_slow_fc.h"      // the FC kernels, sgd_update, StepShape and the host side over it

namespace mc {

constexpr const char *PREFIX = "train_slow_depth";
constexpr int MIN_L2 = MC_TRAIN_SLOW_DEPTH_MIN_L2, MAX_DEPTH = MC_TRAIN_SLOW_DEPTH_MAX_L2;
constexpr int NPRM = MC_TRAIN_SLOW_DEPTH_NPRM;

// The two towers, as train_net.h describes a net, without its L2: nothing the tower kernels instantiate reads one.
struct KittiTower {
	static constexpr int FM = MC_TRAIN_SLOW_FM, PS = MC_TRAIN_SLOW_WS, NL = MC_TRAIN_SLOW_L1, NP = 3, MAX_PAIRS = MC_TRAIN_SLOW_DEPTH_MAX_PAIRS;
	static constexpr int STORE = MC_TRAIN_SLOW_DEPTH_KITTI;
};
struct MbTower {
	static constexpr int FM = MC_TRAIN_MB_SLOW_FM, PS = MC_TRAIN_MB_SLOW_WS, NL = MC_TRAIN_MB_SLOW_L1, NP = 1, MAX_PAIRS = MC_TRAIN_SLOW_DEPTH_MB_MAX_PAIRS;
	static constexpr int STORE = MC_TRAIN_SLOW_DEPTH_MB;
};
template <class T> constexpr StepShape shape_at(int l2) { return {PREFIX, T::PS, T::NP, n_conv<T>(), l2, T::MAX_PAIRS}; }

static_assert(MAX_DEPTH == MAX_L2 && NH == MC_TRAIN_SLOW_DEPTH_NH2, "train_slow_fc.h's deepest stack and hidden units");
static_assert(NPRM == MC_TRAIN_NPRM && NPRM == MC_TRAIN_MB_NPRM && KittiTower::PS == WS, "the samplers' patch and parameter layout");
static_assert(KittiTower::MAX_PAIRS == MC_TRAIN_SLOW_MAX_PAIRS && MbTower::MAX_PAIRS == MC_TRAIN_MB_SLOW_MAX_PAIRS, "the parents' batches");
static_assert(2 * KittiTower::MAX_PAIRS <= MC_FC_HEAD_MAX_ROWS && 2 * MbTower::MAX_PAIRS <= MC_FC_HEAD_MAX_ROWS, "the head kernel's rows");
static_assert(MC_FC_HEAD_MAX_ROWS * 2 * sizeof(float) == 16384, "the head kernel's static LDS");
static_assert(n_conv<KittiTower>() == MC_TRAIN_SLOW_NCONV && n_conv<MbTower>() == MC_TRAIN_MB_SLOW_NCONV, "convolution parameter layout");
// the sizes of mc_train_slow_depth.h
static_assert(shape_at<KittiTower>(1).n_fc() == MC_TRAIN_SLOW_DEPTH_NFC1 && NH * NH + NH == MC_TRAIN_SLOW_DEPTH_NFC_STEP, "NFC(l2) = 86 785 + (l2 - 1) * 147 840");
static_assert(shape_at<MbTower>(7).n_fc() == 86785 + 6 * 147840 && shape_at<KittiTower>(7).n_fc() == 973825, "NFC(7)");
static_assert(shape_at<KittiTower>(1).n_params() == 426929 && shape_at<KittiTower>(7).n_params() == 1313969, "KITTI's nets");
static_assert(shape_at<MbTower>(1).n_params() == 539937 && shape_at<MbTower>(7).n_params() == 1426977, "Middlebury's nets");
static_assert(shape_at<KittiTower>(MC_TRAIN_SLOW_L2).n_params() == MC_TRAIN_SLOW_NPARAMS, "libmctrainslow.so's layout at l2 4");
static_assert(shape_at<MbTower>(MC_TRAIN_MB_SLOW_L2).n_params() == MC_TRAIN_MB_SLOW_NPARAMS, "libmctrainmbslow.so's layout at l2 3");
// fc_weights_aligned at every depth: l2 7's offsets are every shallower net's
static_assert(shape_at<KittiTower>(MAX_DEPTH).fc_weights_aligned() && shape_at<MbTower>(MAX_DEPTH).fc_weights_aligned(), "float4 loads of the FC weights");
static_assert(TOWER_LDS_BYTES<KittiTower> == 113920 && TOWER_LDS_BYTES<MbTower> == 74432, "train_slow.hip's and train_mb_slow.hip's LDS");

// Which of a pair's patches a tower workgroup holds: T::NP of them from patch `first` on.  KITTI: block = pair, patches 0..2;
// Middlebury: block = 3 * pair + patch.  A block's pixels are floats PIX * block .. of (n_pairs, 3, PS, PS).
template <class T> struct Block {
	static constexpr int PER_PAIR = 3 / T::NP, PIX = T::NP * T::PS * T::PS, NFEAT = T::NP * FM;
	static_assert(PIX <= NT && NFEAT <= NT, "one thread per pixel and per feature of the workgroup's patches");
	int pair, first;
	__device__ __forceinline__ Block() : pair(blockIdx.x / PER_PAIR), first((blockIdx.x - (blockIdx.x / PER_PAIR) * PER_PAIR) * T::NP) {}
};

// The body of a forward tower kernel.  SAMPLE: pixel(pair, i) is float i of the pair's (3, PS, PS) patches, drawn from the
// store and kept in xs for the backward kernel; otherwise the pixels are patches'.  Writes the patches' features into rows
// 2 * pair, 2 * pair + 1 of a0 (2n, 224).
template <class T, bool SAMPLE, class Pixel>
__device__ __forceinline__ void forward_block(const float *__restrict__ patches, const float *__restrict__ params, float *__restrict__ xs,
                                              float *__restrict__ a0, float *lds, Pixel pixel)
{
	using B = Block<T>;
	const B b;
	const int t = threadIdx.x;
	if (t < B::PIX) {
		const int64_t e = (int64_t)blockIdx.x * B::PIX + t;
		if constexpr (SAMPLE) {
			const float v = pixel(b.pair, b.first * T::PS * T::PS + t);
			lds[t] = v;
			xs[e] = v;
		} else {
			lds[t] = patches[e];
		}
	}
	__syncthreads();
	tower_forward<T>(params, lds);
	if (t < B::NFEAT) scatter_feature(a0, b.pair, b.first + t / FM, t % FM, lds[lds_act<T>(T::NL) + t]);
}

// Launch 1 on KITTI's store: train_slow.hip's tower_forward_kernel.
template <bool SAMPLE>
__global__ void __launch_bounds__(NT) depth_tower_forward_kernel(const float *__restrict__ patches, const float *__restrict__ x0,
                                                                 const float *__restrict__ x1, int n_img, int H, int W,
                                                                 const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                                 const float *__restrict__ prm, const float *__restrict__ params,
                                                                 float *__restrict__ xs, float *__restrict__ a0)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	forward_block<KittiTower, SAMPLE>(patches, params, xs, a0, lds, [&](int pair, int i) {
		return sample_pair_pixel<KittiTower::PS>(x0, x1, n_img, H, W, nnz, n_nnz, rows[pair], prm + (int64_t)pair * NPRM, i);
	});
}

// Launch 1 on the ragged store: train_mb_slow.hip's mb_tower_forward_kernel.
template <bool SAMPLE>
__global__ void __launch_bounds__(NT) depth_mb_tower_forward_kernel(const float *__restrict__ patches, const float *__restrict__ planes,
                                                                    const mc_train_mb_plane *__restrict__ table, int n_planes,
                                                                    const float *__restrict__ nnz, int64_t n_nnz, const int32_t *__restrict__ rows,
                                                                    const int32_t *__restrict__ src, const float *__restrict__ prm,
                                                                    const float *__restrict__ params, float *__restrict__ xs, float *__restrict__ a0)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	forward_block<MbTower, SAMPLE>(patches, params, xs, a0, lds, [&](int pair, int i) {
		return sample_mb_pixel<MbTower::PS>(planes, table, n_planes, nnz, n_nnz, rows[pair], src + 2 * (int64_t)pair, prm + (int64_t)pair * NPRM, i);
	});
}

// The launch before the update, for either tower: RECOMPUTES the forward pass of the workgroup's patches (given, or what launch 1
// sampled), takes the gradient of their features from dfeat (2n, 224), then the backward pass; the convolutions' gradients go to
// the workgroup's row of slab.
template <class T>
__global__ void __launch_bounds__(NT) depth_tower_backward_kernel(const float *__restrict__ patches, const float *__restrict__ params,
                                                                  const float *__restrict__ dfeat, float *__restrict__ slab)
{
	extern __shared__ __attribute__((aligned(16))) float lds[];
	using B = Block<T>;
	const B b;
	const int t = threadIdx.x;
	float *AL = lds + lds_act<T>(T::NL);
	if (t < B::PIX) lds[t] = patches[(int64_t)blockIdx.x * B::PIX + t];
	__syncthreads();
	tower_forward<T>(params, lds);
	if (t < B::NFEAT) {   // the gradient of the last activations, masked by their ReLU
		const float d = gather_feature_grad(dfeat, b.pair, b.first + t / FM, t % FM);
		AL[t] = AL[t] > 0.f ? d : 0.f;
	}
	__syncthreads();
	tower_backward<T>(params, slab + (int64_t)blockIdx.x * n_conv<T>(), lds);
}

// The last launch: the convolutions' gradient is the slab's n_rows rows summed in order, the FC stack's is gfc as it is;
// v = mom * v - lr * g; w += v.  One kernel for both towers and every depth.
__global__ void __launch_bounds__(256) train_slow_depth_sgd_kernel(const float *__restrict__ slab, const float *__restrict__ gfc, int n_rows,
                                                                   int n_conv, int n_params, float *__restrict__ params, float *__restrict__ moms,
                                                                   float lr, float mom)
{
	const int j = blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= n_params) return;
	sgd_update(j, slab, gfc, n_rows, n_conv, params, moms, lr, mom);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
template <class T> static const void *const *tower_kernels();
template <> const void *const *tower_kernels<KittiTower>()
{
	static const void *const ks[3] = {(const void *)depth_tower_forward_kernel<true>, (const void *)depth_tower_forward_kernel<false>,
	                                  (const void *)depth_tower_backward_kernel<KittiTower>};
	return ks;
}
template <> const void *const *tower_kernels<MbTower>()
{
	static const void *const ks[3] = {(const void *)depth_mb_tower_forward_kernel<true>, (const void *)depth_mb_tower_forward_kernel<false>,
	                                  (const void *)depth_tower_backward_kernel<MbTower>};
	return ks;
}

// Lets tower T's three kernels take its LDS; once per tower (train_net.h's prepare_kernels is once per library).
template <class T> static int prepare_tower()
{
	static int rc = -1;
	if (rc >= 0) return rc;
	for (int k = 0; k < 3; ++k) {
		const hipError_t e = hipFuncSetAttribute(tower_kernels<T>()[k], hipFuncAttributeMaxDynamicSharedMemorySize, (int)TOWER_LDS_BYTES<T>);
		if (e != hipSuccess) {
			set_error("%s: hipFuncSetAttribute(%zu bytes of LDS): %s", PREFIX, TOWER_LDS_BYTES<T>, hipGetErrorString(e));
			return (int)e;
		}
	}
	rc = 0;
	return rc;
}

// refuses every l2 outside [1, 7]
static int check_depth(int l2)
{
	MC_REQUIRE(l2 >= MIN_L2, "%s: l2 %d outside [%d, %d]: the head reads a hidden Linear's %d activations, and a net without one has none", PREFIX,
	           l2, MIN_L2, MAX_DEPTH, NH);
	MC_REQUIRE(l2 <= MAX_DEPTH, "%s: l2 %d outside [%d, %d]: prediction's mc_fc_stack takes %d layers, the last Linear among them", PREFIX, l2,
	           MIN_L2, MAX_DEPTH, MAX_DEPTH + 1);
	return 0;
}

// false (and a message) for a store that is neither of the two
static bool shape_of(int store, int l2, StepShape *s)
{
	if (store == KittiTower::STORE) {
		*s = shape_at<KittiTower>(l2);
	} else if (store == MbTower::STORE) {
		*s = shape_at<MbTower>(l2);
	} else {
		set_error("%s: store %d is neither MC_TRAIN_SLOW_DEPTH_KITTI (%d) nor MC_TRAIN_SLOW_DEPTH_MB (%d)", PREFIX, store, KittiTower::STORE,
		          MbTower::STORE);
		return false;
	}
	return true;
}

// One step of tower T at the depth of s: forward(ws, n_blocks) launches T's forward kernel (patches given or sampled).
template <class T, class Forward>
static int enqueue_step(const StepShape &s, Forward forward, const float *patches, int n_pairs, float *params, float *moms, float lr, float mom,
                        float *loss_out, void *workspace, hipStream_t st)
{
	const StepWorkspace ws = carve(s, (float *)workspace, n_pairs);
	const int n_blocks = Block<T>::PER_PAIR * n_pairs;
	forward(ws, n_blocks);
	if (int rc = check_launch(PREFIX, "tower_forward")) return rc;
	if (int rc = enqueue_fc(s, ws, params, n_pairs, loss_out, st)) return rc;
	depth_tower_backward_kernel<T><<<n_blocks, NT, TOWER_LDS_BYTES<T>, st>>>(patches ? patches : ws.xs, params, ws.dfeat, ws.slab);
	if (int rc = check_launch(PREFIX, "tower_backward")) return rc;
	train_slow_depth_sgd_kernel<<<cdiv(s.n_params(), 256), 256, 0, st>>>(ws.slab, ws.gfc, n_blocks, s.n_conv, s.n_params(), params, moms, lr, mom);
	return check_launch(PREFIX, "sgd");
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_slow_depth_version(void) { return MC_TRAIN_SLOW_DEPTH_ABI_VERSION; }

const char *mc_train_slow_depth_last_error(void) { return last_error(); }

int mc_train_slow_depth_nparams(int store, int l2)
{
	StepShape s;
	if (check_depth(l2) || !shape_of(store, l2, &s)) return 0;
	return s.n_params();
}

size_t mc_train_slow_depth_workspace_bytes(int store, int l2, int n_pairs)
{
	StepShape s;
	if (check_depth(l2) || !shape_of(store, l2, &s)) return 0;
	return step_workspace_bytes(s, n_pairs);
}

int mc_train_slow_depth_step_batch(int store, int l2, const float *patches, int n_pairs, float *params, float *moms, float lr, float mom,
                                   float *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
	StepShape s;
	if (int rc = check_depth(l2)) return rc;
	if (!shape_of(store, l2, &s)) return MC_EINVAL;
	if (int rc = check_step_args(s, n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	MC_REQUIRE(patches && loss_out, "%s_step_batch: null pointer", PREFIX);
	const hipStream_t st = as_stream(stream);
	if (store == KittiTower::STORE) {
		if (int rc = prepare_tower<KittiTower>()) return rc;
		return enqueue_step<KittiTower>(s, [&](const StepWorkspace &ws, int n_blocks) {
			depth_tower_forward_kernel<false><<<n_blocks, NT, TOWER_LDS_BYTES<KittiTower>, st>>>(patches, nullptr, nullptr, 0, 0, 0, nullptr, 0, nullptr,
			                                                                                      nullptr, params, ws.xs, ws.a[0]);
		}, patches, n_pairs, params, moms, lr, mom, loss_out, workspace, st);
	}
	if (int rc = prepare_tower<MbTower>()) return rc;
	return enqueue_step<MbTower>(s, [&](const StepWorkspace &ws, int n_blocks) {
		depth_mb_tower_forward_kernel<false><<<n_blocks, NT, TOWER_LDS_BYTES<MbTower>, st>>>(patches, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr,
		                                                                                      nullptr, params, ws.xs, ws.a[0]);
	}, patches, n_pairs, params, moms, lr, mom, loss_out, workspace, st);
}

int mc_train_slow_depth_run(int l2, const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz,
                            const int32_t *perm, int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const float *prm, float *params, float *moms,
                            float lr, float mom, float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_depth(l2)) return rc;
	const StepShape s = shape_at<KittiTower>(l2);
	if (int rc = check_image_args(PREFIX, x0, x1, n_img, H, W, nnz, n_nnz)) return rc;
	if (int rc = check_step_args(s, n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	const hipStream_t st = as_stream(stream);
	return run_steps(PREFIX, perm && prm && losses, t0, n_steps, n_pairs, n_perm, prepare_tower<KittiTower>, [&](int step, int64_t first) {
		const int32_t *rows = perm + t0 + first;
		const float *p = prm + first * NPRM;
		return enqueue_step<KittiTower>(s, [&](const StepWorkspace &ws, int n_blocks) {
			depth_tower_forward_kernel<true><<<n_blocks, NT, TOWER_LDS_BYTES<KittiTower>, st>>>(nullptr, x0, x1, n_img, H, W, nnz, n_nnz, rows, p, params,
			                                                                                     ws.xs, ws.a[0]);
		}, nullptr, n_pairs, params, moms, lr, mom, losses + step, workspace, st);
	});
}

int mc_train_slow_depth_mb_run(int l2, const float *planes, const mc_train_mb_plane *table, int n_planes, const float *nnz, int64_t n_nnz,
                               const int32_t *perm, int64_t n_perm, int64_t t0, int n_steps, int n_pairs, const int32_t *src, const float *prm,
                               float *params, float *moms, float lr, float mom, float *losses, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_depth(l2)) return rc;
	const StepShape s = shape_at<MbTower>(l2);
	if (int rc = check_store_args(PREFIX, planes, table, n_planes, nnz, n_nnz)) return rc;
	if (int rc = check_step_args(s, n_pairs, params, moms, workspace, workspace_bytes)) return rc;
	const hipStream_t st = as_stream(stream);
	return run_steps(PREFIX, perm && src && prm && losses, t0, n_steps, n_pairs, n_perm, prepare_tower<MbTower>, [&](int step, int64_t first) {
		const int32_t *rows = perm + t0 + first, *sr = src + 2 * first;
		const float *p = prm + first * NPRM;
		return enqueue_step<MbTower>(s, [&](const StepWorkspace &ws, int n_blocks) {
			depth_mb_tower_forward_kernel<true><<<n_blocks, NT, TOWER_LDS_BYTES<MbTower>, st>>>(nullptr, planes, table, n_planes, nnz, n_nnz, rows, sr, p,
			                                                                                     params, ws.xs, ws.a[0]);
		}, nullptr, n_pairs, params, moms, lr, mom, losses + step, workspace, st);
	});
}

}  // extern "C"
