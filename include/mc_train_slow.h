/*
 * mc_train_slow.h -- C ABI of libmctrainslow.so: training of the accurate
 * architecture (main.lua:663-677, 753-875, arch slow on kitti / kitti2015) on
 * the MI355X (gfx950).
 *
 * The net is fixed (main.lua:74-78): four valid 3x3 convolutions
 * 1 -> 112 -> 112 -> 112 -> 112 on 9 x 9 patches (9 -> 7 -> 5 -> 3 -> 1) with
 * ReLU after every one, Reshape(bs, 224), Linear 224 -> 384 -> 384 -> 384 ->
 * 384 -> 1 with ReLUs between, Sigmoid, BCECriterion2.
 *
 * Conventions are those of mc_train.h: device pointers to contiguous fp32
 * (int32 where named), `stream` a hipStream_t (NULL = default), asynchronous,
 * never synchronising, never allocating, return 0 / hipError_t / MC_EINVAL
 * with a thread-local message in mc_train_slow_last_error().  Every argument
 * check happens on the host before the first launch and writes nothing.
 * fp32 throughout (v_mfma_f32_16x16x4_f32 for the GEMMs), no float atomics,
 * every reduction in a fixed order: a step is bitwise reproducible.
 *
 * Parameters live in ONE flat fp32 buffer of MC_TRAIN_SLOW_NPARAMS floats in
 * the order of `params` in main.lua:753-770:
 *   w1 (112,1,3,3) b1 (112)  w2 (112,112,3,3) b2  w3 b3  w4 b4
 *   fw1 (384,224) fb1 (384)  fw2 (384,384) fb2  fw3 fb3  fw4 fb4
 *   fw5 (1,384) fb5 (1)
 * The momenta buffer has the same layout.
 *
 * The batch is that of mc_train.h: three distinct patches per pair (left,
 * positive, negative), augmentation parameters of MC_TRAIN_NPRM floats per
 * pair, nnz rows (img 1-based, row, col, disparity).  Sample 2i of the
 * criterion is (left, positive) of pair i with target 0, sample 2i+1 is
 * (left, negative) with target 1 (main.lua:843-849); the input row of the
 * first Linear is [feat(left) | feat(right)], as Reshape produces it.  The
 * left patch's tower runs once and receives both samples' gradients
 * (positive's, then negative's, added in that order).
 *
 * BCECriterion2 and Sigmoid keep the reference's fp32 operation order:
 *   loss   = -sum_r ( t log(o + 1e-12) + (1 - t) log((1 - o) + 1e-12) ) / n
 *   grad_o = -( t / (o + 1e-12) - (1 - t) / ((1 - o) + 1e-12) ) / n
 * and Sigmoid's backward multiplies by o (1 - o): where o saturates to 0 or 1
 * the gradient is exactly 0, as in the reference.
 *
 * The library has no sampler entry point of its own: mc_train_sample of
 * libmctrain.so draws the same patches (one shared device function).
 */
#ifndef MC_TRAIN_SLOW_H
#define MC_TRAIN_SLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_TRAIN_SLOW_ABI_VERSION 1
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif
#define MC_TRAIN_SLOW_WS 9            /* patch size */
#define MC_TRAIN_SLOW_FM 112          /* feature maps per convolution (-fm) */
#define MC_TRAIN_SLOW_L1 4            /* convolution layers (-l1) */
#define MC_TRAIN_SLOW_L2 4            /* hidden Linear layers (-l2) */
#define MC_TRAIN_SLOW_NH2 384         /* units per hidden Linear (-nh2) */
#define MC_TRAIN_SLOW_NPRM 18         /* augmentation floats per pair, as MC_TRAIN_NPRM */
#define MC_TRAIN_SLOW_NCONV 340144    /* 112*9 + 112 + 3 * (112*112*9 + 112) */
#define MC_TRAIN_SLOW_NFC 530305      /* 384*224 + 384 + 3 * (384*384 + 384) + 384 + 1 */
#define MC_TRAIN_SLOW_NPARAMS 870449  /* NCONV + NFC */
#define MC_TRAIN_SLOW_MAX_PAIRS 1024  /* pairs per batch: bs <= 2048; the workspace grows by ~1.4 MB per pair */

int mc_train_slow_version(void);
const char *mc_train_slow_last_error(void);

/* Bytes of the workspace a step of n_pairs pairs needs (the patches, the FC
 * stack's activations and gradients for 2 * n_pairs rows, the FC parameters'
 * gradient, and one row of MC_TRAIN_SLOW_NCONV floats per pair for the
 * convolutions' gradients); 0 if n_pairs is outside
 * [1, MC_TRAIN_SLOW_MAX_PAIRS]. */
size_t mc_train_slow_workspace_bytes(int n_pairs);

/* One SGD step (main.lua:853-874) on a given batch of patches
 * (n_pairs, 3, 9, 9): forward, BCECriterion2 (mean over the 2 * n_pairs
 * samples), backward, then  v = mom * v - lr * g;  w += v.  loss_out[0]
 * receives the batch's loss.  Twelve kernel launches. */
int mc_train_slow_step_batch(const float *patches, int n_pairs, float *params, float *moms,
                             float lr, float mom, float *loss_out,
                             void *workspace, size_t workspace_bytes, void *stream);

/* n_steps full steps (main.lua:787-875) with no host round trip: step s
 * samples pair i from nnz row perm[t0 + s * n_pairs + i] (0-based int32) with
 * prm[(s * n_pairs + i) * MC_TRAIN_SLOW_NPRM ...], then trains on it.
 * losses[s] receives step s's loss.  mc_train_run without margin and pow. */
int mc_train_slow_run(const float *x0, const float *x1, int n_img, int H, int W,
                      const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                      int n_steps, int n_pairs, const float *prm, float *params, float *moms,
                      float lr, float mom, float *losses,
                      void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
