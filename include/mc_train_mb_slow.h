/*
 * mc_train_mb_slow.h -- C ABI of libmctrainmbslow.so: training of the accurate
 * architecture on Middlebury (main.lua:602-890 with dataset mb, arch slow) on
 * the MI355X (gfx950).
 *
 * The net is fixed (main.lua:116-130): five valid 3x3 convolutions
 * 1 -> 112 -> 112 -> 112 -> 112 -> 112 on 11 x 11 patches
 * (11 -> 9 -> 7 -> 5 -> 3 -> 1) with ReLU after every one, Reshape(bs, 224),
 * Linear 224 -> 384 -> 384 -> 384 -> 1 (-l2 3) with ReLUs between, Sigmoid,
 * BCECriterion2.
 *
 * Conventions are those of mc_train_mb.h: device pointers to contiguous fp32
 * (int32 / int64 where named), explicit dims, `stream` a hipStream_t (NULL =
 * default), asynchronous, never synchronising, never allocating, return 0 /
 * hipError_t / MC_EINVAL with a thread-local message in
 * mc_train_mb_slow_last_error().  Every argument check runs on the host
 * before the first launch and writes nothing.  fp32 throughout
 * (v_mfma_f32_16x16x4_f32 for the GEMMs), no float atomics, every reduction
 * in a fixed order: a step is bitwise reproducible.
 *
 * Parameters live in ONE flat fp32 buffer of MC_TRAIN_MB_SLOW_NPARAMS floats,
 * laid out as mc_train_slow.h does:
 *   w1 (112,1,3,3) b1 (112)  w2 (112,112,3,3) b2  w3 b3  w4 b4  w5 b5
 *   fw1 (384,224) fb1 (384)  fw2 (384,384) fb2  fw3 fb3
 *   fw4 (1,384) fb4 (1)
 * The momenta buffer has the same layout.  Both must be 16-byte aligned, and
 * so must the workspace.
 *
 * The image store (planes, table, src), the nnz rows and the
 * MC_TRAIN_MB_SLOW_NPRM augmentation floats per pair are mc_train_mb.h's; the
 * batch is mc_train_slow.h's: three distinct patches per pair (left,
 * positive, negative), sample 2i of the criterion is (left, positive) of pair
 * i with target 0, sample 2i+1 is (left, negative) with target 1; the input
 * row of the first Linear is [feat(left) | feat(right)].  The left patch's
 * tower runs once and receives both samples' gradients (positive's, then
 * negative's, added in that order).
 *
 * The towers run ONE WORKGROUP PER PATCH (3 * n_pairs workgroups, 74 432
 * bytes of LDS each), and the convolutions' gradients go to one row per patch
 * of a slab of 3 * n_pairs x MC_TRAIN_MB_SLOW_NCONV floats, summed in the
 * order 3 * pair + patch.  A step is ten kernel launches.
 *
 * BCECriterion2 and Sigmoid keep the reference's fp32 operation order (see
 * mc_train_slow.h): where the output saturates to 0 or 1 the gradient is
 * exactly 0, as in the reference.
 *
 * The library has no sampler entry point of its own: mc_train_mb_sample of
 * libmctrainmb.so draws the same patches (one shared device function).
 */
#ifndef MC_TRAIN_MB_SLOW_H
#define MC_TRAIN_MB_SLOW_H

#include <stddef.h>
#include <stdint.h>

#include "mc_train_mb.h" /* mc_train_mb_plane */

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_TRAIN_MB_SLOW_ABI_VERSION 1
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif
#define MC_TRAIN_MB_SLOW_WS 11           /* patch size: get_window_size of 5 valid 3x3 convolutions */
#define MC_TRAIN_MB_SLOW_FM 112          /* feature maps per convolution (-fm) */
#define MC_TRAIN_MB_SLOW_L1 5            /* convolution layers (-l1) */
#define MC_TRAIN_MB_SLOW_L2 3            /* hidden Linear layers (-l2) */
#define MC_TRAIN_MB_SLOW_NH2 384         /* units per hidden Linear (-nh2) */
#define MC_TRAIN_MB_SLOW_NPRM 18         /* augmentation floats per pair, as MC_TRAIN_NPRM */
#define MC_TRAIN_MB_SLOW_NCONV 453152    /* 112*9 + 112 + 4 * (112*112*9 + 112) */
#define MC_TRAIN_MB_SLOW_NFC 382465      /* 384*224 + 384 + 2 * (384*384 + 384) + 384 + 1 */
#define MC_TRAIN_MB_SLOW_NPARAMS 835617  /* NCONV + NFC */
#define MC_TRAIN_MB_SLOW_MAX_PAIRS 256   /* pairs per batch: bs <= 512; the workspace grows by ~5.5 MB per pair (1.4 GB at 256) */

int mc_train_mb_slow_version(void);
const char *mc_train_mb_slow_last_error(void);

/* Bytes of the workspace a step of n_pairs pairs needs (the patches, the FC
 * stack's activations and gradients for 2 * n_pairs rows, the FC parameters'
 * gradient, and one row of MC_TRAIN_MB_SLOW_NCONV floats per PATCH, three per
 * pair, for the convolutions' gradients); 0 if n_pairs is outside
 * [1, MC_TRAIN_MB_SLOW_MAX_PAIRS]. */
size_t mc_train_mb_slow_workspace_bytes(int n_pairs);

/* One SGD step (main.lua:853-874) on a given batch of patches
 * (n_pairs, 3, 11, 11): forward, BCECriterion2 (mean over the 2 * n_pairs
 * samples), backward, then  v = mom * v - lr * g;  w += v.  loss_out[0]
 * receives the batch's loss.  Ten kernel launches. */
int mc_train_mb_slow_step_batch(const float *patches, int n_pairs, float *params, float *moms,
                                float lr, float mom, float *loss_out,
                                void *workspace, size_t workspace_bytes, void *stream);

/* n_steps full steps (main.lua:787-875) with no host round trip: step s
 * samples pair i from nnz row perm[t0 + s * n_pairs + i] (0-based int32),
 * planes src[2 * (s * n_pairs + i) ...] and
 * prm[(s * n_pairs + i) * MC_TRAIN_MB_SLOW_NPRM ...], then trains on it.
 * losses[s] receives step s's loss.  mc_train_mb_run without margin and pow. */
int mc_train_mb_slow_run(const float *planes, const mc_train_mb_plane *table, int n_planes,
                         const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                         int n_steps, int n_pairs, const int32_t *src, const float *prm,
                         float *params, float *moms, float lr, float mom,
                         float *losses, void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
