/*
 * mc_train_depth.h -- C ABI of libmctraindepth.so: training of the fast
 * architecture at any depth the step can hold, `-l1 1..5 -fm 64 -ks 3`
 * (main.lua:212-214, 240-242, 271-273, 726-746), on the MI355X (gfx950), from
 * either image store: KITTI's (mc_train.h) or Middlebury's ragged one
 * (mc_train_mb.h).
 *
 * The net of depth l1 is l1 valid 3x3 convolutions 1 -> 64 -> ... -> 64 on
 * patches of side 2 * l1 + 1, ReLU after all but the last, then Normalize2,
 * StereoJoin1 and the Margin2 hinge.  Every call takes l1 first and dispatches
 * to that depth's kernels; the step is the one of libmctrain.so (l1 = 4) and
 * libmctrainmb.so (l1 = 5), instantiated once per depth, and equals theirs bit
 * for bit at those depths.
 *
 *   l1  patch  parameters  LDS of a step (bytes)
 *    1   3x3        640     34 048
 *    2   5x5     37 568     40 960
 *    3   7x7     74 496     60 672
 *    4   9x9    111 424     98 304
 *    5  11x11   148 352    161 024
 * l1 = 6 is refused: its step would keep 254 464 bytes in LDS (221 696 of
 * them the activations of a pair's three 13 x 13 patches), a CU has 163 840.
 *
 * Conventions are those of mc_train.h: device pointers to contiguous fp32
 * (int32 / int64 where named), explicit dims, `stream` a hipStream_t (NULL =
 * default), asynchronous, never synchronising, never allocating, return 0 /
 * hipError_t / MC_EINVAL with a thread-local message in
 * mc_train_depth_last_error().  Every argument check runs on the host before
 * the first launch; a refused call writes nothing.
 *
 * Parameters live in ONE flat fp32 buffer of mc_train_depth_nparams(l1) floats
 * in the order w1 (64,1,3,3), b1 (64), w2 (64,64,3,3), b2, ... -- at l1 = 4
 * and 5 the layouts of mc_train.h and mc_train_mb.h.  A pair keeps three
 * patches (0 left, 1 positive, 2 negative) and MC_TRAIN_DEPTH_NPRM
 * augmentation floats, mc_train.h's 18 in the same order.
 */
#ifndef MC_TRAIN_DEPTH_H
#define MC_TRAIN_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#include "mc_train_mb.h" /* mc_train_mb_plane: a record of the ragged store's table */

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_TRAIN_DEPTH_ABI_VERSION 1
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif
#define MC_TRAIN_DEPTH_MIN_L1 1
#define MC_TRAIN_DEPTH_MAX_L1 5      /* the deepest net whose step fits a CU's LDS */
#define MC_TRAIN_DEPTH_FM 64         /* feature maps per layer (-fm) */
#define MC_TRAIN_DEPTH_NPRM 18       /* augmentation floats per pair, MC_TRAIN_NPRM's */
#define MC_TRAIN_DEPTH_MAX_PAIRS 1024 /* both stores; the slab of l1 = 5 is then 0.6 GB */

int mc_train_depth_version(void);
const char *mc_train_depth_last_error(void);

/* Patch side 2 * l1 + 1; 0 for l1 outside [1, 5]. */
int mc_train_depth_ws(int l1);

/* Floats of the parameter buffer, 640 + (l1 - 1) * 36 928; 0 for l1 outside
 * [1, 5]. */
int mc_train_depth_nparams(int l1);

/* Bytes of the workspace of a step of n_pairs pairs: a gradient row and a
 * loss per pair, n_pairs * (nparams + 1) * 4; 0 for l1 outside [1, 5] or
 * n_pairs outside [1, MC_TRAIN_DEPTH_MAX_PAIRS]. */
size_t mc_train_depth_workspace_bytes(int l1, int n_pairs);

/* mc_train_step_batch at depth l1: patches (n_pairs, 3, ws, ws). */
int mc_train_depth_step_batch(int l1, const float *patches, int n_pairs, float *params, float *moms,
                              float lr, float mom, float margin, int pow, float *loss_out,
                              void *workspace, size_t workspace_bytes, void *stream);

/* mc_train_sample and mc_train_run (the KITTI store) at depth l1: out is
 * (n_pairs, 3, ws, ws). */
int mc_train_depth_sample(int l1, const float *x0, const float *x1, int n_img, int H, int W,
                          const float *nnz, int64_t n_nnz, const int32_t *rows, const float *prm,
                          int n_pairs, float *out, void *stream);
int mc_train_depth_run(int l1, const float *x0, const float *x1, int n_img, int H, int W,
                       const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                       int n_steps, int n_pairs, const float *prm, float *params, float *moms,
                       float lr, float mom, float margin, int pow, float *losses,
                       void *workspace, size_t workspace_bytes, void *stream);

/* mc_train_mb_sample and mc_train_mb_run (the ragged store) at depth l1. */
int mc_train_depth_mb_sample(int l1, const float *planes, const mc_train_mb_plane *table, int n_planes,
                             const float *nnz, int64_t n_nnz, const int32_t *rows, const int32_t *src,
                             const float *prm, int n_pairs, float *out, void *stream);
int mc_train_depth_mb_run(int l1, const float *planes, const mc_train_mb_plane *table, int n_planes,
                          const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                          int n_steps, int n_pairs, const int32_t *src, const float *prm,
                          float *params, float *moms, float lr, float mom, float margin, int pow,
                          float *losses, void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
