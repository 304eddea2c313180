/*
 * mc_train_slow_depth.h -- C ABI of libmctrainslowdepth.so: training of the
 * accurate architecture at any number of hidden Linears, `-l2 1..7 -nh2 384`
 * (main.lua:73-78, 120-124, 663-695), on the MI355X (gfx950), from either
 * image store with that store's tower:
 *   MC_TRAIN_SLOW_DEPTH_KITTI  KITTI's store (mc_train.h), four valid 3x3
 *                              convolutions of 112 maps on 9 x 9 patches, one
 *                              workgroup per pair (mc_train_slow.h);
 *   MC_TRAIN_SLOW_DEPTH_MB     Middlebury's ragged store (mc_train_mb.h), five
 *                              convolutions on 11 x 11 patches, one workgroup
 *                              per patch (mc_train_mb_slow.h).
 *
 * The net of depth l2 is the store's tower, Reshape(bs, 224), Linear
 * 224 -> 384 (l2 times) -> 1 with ReLUs between, Sigmoid, BCECriterion2.  The
 * step is the one of libmctrainslow.so (KITTI, l2 = 4) and libmctrainmbslow.so
 * (Middlebury, l2 = 3) and equals theirs bit for bit at those depths.  The
 * tower kernels depend on the store alone; l2 is the host's loop count over the
 * FC kernels, which take their layer by pointer.  A step is 2 l2 + 4 launches.
 *
 *   l2   FC parameters   parameters, KITTI   parameters, Middlebury   launches
 *    1        86 785          426 929              539 937                6
 *    2       234 625          574 769              687 777                8
 *    3       382 465          722 609              835 617               10
 *    4       530 305          870 449              983 457               12
 *    5       678 145        1 018 289            1 131 297               14
 *    6       825 985        1 166 129            1 279 137               16
 *    7       973 825        1 313 969            1 426 977               18
 * NFC(l2) = 86 785 + (l2 - 1) * 147 840; parameters = NCONV + NFC with NCONV
 * 340 144 (KITTI) or 453 152 (Middlebury).  l2 = 0 is refused: the head reads
 * 384-wide activations, which a net without a hidden Linear has not.  l2 = 8 is
 * refused: prediction's mc_fc_stack takes 8 layers, the last one among them.
 *
 * Conventions are those of mc_train_slow.h: device pointers to contiguous fp32
 * (int32 / int64 where named), explicit dims, `stream` a hipStream_t (NULL =
 * default), asynchronous, never synchronising, never allocating, return 0 /
 * hipError_t / MC_EINVAL with a thread-local message in
 * mc_train_slow_depth_last_error().  Every argument check runs on the host
 * before the first launch; a refused call writes nothing.
 *
 * Parameters live in ONE flat fp32 buffer of mc_train_slow_depth_nparams(store,
 * l2) floats: the tower's w1 b1 .. as in its parent's header, then
 *   fw1 (384,224) fb1 (384)  fw2 (384,384) fb2 .. fw<l2> fb<l2>
 *   fw<l2+1> (1,384) fb<l2+1> (1)
 * The momenta buffer has the same layout.  Both must be 16-byte aligned, and
 * so must the workspace.  The batch, the augmentation floats
 * (MC_TRAIN_SLOW_DEPTH_NPRM per pair), the criterion and the order of every
 * sum are the parents'.
 */
#ifndef MC_TRAIN_SLOW_DEPTH_H
#define MC_TRAIN_SLOW_DEPTH_H

#include <stddef.h>
#include <stdint.h>

#include "mc_train_mb.h" /* mc_train_mb_plane: a record of the ragged store's table */

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_TRAIN_SLOW_DEPTH_ABI_VERSION 1
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif
#define MC_TRAIN_SLOW_DEPTH_KITTI 0          /* store: x0, x1 (n_img, H, W) */
#define MC_TRAIN_SLOW_DEPTH_MB 1             /* store: planes, table, src */
#define MC_TRAIN_SLOW_DEPTH_MIN_L2 1
#define MC_TRAIN_SLOW_DEPTH_MAX_L2 7         /* mc_fc_stack's 8 layers less the last */
#define MC_TRAIN_SLOW_DEPTH_NH2 384          /* units per hidden Linear (-nh2) */
#define MC_TRAIN_SLOW_DEPTH_NPRM 18          /* augmentation floats per pair, MC_TRAIN_NPRM's */
#define MC_TRAIN_SLOW_DEPTH_NFC1 86785       /* 384*224 + 384 + 384 + 1: the FC parameters at l2 = 1 */
#define MC_TRAIN_SLOW_DEPTH_NFC_STEP 147840  /* 384*384 + 384: one more hidden Linear */
#define MC_TRAIN_SLOW_DEPTH_MAX_PAIRS 1024   /* KITTI's store: MC_TRAIN_SLOW_MAX_PAIRS */
#define MC_TRAIN_SLOW_DEPTH_MB_MAX_PAIRS 256 /* the ragged store: MC_TRAIN_MB_SLOW_MAX_PAIRS */

int mc_train_slow_depth_version(void);
const char *mc_train_slow_depth_last_error(void);

/* Floats of the parameter buffer, NCONV(store) + 86 785 + (l2 - 1) * 147 840;
 * 0 for another store or l2 outside [1, 7]. */
int mc_train_slow_depth_nparams(int store, int l2);

/* Bytes of the workspace of a step of n_pairs pairs (the parents', with l2
 * activation buffers); 0 for another store, l2 outside [1, 7] or n_pairs
 * outside [1, the store's MAX_PAIRS]. */
size_t mc_train_slow_depth_workspace_bytes(int store, int l2, int n_pairs);

/* mc_train_slow_step_batch (store KITTI: patches (n_pairs, 3, 9, 9)) or
 * mc_train_mb_slow_step_batch (store MB: (n_pairs, 3, 11, 11)) at depth l2. */
int mc_train_slow_depth_step_batch(int store, int l2, const float *patches, int n_pairs, float *params,
                                   float *moms, float lr, float mom, float *loss_out,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* mc_train_slow_run at depth l2. */
int mc_train_slow_depth_run(int l2, const float *x0, const float *x1, int n_img, int H, int W,
                            const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                            int n_steps, int n_pairs, const float *prm, float *params, float *moms,
                            float lr, float mom, float *losses,
                            void *workspace, size_t workspace_bytes, void *stream);

/* mc_train_mb_slow_run at depth l2. */
int mc_train_slow_depth_mb_run(int l2, const float *planes, const mc_train_mb_plane *table, int n_planes,
                               const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                               int n_steps, int n_pairs, const int32_t *src, const float *prm,
                               float *params, float *moms, float lr, float mom,
                               float *losses, void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
