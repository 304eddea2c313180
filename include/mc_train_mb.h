/*
 * mc_train_mb.h -- C ABI of libmctrainmb.so: training of the fast
 * architecture on Middlebury (main.lua:602-890 with dataset mb, arch fast)
 * on the MI355X (gfx950).
 *
 * The net is fixed: `mb fast` is -l1 5 -fm 64 (main.lua:271-272), five valid
 * 3x3 convolutions 1 -> 64 -> 64 -> 64 -> 64 -> 64 on 11 x 11 patches
 * (11 -> 9 -> 7 -> 5 -> 3 -> 1), ReLU after all but the last, then
 * Normalize2, StereoJoin1 and the Margin2 hinge (main.lua:726-746).
 *
 * Conventions are those of mc_train.h: device pointers to contiguous fp32
 * (int32 / int64 where named), explicit dims, `stream` a hipStream_t (NULL =
 * default), asynchronous, never synchronising, never allocating, return 0 /
 * hipError_t / MC_EINVAL with a thread-local message in
 * mc_train_mb_last_error().  Every argument check runs on the host before the
 * first launch.
 *
 * Parameters live in ONE flat fp32 buffer of MC_TRAIN_MB_NPARAMS floats in
 * the order w1 (64,1,3,3), b1 (64), w2 (64,64,3,3), b2, ... w5, b5 -- the
 * order of `params` in main.lua:750-765.  The momenta have the same layout.
 *
 * A training pair keeps three distinct patches, as in mc_train.h: 0 left,
 * 1 positive, 2 negative; the MC_TRAIN_MB_NPRM augmentation floats per pair
 * are mc_train.h's 18, in the same order.
 *
 * The image store is ragged (preprocess_mb.py: X[img][light] is
 * (n_exp, 2, 1, H_img, W_img), every image with its own size, lights and
 * exposures).  Here it is
 *   planes: ONE flat fp32 device buffer that holds every image plane, i.e.
 *           every (light >= 2, exposure, view) of every image, each plane
 *           H x W row-major;
 *   table:  n_planes device records mc_train_mb_plane {int64 offset (in
 *           floats, from `planes`), int32 H, int32 W}, 16 bytes each;
 *   src:    two int32 plane ids per pair: src[2i] is the plane of the left
 *           patch (X[img][light][exp, 1]), src[2i+1] the plane of BOTH right
 *           patches (X[img][light_][exp_, 2], main.lua:828-841).  The host
 *           resolves them from (img, light, exp, light_, exp_).
 * The patch centre comes from the pair's nnz row (img, row, col, d), fp32
 * (n_nnz, 4): (row, col) for the left patch and (row, col - d + d_pos | d_neg)
 * for the right ones.  The img column is not read on the device.
 *
 * The table lives only on the device at call time, so the library cannot
 * check it on the host: the Python loader (train_mb.build_store) refuses a
 * plane with H < 4 or W < 4, or a side of 32768 or more (check_image_args'
 * rule in libmctrain.so).  Should such a record reach the device all the
 * same, the sampler treats its id as out of range (see below) rather than
 * read outside the plane.  Offsets are the caller's: offset + H * W must lie
 * inside `planes`.
 */
#ifndef MC_TRAIN_MB_H
#define MC_TRAIN_MB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_TRAIN_MB_ABI_VERSION 1
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif
#define MC_TRAIN_MB_WS 11         /* patch size: get_window_size of 5 valid 3x3 convolutions */
#define MC_TRAIN_MB_L1 5          /* convolution layers (-l1) */
#define MC_TRAIN_MB_FM 64         /* feature maps per layer (-fm) */
#define MC_TRAIN_MB_NPRM 18       /* augmentation floats per pair, MC_TRAIN_NPRM's */
#define MC_TRAIN_MB_NPARAMS 148352 /* 64*9 + 64 + 4 * (64*64*9 + 64) */
#define MC_TRAIN_MB_MAX_PAIRS 1024

typedef struct mc_train_mb_plane {
	int64_t offset; /* first float of the plane in `planes` */
	int32_t H, W;
} mc_train_mb_plane;

int mc_train_mb_version(void);
const char *mc_train_mb_last_error(void);

/* Bytes of the workspace a step of n_pairs pairs needs: per-pair gradient
 * partials (n_pairs x MC_TRAIN_MB_NPARAMS floats) and per-pair losses; 0 if
 * n_pairs is outside [1, MC_TRAIN_MB_MAX_PAIRS]. */
size_t mc_train_mb_workspace_bytes(int n_pairs);

/* make_patch (main.lua:603-619) for a batch: out (n_pairs, 3, 11, 11).  Pair
 * i reads nnz row rows[i] (0-based int32), planes src[2i] / src[2i+1] and
 * prm[i * MC_TRAIN_MB_NPRM ...].  The warp is mc_train_sample's (one device
 * function, with the patch size as its parameter).  A pair whose rows[i] is
 * outside [0, n_nnz) reads 0 everywhere, and so does a patch whose plane id
 * is outside [0, n_planes): such patches are 0 * contrast + brightness.
 * Nothing is read out of bounds. */
int mc_train_mb_sample(const float *planes, const mc_train_mb_plane *table, int n_planes,
                       const float *nnz, int64_t n_nnz, const int32_t *rows, const int32_t *src,
                       const float *prm, int n_pairs, float *out, void *stream);

/* One SGD step (main.lua:853-874) on given patches (n_pairs, 3, 11, 11):
 * forward, Margin2 (margin, pow 1 or 2), backward, then
 * v = mom * v - lr * g;  w += v.  loss_out[0] receives the batch's mean loss.
 * Gradients are reduced over the pairs in a fixed order, without float
 * atomics: the step is bitwise reproducible.  Two kernels. */
int mc_train_mb_step_batch(const float *patches, int n_pairs, float *params, float *moms,
                           float lr, float mom, float margin, int pow, float *loss_out,
                           void *workspace, size_t workspace_bytes, void *stream);

/* n_steps full steps (main.lua:787-875) with no host round trip: step s
 * samples pair i from nnz row perm[t0 + s * n_pairs + i] (0-based int32),
 * planes src[2 * (s * n_pairs + i) ...] and
 * prm[(s * n_pairs + i) * MC_TRAIN_MB_NPRM ...], then trains on it.
 * losses[s] receives step s's mean loss.  Two kernels per step. */
int mc_train_mb_run(const float *planes, const mc_train_mb_plane *table, int n_planes,
                    const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                    int n_steps, int n_pairs, const int32_t *src, const float *prm,
                    float *params, float *moms, float lr, float mom, float margin, int pow,
                    float *losses, void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
