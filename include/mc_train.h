/*
 * mc_train.h -- C ABI of libmctrain.so: training of the fast architecture
 * (main.lua:602-890, arch fast on kitti / kitti2015) on the MI355X (gfx950).
 *
 * The net is fixed: four valid 3x3 convolutions 1 -> 64 -> 64 -> 64 -> 64 on
 * 9 x 9 patches (9 -> 7 -> 5 -> 3 -> 1), ReLU after all but the last, then
 * Normalize2, StereoJoin1 and the Margin2 hinge (main.lua:726-746).
 *
 * Conventions are those of mc_adcensus.h: device pointers to contiguous fp32
 * (int32 where named), explicit dims, `stream` a hipStream_t (NULL = default),
 * asynchronous, never synchronising, never allocating (workspaces come from
 * the caller, sized by mc_train_workspace_bytes), return 0 / hipError_t /
 * MC_EINVAL with a thread-local message in mc_train_last_error().
 *
 * Parameters live in ONE flat fp32 buffer of MC_TRAIN_NPARAMS floats in the
 * order w1 (64,1,3,3), b1 (64), w2 (64,64,3,3), b2, w3, b3, w4, b4 -- the
 * order of `params` in main.lua:750-765.  The momenta buffer has the same
 * layout.
 *
 * A training pair i of a batch (bs = 2 * n_pairs, main.lua:787-851) is the
 * quadruple of patches 4i-3 .. 4i of the reference's x_batch_tr.  Patches
 * 4i-3 and 4i-1 are drawn with identical arguments (main.lua:843,845), so the
 * library keeps three distinct patches per pair, in this order:
 *   0: left  (x0 at (row, col)),
 *   1: positive (x1 at (row, col - d + d_pos)),
 *   2: negative (x1 at (row, col - d + d_neg));
 * the left patch's forward pass is computed once and its gradient is the sum
 * of both pairs' contributions.
 *
 * Per-pair augmentation parameters: MC_TRAIN_NPRM floats per pair, in the
 * order of main.lua:790-814:
 *   0 d_pos  1 d_neg  2 scale_x  3 scale_y  4 phi  5 trans_x  6 trans_y
 *   7 hshear  8 brightness  9 contrast            (the left patch)
 *   10 scale_x_  11 scale_y_  12 phi_  13 trans_x_  14 trans_y_  15 hshear_
 *   16 brightness_  17 contrast_                   (both right patches)
 *
 * nnz: (n_nnz, 4) fp32 rows (img 1-based, row, col, disparity), as
 * make_dataset2 writes them (adcensus.cu:1900-1929).  Images: x0 / x1 are
 * (n_img, H, W) fp32, main.lua's X0 / X1 with their single channel dropped.
 *
 * Dataset preparation (preprocess_kitti.lua:97-113, since ABI 2): the
 * ground-truth filters and make_dataset2 for a batch of maps, so that
 * mc_cnn_amd.preprocess_kitti writes data.kitti / data.kitti2015 on the GPU.
 */
#ifndef MC_TRAIN_H
#define MC_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_TRAIN_ABI_VERSION 2
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif
#define MC_TRAIN_WS 9          /* patch size: get_window_size of 4 valid 3x3 convolutions */
#define MC_TRAIN_FM 64         /* feature maps per layer (-fm) */
#define MC_TRAIN_L1 4          /* convolution layers (-l1) */
#define MC_TRAIN_NPRM 18       /* augmentation floats per pair */
#define MC_TRAIN_NPARAMS 111424 /* 64*9 + 64 + 3 * (64*64*9 + 64) */
#define MC_TRAIN_MAX_PAIRS 4096
#define MC_TRAIN_GT_MAX_W 8192 /* widest ground-truth map mc_train_filter_gt takes (one row in LDS) */

int mc_train_version(void);
const char *mc_train_last_error(void);

/* Bytes of the workspace a step of n_pairs pairs needs: per-pair gradient
 * partials (n_pairs x MC_TRAIN_NPARAMS floats) and per-pair losses. */
size_t mc_train_workspace_bytes(int n_pairs);

/* make_patch (main.lua:603-619) for a batch: the 3 distinct patches of each
 * pair, out (n_pairs, 3, 9, 9).  Pair i reads nnz row rows[i] (0-based int32)
 * and prm[i * MC_TRAIN_NPRM ...].  The warp is OpenCV 2.4 cvWarpAffine with
 * CV_INTER_CUBIC + CV_WARP_FILL_OUTLIERS (cv.cpp:19-43): the matrix is
 * inverted, source coordinates are quantised to 1/32 pixel, bicubic weights
 * use A = -0.75, taps outside the image read 0; then dst * contrast +
 * brightness.  A pair whose rows[i] is outside [0, n_nnz) or whose nnz image
 * id is outside [1, n_img] reads 0 everywhere: its patches are
 * 0 * contrast + brightness. */
int mc_train_sample(const float *x0, const float *x1, int n_img, int H, int W,
                    const float *nnz, int64_t n_nnz, const int32_t *rows, const float *prm,
                    int n_pairs, float *out, void *stream);

/* One SGD step (main.lua:853-874) on a given batch of patches
 * (n_pairs, 3, 9, 9) in the order above: forward, Margin2 (margin, pow 1 or
 * 2), backward, then  v = mom * v - lr * g;  w += v.  loss_out[0] receives
 * the batch's mean loss.  Gradients are reduced over the pairs in a fixed
 * order: the step is bitwise reproducible. */
int mc_train_step_batch(const float *patches, int n_pairs, float *params, float *moms,
                        float lr, float mom, float margin, int pow, float *loss_out,
                        void *workspace, size_t workspace_bytes, void *stream);

/* n_steps full steps (main.lua:787-875) with no host round trip: step s
 * samples pair i from nnz row perm[t0 + s * n_pairs + i] (0-based int32) with
 * prm[(s * n_pairs + i) * MC_TRAIN_NPRM ...], then trains on it.
 * losses[s] receives step s's mean loss.  Two kernels per step. */
int mc_train_run(const float *x0, const float *x1, int n_img, int H, int W,
                 const float *nnz, int64_t n_nnz, const int32_t *perm, int64_t n_perm, int64_t t0,
                 int n_steps, int n_pairs, const float *prm, float *params, float *moms,
                 float lr, float mom, float margin, int pow, float *losses,
                 void *workspace, size_t workspace_bytes, void *stream);

/* preprocess_kitti.lua:99-101 on n maps disp (n, H, W), in place, with their
 * left images x0 (n, H, W), in the reference's order (adcensus.cu:1723-1800):
 *   remove_nonvisible: d >= col                        -> 0;
 *   remove_occluded:   some i >= 1 with col + i < W and
 *                      (float)i - d[col + i] < -d[col] -> 0, where d is the
 *                      row as remove_nonvisible left it (the reference's
 *                      kernel races on the row; for non-negative maps with
 *                      exact arithmetic, e.g. PNG16 ground truth, its result
 *                      is this one);
 *   remove_white:      x0 == 255                       -> 0.
 * W <= MC_TRAIN_GT_MAX_W.  n = 0 is a no-op. */
int mc_train_filter_gt(float *disp, const float *x0, int n, int H, int W, void *stream);

/* Bytes of the workspace of mc_train_nnz_count / _fill for n maps of H rows
 * (a count and an offset per row); 0 if n * H is out of range. */
size_t mc_train_nnz_workspace_bytes(int n, int H);

/* make_dataset2 (adcensus.cu:1900-1929), pass 1: counts the pixels with
 * d > 0.5 of each row of disp (n, H, W), scans the counts into the workspace
 * and writes the total to count[0] (device int64).  The caller reads the
 * total to size the output of mc_train_nnz_fill. */
int mc_train_nnz_count(const float *disp, int n, int H, int W, int64_t *count,
                       void *workspace, size_t workspace_bytes, void *stream);

/* Pass 2, on the workspace pass 1 left for the same disp and dims: writes the
 * rows (ids[k], row, col, d) as fp32 (n_nnz, 4) for every d > 0.5 of map k,
 * in map order, then row-major -- the order in which make_dataset2 appends.
 * ids (n) are int32 image ids (1-based in preprocess_kitti.lua).  Rows past
 * n_nnz are not written; nnz is 16-byte aligned. */
int mc_train_nnz_fill(const float *disp, const int32_t *ids, int n, int H, int W, float *nnz, int64_t n_nnz,
                      const void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
