/*
 * mc_ops.h -- C ABI of libmcops.so: the entries of the reference's `adcensus.*`
 * table (adcensus.cu funcs[], 2061-2096) that its training and dataset scripts
 * call and the other libraries do not serve, on the MI355X (gfx950):
 *
 *   Normalize_backward_input                          Normalize2.lua:17
 *   Margin2                                           Margin2.lua:14
 *   remove_nonvisible, remove_occluded, remove_white  preprocess_kitti.lua:97-99
 *   make_dataset2                                     preprocess_kitti.lua:110-112
 *   subset_dataset                                    main.lua:645
 *
 * Each operator evaluates the reference's expression as written, with fmaf()
 * exactly where the reference's nvcc build contracts, so that the results equal
 * the reference's kernels bit for bit, signs of zeros included.  The library is
 * built with -ffp-contract=off, except the one file that calls powf
 * (csrc/ops_normalize.hip says why).
 *
 * Conventions are those of mc_adcensus.h: pointers to fp32, explicit dims,
 * `stream` a hipStream_t (NULL = default), asynchronous, never synchronising,
 * never allocating, return 0 / hipError_t / MC_EINVAL with a thread-local
 * message in mc_ops_last_error().  Every argument check runs on the host before
 * the launch and writes nothing.  mc_make_dataset2 and mc_subset_dataset are
 * host functions on host pointers, as they are in the reference.
 */
#ifndef MC_OPS_H
#define MC_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_OPS_ABI_VERSION 1
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif
#define MC_OPS_MAX_C 128        /* channels of mc_normalize_backward_input: a pixel tile of both tensors in 64 KiB of LDS */
#define MC_OPS_MAX_W 8192       /* widest row of mc_remove_occluded: one row in LDS */
#define MC_OPS_SUBSET_IMAGES 200 /* subset_dataset's `const int N = 200` (adcensus.cu:1873) */

int mc_ops_version(void);
const char *mc_ops_last_error(void);

/* Normalize_backward_input (adcensus.cu:1335-1377) on device tensors (N, C, H, W), norm (N, 1, H, W) as
 * Normalize_forward left it.  Per element (n, c, p), in fp32:
 *   denom = powf(norm, 1.5f)
 *   sum   = fold over c' = 0 .. C-1, c' != c, ascending, of fmaf(input[c'], grad_output[c'], sum)
 *   grad_input = fmaf(fmaf(-input, input, norm) / denom, grad_output, -(sum * input / denom))
 * The fold leaves out the element's own channel, so it differs between the channels of a pixel and is run once per
 * element (`total - own` is another sum); a workgroup stages a tile of pixels of both tensors in LDS once and folds from there.
 * Refused: null pointers; C outside 1 .. MC_OPS_MAX_C; N, H, W < 1; N * C * H * W >= 2^40. */
int mc_normalize_backward_input(const float *grad_output, const float *input, const float *norm, float *grad_input,
                                int N, int C, int H, int W, void *stream);

/* Margin2 (adcensus.cu:1379-1453) on device tensors: input and grad_input hold n_pairs (pos, neg) pairs, tmp n_pairs losses.
 * With f = neg - pos + margin:
 *   pow 1: tmp = fmaxf(0, f),             grad_input = (-1. * (f > 0), f > 0)
 *   pow 2: tmp = fmaxf(0, f)^2 * 0.5,     grad_input = (-f * (f > 0), f * (f > 0))
 * The sign of zero is the reference's: the first gradient of an inactive pair is -0.0 (pow 1), and -0.0 at f == 0 (pow 2).
 * The module's mean and div(n) (Margin2.lua:15-16) are the caller's.  n_pairs == 0 launches nothing.
 * Refused: null pointers; n_pairs < 0; pow other than 1 and 2 (the reference launches nothing there and returns). */
int mc_margin2(const float *input, float *tmp, float *grad_input, int n_pairs, float margin, int pow, void *stream);

/* remove_nonvisible, remove_occluded, remove_white (adcensus.cu:1723-1796), in place on n device elements in rows of W
 * (x: the image, n elements):
 *   nonvisible: disp[id] = 0 where disp[id] >= column
 *   occluded:   disp[id] = 0 where some i >= 1 inside the row has i - disp[id + i] < -disp[id], in float
 *   white:      disp[id] = 0 where x[id] == 255
 * The reference's remove_occluded reads neighbours that other threads are zeroing.  mc_remove_occluded tests every pixel
 * against the row as it was on entry (a copy in LDS), which is deterministic, and gives the reference's result for
 * maps of multiples of 1/256 in [0, 2^16) (PNG16 ground truth): DESIGN.md section 13 has the argument.  No claim is made for
 * arbitrary floats.  n == 0 launches nothing.
 * Refused: null pointers; n < 0; W < 1; n no multiple of W; for mc_remove_occluded W > MC_OPS_MAX_W. */
int mc_remove_nonvisible(float *disp, int64_t n, int W, void *stream);
int mc_remove_occluded(float *disp, int64_t n, int W, void *stream);
int mc_remove_white(const float *x, float *disp, int64_t n, void *stream);

/* make_dataset2 (adcensus.cu:1900-1929), a HOST function on host pointers: appends a row (img, row, col, d), 0-based row and
 * col, to nnz (nnz_rows x 4) from row t on for every d = disp[row * W + col] > 0.5 of the H x W map, row-major, and stores the
 * new t in *t_out.
 * Where the list does not fit the reference writes past nnz (its assert is compiled out by -DNDEBUG); here that is refused
 * before anything is written.
 * Refused: null pointers; H, W < 1; t < 0 or nnz_rows < 0; t + (pixels above 0.5) > nnz_rows. */
int mc_make_dataset2(const float *disp, int H, int W, float *nnz, int64_t nnz_rows, int img, int64_t t, int64_t *t_out);

/* subset_dataset (adcensus.cu:1863-1898), a HOST function on host pointers: copies to output, in order, the rows of input
 * (n_rows x 4) whose image number (int)input[j * 4] is one of index[0 .. n_index), and stores their count in *n_out.  output
 * holds n_rows rows.
 * An index outside 0 .. MC_OPS_SUBSET_IMAGES - 1 makes the reference write outside its table of 200 flags (its assert is
 * compiled out, and tests only the upper side); here it is refused before anything is written.  A row whose image number
 * lies outside that range, where the reference reads outside the table, is in no subset.
 * Refused: null pointers (index may be null where n_index == 0, input and output where n_rows == 0); n_index, n_rows < 0;
 * an index outside 0 .. 199. */
int mc_subset_dataset(const int64_t *index, int64_t n_index, const float *input, int64_t n_rows, float *output, int64_t *n_out);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
