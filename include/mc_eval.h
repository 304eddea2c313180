/*
 * mc_eval.h -- C ABI of libmceval.so: the error measure of `-a test_te`
 * (main.lua:1224-1236) on the MI355X (gfx950), so that a test set's score
 * needs no per-pair read-back of the disparity map.
 *
 * Conventions are those of mc_adcensus.h: device pointers to fp32 (int32 for
 * the counts), explicit dims, `stream` a hipStream_t (NULL = default),
 * asynchronous, never synchronising, never allocating, return 0 / hipError_t /
 * MC_EINVAL with a thread-local message in mc_eval_last_error().  Every
 * argument check runs on the host before the launch and writes nothing.
 */
#ifndef MC_EVAL_H
#define MC_EVAL_H

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_EVAL_ABI_VERSION 1
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif

int mc_eval_version(void);
const char *mc_eval_last_error(void);

/* The three counts of main.lua:1224-1236 over an H x W map, per pixel in fp32:
 *   counts[0] += pixels with actual != 0                      (mask)
 *   counts[1] += of those, pixels with |actual - pred| > err_at
 *   counts[2] += pixels with pred != pred                     (the reference asserts there is none)
 * pred_ld / actual_ld are the row strides in floats (>= W): KITTI's ground
 * truth is stored 1242 wide and read W wide.  A denormal `actual` is non-zero,
 * -0.0f is zero, a NaN difference is not bad: what numpy gives on float32.
 * The counts are ADDED to (one integer atomicAdd per workgroup and counter), so
 * the caller zeroes them; they are exact and independent of scheduling.
 * Refused: H, W < 1; a stride < W; H * W >= 2^31; null pointers. */
int mc_eval_error(const float *pred, int pred_ld, const float *actual, int actual_ld,
                  int H, int W, float err_at, int *counts /* [3] */, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
