/*
 * mc_fc_split.h -- C ABI of libmcfcsplit.so: the accurate architecture's
 * per-disparity FC stack (main.lua:958-983; mc_fc_stack of mc_adcensus.h) with
 * its hidden layers on the bf16 matrix cores of the MI355X (gfx950), each fp32
 * product taken as three bf16 products ("bf16x3", `-fc_mode bf16x3`).
 *
 * Conventions are those of mc_adcensus.h: device pointers to fp32, explicit
 * dims, `stream` a hipStream_t (NULL = default), asynchronous, never
 * synchronising, never allocating, return 0 / hipError_t / MC_EINVAL with a
 * thread-local message in mc_fc_split_last_error().  Every argument check runs
 * on the host before the first launch; a refused call writes nothing.
 *
 * The arithmetic (tests/fc_split_oracle.py restates it):
 *   split(v): hi = bf16(v), round to nearest even; lo = bf16(v - float(hi)).
 *             Inputs are finite.
 *   layer 1:  as mc_fc_stack: the two per-pixel projections W1L L(x), W1R R(x)
 *             on the fp32 MFMA, then h = max((PL[x] + PR[x-d]) + b1, 0) in fp32.
 *   hidden (384 -> 384), with (hhi, hlo) = split(h) per element and
 *             (Whi, Wlo) = split(W) per element, the weights once per call:
 *               z[n] = sum_k (Whi[n,k] hhi[k] + Whi[n,k] hlo[k] + Wlo[n,k] hhi[k])
 *             every product exact (bf16 x bf16 fits fp32), the sum in fp32 in
 *             the matrix cores' order, the lo x lo term dropped;
 *               h' = max(z + b, 0) in fp32, split again for the next layer.
 *   output:   fp32 w; s = 0; s = fmaf(w[k], float(hhi[k]) + float(hlo[k]), s)
 *             for k = 0..383 in order; s += b; 1 / (1 + expf(-s)).  The kernel
 *             keeps activations only as (hhi, hlo), so the output layer always
 *             reads the split of the last h, never its fp32 value (also where
 *             there is no hidden layer).
 *   results:  volL[d,y,x] and volR[d,y,x-d] for x >= d; every other element is
 *             left as the caller filled it (NaN, main.lua:966).
 * Distance from the exact-product evaluation on sigmoid outputs: <= 1.2e-5 on
 * the project's test inputs, 4e-7 at 370 x 1226 x 228;
 * the operator's bar is 1e-4.
 */
#ifndef MC_FC_SPLIT_H
#define MC_FC_SPLIT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_FC_SPLIT_ABI_VERSION 1
#define MC_FC_SPLIT_NH 384     /* hidden width (nh2 of every accurate preset) */
#define MC_FC_SPLIT_VOXELS 96  /* voxels of one (y, d) per workgroup */
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif

int mc_fc_split_version(void);
const char *mc_fc_split_last_error(void);

/* Bytes of workspace mc_fc_split_stack needs (the two projections, layer 1's
 * transposed halves, the hidden layers' bf16 hi / lo planes); a multiple of
 * 256; 0 for C < 1, n_layers outside 2..8, H < 1 or W < 1. */
size_t mc_fc_split_workspace_bytes(int C, int n_layers, int H, int W);

/* The argument list of mc_fc_stack.  featL / featR: (C,H,W); weights[l]:
 * (layer_out[l], in) row-major, layer 0 with 2C inputs; biases[l]:
 * (layer_out[l]); `weights`, `biases`, `layer_out` are host arrays of n_layers
 * entries.  volL / volR: (D,H,W).
 * Refused (message starts "mc_fc_split_stack:"): null pointers; D, H, W, C < 1
 * or D*H*W >= 2^40; n_layers outside 2..8; a hidden width other than 384; a
 * last layer with other than one output; a workspace below
 * mc_fc_split_workspace_bytes or not 16-byte aligned; more than 2^31 - 1
 * workgroups (ceil(H/8) * ceil(W/96) * D * 8). */
int mc_fc_split_stack(const float *featL, const float *featR, int C, int H, int W, int D,
                      const float *const *weights, const float *const *biases, const int *layer_out, int n_layers,
                      float *volL, float *volR, void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
