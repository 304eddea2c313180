/*
 * mc_conv_split.h -- C ABI of libmcconvsplit.so: the feature nets' 3x3
 * convolution (cudnn.SpatialConvolution(Cin, Cout, 3, 3, 1, 1, 1, 1) [+ ReLU],
 * main.lua:681-686, 727-746; mc_conv3x3 of mc_adcensus.h) on the bf16 matrix
 * cores of the MI355X (gfx950), each fp32 product taken as three bf16 products
 * ("bf16x3", `-conv_mode bf16x3`).
 *
 * Conventions are those of mc_adcensus.h: device pointers to fp32, explicit
 * dims, `stream` a hipStream_t (NULL = default), asynchronous, never
 * synchronising, never allocating, return 0 / hipError_t / MC_EINVAL with a
 * thread-local message in mc_conv_split_last_error().  Every argument check
 * runs on the host before the first launch; a refused call writes nothing.
 * The library is re-entrant: concurrent calls from several threads on several
 * streams are independent as long as their outputs and workspaces are.
 *
 * The arithmetic (tests/conv_split_oracle.py restates it):
 *   split(v): hi = bf16(v), round to nearest even; lo = bf16(v - float(hi)).
 *             Inputs are finite.
 *   with (Xhi, Xlo) = split(in) per element and (Whi, Wlo) = split(weight)
 *   per element:
 *     out[n,co,y,x] = act( sum_{ci,ky,kx} ( Whi[co,ci,ky,kx] Xhi[n,ci,y+ky-1,x+kx-1]
 *                                         + Whi[co,ci,ky,kx] Xlo[n,ci,y+ky-1,x+kx-1]
 *                                         + Wlo[co,ci,ky,kx] Xhi[n,ci,y+ky-1,x+kx-1] )
 *                          + bias[co] )
 *   every product exact (bf16 x bf16 fits fp32), the sum in fp32 in the matrix
 *   cores' order starting from 0, the lo x lo term dropped, the bias added to
 *   the finished sum in fp32; act = max(., 0) for relu != 0, identity
 *   otherwise; positions outside the image are zeros (padding 1).
 *   The output is planar fp32 NCHW, like mc_conv3x3's.
 * Distance from a float64 convolution: about 1.2e-5 of the output scale on the
 * project's test inputs (mc_conv3x3: 8e-7); the operator's bar is 1e-4
 * (DESIGN.md section 12).
 *
 * Eligible layers: Cin % 16 == 0, Cin >= 16, 1 <= Cout <= 128 (a k-step of
 * v_mfma_f32_32x32x16_bf16 is 16 input channels of one filter tap).
 */
#ifndef MC_CONV_SPLIT_H
#define MC_CONV_SPLIT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden */

#define MC_CONV_SPLIT_ABI_VERSION 1
#define MC_CONV_SPLIT_CIN_STEP 16   /* Cin is a multiple of this */
#define MC_CONV_SPLIT_MAX_COUT 128
#ifndef MC_EINVAL
#define MC_EINVAL (-22)
#endif

int mc_conv_split_version(void);
const char *mc_conv_split_last_error(void);

/* Bytes of workspace mc_conv_split needs (the weights' bf16 hi / lo planes in
 * the matrix instruction's operand order); a multiple of 256; 0 for a layer
 * that is not eligible. */
size_t mc_conv_split_workspace_bytes(int Cin, int Cout);

/* The argument list of mc_conv3x3.  in: (N,Cin,H,W); weight: (Cout,Cin,3,3);
 * bias: (Cout); out: (N,Cout,H,W).
 * Refused (message starts "mc_conv_split:"): null pointers; out or workspace
 * equal to another argument; N, H, W < 1; a layer that is not eligible (the
 * message names the rule); max(Cout, Cin + 1) * H * W * 4 >= 2^32 - 256 or
 * N * ceil(W/32) * H >= 2^31 (mc_conv3x3's bounds); a workspace below
 * mc_conv_split_workspace_bytes or not 16-byte aligned. */
int mc_conv_split(const float *in, const float *weight, const float *bias, float *out, int N, int Cin, int Cout, int H, int W,
                  int relu, void *workspace, size_t workspace_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
