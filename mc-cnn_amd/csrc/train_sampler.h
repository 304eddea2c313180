// The patch sampler of the training libraries (libmctrain.so, libmctrainslow.so, libmctrainmb.so, libmctrainmbslow.so): one device function,
// so that all draw the same patches bit for bit.  The patch size PS is a template parameter: 9 for the KITTI nets (WS), 11 for
// Middlebury's two five-layer nets.
#pragma once
#include "mc_common.h"
#include "../../include/mc_train.h"

namespace mc {

constexpr int WS = MC_TRAIN_WS;

// ---- patch sampler: make_patch (main.lua:603-619) + OpenCV 2.4 cvWarpAffine, INTER_CUBIC, constant 0 border ----------
struct Affine { double m[6]; };

// mul32 (main.lua:603-605), in doubles like Lua
__device__ inline Affine mul32(const double a[6], const Affine &b)
{
	Affine r;
	r.m[0] = a[0] * b.m[0] + a[1] * b.m[3];
	r.m[1] = a[0] * b.m[1] + a[1] * b.m[4];
	r.m[2] = a[0] * b.m[2] + a[1] * b.m[5] + a[2];
	r.m[3] = a[3] * b.m[0] + a[4] * b.m[3];
	r.m[4] = a[3] * b.m[1] + a[4] * b.m[4];
	r.m[5] = a[3] * b.m[2] + a[4] * b.m[5] + a[5];
	return r;
}

// interpolateCubic (OpenCV imgproc), A = -0.75, in float
__device__ inline void cubic_coeffs(float x, float c[4])
{
	const float A = -0.75f;
	c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
	c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
	c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
	c[3] = 1.f - c[0] - c[1] - c[2];
}

// One output pixel (dx, dy) of a PS x PS patch of image `src` (H x W) warped by make_patch's matrix for
// (row, col, scale, phi, trans, hshear), then * contrast + brightness.
template <int PS>
__device__ float sample_pixel(const float *__restrict__ src, int H, int W, double row, double col, const float *p, int dx, int dy)
{
	// p: scale_x scale_y phi trans_x trans_y hshear brightness contrast
	Affine m = {{1.0, 0.0, -col, 0.0, 1.0, -row}};
	{ const double t[6] = {1, 0, (double)p[3], 0, 1, (double)p[4]}; m = mul32(t, m); }
	{ const double t[6] = {(double)p[0], 0, 0, 0, (double)p[1], 0}; m = mul32(t, m); }
	{
		const double c = cos((double)p[2]), s = sin((double)p[2]);
		const double t[6] = {c, s, 0, -s, c, 0};
		m = mul32(t, m);
	}
	{ const double t[6] = {1, (double)p[5], 0, 0, 1, 0}; m = mul32(t, m); }
	{ const double t[6] = {1, 0, (PS - 1) / 2.0, 0, 1, (PS - 1) / 2.0}; m = mul32(t, m); }
	double M[6];
	for (int i = 0; i < 6; ++i) M[i] = (double)(float)m.m[i];   // torch.FloatTensor(m), then OpenCV's convertTo(CV_64F)
	// warpAffine without WARP_INVERSE_MAP inverts the matrix
	double D = M[0] * M[4] - M[1] * M[3];
	D = D != 0 ? 1. / D : 0.;
	const double A11 = M[4] * D, A22 = M[0] * D;
	M[0] = A11; M[1] *= -D; M[3] *= -D; M[4] = A22;
	const double b1 = -M[0] * M[2] - M[1] * M[5];
	const double b2 = -M[3] * M[2] - M[4] * M[5];
	M[2] = b1; M[5] = b2;
	// fixed point: AB_BITS = 10, INTER_BITS = 5, round_delta = 16
	const int adelta = (int)rint(M[0] * dx * 1024.0), bdelta = (int)rint(M[3] * dx * 1024.0);
	const int X0 = (int)rint((M[1] * dy + M[2]) * 1024.0) + 16;
	const int Y0 = (int)rint((M[4] * dy + M[5]) * 1024.0) + 16;
	const int X = (X0 + adelta) >> 5, Y = (Y0 + bdelta) >> 5;
	const int sx = (X >> 5) - 1, sy = (Y >> 5) - 1;
	float wx[4], wy[4];
	cubic_coeffs((float)(X & 31) * (1.f / 32), wx);
	cubic_coeffs((float)(Y & 31) * (1.f / 32), wy);
	float sum = 0.f;
	if ((unsigned)sx < (unsigned)(W - 3) && (unsigned)sy < (unsigned)(H - 3)) {
		const float *S = src + (int64_t)sy * W + sx;
		for (int i = 0; i < 4; ++i, S += W) {
			const float r = S[0] * (wy[i] * wx[0]) + S[1] * (wy[i] * wx[1]) + S[2] * (wy[i] * wx[2]) + S[3] * (wy[i] * wx[3]);
			sum = i == 0 ? r : sum + r;
		}
	} else if (sx >= W || sx + 4 <= 0 || sy >= H || sy + 4 <= 0) {
		sum = 0.f;
	} else {
		for (int i = 0; i < 4; ++i) {
			const int yi = sy + i;
			if (yi < 0 || yi >= H) continue;
			for (int j = 0; j < 4; ++j) {
				const int xj = sx + j;
				if (xj >= 0 && xj < W) sum += src[(int64_t)yi * W + xj] * (wy[i] * wx[j]);
			}
		}
	}
	return sum * p[7] + p[6];   // dst:mul(contrast):add(brightness)
}

// Pixel t (0 .. 3*PS*PS-1) of pair `pair`'s three patches.  Rows outside nnz or images outside x0 read 0: the warp's result is
// 0, then * contrast + brightness like any patch that lies outside its image.
template <int PS>
__device__ float sample_pair_pixel(const float *__restrict__ x0, const float *__restrict__ x1, int n_img, int H, int W,
                                   const float *__restrict__ nnz, int64_t n_nnz, int row, const float *__restrict__ prm, int t)
{
	const int patch = t / (PS * PS), pix = t - patch * PS * PS;
	float p[8];
	for (int k = 0; k < 8; ++k) p[k] = prm[(patch == 0 ? 2 : 10) + k];
	if (row < 0 || row >= n_nnz) return 0.f * p[7] + p[6];
	const float *z = nnz + (int64_t)row * 4;
	const int img = (int)z[0];
	if (img < 1 || img > n_img) return 0.f * p[7] + p[6];
	const double dim3 = z[1], dim4 = z[2], d = z[3];
	const double col = patch == 0 ? dim4 : dim4 - d + (double)prm[patch == 1 ? 0 : 1];
	const float *src = (patch == 0 ? x0 : x1) + (int64_t)(img - 1) * H * W;
	return sample_pixel<PS>(src, H, W, dim3, col, p, pix % PS, pix / PS);
}

}  // namespace mc
