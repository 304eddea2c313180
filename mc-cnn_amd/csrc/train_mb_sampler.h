// A pair's patches from Middlebury's ragged image store (include/mc_train_mb.h: planes, table, src), shared by the two
// Middlebury training libraries (libmctrainmb.so, libmctrainmbslow.so) so that both draw the same patches bit for bit.  The
// warp is train_sampler.h's sample_pixel with the patch size PS as its parameter (11 for both five-layer nets).
#pragma once
#include "../../include/mc_train_mb.h"
#include "train_sampler.h"

namespace mc {

// Pixel t (0 .. 3*PS*PS-1) of a pair's three PS x PS patches: the left one from plane src[0], both right ones from plane src[1], centred
// by nnz row `row`.  A row outside nnz or a plane id outside the table reads 0: the warp's result is 0, then * contrast +
// brightness like any patch that lies outside its image.  A record the sampler could not address (a side below 4 or of
// 32768 and more; the loader refuses them) counts as outside the table.
template <int PS>
__device__ float sample_mb_pixel(const float *__restrict__ planes, const mc_train_mb_plane *__restrict__ table, int n_planes,
                                 const float *__restrict__ nnz, int64_t n_nnz, int row, const int32_t *__restrict__ src,
                                 const float *__restrict__ prm, int t)
{
	const int patch = t / (PS * PS), pix = t - patch * PS * PS;
	float p[8];
	for (int k = 0; k < 8; ++k) p[k] = prm[(patch == 0 ? 2 : 10) + k];
	if (row < 0 || row >= n_nnz) return 0.f * p[7] + p[6];
	const int id = src[patch == 0 ? 0 : 1];
	if (id < 0 || id >= n_planes) return 0.f * p[7] + p[6];
	const mc_train_mb_plane pl = table[id];
	if (pl.H < 4 || pl.W < 4 || pl.H >= 32768 || pl.W >= 32768) return 0.f * p[7] + p[6];
	const float *z = nnz + (int64_t)row * 4;
	const double dim3 = z[1], dim4 = z[2], d = z[3];
	const double col = patch == 0 ? dim4 : dim4 - d + (double)prm[patch == 1 ? 0 : 1];
	return sample_pixel<PS>(planes + pl.offset, pl.H, pl.W, dim3, col, p, pix % PS, pix / PS);
}

}  // namespace mc
