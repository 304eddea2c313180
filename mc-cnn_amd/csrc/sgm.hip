// Semiglobal matching for gfx950: one scan LINE per wave64, lanes across the
// disparity axis (VPL consecutive d per lane), the whole line walked inside one
// launch with the previous step's L_r held in VGPRs.
//
// Replaces adcensus.sgm2 (adcensus.cu:620-697; kernels sgm2<0..3>, 535-618),
// which launches one grid per scan STEP (2W+2H launches per call) and keeps
// L_r in a global `tmp` array.  Here a call is 1 prep launch + 4 direction
// sweeps; the recurrence itself (min / + / - only) is evaluated with the same
// operations, so results are bit-identical.
//
// Data layout: (H,W,D) with D contiguous and a pixel stride `ds` (>= D).  A
// wave reads one pixel's D costs as one coalesced run (VPL=4 -> dwordx4 per
// lane, 1 KiB per wave-load at D=256) for every direction.
//
// The intensity tests D1/D2 < tau_so (adcensus.cu:586-605) only select one of
// three penalty pairs, so they are precomputed by sgm_prep_kernel as 2-bit
// classes: cls0[r][y][x] for the reference pixel (wave-uniform) and, for the
// partner pixel x + d*direction, "window" bytes win[o][r][y][s] that pack the
// classes of 4 consecutive pixels s..s+3 (ascending for direction +1,
// descending for -1) so that a lane fetches the classes of its VPL
// disparities with VPL/4 byte loads.
#include "sgm_line.h"

#include <atomic>

namespace mc {

__device__ __forceinline__ int cls_of(float v, float tau) { return v < tau ? 0 : (v > tau ? 2 : 1); }

// r: 0 right (dx=1), 1 left (dx=-1), 2 down (dy=1), 3 up (dy=-1)  (adcensus.cu:541-565)
// The pad of the window rows arrives as Wm = W + 2 * pad (sgm_padw: SGM_PADW for D <= 512, SGM_PADW_WIDE above).
__global__ void __launch_bounds__(256) sgm_prep_kernel(const float *__restrict__ x0, const float *__restrict__ x1,
                                                       uint8_t *__restrict__ cls0, uint8_t *__restrict__ win,
                                                       int H, int W, int Wm, int64_t cls_plane, float tau_so)
{
	const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const int64_t total = (int64_t)4 * H * Wm;
	if (id >= total) return;
	const int i = (int)(id % Wm);
	const int y = (int)((id / Wm) % H);
	const int r = (int)(id / ((int64_t)Wm * H));
	const int dx = r == 0 ? 1 : (r == 1 ? -1 : 0);
	const int dy = r == 2 ? 1 : (r == 3 ? -1 : 0);
	const bool yok = (y - dy >= 0) && (y - dy < H);

	if (i < W) {
		const int x = i;
		int c = 1;
		if (yok && x - dx >= 0 && x - dx < W) {
			// D1 = COLOR_DIFF(x0, ind2, ind2 - dy*size2 - dx), adcensus.cu:587
			c = cls_of(fabsf(x0[y * W + x] - x0[(y - dy) * W + x - dx]), tau_so);
		}
		cls0[(int64_t)r * cls_plane + (int64_t)y * W + x] = (uint8_t)c;
	}
	const int s = i - ((Wm - W) >> 1);
	unsigned asc = 0, desc = 0;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const int xx = s + k;
		float D2 = 10.0f;  // adcensus.cu:590-591
		if (yok && xx >= 0 && xx < W && xx - dx >= 0 && xx - dx < W) {
			D2 = fabsf(x1[y * W + xx] - x1[(y - dy) * W + xx - dx]);  // adcensus.cu:593
		}
		const unsigned c = (unsigned)cls_of(D2, tau_so);
		asc |= c << (2 * k);
		desc |= c << (2 * (3 - k));
	}
	win[((int64_t)(0 * 4 + r) * H + y) * Wm + i] = (uint8_t)asc;
	win[((int64_t)(1 * 4 + r) * H + y) * Wm + i] = (uint8_t)desc;
}

// ---------------------------------------------------------------------------

// mc_sgm2's contract on a caller's volume (debug aid): NaNs form a tail in d and d = 0 is finite
__global__ void __launch_bounds__(256) sgm_contract_kernel(const float *__restrict__ vol, int64_t pixels, int D, unsigned *__restrict__ count)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	bool bad = false;
	if (p < pixels) {
		const float *v = vol + p * D;
		bad = !(fabsf(v[0]) < __builtin_inff());
		bool seen_nan = false;
		for (int d = 0; d < D; ++d) {
			const bool isn = v[d] != v[d];
			bad = bad || (seen_nan && !isn);
			seen_nan = seen_nan || isn;
		}
	}
	const unsigned long long b = __ballot(bad);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned)__builtin_popcountll(b));
}

int sgm_contract_violations(const float *vol, int H, int W, int D, unsigned *count, hipStream_t st)
{
	const int64_t pixels = (int64_t)H * W;
	hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned), st);
	if (e != hipSuccess) {
		set_error("mc_sgm2_contract_violations: hipMemsetAsync: %s", hipGetErrorString(e));
		return (int)e;
	}
	hipLaunchKernelGGL(sgm_contract_kernel, dim3(cdiv(pixels, 256)), dim3(256), 0, st, vol, pixels, D, count);
	return check_launch("sgm_contract");
}

// the maps sgm_prep writes and the sweeps read: cls0[4][plane] then win[2][4][H][Wm] (see SgmPassArgs); cls0 / win = byte offsets.
// The window rows' pad follows D (sgm_padw): every D <= 512 has the layout and the size it always had.
struct SgmMaps { int Wm; size_t plane, cls0, win, bytes; };
static SgmMaps sgm_maps(int H, int W, int D)
{
	const int Wm = W + 2 * sgm_padw(D);
	const size_t plane = ((size_t)H * W + 3 + 4) / 4 * 4;  // dword-aligned class planes (+4: the dword read may straddle)
	return {Wm, plane, 0, 4 * plane, (4 * plane + (size_t)8 * H * Wm + 255) & ~(size_t)255};
}

size_t sgm_maps_bytes(int H, int W) { return sgm_maps(H, W, 1).bytes; }
size_t sgm_maps_bytes_d(int H, int W, int D) { return sgm_maps(H, W, D).bytes; }

int sgm_prep(const float *x0, const float *x1, void *maps, int H, int W, float tau_so, hipStream_t st)
{
	return sgm_prep_d(x0, x1, maps, H, W, 1, tau_so, st);
}

int sgm_prep_d(const float *x0, const float *x1, void *maps, int H, int W, int D, float tau_so, hipStream_t st)
{
	const SgmMaps m = sgm_maps(H, W, D);
	const int64_t total = (int64_t)4 * H * m.Wm;
	hipLaunchKernelGGL(sgm_prep_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, x0, x1, (uint8_t *)maps + m.cls0, (uint8_t *)maps + m.win, H, W,
	                   m.Wm, (int64_t)m.plane, tau_so);
	return check_launch("sgm_prep");
}

// steps kept in flight per wave and sweep (see launch_pass)
constexpr int SGM_U_H = 8, SGM_U_UP = 16;
constexpr int SGM_U_DOWN = 16;   // (A/B on one box: profiles/r05_ab_sgm_depth_per_launch.txt -- 16 steps in flight cost 236 VGPRs, i.e. two waves per SIMD)

template <int DIRN, int MODE, bool ARGMIN, bool DUAL>
static void launch_pass(const SgmPassArgs &A, bool vec, hipStream_t st)
{
	const int nlines = DIRN <= 1 ? A.H : A.W;
	const int waves = A.nvol * nlines * (DUAL ? 2 : 1);
	const dim3 grid(cdiv(waves, 4)), block(256);
	// fewer waves than SIMDs (1024): nothing but prefetch depth hides HBM latency
	// measured on MI355X, A/B on one box (round 4): the depth matters little once >= 4 -- KITTI 370x1226x228 all four
	// sweeps 2.016 ms at (horizontal 4, up 4), 2.024 at (8, 4), 2.009 at (4, 8), 1.982 at (8, 16), 2.008 at (16, 8), the down
	// sweep (three loads per step) at 16 throughout; 1500x1000x256 within 1 % either way.  The sweeps run at what the
	// memory system gives long-lived waves that each walk their own line (4.3-5.1 TB/s), not at a latency bound.
	const int U = DIRN == 2 ? SGM_U_DOWN : (DIRN == 3 ? SGM_U_UP : SGM_U_H);
	// MODE 1 (mc_sgm2, the caller's volumes) has the per-element instances for an unaligned volume or a pixel stride that is not a
	// multiple of 4; the fused modes run on mc_predict's workspace only (ds = Dp, 256-byte aligned slices: sgm_sweeps requires vec)
	constexpr bool SCALAR = MODE == 1;
#define MC_SGM_GO(VPL_, VEC_, U_) \
	hipLaunchKernelGGL((sgm_pass_kernel<DIRN, VPL_, MODE, ARGMIN, VEC_, U_, DUAL, false>), grid, block, 0, st, A)
#define MC_SGM_GO_FAR(VPL_, VEC_, U_) \
	hipLaunchKernelGGL((sgm_pass_kernel<DIRN, VPL_, MODE, ARGMIN, VEC_, U_, DUAL, true>), grid, block, 0, st, A)
	// a volume of 2 GiB or more: 64-bit pixel addresses in every step (one prefetch depth only)
	const bool far = sgm_far(A.H, A.W, A.ds);
	if (A.D > 512) {
		// the walk at 16 values per lane, all its forms (per element, vector, each with and without FAR), lives in this kernel and picks its form
		// itself (sgm_line_wide); (fused modes: sgm_sweeps has required vec)
		MC_SGM_GO(8, true, 8);
	} else if (!vec) {
		if constexpr (SCALAR) {
			if (far) { if (A.D <= 256) MC_SGM_GO_FAR(4, false, 4); else MC_SGM_GO_FAR(8, false, 2); }
			else { if (A.D <= 256) MC_SGM_GO(4, false, 4); else MC_SGM_GO(8, false, 2); }
		}
	} else if (far) {
		if (A.D <= 256) MC_SGM_GO_FAR(4, true, 4); else MC_SGM_GO_FAR(8, true, 4);
	} else if (A.D <= 256) {
		if (U == 16) MC_SGM_GO(4, true, 16); else if (U == 8) MC_SGM_GO(4, true, 8); else MC_SGM_GO(4, true, 4);
	} else {
		if (U >= 8) MC_SGM_GO(8, true, 8); else MC_SGM_GO(8, true, 4);
	}
#undef MC_SGM_GO_FAR
#undef MC_SGM_GO
}


// which vertical launches the fused schedule takes where both forms apply: 1 the down and the up sweep (MODE 3, MODE 2), 2 (the default) the
// checkpoint launch and the recomputing walk.  A handle for A/B measurements and for the tests (mc_test_sgm_vertical), which hold one form
// against the other out of one library.
int sgm_vertical(int set)
{
	static std::atomic<int> forced{0};
	if (set >= 0 && set <= 2) forced.store(set);
	const int f = forced.load();
	return f ? f : 2;
}

// Four direction sweeps over nvol (1 or 2) volumes.
//   fused = false: every sweep does out += L_r (adcensus.sgm2 contract, out pre-zeroed by caller)
//   fused = true : right and left sweeps run concurrently (out = 0 + L_0, out2 = L_1), the down sweep
//                  writes (out + out2) + L_2 to out, the up sweep writes (out + L_3)/4 and, if disp[] is
//                  set, the argmin of the finished pixel.  `out2` is scratch of the same size as out (required),
//                  ds % 4 == 0 and every volume 16-byte aligned (required: mc_predict's workspace).
//                  Bit v of drop_final (fused only): the up sweep does not store volume v's final costs -- out[v] is
//                  left as the down sweep wrote it, the arg-min disp[v] is written as before.
//                  tri (fused only) is the caller's promise that, for every volume v, C[v] is NaN at every (pixel, d) with
//                  d >= Dv, Dv = min(D, x + 1) for direction[v] < 0 and min(D, W - x) for direction[v] > 0 (the voxels whose
//                  partner pixel lies outside the image).  No launch then loads those voxels of C, out or out2 (whole 16-byte pieces
//                  at or beyond Dv; a piece that straddles Dv moves whole).  The horizontal launch writes NaN there into out, as
//                  without the promise; it does not store them into out2, nor into the out of a volume in drop_final.  The two
//                  vertical launches, which work in place on out, neither read nor write them.  So out and disp hold what they
//                  hold without the promise, except: the padding d in [D, ds) of a trimmed column (the horizontal launch's values,
//                  NaN where the piece was not loaded), out2's triangle and the triangle in the out of a volume in drop_final
//                  (both keep what the buffers held before the call).  All three are unspecified and read by nothing.
//                  With checkpoint slots (ck, launchers.h), D <= 256 and no volume of 2 GiB the two vertical launches are the recomputing pair
//                  (sgm_updown_line): a down sweep on C alone that keeps L_down at every SGM_CK_ROWS-th row, in ck[v], and
//                  one walk that runs both vertical recurrences and writes what the up sweep writes -- except that the out of a volume in
//                  drop_final is then left as the horizontal launch wrote it.  Every other shape keeps the down and the up sweep.
int sgm_sweeps(const float *const C[2], float *const out[2], float *const out2[2], float *const disp[2],
               const int direction[2], int nvol, int H, int W, int D, int ds, const void *maps, float pi1, float pi2,
               float alpha1, float q1, float q2, bool fused, unsigned drop_final, bool tri, hipStream_t st)
{
	return sgm_sweeps_ck(C, out, out2, disp, direction, nvol, H, W, D, ds, maps, pi1, pi2, alpha1, q1, q2, fused, drop_final, tri, nullptr, st);
}

int sgm_sweeps_ck(const float *const C[2], float *const out[2], float *const out2[2], float *const disp[2],
                  const int direction[2], int nvol, int H, int W, int D, int ds, const void *maps, float pi1, float pi2,
                  float alpha1, float q1, float q2, bool fused, unsigned drop_final, bool tri, float *const ck[2], hipStream_t st)
{
	// 32-bit pixel indices and line strides in the sweeps (a volume may still exceed 4 GiB: the FAR instances)
	MC_REQUIRE((int64_t)H * W < ((int64_t)1 << 29) && (int64_t)W * ds * 4 < ((int64_t)1 << 31), "sgm: image %dx%d (pixel stride %d) exceeds the sweeps' 32-bit line arithmetic", H, W, ds);
	SgmPassArgs A;
	for (int v = 0; v < 2; ++v) {
		const int k = v < nvol ? v : 0;
		A.C[v] = C[k];
		A.accin[v] = out[k];
		A.accin2[v] = out2 ? out2[k] : nullptr;
		A.out[v] = out[k];
		A.out2[v] = out2 ? out2[k] : nullptr;
		A.disp[v] = disp ? disp[k] : nullptr;
		A.direction[v] = direction[k];
		A.drop_out[v] = 0;
		// (drop_final arrives with the last iteration only: an earlier iteration's out keeps its NaNs, the next one's promise about its input)
		A.drop_h[v] = (fused && tri && v < nvol && ((drop_final >> v) & 1)) ? 1 : 0;
		A.ck[v] = ck ? ck[k] : nullptr;
	}
	A.nvol = nvol;
	A.tri = (fused && tri) ? 1 : 0;
	A.H = H; A.W = W; A.D = D; A.ds = ds;
	const SgmMaps m = sgm_maps(H, W, D);   // (the caller's maps are sgm_prep_d's for this D)
	A.Wm = m.Wm;
	A.cls0 = (const uint8_t *)maps + m.cls0;
	A.cls_plane = (int64_t)m.plane;
	A.win = (const uint8_t *)maps + m.win;
	// adcensus.cu:595-605 -- float divisions exactly as written there
	A.P1[0] = pi1; A.P2[0] = pi2;
	A.P1[1] = pi1 / q1; A.P2[1] = pi2 / q1;
	A.P1[2] = pi1 / (q1 * q2); A.P2[2] = pi2 / (q1 * q2);
	for (int k = 0; k < 3; ++k) A.P1a[k] = A.P1[k] / alpha1;  // adcensus.cu:609,612

	const bool vec = sgm_vec(A);
	const bool am = fused && disp && disp[0];
	if (!fused) {
		launch_pass<0, 1, false, false>(A, vec, st);
		launch_pass<1, 1, false, false>(A, vec, st);
		launch_pass<2, 1, false, false>(A, vec, st);
		launch_pass<3, 1, false, false>(A, vec, st);
	} else {
		// mc_predict: scratch for the concurrent second direction, and its own aligned (H,W,Dp) volumes
		MC_REQUIRE(out2 && vec, "sgm: the fused sweeps need the second direction's scratch and 16-byte aligned volumes with ds %% 4 == 0");
		launch_pass<0, 0, false, true>(A, vec, st);
		if (const int rc = check_launch("sgm_pass horizontal")) return rc;
		const bool far = sgm_far(H, W, ds);
		bool slots = ck != nullptr;
		for (int v = 0; v < nvol && slots; ++v) slots = ck[v] && (uintptr_t)ck[v] % 16 == 0;
		if (slots && D <= 256 && !far && sgm_vertical() == 2) {
			// (the two kernels are libmcsgmrecompute.so's, sgm_recompute.hip: this library's kernel set stays as it is)
			MC_REQUIRE(mc_sgm_recompute_launch(&A, sizeof A, 0, st) == 0, "sgm: the checkpoint launch was refused");
			if (const int rc = check_launch("sgm_pass down checkpoints")) return rc;
			for (int v = 0; v < nvol; ++v) A.drop_out[v] = (drop_final >> v) & 1;
			MC_REQUIRE(mc_sgm_recompute_launch(&A, sizeof A, am ? 2 : 1, st) == 0, "sgm: the recomputing launch was refused");
			return check_launch("sgm_pass up, down recomputed");
		}
		launch_pass<2, 3, false, false>(A, vec, st);
		if (const int rc = check_launch("sgm_pass down")) return rc;
		for (int v = 0; v < nvol; ++v) A.drop_out[v] = (drop_final >> v) & 1;
		if (am) launch_pass<3, 2, true, false>(A, vec, st);
		else launch_pass<3, 2, false, false>(A, vec, st);
		return check_launch("sgm_pass up");
	}
	return check_launch("sgm_pass");
}

}  // namespace mc
