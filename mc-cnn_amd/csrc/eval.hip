// libmceval.so (include/mc_eval.h): the error measure of -a test_te (main.lua:1224-1236) in one pass over the predicted map and the
// ground truth.  A workgroup takes EV_COLS columns of one row: 16-byte loads over the part of the row where both maps are 16-byte
// aligned, dword loads for the ragged ends (and for the whole row where the two maps' alignments differ, which a stride != W brings
// about); every predicate is counted per wave by ballot + popcount, so the counters are wave-uniform and no lane ever leaves a loop
// before the others; then one integer atomicAdd per workgroup and counter.
#include "mc_common.h"
#include "../../include/mc_eval.h"

namespace mc {

constexpr int EV_THREADS = 256;
constexpr int EV_VECS = 1024;             // float4s of a row per workgroup: four per thread
constexpr int EV_COLS = 4 * EV_VECS;
constexpr int EV_MAX_ROWS = 65535;        // gridDim.y; further rows by stride

struct EvCounts {
	int valid, bad, nan;
};

// `in`: this lane holds a pixel.  Bit tests instead of float compares: independent of the denormal mode (a denormal is non-zero).
__device__ __forceinline__ void ev_tally(EvCounts &c, bool in, float p, float a, float err_at)
{
	const bool valid = in && (__float_as_uint(a) & 0x7fffffffu) != 0u;          // actual != 0: -0.0f is zero, NaN is not
	const bool bad = valid && fabsf(a - p) > err_at;                             // false for a NaN difference
	const bool nan = in && (__float_as_uint(p) & 0x7fffffffu) > 0x7f800000u;     // pred != pred
	c.valid += __popcll(__ballot(valid));
	c.bad += __popcll(__ballot(bad));
	c.nan += __popcll(__ballot(nan));
}

__global__ void __launch_bounds__(EV_THREADS) eval_error_kernel(const float *__restrict__ pred, int pred_ld, const float *__restrict__ actual,
                                                                int actual_ld, int H, int W, float err_at, int *__restrict__ counts)
{
	__shared__ int part[EV_THREADS / 64][3];
	const int tid = threadIdx.x;
	EvCounts c = {0, 0, 0};
	for (int row = blockIdx.y; row < H; row += gridDim.y) {
		const float *p = pred + (size_t)row * pred_ld;
		const float *a = actual + (size_t)row * actual_ld;
		const unsigned pm = (unsigned)((uintptr_t)p >> 2) & 3u, am = (unsigned)((uintptr_t)a >> 2) & 3u;
		if (pm == am) {   // uniform over the workgroup
			const int head = min((int)((4u - pm) & 3u), W);   // dwords before the first 16-byte boundary
			const int nvec = (W - head) >> 2;
			const int v1 = min(nvec, (int)(blockIdx.x + 1) * EV_VECS);   // (blockIdx.x + 1) * EV_VECS <= W / 4 + EV_VECS: no overflow
			const float4 *p4 = reinterpret_cast<const float4 *>(p + head);
			const float4 *a4 = reinterpret_cast<const float4 *>(a + head);
			for (int vb = blockIdx.x * EV_VECS; vb < v1; vb += EV_THREADS) {
				const int v = vb + tid;
				const bool in = v < v1;
				float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), av = pv;
				if (in) {
					pv = p4[v];
					av = a4[v];
				}
				ev_tally(c, in, pv.x, av.x, err_at);
				ev_tally(c, in, pv.y, av.y, err_at);
				ev_tally(c, in, pv.z, av.z, err_at);
				ev_tally(c, in, pv.w, av.w, err_at);
			}
			// the ragged ends: the row's first workgroup takes the head, its last one the tail (at most 3 dwords each)
			int col = -1;
			if (blockIdx.x == 0 && tid < head) col = tid;
			const int tail0 = head + 4 * nvec;
			if (blockIdx.x == gridDim.x - 1 && tid >= 4 && tid - 4 < W - tail0) col = tail0 + tid - 4;
			const bool in = col >= 0;
			ev_tally(c, in, in ? p[col] : 0.f, in ? a[col] : 0.f, err_at);
		} else {
			const long long c0 = (long long)blockIdx.x * EV_COLS;
			const long long c1 = min((long long)W, c0 + EV_COLS);
			for (long long cb = c0; cb < c1; cb += EV_THREADS) {
				const long long col = cb + tid;
				const bool in = col < c1;
				ev_tally(c, in, in ? p[col] : 0.f, in ? a[col] : 0.f, err_at);
			}
		}
	}
	if ((tid & 63) == 0) {
		part[tid >> 6][0] = c.valid;
		part[tid >> 6][1] = c.bad;
		part[tid >> 6][2] = c.nan;
	}
	__syncthreads();
	if (tid < 3) {
		int s = 0;
		for (int w = 0; w < EV_THREADS / 64; ++w) s += part[w][tid];
		if (s) atomicAdd(counts + tid, s);
	}
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_eval_version(void) { return MC_EVAL_ABI_VERSION; }

const char *mc_eval_last_error(void) { return last_error(); }

int mc_eval_error(const float *pred, int pred_ld, const float *actual, int actual_ld, int H, int W, float err_at, int *counts, void *stream)
{
	MC_REQUIRE(pred && actual && counts, "mc_eval_error: null pointer (pred %p, actual %p, counts %p)", (const void *)pred, (const void *)actual,
	           (void *)counts);
	MC_REQUIRE(H >= 1 && W >= 1, "mc_eval_error: bad dims %d x %d", H, W);
	MC_REQUIRE(pred_ld >= W && actual_ld >= W, "mc_eval_error: a row stride (pred_ld %d, actual_ld %d) is below W = %d", pred_ld, actual_ld, W);
	MC_REQUIRE((int64_t)H * W < ((int64_t)1 << 31), "mc_eval_error: %d x %d is 2^31 pixels or more: the counts are int32", H, W);
	if (pred_ld == W && actual_ld == W) {   // both maps dense: one long row, so that a flat map is spread over the chip
		W *= H;
		H = 1;
		pred_ld = actual_ld = W;
	}
	const dim3 grid(cdiv(W, EV_COLS), (unsigned)(H < EV_MAX_ROWS ? H : EV_MAX_ROWS));
	hipLaunchKernelGGL(eval_error_kernel, grid, dim3(EV_THREADS), 0, as_stream(stream), pred, pred_ld, actual, actual_ld, H, W, err_at, counts);
	return check_launch("mc_eval_error");
}

}  // extern "C"
