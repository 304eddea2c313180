// KITTI dataset preparation (preprocess_kitti.lua:97-113) on gfx950: the ground-truth filters remove_nonvisible,
// remove_occluded and remove_white (adcensus.cu:1723-1800) and make_dataset2's pixel list (adcensus.cu:1900-1929).
// Part of libmctrain.so (include/mc_train.h).
//
// The filters run as ONE kernel, one workgroup per row of a map.  The reference's remove_occluded zeroes pixels while
// other threads of the row still read them; a zeroed neighbour j gives i - 0 < -d[col], which never holds for d >= 0,
// and the neighbour with the smallest j - d[j] is never zeroed itself, so for non-negative maps with exact arithmetic
// (PNG16 ground truth: multiples of 1/256 below 256) its result equals evaluating every pixel against the row as
// remove_nonvisible left it.  That is what this kernel does: the row goes to LDS once, then each pixel runs the
// reference's loop and float expression on the LDS copy.
//
// The pixel list keeps make_dataset2's order (map, then row-major) without atomics: count the pixels of each row
// (one wave per row, a ballot per 64 columns), an exclusive scan of the row counts in one workgroup, then each row's
// wave writes its rows at its offset, lane order within a ballot.
#include "mc_common.h"
#include "../../include/mc_train.h"

namespace mc {

constexpr int GT_NT = 256;          // threads of a filter workgroup (one row)
constexpr int NNZ_ROWS = 4;         // map rows per count / fill workgroup: one wave each
constexpr int SCAN_NT = 1024;

__global__ __launch_bounds__(GT_NT) void gt_filter_kernel(float *disp, const float *x0, int W)
{
	extern __shared__ float row[];
	const int64_t base = (int64_t)blockIdx.x * W;
	for (int c = threadIdx.x; c < W; c += GT_NT) {
		const float d = disp[base + c];
		row[c] = d >= (float)c ? 0.f : d;                 // remove_nonvisible: y[id] >= x
	}
	__syncthreads();
	for (int c = threadIdx.x; c < W; c += GT_NT) {
		float d = row[c];
		for (int i = 1; c + i < W; i++) {                // remove_occluded
			if ((float)i - row[c + i] < -row[c]) {
				d = 0.f;
				break;
			}
		}
		if (x0[base + c] == 255.f) d = 0.f;              // remove_white
		disp[base + c] = d;
	}
}

__global__ __launch_bounds__(64 * NNZ_ROWS) void nnz_count_kernel(const float *disp, int64_t n_rows, int W, int32_t *counts)
{
	const int64_t r = (int64_t)blockIdx.x * NNZ_ROWS + (threadIdx.x >> 6);
	if (r >= n_rows) return;
	const int lane = threadIdx.x & 63;
	const float *src = disp + r * W;
	int cnt = 0;
	for (int c0 = 0; c0 < W; c0 += 64) {
		const int c = c0 + lane;
		cnt += __popcll(__ballot(c < W && src[c] > 0.5f));   // disp[i * width + j] > 0.5
	}
	if (lane == 0) counts[r] = cnt;
}

// offsets[r] = counts[0] + ... + counts[r - 1] for r <= n_rows; *total = offsets[n_rows].  Each thread sums a contiguous
// chunk, the chunk sums are scanned in LDS, then each thread writes its chunk's offsets.
__global__ __launch_bounds__(SCAN_NT) void nnz_scan_kernel(const int32_t *counts, int64_t n_rows, int64_t *offsets, int64_t *total)
{
	__shared__ int64_t part[SCAN_NT];
	const int t = threadIdx.x;
	const int64_t per = (n_rows + SCAN_NT - 1) / SCAN_NT;
	const int64_t lo = min(n_rows, t * per), hi = min(n_rows, lo + per);
	int64_t s = 0;
	for (int64_t r = lo; r < hi; ++r) s += counts[r];
	part[t] = s;
	__syncthreads();
	for (int k = 1; k < SCAN_NT; k <<= 1) {             // inclusive Hillis-Steele scan
		const int64_t v = t >= k ? part[t - k] : 0;
		__syncthreads();
		part[t] += v;
		__syncthreads();
	}
	int64_t run = t ? part[t - 1] : 0;
	for (int64_t r = lo; r < hi; ++r) {
		offsets[r] = run;
		run += counts[r];
	}
	if (t == SCAN_NT - 1) {
		offsets[n_rows] = part[t];
		*total = part[t];
	}
}

__global__ __launch_bounds__(64 * NNZ_ROWS) void nnz_fill_kernel(const float *disp, const int32_t *ids, int H, int W, int64_t n_rows,
                                                                 const int64_t *offsets, float *nnz, int64_t n_nnz)
{
	const int64_t r = (int64_t)blockIdx.x * NNZ_ROWS + (threadIdx.x >> 6);
	if (r >= n_rows) return;
	const int lane = threadIdx.x & 63;
	const float *src = disp + r * W;
	const float img = (float)ids[r / H];
	const float y = (float)(r % H);
	const uint64_t below = (1ull << lane) - 1;
	int64_t o = offsets[r];
	for (int c0 = 0; c0 < W; c0 += 64) {
		const int c = c0 + lane;
		const float d = c < W ? src[c] : 0.f;
		const bool keep = c < W && d > 0.5f;
		const uint64_t m = __ballot(keep);
		const int64_t k = o + __popcll(m & below);
		if (keep && k < n_nnz)
			*reinterpret_cast<float4 *>(nnz + 4 * k) = make_float4(img, y, (float)c, d);
		o += __popcll(m);
	}
}

static int64_t n_rows_of(int n, int H) { return (int64_t)n * H; }

static size_t counts_bytes(int64_t n_rows) { return ((size_t)n_rows * sizeof(int32_t) + 15) & ~(size_t)15; }

static int check_maps(const float *disp, int n, int H, int W, const char *what)
{
	MC_REQUIRE(n >= 0 && H >= 1 && W >= 1, "%s: bad map dims %d x %d x %d", what, n, H, W);
	MC_REQUIRE(n_rows_of(n, H) < ((int64_t)1 << 31) && n_rows_of(n, H) * W < ((int64_t)1 << 40), "%s: %d maps of %d x %d are too many",
	           what, n, H, W);
	MC_REQUIRE(disp || n == 0, "%s: null map pointer", what);
	return 0;
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_train_filter_gt(float *disp, const float *x0, int n, int H, int W, void *stream)
{
	if (int rc = check_maps(disp, n, H, W, "filter_gt")) return rc;
	MC_REQUIRE(W <= MC_TRAIN_GT_MAX_W, "filter_gt: width %d exceeds %d", W, MC_TRAIN_GT_MAX_W);
	MC_REQUIRE(x0 || n == 0, "filter_gt: null image pointer");
	if (n == 0) return 0;
	gt_filter_kernel<<<(unsigned)n_rows_of(n, H), GT_NT, (size_t)W * sizeof(float), as_stream(stream)>>>(disp, x0, W);
	return check_launch("filter_gt");
}

size_t mc_train_nnz_workspace_bytes(int n, int H)
{
	if (n < 0 || H < 1 || n_rows_of(n, H) >= ((int64_t)1 << 31)) return 0;
	const int64_t rows = n_rows_of(n, H);
	return counts_bytes(rows) + (size_t)(rows + 1) * sizeof(int64_t);
}

int mc_train_nnz_count(const float *disp, int n, int H, int W, int64_t *count, void *workspace, size_t workspace_bytes, void *stream)
{
	if (int rc = check_maps(disp, n, H, W, "nnz_count")) return rc;
	MC_REQUIRE(count && workspace, "nnz_count: null count / workspace pointer");
	MC_REQUIRE(workspace_bytes >= mc_train_nnz_workspace_bytes(n, H), "nnz_count: workspace of %zu bytes, %zu needed", workspace_bytes,
	           mc_train_nnz_workspace_bytes(n, H));
	const int64_t rows = n_rows_of(n, H);
	int32_t *counts = (int32_t *)workspace;
	int64_t *offsets = (int64_t *)((char *)workspace + counts_bytes(rows));
	const hipStream_t st = as_stream(stream);
	if (rows > 0) {
		nnz_count_kernel<<<cdiv(rows, NNZ_ROWS), 64 * NNZ_ROWS, 0, st>>>(disp, rows, W, counts);
		if (int rc = check_launch("nnz_count")) return rc;
	}
	nnz_scan_kernel<<<1, SCAN_NT, 0, st>>>(counts, rows, offsets, count);
	return check_launch("nnz_scan");
}

int mc_train_nnz_fill(const float *disp, const int32_t *ids, int n, int H, int W, float *nnz, int64_t n_nnz, const void *workspace,
                      size_t workspace_bytes, void *stream)
{
	if (int rc = check_maps(disp, n, H, W, "nnz_fill")) return rc;
	MC_REQUIRE(workspace && (ids || n == 0), "nnz_fill: null ids / workspace pointer");
	MC_REQUIRE(workspace_bytes >= mc_train_nnz_workspace_bytes(n, H), "nnz_fill: workspace of %zu bytes, %zu needed", workspace_bytes,
	           mc_train_nnz_workspace_bytes(n, H));
	MC_REQUIRE(n_nnz >= 0 && (nnz || n_nnz == 0), "nnz_fill: null output for %lld rows", (long long)n_nnz);
	MC_REQUIRE(((uintptr_t)nnz & 15) == 0, "nnz_fill: output not 16-byte aligned");
	const int64_t rows = n_rows_of(n, H);
	if (rows == 0 || n_nnz == 0) return 0;
	const int64_t *offsets = (const int64_t *)((const char *)workspace + counts_bytes(rows));
	nnz_fill_kernel<<<cdiv(rows, NNZ_ROWS), 64 * NNZ_ROWS, 0, as_stream(stream)>>>(disp, ids, H, W, rows, offsets, nnz, n_nnz);
	return check_launch("nnz_fill");
}

}  // extern "C"
