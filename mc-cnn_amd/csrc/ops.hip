// libmcops.so (include/mc_ops.h): the training and dataset operators of the reference's adcensus.* table that the other libraries
// do not serve -- here Margin2 (adcensus.cu:1379-1453), remove_nonvisible / remove_occluded / remove_white (1723-1796) and the host
// functions subset_dataset / make_dataset2 (1863-1929); Normalize_backward_input is ops_normalize.hip.
//
// Every expression is the reference's, operation for operation, built with -ffp-contract=off; none of these contracts in the
// reference's build either.
//
// remove_occluded: one workgroup per row, the row copied to LDS first, every pixel tested against that copy
// (why this is the reference's result on PNG16 ground truth, and deterministic on anything).
#include "mc_common.h"
#include "../../include/mc_ops.h"

namespace mc {

constexpr int OPS_NT = 256;

template <int POW>
__global__ __launch_bounds__(OPS_NT) void margin2_kernel(const float *__restrict__ in, float *__restrict__ tmp, float *__restrict__ gi,
                                                        float margin, int n)
{
	const int id = blockIdx.x * OPS_NT + threadIdx.x;
	if (id >= n) return;
	const float pos = in[(int64_t)id * 2], neg = in[(int64_t)id * 2 + 1];
	const float f = neg - pos + margin;
	if (POW == 1) {
		tmp[id] = fmaxf(0.f, f);
		gi[(int64_t)id * 2] = (float)(-1. * (f > 0));           // -0.0 for an inactive pair
		gi[(int64_t)id * 2 + 1] = (float)(f > 0);
	} else {
		const float d = fmaxf(0.f, f);
		tmp[id] = (float)(d * d * 0.5);
		gi[(int64_t)id * 2] = -f * (f > 0);                     // -0.0 at f == 0
		gi[(int64_t)id * 2 + 1] = f * (f > 0);
	}
}

__global__ __launch_bounds__(OPS_NT) void remove_nonvisible_kernel(float *disp, int64_t n, int W)
{
	const int64_t stride = (int64_t)gridDim.x * OPS_NT;
	for (int64_t id = (int64_t)blockIdx.x * OPS_NT + threadIdx.x; id < n; id += stride) {
		const int x = (int)(id % W);
		if (disp[id] >= x) disp[id] = 0.f;
	}
}

__global__ __launch_bounds__(OPS_NT) void remove_white_kernel(const float *__restrict__ x, float *__restrict__ disp, int64_t n)
{
	const int64_t stride = (int64_t)gridDim.x * OPS_NT;
	for (int64_t id = (int64_t)blockIdx.x * OPS_NT + threadIdx.x; id < n; id += stride)
		if (x[id] == 255) disp[id] = 0.f;
}

__global__ __launch_bounds__(OPS_NT) void remove_occluded_kernel(float *disp, int64_t n_rows, int W)
{
	extern __shared__ float row[];           // [W]: the row as it was on entry
	for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
		float *y = disp + r * W;
		for (int c = threadIdx.x; c < W; c += OPS_NT) row[c] = y[c];
		__syncthreads();
		for (int c = threadIdx.x; c < W; c += OPS_NT) {
			for (int i = 1; c + i < W; i++) {
				if (i - row[c + i] < -row[c]) {
					y[c] = 0.f;
					break;
				}
			}
		}
		__syncthreads();                     // before the next row overwrites the copy
	}
}

constexpr unsigned OPS_MAX_BLOCKS = 1u << 20;   // elementwise kernels stride over anything longer

static unsigned capped(int64_t blocks) { return (unsigned)(blocks < (int64_t)OPS_MAX_BLOCKS ? blocks : (int64_t)OPS_MAX_BLOCKS); }
static unsigned blocks_for(int64_t n) { return capped((n + OPS_NT - 1) / OPS_NT); }

}  // namespace mc

using namespace mc;

extern "C" {

int mc_ops_version(void) { return MC_OPS_ABI_VERSION; }

const char *mc_ops_last_error(void) { return last_error(); }

int mc_margin2(const float *input, float *tmp, float *grad_input, int n_pairs, float margin, int pow, void *stream)
{
	MC_REQUIRE(input && tmp && grad_input, "mc_margin2: null pointer (input %p, tmp %p, grad_input %p)", (const void *)input, (void *)tmp,
	           (void *)grad_input);
	MC_REQUIRE(n_pairs >= 0, "mc_margin2: n_pairs %d is negative", n_pairs);
	MC_REQUIRE(pow == 1 || pow == 2, "mc_margin2: pow %d is neither 1 nor 2", pow);
	if (n_pairs == 0) return 0;
	const dim3 grid(cdiv(n_pairs, OPS_NT));
	if (pow == 1)
		hipLaunchKernelGGL(margin2_kernel<1>, grid, dim3(OPS_NT), 0, as_stream(stream), input, tmp, grad_input, margin, n_pairs);
	else
		hipLaunchKernelGGL(margin2_kernel<2>, grid, dim3(OPS_NT), 0, as_stream(stream), input, tmp, grad_input, margin, n_pairs);
	return check_launch("mc_margin2");
}

static int check_rows(const char *what, const float *disp, int64_t n, int W)
{
	MC_REQUIRE(disp, "%s: null pointer", what);
	MC_REQUIRE(n >= 0 && W >= 1, "%s: bad size: %lld elements in rows of %d", what, (long long)n, W);
	MC_REQUIRE(n % W == 0, "%s: %lld elements are no whole number of rows of %d", what, (long long)n, W);
	return 0;
}

int mc_remove_nonvisible(float *disp, int64_t n, int W, void *stream)
{
	if (int rc = check_rows("mc_remove_nonvisible", disp, n, W)) return rc;
	if (n == 0) return 0;
	hipLaunchKernelGGL(remove_nonvisible_kernel, dim3(blocks_for(n)), dim3(OPS_NT), 0, as_stream(stream), disp, n, W);
	return check_launch("mc_remove_nonvisible");
}

int mc_remove_occluded(float *disp, int64_t n, int W, void *stream)
{
	if (int rc = check_rows("mc_remove_occluded", disp, n, W)) return rc;
	MC_REQUIRE(W <= MC_OPS_MAX_W, "mc_remove_occluded: width %d exceeds %d", W, MC_OPS_MAX_W);
	if (n == 0) return 0;
	const int64_t n_rows = n / W;
	hipLaunchKernelGGL(remove_occluded_kernel, dim3(capped(n_rows)), dim3(OPS_NT), (size_t)W * sizeof(float),
	                   as_stream(stream), disp, n_rows, W);
	return check_launch("mc_remove_occluded");
}

int mc_remove_white(const float *x, float *disp, int64_t n, void *stream)
{
	MC_REQUIRE(x && disp, "mc_remove_white: null pointer (x %p, disp %p)", (const void *)x, (void *)disp);
	MC_REQUIRE(n >= 0, "mc_remove_white: bad size: %lld elements", (long long)n);
	if (n == 0) return 0;
	hipLaunchKernelGGL(remove_white_kernel, dim3(blocks_for(n)), dim3(OPS_NT), 0, as_stream(stream), x, disp, n);
	return check_launch("mc_remove_white");
}

int mc_make_dataset2(const float *disp, int H, int W, float *nnz, int64_t nnz_rows, int img, int64_t t, int64_t *t_out)
{
	MC_REQUIRE(disp && nnz && t_out, "mc_make_dataset2: null pointer (disp %p, nnz %p, t_out %p)", (const void *)disp, (void *)nnz, (void *)t_out);
	MC_REQUIRE(H >= 1 && W >= 1, "mc_make_dataset2: bad dims %d x %d", H, W);
	MC_REQUIRE(t >= 0 && nnz_rows >= 0, "mc_make_dataset2: bad list: row %lld of %lld", (long long)t, (long long)nnz_rows);
	const int64_t size = (int64_t)H * W;
	int64_t count = 0;
	for (int64_t k = 0; k < size; ++k) count += disp[k] > 0.5;
	MC_REQUIRE(t <= nnz_rows && count <= nnz_rows - t,
	           "mc_make_dataset2: the list does not fit: %lld pixels from row %lld on, %lld rows in nnz", (long long)count, (long long)t,
	           (long long)nnz_rows);
	for (int i = 0; i < H; ++i) {
		for (int j = 0; j < W; ++j) {
			const float d = disp[(int64_t)i * W + j];
			if (d > 0.5) {
				nnz[t * 4 + 0] = (float)img;
				nnz[t * 4 + 1] = (float)i;
				nnz[t * 4 + 2] = (float)j;
				nnz[t * 4 + 3] = d;
				t++;
			}
		}
	}
	*t_out = t;
	return 0;
}

int mc_subset_dataset(const int64_t *index, int64_t n_index, const float *input, int64_t n_rows, float *output, int64_t *n_out)
{
	MC_REQUIRE(n_index >= 0 && n_rows >= 0, "mc_subset_dataset: bad sizes: %lld indices, %lld rows", (long long)n_index, (long long)n_rows);
	MC_REQUIRE(n_out && (index || n_index == 0) && ((input && output) || n_rows == 0),
	           "mc_subset_dataset: null pointer (index %p, input %p, output %p, n_out %p)", (const void *)index, (const void *)input, (void *)output,
	           (void *)n_out);
	bool set[MC_OPS_SUBSET_IMAGES] = {};
	for (int64_t i = 0; i < n_index; ++i)
		MC_REQUIRE(index[i] >= 0 && index[i] < MC_OPS_SUBSET_IMAGES, "mc_subset_dataset: index %lld (at %lld) outside [0, %d]", (long long)index[i],
		           (long long)i, MC_OPS_SUBSET_IMAGES - 1);
	for (int64_t i = 0; i < n_index; ++i) set[index[i]] = true;
	int64_t i = 0;
	for (int64_t j = 0; j < n_rows; ++j) {
		const float v = input[j * 4];
		if (!(v > -1.f && v < (float)MC_OPS_SUBSET_IMAGES)) continue;   // the reference reads outside its table here
		if (set[(int)v]) {
			for (int k = 0; k < 4; ++k) output[i * 4 + k] = input[j * 4 + k];
			i++;
		}
	}
	*n_out = i;
	return 0;
}

}  // extern "C"
