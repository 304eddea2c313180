// What the four training libraries (train.hip, train_slow.hip, train_mb.hip, train_mb_slow.hip) derive from the description of
// their net, and the host code they share.  A net N is a struct of constants:
//   FM         feature maps per convolution (64: the 32x32x2 GEMMs of train_conv.h; 112: the 16x16x4 GEMMs of train_slow_conv.h)
//   PS         patch side (9 or 11): layer l's activations are side(l) = PS - 2 l pixels wide
//   NL         valid 3x3 convolutions (4 or 5)
//   NP         patches per tower workgroup (3: a pair's; 1)
//   L2         hidden Linears (0 for the fast nets, which have no FC stack; 4 or 3)
//   MAX_PAIRS  pairs per batch
//   PREFIX     what every message starts with ("train", "train_slow", "train_mb", "train_mb_slow")
// The flat parameter buffer starts w1 b1 w2 b2 .. wNL bNL.  The tower kernels' LDS holds the workgroup's patches X in a slot
// of their pixels rounded up to 128 floats, then A_1 .. A_NL, each [NP][FM][side(l)^2], back to back.
#pragma once
#include "mc_common.h"
#include "train_range.h"

#include <initializer_list>

namespace mc {

template <class N> __host__ __device__ constexpr int side(int l) { return N::PS - 2 * l; }
template <class N> __host__ __device__ constexpr int off_w(int l) { return l == 1 ? 0 : N::FM * 9 + N::FM + (l - 2) * (N::FM * N::FM * 9 + N::FM); }
template <class N> __host__ __device__ constexpr int off_b(int l) { return off_w<N>(l) + (l == 1 ? 1 : N::FM) * N::FM * 9; }
template <class N> __host__ __device__ constexpr int n_conv() { return off_b<N>(N::NL) + N::FM; }   // floats of the convolutions' parameters

// LDS offset (floats) of X (l = 0) and A_l; lds_act(NL + 1) is where the activations end
template <class N> __host__ __device__ constexpr int lds_act(int l)
{
	int o = l == 0 ? 0 : (N::NP * N::PS * N::PS + 127) / 128 * 128;
	for (int k = 1; k < l; ++k) o += N::NP * N::FM * side<N>(k) * side<N>(k);
	return o;
}

// ---- host: argument checks, every message byte for byte what each library printed when it had its own copy ----------------
static int check_image_args(const char *prefix, const float *x0, const float *x1, int n_img, int H, int W, const float *nnz, int64_t n_nnz)
{
	MC_REQUIRE(x0 && x1 && nnz, "%s: null image / nnz pointer", prefix);
	MC_REQUIRE(n_img >= 1 && H >= 4 && W >= 4 && (int64_t)n_img * H * W < ((int64_t)1 << 40), "%s: bad image dims %d x %d x %d", prefix, n_img, H, W);
	MC_REQUIRE(H < 32768 && W < 32768, "%s: images of %d x %d exceed the warp's 16-bit coordinates", prefix, H, W);
	MC_REQUIRE(n_nnz >= 1, "%s: empty nnz", prefix);
	return 0;
}

// the ragged image store of the Middlebury libraries (table: mc_train_mb_plane[n_planes])
static int check_store_args(const char *prefix, const float *planes, const void *table, int n_planes, const float *nnz, int64_t n_nnz)
{
	MC_REQUIRE(planes && table && nnz, "%s: null planes / table / nnz pointer", prefix);
	MC_REQUIRE(n_planes >= 1, "%s: n_planes %d", prefix, n_planes);
	MC_REQUIRE(n_nnz >= 1, "%s: empty nnz", prefix);
	return 0;
}

// check_launch("<prefix> <what>")
static int check_launch(const char *prefix, const char *what)
{
	char name[64];
	snprintf(name, sizeof(name), "%s %s", prefix, what);
	return check_launch(name);
}

// Lets the kernels ks take lds_bytes of dynamic LDS; once per library (each calls it from one place).
static int prepare_kernels(const char *prefix, std::initializer_list<const void *> ks, size_t lds_bytes)
{
	static int rc = -1;
	if (rc >= 0) return rc;
	for (const void *k : ks) {
		const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
		if (e != hipSuccess) {
			set_error("%s: hipFuncSetAttribute(%zu bytes of LDS): %s", prefix, lds_bytes, hipGetErrorString(e));
			return (int)e;
		}
	}
	rc = 0;
	return rc;
}

// The body of mc_train*_run after the library's own argument checks: pointers_given is whether the arrays that only a run
// takes are all there; steps [t0, t0 + n_steps * n_pairs) must lie inside the permutation (train_range.h); prepare() is the
// library's prepare_kernels; then step(s, first) enqueues step s, whose pairs are first = s * n_pairs .. of the run's.
template <class Prepare, class Step>
static int run_steps(const char *prefix, bool pointers_given, int64_t t0, int n_steps, int n_pairs, int64_t n_perm, Prepare prepare, Step step)
{
	MC_REQUIRE(pointers_given, "%s_run: null pointer", prefix);
	MC_REQUIRE(n_steps >= 0, "%s_run: n_steps %d", prefix, n_steps);
	int64_t end;   // the first row after the last step's, saturated: train_range.h
	MC_REQUIRE(train_steps_fit(t0, n_steps, n_pairs, n_perm, &end), "%s_run: steps [%lld, %lld) of the permutation exceed its %lld rows", prefix,
	           (long long)t0, (long long)end, (long long)n_perm);
	if (int rc = prepare()) return rc;
	for (int s = 0; s < n_steps; ++s)
		if (int rc = step(s, (int64_t)s * n_pairs)) return rc;
	return 0;
}

}  // namespace mc
