// libmcfcsplit.so (include/mc_fc_split.h): the accurate net's FC stack (fc_stack.hip) with its hidden layers on the bf16 matrix cores,
// every fp32 operand split into hi + lo bf16 parts and every product taken as three bf16 products (hi.hi + hi.lo + lo.hi) accumulated
// in fp32 (v_mfma_f32_32x32x16_bf16: 16 times the fp32-input MFMA's rate, so 16/3 of it per split product).  The header states the
// arithmetic; tests/fc_split_oracle.py restates it.
//   * layer 1 is fc_stack.hip's: two per-pixel projections on the fp32 MFMA (fcs_project_kernel), one add per voxel.
//   * a block owns FS_M = 96 consecutive voxels of one (y, d) and keeps their activations in LDS as two bf16 planes, Hs[plane][voxel][k]
//     (row stride 784 B: the 16-byte operand reads of 32 voxels fall on 32 different 16-byte bank groups).  The layer's product is taken
//     as H'^T = W H^T: the weights are the A operand (rows n), the activations the B operand (columns = voxels, a ds_read_b128 of 8
//     consecutive k per lane), so a result tile has its voxel on the lane and four consecutive n in registers 4g..4g+3: bias, ReLU and the
//     split happen in registers and one 8-byte LDS write per plane stores four n of a voxel, in place after a barrier.
//   * each of the 4 waves owns 96 output rows (three 32-row tiles) for all three voxel tiles: 9 accumulator tiles (144 registers), 27 MFMAs
//     per 16-wide k-step against 6 LDS reads and 6 16-byte weight loads.
//   * fcs_split_weights_kernel writes the weights' hi and lo planes in the A operand's fragment order, Wp[plane][n tile][k-step][lane][8],
//     so a wave's weight load is 1 KiB contiguous; they come from L2 through a register ring FS_BQ k-steps deep (one wave per SIMD:
//     nothing but prefetch covers the latency).  Same bytes per voxel as the fp32 kernel (2 x 2 B per weight).
//   * the output layer reads float(hhi) + float(hlo) back from LDS: one voxel per thread, fmaf chain in k order.
#include <atomic>

#include "mc_common.h"
#include "../../include/mc_fc_split.h"

namespace mc {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int FS_NH = MC_FC_SPLIT_NH;
constexpr int FS_MT = 3;                       // 32-voxel tiles per block
constexpr int FS_M = 32 * FS_MT;               // voxels per block
constexpr int FS_NT = FS_NH / 32;              // 32-row output tiles
constexpr int FS_KS = FS_NH / 16;              // k-steps of one layer
constexpr int FS_ROW = FS_NH * 2 + 16;         // bytes of one voxel's row in a plane
constexpr int FS_PLANE = FS_M * FS_ROW;        // bytes of a plane
constexpr int FS_LDS = 2 * FS_PLANE;
constexpr int FS_BQ = 4;                       // depth of the weight ring, in k-steps
static_assert(FS_M == MC_FC_SPLIT_VOXELS, "the header states the block's voxels");
static_assert(FS_LDS <= 160 * 1024, "LDS of one workgroup");
static_assert(FS_KS % FS_BQ == 0, "k loop shape");

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

// (bf16(a), bf16(b)) packed, a in the low half: the float -> bf16 conversion rounds to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(float a, float b)
{
	const floatx2 v = {a, b};
	return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// split(v) of the header for a pair: hi = bf16(v), lo = bf16(v - float(hi)), each packed with a in the low half
__device__ __forceinline__ void split_bf16_pair(float a, float b, unsigned &hi, unsigned &lo)
{
	hi = pack_bf16(a, b);
	lo = pack_bf16(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

// four consecutive k of one voxel: split and store 8 bytes to each plane
__device__ __forceinline__ void store_split4(unsigned char *Hs, int byte_off, const float (&v)[4])
{
	unsigned hi[2], lo[2];
	split_bf16_pair(v[0], v[1], hi[0], lo[0]);
	split_bf16_pair(v[2], v[3], hi[1], lo[1]);
	*reinterpret_cast<uint2 *>(Hs + byte_off) = make_uint2(hi[0], hi[1]);
	*reinterpret_cast<uint2 *>(Hs + FS_PLANE + byte_off) = make_uint2(lo[0], lo[1]);
}

// out[p][n] = sum_c Wt[c][n] * X[c][p]: fc_project_kernel's arithmetic (fc_stack.hip), k in pairs on the fp32 MFMA
__global__ void __launch_bounds__(256) fcs_project_kernel(const float *__restrict__ X, const float *__restrict__ Wt, float *__restrict__ out,
                                                          int C, int64_t HW)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int nl = lane & 31, kh = lane >> 5;
	const int64_t p0 = (int64_t)blockIdx.x * 32;
	const int n0 = wave * (FS_NH / 4);
	floatx16 acc[3];
#pragma unroll
	for (int t = 0; t < 3; ++t)
#pragma unroll
		for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
	const int64_t p = p0 + nl;
	for (int kk = 0; kk < (C + 1) / 2; ++kk) {
		const int c = 2 * kk + kh;
		const float a = (c < C && p < HW) ? X[(int64_t)c * HW + p] : 0.0f;
#pragma unroll
		for (int t = 0; t < 3; ++t) {
			const float b = c < C ? Wt[(int64_t)c * FS_NH + n0 + 32 * t + nl] : 0.0f;
			acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
		}
	}
#pragma unroll
	for (int t = 0; t < 3; ++t)
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			const int m = (i & 3) + 8 * (i >> 2) + 4 * kh;
			if (p0 + m < HW) out[(p0 + m) * FS_NH + n0 + 32 * t + nl] = acc[t][i];
		}
}

// layer 1's halves, transposed: out[c][r] = in[r][col0 + c], c < ncols
__global__ void __launch_bounds__(256) fcs_transpose_kernel(const float *__restrict__ in, float *__restrict__ out, int rows, int ld, int col0,
                                                            int ncols)
{
	const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (id >= (int64_t)rows * ncols) return;
	const int c = (int)(id / rows), r = (int)(id - (int64_t)c * rows);
	out[id] = in[(int64_t)r * ld + col0 + c];
}

// a hidden layer's (NH, NH) row-major fp32 weights -> Wp[plane][nt][ks][lane][8] bf16: element j of lane (r = lane & 31, h = lane >> 5)
// is W[32 nt + r][16 ks + 8 h + j], the A operand of v_mfma_f32_32x32x16_bf16.  One thread per (nt, ks, lane).
__global__ void __launch_bounds__(256) fcs_split_weights_kernel(const float *__restrict__ Wsrc, uint4 *__restrict__ Wp)
{
	const int id = blockIdx.x * blockDim.x + threadIdx.x;
	if (id >= FS_NT * FS_KS * 64) return;
	const int lane = id & 63, ks = (id >> 6) % FS_KS, nt = (id >> 6) / FS_KS;
	const float *src = Wsrc + (size_t)(32 * nt + (lane & 31)) * FS_NH + 16 * ks + 8 * (lane >> 5);
	unsigned hi[4], lo[4];
#pragma unroll
	for (int j = 0; j < 4; ++j) split_bf16_pair(src[2 * j], src[2 * j + 1], hi[j], lo[j]);
	Wp[id] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
	Wp[FS_NT * FS_KS * 64 + id] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

struct FcSplitArgs {
	const float *PL, *PR;         // (HW, NH) projections of the left / right features through layer 1
	const float *b1;              // (NH)
	const uint4 *Wp[6];           // hidden layers: the hi and lo planes in fragment order
	const float *bh[6];           // hidden biases (NH)
	int n_hidden;
	const float *wlast;           // (NH)
	const float *blast;           // (1)
	float *volL, *volR;           // (D,H,W)
	int D, H, W;
};

__device__ __forceinline__ floatx16 mfma_bf16(const uint4 &a, const uint4 &b, const floatx16 &c)
{
	return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

__global__ void __launch_bounds__(256) fcs_stack_kernel(const FcSplitArgs A)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char Hs[];  // [2][FS_M][FS_ROW]
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int nl = lane & 31, kh = lane >> 5;
	const int W = A.W, H = A.H;
	// the fp32 kernel's block order: all blocks of one image row on one XCD (its PL / PR rows stay in that L2)
	const int tiles_x = (W + FS_M - 1) / FS_M;
	const int b = blockIdx.x;
	const int xcd = b & 7, k = b >> 3;
	const int per_row = tiles_x * A.D;
	const int y = (k / per_row) * 8 + xcd;
	if (y >= H) return;
	const int rem = k % per_row;
	const int d = rem / tiles_x;
	const int x0 = d + (rem - d * tiles_x) * FS_M;   // voxels x0 .. x0+95 of (y, d); valid while x < W
	if (x0 >= W) return;
	const int nvox = min(FS_M, W - x0);
	const int64_t HW = (int64_t)H * W;
	const int64_t rowpix = (int64_t)y * W;

	// ---- layer 1: relu((PL[x] + PR[x-d]) + b1), split, four n per thread and step ----
	// (12 independent 16-byte load pairs in flight per thread: the rows come from L2, and the loop is three latencies long)
	constexpr int FILL_U = 12, NQ = FS_NH / 4;
	static_assert((FS_M * NQ) % (256 * FILL_U) == 0, "fill loop shape");
	for (int base = threadIdx.x; base < FS_M * NQ; base += 256 * FILL_U) {
		float4 pl[FILL_U], pr[FILL_U];
#pragma unroll
		for (int u = 0; u < FILL_U; ++u) {
			const int idx = base + 256 * u;
			const int m = idx / NQ, q = idx - m * NQ;
			const int64_t px = rowpix + x0 + (m < nvox ? m : 0);
			pl[u] = *reinterpret_cast<const float4 *>(A.PL + px * FS_NH + 4 * q);
			pr[u] = *reinterpret_cast<const float4 *>(A.PR + (px - d) * FS_NH + 4 * q);
		}
#pragma unroll
		for (int u = 0; u < FILL_U; ++u) {
			const int idx = base + 256 * u;
			const int m = idx / NQ, q = idx - m * NQ;
			const float4 bv = make_float4(A.b1[4 * q], A.b1[4 * q + 1], A.b1[4 * q + 2], A.b1[4 * q + 3]);   // a caller's bias may be only 4-byte aligned
			const bool in = m < nvox;
			const float v[4] = {in ? fmaxf((pl[u].x + pr[u].x) + bv.x, 0.0f) : 0.0f, in ? fmaxf((pl[u].y + pr[u].y) + bv.y, 0.0f) : 0.0f,
			                    in ? fmaxf((pl[u].z + pr[u].z) + bv.z, 0.0f) : 0.0f, in ? fmaxf((pl[u].w + pr[u].w) + bv.w, 0.0f) : 0.0f};
			store_split4(Hs, m * FS_ROW + 8 * q, v);
		}
	}
	__syncthreads();

	// ---- hidden layers: Hs <- split(relu(W Hs + b)), in place ----
	const int n0 = wave * (FS_NH / 4);
	const int b_off = nl * FS_ROW + 16 * kh;   // this lane's operand bytes of voxel tile 0, k-step 0
	for (int l = 0; l < A.n_hidden; ++l) {
		const uint4 *__restrict__ Wp = A.Wp[l] + (size_t)(3 * wave) * FS_KS * 64 + lane;
		floatx16 acc[FS_MT][3];
#pragma unroll
		for (int mt = 0; mt < FS_MT; ++mt)
#pragma unroll
			for (int t = 0; t < 3; ++t)
#pragma unroll
				for (int i = 0; i < 16; ++i) acc[mt][t][i] = 0.0f;
		uint4 aq[FS_BQ][2][3], bn[2][FS_MT];
		auto load_a = [&](uint4 (&a)[2][3], int ks) {
			const int kc = ks < FS_KS ? ks : FS_KS - 1;
#pragma unroll
			for (int p = 0; p < 2; ++p)
#pragma unroll
				for (int t = 0; t < 3; ++t) a[p][t] = Wp[(size_t)((p * FS_NT + t) * FS_KS + kc) * 64];
		};
		auto load_b = [&](uint4 (&bb)[2][FS_MT], int ks) {
#pragma unroll
			for (int p = 0; p < 2; ++p)
#pragma unroll
				for (int mt = 0; mt < FS_MT; ++mt)
					bb[p][mt] = *reinterpret_cast<const uint4 *>(Hs + p * FS_PLANE + 32 * mt * FS_ROW + b_off + 32 * ks);
		};
#pragma unroll
		for (int u = 0; u < FS_BQ; ++u) load_a(aq[u], u);
		load_b(bn, 0);
		for (int ks0 = 0; ks0 < FS_KS; ks0 += FS_BQ) {
#pragma unroll
			for (int u = 0; u < FS_BQ; ++u) {
				const int ks = ks0 + u;
				uint4 bc[2][FS_MT];
#pragma unroll
				for (int p = 0; p < 2; ++p)
#pragma unroll
					for (int mt = 0; mt < FS_MT; ++mt) bc[p][mt] = bn[p][mt];
				load_b(bn, ks + 1 < FS_KS ? ks + 1 : ks);
				__builtin_amdgcn_sched_barrier(0);
				// the three products of the split: hi.hi, hi.lo, lo.hi (operand 0 = the hi plane)
#pragma unroll
				for (int mt = 0; mt < FS_MT; ++mt)
#pragma unroll
					for (int t = 0; t < 3; ++t) acc[mt][t] = mfma_bf16(aq[u][0][t], bc[0][mt], acc[mt][t]);
#pragma unroll
				for (int mt = 0; mt < FS_MT; ++mt)
#pragma unroll
					for (int t = 0; t < 3; ++t) acc[mt][t] = mfma_bf16(aq[u][0][t], bc[1][mt], acc[mt][t]);
#pragma unroll
				for (int mt = 0; mt < FS_MT; ++mt)
#pragma unroll
					for (int t = 0; t < 3; ++t) acc[mt][t] = mfma_bf16(aq[u][1][t], bc[0][mt], acc[mt][t]);
				// the slot is consumed and refilled FS_BQ steps ahead (fc_stack.hip's ring)
				__builtin_amdgcn_sched_barrier(0);
				load_a(aq[u], ks + FS_BQ);
				__builtin_amdgcn_sched_barrier(0);
			}
		}
		__syncthreads();  // every wave has read the whole of Hs
		const float *__restrict__ bias = A.bh[l];
#pragma unroll
		for (int t = 0; t < 3; ++t)
#pragma unroll
			for (int g = 0; g < 4; ++g) {
				const int n = n0 + 32 * t + 8 * g + 4 * kh;   // registers 4g .. 4g+3 hold rows n .. n+3 of the tile
				const float4 bv = make_float4(bias[n], bias[n + 1], bias[n + 2], bias[n + 3]);
#pragma unroll
				for (int mt = 0; mt < FS_MT; ++mt) {
					const float v[4] = {fmaxf(acc[mt][t][4 * g] + bv.x, 0.0f), fmaxf(acc[mt][t][4 * g + 1] + bv.y, 0.0f),
					                    fmaxf(acc[mt][t][4 * g + 2] + bv.z, 0.0f), fmaxf(acc[mt][t][4 * g + 3] + bv.w, 0.0f)};
					store_split4(Hs, (32 * mt + nl) * FS_ROW + 2 * n, v);
				}
			}
		__syncthreads();
	}

	// ---- output layer: sigmoid(w . (hhi + hlo) + b) ----
	if (threadIdx.x < FS_M) {
		const int m = threadIdx.x;
		if (m < nvox) {
			float s = 0.0f;
			for (int kx = 0; kx < FS_NH; kx += 8) {
				const uint4 hh = *reinterpret_cast<const uint4 *>(Hs + m * FS_ROW + 2 * kx);
				const uint4 hl = *reinterpret_cast<const uint4 *>(Hs + FS_PLANE + m * FS_ROW + 2 * kx);
				const unsigned wh[4] = {hh.x, hh.y, hh.z, hh.w}, wl[4] = {hl.x, hl.y, hl.z, hl.w};
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const float h0 = __uint_as_float(wh[e] << 16) + __uint_as_float(wl[e] << 16);
					const float h1 = __uint_as_float(wh[e] & 0xffff0000u) + __uint_as_float(wl[e] & 0xffff0000u);
					s = fmaf(A.wlast[kx + 2 * e], h0, s);
					s = fmaf(A.wlast[kx + 2 * e + 1], h1, s);
				}
			}
			s += A.blast[0];
			const float r = 1.0f / (1.0f + expf(-s));
			const int x = x0 + m;
			A.volL[(int64_t)d * HW + rowpix + x] = r;
			A.volR[(int64_t)d * HW + rowpix + x - d] = r;
		}
	}
}

static size_t fcs_workspace_bytes(int C, int n_hidden, int H, int W)
{
	const size_t HW = (size_t)H * W;
	size_t b = 2 * HW * FS_NH * sizeof(float);                                 // PL, PR
	b += (size_t)2 * C * FS_NH * sizeof(float);                                // layer 1's halves, transposed
	b += (size_t)n_hidden * 2 * FS_NH * FS_NH * sizeof(unsigned short);        // hi and lo planes
	return (b + 255) & ~(size_t)255;
}

static int64_t fcs_blocks(int H, int W, int D) { return (int64_t)((H + 7) / 8) * ((W + FS_M - 1) / FS_M) * D * 8; }

// the kernel's LDS exceeds the default limit: raised once per device; two threads that race both raise it, which is harmless
static int fcs_raise_lds()
{
	constexpr int MAX_DEV = 64;
	static std::atomic<bool> raised[MAX_DEV];
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e == hipSuccess && (dev < 0 || dev >= MAX_DEV || !raised[dev].load(std::memory_order_acquire))) {
		e = hipFuncSetAttribute((const void *)fcs_stack_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, FS_LDS);
		if (e == hipSuccess && dev >= 0 && dev < MAX_DEV) raised[dev].store(true, std::memory_order_release);
	}
	if (e != hipSuccess) {
		set_error("mc_fc_split_stack: hipFuncSetAttribute: %s", hipGetErrorString(e));
		return (int)e;
	}
	return 0;
}

static int fcs_stack(const float *featL, const float *featR, int C, int H, int W, int D, const float *const *weights,
                     const float *const *biases, int n_layers, float *volL, float *volR, void *workspace, hipStream_t st)
{
	const int n_hidden = n_layers - 2;
	const int64_t HW = (int64_t)H * W;
	float *PL = (float *)workspace, *PR = PL + HW * FS_NH;
	float *W1Lt = PR + HW * FS_NH, *W1Rt = W1Lt + (size_t)C * FS_NH;
	uint4 *Wp = reinterpret_cast<uint4 *>(W1Rt + (size_t)C * FS_NH);
	const int rc = fcs_raise_lds();
	if (rc) return rc;
	hipLaunchKernelGGL(fcs_transpose_kernel, dim3(cdiv((int64_t)FS_NH * C, 256)), dim3(256), 0, st, weights[0], W1Lt, FS_NH, 2 * C, 0, C);
	hipLaunchKernelGGL(fcs_transpose_kernel, dim3(cdiv((int64_t)FS_NH * C, 256)), dim3(256), 0, st, weights[0], W1Rt, FS_NH, 2 * C, C, C);
	FcSplitArgs A;
	constexpr int FRAGS = FS_NT * FS_KS * 64;   // uint4s of one plane
	for (int l = 0; l < n_hidden; ++l) {
		uint4 *wp = Wp + (size_t)l * 2 * FRAGS;
		hipLaunchKernelGGL(fcs_split_weights_kernel, dim3(cdiv(FRAGS, 256)), dim3(256), 0, st, weights[1 + l], wp);
		A.Wp[l] = wp;
		A.bh[l] = biases[1 + l];
	}
	hipLaunchKernelGGL(fcs_project_kernel, dim3(cdiv(HW, 32)), dim3(256), 0, st, featL, W1Lt, PL, C, HW);
	hipLaunchKernelGGL(fcs_project_kernel, dim3(cdiv(HW, 32)), dim3(256), 0, st, featR, W1Rt, PR, C, HW);
	A.PL = PL; A.PR = PR; A.b1 = biases[0];
	A.n_hidden = n_hidden;
	A.wlast = weights[n_layers - 1];
	A.blast = biases[n_layers - 1];
	A.volL = volL; A.volR = volR;
	A.D = D; A.H = H; A.W = W;
	hipLaunchKernelGGL(fcs_stack_kernel, dim3((unsigned)fcs_blocks(H, W, D)), dim3(256), FS_LDS, st, A);
	return check_launch("mc_fc_split_stack");
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_fc_split_version(void) { return MC_FC_SPLIT_ABI_VERSION; }

const char *mc_fc_split_last_error(void) { return last_error(); }

size_t mc_fc_split_workspace_bytes(int C, int n_layers, int H, int W)
{
	if (C < 1 || n_layers < 2 || n_layers > 8 || H < 1 || W < 1) return 0;
	return fcs_workspace_bytes(C, n_layers - 2, H, W);
}

int mc_fc_split_stack(const float *featL, const float *featR, int C, int H, int W, int D, const float *const *weights,
                      const float *const *biases, const int *layer_out, int n_layers, float *volL, float *volR, void *workspace,
                      size_t workspace_bytes, void *stream)
{
	MC_REQUIRE(featL && featR && weights && biases && layer_out && volL && volR && workspace, "mc_fc_split_stack: null pointer");
	MC_REQUIRE(dims_ok(D, H, W) && C >= 1, "mc_fc_split_stack: bad dims C=%d D=%d H=%d W=%d", C, D, H, W);
	MC_REQUIRE(n_layers >= 2 && n_layers <= 8, "mc_fc_split_stack: 2..8 layers supported, not %d", n_layers);
	for (int l = 0; l < n_layers - 1; ++l)
		MC_REQUIRE(layer_out[l] == FS_NH, "mc_fc_split_stack: hidden width %d not supported (nh2 = 384 in every preset, main.lua:77,124)",
		           layer_out[l]);
	MC_REQUIRE(layer_out[n_layers - 1] == 1, "mc_fc_split_stack: the last layer must have one output, not %d", layer_out[n_layers - 1]);
	for (int l = 0; l < n_layers; ++l) MC_REQUIRE(weights[l] && biases[l], "mc_fc_split_stack: null pointer in layer %d", l);
	MC_REQUIRE(workspace_bytes >= fcs_workspace_bytes(C, n_layers - 2, H, W), "mc_fc_split_stack: workspace %zu < %zu bytes", workspace_bytes,
	           fcs_workspace_bytes(C, n_layers - 2, H, W));
	MC_REQUIRE((uintptr_t)workspace % 16 == 0, "mc_fc_split_stack: workspace must be 16-byte aligned");
	MC_REQUIRE(fcs_blocks(H, W, D) < ((int64_t)1 << 31), "mc_fc_split_stack: problem too large for one launch (%lld workgroups)",
	           (long long)fcs_blocks(H, W, D));
	return fcs_stack(featL, featR, C, H, W, D, weights, biases, n_layers, volL, volR, workspace, as_stream(stream));
}

}  // extern "C"
