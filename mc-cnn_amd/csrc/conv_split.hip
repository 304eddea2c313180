// libmcconvsplit.so (include/mc_conv_split.h): the feature nets' 3x3 convolution (conv3x3.hip) on the bf16 matrix cores, every fp32
// operand split into hi + lo bf16 parts and every product taken as three bf16 products (hi.hi + hi.lo + lo.hi) accumulated in fp32
// (v_mfma_f32_32x32x16_bf16: 16 times the fp32-input MFMA's rate, so 16/3 of it per split product).  The header states the arithmetic;
// tests/conv_split_oracle.py restates it.
//   * an implicit GEMM as in conv3x3.hip: the weights are the A operand (32 output channels x 16 input channels of one filter tap), the
//     activations the B operand (16 input channels x 32 pixels of one image row), so a lane ends up with 16 output channels of ONE pixel
//     and the 32 lanes of a half-wave store 32 consecutive pixels of a channel (128-byte lines).
//   * a block of four waves owns CS_ROWS x 32 output pixels of one image for one group of NT x 32 output channels, each wave CS_R
//     rows of them: CS_R x NT accumulator tiles stay in registers over the loop over chunks of 16 input channels.
//   * per chunk the block stages, behind one barrier pair,
//     (a) the tile's input plus a one-pixel halo: read from the planar fp32 input a dword per lane along the row (a raw buffer over the
//     chunk's 16 planes; a position outside the image gets an out-of-range offset and reads 0: the padding), split in registers, written
//     to LDS as two bf16 planes As[plane][half][row][col][8 channels] -- a half = the 8 channels of a lane half of the matrix
//     instruction, 16 bytes per pixel: the operand read of a half-wave is 512 bytes contiguous and free of bank conflicts (with the halves
//     side by side in one 32-byte pixel the 16-lane groups of a ds_read_b128 fell on half of the banks twice).  Once per staged pixel,
//     not once per tap: the nine taps are nine addresses into that image;
//     (b) the chunk's slice of the weights, which conv_split_prep_kernel wrote as hi and lo planes in the A operand's fragment order
//     Wp[group][chunk][tap][tile][plane][lane][8], so the copy is straight and a wave's operand read 1 KiB contiguous.
//     The next chunk's activations are requested into registers before the chunk's products and written after them.
//   * LDS: 38.3 KiB of activations + 36 KiB of weights (NT = 2): two blocks per CU, one staging while the other multiplies.
//   * the stores take 64-bit offsets and test every channel against Cout, so the padded channels of a last, partly filled group
//     never reach memory (ADVICE.md's first finding is about 32-bit offsets of such channels wrapping).
#include <atomic>
#include <type_traits>

#include "mc_common.h"
#include "../../include/mc_conv_split.h"

namespace mc {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

constexpr int CS_R = 4;                         // rows of a wave
constexpr int CS_ROWS = 4 * CS_R;               // rows of a block
constexpr int CS_COLS = 32;                     // columns of a block: the pixel lanes of the matrix instruction
constexpr int CS_TR = CS_ROWS + 2, CS_TC = CS_COLS + 2;   // the staged tile with its halo
constexpr int CS_PIX = CS_TR * CS_TC;
constexpr int CS_AHALF = CS_PIX * 16;           // bytes of one channel half (8 channels per pixel) of a bf16 plane of the staged tile
constexpr int CS_APLANE = 2 * CS_AHALF;         // bytes of one bf16 plane (16 channels per pixel)
constexpr int CS_ITEMS = CS_PIX * 2;            // (pixel, channel half) pairs a block stages per chunk
constexpr int CS_ITERS = (CS_ITEMS + 255) / 256;
constexpr int cs_wslab(int NT) { return 9 * NT * 2 * 64; }      // uint4s of one (group, chunk) slice of the weights
constexpr int cs_lds(int NT) { return 2 * CS_APLANE + cs_wslab(NT) * 16; }
static_assert(cs_lds(2) * 2 <= 160 * 1024, "two blocks per CU");

// (bf16(a), bf16(b)) packed, a in the low half: the float -> bf16 conversion rounds to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned cs_pack_bf16(float a, float b)
{
	const floatx2 v = {a, b};
	return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// split(v) of the header for a pair: hi = bf16(v), lo = bf16(v - float(hi)), each packed with a in the low half
__device__ __forceinline__ void cs_split_pair(float a, float b, unsigned &hi, unsigned &lo)
{
	hi = cs_pack_bf16(a, b);
	lo = cs_pack_bf16(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

constexpr uint32_t CS_OOB = 0xFFFFFFF0u;        // a byte offset beyond every buffer: loads return 0

// A raw buffer over `bytes` bytes at p, both wave-uniform and passed through readfirstlane so that the compiler knows it (conv3x3.hip)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t cs_uniform_rsrc(const float *p, uint32_t bytes)
{
	const uint64_t a = (uint64_t)p;
	const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
	return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), 0, (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

__device__ __forceinline__ floatx16 cs_mfma(const uint4 &a, const uint4 &b, const floatx16 &c)
{
	return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// W (Cout, Cin, 3, 3) fp32 -> Wp[group][chunk][tap][t][plane][lane][8] bf16: element j of lane (r = lane & 31, h = lane >> 5) is
// W[co = 32 (group NT + t) + r][ci = 16 chunk + 8 h + j][tap], zero for co >= Cout.  One thread per (group, chunk, tap, t, lane).
__global__ void __launch_bounds__(256) conv_split_prep_kernel(const float *__restrict__ w, uint4 *__restrict__ Wp, int Cin, int Cout, int NT,
                                                              int groups)
{
	const int nch = Cin / 16;
	const int id = blockIdx.x * blockDim.x + threadIdx.x;
	if (id >= groups * nch * 9 * NT * 64) return;
	const int lane = id & 63;
	int q = id >> 6;
	const int t = q % NT; q /= NT;
	const int tap = q % 9; q /= 9;
	const int ch = q % nch, g = q / nch;
	const int co = 32 * (g * NT + t) + (lane & 31), ci = 16 * ch + 8 * (lane >> 5);
	unsigned hi[4], lo[4];
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const float a = co < Cout ? w[((size_t)co * Cin + ci + 2 * j) * 9 + tap] : 0.0f;
		const float b = co < Cout ? w[((size_t)co * Cin + ci + 2 * j + 1) * 9 + tap] : 0.0f;
		cs_split_pair(a, b, hi[j], lo[j]);
	}
	const size_t o = ((((size_t)(g * nch + ch) * 9 + tap) * NT + t) * 2) * 64 + lane;
	Wp[o] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
	Wp[o + 64] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

// blockIdx.x = ((n * tiles_y + ty) * tiles_x + tx) * groups + group: the groups of a tile run side by side and share its input in L2
template <int NT>
__global__ void __launch_bounds__(256, 2) conv_split_kernel(const float *__restrict__ in, const uint4 *__restrict__ Wp, const float *__restrict__ bias,
                                                            float *__restrict__ out, int Cin, int Cout, int H, int W, int tiles_x, int tiles_y,
                                                            int groups, int relu)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char Ls[];   // As[plane 2][half 2][CS_TR][CS_TC][8] bf16, then Ws[9][NT][2][64] uint4
	constexpr int WSLAB = cs_wslab(NT);
	uint4 *Ws = reinterpret_cast<uint4 *>(Ls + 2 * CS_APLANE);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int nl = lane & 31, kh = lane >> 5;
	int b = blockIdx.x;
	const int grp = b % groups; b /= groups;
	const int tx = b % tiles_x; b /= tiles_x;
	const int ty = b % tiles_y, n = b / tiles_y;
	const int x0 = tx * CS_COLS, y0 = ty * CS_ROWS;
	const int co0 = grp * NT * 32;
	const int nch = Cin / 16;
	const int64_t HW = (int64_t)H * W;
	const uint32_t plane = (uint32_t)HW * 4u;        // bytes of one channel

	// the block's staging items: item = 2 * pixel + channel half, so that consecutive lanes write consecutive 16 bytes of a plane
	// byte offset of the item's pixel and channel half within the chunk's 16 planes; outside the image (or no item): an offset beyond
	// the buffer, for which the hardware returns 0 -- the zero padding
	uint32_t soff[CS_ITERS];
#pragma unroll
	for (int it = 0; it < CS_ITERS; ++it) {
		const int item = it * 256 + tid, pix = item >> 1;
		const int r = pix / CS_TC, c = pix - r * CS_TC;
		const int y = y0 - 1 + r, x = x0 - 1 + c;
		soff[it] = (item < CS_ITEMS && y >= 0 && y < H && x >= 0 && x < W) ? (uint32_t)(8 * (tid & 1)) * plane + (uint32_t)(y * W + x) * 4u : CS_OOB;
	}
	float sv[CS_ITERS][8];
	// a chunk's 16 planes as one raw buffer (16 * plane < 2^32: the entry checks (Cin + 1) * plane); channel j of the thread's half
	// through the scalar offset
	auto request = [&](int ch) {
		const __amdgpu_buffer_rsrc_t rs = cs_uniform_rsrc(in + ((int64_t)n * Cin + 16 * ch) * HW, 16u * plane);
#pragma unroll
		for (int it = 0; it < CS_ITERS; ++it)
#pragma unroll
			for (int j = 0; j < 8; ++j) sv[it][j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, soff[it], (uint32_t)j * plane, 0));
	};
	auto stage = [&](int ch) {
#pragma unroll
		for (int it = 0; it < CS_ITERS; ++it) {
			const int item = it * 256 + tid;
			unsigned hi[4], lo[4];
#pragma unroll
			for (int j = 0; j < 4; ++j) cs_split_pair(sv[it][2 * j], sv[it][2 * j + 1], hi[j], lo[j]);
			if (item < CS_ITEMS) {
				const int o = (item & 1) * CS_AHALF + (item >> 1) * 16;
				*reinterpret_cast<uint4 *>(Ls + o) = make_uint4(hi[0], hi[1], hi[2], hi[3]);
				*reinterpret_cast<uint4 *>(Ls + CS_APLANE + o) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
			}
		}
		const uint4 *__restrict__ src = Wp + (size_t)(grp * nch + ch) * WSLAB;
#pragma unroll
		for (int u = 0; u < (WSLAB + 255) / 256; ++u)
			if (WSLAB % 256 == 0 || u * 256 + tid < WSLAB) Ws[u * 256 + tid] = src[u * 256 + tid];
	};

	floatx16 acc[CS_R][NT];
#pragma unroll
	for (int r = 0; r < CS_R; ++r)
#pragma unroll
		for (int t = 0; t < NT; ++t)
#pragma unroll
			for (int i = 0; i < 16; ++i) acc[r][t][i] = 0.0f;

	// the wave's rows that exist, and the group's channel tiles that do: both wave-uniform
	const int yw = y0 + wave * CS_R;
	const int rows = min(CS_R, H - yw);                              // <= 0: the wave only stages
	const int nt_act = min(NT, (Cout - co0 + 31) / 32);
	const unsigned char *Bl = Ls + kh * CS_AHALF + ((wave * CS_R) * CS_TC + nl) * 16;   // this lane's operand bytes at tap (0, 0) of the wave's row 0

	// a chunk's products; full: every row and channel tile of the wave exists (straight-line code), otherwise each is tested
	auto products = [&](auto full) {
#pragma unroll
		for (int tap = 0; tap < 9; ++tap) {
			const int ky = tap / 3, kx = tap - 3 * ky;
			uint4 a[NT][2], bb[CS_R][2];
#pragma unroll
			for (int t = 0; t < NT; ++t)
#pragma unroll
				for (int p = 0; p < 2; ++p) a[t][p] = Ws[((tap * NT + t) * 2 + p) * 64 + lane];
#pragma unroll
			for (int r = 0; r < CS_R; ++r)
#pragma unroll
				for (int p = 0; p < 2; ++p) bb[r][p] = *reinterpret_cast<const uint4 *>(Bl + p * CS_APLANE + ((r + ky) * CS_TC + kx) * 16);
			// the three products of the split: hi.hi, hi.lo, lo.hi (operand 0 = the hi plane)
#pragma unroll
			for (int pr = 0; pr < 3; ++pr)
#pragma unroll
				for (int r = 0; r < CS_R; ++r)
#pragma unroll
					for (int t = 0; t < NT; ++t)
						if (decltype(full)::value || (r < rows && t < nt_act)) acc[r][t] = cs_mfma(a[t][pr == 2], bb[r][pr == 1], acc[r][t]);
			__builtin_amdgcn_sched_barrier(0);   // a tap's operands at a time: nine taps' reads hoisted ahead of the products would spill
		}
	};

	request(0);
	for (int ch = 0; ch < nch; ++ch) {
		__syncthreads();            // every wave is done with the previous chunk
		stage(ch);
		__syncthreads();
		if (ch + 1 < nch) request(ch + 1);   // in flight during this chunk's products
		if (rows <= 0) continue;
		if (rows == CS_R && nt_act == NT) products(std::true_type());
		else products(std::false_type());
	}

	// a lane holds pixel x0 + nl of rows yw .. yw + rows - 1 for output channels co0 + 32 t + (i & 3) + 8 (i >> 2) + 4 kh
	// Bias and ReLU on every sum first, the stores after them with nothing but stores between.  The bias comes through scalar loads
	// (the channel is wave-uniform up to the lane half: both halves' values are read and one selected): a vector load among the stores
	// is waited for with vmcnt, which counts the stores too -- each channel then waited for the previous channel's rows to reach memory.
	const int ox = x0 + nl;
	if (ox >= W) return;
#pragma unroll
	for (int t = 0; t < NT; ++t)
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			const int cb = co0 + 32 * t + (i & 3) + 8 * (i >> 2);          // wave-uniform; the lane's channel is cb + 4 kh
			const float b0 = bias[min(cb, Cout - 1)], b1 = bias[min(cb + 4, Cout - 1)];
			const float bv = kh ? b1 : b0;
#pragma unroll
			for (int r = 0; r < CS_R; ++r) {
				const float v = acc[r][t][i] + bv;
				acc[r][t][i] = relu ? fmaxf(v, 0.0f) : v;
			}
		}
	__builtin_amdgcn_sched_barrier(0);
#pragma unroll
	for (int t = 0; t < NT; ++t) {
#pragma unroll
		for (int i = 0; i < 16; ++i) {
			const int co = co0 + 32 * t + (i & 3) + 8 * (i >> 2) + 4 * kh;
			if (co >= Cout) continue;
			float *__restrict__ dst = out + ((int64_t)n * Cout + co) * HW + (int64_t)yw * W + ox;   // 64-bit: nothing to wrap
#pragma unroll
			for (int r = 0; r < CS_R; ++r) {
				if (r >= rows) break;
				dst[(int64_t)r * W] = acc[r][t][i];
			}
		}
	}
}

// the split of a layer: NT tiles of 32 output channels per group (one tile for Cout <= 32, otherwise two)
struct ConvSplitPlan { int NT, groups; };

static ConvSplitPlan cs_plan(int Cout)
{
	ConvSplitPlan p;
	p.NT = Cout <= 32 ? 1 : 2;
	p.groups = (Cout + 32 * p.NT - 1) / (32 * p.NT);
	return p;
}

static bool cs_eligible(int Cin, int Cout)
{
	return Cin >= MC_CONV_SPLIT_CIN_STEP && Cin % MC_CONV_SPLIT_CIN_STEP == 0 && Cout >= 1 && Cout <= MC_CONV_SPLIT_MAX_COUT;
}

static size_t cs_workspace_bytes(int Cin, int Cout)
{
	const ConvSplitPlan p = cs_plan(Cout);
	return ((size_t)p.groups * (Cin / 16) * cs_wslab(p.NT) * 16 + 255) & ~(size_t)255;
}

static int64_t cs_blocks(int N, int Cout, int H, int W)
{
	return (int64_t)N * ((H + CS_ROWS - 1) / CS_ROWS) * ((W + CS_COLS - 1) / CS_COLS) * cs_plan(Cout).groups;
}

// NT = 2's LDS exceeds the default limit: raised once per (instance, device); two threads that race both raise it, which is harmless
template <int NT>
static int cs_raise_lds()
{
	constexpr int MAX_DEV = 64;
	static std::atomic<bool> raised[MAX_DEV];
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e == hipSuccess && (dev < 0 || dev >= MAX_DEV || !raised[dev].load(std::memory_order_acquire))) {
		e = hipFuncSetAttribute((const void *)conv_split_kernel<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, cs_lds(NT));
		if (e == hipSuccess && dev >= 0 && dev < MAX_DEV) raised[dev].store(true, std::memory_order_release);
	}
	if (e != hipSuccess) {
		set_error("mc_conv_split: hipFuncSetAttribute: %s", hipGetErrorString(e));
		return (int)e;
	}
	return 0;
}

template <int NT>
static int cs_launch(const float *in, const uint4 *Wp, const float *bias, float *out, int N, int Cin, int Cout, int H, int W, int relu, int groups,
                     hipStream_t st)
{
	const int rc = cs_raise_lds<NT>();
	if (rc) return rc;
	const int tiles_x = (W + CS_COLS - 1) / CS_COLS, tiles_y = (H + CS_ROWS - 1) / CS_ROWS;
	hipLaunchKernelGGL(conv_split_kernel<NT>, dim3((unsigned)cs_blocks(N, Cout, H, W)), dim3(256), cs_lds(NT), st, in, Wp, bias, out, Cin, Cout, H, W,
	                   tiles_x, tiles_y, groups, relu);
	return 0;
}

static int conv_split(const float *in, const float *w, const float *bias, float *out, int N, int Cin, int Cout, int H, int W, int relu,
                      void *workspace, hipStream_t st)
{
	const ConvSplitPlan p = cs_plan(Cout);
	uint4 *Wp = reinterpret_cast<uint4 *>(workspace);
	const int threads = p.groups * (Cin / 16) * 9 * p.NT * 64;
	hipLaunchKernelGGL(conv_split_prep_kernel, dim3(cdiv(threads, 256)), dim3(256), 0, st, w, Wp, Cin, Cout, p.NT, p.groups);
	const int rc = p.NT == 1 ? cs_launch<1>(in, Wp, bias, out, N, Cin, Cout, H, W, relu ? 1 : 0, p.groups, st)
	                         : cs_launch<2>(in, Wp, bias, out, N, Cin, Cout, H, W, relu ? 1 : 0, p.groups, st);
	if (rc) return rc;
	return check_launch("mc_conv_split");
}

}  // namespace mc

using namespace mc;

extern "C" {

int mc_conv_split_version(void) { return MC_CONV_SPLIT_ABI_VERSION; }

const char *mc_conv_split_last_error(void) { return last_error(); }

size_t mc_conv_split_workspace_bytes(int Cin, int Cout)
{
	if (!cs_eligible(Cin, Cout)) return 0;
	return cs_workspace_bytes(Cin, Cout);
}

int mc_conv_split(const float *in, const float *weight, const float *bias, float *out, int N, int Cin, int Cout, int H, int W, int relu,
                  void *workspace, size_t workspace_bytes, void *stream)
{
	MC_REQUIRE(in && weight && bias && out && workspace, "mc_conv_split: null pointer");
	MC_REQUIRE(out != in && out != weight && out != bias && workspace != (const void *)in && workspace != (const void *)weight &&
	               workspace != (const void *)bias && workspace != (const void *)out,
	           "mc_conv_split: aliased pointers (out and workspace must differ from every other argument)");
	MC_REQUIRE(N >= 1 && dims_ok(1, H, W), "mc_conv_split: bad dims N=%d H=%d W=%d", N, H, W);
	MC_REQUIRE(cs_eligible(Cin, Cout),
	           "mc_conv_split: a %d -> %d layer is not eligible: Cin %% 16 == 0, Cin >= 16 and 1 <= Cout <= 128 are (a k-step of the bf16 matrix "
	           "instruction is 16 input channels of one tap); mc_conv3x3 takes every other layer",
	           Cin, Cout);
	// mc_conv3x3's bounds, so that the two operators take the same problems
	MC_REQUIRE((int64_t)(Cout > Cin ? Cout : Cin + 1) * H * W * 4 < (int64_t)0xFFFFFF00 && (int64_t)N * ((W + 31) / 32) * H < ((int64_t)1 << 31) &&
	               cs_blocks(N, Cout, H, W) < ((int64_t)1 << 31),
	           "mc_conv_split: %d x %d x (%d -> %d channels) x %d images exceeds mc_conv3x3's size bounds", H, W, Cin, Cout, N);
	MC_REQUIRE(workspace_bytes >= cs_workspace_bytes(Cin, Cout), "mc_conv_split: workspace %zu < %zu bytes", workspace_bytes,
	           cs_workspace_bytes(Cin, Cout));
	MC_REQUIRE((uintptr_t)workspace % 16 == 0, "mc_conv_split: workspace must be 16-byte aligned");
	return conv_split(in, weight, bias, out, N, Cin, Cout, H, W, relu, workspace, as_stream(stream));
}

}  // extern "C"
