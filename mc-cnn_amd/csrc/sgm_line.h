// The SGM line walks (device code): what sgm.hip's sweeps and sgm_recompute.hip's checkpoint launches instantiate.  A kernel instance lives
// in the library whose unit launches it; this header launches nothing.
#pragma once
#include "launchers.h"

#include <type_traits>

// cache policy of the volume accesses: nt (bit 1) -- every cost run is read or written once per sweep; streaming them keeps
// the edge-class maps (re-read by every line) in L2
#define MC_SGM_VOL_AUX 2
#define MC_SGM_ST_AUX MC_SGM_VOL_AUX   // (the stores' policy on its own: profiles/r05_ab_sgm_store_policy.txt)

namespace mc {

constexpr int SGM_PADW = 520;  // >= 63*8 + 7 + slack: window starts reach -(VPL*63+VPL-1)
// VPL = 16 (D in 513..1024): a lane's window bytes start at -(16*63 + 12 + 3) = -1023 at the least and at W - 1 + 16*63 + 12 at the most; the
// maps of such a call are laid out with this pad (sgm_padw), the bias of the window descriptor follows it.  VPL = 4 and 8 keep 520 and 1024.
constexpr int SGM_PADW_WIDE = 1032;
constexpr int sgm_padw_vpl(int vpl) { return vpl <= 8 ? SGM_PADW : SGM_PADW_WIDE; }
constexpr int sgm_wbias_vpl(int vpl) { return vpl <= 8 ? 1024 : 2048; }   // >= the most negative window start (VPL*63 + VPL - 1 + 3)
static inline int sgm_padw(int D) { return D <= 512 ? SGM_PADW : SGM_PADW_WIDE; }   // the host's: D <= 512 runs VPL 4 or 8, above that VPL 16

struct SgmPassArgs {
	const float *C[2];    // input cost volume(s), (H,W,ds)
	const float *accin[2];// running sum read by MODE 1,2,3
	const float *accin2[2];// second partial sum read by MODE 3
	float *out[2];        // where this sweep writes
	float *out2[2];       // DUAL: where the concurrent second direction writes
	float *disp[2];       // ARGMIN output (H,W), may be null
	int drop_out[2];      // 1: this pass's stores to out[v] are dropped (nothing reads them; the arg-min is still written)
	int direction[2];
	int nvol;
	int H, W, D, ds;
	int tri;              // 1: the caller's promise about the volumes' NaN triangle (sgm_sweeps): the fused sweeps leave it alone where nothing reads it
	                      // (in the padding in front of cls0: every other field keeps its offset, and the other instances their code)
	const uint8_t *cls0;  // [4][cls_plane], plane = H*W bytes padded to a dword multiple
	int64_t cls_plane;
	const uint8_t *win;   // [2][4][H][Wm]
	int Wm;
	float P1[3], P2[3], P1a[3];  // 0: both < tau, 1: mixed, 2: both > tau ; P1a = P1 / alpha1
	int drop_h[2];        // the horizontal launch under `tri`: 1: nothing reads out[v]'s NaN triangle (the volume's final costs are dropped), it is not stored
	                      // (drop_out is set after that launch and drops whole runs.  The struct has no padding left: behind the last field, so that
	                      // every other field keeps its offset, and the other instances their code)
	float *ck[2];         // the recomputing vertical launches: volume v's checkpoint rows, (H / SGM_CK_ROWS, W, ds) -- L_down of the image rows
	                      // y % SGM_CK_ROWS == SGM_CK_ROWS - 1, written by MODE 4 and read by sgm_updown_line (behind drop_h for the same reason)
};

// The two choices of a walk's form, stated once: the host asks them (launch_pass, sgm_sweeps_ck) and so does the device where a kernel holds
// several forms (sgm_line_wide).  FAR: a volume of 2 GiB or more, 64-bit pixel addresses in every step.  Vector: 16-byte pieces -- the pixel
// stride a multiple of 4 and every volume of the call 16-byte aligned (sgm_sweeps_ck fills both entries of each array; a null out2 is aligned).
__host__ __device__ inline bool sgm_far(int H, int W, int ds) { return (int64_t)H * W * ds * 4 >= ((int64_t)1 << 31); }
__host__ __device__ inline bool sgm_vec(const SgmPassArgs &A)
{
	return (A.ds & 3) == 0 && (((uintptr_t)A.C[0] | (uintptr_t)A.C[1] | (uintptr_t)A.out[0] | (uintptr_t)A.out[1] | (uintptr_t)A.out2[0] | (uintptr_t)A.out2[1]) & 15) == 0;
}

typedef unsigned uint4v __attribute__((ext_vector_type(4)));

template <int VPL, int NACC>
struct StepData {
	float c[VPL];
	float a[NACC > 0 ? VPL : 1];
	float a2[NACC > 1 ? VPL : 1];
	unsigned pk;
	unsigned a0;   // class of the reference pixel's edge (same value in every lane)
};


// v_min_f32 / v_min3_f32 as written: fminf() through the compiler canonicalises every operand it cannot prove quiet (a v_max x, x
// each) -- no signalling NaN can reach a minimum here: the operands are results of additions, of other minima, or +INF.
__device__ __forceinline__ float vmin2(float a, float b)
{
	float r;
	asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
	return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c)
{
	float r;
	asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
	return r;
}
// min over the 64 lanes of quiet values, wave-uniform (mc::wave_min with the DPP folded into the minimum: 13 instructions
// instead of 31 -- a sweep runs one or two waves per SIMD, where every instruction is ~8 cycles of the recurrence)
__device__ __forceinline__ float wave_min_q(float v)
{
	float r;
	asm volatile("s_nop 1\n\tv_min_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
	             "s_nop 1\n\tv_min_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
	             "s_nop 1\n\tv_min_f32_dpp %1, %1, %1 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
	             "s_nop 1\n\tv_min_f32_dpp %1, %1, %1 row_mirror row_mask:0xf bank_mask:0xf\n\t"
	             "s_nop 1\n\tv_min_f32_dpp %1, %1, %1 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
	             "s_nop 1\n\tv_min_f32_dpp %1, %1, %1 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
	             "s_nop 0\n\tv_readlane_b32 %0, %1, 63"
	             : "=s"(r), "+v"(v));
	return r;
}

// One pixel's run of costs as a raw buffer: base = vol + pix*ds, num_records = the run's bytes, so that
// lanes whose disparities lie beyond the run are dropped (stores) / zero-filled (loads) by the hardware
// range check instead of by exec-masked branches -- the steady-state loop stays straight-line code and
// the compiler's s_waitcnt vmcnt(N) counts the steps in flight exactly.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pixel_rsrc(const float *base, int64_t elem_off, int bytes)
{
	return __builtin_amdgcn_make_buffer_rsrc((void *)(base + elem_off), 0, bytes, 0x00020000);
}

// What a sweep does with its directional cost L_r (val), given the running sum(s):
// MODE 0: out = 0 + L_r            (first direction: no read of the sum, folds out:zero(), main.lua:1014)
// MODE 1: out = accin + L_r        (reference-compatible accumulate, adcensus.cu:569,616)
// MODE 2: out = (accin + L_r)/4    (last direction; folds vol:copy(out):div(4), main.lua:1017,1020)
// MODE 3: out = (accin + accin2) + L_r   (third direction after a DUAL first launch)
// MODE 4 (DIRN 2 only): ck = L_r at the rows y % SGM_CK_ROWS == SGM_CK_ROWS - 1, nothing at any other row: the down recurrence on C alone, for
//   sgm_updown_line to restart from (below)
// DUAL (DIRN 0 only): waves [0,n) sweep right and write out = 0 + L_0; waves [n,2n) sweep LEFT over the same
//   lines and write out2 = L_1.  The two horizontal directions then run concurrently (twice the waves in
//   flight where a direction alone has fewer lines than the chip has SIMDs); the sum order of the
//   reference, ((0 + L_0) + L_1) + L_2) + L_3, is restored by MODE 3.
// U = steps kept in flight per wave (register ring): the scan is a strict recurrence, so memory latency is
//   covered by prefetch depth, not by occupancy.
// TRIH (the DUAL launch under A.tri; VEC and not FAR only): the horizontal sweeps leave the NaN triangle alone where nothing reads it.
//   A horizontal line crosses the triangle, so the live count is a property of the STEP: at column x, Dv(s) = min(D, x + 1) (direction -1)
//   or min(D, W - x) (direction +1), wave-uniform.  A lane's 16-byte piece that starts at or beyond Dv(s) * 4 bytes (the vertical sweeps'
//   rule: a piece that straddles Dv moves whole) gets the out-of-range offset for that step's load of C, and its c[] is set to NaN in
//   registers -- what memory holds there by the promise, so the recurrence, prev, m and every stored value are the bits of TRIH = false.
//   out2 (the second direction) and the out of a volume with A.drop_h set are not stored in those pieces either; any other out is
//   stored whole, NaNs included (exports, sub-pixel refinement and the next SGM iteration read them).  The cost: per step one scalar
//   multiply-add, compare and select per use (load, recurrence, store), and per piece a v_cmp against that scalar with one select per
//   offset and four on c[].  The per-element and the FAR instances and every launch without the promise run TRIH = false, the code as
//   it was.
template <int DIRN, int VPL, int MODE, bool ARGMIN, bool VEC, int U, bool DUAL, bool FAR, bool TRIH>
__device__ __forceinline__ void sgm_line(const SgmPassArgs &A, int wave)
{
	static_assert(!TRIH || (DIRN == 0 && DUAL && MODE == 0 && VEC && !FAR && !ARGMIN), "TRIH: the fused horizontal launch only");
	static_assert(MODE != 4 || (DIRN == 2 && VPL == 4 && VEC && !FAR && !ARGMIN && !DUAL), "MODE 4: the down checkpoint launch only");
	constexpr int NACC = (MODE == 0 || MODE == 4) ? 0 : (MODE == 3 ? 2 : 1);
	const int lane = threadIdx.x & 63;
	const int H = A.H, W = A.W, D = A.D, ds = A.ds, Wm = A.Wm;
	const int nlines = DIRN <= 1 ? H : W;
	const int nsteps = DIRN <= 1 ? W : H;
	const int nw = A.nvol * nlines;
	bool second = false;
	if (DUAL) {
		if (wave >= 2 * nw) return;
		second = wave >= nw;
		if (second) wave -= nw;
	} else if (wave >= nw) {
		return;
	}
	const int dirn = (DUAL && second) ? 1 : DIRN;
	const int v = wave / nlines;
	const int line = wave - v * nlines;
	const int direction = A.direction[v];
	const float *__restrict__ Cp = A.C[v];
	const float *__restrict__ Ain = A.accin[v];
	const float *__restrict__ Ain2 = A.accin2[v];
	float *__restrict__ Out = MODE == 4 ? A.ck[v] : ((DUAL && second) ? A.out2[v] : A.out[v]);
	float *__restrict__ Disp = A.disp[v];
	// a volume whose output nobody reads: its descriptor gets zero records, the range check drops every store (the loop is unchanged)
	const bool drop = A.drop_out[v];

	// line geometry: pixel of step s is (y0 + s*sy, x0 + s*sx)
	const int x0s = dirn == 0 ? 0 : (dirn == 1 ? W - 1 : line);
	const int y0s = dirn == 2 ? 0 : (dirn == 3 ? H - 1 : line);
	const int sx = dirn == 0 ? 1 : (dirn == 1 ? -1 : 0);
	const int sy = dirn == 2 ? 1 : (dirn == 3 ? -1 : 0);

	const int dbase = VPL * lane;
	const uint8_t *__restrict__ cls0 = A.cls0 + (int64_t)dirn * A.cls_plane;
	// window bytes: buffer base = win row + x + PADW - WBIAS (wave-uniform), per-lane constant voffset
	constexpr int WBIAS = sgm_wbias_vpl(VPL), PADW = sgm_padw_vpl(VPL);
	const uint8_t *__restrict__ win = A.win + ((int64_t)((direction > 0 ? 0 : 1) * 4 + dirn) * H) * Wm + PADW - WBIAS;
	// window start of chunk q at image column x: direction +1: x + VPL*lane + 4q ; -1: x - VPL*lane - 4q - 3
	const int woff = (direction > 0 ? dbase : -dbase - 3) + WBIAS;
	const int wq = direction > 0 ? 4 : -4;
	const int run_bytes = (VEC ? ds : D) * 4;
	// The NaN triangle (A.tri, the fused vertical sweeps only): a vertical line is one image column x, and C is NaN in that column at
	// every d >= Dv = min(D, x + 1) (left volume, direction -1) or min(D, W - x) (right volume) -- so are accin and accin2, and so
	// is what this sweep would store there.  The lanes at d >= Dv neither load nor store: they get the out-of-range offset below, the
	// recurrence gives them +INF by the select (before: vmin2(NaN, INF)), the arg-min leaves them out.  Dv is wave-uniform and
	// loop-invariant; a 16-byte piece that straddles Dv is moved whole (its upper values are NaN in memory and stay NaN).
	constexpr bool TRI = DIRN >= 2 && MODE >= 2;
	int Dv = D;
	if (TRI && A.tri) Dv = __builtin_amdgcn_readfirstlane(min(D, direction < 0 ? line + 1 : W - line));
	const unsigned live_bytes = (TRI && Dv < D) ? (unsigned)Dv * 4u : (unsigned)run_bytes;

	const float INF = __builtin_inff();
	// the nine penalties live in SGPRs for the whole sweep
	const float P1mid = A.P1[1], P2mid = A.P2[1], P1amid = A.P1a[1];
	const float P1lo = A.P1[0], P2lo = A.P2[0], P1alo = A.P1a[0];
	const float P1hi = A.P1[2], P2hi = A.P2[2], P1ahi = A.P1a[2];

	// Addressing.  A line's pixels are pix0 + s*dp (dp = +-1 or +-W).  FAR = false (every line spans < 2 GiB of a volume): one
	// descriptor per volume for the whole sweep -- base = the line's lowest-addressed pixel, num_records = the line's span --
	// and a step costs one scalar multiply-add per array: rel(s)*ds*4 goes into the instruction's scalar offset (which the
	// range check includes on this hardware: a per-pixel num_records cannot be combined with it).  The lanes beyond a pixel's
	// run carry an out-of-range offset instead (loop-invariant), so their loads still return 0 and their stores are dropped.
	// FAR = true rebuilds a 64-bit base per pixel (13 scalar instructions per array and step, a third of the loop).
	const int last = nsteps - 1;
	const int pix0 = y0s * W + x0s, dp = sy * W + sx;
	const int minpix = dp > 0 ? pix0 : pix0 + last * dp;
	const unsigned c1v = (unsigned)(dp * ds * 4);                       // modular: c0v + s*c1v is the true offset in [0, 2^31)
	const unsigned c0v = dp > 0 ? 0u : (unsigned)last * (unsigned)(-dp * ds * 4);
	const unsigned span = (unsigned)last * (unsigned)((dp > 0 ? dp : -dp) * ds * 4) + (unsigned)run_bytes;
	constexpr unsigned OOBV = 0x80000000u;                              // + any scalar offset < 2^31: beyond every span, no wrap
	const __amdgpu_buffer_rsrc_t rC = pixel_rsrc(Cp, (int64_t)minpix * ds, FAR ? 0 : span);
	const __amdgpu_buffer_rsrc_t rA = pixel_rsrc(NACC >= 1 ? Ain : Cp, (int64_t)minpix * ds, FAR ? 0 : span);
	const __amdgpu_buffer_rsrc_t rA2 = pixel_rsrc(NACC >= 2 ? Ain2 : Cp, (int64_t)minpix * ds, FAR ? 0 : span);
	// MODE 4: the checkpoint rows of this column, row s / SGM_CK_ROWS of (H / SGM_CK_ROWS, W, ds); no records where the image has no such row
	const int nck = H / SGM_CK_ROWS;
	const unsigned ck_span = nck > 0 ? (unsigned)(nck - 1) * (unsigned)(W * ds * 4) + (unsigned)run_bytes : 0u;
	const __amdgpu_buffer_rsrc_t rO = MODE == 4 ? pixel_rsrc(Out, (int64_t)line * ds, ck_span) : pixel_rsrc(Out, (int64_t)minpix * ds, (FAR || drop) ? 0 : span);
	const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void *)win, 0, H * Wm + 2 * WBIAS + 64, 0x00020000);
	const int w0 = y0s * Wm + x0s, dw = sy * Wm + sx;
	const __amdgpu_buffer_rsrc_t rCls = __builtin_amdgcn_make_buffer_rsrc((void *)cls0, 0, H * W, 0x00020000);
	const __amdgpu_buffer_rsrc_t rDisp = pixel_rsrc(ARGMIN ? Disp : Out, 0, H * W * 4);
	unsigned lane_off[VEC ? VPL / 4 : VPL];                             // byte offset of this lane's values inside a run, or OOBV
#pragma unroll
	for (int q = 0; q < (VEC ? VPL / 4 : VPL); ++q) {
		const unsigned b = (unsigned)(dbase + (VEC ? 4 * q : q)) * 4u;
		// (FAR: the per-pixel descriptor of run_bytes checks the run's end itself; OOBV lies beyond it too)
		lane_off[q] = ((FAR && !TRI) || b < live_bytes) ? b : OOBV;
	}
	const unsigned lane0_off = lane == 0 ? 0u : OOBV;
	// TRIH: the live bytes of step s's run, Dv(s) * 4 in a trimmed column and the whole run elsewhere (Dv(s) = hdv0 + s * hdv1 >= 1, scalar)
	const int hdv0 = direction < 0 ? x0s + 1 : W - x0s, hdv1 = direction < 0 ? sx : -sx;
	// whose stores leave the triangle out: the second direction's (out2) and those of a volume whose final costs are dropped; the others
	// take the same straight-line code with a count that never falls below D
	const bool trim_st = TRIH && (second || A.drop_h[v] != 0);
	const int sdv0 = trim_st ? hdv0 : D, sdv1 = trim_st ? hdv1 : 0;
	auto live_bytes_of = [&](int dv) -> unsigned { return dv < D ? (unsigned)dv * 4u : (unsigned)run_bytes; };
	auto live_at = [&](int s) -> unsigned { return live_bytes_of(hdv0 + s * hdv1); };
	// a piece's offset at a step with `lim` live bytes (lim <= run_bytes: this is lane_off[q] where lim is the whole run)
	auto piece_off = [&](int q, unsigned lim) -> unsigned {
		const unsigned b = (unsigned)(dbase + 4 * q) * 4u;
		return b < lim ? b : OOBV;
	};

	// rs: the volume's descriptor (FAR: ignored), so: the pixel's scalar byte offset (FAR: ignored); lim (TRIH): the run's live bytes
	auto load_run = [&](float (&dst)[VPL], const float *base, const __amdgpu_buffer_rsrc_t &rs, unsigned so, int64_t pix, unsigned lim = 0u) {
		const __amdgpu_buffer_rsrc_t r = FAR ? pixel_rsrc(base, pix * ds, run_bytes) : rs;
		const unsigned soff = FAR ? 0u : so;
		if (VEC) {
#pragma unroll
			for (int q = 0; q < VPL / 4; ++q) {
				const uint4v t = __builtin_amdgcn_raw_buffer_load_b128(r, TRIH ? piece_off(q, lim) : lane_off[q], soff, MC_SGM_VOL_AUX);
				dst[4 * q + 0] = __uint_as_float(t.x); dst[4 * q + 1] = __uint_as_float(t.y);
				dst[4 * q + 2] = __uint_as_float(t.z); dst[4 * q + 3] = __uint_as_float(t.w);
			}
		} else {
#pragma unroll
			for (int j = 0; j < VPL; ++j) dst[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, lane_off[j], soff, 0));
		}
	};

	auto load_step = [&](StepData<VPL, NACC> &sd, int s) {
		const unsigned so = c0v + (unsigned)s * c1v;
		const int64_t pix = FAR ? (int64_t)(y0s + s * sy) * W + (x0s + s * sx) : 0;
		load_run(sd.c, Cp, rC, so, pix, TRIH ? live_at(s) : 0u);
		if constexpr (NACC >= 1) load_run(sd.a, Ain, rA, so, pix);
		if constexpr (NACC >= 2) load_run(sd.a2, Ain2, rA2, so, pix);
		unsigned pk = 0;
		const unsigned sw = (unsigned)(w0 + s * dw);
#pragma unroll
		for (int q = 0; q < VPL / 4; ++q) pk |= (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rW, woff + q * wq, sw, 0) << (8 * q);
		sd.pk = pk;
		sd.a0 = __builtin_amdgcn_raw_buffer_load_b8(rCls, 0, (unsigned)(pix0 + s * dp), 0);  // every lane reads the same byte
	};

	auto store_step = [&](const float (&o)[VPL], int s) {
		const int64_t pix = FAR ? (int64_t)(y0s + s * sy) * W + (x0s + s * sx) : 0;
		const __amdgpu_buffer_rsrc_t r = FAR ? pixel_rsrc(Out, pix * ds, drop ? 0 : run_bytes) : rO;
		// MODE 4: a row that is no checkpoint gets the out-of-range offset, like every other suppressed store here
		const unsigned soff = MODE == 4 ? (unsigned)(s / SGM_CK_ROWS) * (unsigned)(W * ds * 4) : (FAR ? 0u : c0v + (unsigned)s * c1v);
		const bool ck_row = MODE != 4 || s % SGM_CK_ROWS == SGM_CK_ROWS - 1;
		const unsigned lim = TRIH ? live_bytes_of(sdv0 + s * sdv1) : (unsigned)run_bytes;
		if (VEC) {
#pragma unroll
			for (int q = 0; q < VPL / 4; ++q) {
				uint4v t;
				t.x = __float_as_uint(o[4 * q + 0]); t.y = __float_as_uint(o[4 * q + 1]);
				t.z = __float_as_uint(o[4 * q + 2]); t.w = __float_as_uint(o[4 * q + 3]);
				__builtin_amdgcn_raw_buffer_store_b128(t, r, TRIH ? piece_off(q, lim) : (ck_row ? lane_off[q] : OOBV), soff, MC_SGM_ST_AUX);
				if constexpr (MODE == 4) {   // the store's data registers stay untouched for two more cycles (sgm_updown_line's finish says why)
					__builtin_amdgcn_sched_barrier(0);
					asm volatile("s_nop 1");
					__builtin_amdgcn_sched_barrier(0);
				}
			}
		} else {
#pragma unroll
			for (int j = 0; j < VPL; ++j) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[j]), r, lane_off[j], soff, 0);
		}
		if (ARGMIN) {
			// torch.min(vol,2) - 1 (main.lua:1049-1050) on the finished pixel: first strict
			// minimum from +INF, NaN never wins (spatial_argmin convention, adcensus.cu:251-260)
			float best = INF;
			int bi = 0;
#pragma unroll
			for (int j = 0; j < VPL; ++j) {
				if (dbase + j < Dv && o[j] < best) {
					best = o[j];
					bi = dbase + j;
				}
			}
			const float mall = wave_min_q(best);
			const unsigned long long cand = __ballot(best == mall && best < INF);
			// branch-free: ffs = 0 when no lane holds a finite minimum (all-NaN pixel -> index 0)
			const int f = __builtin_ffsll((long long)cand);
			const int got = __builtin_amdgcn_readlane(bi, (f - 1) & 63);
			const int idx = f ? got : 0;
			// one float per pixel, the pixel in the scalar offset: only lane 0 carries an in-range offset
			__builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((float)idx), rDisp, lane0_off, (unsigned)(pix0 + s * dp) * 4u, 0);
		}
	};

	float prev[VPL];
	float m = 0.0f;
#pragma unroll
	for (int j = 0; j < VPL; ++j) prev[j] = 0.0f;

	// loop-invariant VALU operands, pinned in VGPRs (the compiler re-materialises them from SGPRs in every step otherwise)
	float P1midv = P1mid, P2midv = P2mid, P1amidv = P1amid, INFv = INF;
	asm volatile("" : "+v"(P1midv), "+v"(P2midv), "+v"(P1amidv), "+v"(INFv));
	// MODE 0 writes 0 + L_r (out:zero() then +=, main.lua:1014), its concurrent second direction L_r itself: x + (+0) and x + (-0)
	const float zadd = ((DUAL && second) || MODE == 4) ? -0.0f : 0.0f;

	// keep != nullptr: the step's outputs go there instead of to memory (the horizontal sweeps' batched stores below)
	auto process = [&](const StepData<VPL, NACC> &sd, int s, float *keep = nullptr) {
		float val[VPL], o[VPL], c[VPL];
#pragma unroll
		for (int j = 0; j < VPL; ++j) c[j] = sd.c[j];
		if (TRIH) {   // the pieces this step's load left out: NaN, as C holds there
			const unsigned lim = live_at(s);
#pragma unroll
			for (int j = 0; j < VPL; ++j) c[j] = (unsigned)(dbase + (j & ~3)) * 4u < lim ? c[j] : __builtin_nanf("");
		}
		const int a0 = __builtin_amdgcn_readfirstlane((int)sd.a0);
		const int amatch = a0 == 1 ? 3 : a0;
		// scalar selects, as written: the compiler sends a select of two float SGPRs to the VALU (two moves and a v_cndmask each)
		float P1x, P2x, P1ax = 0.0f;
		if (DIRN >= 2)
			asm("s_cmp_eq_u32 %3, 0\n\ts_cselect_b32 %0, %4, %5\n\ts_cselect_b32 %1, %6, %7\n\ts_cselect_b32 %2, %8, %9"
			    : "=s"(P1x), "=s"(P2x), "=s"(P1ax)
			    : "s"(a0), "s"(P1lo), "s"(P1hi), "s"(P2lo), "s"(P2hi), "s"(P1alo), "s"(P1ahi)
			    : "scc");
		else
			asm("s_cmp_eq_u32 %2, 0\n\ts_cselect_b32 %0, %3, %4\n\ts_cselect_b32 %1, %5, %6"
			    : "=s"(P1x), "=s"(P2x)
			    : "s"(a0), "s"(P1lo), "s"(P1hi), "s"(P2lo), "s"(P2hi)
			    : "scc");
		const float down = lane_from_below(prev[VPL - 1], INF);
		const float up = lane_from_above(prev[0], INF);
#pragma unroll
		for (int j = 0; j < VPL; ++j) {
			const int b = (sd.pk >> (2 * j)) & 3;
			const bool match = b == amatch;
			const float P2 = match ? P2x : P2midv;
			const float P1 = match ? P1x : P1midv;
			const float P1a = match ? P1ax : P1amidv;
			const float pm = j > 0 ? prev[j > 0 ? j - 1 : 0] : down;
			const float pp = j < VPL - 1 ? prev[j < VPL - 1 ? j + 1 : 0] : up;
			// adcensus.cu:607-613: min(min(min(prev, m + P2), pm + P1), pp + P1) as one v_min_f32 + v_min3_f32
			float cost;
			asm("v_min_f32 %0, %1, %2\n\tv_min3_f32 %0, %0, %3, %4"
			    : "=&v"(cost)
			    : "v"(prev[j]), "v"(m + P2), "v"(pm + (DIRN == 2 ? P1a : P1)), "v"(pp + (DIRN == 3 ? P1a : P1)));
			val[j] = (c[j] + cost) - m;  // adcensus.cu:615
		}
		if (s == 0) {   // border branch, adcensus.cu:567-572: L_r = C.  A uniform branch taken once per line, not VPL selects per step
			asm volatile("; border step");
#pragma unroll
			for (int j = 0; j < VPL; ++j) val[j] = c[j];
		}
		float q[VPL];
#pragma unroll
		for (int j = 0; j < VPL; ++j) {
			if (MODE == 0 || MODE == 4) o[j] = val[j] + zadd;
			else if (MODE == 1) o[j] = sd.a[j] + val[j];
			else if (MODE == 2) o[j] = (sd.a[j] + val[j]) * 0.25f;
			else o[j] = (sd.a[j] + sd.a2[j]) + val[j];
			q[j] = vmin2(val[j], INFv);                       // NaN -> +INF: fminf semantics of the recurrence
		}
#pragma unroll
		for (int j = 0; j < VPL; ++j) prev[j] = (dbase + j < Dv) ? q[j] : INFv;
		float nm = vmin3(prev[0], prev[1], prev[2]);
#pragma unroll
		for (int j = 3; j < VPL; j += 2) nm = j + 1 < VPL ? vmin3(nm, prev[j], prev[j + 1]) : vmin2(nm, prev[j]);
		m = wave_min_q(nm);
		if (keep) {
#pragma unroll
			for (int j = 0; j < VPL; ++j) keep[j] = o[j];
		} else {
			store_step(o, s);
		}
	};

	StepData<VPL, NACC> ring[U];
#pragma unroll
	for (int u = 0; u < U; ++u) load_step(ring[u], u < last ? u : last);

	int g = 0;
	// steady state: straight-line code, every slot is consumed and immediately refilled U steps ahead
	// (refills past the end of the line re-read its last pixel; they are never consumed)
	// Horizontal sweeps (SB / LB > 1): consecutive steps of a line are consecutive pixels, i.e. CONTIGUOUS memory -- the outputs of SB steps
	// are stored together (SB runs back to back: one piece of SB x ds floats instead of SB pieces a step's recurrence apart) and the refills of LB slots requested together
	// (A/B on one box, profiles/r05_ab_sgm_batched.txt, the horizontal launch at KITTI size: 772 us at 1 / 1, 761 at SB 4, 751 at LB 4, 746 at 4 / 4, 751 at 8 / 8; 1000 x 1500: 2 470 -> 2 462)
	constexpr int SB = (DIRN <= 1 && !ARGMIN && U % 4 == 0) ? 4 : 1;
	constexpr int LB = (DIRN <= 1 && U % 4 == 0) ? 4 : 1;
	float obuf[SB][VPL];
	for (; g + U <= nsteps; g += U) {
#pragma unroll
		for (int u = 0; u < U; ++u) {
			const int s = g + u;
			// keep each step's work behind its own s_waitcnt: without the barrier the machine scheduler hoists the
			// recurrence-independent adds of ALL ring slots to the loop head, i.e. waits for every prefetch at once
			__builtin_amdgcn_sched_barrier(0);
			if (SB > 1) {
				process(ring[u], s, obuf[u % SB]);
				if (u % SB == SB - 1) {
#pragma unroll
					for (int k = 0; k < SB; ++k) store_step(obuf[k], s - (SB - 1) + k);
				}
			} else {
				process(ring[u], s);
			}
			if (u % LB == LB - 1) {
#pragma unroll
				for (int k = 0; k < LB; ++k) {
					const int sn = s - (LB - 1) + k + U;
					load_step(ring[u - (LB - 1) + k], sn < last ? sn : last);
				}
			}
		}
	}
#pragma unroll
	for (int u = 0; u < U; ++u) {
		if (g + u < nsteps) process(ring[u], g + u);
	}
}

// The down and the up sweep of the fused schedule in one walk (VPL = 4, VEC, not FAR): L_down depends on C and on its own previous row only,
// so it is not carried through memory as (out + out2) + L_down (MODE 3's volume of stores, MODE 2's volume of loads) but recomputed where it
// is consumed.  A wave owns one column and walks its blocks of B = SGM_CK_ROWS rows from the bottom block to the top one.  Per block:
//   (a) the down recurrence's state above the block: prev and m out of MODE 4's checkpoint row (block 0: the border step, L = C);
//   (b) the down recurrence over the block's rows, ascending; val_down and the rows of C stay in registers;
//   (c) the up recurrence over the same rows, descending, its state carried from block to block in registers; each row stores
//       o = (((a + a2) + val_down) + val_up) * 0.25f -- MODE 3 followed by MODE 2, operation for operation -- and its arg-min.
// Loads are never guarded (a row beyond the image re-reads an edge row and is not consumed): the rows of a and a2 are requested during (b),
// the next block's rows of C and its checkpoint during (c), each B steps ahead of its use, into the other of two sets of registers (`cur` /
// `nxt` swap from block to block: no copy, so no wait for a load in front of its use).  Only the bottom block can be short; it takes the
// guarded form of the block (FULL = false), every other block is straight-line code.
// drop_out, tri / Dv, disp and the edge classes are sgm_line's.
template <int B, bool ARGMIN>
__device__ __forceinline__ void sgm_updown_line(const SgmPassArgs &A, int wave)
{
	constexpr int VPL = 4;
	const int lane = threadIdx.x & 63;
	const int H = A.H, W = A.W, D = A.D, ds = A.ds, Wm = A.Wm;
	if (wave >= A.nvol * W) return;
	const int v = wave / W;
	const int x = wave - v * W;
	const int direction = A.direction[v];
	const bool drop = A.drop_out[v];
	const int dbase = VPL * lane;
	constexpr int WBIAS = 1024;
	const int woff = (direction > 0 ? dbase : -dbase - 3) + WBIAS;
	const int run_bytes = ds * 4;
	int Dv = D;
	if (A.tri) Dv = __builtin_amdgcn_readfirstlane(min(D, direction < 0 ? x + 1 : W - x));
	const unsigned live_bytes = Dv < D ? (unsigned)Dv * 4u : (unsigned)run_bytes;
	constexpr unsigned OOBV = 0x80000000u;
	const unsigned lane_off = (unsigned)dbase * 4u < live_bytes ? (unsigned)dbase * 4u : OOBV;
	const unsigned lane0_off = lane == 0 ? 0u : OOBV;

	const float INF = __builtin_inff();
	const float P1mid = A.P1[1], P2mid = A.P2[1], P1amid = A.P1a[1];
	auto sreg = [](float f) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(f))); };
	const float P1lo = sreg(A.P1[0]), P2lo = sreg(A.P2[0]), P1alo = sreg(A.P1a[0]);
	const float P1hi = sreg(A.P1[2]), P2hi = sreg(A.P2[2]), P1ahi = sreg(A.P1a[2]);
	float P1midv = P1mid, P2midv = P2mid, P1amidv = P1amid, INFv = INF;
	asm volatile("" : "+v"(P1midv), "+v"(P2midv), "+v"(P1amidv), "+v"(INFv));

	// one descriptor per array for the whole column: base = the column's top pixel, the row in the scalar offset (sgm_line, FAR = false)
	const unsigned row_bytes = (unsigned)(W * ds * 4);
	const unsigned span = (unsigned)(H - 1) * row_bytes + (unsigned)run_bytes;
	const int nck = H / B;
	const unsigned ck_span = nck > 0 ? (unsigned)(nck - 1) * row_bytes + (unsigned)run_bytes : 0u;
	const __amdgpu_buffer_rsrc_t rC = pixel_rsrc(A.C[v], (int64_t)x * ds, span);
	const __amdgpu_buffer_rsrc_t rA = pixel_rsrc(A.accin[v], (int64_t)x * ds, span);
	const __amdgpu_buffer_rsrc_t rA2 = pixel_rsrc(A.accin2[v], (int64_t)x * ds, span);
	// (the sweep works in place: out is accin, stored through rA; a volume whose output nobody reads stores at the out-of-range offset)
	const unsigned store_off = drop ? OOBV : lane_off;
	const __amdgpu_buffer_rsrc_t rK = pixel_rsrc(A.ck[v], (int64_t)x * ds, ck_span);
	// the window rows and the class planes of directions 2 and 3 lie one behind the other: one descriptor each, the up direction's at `wup` / `cup`
	const int wrows = (direction > 0 ? 0 : 1) * 4 + 2;
	const unsigned wup = (unsigned)(H * Wm), cup = (unsigned)A.cls_plane;
	const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void *)(A.win + ((int64_t)wrows * H) * Wm + SGM_PADW - WBIAS), 0, 2 * H * Wm + 2 * WBIAS + 64, 0x00020000);
	const __amdgpu_buffer_rsrc_t rCls = __builtin_amdgcn_make_buffer_rsrc((void *)(A.cls0 + 2 * A.cls_plane), 0, (int)cup + H * W, 0x00020000);
	const __amdgpu_buffer_rsrc_t rDisp = pixel_rsrc(ARGMIN ? A.disp[v] : A.out[v], 0, H * W * 4);

	struct RowIn { float c[VPL]; unsigned pk, a0; };            // a row as (b) reads it; (c) reads c[] again
	struct RowAcc { float a[VPL], a2[VPL]; unsigned pk, a0; };  // what (c) reads besides
	auto load4 = [&](float (&dst)[VPL], const __amdgpu_buffer_rsrc_t &r, unsigned so) {
		const uint4v t = __builtin_amdgcn_raw_buffer_load_b128(r, lane_off, so, MC_SGM_VOL_AUX);
		dst[0] = __uint_as_float(t.x); dst[1] = __uint_as_float(t.y); dst[2] = __uint_as_float(t.z); dst[3] = __uint_as_float(t.w);
	};
	auto clamp_row = [&](int y) { return y < 0 ? 0 : (y > H - 1 ? H - 1 : y); };
	auto load_in = [&](RowIn &ri, int y) {
		y = clamp_row(y);
		load4(ri.c, rC, (unsigned)y * row_bytes);
		ri.pk = __builtin_amdgcn_raw_buffer_load_b8(rW, woff, (unsigned)(y * Wm + x), 0);
		ri.a0 = __builtin_amdgcn_raw_buffer_load_b8(rCls, 0, (unsigned)(y * W + x), 0);
	};
	auto load_acc = [&](RowAcc &ra, int y) {
		y = clamp_row(y);
		load4(ra.a, rA, (unsigned)y * row_bytes);
		load4(ra.a2, rA2, (unsigned)y * row_bytes);
		ra.pk = __builtin_amdgcn_raw_buffer_load_b8(rW, woff, wup + (unsigned)(y * Wm + x), 0);
		ra.a0 = __builtin_amdgcn_raw_buffer_load_b8(rCls, 0, cup + (unsigned)(y * W + x), 0);
	};
	// the checkpoint above block k: image row k * B - 1, row k - 1 of the checkpoint rows (block 0 has none: the load is not consumed)
	auto load_ck = [&](float (&dst)[VPL], int k) { load4(dst, rK, (unsigned)(k > 1 ? k - 1 : 0) * row_bytes); };

	// prev and m from a row's L_r, as sgm_line's process() leaves them
	auto state_of = [&](const float (&val)[VPL], float (&prev)[VPL], float &m) {
#pragma unroll
		for (int j = 0; j < VPL; ++j) prev[j] = (dbase + j < Dv) ? vmin2(val[j], INFv) : INFv;
		m = wave_min_q(vmin2(vmin3(prev[0], prev[1], prev[2]), prev[3]));
	};
	// one step of the recurrence in direction down (dn = true) or up, sgm_line's process() operation for operation
	auto recur = [&](auto dn, float (&prev)[VPL], float &m, const float (&c)[VPL], unsigned pk, unsigned a0v, bool border, float (&val)[VPL]) {
		constexpr bool DN = decltype(dn)::value;
		const int a0 = __builtin_amdgcn_readfirstlane((int)a0v);
		const int amatch = a0 == 1 ? 3 : a0;
		float P1x, P2x, P1ax;
		asm("s_cmp_eq_u32 %3, 0\n\ts_cselect_b32 %0, %4, %5\n\ts_cselect_b32 %1, %6, %7\n\ts_cselect_b32 %2, %8, %9"
		    : "=s"(P1x), "=s"(P2x), "=s"(P1ax)
		    : "s"(a0), "s"(P1lo), "s"(P1hi), "s"(P2lo), "s"(P2hi), "s"(P1alo), "s"(P1ahi)
		    : "scc");
		const float down = lane_from_below(prev[VPL - 1], INF);
		const float up = lane_from_above(prev[0], INF);
#pragma unroll
		for (int j = 0; j < VPL; ++j) {
			const int b = (pk >> (2 * j)) & 3;
			const bool match = b == amatch;
			const float P2 = match ? P2x : P2midv;
			const float P1 = match ? P1x : P1midv;
			const float P1a = match ? P1ax : P1amidv;
			const float pm = j > 0 ? prev[j > 0 ? j - 1 : 0] : down;
			const float pp = j < VPL - 1 ? prev[j < VPL - 1 ? j + 1 : 0] : up;
			float cost;
			asm("v_min_f32 %0, %1, %2\n\tv_min3_f32 %0, %0, %3, %4"
			    : "=&v"(cost)
			    : "v"(prev[j]), "v"(m + P2), "v"(pm + (DN ? P1a : P1)), "v"(pp + (DN ? P1 : P1a)));
			val[j] = (c[j] + cost) - m;
		}
		if (border) {
			asm volatile("; border step");
#pragma unroll
			for (int j = 0; j < VPL; ++j) val[j] = c[j];
		}
		state_of(val, prev, m);
	};
	auto finish = [&](const float (&o)[VPL], int y) {
		uint4v t;
		t.x = __float_as_uint(o[0]); t.y = __float_as_uint(o[1]); t.z = __float_as_uint(o[2]); t.w = __float_as_uint(o[3]);
		__builtin_amdgcn_raw_buffer_store_b128(t, rA, store_off, (unsigned)y * row_bytes, MC_SGM_ST_AUX);
		// Wait states behind the 128-bit store: the arg-min below starts with `best = o[0] < INF ? o[0] : INF` in o[0]'s own register, and the compiler
		// puts that v_cndmask directly behind the store (it counts a store with an SGPR offset as exempt from the store-data hazard).  On MI355X the store
		// then sometimes sent the overwritten register: +INF instead of NaN at d % 4 == 0, wherever a lane stores a NaN in its first element (raw
		// volumes' triangle; never under the promise, where such lanes do not store), in the first rows a late wave walks, different from run to run.
		// (the barriers keep the scheduler from moving that VALU instruction in front of the s_nop)
		__builtin_amdgcn_sched_barrier(0);
		asm volatile("s_nop 1");
		__builtin_amdgcn_sched_barrier(0);
		if (ARGMIN) {   // sgm_line's
			float best = INF;
			int bi = 0;
#pragma unroll
			for (int j = 0; j < VPL; ++j) {
				if (dbase + j < Dv && o[j] < best) {
					best = o[j];
					bi = dbase + j;
				}
			}
			const float mall = wave_min_q(best);
			const unsigned long long cand = __ballot(best == mall && best < INF);
			const int f = __builtin_ffsll((long long)cand);
			const int got = __builtin_amdgcn_readlane(bi, (f - 1) & 63);
			const int idx = f ? got : 0;
			__builtin_amdgcn_raw_buffer_store_b32(__float_as_uint((float)idx), rDisp, lane0_off, (unsigned)(y * W + x) * 4u, 0);
		}
	};

	float prevd[VPL], prevu[VPL], ckv[VPL], vd[B][VPL];
	float md = 0.0f, mu = 0.0f;
#pragma unroll
	for (int j = 0; j < VPL; ++j) prevd[j] = prevu[j] = 0.0f;
	RowIn in0[B], in1[B];
	RowAcc acc[B];

	auto block = [&](auto full, int k, RowIn (&cur)[B], RowIn (&nxt)[B]) {
		constexpr bool FULL = decltype(full)::value;
		const int y0 = k * B;
		const int n = FULL ? B : H - y0;   // rows of this block, 1 .. B
		if (!FULL) {
#pragma unroll
			for (int r = B - 1; r >= 0; --r) load_acc(acc[r], y0 + r);
		}
		if (k > 0) state_of(ckv, prevd, md);   // (a)
#pragma unroll
		for (int r = 0; r < B; ++r) {          // (b)
			if (FULL || r < n) {
				__builtin_amdgcn_sched_barrier(0);
				recur(std::true_type(), prevd, md, cur[r].c, cur[r].pk, cur[r].a0, y0 + r == 0, vd[r]);
			}
			if (FULL) load_acc(acc[B - 1 - r], y0 + B - 1 - r);
		}
#pragma unroll
		for (int t = 0; t < B; ++t) {          // (c)
			const int r = B - 1 - t;
			if (FULL || r < n) {
				__builtin_amdgcn_sched_barrier(0);
				float vu[VPL], o[VPL];
				recur(std::false_type(), prevu, mu, cur[r].c, acc[r].pk, acc[r].a0, y0 + r == H - 1, vu);
#pragma unroll
				for (int j = 0; j < VPL; ++j) o[j] = (((acc[r].a[j] + acc[r].a2[j]) + vd[r][j]) + vu[j]) * 0.25f;
				finish(o, y0 + r);
			}
			if (t == 0) load_ck(ckv, k - 1);
			load_in(nxt[t], y0 - B + t);
		}
	};

	int k = (H - 1) / B;
#pragma unroll
	for (int r = 0; r < B; ++r) load_in(in0[r], k * B + r);
	load_ck(ckv, k);
	block(std::false_type(), k, in0, in1);
	for (--k; k >= 1; k -= 2) {
		block(std::true_type(), k, in1, in0);
		block(std::true_type(), k - 1, in0, in1);
	}
	if (k == 0) block(std::true_type(), 0, in1, in0);
}

template <int B, bool ARGMIN>
__global__ void __launch_bounds__(256) sgm_updown_kernel(const SgmPassArgs A)
{
	sgm_updown_line<B, ARGMIN>(A, __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)));
}

constexpr int SGM_U_CK = 16;     // steps in flight of the checkpoint launch (MODE 4): a slot is a run of C and two class bytes

// D in 513..1024: the line walk at VPL = 16.  Its forms are no kernels of their own: the library's kernel set is the one tests/kernel_inventory.txt
// lists, so each lives inside the kernel that runs the same sweep at VPL = 8 on aligned volumes below 2 GiB with 8 steps in flight (below) -- an
// instance that already takes more than 256 registers, i.e. one wave per SIMD (the fused horizontal one: under 256 with either walk), so that the
// wider walk costs the D <= 512 path one uniform compare per wave and nothing else.  Which form runs is decided here as launch_pass decides it for
// the narrower walks, by the same two functions (sgm_far, sgm_vec): FAR for a volume of 2 GiB, per element (MODE 1 only) without alignment.
// Steps in flight: a step is 18 + 16 * NACC registers (StepData<16, NACC>); sized so that no form has scratch and none lifts its host kernel
// out of its register class.  Not tuned.
constexpr int SGM_U_WIDE = 4, SGM_U_WIDE_ELEM = 2;

template <int DIRN, int MODE, bool ARGMIN, bool DUAL>
__device__ __forceinline__ void sgm_line_wide(const SgmPassArgs &A, int wave)
{
	const bool far = sgm_far(A.H, A.W, A.ds);
	if constexpr (MODE == 1) {   // mc_sgm2, the caller's volumes; the fused modes run on aligned volumes only (sgm_sweeps_ck requires it)
		if (!sgm_vec(A)) {
			if (far) sgm_line<DIRN, 16, MODE, ARGMIN, false, SGM_U_WIDE_ELEM, DUAL, true, false>(A, wave);
			else sgm_line<DIRN, 16, MODE, ARGMIN, false, SGM_U_WIDE_ELEM, DUAL, false, false>(A, wave);
			return;
		}
	}
	// (no trimmed form of the horizontal launch at 16: it runs without the promise, which gives the same bits by sgm_sweeps' contract)
	if (far) sgm_line<DIRN, 16, MODE, ARGMIN, true, SGM_U_WIDE, DUAL, true, false>(A, wave);
	else sgm_line<DIRN, 16, MODE, ARGMIN, true, SGM_U_WIDE, DUAL, false, false>(A, wave);
}

template <int DIRN, int VPL, int MODE, bool ARGMIN, bool VEC, int U, bool DUAL, bool FAR>
__global__ void __launch_bounds__(256) sgm_pass_kernel(const SgmPassArgs A)
{
	const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
	if constexpr (VPL == 8 && VEC && U == 8 && !FAR && MODE != 4) {
		if (A.D > 512) {
			sgm_line_wide<DIRN, MODE, ARGMIN, DUAL>(A, wave);
			return;
		}
	}
	// the fused horizontal launch holds both forms of its line walk and takes the trimmed one under the caller's promise (one uniform branch
	// per wave); without it, and in every other instance, the walk is the code it was
	if constexpr (DIRN == 0 && DUAL && MODE == 0 && VEC && !FAR && !ARGMIN) {
		if (A.tri) {
			sgm_line<DIRN, VPL, MODE, ARGMIN, VEC, U, DUAL, FAR, true>(A, wave);
			return;
		}
	}
	sgm_line<DIRN, VPL, MODE, ARGMIN, VEC, U, DUAL, FAR, false>(A, wave);
}

}  // namespace mc

// libmcsgmrecompute.so (sgm_recompute.hip): launches one of the recomputing vertical kernels on A -- which 0: the checkpoint launch (MODE 4),
// 1: sgm_updown_kernel without the arg-min, 2: with it.  Returns 0, or MC_EINVAL where `bytes` is not this build's sizeof(SgmPassArgs) or
// `which` is none of the three; the caller asks check_launch about the launch itself.
extern "C" int mc_sgm_recompute_launch(const mc::SgmPassArgs *A, size_t bytes, int which, hipStream_t st);
