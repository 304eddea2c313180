// Host check of the fused SGM schedule's vertical launches (mc-cnn_amd/csrc/sgm.hip: sgm_sweeps; predict.hip: make_plan's checkpoint slots).
// tests/test_sgm_vertical_host.py builds this file -- which includes sgm.hip and sgm_recompute.hip themselves, so that it can name the kernel instances -- with the host
// side of predict.hip and error.hip, with the address and undefined-behaviour sanitizers, and runs the program: no GPU and no HIP runtime is
// involved.  A kernel launch arrives at the hipLaunchKernel stub below, which writes the stream, the kernel's kind and its SgmPassArgs into a
// log; hipPeekAtLastError (check_launch) can be told to fail at its n-th call.  Every launcher of the other units is a stub that logs its name.
#include "../mc-cnn_amd/csrc/sgm.hip"
#include "../mc-cnn_amd/csrc/sgm_recompute.hip"   // (libmcsgmrecompute.so's unit: the two recomputing kernels and their launcher)

#include <string.h>

#include <string>

using namespace mc;

// ---- the log -------------------------------------------------------------------------------------------------------------------
enum Kind { K_OTHER, K_PREP, K_H, K_H8, K_HFAR, K_DOWN, K_DOWN8, K_DOWNFAR, K_UP, K_UP8, K_UPFAR, K_CK, K_UPDOWN };
struct Entry { const void *stream; std::string what; Kind kind; bool argmin; SgmPassArgs A; unsigned grid; };
static std::vector<Entry> g_log;
static int g_peeks = 0, g_fail_at = -1;   // the g_fail_at-th check_launch of a run fails (0-based)

static int note(const void *stream, const std::string &what)
{
	Entry e;
	memset(&e.A, 0, sizeof e.A);
	e.stream = stream; e.what = what; e.kind = K_OTHER; e.argmin = false; e.grid = 0;
	g_log.push_back(e);
	return 0;
}

struct Inst { const void *fn; Kind kind; bool argmin; };
#define PASS(...) (const void *)sgm_pass_kernel<__VA_ARGS__>
static const std::vector<Inst> &instances()
{
	static const std::vector<Inst> t = {
		{(const void *)sgm_prep_kernel, K_PREP, false},
		{PASS(0, 4, 0, false, true, SGM_U_H, true, false), K_H, false},
		{PASS(0, 8, 0, false, true, 8, true, false), K_H8, false},
		{PASS(0, 4, 0, false, true, 4, true, true), K_HFAR, false},
		{PASS(2, 4, 3, false, true, SGM_U_DOWN, false, false), K_DOWN, false},
		{PASS(2, 8, 3, false, true, 8, false, false), K_DOWN8, false},
		{PASS(2, 4, 3, false, true, 4, false, true), K_DOWNFAR, false},
		{PASS(3, 4, 2, false, true, SGM_U_UP, false, false), K_UP, false},
		{PASS(3, 4, 2, true, true, SGM_U_UP, false, false), K_UP, true},
		{PASS(3, 8, 2, false, true, 8, false, false), K_UP8, false},
		{PASS(3, 8, 2, true, true, 8, false, false), K_UP8, true},
		{PASS(3, 4, 2, false, true, 4, false, true), K_UPFAR, false},
		{PASS(3, 4, 2, true, true, 4, false, true), K_UPFAR, true},
		{PASS(2, 4, 4, false, true, SGM_U_CK, false, false), K_CK, false},
		{(const void *)sgm_updown_kernel<SGM_CK_ROWS, false>, K_UPDOWN, false},
		{(const void *)sgm_updown_kernel<SGM_CK_ROWS, true>, K_UPDOWN, true},
	};
	return t;
}

// ---- HIP stubs -----------------------------------------------------------------------------------------------------------------
// (an executable's own definitions come before those of any shared library the compiler driver links)
static thread_local struct { dim3 grid, block; size_t shmem; hipStream_t st; } t_cfg;
extern "C" {
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t st) { t_cfg = {grid, block, shmem, st}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *st)
{
	*grid = t_cfg.grid; *block = t_cfg.block; *shmem = t_cfg.shmem; *st = t_cfg.st;
	return hipSuccess;
}
hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t, hipStream_t st)
{
	Entry e;
	memset(&e.A, 0, sizeof e.A);
	e.stream = st; e.what = "kernel"; e.kind = K_OTHER; e.argmin = false; e.grid = grid.x;
	for (const Inst &i : instances())
		if (i.fn == fn) { e.kind = i.kind; e.argmin = i.argmin; }
	if (e.kind != K_OTHER && e.kind != K_PREP) memcpy((void *)&e.A, args[0], sizeof e.A);
	if (block.x != 256) e.kind = K_OTHER;
	g_log.push_back(e);
	return hipSuccess;
}
// what a unit with kernels does at start-up and exit: nothing to register them with
void **__hipRegisterFatBinary(const void *) { static void *handle; return &handle; }
void __hipRegisterFunction(void **, const void *, char *, const char *, unsigned, void *, void *, void *, void *, int *) {}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void **) {}
hipError_t hipPeekAtLastError() { return g_peeks++ == g_fail_at ? hipErrorLaunchFailure : hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }
hipError_t hipMemsetAsync(void *, int, size_t, hipStream_t) { return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub error"; }
hipError_t hipMalloc(void **p, size_t n) { static float table[4096]; *p = n <= sizeof table ? table : nullptr; return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void *) { return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { *s = (hipStream_t)malloc(1); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { free(s); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = (hipEvent_t)malloc(1); return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) { *e = (hipEvent_t)malloc(1); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { free(e); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t s) { note(s, "record"); return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t, unsigned) { note(s, "wait"); return hipSuccess; }
}

// ---- launcher stubs of the other units -----------------------------------------------------------------------------------------
namespace mc {
size_t cbca_scratch_bytes(int H, int W) { return align_up((size_t)H * W * 4, 256); }   // (a multiple of 256, as the real one: make_plan adds it as it is)
size_t cbca_plan_bytes(int D, int H, int W) { return (size_t)D * H * W * 4; }
bool packed_dims_ok(int, int) { return true; }
bool cbca_lean_fits(int, int, int, size_t, bool, int) { return false; }
int fill_nan(float *, int64_t, hipStream_t s) { return note(s, "fill_nan"); }
int scale(const float *, float *, int64_t, float, hipStream_t s) { return note(s, "scale"); }
int transpose(const float *, float *, int64_t, int64_t, int64_t, int64_t, float, hipStream_t s, int) { return note(s, "transpose"); }
int fix_border(float *, int, int, int, int, int, hipStream_t s) { return note(s, "fix_border"); }
int argmin_dhw(const float *, float *, int, int, int, int, hipStream_t s) { return note(s, "argmin"); }
int outlier_detection(const float *, const float *, float *, int, int, int, hipStream_t s) { return note(s, "outlier_detection"); }
int interpolate_occlusion(const float *, const float *, float *, int, int, hipStream_t s, unsigned *) { return note(s, "interpolate_occlusion"); }
int interpolate_mismatch(const float *, const float *, float *, int, int, hipStream_t s, const unsigned *) { return note(s, "interpolate_mismatch"); }
int subpixel(const float *, const float *, float *, int, int, int, int64_t, int64_t, hipStream_t s) { return note(s, "subpixel"); }
int median2d(const float *, float *, int, int, int, hipStream_t s) { return note(s, "median2d"); }
int mean2d(const float *, const float *, float *, int, int, int, float, hipStream_t s) { return note(s, "mean2d"); }
int stereo_join_dhw(const float *, const float *, float *, float *, int, int, int, int, hipStream_t s) { return note(s, "stereo_join_dhw"); }
int stereo_join_hwd(const float *, const float *, float *, float *, int, int, int, int, int, int, hipStream_t s, int) { return note(s, "stereo_join_hwd"); }
int cross(const float *, float *, int, int, int, float, hipStream_t s) { return note(s, "cross"); }
int cbca(const float *, const float *, const float *, float *, int, int, int, int, hipStream_t s) { return note(s, "cbca"); }
int cbca_pack(const float *, const float *, void *, int, int, hipStream_t s) { return note(s, "cbca_pack"); }
int cbca_by_arms(const void *, const float *, float *, int, int, int, int, int, hipStream_t s, const CbcaCfg &) { return note(s, "cbca_by_arms"); }
int cbca_classify(const void *, void *, size_t, int, int, int, int, int, int, int, hipStream_t s, bool, float) { return note(s, "cbca_classify"); }
int cbca_lean2x(const void *, const void *, size_t, const float *, float *, int, int, int, int, int, hipStream_t s, const CbcaCfg &) { return note(s, "cbca_lean2x"); }
}  // namespace mc

// ---- the checks ----------------------------------------------------------------------------------------------------------------
static int g_failed = 0, g_checked = 0;
#define CHECK(cond) do { ++g_checked; if (!(cond)) { ++g_failed; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

static std::vector<Entry> take_log() { std::vector<Entry> l; l.swap(g_log); g_peeks = 0; return l; }
static std::vector<Entry> kernels_on(const std::vector<Entry> &l, const void *st)
{
	std::vector<Entry> k;
	for (const Entry &e : l) if (e.stream == st && e.what == "kernel" && e.kind != K_PREP) k.push_back(e);
	return k;
}

// sgm_sweeps itself on made-up addresses (nothing is dereferenced: every launch is a stub)
struct Sweep {
	int nvol = 2, H = 9, W = 40, D = 20, ds = 20;
	int direction[2] = {-1, 1};
	unsigned drop_final = 2;
	bool tri = true, argmin = true, slots = true;
	float *ck0 = (float *)0x8000000, *ck1 = (float *)0x9000000;
	char *maps = (char *)0x10000000;
	hipStream_t st = (hipStream_t)0x1000;
	int run()
	{
		const float *C[2] = {(const float *)0x20000000, (const float *)0x30000000};
		float *out[2] = {(float *)0x40000000, (float *)0x50000000}, *out2[2] = {(float *)0x60000000, (float *)0x70000000};
		float *disp[2] = {(float *)0x1000000, (float *)0x2000000};
		float *ck[2] = {ck0, ck1};
		if (!slots) return sgm_sweeps(C, out, out2, argmin ? disp : nullptr, direction, nvol, H, W, D, ds, maps, 4, 55.72f, 1.5f, 3, 2.5f, true, drop_final, tri, st);
		return sgm_sweeps_ck(C, out, out2, argmin ? disp : nullptr, direction, nvol, H, W, D, ds, maps, 4, 55.72f, 1.5f, 3, 2.5f, true, drop_final, tri, ck, st);
	}
};

// the recomputing form's three launches: order, grids, checkpoint slots, and the drop of a volume's final costs at the last launch only
static void check_recompute_log(const std::vector<Entry> &l, const Sweep &s)
{
	CHECK(l.size() == 3);
	if (l.size() != 3) return;
	CHECK(l[0].kind == K_H && l[1].kind == K_CK && l[2].kind == K_UPDOWN && l[2].argmin == s.argmin);
	CHECK(l[0].grid == cdiv(2 * s.nvol * s.H, 4) && l[1].grid == cdiv(s.nvol * s.W, 4) && l[2].grid == l[1].grid);
	for (const Entry &e : l) CHECK(e.stream == s.st && e.A.nvol == s.nvol && e.A.H == s.H && e.A.W == s.W && e.A.D == s.D && e.A.ds == s.ds && e.A.tri == (s.tri ? 1 : 0));
	for (int v = 0; v < s.nvol; ++v) {
		float *want = v == 0 ? s.ck0 : s.ck1;
		CHECK(l[1].A.ck[v] == want && l[2].A.ck[v] == want);
		CHECK(l[0].A.drop_out[v] == 0 && l[1].A.drop_out[v] == 0 && l[2].A.drop_out[v] == (int)((s.drop_final >> v) & 1));
		CHECK(l[2].A.accin[v] == l[2].A.out[v] && l[2].A.accin2[v] == l[0].A.out2[v] && l[1].A.C[v] == l[2].A.C[v]);
	}
}

static mc_params kitti_fast()
{
	mc_params p;
	memset(&p, 0, sizeof p);
	p.pi1 = 4; p.pi2 = 55.72f; p.sgm_i = 1; p.sgm_q1 = 3; p.sgm_q2 = 2.5f; p.alpha1 = 1.5f; p.tau_so = 0.02f;
	p.blur_sigma = 7.74; p.blur_t = 5; p.lr_check = 1; p.border_n = 4; p.median_k = 5;
	return p;
}

struct Area { const char *name; const char *lo; size_t bytes; };

int main()
{
	CHECK(sgm_vertical() == 2);               // the default
	CHECK(sgm_vertical(7) == 2 && sgm_vertical(-3) == 2);   // not a setting: ignored

	// ---- sgm_sweeps: horizontal, checkpoints, recomputing walk -- for a pair, for each volume alone (the two lanes), with and without arg-min ----
	for (int variant = 0; variant < 8; ++variant) {
		Sweep s;
		s.argmin = variant & 1;
		if (variant & 2) { s.nvol = 1; s.drop_final = 0; }                                           // the left lane
		if (variant & 4) { s.nvol = 1; s.direction[0] = 1; s.drop_final = (variant & 2) ? 0 : 1; }   // the right lane, its final costs dropped or kept
		if (!s.argmin) s.drop_final = 0;
		CHECK(s.run() == 0);
		check_recompute_log(take_log(), s);
	}
	// the shapes of the GPU tests, and one of KITTI's size
	for (int H : {1, 2, 7, 8, 9, 16, 17, 29, 370})
		for (int W : {20, 36, 70, 1226}) {
			Sweep s;
			s.H = H; s.W = W; s.D = W == 1226 ? 228 : 35; s.ds = (s.D + 3) / 4 * 4;
			CHECK(s.run() == 0);
			check_recompute_log(take_log(), s);
			// what the checkpoint launch can write: row H / B - 1 of the last column ends inside the slot
			const size_t nck = H / SGM_CK_ROWS;
			if (nck) CHECK(((nck - 1) * W + (W - 1) + 1) * s.ds * sizeof(float) <= sgm_ck_bytes(H, W, s.ds));
		}

	// ---- the shapes the recomputing form does not cover keep the down and the up sweep ----
	{
		Sweep s;
		s.D = 260; s.ds = 260; s.W = 300;                       // 8 disparities per lane
		CHECK(s.run() == 0);
		auto l = take_log();
		CHECK(l.size() == 3 && l[0].kind == K_H8 && l[1].kind == K_DOWN8 && l[2].kind == K_UP8 && l[2].argmin);
		CHECK(l[1].A.drop_out[1] == 0 && l[2].A.drop_out[1] == 1 && l[2].A.drop_out[0] == 0);
		Sweep f;
		f.H = 1100; f.W = 2000; f.D = 256; f.ds = 256;          // a volume of 2 GiB or more
		CHECK(f.run() == 0);
		l = take_log();
		CHECK(l.size() == 3 && l[0].kind == K_HFAR && l[1].kind == K_DOWNFAR && l[2].kind == K_UPFAR);
		Sweep n;
		n.slots = false;                                        // a caller without checkpoint slots (a workspace of mc_predict_workspace_bytes)
		CHECK(n.run() == 0);
		l = take_log();
		CHECK(l.size() == 3 && l[0].kind == K_H && l[1].kind == K_DOWN && l[2].kind == K_UP && l[2].argmin);
		n.slots = true; n.ck1 = nullptr;                        // ... or with one missing, or misaligned
		CHECK(n.run() == 0);
		l = take_log();
		CHECK(l.size() == 3 && l[1].kind == K_DOWN && l[2].kind == K_UP);
		n.ck1 = (float *)0x9000004;
		CHECK(n.run() == 0);
		l = take_log();
		CHECK(l.size() == 3 && l[1].kind == K_DOWN && l[2].kind == K_UP);
		Sweep r;
		r.tri = false;                                          // volumes without the triangle promise (a caller's raw volumes): the same three launches
		CHECK(r.run() == 0);
		check_recompute_log(take_log(), r);
		Sweep t;
		CHECK(sgm_vertical(1) == 1);                            // the test entry's switch
		CHECK(t.run() == 0);
		l = take_log();
		CHECK(l.size() == 3 && l[0].kind == K_H && l[1].kind == K_DOWN && l[2].kind == K_UP && l[2].argmin);
		CHECK(l[2].A.drop_out[1] == 1 && l[1].A.drop_out[1] == 0);
		CHECK(sgm_vertical(2) == 2 && sgm_vertical(0) == 2);
		CHECK(t.run() == 0);
		check_recompute_log(take_log(), t);
	}

	// ---- a failure at each launch: the call reports it and launches nothing more ----
	for (int form = 1; form <= 2; ++form) {
		sgm_vertical(form);
		for (int f = 0; f < 3; ++f) {
			Sweep s;
			g_fail_at = f;
			const int rc = s.run();
			g_fail_at = -1;
			CHECK(rc == (int)hipErrorLaunchFailure);
			CHECK(strstr(last_error(), "sgm_pass") != nullptr);
			CHECK((int)take_log().size() == f + 1);
		}
	}
	sgm_vertical(0);

	// ---- make_plan: the checkpoint slots lie behind what mc_predict needs, inside the full workspace, and apart from every other area ----
	for (int H : {1, 2, 7, 8, 9, 16, 17, 29, 370})
		for (int W : {20, 36, 70, 1226})
			for (int cb = 0; cb < 2; ++cb) {
				mc_params p = kitti_fast();
				if (cb) { p.cbca_i1 = 2; p.cbca_i2 = 2; p.L1 = 5; }
				const int D = W == 1226 ? 228 : 35;
				char *base = (char *)0x7f0000000000;
				const Plan pl = make_plan(&p, D, H, W, base);
				CHECK(pl.total == make_plan(&p, D, H, W).total && pl.total_ck == make_plan(&p, D, H, W).total_ck);
				const size_t HW = (size_t)H * W, vol = align_up((size_t)pl.Dp * HW * 4, 256), img = align_up(HW * 4, 256), ckb = sgm_ck_bytes(H, W, pl.Dp);
				CHECK(ckb >= (size_t)((H + SGM_CK_ROWS - 1) / SGM_CK_ROWS) * W * pl.Dp * 4 && ckb % 256 == 0);
				CHECK((char *)pl.ck[0] == base + pl.total && (char *)pl.ck[1] == (char *)pl.ck[0] + ckb && pl.total_ck == pl.total + 2 * ckb);
				std::vector<Area> a = {{"maps", (char *)pl.maps, sgm_maps_bytes(H, W)}, {"ck0", (char *)pl.ck[0], ckb}, {"ck1", (char *)pl.ck[1], ckb},
				                       {"arms", (char *)pl.x0c, 8 * HW * 4}, {"packed", (char *)pl.packed, cbca_scratch_bytes(H, W)}, {"gk", (char *)pl.gk, 4}};
				for (int v = 0; v < 2; ++v) {
					a.push_back({"bufA", (char *)pl.bufA[v], vol}); a.push_back({"bufB", (char *)pl.bufB[v], vol}); a.push_back({"bufC", (char *)pl.bufC[v], vol});
					if (pl.cplan[v]) a.push_back({"cplan", (char *)pl.cplan[v], pl.cplan_bytes});
				}
				for (float *im : pl.img) a.push_back({"img", (char *)im, img});
				for (size_t i = 0; i < a.size(); ++i) {
					CHECK(a[i].lo >= base && a[i].lo + a[i].bytes <= base + pl.total_ck && (uintptr_t)a[i].lo % 256 == 0);
					if (a[i].name[0] != 'c' || a[i].name[1] != 'k') CHECK(a[i].lo + a[i].bytes <= base + pl.total);
					for (size_t j = i + 1; j < a.size(); ++j) CHECK(a[i].lo + a[i].bytes <= a[j].lo || a[j].lo + a[j].bytes <= a[i].lo);
				}
			}

	// ---- mc_predict on two lanes: each stream gets its volume's three launches in order, each volume its own slot; a failure at any
	//      launch still ends with the side stream's record and the caller stream's wait ----
	{
		mc_params p = kitti_fast();
		const int C = 64, D = 20, H = 17, W = 40;
		const size_t bytes = make_plan(&p, D, H, W).total_ck, bytes_min = make_plan(&p, D, H, W).total;
		std::vector<char> ws(bytes + 256);
		void *base = (void *)(((uintptr_t)ws.data() + 255) / 256 * 256);
		const Plan pl = make_plan(&p, D, H, W, base);
		const hipStream_t st = (hipStream_t)0x2000;
		const float *x = (const float *)0x100;
		predict_lanes(2);
		auto call = [&](bool timed) {
			StageTimer tm;
			tm.on = timed; tm.st = st;
			const int rc = predict_impl(&p, x, x, x, x, C, nullptr, nullptr, D, H, W, base, bytes, nullptr, nullptr, nullptr, nullptr, (float *)0x50, st, tm);
			float ms[MC_N_STAGES];
			if (timed) tm.collect(ms);
			return rc;
		};
		CHECK(call(false) == 0);
		auto l = take_log();
		const void *side = nullptr;
		for (const Entry &e : l) if (e.stream != st) { side = e.stream; break; }
		CHECK(side != nullptr);
		const auto a = kernels_on(l, st), b = kernels_on(l, side);
		CHECK(a.size() == 3 && b.size() == 3);
		if (a.size() == 3 && b.size() == 3) {
			for (const auto *k : {&a, &b}) CHECK((*k)[0].kind == K_H && (*k)[1].kind == K_CK && (*k)[2].kind == K_UPDOWN && (*k)[2].argmin && (*k)[0].A.nvol == 1);
			CHECK(a[1].A.direction[0] == -1 && a[1].A.ck[0] == pl.ck[0] && a[2].A.ck[0] == pl.ck[0] && a[2].A.drop_out[0] == 0);
			CHECK(b[1].A.direction[0] == 1 && b[1].A.ck[0] == pl.ck[1] && b[2].A.ck[0] == pl.ck[1] && b[2].A.drop_out[0] == 1);
			CHECK(a[2].A.out[0] == pl.bufB[0] && b[2].A.out[0] == pl.bufB[1] && a[2].A.disp[0] == pl.img[0] && b[2].A.disp[0] == pl.img[1]);
		}
		const int n_peeks = 7;   // sgm_prep, then three per lane
		for (int f = 0; f < n_peeks; ++f) {
			g_fail_at = f;
			const int rc = call(false);
			g_fail_at = -1;
			CHECK(rc != 0);
			l = take_log();
			bool side_used = false;
			for (const Entry &e : l) side_used = side_used || e.stream == side;
			if (!side_used) continue;   // failed in front of the fork's first wait
			CHECK(l.size() >= 2 && l[l.size() - 2].stream == side && l[l.size() - 2].what == "record" && l.back().stream == st && l.back().what == "wait");
		}
		CHECK(call(false) == 0);   // and the lane's lock was released every time
		take_log();
		// the timed form and one lane: one stream, the pair's three launches (stage_ms describes what runs)
		CHECK(call(true) == 0);
		l = take_log();
		for (const Entry &e : l) CHECK(e.stream == st);
		auto k = kernels_on(l, st);
		CHECK(k.size() == 3 && k[0].kind == K_H && k[1].kind == K_CK && k[2].kind == K_UPDOWN && k[2].argmin && k[1].A.nvol == 2);
		if (k.size() == 3) CHECK(k[2].A.ck[0] == pl.ck[0] && k[2].A.ck[1] == pl.ck[1] && k[2].A.drop_out[0] == 0 && k[2].A.drop_out[1] == 1);
		// a workspace without the slots: the down and the up sweep, and nothing refused
		{
			StageTimer tm;
			tm.on = true; tm.st = st;
			CHECK(predict_impl(&p, x, x, x, x, C, nullptr, nullptr, D, H, W, base, bytes_min, nullptr, nullptr, nullptr, nullptr, (float *)0x50, st, tm) == 0);
			float ms[MC_N_STAGES];
			tm.collect(ms);
			k = kernels_on(take_log(), st);
			CHECK(k.size() == 3 && k[0].kind == K_H && k[1].kind == K_DOWN && k[2].kind == K_UP && k[2].argmin);
			StageTimer tm2;
			CHECK(predict_impl(&p, x, x, x, x, C, nullptr, nullptr, D, H, W, base, bytes_min - 1, nullptr, nullptr, nullptr, nullptr, (float *)0x50, st, tm2) == MC_EINVAL);
			CHECK(take_log().empty());
		}
		// two iterations: the second one's launches again in order, on the swapped buffers and the same slots
		p.sgm_i = 2;
		CHECK(call(true) == 0);
		k = kernels_on(take_log(), st);
		CHECK(k.size() == 6);
		if (k.size() == 6) {
			CHECK(k[3].kind == K_H && k[4].kind == K_CK && k[5].kind == K_UPDOWN && k[5].argmin && !k[2].argmin);
			CHECK(k[4].A.C[0] == k[2].A.out[0] && k[5].A.out[0] == pl.bufA[0] && k[5].A.ck[0] == pl.ck[0] && k[2].A.drop_out[1] == 0 && k[5].A.drop_out[1] == 1);
		}
	}
	printf("%d %d\n", g_checked, g_failed);
	return g_failed ? 1 : 0;
}
