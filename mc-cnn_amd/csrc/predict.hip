// The fused stereo_predict pipeline behind mc_predict / mc_predict_timed (main.lua:929-1082): its workspace, the stages that
// -sm_terminate / -sm_skip leave, and the launches in order.  The extern "C" surface is api.hip.
#include "launchers.h"

#include <atomic>
#include <map>
#include <mutex>
#include <utility>

namespace mc {

// The maps of a range above 512 (sgm.hip).  Weak HERE only, like sgm_sweeps_ck: the host check of the two lanes links this unit against stubs of
// sgm_maps_bytes / sgm_prep alone.  Without them a range above 512 is refused (predict_impl), never run on the narrower maps.
size_t sgm_maps_bytes_d(int H, int W, int D) __attribute__((weak));
int sgm_prep_d(const float *x0, const float *x1, void *maps, int H, int W, int D, float tau_so, hipStream_t st) __attribute__((weak));
// The sub-pixel stage with its confidence maps (post.hip), weak HERE only for the same reason: those host checks define subpixel alone, and
// no call of theirs asks for a map.  Without it such a call is refused (predict_impl).
int subpixel_conf(const float *d0, const float *vol, float *out, int D, int H, int W, int64_t sd, int64_t sp, hipStream_t st, float *cost_out,
                  float *curv_out) __attribute__((weak));
// ... and the two mirrored forms of mc_predict_views' right tail (post.hip): without them a right-view map is refused (predict_impl).
int mirror_rows(const float *in, float *out, int H, int W, hipStream_t st) __attribute__((weak));
int subpixel_mirrored(const float *d0, const float *vol, float *out, int D, int H, int W, int64_t sd, int64_t sp, hipStream_t st) __attribute__((weak));

// gaussian(sigma), main.lua:528-540, double on the host.  mc_predict reads it from DEVICE memory, cached per (device, sigma): allocated and
// uploaded synchronously at first use (complete before any stream can be given it) and never freed; it depends on the preset alone.
void gaussian_fill(double sigma, float *k)
{
	const int ks = gaussian_ks(sigma), kr = ks / 2;
	for (int i = 1; i <= ks; ++i) {
		for (int j = 1; j <= ks; ++j) {
			const double y = (i - 1) - kr;
			const double x = (j - 1) - kr;
			k[(size_t)(i - 1) * ks + (j - 1)] = (float)exp(-(x * x + y * y) / (2 * sigma * sigma));
		}
	}
}
static int gaussian_cached(double sigma, const float *&out)
{
	static std::mutex mu;
	static std::map<std::pair<int, double>, const float *> cache;
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess) {
		set_error("gaussian: hipGetDevice: %s", hipGetErrorString(e));
		return (int)e;
	}
	std::lock_guard<std::mutex> lk(mu);
	auto it = cache.find({dev, sigma});
	if (it != cache.end()) { out = it->second; return 0; }
	const int ks = gaussian_ks(sigma);
	std::vector<float> k((size_t)ks * ks);
	gaussian_fill(sigma, k.data());
	float *dk = nullptr;
	e = hipMalloc((void **)&dk, k.size() * sizeof(float));
	if (e == hipSuccess) e = hipMemcpy(dk, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice);
	if (e != hipSuccess) {
		set_error("gaussian: device table of %zu floats: %s", k.size(), hipGetErrorString(e));
		if (dk) (void)hipFree(dk);
		return (int)e;
	}
	out = cache[{dev, sigma}] = dk;
	return 0;
}

// ---- the fast path's two lanes (predict_impl) ----
// MC_PREDICT_LANES, read once per process: "1" keeps the fast path on the caller's stream alone, anything else (and no value) is the
// default, 2.  A handle for A/B measurements and for the tests, which get both schedules from one library through predict_lanes(1 / 2).
int parse_predict_lanes(const char *s) { return (s && s[0] == '1' && s[1] == '\0') ? 1 : 2; }
int predict_lanes(int set, bool *is_forced)
{
	static const int from_env = parse_predict_lanes(getenv("MC_PREDICT_LANES"));
	static std::atomic<int> forced{0};   // 0: what the environment says
	if (set >= 0 && set <= 2) forced.store(set);
	const int f = forced.load();
	if (is_forced) *is_forced = f != 0;
	return f ? f : from_env;
}

#define MC_HIP(call, what) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { set_error("mc_predict: %s: %s", what, hipGetErrorString(e_)); return (int)e_; } } while (0)

// The side stream (non-blocking) and the three events of a caller's stream, made at the first two-lane call on (device, stream) and kept,
// like the Gaussian table: nothing is created per call.  `mu` is held while a call enqueues between its fork and its join: two host
// threads on ONE caller stream would otherwise re-record an event between the other's record and wait.
// Several caller streams in one process (pairs in flight): their pairs already run beside each other, and with a side stream each -- or
// with one left over from a single-stream phase: the process then has more streams than the four hardware queues it opens, and two
// callers share one -- K = 2 and 3 got slower (profiles/two_lane_ab.txt).  So once a device has seen a fast-path call from a second caller
// stream, it keeps one lane for the life of the process: no side stream is made any more (out = null), and those that exist and are not
// between a fork and a join are released.  A rule on the order of the calls alone: nothing is asked of the device.  `solo_only` = false
// (the tests' forced setting) stands outside the rule.  The entry comes back locked (`held`), taken under the cache's own lock, so that
// no entry is released while a call holds or awaits it.
static int lanes_cached(hipStream_t st, bool solo_only, Lanes *&out, std::unique_lock<std::mutex> &held)
{
	static std::mutex mu;
	static auto &cache = *new std::map<std::pair<int, hipStream_t>, Lanes *>;   // never destroyed: a call may be under way at exit
	static auto &first_caller = *new std::map<int, hipStream_t>;               // per device: the caller stream of its first fast-path call
	static auto &many_callers = *new std::map<int, bool>;
	int dev = 0;
	MC_HIP(hipGetDevice(&dev), "hipGetDevice");
	std::lock_guard<std::mutex> lk(mu);
	out = nullptr;
	if (solo_only) {
		auto fc = first_caller.find(dev);
		if (fc == first_caller.end()) first_caller[dev] = st;
		else if (fc->second != st) many_callers[dev] = true;
		if (many_callers[dev]) {
			for (auto it = cache.begin(); it != cache.end();) {
				Lanes *l = it->second;
				if (it->first.first != dev || !l->mu.try_lock()) { ++it; continue; }
				(void)hipStreamDestroy(l->side);   // (what it still has queued runs to its end: the caller's stream waits for it)
				for (hipEvent_t ev : {l->fork, l->join_left, l->right_done}) (void)hipEventDestroy(ev);
				l->mu.unlock();
				delete l;
				it = cache.erase(it);
			}
			return 0;
		}
	}
	auto it = cache.find({dev, st});
	if (it == cache.end()) {
		Lanes *l = new Lanes;
		hipError_t e = hipStreamCreateWithFlags(&l->side, hipStreamNonBlocking);
		hipEvent_t *const evs[3] = {&l->fork, &l->join_left, &l->right_done};
		for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(evs[i], hipEventDisableTiming);
		if (e != hipSuccess) {
			set_error("mc_predict: side stream and events: %s", hipGetErrorString(e));
			for (hipEvent_t *ev : evs) if (*ev) (void)hipEventDestroy(*ev);
			if (l->side) (void)hipStreamDestroy(l->side);
			delete l;
			return (int)e;
		}
		it = cache.emplace(std::make_pair(dev, st), l).first;
	}
	out = it->second;
	held = std::unique_lock<std::mutex>(out->mu);
	return 0;
}

// From the fork on, whichever way predict_impl returns, the caller's stream waits for the side stream's last recorded event: it is
// never left ahead of work that still writes the workspace.  (Declared after the lock on Lanes::mu: the wait is enqueued under it.)
struct LaneJoin {
	hipStream_t st = nullptr;
	Lanes *ln = nullptr;
	bool armed = false;
	int join()   // side: record right_done; caller's stream: wait for it
	{
		if (!armed) return 0;
		armed = false;
		MC_HIP(hipEventRecord(ln->right_done, ln->side), "hipEventRecord (right lane done)");
		MC_HIP(hipStreamWaitEvent(st, ln->right_done, 0), "hipStreamWaitEvent (right lane done)");
		return 0;
	}
	~LaneJoin() { (void)join(); }
};

// -sm_terminate / -sm_skip (main.lua:956,988-1040) are identical for both directions, so for the three volume stages they
// reduce to effective iteration counts; for the stages on the left disparity behind them (main.lua:1054-1079), to whether each runs.
// The one place that reads sm_terminate / sm_skip: predict_impl runs what it says, and refuses a map of a stage that it leaves out.
struct StageCounts { int cbca1, sgm, cbca2; bool occlusion, mismatch, subpixel, median, bilateral; };
static StageCounts stage_counts(const mc_params *p)
{
	StageCounts c;
	bool sm_active = p->sm_terminate != MC_SM_CNN;
	c.cbca1 = (sm_active && p->sm_skip != MC_SKIP_CBCA) ? p->cbca_i1 : 0;
	sm_active = sm_active && p->sm_terminate != MC_SM_CBCA1;
	c.sgm = (sm_active && p->sm_skip != MC_SKIP_SGM) ? p->sgm_i : 0;
	sm_active = sm_active && p->sm_terminate != MC_SM_SGM;
	c.cbca2 = (sm_active && p->sm_skip != MC_SKIP_CBCA) ? p->cbca_i2 : 0;
	sm_active = sm_active && p->sm_terminate != MC_SM_CBCA2;
	// a stage runs if the method is still active and the stage is not skipped; then -sm_terminate applies
	auto stage = [&](int skip, int terminate) {
		const bool runs = sm_active && p->sm_skip != skip;
		sm_active = sm_active && p->sm_terminate != terminate;
		return runs;
	};
	c.occlusion = c.mismatch = false;
	if (p->lr_check) {   // (without the LR check the two stages do not exist: their -sm_terminate names end nothing)
		c.occlusion = stage(MC_SKIP_OCCLUSION, MC_SM_OCCLUSION);
		c.mismatch = stage(MC_SKIP_OCCLUSION, MC_SM_MISMATCH);
	}
	c.subpixel = stage(MC_SKIP_SUBPIXEL, MC_SM_SUBPIXEL);
	c.median = stage(MC_SKIP_MEDIAN, MC_SM_MEDIAN);
	c.bilateral = stage(MC_SKIP_BILATERAL, MC_SM_BILATERAL);
	return c;
}

// The one place that lays mc_predict's workspace out: the sizes of its areas, their sum and -- unless base is null -- where each lies.
Plan make_plan(const mc_params *p, int D, int H, int W, void *base)
{
	Plan pl;
	// pixel stride of the (H,W,ds) volumes: D rounded up to 4 (16-byte runs).  Rounding up to 32 (every run on whole 128-byte
	// lines) was measured on one box at 370x1226x228 (ds 228 -> 256): the transposes 0.465 -> 0.377 ms, the sweeps 2.016 ->
	// 2.105 ms (12 % more bytes), StereoJoin unchanged; 6.000 -> 5.998 ms with the aggregation, 2.87 -> 2.97 ms without: not adopted.
	pl.Dp = (D + 3) / 4 * 4;
	const size_t HW = (size_t)H * W;
	const size_t vol = align_up((size_t)pl.Dp * HW * sizeof(float), 256), img = align_up(HW * sizeof(float), 256);
	const int ks = gaussian_ks(p->blur_sigma);
	// the tile kernel's bookkeeping is the same in every aggregation pass over the pair and direction: kept from the first pass
	// on (cbca_plan_bytes: ~3.6 bytes per voxel) -- where a second pass exists to read it (after -sm_skip / -sm_terminate),
	// and per direction that is computed (left_only without the LR check: the left volume only; a caller who then asks for
	// right-side outputs gets that direction without a plan)
	const StageCounts sc = stage_counts(p);
	pl.cplan_bytes = (sc.cbca1 + sc.cbca2 >= 2 && p->L1 - 1 <= 13) ? align_up(cbca_plan_bytes(D, H, W), 256) : 0;
	const int nplan = (p->left_only && !p->lr_check) ? 1 : 2;   // directions that get one

	size_t off = 0;
	auto take = [&](size_t bytes) { off += bytes; return base ? (char *)base + (off - bytes) : nullptr; };
	// (D > 512: the wider window rows of the VPL = 16 line walks; a program without sgm.hip gets the plain size here and predict_impl's refusal)
	pl.maps = take(align_up((D > 512 && sgm_maps_bytes_d) ? sgm_maps_bytes_d(H, W, D) : sgm_maps_bytes(H, W), 256));
	pl.x0c = (float *)take(align_up(8 * HW * sizeof(float), 256));
	pl.x1c = base ? pl.x0c + 4 * HW : nullptr;
	pl.packed = take(cbca_scratch_bytes(H, W));
	for (float **buf : {pl.bufA, pl.bufB, pl.bufC})
		for (int v = 0; v < 2; ++v) buf[v] = (float *)take(vol);
	for (float *&im : pl.img) im = (float *)take(img);
	pl.gk = (float *)take(align_up((size_t)ks * ks * sizeof(float), 256));
	for (int v = 0; v < 2; ++v) pl.cplan[v] = (pl.cplan_bytes && v < nplan) ? take(pl.cplan_bytes) : nullptr;
	pl.total = off;
	// the optional tail: mc_predict_workspace_bytes stays what it was (a workspace of that size runs the down and the up sweep)
	for (float *&ck : pl.ck) ck = (float *)take(sgm_ck_bytes(H, W, pl.Dp));
	pl.total_ck = off;
	return pl;
}

void StageTimer::mark(int stage)
{
	if (!on) return;
	hipEvent_t e;
	(void)hipEventCreate(&e);
	(void)hipEventRecord(e, st);
	ev.push_back(e);
	tag.push_back(stage);
}
void StageTimer::collect(float out[MC_N_STAGES])
{
	for (int i = 0; i < MC_N_STAGES; ++i) out[i] = 0;
	if (!on || ev.empty()) return;
	(void)hipEventSynchronize(ev.back());
	for (size_t i = 1; i < ev.size(); ++i) {
		float ms = 0;
		(void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]);
		if (tag[i] >= 0 && tag[i] < MC_N_STAGES) out[tag[i]] += ms;
	}
	for (auto e : ev) (void)hipEventDestroy(e);
	ev.clear();
}

int predict_impl(const mc_params *p, const float *x0, const float *x1, const float *featL, const float *featR, int C,
                 const float *rawL, const float *rawR, int D, int H, int W, void *workspace, size_t workspace_bytes,
                 float *volL_out, float *volR_out, float *dispL0_out, float *dispR0_out, float *disp_out, hipStream_t st,
                 StageTimer &tm, const PredictExtras &ex)
{
	MC_REQUIRE(p && x0 && x1 && disp_out && workspace, "mc_predict: null argument");
	MC_REQUIRE(dims_ok(D, H, W), "mc_predict: bad dims D=%d H=%d W=%d", D, H, W);
	MC_REQUIRE(D <= MC_SGM_MAX_D, "mc_predict: D=%d exceeds %d", D, MC_SGM_MAX_D);
	MC_REQUIRE(D <= 512 || (sgm_maps_bytes_d && sgm_prep_d), "mc_predict: D=%d needs the wide SGM maps, which this program does not link", D);
	MC_REQUIRE((featL && featR && C >= 1) || (rawL && rawR), "mc_predict: need features or raw volumes");
	MC_REQUIRE(p->cbca_i1 >= 0 && p->cbca_i2 >= 0 && p->sgm_i >= 0, "mc_predict: negative iteration count");
	MC_REQUIRE(p->median_k % 2 == 1 && p->median_k <= 11, "mc_predict: median_k must be odd and <= 11");
	MC_REQUIRE(p->blur_sigma > 0, "mc_predict: blur_sigma must be > 0");
	MC_REQUIRE(p->sm_terminate >= 0 && p->sm_terminate <= MC_SM_BILATERAL && p->sm_skip >= 0 && p->sm_skip <= MC_SKIP_BILATERAL,
	           "mc_predict: bad sm_terminate / sm_skip");
	const bool from_feat = featL != nullptr;
	if (from_feat) MC_REQUIRE(p->border_n >= 0 && p->border_n < W, "mc_predict: border_n=%d out of range", p->border_n);
	if (from_feat) MC_REQUIRE(C <= MC_JOIN_MAX_C, "mc_predict: C=%d exceeds %d (adcensus.cu:1460)", C, MC_JOIN_MAX_C);
	const Plan pl = make_plan(p, D, H, W, workspace);   // (addresses only: nothing is touched before the two checks)
	MC_REQUIRE(workspace_bytes >= pl.total, "mc_predict: workspace %zu < %zu bytes", workspace_bytes, pl.total);
	MC_REQUIRE((uintptr_t)workspace % 256 == 0, "mc_predict: workspace must be 256-byte aligned");
	const StageCounts sc = stage_counts(p);   // -sm_terminate / -sm_skip as effective iteration counts and stages that run
	{   // mc_predict_ex's maps: none of a stage that does not run, none on top of anything else the call reads back or works in
		const size_t map_bytes = (size_t)H * W * sizeof(float), vol_bytes = (size_t)D * map_bytes;
		struct Range { const char *name; const void *at; size_t bytes; };
		const Range extras[3] = {{"outlier_out", ex.outlier, map_bytes}, {"cost_out", ex.cost, map_bytes}, {"curv_out", ex.curv, map_bytes}};
		const Range others[6] = {{"disp_out", disp_out, map_bytes}, {"volL_out", volL_out, vol_bytes}, {"volR_out", volR_out, vol_bytes},
		                         {"dispL0_out", dispL0_out, map_bytes}, {"dispR0_out", dispR0_out, map_bytes}, {"the workspace", workspace, workspace_bytes}};
		auto overlap = [](const Range &a, const Range &b) {
			return a.at && b.at && (uintptr_t)a.at < (uintptr_t)b.at + b.bytes && (uintptr_t)b.at < (uintptr_t)a.at + a.bytes;
		};
		// mc_predict_views' two maps of the right view: the same range check
		const Range views[2] = {{"dispR_out", ex.dispR, map_bytes}, {"outlierR_out", ex.outlierR, map_bytes}};
		for (int i = 0; i < 2; ++i) {
			if (views[i].at) MC_REQUIRE(mirror_rows && subpixel_mirrored, "mc_predict_views: %s needs the mirrored kernels, which this program does not link", views[i].name);
			for (const Range &o : others) MC_REQUIRE(!overlap(views[i], o), "mc_predict_views: %s overlaps %s", views[i].name, o.name);
			for (const Range &o : extras) MC_REQUIRE(!overlap(views[i], o), "mc_predict_views: %s overlaps %s", views[i].name, o.name);
			for (int j = 0; j < i; ++j) MC_REQUIRE(!overlap(views[i], views[j]), "mc_predict_views: %s overlaps %s", views[i].name, views[j].name);
		}
		for (int i = 0; i < 3; ++i) {
			if (i > 0 && extras[i].at) {
				MC_REQUIRE(sc.subpixel, "mc_predict_ex: %s is written by the sub-pixel stage, which sm_terminate=%d / sm_skip=%d leave out",
				           extras[i].name, p->sm_terminate, p->sm_skip);
				MC_REQUIRE(subpixel_conf, "mc_predict_ex: %s needs the sub-pixel stage's maps, which this program does not link", extras[i].name);
			}
			for (const Range &o : others) MC_REQUIRE(!overlap(extras[i], o), "mc_predict_ex: %s overlaps %s", extras[i].name, o.name);
			for (int j = 0; j < i; ++j) MC_REQUIRE(!overlap(extras[i], extras[j]), "mc_predict_ex: %s overlaps %s", extras[i].name, extras[j].name);
		}
	}

	const bool have_ck = workspace_bytes >= pl.total_ck && sgm_sweeps_ck != nullptr;   // the workspace holds the SGM's checkpoint slots

	const int64_t HW = (int64_t)H * W;
	const int64_t V = (int64_t)D * HW;
	int cplan_passes[2] = {0, 0};   // aggregation passes so far: the first one writes the plan, the others read it
	bool cplan_listed[2] = {false, false};   // ... the texture route's list has been written
	int rc;
#define RUN(call) do { rc = (call); if (rc) return rc; } while (0)

	// index 0 = left volume (direction -1), 1 = right volume (direction +1)  (main.lua:986)
	const int direction[2] = {-1, 1};
	const int n_cbca1 = sc.cbca1, n_sgm = sc.sgm, n_cbca2 = sc.cbca2;
	const bool use_cbca = (n_cbca1 + n_cbca2) > 0;
	tm.mark(-1);

	if (n_sgm > 0) RUN(D > 512 ? sgm_prep_d(x0, x1, pl.maps, H, W, D, p->tau_so, st) : sgm_prep(x0, x1, pl.maps, H, W, p->tau_so, st));
	if (use_cbca) {  // main.lua:993-996: x0c from the LEFT image, x1c from the RIGHT, for both directions
		RUN(cross(x0, pl.x0c, H, W, p->L1, p->tau1, st));
		RUN(cross(x1, pl.x1c, H, W, p->L1, p->tau1, st));
		RUN(cbca_pack(pl.x0c, pl.x1c, pl.packed, H, W, st));
	}
	const int cbca_cap = p->L1 - 1;  // cross(): an arm never exceeds L1-1 pixels (adcensus.cu:314)
	tm.mark(MC_STAGE_PREP);

	// ---- (A) cost volumes + CBCA-1; ends with cur[v] and its layout ----
	// Internal (H,W,ds) volumes use the padded pixel stride ds = Dp (multiple of 4) so that
	// every lane's run of 4 disparities is one aligned 16-byte access.
	const int ds = pl.Dp;
	const float *cur[2];
	auto other = [&](int v) -> float * { return cur[v] == pl.bufA[v] ? pl.bufB[v] : pl.bufA[v]; };
	bool hwd;  // layout of cur[]
	// direction +1 (the right volume) is skipped where the reference skips it: dataset mb outside `-a predict`
	// (mb_directions, main.lua:953-955) -- only when nothing of it is asked for (the class map compares the two arg-min maps)
	const bool right_view = ex.dispR || ex.outlierR;   // mc_predict_views: the tail runs a second time, on the right view (below)
	const int nvol = (p->left_only && !p->lr_check && !volR_out && !dispR0_out && !ex.outlier && !right_view) ? 1 : 2;
	// n CBCA iterations on the (D,H,W) volumes, ping-pong between the two buffers of each side (instead of vol:copy(tmp)).
	// Where the pair's route may be the texture one (cfg.lean), the iterations go in PAIRS: cbca_lean2x runs two passes in one launch
	// (cur -> dst) out of a list written once per pair and direction; the kernels of the other routes -- which one runs is decided on
	// the device by the route word, the others stand down at their first instruction -- take the same two passes through the SGM's
	// scratch volume (cur -> bufC -> dst), so that every route ends in the same buffer.  An odd last iteration is a single pass.
	auto cbca_iterations = [&](int n) -> int {
		const bool packed_ok = cbca_cap <= 254 && packed_dims_ok(H, W);  // packed lengths saturate at 255
		for (int v = 0; v < nvol; ++v) {
			// the plan area serves whichever kernel the pair's route word picks: the tile kernel's plan (written by its first pass) or, on
			// textures, the records of the outputs whose support is not the minimal 3 x 3 -- written HERE, before the direction's first pass
			// (route-gated, on the device), so that every later launch finds the list's state final: usable -> cbca_lean2x per pair of passes
			// and the strip kernel for a single one; unusable (flat regions next to the texture) -> the tile kernel
			const bool planned = packed_ok && pl.cplan[v] && cbca_cap > 4 && cbca_cap <= 13 && cbca_lean_fits(D, H, W, pl.cplan_bytes, true);
			if (planned && n > 0 && !cplan_listed[v]) {
				const int rc1 = cbca_classify(pl.packed, pl.cplan[v], pl.cplan_bytes, D, H, W, direction[v], CR_STRIP, 0, 0, st, true);
				if (rc1) return rc1;
				cplan_listed[v] = true;
			}
			for (int i = 0; i < n;) {
				float *dst = other(v);
				CbcaCfg cfg;
				cfg.plan = pl.cplan[v];
				cfg.plan_bytes = pl.cplan_bytes;
				cfg.planned = planned;
				const bool two = planned && i + 1 < n;
				cfg.lean = cfg.lean_two_pass = two;   // (a single pass: the strip kernel serves the texture route itself)
				float *mid = two ? pl.bufC[v] : dst;
				for (int half = 0; half < (two ? 2 : 1); ++half) {   // the routes that take one pass per launch
					cfg.plan_mode = pl.cplan[v] ? (cplan_passes[v]++ == 0 ? 1 : 2) : 0;
					const float *src = half == 0 ? cur[v] : mid;
					float *to = (two && half == 0) ? mid : dst;
					const int rc2 = packed_ok ? cbca_by_arms(pl.packed, src, to, D, H, W, direction[v], cbca_cap, st, cfg)
					                          : cbca(pl.x0c, pl.x1c, src, to, D, H, W, direction[v], st);
					if (rc2) return rc2;
				}
				if (two) {
					const int rc3 = cbca_lean2x(pl.packed, pl.cplan[v], pl.cplan_bytes, cur[v], dst, D, H, W, direction[v], CR_STRIP, st, cfg);
					if (rc3) return rc3;
				}
				cur[v] = dst;
				i += two ? 2 : 1;
			}
		}
		return 0;
	};
	// (C + 64: the kernels pad the channel count to their k-step sizes and add channel offsets to range-checked 32-bit byte
	// offsets -- no padded channel's offset may wrap)
	const bool join_fits = (int64_t)W * ((D + 3) / 4 * 4) * 4 < ((int64_t)1 << 31) && ((int64_t)(C + 64) * HW + W) * 4 < ((int64_t)1 << 31);
	// the volumes hold NaN wherever the partner pixel lies outside the image (left: d > x, right: x + d >= W), sgm_sweeps' `tri`
	bool nan_triangle = false;
	// (B) below, for volumes [v0, v0 + nv) on stream s
	float *dispv[2] = {pl.img[0], pl.img[1]};  // [0] = left disparity (disp[2] in Lua), [1] = right
	bool have_disp = false;
	auto sgm_iterations = [&](int v0, int nv, hipStream_t s) -> int {
		for (int it = 0; it < n_sgm; ++it) {
			// out:zero(); sgm2(...); vol:copy(out):div(4)  (main.lua:1013-1018): the zero is folded
			// into the first sweep (0 + L_0) and the /4 into the last
			const float *Cv[2];
			float *outv[2], *scratch[2], *dv[2], *ckv[2] = {nullptr, nullptr};
			int dir[2];
			for (int k = 0; k < nv; ++k) {
				Cv[k] = cur[v0 + k]; outv[k] = other(v0 + k); scratch[k] = pl.bufC[v0 + k]; dv[k] = dispv[v0 + k]; dir[k] = direction[v0 + k];
				ckv[k] = pl.ck[v0 + k];
			}
			const bool am = (it == n_sgm - 1) && n_cbca2 == 0;
			// the right volume's final costs: where no CBCA-2 follows, only right.bin reads them (sub-pixel refinement reads the
			// left volume, the LR check the arg-min maps that the up sweep writes regardless) -- not stored unless asked for.
			// sgm_sweeps counts its bits from the first volume it is given: bit 1 of a pair, bit 0 of the right volume alone
			const bool has_right = v0 + nv == 2;
			// (... and the right view's sub-pixel stage, where its map is asked for)
			const unsigned drop_final = (am && has_right && !volR_out && !(ex.dispR && sc.subpixel)) ? 1u << (1 - v0) : 0u;
			const int rc1 = have_ck ? sgm_sweeps_ck(Cv, outv, scratch, am ? dv : nullptr, dir, nv, H, W, D, ds, pl.maps, p->pi1, p->pi2, p->alpha1,
			                                        p->sgm_q1, p->sgm_q2, true, drop_final, nan_triangle, ckv, s)
			                        : sgm_sweeps(Cv, outv, scratch, am ? dv : nullptr, dir, nv, H, W, D, ds, pl.maps, p->pi1, p->pi2, p->alpha1,
			                                     p->sgm_q1, p->sgm_q2, true, drop_final, nan_triangle, s);
			if (rc1) return rc1;
			have_disp = am;
			for (int k = 0; k < nv; ++k) cur[v0 + k] = outv[k];
		}
		return 0;
	};
	// Two lanes: the left volume's chain stays on the caller's stream, the right volume's runs on a side stream one stage behind it --
	// its StereoJoin (matrix pipes) beside the left volume's horizontal sweeps (memory), then sweep beside sweep -- and joins in front of
	// the LR check.  The volumes share nothing between StereoJoin and the LR check but the SGM maps, which both only read.
	std::unique_lock<std::mutex> lane_lock;
	LaneJoin lane_b;
	if (from_feat && n_cbca1 == 0 && n_sgm > 0 && join_fits) {
		// fast path: StereoJoin straight into (H,W,ds) with NaN fill and fix_border folded in
		bool forced = false;
		const bool two_lanes = nvol == 2 && n_cbca2 == 0 && C <= 64 && !tm.on && predict_lanes(-1, &forced) == 2;
		cur[0] = pl.bufA[0]; cur[1] = pl.bufA[1];
		hwd = true;
		nan_triangle = true;   // (why: below)
		Lanes *ln = nullptr;
		if (two_lanes) RUN(lanes_cached(st, !forced, ln, lane_lock));
		if (ln) {
			MC_HIP(hipEventRecord(ln->fork, st), "hipEventRecord (fork)");   // after sgm_prep: the maps are the right lane's too
			RUN(stereo_join_hwd(featL, featR, pl.bufA[0], pl.bufA[1], C, D, ds, H, W, p->border_n, st, 1));
			MC_HIP(hipEventRecord(ln->join_left, st), "hipEventRecord (left join)");
			// the right lane, start to end; the stagger: its join starts when the left one has finished, not beside it
			lane_b.st = st; lane_b.ln = ln; lane_b.armed = true;
			MC_HIP(hipStreamWaitEvent(ln->side, ln->fork, 0), "hipStreamWaitEvent (fork)");
#ifndef MC_LANES_NO_STAGGER
			MC_HIP(hipStreamWaitEvent(ln->side, ln->join_left, 0), "hipStreamWaitEvent (left join)");
#endif
			RUN(stereo_join_hwd(featL, featR, pl.bufA[0], pl.bufA[1], C, D, ds, H, W, p->border_n, ln->side, 2));
			RUN(sgm_iterations(1, 1, ln->side));
			if (volR_out) RUN(transpose(cur[1], volR_out, HW, D, ds, HW, 1.0f, ln->side));
			if (dispR0_out) RUN(scale(dispv[1], dispR0_out, HW, 1.0f, ln->side));
			// (right_done is recorded behind these launches where the lanes meet, or on the way out of a failed call: LaneJoin)
		} else {
			RUN(stereo_join_hwd(featL, featR, pl.bufA[0], pl.bufA[1], C, D, ds, H, W, p->border_n, st));
		}
		// stereo_join_hwd writes NaN there itself.  Its fix_border_hwd then copies the whole cost vector of column W - (n + 1) to the
		// columns right of it (left volume) and of column n to the columns left of it (right volume): the source column has no more
		// live disparities than any target (x + 1 grows to the right, W - x to the left), so the copy may add NaNs below a
		// target's Dv but leaves none out at or above it.  Every SGM iteration keeps the triangle NaN (NaN + anything).
		tm.mark(MC_STAGE_JOIN);
	} else {
		if (from_feat) {  // main.lua:946-949
			RUN(fill_nan(pl.bufA[0], V, st));
			RUN(fill_nan(pl.bufA[1], V, st));
			RUN(stereo_join_dhw(featL, featR, pl.bufA[0], pl.bufA[1], C, D, H, W, st));
			RUN(fix_border(pl.bufA[0], D, H, W, p->border_n, -1, st));
			RUN(fix_border(pl.bufA[1], D, H, W, p->border_n, 1, st));
			cur[0] = pl.bufA[0]; cur[1] = pl.bufA[1];
		} else {
			cur[0] = rawL; cur[1] = rawR;
		}
		hwd = false;
		tm.mark(MC_STAGE_JOIN);
		RUN(cbca_iterations(n_cbca1));  // main.lua:998-1001 (ping-pong instead of vol:copy(tmp))
		tm.mark(MC_STAGE_CBCA);
	}

	// ---- (B) SGM, main.lua:1007-1030 ----
	const int nmain = lane_b.armed ? 1 : nvol;   // volumes whose chain runs on the caller's stream
	if (n_sgm > 0) {
		if (!hwd) {  // vol:transpose(2,3):transpose(3,4):clone(), main.lua:1008
			for (int v = 0; v < nvol; ++v) {
				float *dst = other(v);
				RUN(transpose(cur[v], dst, D, HW, HW, ds, 1.0f, st));
				cur[v] = dst;
			}
			hwd = true;
			tm.mark(MC_STAGE_LAYOUT);
		}
		RUN(sgm_iterations(0, nmain, st));
		tm.mark(MC_STAGE_SGM);
		if (n_cbca2 > 0) {  // back to (D,H,W): vol:copy(out:transpose(3,4):transpose(2,3)), main.lua:1019-1020
			for (int v = 0; v < nvol; ++v) {
				float *dst = other(v);
				RUN(transpose(cur[v], dst, HW, D, ds, HW, 1.0f, st));
				cur[v] = dst;
			}
			hwd = false;
			tm.mark(MC_STAGE_LAYOUT);
		}
	}
	if (!hwd) {  // CBCA-2, main.lua:1033-1039
		RUN(cbca_iterations(n_cbca2));
		tm.mark(MC_STAGE_CBCA);
	}

	// ---- argmin, main.lua:1049-1050 ----
	// an (H,W,ds) volume exists only around the SGM, whose last up sweep folds the arg-min in where no CBCA-2 follows (have_disp)
	MC_REQUIRE(have_disp || !hwd, "mc_predict: an (H,W,D) volume without its arg-min");
	if (!have_disp) {
		for (int v = 0; v < nvol; ++v) RUN(argmin_dhw(cur[v], dispv[v], D, H, W, 0, st));
	}
	// ---- left.bin / right.bin contents, main.lua:1042-1047 ----
	float *vout[2] = {volL_out, volR_out};
	for (int v = 0; v < nmain; ++v) {   // (the right lane has exported its own)
		if (!vout[v]) continue;
		if (hwd) RUN(transpose(cur[v], vout[v], HW, D, ds, HW, 1.0f, st));
		else RUN(scale(cur[v], vout[v], V, 1.0f, st));
	}
	if (dispL0_out) RUN(scale(dispv[0], dispL0_out, HW, 1.0f, st));
	if (dispR0_out && nmain == nvol) RUN(scale(dispv[1], dispR0_out, HW, 1.0f, st));
	tm.mark(MC_STAGE_ARGMIN);
	// the lanes meet: everything below is the caller's stream alone (the LR check reads the right arg-min)
	RUN(lane_b.join());
	if (lane_lock.owns_lock()) lane_lock.unlock();

	// ---- (C) post-processing on the LEFT disparity, main.lua:1054-1081 ----
	// every stage reads `d` and writes the next free image; -sm_skip / -sm_terminate drop stages (main.lua:1057-1079)
	float *d = dispv[0];
	float *outl = ex.outlier ? ex.outlier : pl.img[4];   // the LR check's classes: in the caller's map where one is given, and read from there
	int nfree = 0;
	float *freeimg[3] = {pl.img[2], pl.img[3], pl.img[5]};
	auto next = [&]() -> float * {
		float *r = freeimg[nfree % 3];
		if (r == d) r = freeimg[++nfree % 3];
		++nfree;
		return r;
	};
	// one stage: if it runs (stage_counts) it runs into the next free image, which becomes `d`
	auto stage = [&](bool runs, auto &&run) -> int {
		if (runs) {
			float *o = next();
			if (const int rc1 = run(o)) return rc1;
			d = o;
		}
		return 0;
	};
	if (p->lr_check) {
		RUN(outlier_detection(d, dispv[1], outl, H, W, D, st));
		// the occlusion stage leaves the mismatch marks as a bitmask for the ray walk, in the cross arms' area (dead since the last
		// aggregation pass); where that stage does not run there is none and the walk reads the marks themselves
		const unsigned *mis_mask = nullptr;
		RUN(stage(sc.occlusion, [&](float *o) {
			unsigned *m = HW <= MC_MIS_MASK_MAX_PIXELS ? (unsigned *)pl.x0c : nullptr;
			mis_mask = m;
			return interpolate_occlusion(d, outl, o, H, W, st, m);
		}));
		RUN(stage(sc.mismatch, [&](float *o) { return interpolate_mismatch(d, outl, o, H, W, st, mis_mask); }));
	} else if (ex.outlier) {
		RUN(outlier_detection(d, dispv[1], ex.outlier, H, W, D, st));   // the classes alone: nothing here reads them
	}
	// subpixel on the LEFT volume (vol of the last loop iteration, main.lua:1068)
	RUN(stage(sc.subpixel, [&](float *o) {
		const int64_t sd = hwd ? 1 : HW, sp = hwd ? ds : 1;
		return (ex.cost || ex.curv) ? subpixel_conf(d, cur[0], o, D, H, W, sd, sp, st, ex.cost, ex.curv) : subpixel(d, cur[0], o, D, H, W, sd, sp, st);
	}));
	RUN(stage(sc.median, [&](float *o) { return median2d(d, o, H, W, p->median_k, st); }));
	if (sc.bilateral) {
		const float *gk = nullptr;
		RUN(gaussian_cached(p->blur_sigma, gk));
		RUN(mean2d(d, gk, disp_out, H, W, gaussian_ks(p->blur_sigma), p->blur_t, st));
	} else {
		RUN(scale(d, disp_out, HW, 1.0f, st));  // the last stage that ran is the result
	}

	// ---- (D) mc_predict_views: the same tail on the RIGHT view ----
	// Mirroring the scene along x, M(a)[y, x] = a[y, W-1-x], turns the right image into a left one, so the right view's map is what the tail
	// above gives on the mirrored maps, mirrored back: the classes from (M(dispR0), M(dispL0)), the two interpolations, the sub-pixel stage
	// on M(volR), median, blur.  The direction-dependent stages -- the LR check's x - d, the occlusion stage's "look left first" and the
	// roundf of the half-step mismatch rays, which is NOT mirror-symmetric -- are thereby fixed by the mirror: the kernels are the left
	// view's, fed physically mirrored maps, and no right-handed variant of any of them exists.  Only the sub-pixel stage, which is
	// pointwise, reads the volume at the mirrored pixel instead of a mirrored volume (the mean's float sum runs in tap order and does not
	// commute with M, so it is not given M's output but M's input, like the others).
	// The workspace: the left tail is done, so of the six images only the arg-min maps 0 and 1 are live, and they die with the two
	// mirrored copies (into 2 and 3).  The classes go to 4 (the left view's are in the caller's map or no longer read), the stages rotate
	// through 0, 1, 5 and, once the classes are computed, 3.  The right volume cur[1] is whole: nothing above writes a volume behind the
	// arg-min (the left tail writes images, the caller's maps and the mismatch bitmask in the cross arms' area), the two-lane path has
	// joined, and drop_final keeps the final costs where this map is asked for.
	if (right_view) {
		float *const mR = pl.img[2], *const mL = pl.img[3], *const oR = pl.img[4];
		RUN(mirror_rows(dispv[1], mR, H, W, st));
		RUN(mirror_rows(dispv[0], mL, H, W, st));
		RUN(outlier_detection(mR, mL, oR, H, W, D, st));
		if (ex.outlierR) RUN(mirror_rows(oR, ex.outlierR, H, W, st));
		if (ex.dispR) {
			d = mR;
			float *const rimg[4] = {pl.img[0], pl.img[1], pl.img[5], pl.img[3]};
			int nr = 0;
			auto rstage = [&](bool runs, auto &&run) -> int {
				if (runs) {
					float *o = rimg[nr++ % 4];
					if (const int rc1 = run(o)) return rc1;
					d = o;
				}
				return 0;
			};
			if (p->lr_check) {
				const unsigned *mis_mask = nullptr;
				RUN(rstage(sc.occlusion, [&](float *o) {
					unsigned *m = HW <= MC_MIS_MASK_MAX_PIXELS ? (unsigned *)pl.x0c : nullptr;
					mis_mask = m;
					return interpolate_occlusion(d, oR, o, H, W, st, m);
				}));
				RUN(rstage(sc.mismatch, [&](float *o) { return interpolate_mismatch(d, oR, o, H, W, st, mis_mask); }));
			}
			RUN(rstage(sc.subpixel, [&](float *o) {
				const int64_t sd = hwd ? 1 : HW, sp = hwd ? ds : 1;
				return subpixel_mirrored(d, cur[1], o, D, H, W, sd, sp, st);
			}));
			RUN(rstage(sc.median, [&](float *o) { return median2d(d, o, H, W, p->median_k, st); }));
			if (sc.bilateral) {
				const float *gk = nullptr;
				RUN(gaussian_cached(p->blur_sigma, gk));
				RUN(rstage(true, [&](float *o) { return mean2d(d, gk, o, H, W, gaussian_ks(p->blur_sigma), p->blur_t, st); }));
			}
			RUN(mirror_rows(d, ex.dispR, H, W, st));
		}
	}
	tm.mark(MC_STAGE_POST);
#undef RUN
#undef MC_HIP
	return 0;
}

}  // namespace mc
