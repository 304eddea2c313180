// Host check of mc_predict's two-lane schedule (mc-cnn_amd/csrc/predict.hip).  tests/test_predict_lanes_host.py builds the host side of
// predict.hip and error.hip together with this file, with the address and undefined-behaviour sanitizers, and runs the program: no GPU and
// no HIP runtime is involved.  Every launcher predict_impl calls and every HIP call it makes is a stub below that writes one line
// "<stream> <what>" into a log, so that the order of launches, records and waits per stream can be read back; a stub can be told to fail.
#include "../mc-cnn_amd/csrc/launchers.h"

#include <string.h>

#include <string>
#include <thread>

using namespace mc;

// ---- the log -------------------------------------------------------------------------------------------------------------------
struct Entry { const void *stream; std::string what; };
static std::mutex g_mu;
static std::vector<Entry> g_log;
static int g_streams_made = 0, g_events_made = 0, g_streams_destroyed = 0, g_events_destroyed = 0, g_timer_events = 0;
static thread_local int t_calls = 0, t_fail_at = -1;   // the t_fail_at-th stub call of this thread fails (0-based)
static const int FAIL = 77;

static int note(const void *stream, const std::string &what)
{
	std::lock_guard<std::mutex> lk(g_mu);
	g_log.push_back({stream, what});
	return t_calls++ == t_fail_at ? FAIL : 0;
}
static std::string ptr(const void *p) { char b[32]; snprintf(b, sizeof b, "%p", p); return b; }

// ---- HIP stubs -----------------------------------------------------------------------------------------------------------------
// (an executable's own definitions come before those of any shared library the compiler driver links)
extern "C" {
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stub error"; }
hipError_t hipMalloc(void **p, size_t n) { static float table[4096]; *p = n <= sizeof table ? table : nullptr; return *p ? hipSuccess : hipErrorOutOfMemory; }   // (the Gaussian table, once)
hipError_t hipFree(void *) { return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags)
{
	if (flags != hipStreamNonBlocking) return hipErrorInvalidValue;
	std::lock_guard<std::mutex> lk(g_mu);
	++g_streams_made;
	*s = (hipStream_t)malloc(1);
	return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { std::lock_guard<std::mutex> lk(g_mu); ++g_streams_destroyed; free(s); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
	if (flags != hipEventDisableTiming) return hipErrorInvalidValue;
	std::lock_guard<std::mutex> lk(g_mu);
	++g_events_made;
	*e = (hipEvent_t)malloc(1);
	return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { std::lock_guard<std::mutex> lk(g_mu); ++g_timer_events; *e = (hipEvent_t)malloc(1); return hipSuccess; }   // (the StageTimer's)
hipError_t hipEventDestroy(hipEvent_t e) { std::lock_guard<std::mutex> lk(g_mu); ++g_events_destroyed; free(e); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { return note(s, "record " + ptr(e)) ? hipErrorUnknown : hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { return note(s, "wait " + ptr(e)) ? hipErrorUnknown : hipSuccess; }
}

// ---- launcher stubs ------------------------------------------------------------------------------------------------------------
namespace mc {
size_t sgm_maps_bytes(int H, int W) { return (size_t)H * W * 12; }
size_t cbca_scratch_bytes(int H, int W) { return (size_t)H * W * 4; }
size_t cbca_plan_bytes(int D, int H, int W) { return (size_t)D * H * W * 4; }
bool packed_dims_ok(int, int) { return true; }
bool cbca_lean_fits(int, int, int, size_t, bool, int) { return false; }
int fill_nan(float *, int64_t, hipStream_t s) { return note(s, "fill_nan"); }
int scale(const float *, float *out, int64_t, float, hipStream_t s) { return note(s, "scale -> " + ptr(out)); }
int transpose(const float *, float *out, int64_t, int64_t, int64_t, int64_t, float, hipStream_t s, int) { return note(s, "transpose -> " + ptr(out)); }
int fix_border(float *, int, int, int, int, int, hipStream_t s) { return note(s, "fix_border"); }
int argmin_dhw(const float *, float *, int, int, int, int, hipStream_t s) { return note(s, "argmin"); }
int outlier_detection(const float *, const float *d1, float *, int, int, int, hipStream_t s) { return note(s, "outlier_detection d1 " + ptr(d1)); }
int interpolate_occlusion(const float *, const float *, float *, int, int, hipStream_t s, unsigned *) { return note(s, "interpolate_occlusion"); }
int interpolate_mismatch(const float *, const float *, float *, int, int, hipStream_t s, const unsigned *) { return note(s, "interpolate_mismatch"); }
int subpixel(const float *, const float *, float *, int, int, int, int64_t, int64_t, hipStream_t s) { return note(s, "subpixel"); }
int median2d(const float *, float *, int, int, int, hipStream_t s) { return note(s, "median2d"); }
int mean2d(const float *, const float *, float *, int, int, int, float, hipStream_t s) { return note(s, "mean2d"); }
int stereo_join_dhw(const float *, const float *, float *, float *, int, int, int, int, hipStream_t s) { return note(s, "stereo_join_dhw"); }
int stereo_join_hwd(const float *, const float *, float *, float *, int, int, int, int, int, int, hipStream_t s, int sides)
{
	return note(s, "stereo_join_hwd sides " + std::to_string(sides));
}
int cross(const float *, float *, int, int, int, float, hipStream_t s) { return note(s, "cross"); }
int cbca(const float *, const float *, const float *, float *, int, int, int, int, hipStream_t s) { return note(s, "cbca"); }
int cbca_pack(const float *, const float *, void *, int, int, hipStream_t s) { return note(s, "cbca_pack"); }
int cbca_by_arms(const void *, const float *, float *, int, int, int, int, int, hipStream_t s, const CbcaCfg &) { return note(s, "cbca_by_arms"); }
int cbca_classify(const void *, void *, size_t, int, int, int, int, int, int, int, hipStream_t s, bool, float) { return note(s, "cbca_classify"); }
int cbca_lean2x(const void *, const void *, size_t, const float *, float *, int, int, int, int, int, hipStream_t s, const CbcaCfg &) { return note(s, "cbca_lean2x"); }
int sgm_prep(const float *, const float *, void *, int, int, float, hipStream_t s) { return note(s, "sgm_prep"); }
int sgm_sweeps(const float *const C[2], float *const out[2], float *const out2[2], float *const disp[2], const int direction[2], int nvol,
               int, int, int, int, const void *, float, float, float, float, float, bool, unsigned drop_final, bool tri, hipStream_t s)
{
	std::string w = "sgm_sweeps nvol " + std::to_string(nvol) + " drop " + std::to_string(drop_final) + " tri " + std::to_string((int)tri);
	for (int v = 0; v < nvol; ++v)
		w += " [dir " + std::to_string(direction[v]) + " C " + ptr(C[v]) + " out " + ptr(out[v]) + " out2 " + ptr(out2[v]) + " disp " + ptr(disp ? disp[v] : nullptr) + "]";
	return note(s, w);
}
}  // namespace mc

// ---- the checks ----------------------------------------------------------------------------------------------------------------
static int g_failed = 0, g_checked = 0;
#define CHECK(cond) do { ++g_checked; if (!(cond)) { ++g_failed; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

static mc_params kitti_fast()
{
	mc_params p;
	memset(&p, 0, sizeof p);
	p.L1 = 0; p.cbca_i1 = 0; p.cbca_i2 = 0; p.tau1 = 0;
	p.pi1 = 4; p.pi2 = 55.72f; p.sgm_i = 1; p.sgm_q1 = 3; p.sgm_q2 = 2.5f; p.alpha1 = 1.5f; p.tau_so = 0.02f;
	p.blur_sigma = 7.74; p.blur_t = 5; p.lr_check = 1; p.border_n = 4; p.median_k = 5;
	return p;
}

struct Call {
	mc_params p = kitti_fast();
	int C = 64, D = 20, H = 9, W = 40;
	bool feat = true, want_vol = false, want_disp0 = false, timed = false;
	hipStream_t st = (hipStream_t)0x1000;
	std::vector<char> ws;
	void *base = nullptr;
	size_t bytes = 0;
	float *volL = (float *)0x10, *volR = (float *)0x20, *dL = (float *)0x30, *dR = (float *)0x40;
	int run()
	{
		bytes = make_plan(&p, D, H, W).total;
		ws.resize(bytes + 256);
		base = (void *)(((uintptr_t)ws.data() + 255) / 256 * 256);
		const float *x = (const float *)0x100;   // never dereferenced: every launcher is a stub
		StageTimer tm;
		tm.on = timed;
		tm.st = st;
		const int rc = predict_impl(&p, x, x, feat ? x : nullptr, feat ? x : nullptr, C, feat ? nullptr : x, feat ? nullptr : x, D, H, W, base, bytes,
		                            want_vol ? volL : nullptr, want_vol ? volR : nullptr, want_disp0 ? dL : nullptr, want_disp0 ? dR : nullptr,
		                            (float *)0x50, st, tm);
		float ms[MC_N_STAGES];
		if (timed) tm.collect(ms);
		return rc;
	}
};

static std::vector<Entry> take_log()
{
	std::lock_guard<std::mutex> lk(g_mu);
	std::vector<Entry> l;
	l.swap(g_log);
	return l;
}
static int find(const std::vector<Entry> &l, const std::string &prefix, const void *stream, int from = 0)
{
	for (int i = from; i < (int)l.size(); ++i)
		if (l[i].stream == stream && l[i].what.compare(0, prefix.size(), prefix) == 0) return i;
	return -1;
}
static bool has_waits(const std::vector<Entry> &l)
{
	for (const Entry &e : l)
		if (e.what.compare(0, 5, "wait ") == 0) return true;
	return false;
}
static bool has_event_ops(const std::vector<Entry> &l)
{
	for (const Entry &e : l)
		if (e.what.compare(0, 7, "record ") == 0 || e.what.compare(0, 5, "wait ") == 0) return true;
	return false;
}

// a two-lane call's log: the order the issue of the schedule rests on
static void check_two_lane_log(const std::vector<Entry> &l, const Call &c, int n_sgm)
{
	const void *st = c.st;
	const void *side = nullptr;
	for (const Entry &e : l) if (e.stream != st) { side = e.stream; break; }
	CHECK(side != nullptr);
	for (const Entry &e : l) CHECK(e.stream == st || e.stream == side);
	const Plan pl = make_plan(&c.p, c.D, c.H, c.W, c.base);
	// lane A up to the fork and the left join
	CHECK(l[0].stream == st && l[0].what == "sgm_prep");
	CHECK(l[1].stream == st && l[1].what.compare(0, 7, "record ") == 0);
	const std::string ev_fork = l[1].what.substr(7);
	CHECK(l[2].stream == st && l[2].what == "stereo_join_hwd sides 1");
	CHECK(l[3].stream == st && l[3].what.compare(0, 7, "record ") == 0);
	const std::string ev_join_left = l[3].what.substr(7);
	CHECK(ev_fork != ev_join_left);
	// lane B: both waits in front of everything else it does, then join(right), its sweeps, its exports, the last record
	std::vector<std::string> b;
	for (const Entry &e : l) if (e.stream == side) b.push_back(e.what);
	size_t i = 0;
	CHECK(b.size() >= 4 && b[i++] == "wait " + ev_fork);
	CHECK(b[i++] == "wait " + ev_join_left);
	CHECK(b[i++] == "stereo_join_hwd sides 2");
	for (int it = 0; it < n_sgm; ++it, ++i) {
		const bool last = it == n_sgm - 1;
		const float *Cin = it % 2 ? pl.bufB[1] : pl.bufA[1], *out = it % 2 ? pl.bufA[1] : pl.bufB[1];
		const std::string want = "sgm_sweeps nvol 1 drop " + std::to_string(last && !c.want_vol ? 1 : 0) + " tri 1 [dir 1 C " + ptr(Cin) + " out " + ptr(out) +
		                         " out2 " + ptr(pl.bufC[1]) + " disp " + ptr(last ? pl.img[1] : nullptr) + "]";
		CHECK(i < b.size() && b[i] == want);
	}
	if (c.want_vol) CHECK(i < b.size() && b[i++] == "transpose -> " + ptr(c.volR));
	if (c.want_disp0) CHECK(i < b.size() && b[i++] == "scale -> " + ptr(c.dR));
	CHECK(i + 1 == b.size() && b[i].compare(0, 7, "record ") == 0);
	const std::string ev_done = b.back().substr(7);
	CHECK(ev_done != ev_fork && ev_done != ev_join_left);
	// lane A: the left sweeps alone, its exports, then the wait, and only then the LR check on the right arg-min
	std::vector<std::string> a;
	for (size_t k = 4; k < l.size(); ++k) if (l[k].stream == st) a.push_back(l[k].what);
	i = 0;
	for (int it = 0; it < n_sgm; ++it, ++i) {
		const bool last = it == n_sgm - 1;
		const float *Cin = it % 2 ? pl.bufB[0] : pl.bufA[0], *out = it % 2 ? pl.bufA[0] : pl.bufB[0];
		const std::string want = "sgm_sweeps nvol 1 drop 0 tri 1 [dir -1 C " + ptr(Cin) + " out " + ptr(out) + " out2 " + ptr(pl.bufC[0]) + " disp " +
		                         ptr(last ? pl.img[0] : nullptr) + "]";
		CHECK(i < a.size() && a[i] == want);
	}
	if (c.want_vol) CHECK(a[i++] == "transpose -> " + ptr(c.volL));
	if (c.want_disp0) CHECK(a[i++] == "scale -> " + ptr(c.dL));
	CHECK(a[i++] == "wait " + ev_done);
	CHECK(a[i++] == "outlier_detection d1 " + ptr(pl.img[1]));
	CHECK(a.back() == "mean2d");
	for (; i < a.size(); ++i) CHECK(a[i].compare(0, 7, "record ") != 0 && a[i].compare(0, 5, "wait ") != 0);
	// in the order of the calls: the record of right_done comes before the wait for it
	CHECK(find(l, "record " + ev_done, side) < find(l, "wait " + ev_done, st));
}

int main()
{
	// ---- the switch ----
	CHECK(parse_predict_lanes(nullptr) == 2);
	CHECK(parse_predict_lanes("") == 2);
	CHECK(parse_predict_lanes("1") == 1);
	CHECK(parse_predict_lanes("2") == 2);
	CHECK(parse_predict_lanes("0") == 2);
	CHECK(parse_predict_lanes("11") == 2);
	CHECK(parse_predict_lanes("1 ") == 2);
	CHECK(parse_predict_lanes(" 1") == 2);
	CHECK(parse_predict_lanes("one") == 2);
	setenv("MC_PREDICT_LANES", "2", 1);
	bool forced = true;
	CHECK(predict_lanes(-1, &forced) == 2 && !forced);   // read here, once
	setenv("MC_PREDICT_LANES", "1", 1);
	CHECK(predict_lanes() == 2);              // ... and not again
	CHECK(predict_lanes(1) == 1 && predict_lanes() == 1);
	CHECK(predict_lanes(7) == 1 && predict_lanes(-5) == 1);   // not a setting: ignored
	CHECK(predict_lanes(0) == 2);             // back to the environment's
	CHECK(predict_lanes(1, &forced) == 1 && forced);

	// ---- one lane: today's order, no stream, no event ----
	{
		Call c;
		CHECK(c.run() == 0);
		const auto l = take_log();
		CHECK(!has_event_ops(l) && g_streams_made == 0 && g_events_made == 0);
		CHECK(l.size() == 9 && l[0].what == "sgm_prep" && l[1].what == "stereo_join_hwd sides 3");
		CHECK(l[2].what.find("sgm_sweeps nvol 2 drop 2 tri 1 [dir -1 ") == 0 && l[2].what.find("] [dir 1 ") != std::string::npos);
		for (const Entry &e : l) CHECK(e.stream == c.st);
	}
	predict_lanes(2);

	// ---- refusals in front of the first launch: nothing logged, nothing created ----
	{
		Call c;
		c.D = 0; CHECK(c.run() == MC_EINVAL); c.D = 20;
		c.D = MC_SGM_MAX_D + 1; CHECK(c.run() == MC_EINVAL); c.D = 20;
		c.C = MC_JOIN_MAX_C + 1; CHECK(c.run() == MC_EINVAL); c.C = 64;
		c.C = 0; CHECK(c.run() == MC_EINVAL); c.C = 64;
		c.p.sgm_i = -1; CHECK(c.run() == MC_EINVAL); c.p.sgm_i = 1;
		c.p.median_k = 4; CHECK(c.run() == MC_EINVAL); c.p.median_k = 5;
		c.p.border_n = c.W; CHECK(c.run() == MC_EINVAL); c.p.border_n = 4;
		c.p.sm_skip = 9; CHECK(c.run() == MC_EINVAL); c.p.sm_skip = 0;
		CHECK(c.run() == 0);
		take_log();
		const int s0 = g_streams_made, e0 = g_events_made;
		StageTimer tm;
		const float *x = (const float *)0x100;
		CHECK(predict_impl(&c.p, x, x, x, x, 64, nullptr, nullptr, c.D, c.H, c.W, c.base, c.bytes - 1, nullptr, nullptr, nullptr, nullptr, (float *)0x50, c.st, tm) == MC_EINVAL);
		CHECK(strstr(last_error(), "workspace") != nullptr);
		CHECK(predict_impl(&c.p, x, x, x, x, 64, nullptr, nullptr, c.D, c.H, c.W, (char *)c.base + 16, c.bytes, nullptr, nullptr, nullptr, nullptr, (float *)0x50, c.st, tm) == MC_EINVAL);
		CHECK(predict_impl(&c.p, x, x, x, x, 64, nullptr, nullptr, c.D, c.H, c.W, nullptr, c.bytes, nullptr, nullptr, nullptr, nullptr, (float *)0x50, c.st, tm) == MC_EINVAL);
		CHECK(predict_impl(&c.p, x, x, x, x, 64, nullptr, nullptr, c.D, c.H, c.W, c.base, c.bytes, nullptr, nullptr, nullptr, nullptr, nullptr, c.st, tm) == MC_EINVAL);
		CHECK(take_log().empty() && g_streams_made == s0 && g_events_made == e0);
	}

	// ---- two lanes: the schedule, with and without exports, one and two SGM iterations; the cache ----
	{
		const int s0 = g_streams_made, e0 = g_events_made;
		for (int variant = 0; variant < 8; ++variant) {
			Call c;
			c.want_vol = variant & 1; c.want_disp0 = variant & 2; c.p.sgm_i = variant & 4 ? 2 : 1;
			c.st = (hipStream_t)0x2000;
			CHECK(c.run() == 0);
			check_two_lane_log(take_log(), c, c.p.sgm_i);
		}
		CHECK(g_streams_made == s0 + 1 && g_events_made == e0 + 3);   // one miss, seven hits
		Call c;
		c.st = nullptr;   // the null stream is a key like any other
		CHECK(c.run() == 0);
		check_two_lane_log(take_log(), c, 1);
		CHECK(g_streams_made == s0 + 2 && g_events_made == e0 + 6);
	}

	// ---- configurations that keep one lane whatever the switch says ----
	{
		const int s0 = g_streams_made;
		Call c;
		c.timed = true; CHECK(c.run() == 0); CHECK(!has_waits(take_log())); c.timed = false;                      // mc_predict_timed (records its stage marks, waits for nothing)
		c.feat = false; CHECK(c.run() == 0); CHECK(!has_event_ops(take_log())); c.feat = true;                    // raw volumes
		c.C = 112; CHECK(c.run() == 0); CHECK(!has_event_ops(take_log())); c.C = 64;                              // C > 64
		c.p.lr_check = 0; c.p.left_only = 1; CHECK(c.run() == 0); CHECK(!has_event_ops(take_log()));              // the left volume only
		c.want_disp0 = true; CHECK(c.run() == 0); CHECK(has_event_ops(take_log())); c.want_disp0 = false;         // ... unless the right one is asked for
		c.p.lr_check = 1; c.p.left_only = 0;
		c.p.sm_skip = MC_SKIP_SGM; CHECK(c.run() == 0); CHECK(!has_event_ops(take_log())); c.p.sm_skip = 0;
		c.p.sm_terminate = MC_SM_CNN; CHECK(c.run() == 0); CHECK(!has_event_ops(take_log())); c.p.sm_terminate = 0;
		c.p.cbca_i1 = 2; c.p.L1 = 5; CHECK(c.run() == 0); CHECK(!has_event_ops(take_log())); c.p.cbca_i1 = 0;     // CBCA-1
		c.p.cbca_i2 = 2; CHECK(c.run() == 0); CHECK(!has_event_ops(take_log())); c.p.cbca_i2 = 0; c.p.L1 = 0;     // CBCA-2
		c.p.sm_terminate = MC_SM_SGM; CHECK(c.run() == 0); CHECK(has_event_ops(take_log())); c.p.sm_terminate = 0;   // stays in the branch: two lanes
		CHECK(g_streams_made == s0);   // (this caller stream has its side stream since the block before last)
	}

	// ---- a failure at every position of a two-lane call: the caller's stream ends behind the right lane ----
	{
		Call c;
		c.want_vol = c.want_disp0 = true;
		c.st = (hipStream_t)0x3000;
		CHECK(c.run() == 0);
		const int n = (int)take_log().size();
		CHECK(n > 15);
		for (int f = 0; f < n; ++f) {
			t_calls = 0; t_fail_at = f;
			const int rc = c.run();
			t_fail_at = -1;
			CHECK(rc != 0);
			const auto l = take_log();
			CHECK((int)l.size() >= f + 1);
			const void *side = nullptr;
			for (const Entry &e : l) if (e.stream != c.st) side = e.stream;
			if (!side) { CHECK((int)l.size() == f + 1); continue; }   // failed in front of the fork's first wait: nothing more was queued
			// something was queued on the side stream: after the failing call come exactly the record on the side stream and the wait
			// for it on the caller's (or, where one of these two is what failed, what is left of them)
			const int last_rec = [&] { int k = -1; for (int i = 0; i < (int)l.size(); ++i) if (l[i].stream == side && l[i].what.compare(0, 7, "record ") == 0) k = i; return k; }();
			CHECK(last_rec >= 0);
			if (last_rec < 0) continue;
			const std::string ev = l[last_rec].what.substr(7);
			for (int i = last_rec + 1; i < (int)l.size(); ++i) CHECK(l[i].stream != side);   // nothing on the side stream behind its record
			if (last_rec == f) { CHECK((int)l.size() == f + 1); continue; }   // the record itself failed: the call reports that and stops
			const int w = find(l, "wait " + ev, c.st, last_rec);
			CHECK(w > last_rec);
			if (w > f) CHECK(last_rec == f + 1 && w == f + 2 && (int)l.size() == f + 3);   // the failed call, then the record and the wait, then nothing
			else CHECK((int)l.size() == f + 1);                                            // the lanes had met before the failure
		}
		t_calls = 0;
		CHECK(c.run() == 0);   // and the entry's lock was released every time
		take_log();
	}

	// ---- not forced: once a second caller stream has appeared the device keeps one lane, and the idle side streams are released ----
	int released = 0;
	{
		predict_lanes(0);
		const hipStream_t a = (hipStream_t)0x4000, b = (hipStream_t)0x5000;
		const hipStream_t order[6] = {a, a, b, b, a, a};
		for (int i = 0; i < 6; ++i) {
			Call c;
			c.st = order[i];
			CHECK(c.run() == 0);
			const auto l = take_log();
			const bool want_two = i < 2;
			CHECK(has_event_ops(l) == want_two);
			if (want_two) { check_two_lane_log(l, c, 1); released = g_streams_made; CHECK(g_streams_destroyed == 0); }
			else for (const Entry &e : l) CHECK(e.stream == c.st);
			if (!want_two) CHECK(g_streams_destroyed == released && g_streams_made == released);   // every one was idle; none is made any more
		}
		predict_lanes(2);
	}

	// ---- several threads: hits and misses at once ----
	{
		const int s0 = g_streams_made, e0 = g_events_made;
		const int T = 8, K = 4, N = 40;
		std::vector<std::thread> th;
		std::vector<int> bad(T, 0);
		for (int t = 0; t < T; ++t)
			th.emplace_back([&, t] {
				for (int i = 0; i < N; ++i) {
					Call c;
					c.st = (hipStream_t)(uintptr_t)(0x10000 + 0x100 * ((t + i) % K));
					c.H = 3; c.W = 33; c.D = 16;
					if (c.run() != 0) ++bad[t];
				}
			});
		for (auto &t : th) t.join();
		for (int t = 0; t < T; ++t) CHECK(bad[t] == 0);
		CHECK(g_streams_made == s0 + K && g_events_made == e0 + 3 * K);
		// per caller stream: between a fork and the wait that ends the call, no other call's record or wait on the same pair of streams
		const auto l = take_log();
		for (int k = 0; k < K; ++k) {
			const void *st = (const void *)(uintptr_t)(0x10000 + 0x100 * k);
			int open = 0, calls = 0;
			std::string ev_fork;
			for (const Entry &e : l) {
				if (e.stream != st) continue;
				if (e.what == "sgm_prep") ++calls;
				if (e.what.compare(0, 7, "record ") == 0) { if (ev_fork.empty()) ev_fork = e.what; if (e.what == ev_fork) { CHECK(open == 0); open = 1; } }
				if (e.what.compare(0, 5, "wait ") == 0) { CHECK(open == 1); open = 0; }
			}
			CHECK(open == 0 && calls == T * N / K);
		}
	}
	CHECK(g_streams_destroyed == released && g_events_destroyed == g_timer_events + 3 * released);   // the rest is kept (the StageTimer's events are its own)
	printf("%d %d\n", g_checked, g_failed);
	return g_failed ? 1 : 0;
}
