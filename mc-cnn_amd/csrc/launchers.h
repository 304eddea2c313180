// Every host function of libmcadcensus.so that one unit defines and another calls, declared once.  Every unit includes this,
// the defining one too, so the compiler sees each declaration next to its definition.  Default arguments live here only.
#pragma once
#include "cbca_common.h"

#include <mutex>
#include <vector>

namespace mc {

// post.hip
int fill_nan(float *p, int64_t n, hipStream_t st);
int scale(const float *in, float *out, int64_t n, float s, hipStream_t st);
int transpose(const float *in, float *out, int64_t R, int64_t Cn, int64_t ldin, int64_t ldout, float s, hipStream_t st, int nt = -1);
int fix_border(float *vol, int D, int H, int W, int n, int direction, hipStream_t st);
int argmin_dhw(const float *vol, float *out, int D, int H, int W, int base1, hipStream_t st);
// mc_cost_margins: argmin_dhw's kernels (base1 = 0) with up to three (H,W) maps of the cost curve beside the arg-min d1 -- its minimum c1, the
// smallest value at another d (c2) and the smallest local minimum at another d (c2l); any may be null, not all four.  (A name of its own, as
// subpixel_conf below: the host checks of predict.hip define argmin_dhw as it stands above.)
int cost_margins_dhw(const float *vol, float *d1, float *c1, float *c2, float *c2l, int D, int H, int W, hipStream_t st);
int outlier_detection(const float *d0, const float *d1, float *outlier, int H, int W, int disp_max, hipStream_t st);
// mask: one bit per pixel, set where outlier == 2 (word p >> 5, bit p & 31 of the flat pixel index p; (H*W + 31) / 32 words): written by
// interpolate_occlusion, read by interpolate_mismatch, which walks its rays on an LDS copy of it where the image has at most 524288 pixels
constexpr int MC_MIS_MASK_MAX_PIXELS = 524288;   // a 64 KiB mask
int interpolate_occlusion(const float *d0, const float *outlier, float *out, int H, int W, hipStream_t st, unsigned *mask = nullptr);
int interpolate_mismatch(const float *d0, const float *outlier, float *out, int H, int W, hipStream_t st, const unsigned *mask = nullptr);
int subpixel(const float *d0, const float *vol, float *out, int D, int H, int W, int64_t sd, int64_t sp, hipStream_t st);
// subpixel with the stage's two confidence maps, (H,W) each, either may be null: cost_out = c(d), curv_out = 2 (cp + cn - 2 cz), 0 where d has no
// two neighbours.  subpixel is this with both null: the same kernel, which then loads and stores nothing more.  (A name of its own, no default
// arguments on subpixel: the host checks of predict.hip define subpixel as it stands above.)
int subpixel_conf(const float *d0, const float *vol, float *out, int D, int H, int W, int64_t sd, int64_t sp, hipStream_t st, float *cost_out,
                  float *curv_out);
// The mirror M of mc_predict_views, out[y, W-1-x] = in[y, x] (scale_kernel's mirrored form; in and out must not overlap), and the sub-pixel stage
// on M(vol) without a mirrored volume: out[y, x] from d0[y, x] and the costs of pixel (y, W-1-x) (subpixel_kernel's mirrored form).  Names of
// their own for the reason given above: predict.hip re-declares the two weak and refuses a right view without them.
int mirror_rows(const float *in, float *out, int H, int W, hipStream_t st);
int subpixel_mirrored(const float *d0, const float *vol, float *out, int D, int H, int W, int64_t sd, int64_t sp, hipStream_t st);
int median2d(const float *img, float *out, int H, int W, int k, hipStream_t st);
int mean2d(const float *img, const float *kernel, float *out, int H, int W, int ks, float alpha2, hipStream_t st);
int normalize_forward(const float *in, float *norm, float *out, int N, int C, int H, int W, hipStream_t st);

// stereo_join.hip
int stereo_join_dhw(const float *fL, const float *fR, float *volL, float *volR, int C, int D, int H, int W, hipStream_t st);
int stereo_join_hwd(const float *fL, const float *fR, float *volL, float *volR, int C, int D, int ds, int H, int W, int n, hipStream_t st,
                    int sides = 3);   // bit 0: the left volume, bit 1: the right one
int ad_tiled(const float *x0, const float *x1, float *vol, int D, int H, int W, int direction, hipStream_t st);
size_t census_scratch_bytes(int Cimg, int H, int W);
int census_sig(const float *x0, const float *x1, float *vol, void *scratch, int Cimg, int D, int H, int W, int direction, hipStream_t st);

// cbca.hip
int cross(const float *img, float *arms, int H, int W, int L1, float tau1, hipStream_t st);
int cbca(const float *x0c, const float *x1c, const float *vin, float *vout, int D, int H, int W, int direction, hipStream_t st);
size_t cbca_scratch_bytes(int H, int W);   // what cbca_scratch() (cbca_common.h) lays out
int cbca_pack(const float *x0c, const float *x1c, void *scratch, int H, int W, hipStream_t st);
int cbca_if_overflow(const float *x0c, const float *x1c, const void *packed, const float *vin, float *vout, int D, int H, int W, int direction, hipStream_t st);
int cbca_strips(const void *packed, const float *vin, float *vout, int D, int H, int W, int direction, int route,
                hipStream_t st, const CbcaCfg &cfg = CbcaCfg());
bool packed_dims_ok(int H, int W);
int cbca_by_arms(const void *packed, const float *vin, float *vout, int D, int H, int W, int direction, int max_arm, hipStream_t st,
                 const CbcaCfg &cfg = CbcaCfg());

// cbca_tile.hip
size_t cbca_plan_bytes(int D, int H, int W);
int cbca_tiles(const void *packed, const float *vin, float *vout, int D, int H, int W, int direction, int arm_class, int route,
               hipStream_t st, const CbcaCfg &cfg = CbcaCfg());

// cbca_lean.hip
int cbca_lean_rows(int D, int H, int W, int rb, bool two_pass);
size_t cbca_lean2x_bytes(int D, int H, int W);   // what the texture route's two-pass records take of the plan area
bool cbca_lean_fits(int D, int H, int W, size_t plan_bytes, bool two_pass = false, int rb = 0);
int cbca_classify(const void *packed, void *plan, size_t plan_bytes, int D, int H, int W, int direction, int route, int rb, int cap_limit,
                  hipStream_t st, bool two_pass = false, float cost_limit = 0);
int cbca_lean2x(const void *packed, const void *plan, size_t plan_bytes, const float *vin, float *vout, int D, int H, int W, int direction,
                int route, hipStream_t st, const CbcaCfg &cfg);
int cbca_lean(const void *packed, const void *plan, size_t plan_bytes, const float *vin, float *vout, int D, int H, int W, int direction,
              int route, hipStream_t st, const CbcaCfg &cfg);

// conv3x3.hip
size_t conv3x3_workspace_bytes(int Cin, int Cout);
int conv3x3(const float *in, const float *w, const float *bias, float *out, int N, int Cin, int Cout, int H, int W, int relu, void *workspace, hipStream_t st);

// fc_stack.hip
size_t fc_workspace_bytes(int C, int n_hidden, int H, int W);
int fc_stack(const float *featL, const float *featR, int C, int H, int W, int D, const float *const *weights,
             const float *const *biases, int n_layers, float *volL, float *volR, void *workspace, hipStream_t st);

// sgm.hip
size_t sgm_maps_bytes(int H, int W);
int sgm_prep(const float *x0, const float *x1, void *maps, int H, int W, float tau_so, hipStream_t st);
// The maps of a call with D > 512 have wider window rows (sgm_line.h, SGM_PADW_WIDE): the two functions above are these at any D <= 512, where
// size and layout are what they always were.  (predict.hip re-declares the two weak for itself: it asks them only where D > 512, and the host
// check of the two lanes links it against stubs of the two functions above alone.)
size_t sgm_maps_bytes_d(int H, int W, int D);
int sgm_prep_d(const float *x0, const float *x1, void *maps, int H, int W, int D, float tau_so, hipStream_t st);
int sgm_contract_violations(const float *vol, int H, int W, int D, unsigned *count, hipStream_t st);
int sgm_sweeps(const float *const C[2], float *const out[2], float *const out2[2], float *const disp[2],
               const int direction[2], int nvol, int H, int W, int D, int ds, const void *maps, float pi1, float pi2,
               float alpha1, float q1, float q2, bool fused, unsigned drop_final, bool tri, hipStream_t st);
// sgm_sweeps for a caller that has checkpoint slots: ck[v] (sgm_ck_bytes, 16-byte aligned) belongs to volume v, or ck is null.  With slots, fused,
// D <= 256 and volumes below 2 GiB, the vertical launches recompute the down pass: L_down is kept at every SGM_CK_ROWS-th row only, in ck[v].
// sgm_sweeps is this with ck = null.  Declared weak: a program that links predict.hip without sgm.hip behind a stub of sgm_sweeps (the host check
// of the two lanes) has no definition, and predict_impl then calls sgm_sweeps.
constexpr int SGM_CK_ROWS = 8;
static inline size_t sgm_ck_bytes(int H, int W, int ds) { return ((size_t)((H + SGM_CK_ROWS - 1) / SGM_CK_ROWS) * W * ds * sizeof(float) + 255) / 256 * 256; }
int sgm_sweeps_ck(const float *const C[2], float *const out[2], float *const out2[2], float *const disp[2],
                  const int direction[2], int nvol, int H, int W, int D, int ds, const void *maps, float pi1, float pi2,
                  float alpha1, float q1, float q2, bool fused, unsigned drop_final, bool tri, float *const ck[2], hipStream_t st) __attribute__((weak));
int sgm_vertical(int set = -1);   // set 1 / 2: force the two-launch / the recomputing form where it applies (the tests), 0: back to the default (2); returns the one in force

// predict.hip
static inline int gaussian_ks(double sigma) { return 2 * (int)ceil(sigma * 3) + 1; }   // main.lua:529-530
void gaussian_fill(double sigma, float *k);

// mc_predict's workspace (make_plan): its size and, for a given base, its areas in the order they lie there
struct Plan {
	int Dp;                 // padded pixel stride of the (H,W,Dp) volumes
	size_t cplan_bytes;     // per direction: the tile kernel's plan (cbca_tile.hip), 0 where it would not be reused
	size_t total;           // what mc_predict needs
	size_t total_ck;        // ... and with the SGM's checkpoint slots behind it, what it takes to run the recomputing vertical launches
	void *maps, *packed;
	float *x0c, *x1c, *img[6], *gk;   // gk: unused (the Gaussian table has its own device memory); kept so that the layout stays
	float *bufA[2], *bufB[2], *bufC[2];   // ping-pong per side; bufC: scratch of the SGM's concurrent second direction and of pairs of CBCA passes
	void *cplan[2];             // null where the direction has none
	float *ck[2];               // the SGM's checkpoint rows of the left and of the right volume (sgm_ck_bytes each): behind `total`, there in a workspace of total_ck bytes
};
Plan make_plan(const mc_params *p, int D, int H, int W, void *base = nullptr);

// the fast path's two lanes: MC_PREDICT_LANES (1 or 2, default 2), and what a caller's stream keeps for its right lane
int parse_predict_lanes(const char *s);
int predict_lanes(int set = -1, bool *is_forced = nullptr);   // set 1 / 2: force that schedule (the tests), 0: back to the environment's; returns the one in force
struct Lanes {
	hipStream_t side = nullptr;
	hipEvent_t fork = nullptr, join_left = nullptr, right_done = nullptr;
	std::mutex mu;
};

struct StageTimer {   // mc_predict_timed: an event at every stage boundary
	bool on = false;
	hipStream_t st;
	std::vector<hipEvent_t> ev;
	std::vector<int> tag;  // stage id the interval ENDING at this event belongs to
	void mark(int stage);
	void collect(float out[MC_N_STAGES]);
};
// mc_predict_ex's optional (H,W) maps: the LR check's classes (0 match, 1 occlusion, 2 mismatch), and the sub-pixel stage's cost at the
// disparity it reads and the curvature of the cost curve there
// ... and mc_predict_views' two (H,W) maps of the RIGHT view: its finished disparity map and its classes (predict.hip, the right tail)
struct PredictExtras { float *outlier = nullptr, *cost = nullptr, *curv = nullptr, *dispR = nullptr, *outlierR = nullptr; };
int predict_impl(const mc_params *p, const float *x0, const float *x1, const float *featL, const float *featR, int C,
                 const float *rawL, const float *rawR, int D, int H, int W, void *workspace, size_t workspace_bytes,
                 float *volL_out, float *volR_out, float *dispL0_out, float *dispR0_out, float *disp_out, hipStream_t st,
                 StageTimer &tm, const PredictExtras &ex = PredictExtras());

}  // namespace mc
