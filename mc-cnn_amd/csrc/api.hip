// extern "C" surface of libmcadcensus.so (see include/mc_adcensus.h); the fused pipeline behind mc_predict is predict.hip.
#include "launchers.h"

using namespace mc;

#define MC_REQUIRE_DIRECTION(name, direction) MC_REQUIRE((direction) == -1 || (direction) == 1, name ": direction must be -1 or 1")

// the plan / list area the test hook keeps behind the packed lengths in its scratch
struct PlanArea { size_t off, bytes; };
static PlanArea plan_area(int D, int H, int W) { return {align_up(cbca_scratch_bytes(H, W), 256), cbca_plan_bytes(D, H, W)}; }

extern "C" {

int mc_version(void) { return MC_ABI_VERSION; }
const char *mc_last_error(void) { return last_error(); }

int mc_fill_nan(float *p, int64_t n, void *stream)
{
	MC_REQUIRE(p || n == 0, "mc_fill_nan: null pointer");
	MC_REQUIRE(n >= 0, "mc_fill_nan: negative size");
	return fill_nan(p, n, as_stream(stream));
}

int mc_stereo_join(const float *featL, const float *featR, float *volL, float *volR, int C, int D, int H, int W, void *stream)
{
	MC_REQUIRE(featL && featR && volL && volR, "mc_stereo_join: null pointer");
	MC_REQUIRE(dims_ok(D, H, W) && C >= 1, "mc_stereo_join: bad dims C=%d D=%d H=%d W=%d", C, D, H, W);
	MC_REQUIRE(C <= MC_JOIN_MAX_C, "mc_stereo_join: C=%d exceeds %d (adcensus.cu:1460)", C, MC_JOIN_MAX_C);
	MC_REQUIRE(D <= 65535, "mc_stereo_join: D too large");
	return stereo_join_dhw(featL, featR, volL, volR, C, D, H, W, as_stream(stream));
}

int mc_ad(const float *x0, const float *x1, float *vol, int D, int H, int W, int direction, void *stream)
{
	MC_REQUIRE(x0 && x1 && vol, "mc_ad: null pointer");
	MC_REQUIRE(dims_ok(D, H, W), "mc_ad: bad dims");
	MC_REQUIRE_DIRECTION("mc_ad", direction);
	MC_REQUIRE(D <= 65535, "mc_ad: D too large");
	return ad_tiled(x0, x1, vol, D, H, W, direction, as_stream(stream));
}

size_t mc_census_scratch_bytes(int Cimg, int H, int W)
{
	if (Cimg < 1 || H < 1 || W < 1) return 0;
	return census_scratch_bytes(Cimg, H, W);
}

int mc_census_ws(const float *x0, const float *x1, float *vol, int Cimg, int D, int H, int W, int direction, void *scratch,
                 size_t scratch_bytes, void *stream)
{
	MC_REQUIRE(x0 && x1 && vol && scratch, "mc_census_ws: null pointer");
	MC_REQUIRE(dims_ok(D, H, W) && Cimg >= 1 && D <= 65535, "mc_census_ws: bad dims");
	MC_REQUIRE_DIRECTION("mc_census_ws", direction);
	MC_REQUIRE(scratch_bytes >= census_scratch_bytes(Cimg, H, W), "mc_census_ws: scratch holds %zu bytes, needs %zu", scratch_bytes,
	           census_scratch_bytes(Cimg, H, W));
	MC_REQUIRE((uintptr_t)scratch % 4 == 0, "mc_census_ws: scratch must be 4-byte aligned");
	return census_sig(x0, x1, vol, scratch, Cimg, D, H, W, direction, as_stream(stream));
}

size_t mc_fc_stack_workspace_bytes(int C, int n_layers, int H, int W)
{
	if (C < 1 || n_layers < 2 || n_layers > 8 || H < 1 || W < 1) return 0;
	return fc_workspace_bytes(C, n_layers - 2, H, W);
}

int mc_fc_stack(const float *featL, const float *featR, int C, int H, int W, int D, const float *const *weights,
                const float *const *biases, const int *layer_out, int n_layers, float *volL, float *volR, void *workspace,
                size_t workspace_bytes, void *stream)
{
	MC_REQUIRE(featL && featR && weights && biases && layer_out && volL && volR && workspace, "mc_fc_stack: null pointer");
	MC_REQUIRE(dims_ok(D, H, W) && C >= 1, "mc_fc_stack: bad dims");
	MC_REQUIRE(n_layers >= 2 && n_layers <= 8, "mc_fc_stack: 2..8 layers supported");
	for (int l = 0; l < n_layers - 1; ++l)
		MC_REQUIRE(layer_out[l] == 384, "mc_fc_stack: hidden width %d not supported (nh2 = 384 in every preset, main.lua:77,124)",
		           layer_out[l]);
	MC_REQUIRE(layer_out[n_layers - 1] == 1, "mc_fc_stack: the last layer must have one output");
	for (int l = 0; l < n_layers; ++l) MC_REQUIRE(weights[l] && biases[l], "mc_fc_stack: null layer %d", l);
	MC_REQUIRE(workspace_bytes >= fc_workspace_bytes(C, n_layers - 2, H, W), "mc_fc_stack: workspace %zu < %zu bytes",
	           workspace_bytes, fc_workspace_bytes(C, n_layers - 2, H, W));
	MC_REQUIRE((uintptr_t)workspace % 16 == 0, "mc_fc_stack: workspace must be 16-byte aligned");
	MC_REQUIRE((int64_t)((H + 7) / 8) * ((W + 95) / 96) * D * 8 < ((int64_t)1 << 31), "mc_fc_stack: problem too large for one launch");
	return fc_stack(featL, featR, C, H, W, D, weights, biases, n_layers, volL, volR, workspace, as_stream(stream));
}

size_t mc_conv3x3_workspace_bytes(int Cin, int Cout)
{
	if (Cin < 1 || Cout < 1 || Cout > 128) return 0;
	return conv3x3_workspace_bytes(Cin, Cout);
}

int mc_conv3x3(const float *in, const float *weight, const float *bias, float *out, int N, int Cin, int Cout, int H, int W,
               int relu, void *workspace, size_t workspace_bytes, void *stream)
{
	MC_REQUIRE(in && weight && bias && out && workspace && in != out, "mc_conv3x3: bad pointers");
	MC_REQUIRE(N >= 1 && Cin >= 1 && Cout >= 1 && dims_ok(1, H, W), "mc_conv3x3: bad dims");
	MC_REQUIRE(Cout <= 128, "mc_conv3x3: Cout=%d exceeds 128 (the nets of main.lua:73-75, 120-122 use 64 and 112)", Cout);
	// 32-bit byte offsets inside one image's planes (buffer addressing) and 32-bit unit counts
	MC_REQUIRE((int64_t)(Cout > Cin ? Cout : Cin + 1) * H * W * 4 < (int64_t)0xFFFFFF00 && (int64_t)N * ((W + 31) / 32) * H < ((int64_t)1 << 31),
	           "mc_conv3x3: %d x %d x (%d -> %d channels) x %d images exceeds the kernel's 32-bit offsets", H, W, Cin, Cout, N);
	MC_REQUIRE(workspace_bytes >= conv3x3_workspace_bytes(Cin, Cout), "mc_conv3x3: workspace %zu < %zu bytes", workspace_bytes,
	           conv3x3_workspace_bytes(Cin, Cout));
	MC_REQUIRE((uintptr_t)workspace % 16 == 0, "mc_conv3x3: workspace must be 16-byte aligned");
	return conv3x3(in, weight, bias, out, N, Cin, Cout, H, W, relu, workspace, as_stream(stream));
}

int mc_fix_border(float *vol, int D, int H, int W, int n, int direction, void *stream)
{
	MC_REQUIRE(vol, "mc_fix_border: null pointer");
	MC_REQUIRE(dims_ok(D, H, W), "mc_fix_border: bad dims");
	MC_REQUIRE(n >= 0 && n < W, "mc_fix_border: n=%d out of range for W=%d", n, W);
	MC_REQUIRE_DIRECTION("mc_fix_border", direction);
	return fix_border(vol, D, H, W, n, direction, as_stream(stream));
}

int mc_cross(const float *img, float *arms, int H, int W, int L1, float tau1, void *stream)
{
	MC_REQUIRE(img && arms, "mc_cross: null pointer");
	MC_REQUIRE(dims_ok(1, H, W), "mc_cross: bad dims");
	return cross(img, arms, H, W, L1, tau1, as_stream(stream));
}

int mc_cbca(const float *x0c, const float *x1c, const float *vol_in, float *vol_out, int D, int H, int W, int direction,
            void *stream)
{
	MC_REQUIRE(x0c && x1c && vol_in && vol_out, "mc_cbca: null pointer");
	MC_REQUIRE(vol_in != vol_out, "mc_cbca: in-place aggregation is not supported (the reference uses a tmp volume too)");
	MC_REQUIRE(dims_ok(D, H, W) && D <= 65535, "mc_cbca: bad dims");
	MC_REQUIRE_DIRECTION("mc_cbca", direction);
	return cbca(x0c, x1c, vol_in, vol_out, D, H, W, direction, as_stream(stream));
}

size_t mc_cbca_scratch_bytes(int H, int W)
{
	if (H < 1 || W < 1) return 0;
	return cbca_scratch_bytes(H, W);
}

int mc_cbca_ws(const float *x0c, const float *x1c, const float *vol_in, float *vol_out, int D, int H, int W, int direction,
               void *scratch, size_t scratch_bytes, void *stream)
{
	MC_REQUIRE(x0c && x1c && vol_in && vol_out && scratch, "mc_cbca_ws: null pointer");
	MC_REQUIRE(vol_in != vol_out, "mc_cbca_ws: in-place aggregation is not supported (the reference uses a tmp volume too)");
	MC_REQUIRE(dims_ok(D, H, W) && D <= 65535 * 8, "mc_cbca_ws: bad dims");
	MC_REQUIRE_DIRECTION("mc_cbca_ws", direction);
	MC_REQUIRE(scratch_bytes >= cbca_scratch_bytes(H, W), "mc_cbca_ws: scratch holds %zu bytes, needs %zu", scratch_bytes,
	           cbca_scratch_bytes(H, W));
	MC_REQUIRE((uintptr_t)scratch % 4 == 0, "mc_cbca_ws: scratch must be 4-byte aligned");
	hipStream_t st = as_stream(stream);
	if (!packed_dims_ok(H, W))   // (huge or extremely elongated images: one thread per voxel, 64-bit offsets)
		return cbca(x0c, x1c, vol_in, vol_out, D, H, W, direction, st);
	int rc = cbca_pack(x0c, x1c, scratch, H, W, st);
	if (rc) return rc;
	rc = cbca_by_arms(scratch, vol_in, vol_out, D, H, W, direction, -1, st);
	if (rc) return rc;
	return cbca_if_overflow(x0c, x1c, scratch, vol_in, vol_out, D, H, W, direction, st);
}

size_t mc_cbca_plan_bytes(int D, int H, int W)
{
	if (!dims_ok(D, H, W)) return 0;
	const PlanArea pa = plan_area(D, H, W);
	return pa.off - cbca_scratch_bytes(H, W) + pa.bytes;
}

int mc_cbca_ws_cfg(const float *x0c, const float *x1c, const float *vol_in, float *vol_out, int D, int H, int W, int direction,
                   void *scratch, size_t scratch_bytes, int rb, int nt, int d0, int nd, int form, void *stream)
{
	MC_REQUIRE(x0c && x1c && vol_in && vol_out && scratch, "mc_cbca_ws_cfg: null pointer");
	MC_REQUIRE(vol_in != vol_out, "mc_cbca_ws_cfg: in-place aggregation is not supported");
	MC_REQUIRE(dims_ok(D, H, W) && D <= 65535 * 8, "mc_cbca_ws_cfg: bad dims");
	MC_REQUIRE_DIRECTION("mc_cbca_ws_cfg", direction);
	MC_REQUIRE(scratch_bytes >= cbca_scratch_bytes(H, W), "mc_cbca_ws_cfg: scratch holds %zu bytes, needs %zu", scratch_bytes,
	           cbca_scratch_bytes(H, W));
	MC_REQUIRE((uintptr_t)scratch % 4 == 0, "mc_cbca_ws_cfg: scratch must be 4-byte aligned");
	MC_REQUIRE(packed_dims_ok(H, W), "mc_cbca_ws_cfg: image too large for the packed-length kernels (32-bit plane offsets, 24-bit row indices)");
	MC_REQUIRE(rb >= 0 && rb <= 4096 && nt >= -1 && nt <= 1 && form >= 0 && form <= 11, "mc_cbca_ws_cfg: bad rb / nt / form");
	MC_REQUIRE(d0 >= 0 && nd >= 0 && (form >= 8 || d0 + nd <= D), "mc_cbca_ws_cfg: planes [%d, %d) outside the volume", d0, d0 + nd);
	hipStream_t st = as_stream(stream);
	int rc = cbca_pack(x0c, x1c, scratch, H, W, st);
	if (rc) return rc;
	CbcaCfg cfg;
	cfg.nt = nt; cfg.d0 = d0; cfg.nd = nd;
	if (form >= 10) {   // TWO passes in one launch (cbca_lean2x): 10 writes the list of its wave geometry first, 11 reads it; vol_out = the volume after
		// the second pass.  The strip kernel takes both passes (through a volume behind the list) if the list is not this problem's or did not fit.
		const PlanArea pa = plan_area(D, H, W);
		const size_t off = pa.off, pb = align_up(pa.bytes, 256);
		const size_t vb = (size_t)D * H * W * sizeof(float);
		MC_REQUIRE(scratch_bytes >= off + pb + vb, "mc_cbca_ws_cfg: scratch holds %zu bytes, needs %zu with the list and a volume", scratch_bytes, off + pb + vb);
		MC_REQUIRE((uintptr_t)scratch % 16 == 0, "mc_cbca_ws_cfg: scratch must be 16-byte aligned for the list");
		cfg.plan = (char *)scratch + off;
		cfg.plan_bytes = pb;
		cfg.lean_rb = rb;
		cfg.lean_two_pass = true;
		cfg.d0 = 0; cfg.nd = 0;
		float *mid = (float *)((char *)scratch + off + pb);
		const bool fits = cbca_lean_fits(D, H, W, pb, true, rb);   // (the records of this many rows per wave fit the area; else: the strip kernel, unconditionally)
		if (fits && form == 10) {
			rc = cbca_classify(scratch, cfg.plan, cfg.plan_bytes, D, H, W, direction, CR_NOT_DIRECT, rb, 0, st, true, (float)d0);   // (d0 > 0: the cost limit, in values per voxel)
			if (rc) return rc;
		}
		if (fits) {
			rc = cbca_lean2x(scratch, cfg.plan, cfg.plan_bytes, vol_in, vol_out, D, H, W, direction, CR_NOT_DIRECT, st, cfg);
			if (rc) return rc;
		}
		const int sroute = fits ? CR_NOT_DIRECT_IF_NO_LIST : CR_NOT_DIRECT;
		rc = cbca_strips(scratch, vol_in, mid, D, H, W, direction, sroute, st, cfg);
		if (rc) return rc;
		rc = cbca_strips(scratch, mid, vol_out, D, H, W, direction, sroute, st, cfg);
		if (rc) return rc;
		rc = cbca_if_overflow(x0c, x1c, scratch, vol_in, mid, D, H, W, direction, st);
		if (rc) return rc;
		return cbca_if_overflow(x0c, x1c, scratch, mid, vol_out, D, H, W, direction, st);
	}
	if (form >= 8) {   // lean kernel (textures): 8 lists the outputs whose support is not the minimal 3 x 3 behind the packed lengths first, 9 reads that list
		const auto [off, pb] = plan_area(D, H, W);
		MC_REQUIRE(scratch_bytes >= off + pb, "mc_cbca_ws_cfg: scratch holds %zu bytes, needs %zu with the list", scratch_bytes, off + pb);
		MC_REQUIRE((uintptr_t)scratch % 16 == 0, "mc_cbca_ws_cfg: scratch must be 16-byte aligned for the list");
		MC_REQUIRE(cbca_lean_fits(D, H, W, pb), "mc_cbca_ws_cfg: volume too large for 32-bit list entries");
		// (forms 8 / 9 take the whole volume; rb = rows per wave, d0 = launch variant, nd > 0 = slots the list may hold, to exercise the fallback)
		cfg.plan = (char *)scratch + off;
		cfg.plan_bytes = pb;
		cfg.lean_rb = rb;
		cfg.lean_variant = d0; cfg.d0 = 0; cfg.nd = nd;
		if (form == 8) {
			rc = cbca_classify(scratch, cfg.plan, cfg.plan_bytes, D, H, W, direction, CR_NOT_DIRECT, rb, nd, st);
			if (rc) return rc;
		}
		rc = cbca_lean(scratch, cfg.plan, cfg.plan_bytes, vol_in, vol_out, D, H, W, direction, CR_NOT_DIRECT, st, cfg);
		if (rc) return rc;
		cfg.nd = 0;
		rc = cbca_strips(scratch, vol_in, vol_out, D, H, W, direction, CR_NOT_DIRECT_IF_NO_LIST, st, cfg);
		if (rc) return rc;
		return cbca_if_overflow(x0c, x1c, scratch, vol_in, vol_out, D, H, W, direction, st);
	}
	if (form >= 4) {   // tile kernel with the item order kept behind the packed lengths: 4 / 5 write it (short- / long-arm instance), 6 / 7 read it
		const auto [off, pb] = plan_area(D, H, W);
		MC_REQUIRE(scratch_bytes >= off + pb, "mc_cbca_ws_cfg: scratch holds %zu bytes, needs %zu with the plan", scratch_bytes, off + pb);
		MC_REQUIRE((uintptr_t)scratch % 16 == 0, "mc_cbca_ws_cfg: scratch must be 16-byte aligned for the plan");
		cfg.plan = (char *)scratch + off;
		cfg.plan_mode = form <= 5 ? 1 : 2;
		const bool shortarm = form == 4 || form == 6;
		return cbca_tiles(scratch, vol_in, vol_out, D, H, W, direction, shortarm ? 4 : 13, shortarm ? CR_ARMS_LE4 : CR_ARMS_LE13, st, cfg);
	}
	if (form >= 2) {   // tile kernel, short-arm (2) / long-arm (3) instance, rb = geometry variant; nothing is written if an arm exceeds 4 / 13
		cfg.variant = rb;
		return cbca_tiles(scratch, vol_in, vol_out, D, H, W, direction, form == 2 ? 4 : 13, form == 2 ? CR_ARMS_LE4 : CR_ARMS_LE13, st, cfg);
	}
	cfg.rb = rb;
	rc = form == 1 ? cbca_strips(scratch, vol_in, vol_out, D, H, W, direction, CR_NOT_DIRECT, st, cfg)
	               : cbca_by_arms(scratch, vol_in, vol_out, D, H, W, direction, -1, st, cfg);
	if (rc) return rc;
	return cbca_if_overflow(x0c, x1c, scratch, vol_in, vol_out, D, H, W, direction, st);
}

int mc_transpose_cfg(const float *in, float *out, int64_t rows, int64_t cols, int64_t ldin, int64_t ldout, float scale_, int nt,
                     void *stream)
{
	MC_REQUIRE(in && out && in != out, "mc_transpose_cfg: bad pointers");
	MC_REQUIRE(rows >= 1 && cols >= 1 && ldin >= cols && ldout >= rows, "mc_transpose_cfg: bad dims");
	MC_REQUIRE(nt >= -1 && nt <= 1, "mc_transpose_cfg: bad nt");
	return transpose(in, out, rows, cols, ldin, ldout, scale_, as_stream(stream), nt);
}


int mc_sgm2_contract_violations(const float *in_hwd, int H, int W, int D, unsigned *count, void *stream)
{
	MC_REQUIRE(in_hwd && count, "mc_sgm2_contract_violations: null pointer");
	MC_REQUIRE(dims_ok(D, H, W), "mc_sgm2_contract_violations: bad dims");
	return sgm_contract_violations(in_hwd, H, W, D, count, as_stream(stream));
}

size_t mc_sgm2_tmp_bytes(int H, int W, int D)
{
	if (H < 1 || W < 1) return 0;
	return sgm_maps_bytes_d(H, W, D);   // one size for every D <= 512, a larger one above (the window rows' pad)
}

int mc_sgm2(const float *x0, const float *x1, const float *in_hwd, float *out_hwd, void *tmp, size_t tmp_bytes, int H, int W,
            int D, float pi1, float pi2, float tau_so, float alpha1, float sgm_q1, float sgm_q2, int direction, void *stream)
{
	MC_REQUIRE(x0 && x1 && in_hwd && out_hwd && tmp, "mc_sgm2: null pointer");
	MC_REQUIRE(dims_ok(D, H, W), "mc_sgm2: bad dims");
	MC_REQUIRE(D <= MC_SGM_MAX_D, "mc_sgm2: D=%d exceeds %d", D, MC_SGM_MAX_D);
	MC_REQUIRE_DIRECTION("mc_sgm2", direction);
	MC_REQUIRE(tmp_bytes >= sgm_maps_bytes_d(H, W, D), "mc_sgm2: tmp holds %zu bytes, needs %zu", tmp_bytes, sgm_maps_bytes_d(H, W, D));
	MC_REQUIRE(in_hwd != out_hwd, "mc_sgm2: input and output must differ");
	hipStream_t st = as_stream(stream);
	int rc = sgm_prep_d(x0, x1, tmp, H, W, D, tau_so, st);
	if (rc) return rc;
	const float *Cv[2] = {in_hwd, in_hwd};
	float *outv[2] = {out_hwd, out_hwd};
	const int dirv[2] = {direction, direction};
	return sgm_sweeps(Cv, outv, nullptr, nullptr, dirv, 1, H, W, D, D, tmp, pi1, pi2, alpha1, sgm_q1, sgm_q2, false, 0u, false, st);
}

int mc_dhw_to_hwd(const float *in, float *out, int D, int H, int W, void *stream)
{
	MC_REQUIRE(in && out && in != out, "mc_dhw_to_hwd: bad pointers");
	MC_REQUIRE(dims_ok(D, H, W), "mc_dhw_to_hwd: bad dims");
	return transpose(in, out, D, (int64_t)H * W, (int64_t)H * W, D, 1.0f, as_stream(stream));
}

int mc_hwd_to_dhw(const float *in, float *out, int D, int H, int W, float scale_, void *stream)
{
	MC_REQUIRE(in && out && in != out, "mc_hwd_to_dhw: bad pointers");
	MC_REQUIRE(dims_ok(D, H, W), "mc_hwd_to_dhw: bad dims");
	return transpose(in, out, (int64_t)H * W, D, D, (int64_t)H * W, scale_, as_stream(stream));
}

int mc_scale(const float *in, float *out, int64_t n, float s, void *stream)
{
	MC_REQUIRE((in && out) || n == 0, "mc_scale: null pointer");
	MC_REQUIRE(n >= 0, "mc_scale: negative size");
	return scale(in, out, n, s, as_stream(stream));
}

int mc_argmin(const float *vol, float *disp, int D, int H, int W, void *stream)
{
	MC_REQUIRE(vol && disp, "mc_argmin: null pointer");
	MC_REQUIRE(dims_ok(D, H, W), "mc_argmin: bad dims");
	return argmin_dhw(vol, disp, D, H, W, 0, as_stream(stream));
}

int mc_spatial_argmin(const float *vol, float *out, int D, int H, int W, void *stream)
{
	MC_REQUIRE(vol && out, "mc_spatial_argmin: null pointer");
	MC_REQUIRE(dims_ok(D, H, W), "mc_spatial_argmin: bad dims");
	return argmin_dhw(vol, out, D, H, W, 1, as_stream(stream));
}

int mc_cost_margins(const float *vol, int D, int H, int W, float *d1_out, float *c1_out, float *c2_out, float *c2l_out, void *stream)
{
	MC_REQUIRE(dims_ok(D, H, W), "mc_cost_margins: bad dims D=%d H=%d W=%d", D, H, W);
	MC_REQUIRE(vol, "mc_cost_margins: null volume");
	MC_REQUIRE(d1_out || c1_out || c2_out || c2l_out, "mc_cost_margins: no output asked for");
	const size_t map_bytes = (size_t)H * W * sizeof(float);
	struct Range { const char *name; uintptr_t at; size_t bytes; };
	const Range r[5] = {{"vol", (uintptr_t)vol, map_bytes * D}, {"d1_out", (uintptr_t)d1_out, map_bytes}, {"c1_out", (uintptr_t)c1_out, map_bytes},
	                    {"c2_out", (uintptr_t)c2_out, map_bytes}, {"c2l_out", (uintptr_t)c2l_out, map_bytes}};
	for (int i = 1; i < 5; ++i)
		for (int j = 0; j < i; ++j)
			MC_REQUIRE(!r[i].at || !r[j].at || r[i].at + r[i].bytes <= r[j].at || r[j].at + r[j].bytes <= r[i].at,
			           "mc_cost_margins: %s overlaps %s", r[i].name, r[j].name);
	return cost_margins_dhw(vol, d1_out, c1_out, c2_out, c2l_out, D, H, W, as_stream(stream));
}

int mc_outlier_detection(const float *d0, const float *d1, float *outlier, int H, int W, int disp_max, void *stream)
{
	MC_REQUIRE(d0 && d1 && outlier, "mc_outlier_detection: null pointer");
	MC_REQUIRE(dims_ok(1, H, W) && disp_max >= 0, "mc_outlier_detection: bad dims");
	return outlier_detection(d0, d1, outlier, H, W, disp_max, as_stream(stream));
}

int mc_interpolate_occlusion(const float *d0, const float *outlier, float *out, int H, int W, void *stream)
{
	MC_REQUIRE(d0 && outlier && out && out != d0, "mc_interpolate_occlusion: bad pointers");
	MC_REQUIRE(dims_ok(1, H, W), "mc_interpolate_occlusion: bad dims");
	return interpolate_occlusion(d0, outlier, out, H, W, as_stream(stream));
}

int mc_interpolate_mismatch(const float *d0, const float *outlier, float *out, int H, int W, void *stream)
{
	MC_REQUIRE(d0 && outlier && out && out != d0, "mc_interpolate_mismatch: bad pointers");
	MC_REQUIRE(dims_ok(1, H, W), "mc_interpolate_mismatch: bad dims");
	return interpolate_mismatch(d0, outlier, out, H, W, as_stream(stream));
}

int mc_subpixel_enchancement(const float *d0, const float *vol, float *out, int D, int H, int W, void *stream)
{
	MC_REQUIRE(d0 && vol && out, "mc_subpixel_enchancement: null pointer");
	MC_REQUIRE(dims_ok(D, H, W), "mc_subpixel_enchancement: bad dims");
	return subpixel(d0, vol, out, D, H, W, (int64_t)H * W, 1, as_stream(stream));
}

int mc_median2d(const float *img, float *out, int H, int W, int kernel_size, void *stream)
{
	MC_REQUIRE(img && out && img != out, "mc_median2d: bad pointers");
	MC_REQUIRE(dims_ok(1, H, W), "mc_median2d: bad dims");
	MC_REQUIRE(kernel_size % 2 == 1 && kernel_size >= 1 && kernel_size <= 11,
	           "mc_median2d: kernel_size must be odd and <= 11 (adcensus.cu:1601-1602)");
	return median2d(img, out, H, W, kernel_size, as_stream(stream));
}

int mc_mean2d(const float *img, const float *kernel, float *out, int H, int W, int ks, float alpha2, void *stream)
{
	MC_REQUIRE(img && kernel && out && img != out, "mc_mean2d: bad pointers");
	MC_REQUIRE(dims_ok(1, H, W), "mc_mean2d: bad dims");
	MC_REQUIRE(ks % 2 == 1 && ks >= 1, "mc_mean2d: kernel size must be odd (adcensus.cu:1269)");
	return mean2d(img, kernel, out, H, W, ks, alpha2, as_stream(stream));
}

int mc_gaussian_host(double sigma, float *host_kernel, int capacity)
{
	MC_REQUIRE(sigma > 0, "mc_gaussian_host: sigma must be > 0");
	const int ks = gaussian_ks(sigma);
	if (host_kernel) {  // plain host arithmetic: works without a device
		MC_REQUIRE(capacity >= ks * ks, "mc_gaussian_host: capacity %d < %d", capacity, ks * ks);
		gaussian_fill(sigma, host_kernel);
	}
	return ks;
}

int mc_normalize_forward(const float *in, float *norm, float *out, int N, int C, int H, int W, void *stream)
{
	MC_REQUIRE(in && out, "mc_normalize_forward: null pointer");
	MC_REQUIRE(N >= 1 && C >= 1 && dims_ok(1, H, W), "mc_normalize_forward: bad dims");
	return normalize_forward(in, norm, out, N, C, H, W, as_stream(stream));
}

size_t mc_predict_workspace_bytes(const mc_params *p, int C, int D, int H, int W)
{
	(void)C;
	if (!p || !dims_ok(D, H, W) || !(p->blur_sigma > 0)) return 0;
	return make_plan(p, D, H, W).total;
}

size_t mc_predict_workspace_bytes_full(const mc_params *p, int C, int D, int H, int W)
{
	(void)C;
	if (!p || !dims_ok(D, H, W) || !(p->blur_sigma > 0)) return 0;
	return make_plan(p, D, H, W).total_ck;
}

int mc_predict(const mc_params *p, const float *x0, const float *x1, const float *featL, const float *featR, int C,
               const float *rawL, const float *rawR, int D, int H, int W, void *workspace, size_t workspace_bytes,
               float *volL_out, float *volR_out, float *dispL0_out, float *dispR0_out, float *disp_out, void *stream)
{
	return mc_predict_ex(p, x0, x1, featL, featR, C, rawL, rawR, D, H, W, workspace, workspace_bytes, volL_out, volR_out, dispL0_out, dispR0_out,
	                     nullptr, nullptr, nullptr, disp_out, stream);
}

int mc_predict_ex(const mc_params *p, const float *x0, const float *x1, const float *featL, const float *featR, int C,
                  const float *rawL, const float *rawR, int D, int H, int W, void *workspace, size_t workspace_bytes,
                  float *volL_out, float *volR_out, float *dispL0_out, float *dispR0_out, float *outlier_out, float *cost_out, float *curv_out,
                  float *disp_out, void *stream)
{
	StageTimer tm;
	PredictExtras ex;
	ex.outlier = outlier_out; ex.cost = cost_out; ex.curv = curv_out;
	return predict_impl(p, x0, x1, featL, featR, C, rawL, rawR, D, H, W, workspace, workspace_bytes, volL_out, volR_out,
	                    dispL0_out, dispR0_out, disp_out, as_stream(stream), tm, ex);
}

int mc_predict_views(const mc_params *p, const float *x0, const float *x1, const float *featL, const float *featR, int C,
                     const float *rawL, const float *rawR, int D, int H, int W, void *workspace, size_t workspace_bytes,
                     float *volL_out, float *volR_out, float *dispL0_out, float *dispR0_out, float *outlier_out, float *cost_out, float *curv_out,
                     float *dispR_out, float *outlierR_out, float *disp_out, void *stream)
{
	StageTimer tm;
	PredictExtras ex;
	ex.outlier = outlier_out; ex.cost = cost_out; ex.curv = curv_out;
	ex.dispR = dispR_out; ex.outlierR = outlierR_out;
	return predict_impl(p, x0, x1, featL, featR, C, rawL, rawR, D, H, W, workspace, workspace_bytes, volL_out, volR_out,
	                    dispL0_out, dispR0_out, disp_out, as_stream(stream), tm, ex);
}

int mc_predict_timed(const mc_params *p, const float *x0, const float *x1, const float *featL, const float *featR, int C,
                     const float *rawL, const float *rawR, int D, int H, int W, void *workspace, size_t workspace_bytes,
                     float *disp_out, void *stream, float *stage_ms)
{
	StageTimer tm;
	tm.on = stage_ms != nullptr;
	tm.st = as_stream(stream);
	const int rc = predict_impl(p, x0, x1, featL, featR, C, rawL, rawR, D, H, W, workspace, workspace_bytes, nullptr, nullptr,
	                            nullptr, nullptr, disp_out, tm.st, tm);
	if (stage_ms) tm.collect(stage_ms);
	return rc;
}

// ---- for the tests only: not declared in include/mc_adcensus.h, not part of the ABI ----
#pragma GCC visibility push(default)
// the fast path's schedule: 1 / 2 force one lane / two lanes (2: also where the callers' streams alternate), 0 returns to MC_PREDICT_LANES,
// -1 only asks; returns the one in force
int mc_test_predict_lanes(int set) { return predict_lanes(set); }

// the fused schedule's vertical launches where both forms apply: 1 forces the down and the up sweep, 2 the checkpoint launch and the recomputing
// walk, 0 returns to the default (2), -1 only asks; returns the one in force
int mc_test_sgm_vertical(int mode) { return sgm_vertical(mode); }

// stereo_join_hwd (StereoJoin + fix_border into mc_predict's (H,W,ds) layout) for the chosen volumes: sides bit 0 left, bit 1 right
int mc_test_stereo_join_hwd(const float *featL, const float *featR, float *volL, float *volR, int C, int D, int ds, int H, int W, int border_n,
                            int sides, void *stream)
{
	MC_REQUIRE(featL && featR && volL && volR, "mc_test_stereo_join_hwd: null pointer");
	MC_REQUIRE(dims_ok(D, H, W) && C >= 1 && C <= MC_JOIN_MAX_C && ds >= D && border_n >= 0 && border_n < W, "mc_test_stereo_join_hwd: bad dims");
	const int64_t HW = (int64_t)H * W;   // the kernels' 32-bit offsets, as mc_predict checks them in front of its fast path
	MC_REQUIRE((int64_t)W * ds * 4 < ((int64_t)1 << 31) && ((int64_t)(C + 64) * HW + W) * 4 < ((int64_t)1 << 31), "mc_test_stereo_join_hwd: too large");
	return stereo_join_hwd(featL, featR, volL, volR, C, D, ds, H, W, border_n, as_stream(stream), sides);
}
#pragma GCC visibility pop

}  // extern "C"
