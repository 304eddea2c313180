"""stereo_predict (main.lua:929-1082) on MI355X.

Two drivers over the same kernels:

* `stereo_predict`        -- the reference's call sequence op by op through the
  `adcensus.*` mirror (what main.lua does once the LuaJIT shim replaces
  libadcensus.so): (D,H,W) volumes, explicit transposes around sgm2, ping-pong
  tmp volumes for cbca.
* `stereo_predict_fused`  -- one C-ABI call (`mc_predict`) that runs the whole
  post-CNN pipeline on one stream inside a caller-owned workspace: StereoJoin
  writes (H,W,D) directly with NaN fill and fix_border folded in, the SGM sweeps
  fold the zeroing, the /4 and the arg-min, and nothing is copied in between.

Both take the cost-volume stage as input: `feat` = (2,C,H,W) normalised features
(arch fast) or `raw` = the two raw (D,H,W) volumes of arch slow / ad / census.
"""
import ctypes as C

import torch

from . import adcensus
from ._lib import check, lib
from .params import make_params


STAGES = ("prep", "join", "cbca", "layout", "sgm", "argmin", "post", "_")  # MC_STAGE_* of mc_adcensus.h


def _img2(x_batch):
    H, W = x_batch.shape[-2:]
    xb = x_batch.reshape(2, H, W)
    return xb[0].contiguous(), xb[1].contiguous(), H, W


def stereo_predict(x_batch, params, disp_max, feat=None, raw=None, return_all=False):
    """Op-by-op mirror of stereo_predict(x_batch, id), main.lua:929-1082.

    x_batch: (2,1,H,W) normalised images.  Returns disp[2] (1,1,H,W); with
    return_all also the final volumes (what left.bin / right.bin hold), the
    intermediate maps and the three per-pixel maps of mc_predict_ex: `outlier`
    (the LR check's classes; without the LR check it runs for the map alone),
    `cost` and `curvature` (the left volume around the disparity the sub-pixel
    stage reads), each (1,1,H,W), the two maps of mc_predict_views,
    `disp_right` and `outlier_right` (right_view below), and the margins of
    both final volumes' cost curves, `c1`, `c2`, `c2l` and `c1_right`,
    `c2_right`, `c2l_right` (cost_margins below: mc_cost_margins with torch alone)."""
    p = make_params(params)
    x0, x1, H, W = _img2(x_batch)
    D = int(disp_max)
    dev = x_batch.device

    vols = [None, None]  # [0] = left (direction -1), [1] = right (+1): vols[{{direction == -1 and 1 or 2}}]
    if feat is not None:  # arch == 'fast', main.lua:944-951
        feat = feat.contiguous()
        vl = adcensus.fill_nan(torch.empty((1, D, H, W), dtype=torch.float32, device=dev))
        vr = adcensus.fill_nan(torch.empty((1, D, H, W), dtype=torch.float32, device=dev))
        adcensus.StereoJoin(feat[0], feat[1], vl, vr)
        adcensus.fix_border(vl, p.border_n, -1)
        adcensus.fix_border(vr, p.border_n, 1)
        vols = [vl, vr]
    else:
        vols = [raw[0].reshape(1, D, H, W).clone(), raw[1].reshape(1, D, H, W).clone()]

    disp = {}
    out_vols = {}
    for direction in (1, -1):  # main.lua:954-955
        vol = vols[0 if direction == -1 else 1]
        # main.lua:992-1004: cross is computed whenever cbca is not skipped, even for 0 iterations
        x0c = torch.empty((1, 4, H, W), dtype=torch.float32, device=dev)
        x1c = torch.empty((1, 4, H, W), dtype=torch.float32, device=dev)
        adcensus.cross(x0, x0c, p.L1, p.tau1)
        adcensus.cross(x1, x1c, p.L1, p.tau1)
        tmp_cbca = torch.empty_like(vol)
        for _ in range(p.cbca_i1):
            adcensus.cbca(x0c, x1c, vol, tmp_cbca, direction)
            vol, tmp_cbca = tmp_cbca, vol  # vol:copy(tmp_cbca)
        if p.sgm_i > 0:  # main.lua:1007-1030
            volh = adcensus.dhw_to_hwd(vol)
            out = torch.empty_like(volh)
            tmp = torch.empty((W, D), dtype=torch.float32, device=dev)
            for _ in range(p.sgm_i):
                out.zero_()
                adcensus.sgm2(x0, x1, volh, out, tmp, p.pi1, p.pi2, p.tau_so, p.alpha1, p.sgm_q1, p.sgm_q2, direction)
                adcensus.scale(out, volh, 0.25)  # vol:copy(out):div(4)
            vol = adcensus.hwd_to_dhw(out, 0.25, out=vol.reshape(1, D, H, W))  # main.lua:1019-1020
        tmp_cbca = torch.empty_like(vol)
        for _ in range(p.cbca_i2):  # main.lua:1033-1039
            adcensus.cbca(x0c, x1c, vol, tmp_cbca, direction)
            vol, tmp_cbca = tmp_cbca, vol
        out_vols[direction] = vol
        disp[1 if direction == 1 else 2] = adcensus.argmin(vol)  # main.lua:1049-1050

    d = disp[2]
    outlier = torch.zeros_like(d)
    if p.lr_check:  # main.lua:1054-1066
        adcensus.outlier_detection(d, disp[1], outlier, D)
        d = adcensus.interpolate_occlusion(d, outlier)
        d = adcensus.interpolate_mismatch(d, outlier)
    elif return_all:
        adcensus.outlier_detection(d, disp[1], outlier, D)
    if return_all:
        cost, curvature = confidence_maps(d, out_vols[-1])
    d = adcensus.subpixel_enchancement(d, out_vols[-1], D)  # vol = LEFT volume, main.lua:1068
    d = adcensus.median2d(d, p.median_k)
    d = adcensus.mean2d(d, adcensus.gaussian(p.blur_sigma).to(dev), p.blur_t)
    if return_all:
        disp_right, outlier_right = right_view(p, disp[2], disp[1], out_vols[1], D)
        res = dict(disp=d, volL=out_vols[-1], volR=out_vols[1], dispL0=disp[2], dispR0=disp[1], outlier=outlier, cost=cost,
                   curvature=curvature, disp_right=disp_right, outlier_right=outlier_right)
        for direction, suffix in ((-1, ""), (1, "_right")):
            _, res["c1" + suffix], res["c2" + suffix], res["c2l" + suffix] = cost_margins(out_vols[direction])
        return res
    return d


def _first_min(vals):
    """(index, value) of the first minimum along dim 1 of a (1,D,H,W) tensor without NaN: the value is gathered, so it keeps its bits"""
    D = vals.shape[1]
    idx = torch.arange(D, device=vals.device).reshape(1, D, 1, 1)
    m = vals.min(dim=1, keepdim=True).values
    at = torch.where(vals == m, idx, D).min(dim=1, keepdim=True).values
    return at, vals.gather(1, at)


def cost_margins(vol):
    """mc_cost_margins with torch alone, for a (1,D,H,W) volume: (d1, c1, c2, c2l), (1,1,H,W) each.  Values that are not below +INF
    (NaN, +INF) are no candidates; d1 is the first minimum of the rest (0 where there is none) and c1 its cost; c2 is the smallest
    candidate at another d; c2l is the smallest at another d among the local minima -- candidates with !(c[d-1] <= c[d]) and
    !(c[d+1] < c[d]), the comparisons taken on shifted copies whose missing neighbour is NaN.  +INF where there is none."""
    D = vol.shape[1]
    inf = torch.full_like(vol, float("inf"))
    idx = torch.arange(D, device=vol.device).reshape(1, D, 1, 1)
    valid = vol < inf
    d1, c1 = _first_min(torch.where(valid, vol, inf))
    d1 = torch.where(c1 < inf[:, :1], d1, torch.zeros_like(d1))
    others = valid & (idx != d1)
    _, c2 = _first_min(torch.where(others, vol, inf))
    nan = torch.full_like(vol[:, :1], float("nan"))
    before, after = torch.cat([nan, vol[:, :-1]], 1), torch.cat([vol[:, 1:], nan], 1)
    local_min = others & ~(before <= vol) & ~(after < vol)
    _, c2l = _first_min(torch.where(local_min, vol, inf))
    return d1.to(torch.float32), c1, c2, c2l


def right_view(p, dispL0, dispR0, volR, D):
    """mc_predict_views' dispR_out and outlierR_out with the stand-alone operators and torch.flip.  Mirroring the scene along x turns
    the right image into a left one, so the right view's map is the post-processing above on the mirrored arg-min maps and the
    mirrored right volume, mirrored back; the stages follow the parameter set's lr_check as above.  (The direction-dependent
    stages -- the LR check's x - d, the occlusion stage's look to the left, the rounding of the mismatch rays' half steps -- are
    the left view's on mirrored data: that IS the definition.)  Returns (disp_right, outlier_right), (1,1,H,W) each."""
    def M(a):
        return torch.flip(a, dims=[-1]).contiguous()

    t = M(dispR0)
    outlier = torch.zeros_like(t)
    adcensus.outlier_detection(t, M(dispL0), outlier, D)
    if p.lr_check:
        t = adcensus.interpolate_occlusion(t, outlier)
        t = adcensus.interpolate_mismatch(t, outlier)
    t = adcensus.subpixel_enchancement(t, M(volR), D)
    t = adcensus.median2d(t, p.median_k)
    t = adcensus.mean2d(t, adcensus.gaussian(p.blur_sigma).to(t.device), p.blur_t)
    return M(t), M(outlier)


def confidence_maps(d, vol):
    """mc_predict_ex's cost_out and curv_out with torch indexing: for the integer disparity map d (1,1,H,W) and the volume
    (1,D,H,W), c(d) and 2 * (c(d+1) + c(d-1) - 2 * c(d)) in float32 in that order, the curvature 0 where d < 1 or d >= D - 1."""
    D = vol.shape[1]
    di = d.to(torch.int64)
    cz = vol.gather(1, di)
    cn = vol.gather(1, (di - 1).clamp(0, D - 1))
    cp = vol.gather(1, (di + 1).clamp(0, D - 1))
    curvature = 2 * ((cp + cn) - 2 * cz)
    inner = (di >= 1) & (di < D - 1)
    return cz, torch.where(inner, curvature, torch.zeros_like(curvature))


def workspace_bytes(params, disp_max, H, W, C_feat=0, full=False):
    """what mc_predict needs; full: with the SGM's checkpoint slots behind it, the size at which it runs its faster vertical sweeps"""
    p = make_params(params)
    fn = lib.mc_predict_workspace_bytes_full if full else lib.mc_predict_workspace_bytes
    n = fn(C.byref(p), int(C_feat), int(disp_max), int(H), int(W))
    if n == 0:
        raise ValueError("mc_predict_workspace_bytes: bad arguments")
    return n


class Workspace:
    """Caller-owned device scratch for mc_predict (one per concurrent stream): nbytes is what mc_predict needs, nbytes_full what is
    allocated and handed to it -- the SGM's checkpoint slots lie behind nbytes."""

    def __init__(self, params, disp_max, H, W, device):
        self.nbytes = workspace_bytes(params, disp_max, H, W)
        self.nbytes_full = workspace_bytes(params, disp_max, H, W, full=True)
        self.buf = torch.empty(self.nbytes_full + 256, dtype=torch.uint8, device=device)
        off = (-self.buf.data_ptr()) % 256
        self.ptr = self.buf.data_ptr() + off


def stereo_predict_fused(x_batch, params, disp_max, feat=None, raw=None, workspace=None, want_volumes=False,
                         want_disp0=False, out=None, timed=False, want_outlier=False, want_confidence=False, want_right=False,
                         want_margins=False):
    """The whole of stereo_predict from the cost-volume stage on, in one C-ABI call.

    want_outlier adds res["outlier"], the LR check's class per pixel (0 match, 1 occlusion, 2 mismatch); want_confidence adds
    res["cost"] and res["curvature"], the final left volume at the disparity the sub-pixel stage reads and the curvature of the cost
    curve there.  Each is (1,1,H,W); with either flag the call is mc_predict_ex, otherwise mc_predict.

    want_right adds res["disp_right"] and res["outlier_right"], the right view's finished disparity map and its classes (right_view
    above states them op by op); the call is then mc_predict_views, and the right view costs the (H,W) tail alone.

    want_margins adds res["c1"], res["c2"] and res["c2l"], the margins of every pixel's cost curve in the final left volume
    (mc_cost_margins: the minimum, the smallest cost at another disparity, the smallest local minimum at another disparity), and with
    want_right also res["c1_right"], res["c2_right"], res["c2l_right"] from the final right volume.  The volumes are exported for the
    scan, which follows the pipeline's call on the same stream; they are returned with want_volumes only."""
    p = make_params(params)
    x0, x1, H, W = _img2(x_batch)
    D = int(disp_max)
    dev = x_batch.device
    if workspace is None:
        workspace = Workspace(p, D, H, W, dev)
    if out is None:
        out = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
    fl = fr = rl = rr = None
    Cn = 0
    if feat is not None:
        feat = feat.contiguous()
        Cn = feat.shape[-3]
        fl, fr = feat[0].data_ptr(), feat[1].data_ptr()
        keep = feat
    else:
        keep = (raw[0].contiguous(), raw[1].contiguous())
        rl, rr = keep[0].data_ptr(), keep[1].data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    ws_bytes = getattr(workspace, "nbytes_full", workspace.nbytes)
    res = dict(disp=out)
    if timed:
        ms = (C.c_float * 8)()
        check(lib.mc_predict_timed(C.byref(p), x0.data_ptr(), x1.data_ptr(), fl, fr, Cn, rl, rr, D, H, W, workspace.ptr,
                                   ws_bytes, out.data_ptr(), st, ms), "mc_predict_timed")
        res["stage_ms"] = dict(zip(STAGES, list(ms)))
        return res
    vl = vr = dl = dr = None
    scan = {}   # want_margins: suffix of the three keys -> the exported volume they are scanned from
    if want_volumes:
        res["volL"] = torch.empty((1, D, H, W), dtype=torch.float32, device=dev)
        res["volR"] = torch.empty((1, D, H, W), dtype=torch.float32, device=dev)
        vl, vr = res["volL"].data_ptr(), res["volR"].data_ptr()
    if want_margins:
        scan[""] = res["volL"] if want_volumes else torch.empty((1, D, H, W), dtype=torch.float32, device=dev)
        vl = scan[""].data_ptr()
        if want_right:
            scan["_right"] = res["volR"] if want_volumes else torch.empty((1, D, H, W), dtype=torch.float32, device=dev)
            vr = scan["_right"].data_ptr()
    if want_disp0:
        res["dispL0"] = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
        res["dispR0"] = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
        dl, dr = res["dispL0"].data_ptr(), res["dispR0"].data_ptr()
    if want_right:
        names = (("outlier",) if want_outlier else ()) + (("cost", "curvature") if want_confidence else ()) + ("disp_right", "outlier_right")
        for name in names:
            res[name] = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
        ex = [res[name].data_ptr() if name in res else None for name in ("outlier", "cost", "curvature", "disp_right", "outlier_right")]
        check(lib.mc_predict_views(C.byref(p), x0.data_ptr(), x1.data_ptr(), fl, fr, Cn, rl, rr, D, H, W, workspace.ptr,
                                   ws_bytes, vl, vr, dl, dr, ex[0], ex[1], ex[2], ex[3], ex[4], out.data_ptr(), st), "mc_predict_views")
    elif want_outlier or want_confidence:
        names = (("outlier",) if want_outlier else ()) + (("cost", "curvature") if want_confidence else ())
        for name in names:
            res[name] = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
        ex = [res[name].data_ptr() if name in res else None for name in ("outlier", "cost", "curvature")]
        check(lib.mc_predict_ex(C.byref(p), x0.data_ptr(), x1.data_ptr(), fl, fr, Cn, rl, rr, D, H, W, workspace.ptr,
                                ws_bytes, vl, vr, dl, dr, ex[0], ex[1], ex[2], out.data_ptr(), st), "mc_predict_ex")
    else:
        check(lib.mc_predict(C.byref(p), x0.data_ptr(), x1.data_ptr(), fl, fr, Cn, rl, rr, D, H, W, workspace.ptr,
                             ws_bytes, vl, vr, dl, dr, out.data_ptr(), st), "mc_predict")
    for suffix, vol in scan.items():
        for name in ("c1", "c2", "c2l"):
            res[name + suffix] = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
        check(lib.mc_cost_margins(vol.data_ptr(), D, H, W, None, res["c1" + suffix].data_ptr(), res["c2" + suffix].data_ptr(),
                                  res["c2l" + suffix].data_ptr(), st), "mc_cost_margins")
    del keep
    return res
