"""-m gpu: mc_predict against the CPU oracle at every value the parameter search draws (hs.GRIDS), at small shapes.

hs.py and EvalSet score candidates drawn from hs.GRIDS; test_gpu_hs.py holds a score to what main.py prints, and both sides of that
comparison run the same kernels.  Here every grid value meets the oracle, bit for bit and with identical NaN masks, in the fused call:

* one axis at a time, the rest of the table at its defaults (tests/predict_grid_cases.py: the families, their inputs and shapes);
* the corners of every grid, of the aggregation's iteration counts and of L1 x tau1 around the tile kernel's arm classes;
* the first 40 candidates of the seeded random search on ONE workspace, replaced only where a candidate needs more than is held -- what
  EvalSet._workspace does -- forwards and then backwards: every call finds the previous candidate's plan or record heads in the area;
* EvalSet's split path: mc_predict cut after the median into a held map, then the stand-alone mean2d, for every blur_sigma and blur_t;
* EvalSet.score itself against a numpy restatement of the error on the oracle's disparity maps.

tests/test_predict_grid_host.py (CPU) shows that no comparison here is vacuous: every axis moves the oracle's map, none gives NaN."""
import types

import numpy as np
import pytest

import predict_grid_cases as pg
from test_gpu_planned_routes import LIST_MAGIC, PLAN_MAGIC, heads
from train_fixtures import write_synthetic_kitti
from util import diff_report, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_dev = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def dev_inputs(fam):
    """(xb, the cost stage as stereo_predict_fused's keyword) on the device, uploaded once per family."""
    if fam not in _dev:
        x0, x1, stage = pg.inputs(fam)
        kw = dict(feat=dev(np.stack([stage["featL"], stage["featR"]]))) if "featL" in stage else dict(raw=(dev(stage["rawL"]), dev(stage["rawR"])))
        _dev[fam] = (dev(np.stack([x0, x1]))[:, None], kw)
    return _dev[fam]


def check(mc, fam, prm, want, left_only=0, ws=None):
    """One fused call under prm against the oracle's outputs `want`."""
    f = pg.FAMILIES[fam]
    xb, kw = dev_inputs(fam)
    got = mc.stereo_predict_fused(xb, dict(prm, left_only=left_only), f["D"], workspace=ws, want_volumes=True, want_disp0=True, **kw)
    torch.cuda.synchronize()
    for k in pg.COMPARED[left_only]:
        g = got[k].cpu().numpy()
        assert same_bits(g, want[k]), diff_report(g, want[k], "%s left_only=%d: %s" % (pg.label(fam, prm), left_only, k))


def fam_lo():
    return [(fam, lo) for fam in pg.FAMILIES for lo in pg.LEFT_ONLY[fam]]


@pytest.mark.parametrize("fam,axis,left_only", [(fam, axis, lo) for fam, axis in pg.axes() for lo in pg.LEFT_ONLY[fam]], ids=lambda v: str(v))
def test_one_axis_at_a_time(mc, oracle, fam, axis, left_only):
    cases = pg.axis_cases(fam, axis)
    assert len(cases) == len(dict(pg.grid(fam))[axis])          # nothing of a one-axis sweep has pi1 > pi2
    for prm in cases:
        check(mc, fam, prm, pg.want(oracle, fam, prm), left_only)


@pytest.mark.parametrize("fam,left_only", fam_lo(), ids=lambda v: str(v))
def test_corners(mc, oracle, fam, left_only):
    for name, prm in pg.corner_cases(fam):
        check(mc, fam, prm, pg.want(oracle, fam, prm), left_only)


def plan_heads(mc, ws, prm, left_only, D, H, W):
    """The heads of every direction's plan area as THIS candidate's layout places them (the areas end where its workspace_bytes end,
    not where a larger workspace held from an earlier candidate ends); None where the candidate has no plan area (predict.hip's
    make_plan: fewer than two aggregation passes)."""
    if prm["cbca_i1"] + prm["cbca_i2"] < 2 or prm["L1"] - 1 > 13:
        return None
    p = dict(prm, left_only=left_only)
    view = types.SimpleNamespace(ptr=ws.ptr, buf=ws.buf, nbytes=mc.predict.workspace_bytes(p, D, H, W))
    return heads(mc, view, D, H, W, nplan=1 if left_only and not prm["lr_check"] else 2)


@pytest.mark.parametrize("fam,left_only", fam_lo(), ids=lambda v: str(v))
def test_a_seeded_walk_on_one_workspace(mc, oracle, fam, left_only):
    f = pg.FAMILIES[fam]
    D, H, W = f["D"], f["H"], f["W"]
    cands = pg.walk(fam)
    wants = [pg.want(oracle, fam, p) for p in cands]             # once, for both passes
    ws, grown, with_plan = None, 0, {4: 0, 13: 0}               # calls that left a plan of their own arm class, per class
    for order in (range(len(cands)), reversed(range(len(cands)))):
        for i in order:
            prm = dict(cands[i], left_only=left_only)
            if ws is None or ws.nbytes < mc.predict.workspace_bytes(prm, D, H, W):      # EvalSet._workspace
                ws = None                                        # release the smaller one before taking the next
                ws = mc.predict.Workspace(prm, D, H, W, torch.device("cuda", 0))
                grown += 1
            check(mc, fam, cands[i], wants[i], left_only, ws)
            hd = plan_heads(mc, ws, cands[i], left_only, D, H, W)
            route = "no plan area"
            if hd is not None:
                lst, pln = hd[0]
                own = 4 if cands[i]["L1"] - 1 <= 4 else 13      # the tile kernel's instance for arms of at most L1 - 1
                tile = pln[0] == PLAN_MAGIC and pln[1:4] == [D, H, W]
                with_plan[own] += tile and pln[5] == own
                route = "%s%s" % ("tile kernel's plan, arm class %d%s" % (pln[5], "" if pln[5] == own else " (an earlier candidate's)") if tile
                                  else "no plan head", "; records, overflow word %d" % lst[1] if lst[6] == LIST_MAGIC else "")
            print("%s left_only=%d candidate %2d: %s" % (pg.label(fam, cands[i]), left_only, i, route))
    print("%s: %d workspaces taken, calls that left the tile kernel's plan head of their own arm class in place: %r" % (fam, grown, with_plan))
    if fam == "E":   # the real-scene shape: the plan is taken in both arm classes, each finding the other's head from the candidate before
        assert with_plan[4] >= 1 and with_plan[13] >= 1, "the walk did not take the tile kernel's planned passes: %r" % (with_plan,)


@pytest.mark.parametrize("fam", ["A", "B", "C"])
def test_evalset_split_path(mc, oracle, fam):
    """What EvalSet.score runs with reuse on: mc_predict with sm_terminate = 'median' into a map that is held, then adcensus.mean2d on
    adcensus.gaussian per blur-only candidate; mb with left_only = 1.  Two upstream tables in turn into the same map."""
    f = pg.FAMILIES[fam]
    D, H, W = f["D"], f["H"], f["W"]
    xb, kw = dev_inputs(fam)
    g, b = dict(pg.grid(fam)), pg.base(fam)
    left_only = 1 if f["dataset"] == "mb" else 0
    held = torch.empty((1, 1, H, W), dtype=torch.float32, device=xb.device)
    ws = mc.predict.Workspace(dict(b, left_only=left_only, sm_terminate="median"), D, H, W, xb.device)
    gauss = {}
    for up in (b, dict(pg.corner_cases(fam))["lowest"]):
        cut = dict(up, sm_terminate="median")
        mc.stereo_predict_fused(xb, dict(cut, left_only=left_only), D, workspace=ws, out=held, **kw)
        torch.cuda.synchronize()
        med = held.cpu().numpy()
        w = pg.want(oracle, fam, cut)["disp"]
        assert same_bits(med, w), diff_report(med, w, "%s: the held map" % pg.label(fam, up))
        blurs = [(s, up["blur_t"]) for s in g["blur_sigma"]] + [(up["blur_sigma"], t) for t in g["blur_t"]]
        for sigma, t in blurs:
            if sigma not in gauss:
                gauss[sigma] = mc.adcensus.gaussian(sigma).cuda()
            got = mc.adcensus.mean2d(held, gauss[sigma], t).cpu().numpy()
            w = pg.want(oracle, fam, dict(up, blur_sigma=sigma, blur_t=t))["disp"]
            assert same_bits(got, w), diff_report(got, w, "%s: blur_sigma=%g blur_t=%g of the held map" % (pg.label(fam, up), sigma, t))
        assert same_bits(held.cpu().numpy(), med)                # the blurs left the held map alone


# ---- the score -------------------------------------------------------------------------------------------------------------------
DISP_MAX = 32


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    d = tmp_path_factory.mktemp("predict_grid")
    write_synthetic_kitti(str(d / "data.kitti"))      # 6 images of 48 x 160, two of them test images
    return d


@pytest.mark.parametrize("arch", ["census", "fast"])
def test_score_equals_the_error_of_the_oracles_maps(mc, oracle, arch, data_root, monkeypatch):
    """EvalSet.score against the error of the ORACLE's disparity maps (test_gpu_hs.py holds it to main.py's, which runs the same
    kernels).  The cost stage: oracle.census on the CPU; for arch fast each example's features from the device (the net is held to
    1e-4 elsewhere, not to bits, and this test is not about it)."""
    from mc_cnn_amd import hs
    from mc_cnn_amd.evalset import EvalSet
    monkeypatch.chdir(data_root)
    net = "random:3"
    opt = hs.parse(["random", "kitti", arch, "test_te", net, "-disp_max", str(DISP_MAX)])
    layers, fc = hs.check_net(net, "kitti", arch)
    es = EvalSet("kitti", arch, opt, layers, fc, torch.device("cuda", 0), 1 << 30)
    assert es.n == 2 and es.n_cached == 2
    examples = []
    for e in es.examples:
        H, W = e["H"], e["W"]
        xb = e["xb"].cpu().numpy()
        x0, x1 = xb[0].reshape(1, H, W), xb[1].reshape(1, H, W)
        if arch == "census":
            stage = dict(rawL=oracle.census(x0, x1, DISP_MAX, -1), rawR=oracle.census(x1, x0, DISP_MAX, 1))
        else:
            ft = e["stage"]["feat"].cpu().numpy()
            stage = dict(featL=ft[0], featR=ft[1])
        gt = e["gt"].cpu().numpy().reshape(-1, e["gt_ld"])[:H, :W]
        examples.append((x0[0], x1[0], stage, gt))
    g = hs.grid_of("kitti", arch)
    scores = []
    for prm in [dict(es.prm)] + pg.walk_of(g, dict(es.prm), 5):
        errs = []
        for x0, x1, stage, gt in examples:
            with np.errstate(all="ignore"):
                pred = oracle.stereo_predict(prm, x0, x1, DISP_MAX, **stage)["disp"]
            mask = gt != 0                                       # main.lua:1224-1234, restated
            bad = (np.abs(gt - pred) > 3) & mask
            errs.append(float(bad.sum()) / float(mask.sum()))
        want = sum(errs) / len(errs)
        got = es.score(prm)
        print("kitti", arch, " ".join("%s=%g" % (k, prm[k]) for k, _ in g), got, want)
        assert got == want
        scores.append(got)
    assert len(set(scores)) > 1, "the six candidates all score alike: the comparison cannot tell them apart"
