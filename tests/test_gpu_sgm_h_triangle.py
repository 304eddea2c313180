"""-m gpu: the horizontal SGM sweeps leave the cost volumes' NaN triangle alone where nothing reads it.

On the feature path (stereo_join_hwd + fix_border_hwd made the volumes: NaN wherever the partner pixel lies outside the image, left
volume d > x, right volume x + d >= W) the fused horizontal launch does not load C in the triangle, does not store the second
direction's partial sums (out2) there and, for a volume whose final costs are dropped (the right one when right.bin is not asked
for, last SGM iteration only), does not store out there either.  The live count changes with every step of a line, so the shapes
are those at which a step's rule can go wrong: one row, W < D (every column trimmed), W = D, D % 4 != 0 (16-byte pieces straddle
the count), and a shape with and without a border.  Every case runs from features with all exports, with left.bin only and with no
volume (the last two drop the right volume's final costs), each on a workspace pre-filled with NaN and with 1e3 -- what is no
longer stored keeps the fill, and nothing may read it --, under one lane and under two, and compares disp, dispL0, dispR0, volL and
volR (where exported), NaN triangle included, bit for bit with the CPU oracle.  The library has no switch that withholds the
promise, so the oracle is the only reference."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [
    # H, W, D, C, preset overrides
    (1, 33, 16, 4, {}),                    # one row, W > D
    (3, 12, 16, 4, {}),                    # W < D: every column is trimmed, in both volumes
    (2, 16, 16, 4, {}),                    # W = D: the last column of the left / first of the right volume is the only whole one
    (5, 40, 18, 8, {}),                    # D % 4 != 0 (ds = 20): pieces straddle Dv
    (4, 70, 36, 8, {"border_n": 0}),
    (4, 70, 36, 8, {"border_n": 4}),       # more steps than two rounds of the ring (70 = 8 * 8 + 6), a border copied over the volumes' edges
    (2, 300, 36, 4, {}),                   # a long line: thirty rounds of whole columns in front of (or behind) the trimmed ones
]
IDS = ["-".join(["%dx%dx%dx%d" % c[:4]] + ["%s=%s" % kv for kv in c[4].items()]) for c in CASES]
FORMS = [
    ("all exports", ("volL", "volR", "dispL0", "dispR0")),
    ("left.bin only", ("volL", "dispL0", "dispR0")),   # the right volume's final costs are dropped
    ("no volume", ("dispL0", "dispR0")),               # likewise
]
_cache = {}


@pytest.fixture(autouse=True)
def lanes(mc):
    fn = mc._lib.lib.mc_test_predict_lanes
    fn.argtypes, fn.restype = [C.c_int], C.c_int
    yield fn
    fn(0)   # back to what the environment says


def _inputs(oracle, mc, case, sgm_i):
    """the pair, its features and the oracle's outputs: computed once per (case, sgm_i), shared, never written to"""
    from util import features, smooth_pair

    key = (CASES.index(case), sgm_i)
    if key not in _cache:
        H, W, D, Cn, over = case
        prm = dict(mc.PRESETS["kitti_fast"])
        prm.update(over)
        prm["sgm_i"] = sgm_i
        assert prm["cbca_i1"] == 0 and prm["cbca_i2"] == 0   # the path that makes the promise
        x0, x1 = smooth_pair(H, W, min(D, 10), seed=31 + key[0])
        f = features(Cn, H, W, seed=41 + key[0])
        want = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
        _cache[key] = (prm, np.stack([x0, x1])[:, None], f, want)
    return _cache[key]


def _run(mc, prm, xb, feat, D, outs, fill):
    """mc_predict on a workspace every float of which is `fill`, writing disp and the outputs named in `outs`"""
    from mc_cnn_amd._lib import check, lib

    p = mc.make_params(prm)
    H, W = xb.shape[-2:]
    x = xb.reshape(2, H, W)
    x0, x1 = x[0].contiguous(), x[1].contiguous()
    nbytes = mc.predict.workspace_bytes(prm, D, H, W, feat.shape[-3])
    buf = torch.full(((nbytes + 256) // 4 + 1,), fill, dtype=torch.float32, device="cuda")
    ws = buf.data_ptr() + (-buf.data_ptr()) % 256
    res = {"disp": torch.empty((1, 1, H, W), dtype=torch.float32, device="cuda")}
    for k in outs:
        res[k] = torch.empty((1, D if k.startswith("vol") else 1, H, W), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda k: res[k].data_ptr() if k in res else None
    check(lib.mc_predict(C.byref(p), x0.data_ptr(), x1.data_ptr(), feat[0].data_ptr(), feat[1].data_ptr(), feat.shape[-3], None, None,
                         D, H, W, ws, nbytes, ptr("volL"), ptr("volR"), ptr("dispL0"), ptr("dispR0"), res["disp"].data_ptr(), st),
          "mc_predict")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("n_lanes", [1, 2])
@pytest.mark.parametrize("sgm_i", [1, 2])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_horizontal_sweeps_skip_the_nan_triangle(mc, oracle, lanes, case, sgm_i, n_lanes):
    from util import diff_report, same_bits

    prm, x, f, want = _inputs(oracle, mc, case, sgm_i)
    D = case[2]
    xb, feat = torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda()
    assert lanes(n_lanes) == n_lanes
    for form, outs in FORMS:
        for fill in (float("nan"), 1e3):
            got = _run(mc, prm, xb, feat, D, outs, fill)
            for k, g in got.items():
                w = want[k]
                assert same_bits(g.reshape(w.shape), w), diff_report(
                    g.reshape(w.shape), w, "%s (%s, %d lane(s), workspace pre-filled with %g) against the oracle" % (k, form, n_lanes, fill))


@pytest.mark.parametrize("sgm_i", [1, 2])
def test_exported_volumes_keep_their_triangle(mc, oracle, lanes, sgm_i):
    """left.bin (and right.bin where it is asked for) is NaN at every voxel of the triangle, and has the oracle's NaN mask, though the
    workspace held 1e3 everywhere before: sub-pixel refinement and a later SGM iteration read those NaNs out of the same buffer"""
    case = CASES[3]
    H, W, D = case[:3]
    prm, x, f, want = _inputs(oracle, mc, case, sgm_i)
    xb, feat = torch.from_numpy(x).cuda(), torch.from_numpy(f).cuda()
    d, xs = np.arange(D)[:, None, None], np.arange(W)[None, None, :]
    tri_l = np.broadcast_to(d > xs, (D, H, W))
    tri_r = np.broadcast_to(xs + d >= W, (D, H, W))
    assert tri_l.any() and not tri_l.all()
    for n in (1, 2):
        assert lanes(n) == n
        for form, outs in FORMS[:2]:
            got = _run(mc, prm, xb, feat, D, outs, 1e3)
            for k, tri in (("volL", tri_l), ("volR", tri_r)):
                if k in got:
                    isn = np.isnan(got[k].reshape(D, H, W))
                    assert isn[tri].all(), "%s, %d lane(s): %s holds %d numbers inside the triangle" % (form, n, k, int((~isn[tri]).sum()))
                    assert np.array_equal(isn, np.isnan(want[k].reshape(D, H, W))), "%s, %d lane(s): %s's NaN mask is not the oracle's" % (form, n, k)
