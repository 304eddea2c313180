"""-m gpu: the vertical SGM sweeps leave the cost volumes' NaN triangle alone on the feature path.

Where mc_predict made the volumes itself (stereo_join_hwd + fix_border_hwd), every voxel whose partner pixel lies outside
the image (left volume d > x, right volume x + d >= W) is NaN, and the down and up sweeps neither load nor store the lanes
at d >= Dv of their column.  Every case runs from features, with both volumes, left.bin only and no volume asked for (the
timed call form, where the up sweep also drops the right volume's stores), each on a workspace pre-filled with NaN and with
1e3: all runs agree bit for bit on what they share and with the CPU oracle.  A raw-volume call, whose triangle may hold
finite values, must still equal the oracle: the promise is not made there."""
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


class FilledWorkspace:
    """mc_predict's workspace, every float of it `fill` before the call"""

    def __init__(self, nbytes, fill):
        self.nbytes = nbytes
        self.buf = torch.full(((nbytes + 256) // 4 + 1,), fill, dtype=torch.float32, device="cuda")
        self.ptr = self.buf.data_ptr() + (-self.buf.data_ptr()) % 256


def _run(mc, prm, xb, D, outs, fill, feat=None, raw=None):
    """mc_predict writing `disp` and the outputs named in `outs`"""
    from mc_cnn_amd._lib import check, lib

    p = mc.make_params(prm)
    H, W = xb.shape[-2:]
    x = xb.reshape(2, H, W)
    x0, x1 = x[0].contiguous(), x[1].contiguous()
    ws = FilledWorkspace(mc.predict.workspace_bytes(prm, D, H, W, feat.shape[-3] if feat is not None else 0), fill)
    res = {"disp": torch.empty((1, 1, H, W), dtype=torch.float32, device="cuda")}
    for k in outs:
        res[k] = torch.empty((1, D if k.startswith("vol") else 1, H, W), dtype=torch.float32, device="cuda")
    fl = fr = rl = rr = None
    Cn = 0
    if feat is not None:
        Cn = feat.shape[-3]
        fl, fr = feat[0].data_ptr(), feat[1].data_ptr()
    else:
        rl, rr = raw[0].data_ptr(), raw[1].data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda k: res[k].data_ptr() if k in res else None
    check(lib.mc_predict(C.byref(p), x0.data_ptr(), x1.data_ptr(), fl, fr, Cn, rl, rr, D, H, W, ws.ptr, ws.nbytes,
                         ptr("volL"), ptr("volR"), ptr("dispL0"), ptr("dispR0"), res["disp"].data_ptr(), st), "mc_predict")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _check(mc, prm, xb, D, want, right, **kw):
    """Three call forms x two workspace fills; every output against the oracle (hence against every other run).
    right = False: one volume only (left_only without the LR check) -- nothing of the right volume is asked for or compared
    outside the first form, which asks for everything and so runs both volumes."""
    from util import diff_report, same_bits

    forms = [
        ("both volumes", ("volL", "volR", "dispL0", "dispR0")),
        ("left.bin only", ("volL", "dispL0", "dispR0") if right else ("volL", "dispL0")),
        ("no volume", ()),
    ]
    first = None
    for form, outs in forms:
        for fill in (float("nan"), 1e3):
            got = _run(mc, prm, xb, D, outs, fill, **kw)
            what = "%s, workspace pre-filled with %g" % (form, fill)
            for k, g in got.items():
                if k in ("volR", "dispR0") and not right:
                    continue
                w = want[k]
                assert same_bits(g.reshape(w.shape), w), diff_report(g.reshape(w.shape), w, "%s (%s) against the oracle" % (k, what))
            if first is None:
                first = got
            for k, g in got.items():   # (implied by the oracle where it is compared; the right outputs of a one-volume case are not)
                assert same_bits(g, first[k]), diff_report(g, first[k], "%s (%s) against the first run" % (k, what))


CASES = [
    # H, W, D, C, preset overrides
    (6, 9, 12, 4, {}),                    # W < D: every column of both volumes is trimmed, Dv = 1..9 never reaches D
    (5, 40, 37, 8, {}),                   # D % 4 != 0 (ds = 40): Dv inside 16-byte pieces; the triangles overlap in the middle columns
    (40, 24, 20, 4, {}),                  # H > 16: the ring's steady-state loop and its remainder (2 * 16 + 8)
    (1, 33, 16, 4, {}),                   # the border step alone
    (2, 33, 16, 4, {}),                   # and one step after it
    (4, 300, 260, 4, {}),                 # D > 256: the instances with 8 disparities per lane
    (5, 20, 18, 4, {"border_n": 4}),      # fix_border's source column (15) lies inside the triangle region
    (7, 64, 32, 16, {"border_n": 4}),     # an ordinary shape with a border
    (5, 40, 37, 8, {"sgm_i": 2}),         # a second iteration reads the first one's output
    (5, 40, 37, 8, {"left_only": 1, "lr_check": 0}),   # one volume
]


@pytest.mark.parametrize("H,W,D,Cn,over", CASES,
                         ids=["-".join(["%dx%dx%dx%d" % c[:4]] + ["%s=%s" % kv for kv in c[4].items()]) for c in CASES])
def test_vertical_sweeps_skip_the_nan_triangle(mc, oracle, H, W, D, Cn, over):
    from util import diff_report, features, same_bits, smooth_pair

    prm = dict(mc.PRESETS["kitti_fast"])
    prm.update(over)
    assert prm["cbca_i1"] == 0 and prm["cbca_i2"] == 0 and prm["sgm_i"] >= 1   # the path that makes the promise
    x0, x1 = smooth_pair(H, W, min(D, 10), seed=21)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    f = features(Cn, H, W, seed=22)
    want = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
    right = not over.get("left_only")
    feat = torch.from_numpy(f).cuda()

    got = mc.stereo_predict_fused(xb, prm, D, feat=feat, want_volumes=True, want_disp0=True)
    torch.cuda.synchronize()
    for k in ("volL", "volR", "dispL0", "dispR0", "disp") if right else ("volL", "dispL0", "disp"):
        g = got[k].cpu().numpy().reshape(want[k].shape)
        assert same_bits(g, want[k]), diff_report(g, want[k], k + " (stereo_predict_fused)")
    _check(mc, prm, xb, D, want, right, feat=feat)


def test_raw_volumes_with_a_finite_triangle_are_swept_whole(mc, oracle):
    """a caller's volumes need not have the triangle: finite costs there take part in the recurrence as before"""
    from util import raw_volumes, smooth_pair

    H, W, D = 5, 40, 37
    prm = dict(mc.PRESETS["kitti_fast"])
    x0, x1 = smooth_pair(H, W, 10, seed=23)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    vl, vr = raw_volumes(D, H, W, seed=24)
    rng = np.random.default_rng(25)
    for v in (vl, vr):
        n = np.isnan(v)
        assert n.any()
        v[n] = rng.random(int(n.sum()), dtype=np.float32)
    want = oracle.stereo_predict(prm, x0, x1, D, rawL=vl, rawR=vr)
    _check(mc, prm, xb, D, want, True, raw=(torch.from_numpy(vl).cuda(), torch.from_numpy(vr).cuda()))
