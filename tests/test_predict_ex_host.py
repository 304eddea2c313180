"""CPU: mc_predict_ex, mc_predict with three more optional outputs (the LR check's class map, and the cost and the curvature of the cost
curve at the disparity the sub-pixel stage reads), as far as it can be held without a GPU: the symbol and its declarations, the refusals,
all of which precede the first launch (fake non-null device pointers: nothing is dereferenced before the checks pass, and every call
here is one that must be refused), `main.py -extras`, and `predict_kitti.py -sparse` on a fake predictor."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
D, H, W = 8, 12, 40
MAP = 4 * H * W
# fake device addresses: a 256-byte aligned workspace and buffers far enough apart for a (D,H,W) volume each
WS, X0, X1, FL, FR, DISP, VOLL, VOLR, DL0, DR0, OUTL, COST, CURV = (0x10000000 + k * 0x1000000 for k in range(13))


def call(lib, p, ws_bytes, outl=None, cost=None, curv=None, ex=True, disp=DISP, vols=(None, None), disp0=(None, None), **kw):
    a = dict(x0=X0, x1=X1, fl=FL, fr=FR, Cn=16, rl=None, rr=None, D=D, H=H, W=W, ws=WS)
    a.update(kw)
    head = (C.byref(p), a["x0"], a["x1"], a["fl"], a["fr"], a["Cn"], a["rl"], a["rr"], a["D"], a["H"], a["W"], a["ws"], ws_bytes,
            vols[0], vols[1], disp0[0], disp0[1])
    rc = lib.mc_predict_ex(*head, outl, cost, curv, disp, None) if ex else lib.mc_predict(*head, disp, None)
    return rc, lib.mc_last_error().decode()


@pytest.fixture(scope="module")
def setup(mc):
    lib = mc._lib.lib
    p = mc.make_params("kitti_fast")
    return lib, mc, lib.mc_predict_workspace_bytes(C.byref(p), 16, D, H, W)


def test_symbol_is_exported_declared_and_bound(mc):
    assert "mc_predict_ex" in mc._lib.SYMBOLS
    lib = C.CDLL(mc._lib.LIB_PATH)
    assert hasattr(lib, "mc_predict_ex")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mc_adcensus.h")).read(), flags=re.S)
    m = re.search(r"int mc_predict_ex\((.*?)\);", header, flags=re.S)
    assert m, "include/mc_adcensus.h does not declare mc_predict_ex"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 22 == len(mc._lib.lib.mc_predict_ex.argtypes)
    assert args[17:20] == ["float *outlier_out", "float *cost_out", "float *curv_out"] and args[20] == "float *disp_out"
    # mc_predict's own arguments, in its order, around the three new ones
    m0 = re.search(r"int mc_predict\((.*?)\);", header, flags=re.S)
    args0 = [a.strip() for a in m0.group(1).split(",")]
    assert args[:17] + args[20:] == args0
    lua = open(os.path.join(ROOT, "mc-cnn_amd", "lua", "adcensus.lua")).read()
    assert "int mc_predict_ex(" in lua and "lib.mc_predict_ex(" in lua
    assert mc._lib.lib.mc_version() == 8 and C.sizeof(mc.params.McParams) == 88


BAD = [   # (what is wrong, keyword overrides of call(), parameter overrides): each refused by mc_predict in front of its first launch
    ("no disparity output", dict(disp=None), {}),
    ("neither features nor volumes", dict(fl=None, fr=None, Cn=0), {}),
    ("range beyond the limit", dict(D=1025), {}),
    ("bad dims", dict(H=0), {}),
    ("even median", {}, dict(median_k=4)),
    ("bad stage name", {}, dict(sm_terminate=10)),
    ("border beyond the row", {}, dict(border_n=W)),
    ("too many channels", dict(Cn=129), {}),
    ("unaligned workspace", dict(ws=WS + 16), {}),
    ("small workspace", dict(short=1), {}),
]


@pytest.mark.parametrize("what,kw,over", BAD, ids=[b[0] for b in BAD])
def test_without_extras_a_bad_call_is_refused_as_mc_predict_refuses_it(setup, what, kw, over):
    lib, mc, ws_bytes = setup
    p = mc.make_params("kitti_fast")
    for k, v in over.items():
        setattr(p, k, v)
    kw = dict(kw)
    ws_bytes -= kw.pop("short", 0)
    want = call(lib, p, ws_bytes, ex=False, **kw)
    got = call(lib, p, ws_bytes, **kw)
    assert want[0] == EINVAL and want[1].startswith("mc_predict: ")
    assert got == want, what
    # ... and the same in front of the extras' own checks, which come last
    assert call(lib, p, ws_bytes, outl=OUTL, cost=DISP, curv=CURV, **kw) == want, what


SUBPIXEL_OFF = [dict(sm_skip="subpixel_enchancement")] + [dict(sm_terminate=t) for t in ("cnn", "cbca1", "sgm", "cbca2", "occlusion", "mismatch")]


@pytest.mark.parametrize("sw", SUBPIXEL_OFF, ids=lambda d: "%s=%s" % tuple(d.items())[0])
@pytest.mark.parametrize("which", ["cost_out", "curv_out"])
def test_confidence_maps_are_refused_where_the_subpixel_stage_does_not_run(setup, sw, which):
    lib, mc, _ = setup
    p = mc.make_params(dict(mc.PRESETS["kitti_fast"], **sw))
    ws_bytes = lib.mc_predict_workspace_bytes(C.byref(p), 16, D, H, W)
    rc, msg = call(lib, p, ws_bytes, **{"cost" if which == "cost_out" else "curv": COST})
    assert rc == EINVAL
    assert msg == "mc_predict_ex: %s is written by the sub-pixel stage, which sm_terminate=%d / sm_skip=%d leave out" % (
        which, p.sm_terminate, p.sm_skip)


def test_without_the_lr_check_its_stage_names_end_nothing(setup):
    """-sm_terminate occlusion / mismatch name stages that lr_check = 0 does not have (main.lua:1054-1066): the sub-pixel stage runs, so
    the maps are not refused for that -- shown on a call that is refused for another reason, behind that check."""
    lib, mc, _ = setup
    for t in ("occlusion", "mismatch"):
        p = mc.make_params(dict(mc.PRESETS["mb_slow"], sm_terminate=t))
        ws_bytes = lib.mc_predict_workspace_bytes(C.byref(p), 16, D, H, W)
        rc, msg = call(lib, p, ws_bytes, cost=COST, curv=COST)
        assert rc == EINVAL and msg == "mc_predict_ex: curv_out overlaps cost_out"
        p.lr_check = 1
        rc, msg = call(lib, p, ws_bytes, cost=COST, curv=COST)
        assert rc == EINVAL and msg.startswith("mc_predict_ex: cost_out is written by the sub-pixel stage")


ARG = dict(outl="outlier_out", cost="cost_out", curv="curv_out")


@pytest.mark.parametrize("extra", sorted(ARG))
def test_an_extra_output_may_not_overlap_anything_the_call_writes(setup, extra):
    lib, mc, ws_bytes = setup
    p = mc.make_params("kitti_fast")
    full = dict(vols=(VOLL, VOLR), disp0=(DL0, DR0))
    others = [("disp_out", DISP, MAP), ("volL_out", VOLL, D * MAP), ("volR_out", VOLR, D * MAP), ("dispL0_out", DL0, MAP),
              ("dispR0_out", DR0, MAP), ("the workspace", WS, ws_bytes)]
    for name, at, size in others:
        for where in (at, at + size - 4, at - MAP + 4):   # the same start, the last float of the other, the last float of the extra
            rc, msg = call(lib, p, ws_bytes, **{extra: where}, **full)
            assert rc == EINVAL and msg == "mc_predict_ex: %s overlaps %s" % (ARG[extra], name), (name, hex(where))
    order = ["outl", "cost", "curv"]
    for other in order:
        if other == extra:
            continue
        later, earlier = (extra, other) if order.index(extra) > order.index(other) else (other, extra)
        rc, msg = call(lib, p, ws_bytes, **{extra: OUTL, other: OUTL + MAP - 4}, **full)
        assert rc == EINVAL and msg == "mc_predict_ex: %s overlaps %s" % (ARG[later], ARG[earlier])


def test_workspace_sizes_do_not_depend_on_the_extras(mc):
    """the maps are the caller's: mc_predict_workspace_bytes[_full] are what tests/test_abi.py pins (spot check of its table)"""
    lib = mc._lib.lib
    p = mc.make_params("kitti_fast")
    assert lib.mc_predict_workspace_bytes(C.byref(p), 0, 228, 370, 1226) == 2519785984


def test_main_takes_extras_with_predict_only():
    from mc_cnn_amd import main as mcmain
    for dataset in ("kitti", "kitti2015", "mb"):
        for arch in ("fast", "slow", "ad", "census"):
            assert mcmain.parse([dataset, arch, "-a", "predict", "-extras"])[2].extras is True
            assert mcmain.parse([dataset, arch, "-extras"])[2].extras is True            # -a predict is the default
            assert mcmain.parse([dataset, arch, "-a", "predict"])[2].extras is False
    with pytest.raises(SystemExit) as e:
        mcmain.parse(["kitti", "fast", "-a", "time", "-extras"])
    assert "-extras" in str(e.value) and "-a predict" in str(e.value)
    with pytest.raises(SystemExit):
        mcmain.parse(["kitti", "fast", "-a", "test_te", "-extras"])


def test_predict_kitti_takes_sparse():
    from mc_cnn_amd import predict_kitti as pk
    assert pk.parse(["test"]).sparse is False and pk.parse(["submit", "-n", "3"]).sparse is False
    assert pk.parse(["test", "-sparse"]).sparse is True and pk.parse(["submit", "-sparse", "-n", "3"]).sparse is True


def test_predict_kitti_sparse_on_a_fake_predictor(tmp_path):
    """submit -sparse: 0 wherever the class is not 0; test -sparse: the error over the ground-truth pixels of class 0, their share of all
    ground-truth pixels, per pair and summed; without the flag the run is what it was."""
    from PIL import Image
    from mc_cnn_amd import binio, predict_kitti as pk
    root = tmp_path / "unzip"
    for d in ("training/image_0", "training/image_1", "training/disp_noc", "testing/image_0", "testing/image_1"):
        (root / d).mkdir(parents=True)
    h, w, n = 6, 9, 3
    rng = np.random.default_rng(1)
    gts, disps, classes = [], [], []
    for i in range(n):
        for cam in (0, 1):
            for d in ("training", "testing"):
                Image.fromarray(rng.integers(0, 255, (h, w), dtype=np.uint8)).save(root / ("%s/image_%d/%06d_10.png" % (d, cam, i)))
        gt = rng.integers(1, 40, (h, w)).astype(np.float32)
        gt[rng.random((h, w)) < 0.3] = 0            # no ground truth
        binio.write_png16(gt, str(root / ("training/disp_noc/%06d_10.png" % i)))
        gts.append(gt)
        disps.append((gt + rng.choice([0.0, 1.0, 5.0], (h, w))).astype(np.float32) + 1)   # (+ 1: no 0 among the estimates)
        classes.append(rng.choice([0.0, 1.0, 2.0], (h, w), p=[0.6, 0.2, 0.2]).astype(np.float32))
    classes[2][gts[2] != 0] = 1                     # a pair without a single kept ground-truth pixel
    for c in classes[:2]:
        assert set(np.unique(c)) == {0.0, 1.0, 2.0}

    def index(im0):
        return int(os.path.basename(im0)[:6])

    def dense(im0, im1):
        return disps[index(im0)]

    def sparse(im0, im1):
        return disps[index(im0)], classes[index(im0)]

    logs = []
    err_sum, done, density_sum = pk.run("test", str(root), sparse, n_pairs=n, log=lambda *a: logs.append(a), sparse=True)
    assert done == n and [a[0] for a in logs] == [0, 1, 2] and all(len(a) == 3 for a in logs)
    want_err, want_density = [], []
    for i in range(n):
        gt_mask = gts[i] != 0
        kept = gt_mask & (classes[i] == 0)
        bad = (np.abs(disps[i] - gts[i]) > 3) & kept
        want_err.append(bad.sum() / kept.sum() if kept.sum() else 0.0)
        want_density.append(kept.sum() / gt_mask.sum())
    assert [a[1] for a in logs] == want_err and [a[2] for a in logs] == want_density
    assert want_density[2] == 0.0 and want_err[2] == 0.0 and 0.3 < want_density[0] < 0.9
    assert abs(err_sum - sum(want_err)) < 1e-12 and abs(density_sum - sum(want_density)) < 1e-12
    # the dense error differs: the pixels that were filled in count there
    logs_dense = []
    total, done = pk.run("test", str(root), dense, n_pairs=n, log=lambda *a: logs_dense.append(a))
    assert done == n and all(len(a) == 2 for a in logs_dense)
    assert [a[1] for a in logs_dense] == [pk.three_pixel_error(disps[i], gts[i]) for i in range(n)]
    assert [a[1] for a in logs_dense] != want_err
    # a staged predictor with pairs in flight: same results
    class Staged:
        def submit(self, im0, im1):
            return (im0, im1)

        def result(self, t):
            return sparse(*t)

    again = pk.run("test", str(root), Staged(), n_pairs=n, log=lambda *a: None, in_flight=2, sparse=True)
    assert again == (err_sum, done, density_sum)
    # submit
    out_s, out_d = tmp_path / "sparse", tmp_path / "dense"
    assert pk.run("submit", str(root), sparse, n_pairs=n, out_dir=str(out_s), log=lambda *a: None, sparse=True) == (0.0, n, 0.0)
    assert pk.run("submit", str(root), dense, n_pairs=n, out_dir=str(out_d), log=lambda *a: None) == (0.0, n)
    assert sorted(os.listdir(out_s)) == sorted(os.listdir(out_d)) == ["%06d_10.png" % i for i in range(n)]
    for i in range(n):
        got_s = binio.read_png16(str(out_s / ("%06d_10.png" % i)))
        got_d = binio.read_png16(str(out_d / ("%06d_10.png" % i)))
        assert np.array_equal(got_d, disps[i]) and (got_d != 0).all()
        assert np.array_equal(got_s, np.where(classes[i] == 0, disps[i], 0))
        assert ((got_s == 0) == (classes[i] != 0)).all()
