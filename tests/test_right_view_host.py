"""CPU: mc_predict_views, mc_predict_ex with the right view's finished disparity map and class map, as far as it can be held without a
GPU: the symbol and its declarations, the Lua prototype, `main.py -right_view`, the refusals (all of which precede the first launch: fake
non-null device pointers, nothing is dereferenced before the checks pass, and every call here is one that must be refused), and the
definition itself (tests/right_view_cases.py) on a pair whose answer is known."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import right_view_cases as rv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
D, H, W = 8, 12, 40
MAP = 4 * H * W
# fake device addresses: a 256-byte aligned workspace and buffers far enough apart for a (D,H,W) volume each
WS, X0, X1, FL, FR, DISP, VOLL, VOLR, DL0, DR0, OUTL, COST, CURV, DISPR, OUTLR = (0x10000000 + k * 0x1000000 for k in range(15))


def call(lib, p, ws_bytes, dispR=None, outlR=None, outl=None, cost=None, curv=None, disp=DISP, vols=(None, None), disp0=(None, None), views=True, **kw):
    a = dict(x0=X0, x1=X1, fl=FL, fr=FR, Cn=16, rl=None, rr=None, D=D, H=H, W=W, ws=WS)
    a.update(kw)
    head = (C.byref(p), a["x0"], a["x1"], a["fl"], a["fr"], a["Cn"], a["rl"], a["rr"], a["D"], a["H"], a["W"], a["ws"], ws_bytes,
            vols[0], vols[1], disp0[0], disp0[1], outl, cost, curv)
    rc = lib.mc_predict_views(*head, dispR, outlR, disp, None) if views else lib.mc_predict_ex(*head, disp, None)
    return rc, lib.mc_last_error().decode()


@pytest.fixture(scope="module")
def setup(mc):
    lib = mc._lib.lib
    p = mc.make_params("kitti_fast")
    return lib, mc, lib.mc_predict_workspace_bytes(C.byref(p), 16, D, H, W)


def prototype(text, name):
    m = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S)
    assert m, "no prototype of %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbol_is_exported_declared_and_bound(mc):
    import libraries as L
    assert "mc_predict_views" in mc._lib.SYMBOLS
    assert "mc_predict_views" in L.exported_abi(mc._lib.LIB_PATH)
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mc_adcensus.h")).read(), flags=re.S)
    assert "mc_predict_views" in L.header_symbols(header)
    assert L.exported_abi(mc._lib.LIB_PATH) - L.TEST_HOOKS["libmcadcensus.so"] == L.header_symbols(header) == set(mc._lib.SYMBOLS)
    args = prototype(header, "mc_predict_views")
    assert len(args) == 24 == len(mc._lib.lib.mc_predict_views.argtypes)
    assert args[20:22] == ["float *dispR_out", "float *outlierR_out"] and args[22] == "float *disp_out"
    # mc_predict_ex's own arguments, in its order, around the two new ones
    assert args[:20] + args[22:] == prototype(header, "mc_predict_ex")
    assert mc._lib.lib.mc_version() == mc._lib.ABI_VERSION == 8 and "#define MC_ABI_VERSION 8" in header
    assert C.sizeof(mc.params.McParams) == 88


def test_lua_cdef_carries_the_prototype():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mc_adcensus.h")).read(), flags=re.S)
    lua = open(os.path.join(ROOT, "mc-cnn_amd", "lua", "adcensus.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    assert prototype(cdef, "mc_predict_views") == prototype(header, "mc_predict_views")
    assert "lib.mc_predict_views(" in lua and "'disp_right'" in lua and "'outlier_right'" in lua


def test_main_takes_right_view_with_predict_only():
    from mc_cnn_amd import main as mcmain
    for dataset in ("kitti", "kitti2015", "mb"):
        for arch in ("fast", "slow", "ad", "census"):
            assert mcmain.parse([dataset, arch, "-a", "predict", "-right_view"])[2].right_view is True
            assert mcmain.parse([dataset, arch, "-right_view", "-extras"])[2].right_view is True     # -a predict is the default
            assert mcmain.parse([dataset, arch, "-a", "predict"])[2].right_view is False
    for action in ("time", "test_te"):
        with pytest.raises(SystemExit) as e:
            mcmain.parse(["kitti", "fast", "-a", action, "-right_view"])
        assert "-right_view" in str(e.value) and "-a predict" in str(e.value)


BAD = [   # (what is wrong, keyword overrides of call(), parameter overrides): each refused by mc_predict in front of its first launch
    ("no disparity output", dict(disp=None), {}),
    ("neither features nor volumes", dict(fl=None, fr=None, Cn=0), {}),
    ("bad dims", dict(H=0), {}),
    ("even median", {}, dict(median_k=4)),
    ("unaligned workspace", dict(ws=WS + 16), {}),
    ("small workspace", dict(short=1), {}),
]


@pytest.mark.parametrize("what,kw,over", BAD, ids=[b[0] for b in BAD])
def test_a_bad_call_is_refused_as_mc_predict_ex_refuses_it(setup, what, kw, over):
    lib, mc, ws_bytes = setup
    p = mc.make_params("kitti_fast")
    for k, v in over.items():
        setattr(p, k, v)
    kw = dict(kw)
    ws_bytes -= kw.pop("short", 0)
    want = call(lib, p, ws_bytes, views=False, **kw)
    assert want[0] == EINVAL and want[1].startswith("mc_predict: ")
    assert call(lib, p, ws_bytes, **kw) == want, what
    assert call(lib, p, ws_bytes, dispR=DISPR, outlR=OUTLR, **kw) == want, what
    # ... and in front of the new maps' own check
    assert call(lib, p, ws_bytes, dispR=DISP, outlR=DISP, **kw) == want, what


def test_with_both_maps_null_the_refusals_are_mc_predict_exs(setup):
    lib, mc, ws_bytes = setup
    p = mc.make_params(dict(mc.PRESETS["kitti_fast"], sm_terminate="sgm"))
    ws_bytes = lib.mc_predict_workspace_bytes(C.byref(p), 16, D, H, W)
    want = call(lib, p, ws_bytes, cost=COST, views=False)
    assert want[0] == EINVAL and want[1].startswith("mc_predict_ex: cost_out is written by the sub-pixel stage")
    assert call(lib, p, ws_bytes, cost=COST) == want
    assert call(lib, p, ws_bytes, outl=OUTL, cost=OUTL, views=False) == call(lib, p, ws_bytes, outl=OUTL, cost=OUTL)


ARG = dict(dispR="dispR_out", outlR="outlierR_out")


@pytest.mark.parametrize("view", sorted(ARG))
def test_a_right_view_map_may_not_overlap_anything_the_call_writes(setup, view):
    lib, mc, ws_bytes = setup
    p = mc.make_params("kitti_fast")
    full = dict(vols=(VOLL, VOLR), disp0=(DL0, DR0), outl=OUTL, cost=COST, curv=CURV)
    others = [("disp_out", DISP, MAP), ("volL_out", VOLL, D * MAP), ("volR_out", VOLR, D * MAP), ("dispL0_out", DL0, MAP),
              ("dispR0_out", DR0, MAP), ("the workspace", WS, ws_bytes), ("outlier_out", OUTL, MAP), ("cost_out", COST, MAP),
              ("curv_out", CURV, MAP)]
    for name, at, size in others:
        for where in (at, at + size - 4, at - MAP + 4):   # the same start, the last float of the other, the last float of the map
            rc, msg = call(lib, p, ws_bytes, **{view: where}, **full)
            assert rc == EINVAL and msg == "mc_predict_views: %s overlaps %s" % (ARG[view], name), (name, hex(where))
    # each other: the later argument is the one named first
    for a, b in ((DISPR, DISPR), (DISPR, DISPR + MAP - 4), (DISPR + MAP - 4, DISPR)):
        rc, msg = call(lib, p, ws_bytes, dispR=a, outlR=b, **full)
        assert rc == EINVAL and msg == "mc_predict_views: outlierR_out overlaps dispR_out"
    # with left_only and no LR check too: the maps are checked whatever the parameter set computes
    p = mc.make_params(dict(mc.PRESETS["mb_slow"], left_only=1))
    wb = lib.mc_predict_workspace_bytes(C.byref(p), 16, D, H, W)
    rc, msg = call(lib, p, wb, **{view: DISP})
    assert rc == EINVAL and msg == "mc_predict_views: %s overlaps disp_out" % ARG[view]


def test_workspace_sizes_do_not_depend_on_the_right_view(mc):
    """the maps are the caller's and the tail runs in images the left view has finished with: the sizes are what tests/test_abi.py pins"""
    lib = mc._lib.lib
    p = mc.make_params("kitti_fast")
    assert lib.mc_predict_workspace_bytes(C.byref(p), 0, 228, 370, 1226) == 2519785984


def test_stage_table():
    """right_view_cases.stages: which of (occlusion, mismatch, subpixel, median, bilateral) run (main.lua:1054-1079)"""
    base = dict(lr_check=1, sm_terminate=0, sm_skip=0)
    assert rv.stages(base) == (True, True, True, True, True)
    assert rv.stages(dict(base, lr_check=0)) == (False, False, True, True, True)
    assert rv.stages(dict(base, sm_skip="occlusion")) == (False, False, True, True, True)
    assert rv.stages(dict(base, sm_skip="subpixel_enchancement")) == (True, True, False, True, True)
    assert rv.stages(dict(base, sm_skip="median")) == (True, True, True, False, True)
    assert rv.stages(dict(base, sm_skip="bilateral")) == (True, True, True, True, False)
    assert rv.stages(dict(base, sm_terminate="sgm")) == (False,) * 5
    assert rv.stages(dict(base, sm_terminate="occlusion")) == (True, False, False, False, False)
    assert rv.stages(dict(base, sm_terminate="mismatch")) == (True, True, False, False, False)
    assert rv.stages(dict(base, sm_terminate="subpixel_enchancement")) == (True, True, True, False, False)
    assert rv.stages(dict(base, sm_terminate="median")) == (True, True, True, True, False)
    assert rv.stages(dict(base, lr_check=0, sm_terminate="occlusion")) == (False, False, True, True, True)


DROPS = [dict(sm_skip=s) for s in ("", "cbca", "sgm", "occlusion", "subpixel_enchancement", "median", "bilateral")] + \
        [dict(sm_terminate=t) for t in ("sgm", "cbca2", "occlusion", "mismatch", "subpixel_enchancement", "median", "bilateral")]


@pytest.mark.parametrize("route", ["fast", "mb"])
def test_stage_table_composes_the_oracles_own_left_map(mc, oracle, route):
    """the same composition without the mirror, on the left view's maps, is the oracle pipeline's own `disp`, whatever is dropped: the
    stage table of oracle_right is the oracle's"""
    for over in DROPS:
        o, prm = rv.oracle_maps(oracle, mc.PRESETS, route, 7, over=over)
        occlusion, mismatch, subpixel, median, bilateral = rv.stages(prm)
        outl = oracle.outlier_detection(o["dispL0"], o["dispR0"], 7)
        t = o["dispL0"]
        t = oracle.interpolate_occlusion(t, outl) if occlusion else t
        t = oracle.interpolate_mismatch(t, outl) if mismatch else t
        t = oracle.subpixel_enchancement(t, o["volL"]) if subpixel else t
        t = oracle.median2d(t, prm["median_k"]) if median else t
        t = oracle.mean2d(t, oracle.gaussian(prm["blur_sigma"]), prm["blur_t"]) if bilateral else t
        assert np.array_equal(t.view(np.uint32), o["disp"].view(np.uint32)), over


def test_seed_condition_holds_on_the_oracle(mc, oracle):
    for route, Dd, width in rv.CASES:
        o, prm = rv.oracle_maps(oracle, mc.PRESETS, route, Dd, width)
        dr, outl = rv.oracle_right(oracle, o, prm, Dd)
        assert dr.shape == outl.shape == (H, width)
        assert rv.has_all_classes(outl), (route, Dd, width)


def test_the_definition_on_a_pair_shifted_by_a_constant(mc, oracle):
    """A noise-free pair whose right view is the left one shifted by s, right[y, x] = left[y, x + s], through the oracle on the kitti_fast
    route.  A right pixel x shows what the left pixel x + s shows, so it is visible in both views for x <= W-1-s, and its disparity is s.

    The class map tells the two views apart: in the right view the pixels WITHOUT a partner are the s rightmost ones (in the left view
    the s leftmost), so outlier_right is 0 on x <= W-1-s and every row has non-matches among x >= W-s
    (not all of them: a pixel without a partner may take a disparity that passes the check by chance).  With the roles of the two arg-min maps swapped in the
    composition (d0 = M(dispL0)) the non-matches land on both edges and this fails.
    The disparity: up to and including the mismatch interpolation the map holds integers, and equals s exactly on every x <=
    W-1-s-border.  The three stages behind it do not keep integers -- the sub-pixel stage moves a disparity by the cost curve's
    asymmetry and the range-gated blur averages over the strip without a partner -- so the finished map is held to s there within
    the sub-pixel stage's own clamp, 1 (measured on this pair: at most 0.063 off)."""
    s, Cn = 3, 16
    rng = np.random.default_rng(5)
    x0 = rng.standard_normal((H, W)).astype(np.float32)
    x1 = rng.standard_normal((H, W)).astype(np.float32)
    x1[:, :W - s] = x0[:, s:]
    fl = rng.standard_normal((Cn, H, W)).astype(np.float32)
    fr = rng.standard_normal((Cn, H, W)).astype(np.float32)
    fr[..., :W - s] = fl[..., s:]
    f = np.stack([fl, fr])
    f = (f / np.sqrt((f * f).sum(1, keepdims=True))).astype(np.float32)
    prm = dict(mc.PRESETS["kitti_fast"])
    border = prm["border_n"]
    o = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
    dr, outl = rv.oracle_right(oracle, o, prm, D)
    assert (outl[:, :W - s] == 0).all() and (outl[:, W - s:] != 0).any(axis=1).all()
    integer = dict(prm, sm_terminate="mismatch")
    dr_int, outl_int = rv.oracle_right(oracle, oracle.stereo_predict(integer, x0, x1, D, featL=f[0], featR=f[1]), integer, D)
    assert np.array_equal(outl_int, outl)
    assert (dr_int[:, :W - s - border] == s).all()
    print("finished right map against s on x <= W-1-s-border: at most %.4f off" % np.abs(dr[:, :W - s - border] - s).max())
    assert (np.abs(dr[:, :W - s - border] - s) < 1).all()
    # the composition with the roles swapped is a different map: the check above is not vacuous
    swapped = rv.M(oracle.outlier_detection(rv.M(o["dispL0"]), rv.M(o["dispR0"]), D))
    assert (swapped[:, :s] != 0).any()
