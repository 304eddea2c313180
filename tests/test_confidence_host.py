"""CPU: mc_cost_margins and mc-cnn_amd/confidence.py as far as they can be held without a GPU -- the symbol and its declarations, the Lua
prototype and keys, mc_cost_margins' refusals (all of which precede the launch: fake non-null device pointers, nothing is dereferenced,
and every call here is one that must be refused), the torch statement of the margins (predict.cost_margins, on CPU tensors) and the
measures against explicit numpy, sparsification / keep_mask against np.argsort(kind="stable") (integer counts, equal), and the flag
refusals of main.py and predict_kitti.py.  The numpy side is tests/confidence_cases.py."""
import os
import re

import numpy as np
import pytest

import confidence_cases as cc

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22
D, H, W = 9, 4, 6
MAP = 4 * H * W
VOL, D1, C1, C2, C2L = (0x10000000 + k * 0x1000000 for k in range(5))   # fake device addresses, far apart


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def prototype(text, name):
    m = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S)
    assert m, "no prototype of %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mc_adcensus.h")).read(), flags=re.S)


def test_symbol_is_exported_declared_and_bound(mc):
    import libraries as L
    assert "mc_cost_margins" in mc._lib.SYMBOLS
    assert "mc_cost_margins" in L.exported_abi(mc._lib.LIB_PATH)
    assert "mc_cost_margins" in L.header_symbols(header())
    assert L.exported_abi(mc._lib.LIB_PATH) - L.TEST_HOOKS["libmcadcensus.so"] == L.header_symbols(header()) == set(mc._lib.SYMBOLS)
    args = prototype(header(), "mc_cost_margins")
    assert args == ["const float *vol", "int D", "int H", "int W", "float *d1_out", "float *c1_out", "float *c2_out", "float *c2l_out",
                    "void *stream"]
    assert len(args) == len(mc._lib.lib.mc_cost_margins.argtypes)
    # header, loader and library agree on the version they speak
    define = int(re.search(r"#define MC_ABI_VERSION (\d+)", header()).group(1))
    assert mc._lib.lib.mc_version() == mc._lib.ABI_VERSION == define


def test_lua_shim_carries_the_prototype_the_function_and_the_keys():
    lua = open(os.path.join(ROOT, "mc-cnn_amd", "lua", "adcensus.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    assert prototype(cdef, "mc_cost_margins") == prototype(header(), "mc_cost_margins")
    assert re.search(r"function adcensus\.cost_margins\(vol, d1, c1, c2, c2l\)", lua) and "lib.mc_cost_margins(" in lua
    assert int(re.search(r"local MC_ABI_VERSION = (\d+)", lua).group(1)) == int(re.search(r"#define MC_ABI_VERSION (\d+)", header()).group(1))
    predict = lua[lua.index("function adcensus.predict("):]
    for key in ("c1", "c2", "c2l"):
        assert "extras.%s" % key in predict and "k ~= '%s'" % key in predict


def call(mc, vol=VOL, d=D, h=H, w=W, d1=D1, c1=C1, c2=C2, c2l=C2L):
    lib = mc._lib.lib
    return lib.mc_cost_margins(vol, d, h, w, d1, c1, c2, c2l, None), lib.mc_last_error().decode()


REFUSED = [
    ("D < 1", dict(d=0), "bad dims"), ("H < 1", dict(h=0), "bad dims"), ("W < 1", dict(w=-3), "bad dims"),
    ("all outputs null", dict(d1=None, c1=None, c2=None, c2l=None), "no output"),
    ("null volume", dict(vol=None), "null volume"),
    ("d1 inside the volume", dict(d1=VOL + 4 * MAP), "d1_out overlaps vol"),
    ("c1 on the volume's last float", dict(c1=VOL + D * MAP - 4), "c1_out overlaps vol"),
    ("c2 ends on the volume's first float", dict(c2=VOL - MAP + 4), "c2_out overlaps vol"),
    ("c2l on the volume", dict(c2l=VOL), "c2l_out overlaps vol"),
    ("c1 on d1", dict(c1=D1), "c1_out overlaps d1_out"),
    ("c2 on c1's last float", dict(c2=C1 + MAP - 4), "c2_out overlaps c1_out"),
    ("c2l ends on c2's first float", dict(c2l=C2 - MAP + 4), "c2l_out overlaps c2_out"),
    ("c2l on d1, the rest null", dict(c1=None, c2=None, c2l=D1), "c2l_out overlaps d1_out"),
]


@pytest.mark.parametrize("what,kw,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_a_bad_call_is_refused_in_front_of_the_launch(mc, what, kw, message):
    rc, msg = call(mc, **kw)
    assert rc == EINVAL and msg.startswith("mc_cost_margins: ") and message in msg, (what, rc, msg)


# ---- the torch statement of the margins, on CPU tensors ----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", cc.SHAPES, ids=["x".join(map(str, s)) for s in cc.SHAPES])
@pytest.mark.parametrize("seed", (0, 1))
def test_the_torch_margins_are_the_oracles(mc, shape, seed):
    from mc_cnn_amd.predict import cost_margins
    got = cost_margins(torch.from_numpy(cc.volume(*shape, seed).copy())[None])
    for name, g, w in zip(("d1", "c1", "c2", "c2l"), got, cc.wanted(*shape, seed)):
        assert g.shape == (1, 1) + shape[1:] and g.dtype == torch.float32
        assert np.array_equal(bits(g.numpy()[0, 0]), bits(w)), name


def test_the_planted_curves_say_what_the_definition_says():
    """the oracle itself, on curves whose answer is read off by eye"""
    rows = [   # curve -> (d1, c1, c2, c2l)
        ([1.0, 0.5, 0.5, 0.5, 1.0], (1, 0.5, 0.5, np.inf)),            # a plateau counts once, at its first d
        ([1.0, 0.5, 0.5, 0.25, 1.0], (3, 0.25, 0.5, 0.5)),             # the plateau's first d is a local minimum, the descent's end is d1
        ([0.0, -1.0, 0.5, -1.0, 0.75], (1, -1.0, -1.0, -1.0)),         # a tie at a later d: c2 == c1
        ([0.5, -1.0, -0.5, 0.0, 0.25], (1, -1.0, -0.5, np.inf)),       # the runner-up is no local minimum
        ([0.0, 1.0, 2.0], (0, 0.0, 1.0, np.inf)),                      # strictly monotone: c2 finite, c2l +INF
        ([np.nan, np.nan], (0, np.inf, np.inf, np.inf)),
        ([np.nan, 7.0, np.nan], (1, 7.0, np.inf, np.inf)),             # a single candidate
        ([np.inf, 3.0, np.inf, 4.0], (1, 3.0, 4.0, 4.0)),
        ([3.0, 1.0, 2.0, np.nan, 0.5, np.nan, 0.75], (4, 0.5, 0.75, 0.75)),   # NaN neighbours block nothing
    ]
    for curve, want in rows:
        got = cc.margins_oracle(np.array(curve, np.float32).reshape(-1, 1, 1))
        assert tuple(float(g[0, 0]) for g in got) == tuple(float(v) for v in want), curve


# ---- measures ----------------------------------------------------------------------------------------------------------------------

def hand_made():
    """maps of a 3 x 6 pair with D = 5 that hold x' < 0, x' >= W, a single-candidate pixel, a unimodal one, a pixel with nothing at all
    and a NaN curvature"""
    inf, nan = np.inf, np.nan
    res = dict(
        dispL0=[[0, 1, 2, 4, 1, 0], [3, 0, 0, 1, 4, 2], [1, 1, 1, 1, 1, 1]],
        dispR0=[[0, 1, 3, 0, 1, 2], [4, 0, 2, 1, 0, 3], [1, 1, 1, 1, 1, 1]],
        c1=[[-0.5, -1.0, 0.25, inf, -2.0, 0.0], [1.0, 1.5, -0.75, 0.5, 0.5, -3.0], [0.0] * 6],
        c2=[[inf, -0.5, 0.5, inf, -2.0, 1.0], [inf, 2.0, -0.5, 0.75, 4.0, -1.0], [1.0] * 6],
        c2l=[[inf, inf, 0.75, inf, -1.0, inf], [inf, 2.5, inf, 0.75, inf, 2.0], [inf] * 6],
        curvature=[[0.0, 0.5, nan, 0.0, 2.0, 0.0], [1.0, 0.0, 0.25, nan, 0.0, 3.0], [0.5] * 6],
        outlier=[[0, 1, 2, 0, 0, 1], [2, 0, 0, 0, 1, 0], [0] * 6],
    )
    res = {k: np.array(v, np.float32) for k, v in res.items()}
    for k in ("c1", "c2", "c2l", "outlier"):
        res[k + "_right"] = np.ascontiguousarray(res[k][:, ::-1] * np.float32(1 if k == "outlier" else 0.5))
    return res


def measures_oracle(res, D, view):
    """the table of confidence.measures' docstring, pixel by pixel"""
    s = "" if view == "left" else "_right"
    Hh, Ww = res["dispL0"].shape
    out = {k: np.zeros((Hh, Ww), np.float32) for k in ("msm", "mmn", "mlm", "cls", "lrc")}
    for y in range(Hh):
        for x in range(Ww):
            c1, c2, c2l = (res[k + s][y, x] for k in ("c1", "c2", "c2l"))
            out["msm"][y, x] = -c1
            out["mmn"][y, x] = 0 if c2 == np.inf else c2 - c1
            out["mlm"][y, x] = 0 if c2 == np.inf else c2l - c1
            out["cls"][y, x] = 1 if res["outlier" + s][y, x] == 0 else 0
            d = res["dispL0" if view == "left" else "dispR0"][y, x]
            xp = x - int(d) if view == "left" else x + int(d)
            if xp < 0 or xp >= Ww:
                out["lrc"][y, x] = -float(D)
            else:
                out["lrc"][y, x] = -abs(d - res["dispR0" if view == "left" else "dispL0"][y, xp])
    if view == "left":
        out["cur"] = res["curvature"].copy()
    for v in out.values():
        v[np.isnan(v)] = -np.inf
    return out


@pytest.mark.parametrize("view", ("left", "right"))
def test_measures_are_the_tables(mc, view):
    from mc_cnn_amd import confidence
    res = hand_made()
    want = measures_oracle(res, 5, view)
    # the cases the maps are made for are there
    x = np.arange(6)[None]
    assert ((x - res["dispL0"]) < 0).any() and ((x + res["dispR0"]) >= 6).any()
    assert (res["c2"] == np.inf).any() and ((res["c2"] < np.inf) & (res["c2l"] == np.inf)).any() and (res["c1"] == np.inf).any()
    got = confidence.measures({k: torch.from_numpy(v)[None, None] for k, v in res.items()}, 5, view=view)
    assert tuple(got) == tuple(k for k in confidence.NAMES if k in want)
    assert ("cur" in got) == (view == "left")
    for k in got:
        assert got[k].shape == (3, 6) and got[k].dtype == torch.float32
        assert np.array_equal(bits(got[k].numpy()), bits(want[k])), (view, k, got[k], want[k])
    if view == "left":
        assert got["mmn"][0, 0] == 0 and got["mlm"][0, 0] == 0            # one candidate
        assert got["mlm"][0, 1] == np.inf and got["mmn"][0, 1] == 0.5     # a unimodal curve
        assert got["msm"][0, 3] == -np.inf and got["mmn"][0, 3] == 0      # nothing below +INF
        assert got["cur"][0, 2] == -np.inf                                # a NaN measure
        assert got["lrc"][0, 3] == -5.0 and got["lrc"][0, 1] == -1.0 and got["lrc"][1, 1] == 0.0 and got["lrc"][0, 2] == -2.0


def test_a_measure_whose_inputs_are_missing_is_left_out(mc):
    from mc_cnn_amd import confidence
    res = {k: torch.from_numpy(v) for k, v in hand_made().items()}
    assert tuple(confidence.measures(res, 5)) == confidence.NAMES
    for gone, lost in (("curvature", {"cur"}), ("c2l", {"msm", "mmn", "mlm"}), ("outlier", {"cls"}), ("dispR0", {"lrc"})):
        less = {k: v for k, v in res.items() if k != gone}
        assert set(confidence.NAMES) - set(confidence.measures(less, 5)) == lost, gone
    assert "cur" not in confidence.measures(res, 5, view="right")
    with pytest.raises(ValueError):
        confidence.measures(res, 5, view="up")
    from mc_cnn_amd import predict_kitti
    assert predict_kitti.MEASURES == confidence.NAMES


# ---- sparsification, area, keep_mask -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.RANKING_CASES)
def test_sparsification_counts_are_the_stable_argsorts(mc, name):
    from mc_cnn_amd import confidence
    conf, pred, actual, err_at, n = cc.ranking_case(name)
    want = cc.sparsification_oracle(conf, pred, actual, err_at, n)
    got = confidence.sparsification(*(torch.from_numpy(a.copy()) for a in (conf, pred, actual)), err_at, n=n)
    for g, w, what in zip(got, want, ("bad", "bad_oracle", "m")):
        assert g.dtype == torch.int64 and np.array_equal(g.numpy(), w), (name, what)
    bad, bad_oracle, m = got
    N = int((actual != 0).sum())
    assert m[-1] == N and bad[-1] == bad_oracle[-1] and (m >= 1).all()       # the whole set: the same pixels in any order
    assert (bad_oracle <= bad).all()                                          # no ranking has fewer bad pixels in its first m
    assert confidence.area(bad_oracle, m) <= confidence.area(bad, m)
    # (counts are what is compared exactly; the area is a float64 mean of n rates in [0, 1], whose order of summation is free: n * 2^-53)
    assert abs(confidence.area(bad, m) - float(np.mean(want[0].astype(np.float64) / want[2].astype(np.float64)))) <= n * 2.0 ** -53
    # ... nor has any other measure: the error itself, negated, reaches the floor; its opposite is the worst
    err = np.abs(actual - pred)
    best = confidence.sparsification(torch.from_numpy(-err), torch.from_numpy(pred.copy()), torch.from_numpy(actual.copy()), err_at, n=n)
    assert np.array_equal(best[0].numpy(), want[1])
    worst = confidence.sparsification(torch.from_numpy(err), torch.from_numpy(pred.copy()), torch.from_numpy(actual.copy()), err_at, n=n)
    assert confidence.area(worst[0], m) >= confidence.area(bad, m)


def test_sparsification_refuses_an_image_without_ground_truth(mc):
    from mc_cnn_amd import confidence
    z = torch.zeros(3, 4)
    with pytest.raises(ValueError):
        confidence.sparsification(z, z, z, 3.0)
    with pytest.raises(ValueError):
        confidence.sparsification(z, z, z + 1, 3.0, n=0)


@pytest.mark.parametrize("name", cc.RANKING_CASES)
def test_keep_mask_keeps_the_first_of_the_stable_order(mc, name):
    from mc_cnn_amd import confidence
    conf = cc.ranking_case(name)[0]
    for fraction in (1.0, 0.5, 1.0 / 3.0, 0.999, 1e-9, 1.0 / conf.size):
        got = confidence.keep_mask(torch.from_numpy(conf.copy()), fraction)
        assert got.dtype == torch.bool and got.shape == conf.shape
        assert int(got.sum()) == int(np.ceil(fraction * conf.size))
        assert np.array_equal(got.numpy(), cc.keep_mask_oracle(conf, fraction)), (name, fraction)
    for fraction in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError):
            confidence.keep_mask(torch.from_numpy(conf.copy()), fraction)


# ---- command lines -----------------------------------------------------------------------------------------------------------------

def test_main_takes_margins_with_predict_only():
    from mc_cnn_amd import main as mcmain
    for dataset in ("kitti", "kitti2015", "mb"):
        for arch in ("fast", "slow", "ad", "census"):
            assert mcmain.parse([dataset, arch, "-a", "predict", "-margins"])[2].margins is True
            assert mcmain.parse([dataset, arch, "-margins", "-right_view", "-extras"])[2].margins is True     # -a predict is the default
            assert mcmain.parse([dataset, arch, "-a", "predict"])[2].margins is False
    for action in ("time", "test_te"):
        with pytest.raises(SystemExit) as e:
            mcmain.parse(["kitti", "fast", "-a", action, "-margins"])
        assert "-margins" in str(e.value) and "-a predict" in str(e.value)


def test_predict_kitti_takes_the_new_flags():
    from mc_cnn_amd import predict_kitti as pk
    opt = pk.parse(["test"])
    assert (opt.roc, opt.sparse_by, opt.keep, opt.sparse, opt.sm_skip) == (False, None, None, False, "")
    assert pk.parse(["test", "-roc"]).roc is True
    for action in ("test", "submit"):
        for name in pk.MEASURES:
            opt = pk.parse([action, "-sparse_by", name, "-keep", "0.25"])
            assert (opt.sparse_by, opt.keep) == (name, 0.25)
        assert pk.parse([action, "-sparse_by", "mmn", "-keep", "1"]).keep == 1.0
    assert pk.parse(["test", "-sparse_by", "mlm", "-keep", "0.5", "-sm_skip", "subpixel_enchancement"]).sparse_by == "mlm"
    assert pk.available_measures("") == pk.MEASURES and "cur" not in pk.available_measures("subpixel_enchancement")


REFUSED_FLAGS = [
    ("an unknown name", ["test", "-sparse_by", "entropy", "-keep", "0.5"], ("entropy", "msm | mmn | mlm | cur | cls | lrc")),
    ("F = 0", ["test", "-sparse_by", "mmn", "-keep", "0"], ("-keep", "(0, 1]")),
    ("F > 1", ["submit", "-sparse_by", "mmn", "-keep", "1.5"], ("-keep", "(0, 1]")),
    ("F < 0", ["test", "-sparse_by", "mmn", "-keep", "-0.5"], ("-keep", "(0, 1]")),
    ("F not a number", ["test", "-sparse_by", "mmn", "-keep", "nan"], ("-keep", "(0, 1]")),
    ("-sparse_by alone", ["test", "-sparse_by", "mmn"], ("-sparse_by NAME", "-keep F", "go together")),
    ("-keep alone", ["submit", "-keep", "0.5"], ("-sparse_by NAME", "-keep F", "go together")),
    ("with -sparse", ["test", "-sparse", "-sparse_by", "cls", "-keep", "0.5"], ("-sparse",)),
    ("-sparse_by alone with -sparse", ["test", "-sparse", "-sparse_by", "cls"], ("-sparse_by", "-keep")),
    ("-keep alone with -sparse", ["submit", "-sparse", "-keep", "0.5"], ("-sparse_by", "-keep")),
    ("cur without the sub-pixel stage", ["test", "-sparse_by", "cur", "-keep", "0.5", "-sm_skip", "subpixel_enchancement"],
     ("cur", "subpixel_enchancement", "msm | mmn | mlm | cls | lrc")),
    ("-roc on submit", ["submit", "-roc"], ("-roc", "test")),
    ("-roc with -sparse", ["test", "-roc", "-sparse"], ("-roc", "-sparse")),
]


@pytest.mark.parametrize("what,argv,said", REFUSED_FLAGS, ids=[r[0] for r in REFUSED_FLAGS])
def test_predict_kitti_refuses_with_what_is_supported(what, argv, said):
    from mc_cnn_amd import predict_kitti as pk
    with pytest.raises(SystemExit) as e:
        pk.parse(argv)
    msg = str(e.value)
    assert msg.startswith("predict_kitti: ") and all(s in msg for s in said), (what, msg)


def test_run_scores_and_writes_by_the_dial(tmp_path):
    """predict_kitti.run with a stand-in for the GPU: -sparse_by keeps keep_mask(measure, F) per image, -roc reports the areas"""
    from mc_cnn_amd import confidence, predict_kitti as pk
    from mc_cnn_amd.binio import read_png16, write_png16
    conf, pred, actual, err_at, n = cc.ranking_case("ties")
    root = tmp_path / "kitti"
    (root / "training" / "disp_noc").mkdir(parents=True)
    (root / "testing").mkdir()
    gt = np.round(actual * 256) / 256
    write_png16(gt.astype(np.float32), str(root / "training" / "disp_noc" / "000000_10.png"))
    gt = read_png16(str(root / "training" / "disp_noc" / "000000_10.png"))
    maps = {"mmn": conf, "cls": (conf > 1).astype(np.float32)}
    lines = []
    sums = pk.run("test", str(root), lambda a, b: (pred.copy(), {k: v.copy() for k, v in maps.items()}), n_pairs=1, log=lambda *a: lines.append(a), sparse_by="mmn", keep=0.4)
    kept = cc.keep_mask_oracle(conf, 0.4)
    assert lines == [(0,) + pk.kept_error(pred, gt, kept)] and sums == (lines[0][1], 1, lines[0][2])
    assert 0 < lines[0][2] < 1
    out = tmp_path / "out"
    pk.run("submit", str(root), lambda a, b: (pred.copy(), {k: v.copy() for k, v in maps.items()}), n_pairs=1, log=lambda *a: None, out_dir=str(out), sparse_by="mmn", keep=0.4)
    written = read_png16(str(out / "000000_10.png"))
    assert np.array_equal(written == 0, ~kept) and np.abs(written - pred)[kept].max() <= 1 / 256
    lines = []
    sums = pk.run("test", str(root), lambda a, b: (pred.copy(), {k: v.copy() for k, v in maps.items()}), n_pairs=1, log=lambda *a: lines.append(a), roc=("mmn", "cls"))
    want = {k: cc.sparsification_oracle(v, pred, gt, pk.ERR_AT) for k, v in maps.items()}
    areas = [float(np.mean(want[k][0] / want[k][2])) for k in ("mmn", "cls")] + [float(np.mean(want["mmn"][1] / want["mmn"][2]))]
    assert len(lines) == 1 and lines[0][:2] == (0, pk.three_pixel_error(pred, gt)) and sums == (lines[0][1], 1) + lines[0][2:]
    assert len(lines[0]) == 5 and all(abs(g - w) <= 100 * 2.0 ** -53 for g, w in zip(lines[0][2:], areas))   # (float64 means of 100 rates)
    assert areas[2] <= min(areas[:2])
