"""CPU: the host side of `-conv_mode bf16x3` (include/mc_conv_split.h): libmcconvsplit.so's symbols, workspace formula and refusals, its
place in the Makefile and the kernel inventory, the flag on the parsers, hs.py and predict_kitti.py, the default path's independence of
the new library, and the arithmetic's restatement (tests/conv_split_oracle.py) against a float64 convolution and against rational
arithmetic."""
import os
import re
import subprocess
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_split_oracle as co  # noqa: E402
import libraries as L  # noqa: E402
from mc_cnn_amd import _conv_split_lib as csl  # noqa: E402
from mc_cnn_amd import hs, predict_kitti, train, train_mb, train_mb_slow, train_slow  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402

HEADER = os.path.join(ROOT, "include", "mc_conv_split.h")


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_loads_without_a_gpu_and_exports_exactly_the_headers_symbols():
    """what only libmcconvsplit.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    text = open(HEADER).read()
    assert csl.load().mc_conv_split_version() == csl.ABI_VERSION == 1
    assert L.exported_abi(csl.LIB_PATH) == {"mc_conv_split_version", "mc_conv_split_last_error", "mc_conv_split_workspace_bytes", "mc_conv_split"}
    assert re.search(r"#define MC_CONV_SPLIT_CIN_STEP %d\b" % csl.CIN_STEP, text) and re.search(r"#define MC_CONV_SPLIT_MAX_COUT %d\b" % csl.MAX_COUT, text)
    assert (csl.CIN_STEP, csl.MAX_COUT, csl.EINVAL) == (16, 128, -22) and os.path.basename(csl.LIB_PATH) == "libmcconvsplit.so"
    assert "Inputs are finite" in text and "round to nearest even" in text


def test_workspace_formula_is_monotone_and_256_aligned():
    lib = csl.load()
    # a hi and a lo bf16 plane of the bank, padded to whole groups of 64 (or, up to 32, of 32) output channels
    assert lib.mc_conv_split_workspace_bytes(64, 64) == 2 * 2 * 9 * 64 * 64 == 147456
    assert lib.mc_conv_split_workspace_bytes(112, 112) == 2 * 2 * 9 * 112 * 128
    assert lib.mc_conv_split_workspace_bytes(16, 7) == 2 * 2 * 9 * 16 * 32
    for Cin in (16, 32, 64, 112, 160):
        last = 0
        for Cout in range(1, 129):
            b = lib.mc_conv_split_workspace_bytes(Cin, Cout)
            assert b > 0 and b % 256 == 0 and b >= last and lib.mc_conv_split_workspace_bytes(Cin + 16, Cout) > b
            last = b
    for Cin, Cout in ((0, 64), (1, 64), (3, 64), (8, 64), (40, 64), (-16, 64), (64, 0), (64, 129), (64, -1)):
        assert lib.mc_conv_split_workspace_bytes(Cin, Cout) == 0 and not csl.eligible(Cin, Cout)
    for Cin, Cout in ((16, 1), (64, 64), (80, 96), (96, 128), (112, 112)):
        assert csl.eligible(Cin, Cout)


def test_every_refusal_returns_einval_with_its_message_before_any_launch():
    lib = csl.load()
    P = 1 << 20                      # never dereferenced: every check precedes the first launch

    def call(x=P, w=2 * P, b=3 * P, out=4 * P, N=1, Cin=64, Cout=64, H=5, W=9, ws=5 * P, ws_bytes=None):
        need = lib.mc_conv_split_workspace_bytes(64, 64) if ws_bytes is None else ws_bytes
        return lib.mc_conv_split(x, w, b, out, N, Cin, Cout, H, W, 1, ws, need, None)

    need = lib.mc_conv_split_workspace_bytes(64, 64)
    bad = [("null in", lambda: call(x=None), "null pointer"), ("null weight", lambda: call(w=None), "null pointer"),
           ("null bias", lambda: call(b=None), "null pointer"), ("null out", lambda: call(out=None), "null pointer"),
           ("null workspace", lambda: call(ws=None), "null pointer"),
           ("out = in", lambda: call(out=P), "aliased"), ("out = weight", lambda: call(out=2 * P), "aliased"),
           ("out = bias", lambda: call(out=3 * P), "aliased"), ("workspace = in", lambda: call(ws=P), "aliased"),
           ("workspace = out", lambda: call(ws=4 * P), "aliased"), ("workspace = weight", lambda: call(ws=2 * P), "aliased"),
           ("N 0", lambda: call(N=0), "bad dims"), ("H 0", lambda: call(H=0), "bad dims"), ("W -1", lambda: call(W=-1), "bad dims"),
           ("Cin 1", lambda: call(Cin=1), "a 1 -> 64 layer is not eligible"), ("Cin 3", lambda: call(Cin=3), "a 3 -> 64 layer is not eligible"),
           ("Cin 8", lambda: call(Cin=8), "a 8 -> 64 layer is not eligible"), ("Cin 40", lambda: call(Cin=40), "a 40 -> 64 layer is not eligible"),
           ("Cout 0", lambda: call(Cout=0), "a 64 -> 0 layer is not eligible"), ("Cout 129", lambda: call(Cout=129), "a 64 -> 129 layer is not eligible"),
           ("planes past 32-bit offsets", lambda: call(H=1 << 13, W=1 << 11), "size bounds"),
           ("units past 2^31", lambda: call(N=1 << 20, H=1 << 7, W=1 << 10), "size bounds"),
           ("workspace one byte short", lambda: call(ws_bytes=need - 1), "workspace %d < %d" % (need - 1, need)),
           ("the workspace of a narrower layer", lambda: call(ws_bytes=lib.mc_conv_split_workspace_bytes(48, 64)), "workspace"),
           ("workspace off alignment", lambda: call(ws=5 * P + 8), "16-byte aligned")]
    for what, f, word in bad:
        rc = f()
        assert rc == csl.EINVAL, (what, rc)
        msg = csl.last_error()
        assert msg.startswith("mc_conv_split:") and word in msg, (what, msg)
    for what in ("Cin 8", "Cin 40"):       # the refusal names the rule
        dict((w, f) for w, f, _ in bad)[what]()
        assert "Cin % 16 == 0" in csl.last_error() and "Cout <= 128" in csl.last_error() and "mc_conv3x3" in csl.last_error()
    with pytest.raises(csl.ConvSplitError, match="not eligible"):
        csl.check(call(Cin=40), "mc_conv_split")


def test_the_library_is_built_from_its_own_unit_and_holds_its_own_kernels():
    assert L.print_libraries()["libmcconvsplit.so"] == ["conv_split.o", "error.o"]
    out = L.make("-n", "-B", "../libmcconvsplit.so")
    assert "conv_split.hip" in out and "error.hip" in out and "-o ../libmcconvsplit.so" in out and "conv3x3.hip" not in out
    assert "conv_split" not in L.make("-n", "-B", "../libmcadcensus.so")             # libmcadcensus.so keeps its kernel set
    assert L.built_kernels(csl.LIB_PATH) == {"conv_split_prep_kernel", "conv_split_kernel<1>", "conv_split_kernel<2>"}


# ---- the flag ------------------------------------------------------------------------------------------------------------------
HS = hs.METHODS[0]
NET_LINES = [(mcmain.parse, ["kitti", "fast", "-a", "predict"]), (mcmain.parse, ["kitti2015", "fast", "-a", "time"]),
             (mcmain.parse, ["kitti", "fast", "-a", "test_te"]), (mcmain.parse, ["kitti", "fast", "-a", "test_all"]),
             (mcmain.parse, ["kitti", "fast", "-a", "train_tr"]), (mcmain.parse, ["kitti", "slow", "-a", "predict"]),
             (mcmain.parse, ["mb", "slow", "-a", "time"]), (mcmain.parse, ["mb", "fast", "-a", "predict"]),
             (train_slow.parse, ["kitti", "slow", "-a", "test_te"]), (train_slow.parse, ["kitti2015", "slow", "-a", "train_tr"]),
             (train_slow.parse, ["kitti", "slow", "-a", "test_all"]), (train_mb.parse, ["mb", "fast", "-a", "test_te"]),
             (train_mb.parse, ["mb", "fast", "-a", "train_tr"]), (train_mb_slow.parse, ["mb", "slow", "-a", "test_te"]),
             (train_mb_slow.parse, ["mb", "slow", "-a", "train_tr"])]


def opt_of(parsed):
    return parsed[2] if isinstance(parsed, tuple) else parsed


@pytest.mark.parametrize("parse, argv", NET_LINES + [
    (hs.parse, [HS, "kitti", "fast", "test_te", "net.t7"]), (hs.parse, [HS, "mb", "slow", "test_te", "net.t7"]),
    (predict_kitti.parse, ["test"]), (predict_kitti.parse, ["submit", "-n", "3"])])
def test_the_flag_is_taken_wherever_a_net_predicts_and_leaves_the_namespace_alone_without_it(parse, argv):
    plain, fp32, split = opt_of(parse(argv)), opt_of(parse(argv + ["-conv_mode", "fp32"])), opt_of(parse(argv + ["-conv_mode", "bf16x3"]))
    assert not hasattr(plain, "conv_mode") and vars(plain) == vars(fp32)           # what the command line parsed to before the flag existed
    assert split.conv_mode == "bf16x3" and {k: v for k, v in vars(split).items() if k != "conv_mode"} == vars(plain)
    assert getattr(plain, "conv_mode", "fp32") == "fp32"
    with pytest.raises(SystemExit):
        parse(argv + ["-conv_mode", "bf16"])            # the one-pass mode is not offered
    with pytest.raises(SystemExit):
        parse(argv + ["-conv_mode", "bf16x4"])


def test_the_flag_and_fc_mode_are_independent_on_arch_slow_and_main_routes_them():
    for parse, argv in ((mcmain.parse, ["kitti", "slow", "-a", "predict"]), (train_slow.parse, ["kitti", "slow", "-a", "test_te"]),
                        (train_mb_slow.parse, ["mb", "slow", "-a", "test_te"])):
        for conv in ("fp32", "bf16x3"):
            for fc in ("fp32", "bf16x3"):
                opt = parse(argv + ["-conv_mode", conv, "-fc_mode", fc])[2]
                assert getattr(opt, "conv_mode", "fp32") == conv and opt.fc_mode == fc
    assert mcmain.route(["kitti", "slow", "-a", "train_tr", "-conv_mode", "bf16x3"])[4].conv_mode == "bf16x3"
    assert mcmain.route(["mb", "fast", "-a", "test_te", "-conv_mode", "bf16x3"])[4].conv_mode == "bf16x3"
    assert mcmain.route(["kitti", "fast", "-a", "train_tr", "-l1", "2", "-conv_mode", "bf16x3"])[4].conv_mode == "bf16x3"
    assert not hasattr(mcmain.route(["mb", "slow", "-a", "test_te"])[4], "conv_mode")
    o = hs.parse([HS, "kitti", "slow", "test_te", "net.t7", "-conv_mode", "bf16x3", "-fc_mode", "bf16x3"])
    assert (o.conv_mode, o.fc_mode) == ("bf16x3", "bf16x3")


@pytest.mark.parametrize("parse, argv, who", [
    (mcmain.parse, ["kitti", "ad", "-a", "predict"], "main.py"), (mcmain.parse, ["mb", "census", "-a", "time"], "main.py"),
    (mcmain.parse, ["kitti2015", "census", "-a", "predict"], "main.py"),
    (hs.parse, [HS, "kitti", "ad", "test_te", "net.t7"], "hs"), (hs.parse, [HS, "kitti", "census", "test_te", "net.t7"], "hs")])
def test_bf16x3_is_refused_where_there_is_no_net(parse, argv, who):
    arch = argv[1] if parse is mcmain.parse else argv[2]
    with pytest.raises(SystemExit) as e:
        parse(argv + ["-conv_mode", "bf16x3"])
    for word in (who + ": -conv_mode bf16x3", "arch " + arch, "no net", "arch fast and arch slow"):
        assert word in str(e.value), (word, str(e.value))
    plain, given = opt_of(parse(argv)), opt_of(parse(argv + ["-conv_mode", "fp32"]))
    assert vars(plain) == vars(given) and not hasattr(plain, "conv_mode")          # -conv_mode fp32 there changes nothing


def test_evalset_and_the_pair_pipeline_take_the_mode():
    src = open(os.path.join(ROOT, "mc-cnn_amd", "evalset.py")).read()
    assert 'getattr(opt, "conv_mode", "fp32")' in src and "features_fast(xb, self.layers, self.conv_mode)" in src
    assert "features_slow(xb, self.layers, self.conv_mode)" in src
    src = open(os.path.join(ROOT, "mc-cnn_amd", "predict_kitti.py")).read()
    assert "features_fast(xb, self.layers, self.conv_mode)" in src and 'conv_mode=getattr(opt, "conv_mode", "fp32")' in src
    import inspect
    assert inspect.signature(mcmain.features_fast).parameters["conv_mode"].default == "fp32"
    assert inspect.signature(mcmain.features_slow).parameters["conv_mode"].default == "fp32"
    from mc_cnn_amd import adcensus
    assert inspect.signature(adcensus.conv3x3).parameters["mode"].default == "fp32"
    assert list(inspect.signature(adcensus.conv3x3).parameters) == ["x", "weight", "bias", "relu", "out", "mode"]


def test_a_saved_net_does_not_record_the_flag(tmp_path):
    _, _, opt, _ = train_slow.parse(["kitti", "slow", "-a", "train_tr", "-conv_mode", "bf16x3"])
    _, _, opt0, _ = train_slow.parse(["kitti", "slow", "-a", "train_tr"])
    conv, fc = train_slow.init_net(3)
    a = train_slow.save_net(str(tmp_path / "a.t7"), conv, fc, opt)
    b = train_slow.save_net(str(tmp_path / "b.t7"), conv, fc, opt0)
    assert open(a, "rb").read() == open(b, "rb").read()
    _, _, opt, _ = mcmain.parse(["kitti", "fast", "-a", "train_tr", "-conv_mode", "bf16x3"])
    _, _, opt0, _ = mcmain.parse(["kitti", "fast", "-a", "train_tr"])
    layers = mcmain.load_net("random:3", "kitti", "fast")
    a = train.save_net(str(tmp_path / "c.t7"), layers, opt)
    b = train.save_net(str(tmp_path / "d.t7"), layers, opt0)
    assert open(a, "rb").read() == open(b, "rb").read() and b"conv_mode" not in open(a, "rb").read()


# ---- the default path never touches the new library ---------------------------------------------------------------------------------
def test_without_the_flag_the_library_is_never_loaded():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from mc_cnn_amd import main, hs, predict_kitti, train_slow, train_mb, train_mb_slow, adcensus, evalset\n"
            "main.parse(['kitti', 'fast', '-a', 'predict']); main.parse(['kitti', 'slow', '-a', 'time', '-conv_mode', 'fp32'])\n"
            "train_slow.parse(['kitti', 'slow', '-a', 'test_te']); predict_kitti.parse(['test'])\n"
            "assert not any('conv_split' in m for m in sys.modules), [m for m in sys.modules if 'conv_split' in m]\n"
            "assert 'libmcconvsplit' not in open('/proc/self/maps').read()\n"
            "assert 'libmcadcensus' in open('/proc/self/maps').read()\n"
            "main.parse(['kitti', 'fast', '-a', 'predict', '-conv_mode', 'bf16x3'])\n"
            "assert 'libmcconvsplit' not in open('/proc/self/maps').read()\n"     # parsing alone does not load it either
            "print('ok')\n" % ROOT)
    out = subprocess.check_output([sys.executable, "-c", code]).decode()
    assert out.strip().endswith("ok")


class FakeTensor:
    """What adcensus.conv3x3 asks of a CUDA tensor, on the host."""
    is_cuda, device = True, types.SimpleNamespace(index=0)

    def __init__(self, shape, ptr):
        import torch
        self.shape, self.ptr, self.dtype = tuple(shape), ptr, torch.float32

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.ptr


@pytest.mark.parametrize("mode, Cin, Cout, which", [("fp32", 64, 64, "fp32"), (None, 64, 64, "fp32"), ("bf16x3", 64, 64, "split"),
                                                    ("bf16x3", 112, 112, "split"), ("bf16x3", 1, 64, "fp32"), ("bf16x3", 3, 7, "fp32"),
                                                    ("bf16x3", 40, 64, "fp32"), ("bf16x3", 64, 129, "fp32")])
def test_conv3x3_calls_the_library_of_its_mode_and_layer_only(mode, Cin, Cout, which, monkeypatch):
    import torch
    from mc_cnn_amd import adcensus
    calls, loads = [], []

    def stub(name, ret):
        def f(*a):
            calls.append((name, a))
            return ret
        return f
    monkeypatch.setattr(adcensus, "torch", types.SimpleNamespace(
        Tensor=FakeTensor, float32=torch.float32, uint8=torch.uint8, empty=lambda n, **k: FakeTensor((n,), 0x9000000),
        cuda=types.SimpleNamespace(current_stream=lambda: types.SimpleNamespace(cuda_stream=0))))
    monkeypatch.setattr(adcensus, "_scratch", {})
    monkeypatch.setattr(adcensus, "lib", types.SimpleNamespace(mc_conv3x3_workspace_bytes=stub("mc_conv3x3_workspace_bytes", 1024),
                                                              mc_conv3x3=stub("mc_conv3x3", 0)))
    split = types.SimpleNamespace(mc_conv_split_workspace_bytes=stub("mc_conv_split_workspace_bytes", 2048), mc_conv_split=stub("mc_conv_split", 0))
    monkeypatch.setattr(csl, "load", lambda: loads.append(1) or split)
    x, w, b, out = FakeTensor((2, Cin, 5, 9), 0x1000000), FakeTensor((Cout, Cin, 3, 3), 0x2000000), FakeTensor((Cout,), 0x3000000), FakeTensor((2, Cout, 5, 9), 0x4000000)
    kw = {} if mode is None else {"mode": mode}
    assert adcensus.conv3x3(x, w, b, True, out=out, **kw) is out
    names = [n for n, _ in calls]
    if which == "fp32":
        assert names == ["mc_conv3x3_workspace_bytes", "mc_conv3x3"] and not loads
    else:
        assert names == ["mc_conv_split_workspace_bytes", "mc_conv_split"] and loads
    args = calls[1][1]               # mc_conv3x3's argument list, whichever library takes it
    assert args[:4] == (0x1000000, 0x2000000, 0x3000000, 0x4000000) and args[4:10] == (2, Cin, Cout, 5, 9, 1)
    assert args[10] == 0x9000000 and args[11] == (1024 if which == "fp32" else 2048)
    with pytest.raises(ValueError, match="fp32 | bf16x3"):
        adcensus.conv3x3(x, w, b, True, out=out, mode="bf16")


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def test_split_is_round_to_nearest_even_and_exact_in_two_parts():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 6, 4000).astype(np.float32),
                        np.array([0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-30], np.float32)])
    hi, lo = co.split(v)
    np.testing.assert_array_equal(hi, torch.from_numpy(v).to(torch.bfloat16).float().numpy())       # ties to even: 1.00390625 -> 1.0
    np.testing.assert_array_equal(lo, torch.from_numpy(v - hi).to(torch.bfloat16).float().numpy())
    assert hi[-5] == 1.0 and hi[-4] == np.float32(1.015625)
    ok = np.abs(v) > 1e-20
    assert np.all(np.abs((v - hi - lo)[ok]) <= np.abs(v[ok]) * 2.0 ** -16)                           # what the lo x lo term's neglect rests on


@pytest.fixture(scope="module")
def restated():
    """per GPU test shape: (float64 convolution, restatement, inputs, relu), computed once"""
    out = []
    for N, Cin, Cout, H, W, relu in co.CASES:
        x, w, b = co.inputs(N, Cin, Cout, H, W)
        out.append((co.conv_f64(x, w, b, relu), co.conv_split(x, w, b, relu), (x, w, b), relu))
    return out


def test_the_gpu_tests_shapes_are_the_issues_and_cover_every_route():
    assert co.CASES[:12] == [(2, 64, 64, 33, 65, True), (2, 64, 64, 20, 31, False), (2, 112, 112, 18, 45, True), (1, 16, 128, 8, 40, False),
                             (1, 48, 96, 5, 33, True), (1, 64, 64, 1, 5, True), (3, 16, 64, 61, 33, False), (1, 64, 33, 9, 40, False),
                             (3, 32, 100, 13, 70, True), (1, 160, 40, 9, 70, True), (1, 64, 64, 300, 100, True), (1, 112, 112, 130, 70, True)]
    assert any(c[2] <= 32 for c in co.CASES) and all(csl.eligible(c[1], c[2]) for c in co.CASES)


def test_the_restatement_is_within_3e_5_of_the_scale_from_float64_at_every_gpu_shape(restated):
    for (exact, rest, _, _), case in zip(restated, co.CASES):
        scale = float(np.abs(exact).max())
        err = float(np.abs(rest - exact).max())
        print("%s: scale %.3g, restatement vs float64 %.3g" % (case, scale, err))
        assert err <= 3e-5 * scale and scale > 0.5


@pytest.mark.parametrize("drop", ["hi.lo", "lo.hi"])
def test_a_missing_cross_term_moves_the_restatement_by_100_times_the_first_bar(restated, drop):
    """so the GPU tests' 1e-5 * max(1, scale) bar against the restatement sees a kernel that leaves a term out"""
    for (exact, rest, (x, w, b), relu), case in zip(restated, co.CASES):
        scale = float(np.abs(exact).max())
        moved = float(np.abs(co.conv_split(x, w, b, relu, drop=drop) - rest).max())
        print("%s without %s: %.3g" % (case, drop, moved))
        assert moved >= 100 * 1e-5 * max(1.0, scale)


def test_the_restatement_equals_rational_arithmetic_on_exact_data():
    """exact data (every partial sum an fp32 number): the restatement's float64 sums are the exact sums, checked here with Fractions at
    the image's corners, edges and a few interior pixels, term by term from the definition."""
    N, Cin, Cout, H, W = 2, 32, 40, 21, 37
    x, w, b = co.exact_data(N, Cin, Cout, H, W)
    assert co.exact_data_is_exact(x, w)
    rest = co.conv_split(x, w, b, False)
    xhi, xlo = co.split(x)
    whi, wlo = co.split(w)
    F = lambda v: Fraction(float(v))           # noqa: E731  (every float is a dyadic rational)
    for n, o, y, xx in ((0, 0, 0, 0), (1, 39, H - 1, W - 1), (0, 17, 0, W - 1), (1, 5, H - 1, 0), (0, 33, 10, 0), (1, 8, 0, 20), (0, 21, 11, 18),
                        (1, 30, 7, 31)):
        s = Fraction(0)
        for ci in range(Cin):
            for ky in range(3):
                for kx in range(3):
                    yy, xc = y + ky - 1, xx + kx - 1
                    if 0 <= yy < H and 0 <= xc < W:
                        s += F(whi[o, ci, ky, kx]) * F(xhi[n, ci, yy, xc]) + F(whi[o, ci, ky, kx]) * F(xlo[n, ci, yy, xc]) \
                            + F(wlo[o, ci, ky, kx]) * F(xhi[n, ci, yy, xc])
        assert Fraction(float(np.float32(float(s)))) == s                  # the sum is an fp32 number
        assert float(rest[n, o, y, xx]) == float(np.float32(np.float32(float(s)) + b[o]))
