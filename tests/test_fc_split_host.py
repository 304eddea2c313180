"""CPU: the host side of `-fc_mode bf16x3` (include/mc_fc_split.h): libmcfcsplit.so's symbols, workspace formula and refusals, its place
in the Makefile and the kernel inventory, the flag on the parsers and hs.py, the default path's independence of the new library, and
the arithmetic's restatement (tests/fc_split_oracle.py) against the exact-product evaluation."""
import ctypes as C
import os
import re
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fc_split_oracle as fo  # noqa: E402
import libraries as L  # noqa: E402
from mc_cnn_amd import _fc_split_lib as fsl  # noqa: E402
from mc_cnn_amd import hs, train_mb, train_mb_slow, train_slow  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402

HEADER = os.path.join(ROOT, "include", "mc_fc_split.h")
FC_CASES = [(8, 5, 50, 10, 3), (16, 3, 100, 7, 2), (112, 2, 40, 48, 3), (4, 9, 97, 5, 1)]     # tests/test_gpu_fc.py::test_fc_stack


def fc_inputs(C_, H, W, n_hidden):
    """the inputs of tests/test_gpu_fc.py::test_fc_stack"""
    from test_gpu_fc import make_layers
    from util import features
    return np.maximum(features(C_, H, W, seed=C_ + W), 0) * 3.0, make_layers(C_, n_hidden, seed=W)


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_loads_without_a_gpu_and_exports_exactly_the_headers_symbols():
    """what only libmcfcsplit.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    text = open(HEADER).read()
    assert fsl.load().mc_fc_split_version() == fsl.ABI_VERSION == 1
    assert L.exported_abi(fsl.LIB_PATH) == {"mc_fc_split_version", "mc_fc_split_last_error", "mc_fc_split_workspace_bytes", "mc_fc_split_stack"}
    assert re.search(r"#define MC_FC_SPLIT_NH %d\b" % fsl.NH, text) and re.search(r"#define MC_FC_SPLIT_VOXELS %d\b" % fsl.VOXELS, text)
    assert (fsl.NH, fsl.EINVAL) == (384, -22) and os.path.basename(fsl.LIB_PATH) == "libmcfcsplit.so"


def test_workspace_formula_is_monotone_and_256_aligned():
    lib = fsl.load()
    base = lib.mc_fc_split_workspace_bytes(112, 5, 370, 1226)
    # the two projections, layer 1's transposed halves, a hi and a lo bf16 plane per hidden layer
    assert base == (2 * 370 * 1226 * 384 * 4 + 2 * 112 * 384 * 4 + 3 * 2 * 384 * 384 * 2 + 255) // 256 * 256
    for Cn, n, H, W in ((1, 2, 1, 1), (5, 3, 7, 9), (112, 5, 370, 1226), (112, 8, 1000, 1500)):
        b = lib.mc_fc_split_workspace_bytes(Cn, n, H, W)
        assert b > 0 and b % 256 == 0
        assert lib.mc_fc_split_workspace_bytes(Cn + 1, n, H, W) >= b and lib.mc_fc_split_workspace_bytes(Cn, n, H + 1, W) >= b
        assert lib.mc_fc_split_workspace_bytes(Cn, n, H, W + 1) >= b
        if n < 8:
            assert lib.mc_fc_split_workspace_bytes(Cn, n + 1, H, W) > b
    for bad in ((0, 3, 4, 4), (4, 1, 4, 4), (4, 9, 4, 4), (4, 3, 0, 4), (4, 3, 4, 0), (-1, 3, 4, 4)):
        assert lib.mc_fc_split_workspace_bytes(*bad) == 0


def test_every_refusal_returns_einval_with_its_message_before_any_launch():
    lib = fsl.load()
    P = 1 << 20                      # never dereferenced: every check precedes the first launch

    def call(featL=P, featR=P, Cn=8, H=5, W=50, D=10, widths=(384, 384, 384, 1), weights=None, biases=None, null_arrays=(), volL=P, volR=P,
             ws=P, ws_bytes=None, n=None):
        n_arr = len(widths)
        n = n_arr if n is None else n
        wp = (C.c_void_p * n_arr)(*(weights if weights is not None else [P] * n_arr))
        bp = (C.c_void_p * n_arr)(*(biases if biases is not None else [P] * n_arr))
        lo = (C.c_int * n_arr)(*widths)
        need = lib.mc_fc_split_workspace_bytes(Cn, n, H, W) if ws_bytes is None else ws_bytes
        return lib.mc_fc_split_stack(featL, featR, Cn, H, W, D, None if "weights" in null_arrays else wp, None if "biases" in null_arrays else bp,
                                     None if "widths" in null_arrays else lo, n, volL, volR, ws, need, None)

    need = lib.mc_fc_split_workspace_bytes(8, 4, 5, 50)
    bad = [("null featL", lambda: call(featL=None), "null pointer"), ("null featR", lambda: call(featR=None), "null pointer"),
           ("null volL", lambda: call(volL=None), "null pointer"), ("null volR", lambda: call(volR=None), "null pointer"),
           ("null workspace", lambda: call(ws=None, ws_bytes=need), "null pointer"),
           ("null weights", lambda: call(null_arrays=("weights",)), "null pointer"), ("null biases", lambda: call(null_arrays=("biases",)), "null pointer"),
           ("null widths", lambda: call(null_arrays=("widths",)), "null pointer"),
           ("a null weight", lambda: call(weights=[P, None, P, P]), "null pointer in layer 1"),
           ("a null bias", lambda: call(biases=[P, P, P, None]), "null pointer in layer 3"),
           ("C 0", lambda: call(Cn=0, ws_bytes=need), "bad dims"), ("H 0", lambda: call(H=0, ws_bytes=need), "bad dims"),
           ("W -1", lambda: call(W=-1, ws_bytes=need), "bad dims"), ("D 0", lambda: call(D=0), "bad dims"),
           ("one layer", lambda: call(widths=(1,), ws_bytes=need), "2..8 layers"),
           ("nine layers", lambda: call(widths=(384,) * 8 + (1,), ws_bytes=need), "2..8 layers"),
           ("hidden width 256", lambda: call(widths=(384, 256, 384, 1)), "hidden width 256"),
           ("first width 128", lambda: call(widths=(128, 1)), "hidden width 128"),
           ("two outputs", lambda: call(widths=(384, 384, 2)), "one output"),
           ("workspace one byte short", lambda: call(ws_bytes=need - 1), "workspace %d < %d" % (need - 1, need)),
           ("the workspace of a shallower stack", lambda: call(ws_bytes=lib.mc_fc_split_workspace_bytes(8, 3, 5, 50)), "workspace"),
           ("workspace off alignment", lambda: call(ws=P + 8), "16-byte aligned"),
           ("a grid past one launch", lambda: call(H=1 << 16, W=1, D=1 << 15, ws_bytes=1 << 62), "too large for one launch")]
    for what, f, word in bad:
        rc = f()
        assert rc == fsl.EINVAL, (what, rc)
        msg = fsl.last_error()
        assert msg.startswith("mc_fc_split_stack:") and word in msg, (what, msg)
    with pytest.raises(fsl.FcSplitError, match="hidden width 256"):
        fsl.check(call(widths=(384, 256, 384, 1)), "mc_fc_split_stack")


def test_the_library_is_built_from_its_own_unit_and_holds_its_own_kernels():
    assert L.print_libraries()["libmcfcsplit.so"] == ["fc_split.o", "error.o"]
    out = L.make("-n", "-B", "../libmcfcsplit.so")
    assert "fc_split.hip" in out and "error.hip" in out and "-o ../libmcfcsplit.so" in out and "fc_stack.hip" not in out
    assert "fc_split" not in L.make("-n", "-B", "../libmcadcensus.so")               # libmcadcensus.so keeps its kernel set
    assert L.built_kernels(fsl.LIB_PATH) == {"fcs_project_kernel", "fcs_transpose_kernel", "fcs_split_weights_kernel", "fcs_stack_kernel"}


# ---- the flag ------------------------------------------------------------------------------------------------------------------
SLOW_LINES = [(mcmain.parse, ["kitti", "slow", "-a", "predict"]), (mcmain.parse, ["mb", "slow", "-a", "time"]),
              (train_slow.parse, ["kitti", "slow", "-a", "test_te"]), (train_slow.parse, ["kitti2015", "slow", "-a", "train_tr"]),
              (train_slow.parse, ["kitti", "slow", "-a", "test_all"]), (train_mb_slow.parse, ["mb", "slow", "-a", "test_te"]),
              (train_mb_slow.parse, ["mb", "slow", "-a", "train_tr"])]


def test_the_default_is_fp32_and_bf16x3_is_accepted_on_arch_slow():
    for parse, argv in SLOW_LINES:
        assert parse(argv)[2].fc_mode == "fp32", argv
        assert parse(argv + ["-fc_mode", "fp32"])[2].fc_mode == "fp32", argv
        assert parse(argv + ["-fc_mode", "bf16x3"])[2].fc_mode == "bf16x3", argv
        with pytest.raises(SystemExit):
            parse(argv + ["-fc_mode", "bf16"])          # the one-pass mode is not offered
    # main.route sends the same lines to the same parsers
    assert mcmain.route(["kitti", "slow", "-a", "train_tr", "-fc_mode", "bf16x3"])[4].fc_mode == "bf16x3"
    assert mcmain.route(["mb", "slow", "-a", "test_te"])[4].fc_mode == "fp32"
    for argv in (["random", "kitti", "slow", "test_te", "net.t7"], ["grid", "mb", "slow", "test_te", "net.t7"]):
        argv[0] = hs.METHODS[0]
        assert hs.parse(argv).fc_mode == "fp32" and hs.parse(argv + ["-fc_mode", "bf16x3"]).fc_mode == "bf16x3"


@pytest.mark.parametrize("parse, argv", [
    (mcmain.parse, ["kitti", "fast", "-a", "predict"]), (mcmain.parse, ["kitti", "ad", "-a", "predict"]),
    (mcmain.parse, ["mb", "census", "-a", "time"]), (mcmain.parse, ["kitti2015", "fast", "-a", "test_te"]),
    (train_mb.parse, ["mb", "fast", "-a", "test_te"])])
def test_bf16x3_is_refused_where_there_is_no_fc_stack(parse, argv):
    with pytest.raises(SystemExit) as e:
        parse(argv + ["-fc_mode", "bf16x3"])
    for word in ("-fc_mode bf16x3", "arch " + argv[1], "no FC stack", "arch slow"):
        assert word in str(e.value), (word, str(e.value))
    plain, given = parse(argv)[2], parse(argv + ["-fc_mode", "fp32"])[2]
    assert vars(plain) == vars(given) and not hasattr(plain, "fc_mode")          # -fc_mode fp32 there changes nothing


def test_hs_refuses_bf16x3_off_arch_slow_and_evalset_takes_the_mode():
    for arch in ("fast", "ad", "census"):
        with pytest.raises(SystemExit, match="only arch slow has an FC stack"):
            hs.parse([hs.METHODS[0], "kitti", arch, "test_te", "net.t7", "-fc_mode", "bf16x3"])
    src = open(os.path.join(ROOT, "mc-cnn_amd", "evalset.py")).read()
    assert "fc_mode=self.fc_mode" in src and 'getattr(opt, "fc_mode", "fp32")' in src


def test_a_saved_net_does_not_record_the_flag(tmp_path):
    _, _, opt, _ = train_slow.parse(["kitti", "slow", "-a", "train_tr", "-fc_mode", "bf16x3"])
    _, _, opt0, _ = train_slow.parse(["kitti", "slow", "-a", "train_tr"])
    conv, fc = train_slow.init_net(3)
    a = train_slow.save_net(str(tmp_path / "a.t7"), conv, fc, opt)
    b = train_slow.save_net(str(tmp_path / "b.t7"), conv, fc, opt0)
    assert open(a, "rb").read() == open(b, "rb").read()


# ---- the default path never touches the new library ---------------------------------------------------------------------------------
class FakeTensor:
    """What fc_cost_volumes asks of a CUDA tensor, on the host."""
    is_cuda, device = True, "cuda:0"

    def __init__(self, shape, ptr, dtype):
        self.shape, self.ptr, self.dtype = tuple(shape), ptr, dtype

    def contiguous(self):
        return self

    def reshape(self, *a):
        return self

    def numel(self):
        return int(np.prod(self.shape))

    def data_ptr(self):
        return self.ptr

    def __getitem__(self, i):
        return FakeTensor(self.shape[1:], self.ptr + 4096 * (i + 1), self.dtype)


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_fc_cost_volumes_calls_the_library_of_its_mode_only(mode, monkeypatch):
    import torch
    from mc_cnn_amd import fc
    calls = []

    def stub(name, ret):
        def f(*a):
            calls.append((name, a))
            return ret
        return f
    fake_torch = types.SimpleNamespace(
        float32=torch.float32, uint8=torch.uint8, full=lambda shape, *a, **k: FakeTensor(shape, 0x7000000, torch.float32),
        empty=lambda n, **k: FakeTensor((n,), 0x9000000, torch.uint8), cuda=types.SimpleNamespace(current_stream=lambda: types.SimpleNamespace(cuda_stream=0)))
    monkeypatch.setattr(fc, "torch", fake_torch)
    monkeypatch.setattr(fc, "lib", types.SimpleNamespace(mc_fc_stack_workspace_bytes=stub("mc_fc_stack_workspace_bytes", 1024),
                                                         mc_fc_stack=stub("mc_fc_stack", 0)))
    split = types.SimpleNamespace(mc_fc_split_workspace_bytes=stub("mc_fc_split_workspace_bytes", 2048), mc_fc_split_stack=stub("mc_fc_split_stack", 0))
    loads = []
    monkeypatch.setattr(fsl, "load", lambda: loads.append(1) or split)
    feat = FakeTensor((2, 4, 3, 10), 0x1000000, torch.float32)
    layers = [(FakeTensor(s, 0x2000000 + 65536 * i, torch.float32), FakeTensor((s[0],), 0x3000000 + 65536 * i, torch.float32))
              for i, s in enumerate(((384, 8), (384, 384), (1, 384)))]
    kw = {} if mode == "fp32" else {"mode": mode}          # the default is fp32
    vl, vr = fc.fc_cost_volumes(feat, layers, 5, **kw)
    names = [n for n, _ in calls]
    if mode == "fp32":
        assert names == ["mc_fc_stack_workspace_bytes", "mc_fc_stack"] and not loads
    else:
        assert names == ["mc_fc_split_workspace_bytes", "mc_fc_split_stack"] and loads
    args = calls[1][1]              # the argument list of mc_fc_stack, whichever library takes it
    assert args[2:6] == (4, 3, 10, 5) and args[9] == 3 and list(args[8]) == [384, 384, 1] and args[13] == (1024 if mode == "fp32" else 2048)
    assert args[0] == feat[0].data_ptr() and args[1] == feat[1].data_ptr() and args[12] % 16 == 0
    with pytest.raises(ValueError, match="fp32 | bf16x3"):
        fc.fc_cost_volumes(feat, layers, 5, mode="bf16")


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def test_split_is_round_to_nearest_even_and_exact_in_two_parts():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 6, 4000).astype(np.float32),
                        np.array([0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-30], np.float32)])
    hi, lo = fo.split(v)
    np.testing.assert_array_equal(hi, torch.from_numpy(v).to(torch.bfloat16).float().numpy())       # ties to even: 1.00390625 -> 1.0
    np.testing.assert_array_equal(lo, torch.from_numpy(v - hi).to(torch.bfloat16).float().numpy())
    assert hi[-5] == 1.0 and hi[-4] == np.float32(1.015625)
    ok = np.abs(v) > 1e-20
    assert np.all(np.abs((v - hi - lo)[ok]) <= np.abs(v[ok]) * 2.0 ** -16)                           # what the lo x lo term's neglect rests on


@pytest.fixture(scope="module")
def restated(oracle):
    """per case of test_fc_stack: (exact-product volL, the restatement's volL, the mask of defined voxels, the inputs)"""
    out = []
    for C_, H, W, D, n_hidden in FC_CASES:
        f, layers = fc_inputs(C_, H, W, n_hidden)
        wl, wr = oracle.fc_stack(f[0], f[1], D, layers)
        sl, sr = fo.fc_split_stack(f[0], f[1], D, layers)
        assert np.array_equal(np.isnan(sl), np.isnan(wl)) and np.array_equal(np.isnan(sr), np.isnan(wr))
        out.append((wl, sl, ~np.isnan(wl), (f, layers, D)))
    return out


def test_the_restatement_is_within_1e_5_of_the_exact_product_evaluation(restated):
    for wl, sl, ok, _ in restated:
        err = np.abs(sl[ok] - wl[ok]).max()
        print("restatement vs exact products: %.3g" % err)
        assert err <= 1e-5 and wl[ok].std() > 1e-3


@pytest.mark.parametrize("drop", ["hi.lo", "lo.hi"])
def test_a_missing_cross_term_moves_the_restatement_by_5e_5_or_more(restated, drop):
    """so the GPU tests' 1e-5 bar against the restatement sees a kernel that leaves a term out"""
    for wl, sl, ok, (f, layers, D) in restated:
        less, _ = fo.fc_split_stack(f[0], f[1], D, layers, drop=drop)
        moved = np.abs(less[ok] - sl[ok]).max()
        print("without %s: %.3g" % (drop, moved))
        assert moved >= 5e-5
