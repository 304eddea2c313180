"""CPU: the host side of `mb slow -a train_tr | train_all | test_te` (main.lua:116-130, 602-890): flags and routing (one
routing table; the other parsers keep refusing `mb slow`), the flat parameter layout and the saved net, libmctrainmbslow.so's
symbols, constants, workspace sizes, argument checks and kernel inventory, and the host loop of `train_mb_slow.train` with a
recording stand-in for its Trainer."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libraries as L  # noqa: E402
import train_mb_slow_oracle as so  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402
from mc_cnn_amd import train_mb as tm  # noqa: E402
from mc_cnn_amd import train_mb_slow as tms  # noqa: E402
from mc_cnn_amd import train_slow as ts  # noqa: E402


# ---- parse and routing -----------------------------------------------------------------------------------------------------
def test_parse_defaults_are_main_luas_for_mb_slow():
    for a in ("train_tr", "train_all", "test_te"):
        dataset, arch, opt, prm = tms.parse(["mb", "slow", "-a", a])
        assert (dataset, arch, opt.a) == ("mb", "slow", a)
    want = dict(seed=42, lr=0.003, bs=128, mom=0.9, true1=0.5, false1=1.5, false2=18, d_exp=0.2, d_light=0.2, ds=2001,   # main.lua:116-130
                hflip=0, vflip=0, rotate=28, hscale=0.8, scale=0.8, trans=0, hshear=0.1, brightness=1.3, contrast=1.1,   # main.lua:51-65
                d_vtrans=1, d_rotate=3, d_hscale=0.9, d_hshear=0.3, d_brightness=0.7, d_contrast=1.1,
                rect="imperfect", color="gray", data_dir="", epochs=14, max_steps=0, gpu=1, net_fname="random:42")
    for k, v in want.items():
        assert getattr(opt, k) == v, k
    assert not hasattr(opt, "m") and not hasattr(opt, "pow")
    assert tms.data_dir_of(opt) == "data.mb.imperfect_gray"
    # the hyper-parameters of main.lua:132-144, as main.parse builds them for -a predict, and direction -1 only
    _, _, _, want_prm = mcmain.parse(["mb", "slow", "-a", "predict"])
    assert prm.pop("left_only") == 1 and want_prm.get("left_only", 0) == 0
    want_prm.pop("left_only", None)
    assert prm == want_prm and prm["L1"] == 14 and prm["pi2"] == 13.9 and prm["blur_sigma"] == 1.67


def test_parse_overrides():
    _, _, opt, prm = tms.parse(["mb", "slow", "-a", "train_all", "-seed", "7", "-lr", "0.01", "-bs", "64", "-d_exp", "0.5", "-d_light", "0",
                                "-ds", "5", "-rect", "perfect", "-max_steps", "5", "-epochs", "2", "-pi1", "2.5", "-net_fname", "x.t7",
                                "-false2", "8", "-hflip", "1"])
    assert (opt.seed, opt.lr, opt.bs, opt.d_exp, opt.d_light, opt.ds, opt.max_steps, opt.epochs, opt.net_fname, opt.false2, opt.hflip) == \
        (7, 0.01, 64, 0.5, 0, 5, 5, 2, "x.t7", 8, 1)
    assert prm["pi1"] == 2.5 and tms.data_dir_of(opt) == "data.mb.perfect_gray"
    assert tms.data_dir_of(tms.parse(["mb", "slow", "-a", "test_te", "-data_dir", "d"])[2]) == "d"


@pytest.mark.parametrize("argv, word", [
    (["mb", "slow", "-a", "train_tr", "-color", "rgb"], "one input plane"),
    (["mb", "slow", "-a", "test_all"], "main.lua:1136"),
    (["mb", "slow", "-a", "submit"], "submit is out of scope"),
    (["mb", "slow", "-a", "train_tr", "-subset", "0.5"], "-subset"),
    (["mb", "slow", "-a", "train_tr", "-debug"], "-debug"),
    (["mb", "slow", "-a", "predict"], "not a training or testing action"),
    (["mb", "fast", "-a", "train_tr"], "mb slow"),
    (["kitti", "slow", "-a", "train_tr"], "mb slow"),
    (["mb", "slow", "-a", "train_tr", "-bs", "7"], "pairs of samples"),
    (["mb", "slow", "-a", "train_tr", "-bs", "0"], "pairs of samples")])
def test_parse_refuses_what_is_out_of_scope_and_says_why(argv, word):
    with pytest.raises(SystemExit) as e:
        tms.parse(argv)
    assert word in str(e.value), str(e.value)


@pytest.mark.parametrize("flag", [["-m", "0.2"], ["-pow", "1"]])
def test_parse_has_no_margin_and_no_pow(flag):
    with pytest.raises(SystemExit):
        tms.parse(["mb", "slow", "-a", "train_tr"] + flag)


def test_main_routes_mb_slow_training_and_the_old_routes_keep_refusing_it():
    route = mcmain.training_module
    for a in ("train_tr", "train_all", "test_te"):
        # to train_mb_slow and so to neither train_slow nor train_mb, whose parsers refuse these command lines as before
        assert route(["mb", "slow", "-a", a]) is tms and route(["mb", "slow", "-seed", "3", "-a", a, "-bs", "64"]) is tms
        with pytest.raises(SystemExit, match="fast only"):
            mcmain.parse(["mb", "slow", "-a", a])
        with pytest.raises(SystemExit, match="train_mb.parse"):
            mcmain.parse(["mb", "slow", "-a", a])
        with pytest.raises(SystemExit, match="221 KB"):
            tm.parse(["mb", "slow", "-a", a])
        with pytest.raises(SystemExit):
            ts.parse(["mb", "slow", "-a", a])
    # everything that routes to the other modules, and what routes to none
    for argv, want in ((["mb", "fast", "-a", "train_tr"], tm), (["mb", "fast", "-a", "test_te"], tm), (["kitti", "slow", "-a", "train_tr"], ts),
                       (["kitti2015", "slow", "-a", "test_all"], ts), (["kitti", "fast", "-a", "train_tr"], None),
                       (["mb", "slow", "-a", "predict"], None), (["mb", "slow", "-a", "time"], None), (["mb", "slow", "-a", "test_all"], None),
                       (["mb", "slow", "-a", "submit"], None), (["mb", "slow"], None), (["mb", "slow", "-a"], None),
                       (["mb", "census", "-a", "train_tr"], None)):
        assert route(argv) is want, argv
    assert "train_mb_slow" in str(pytest.raises(SystemExit, tm.parse, ["mb", "slow", "-a", "train_tr"]).value)


# ---- parameters and the saved net ----------------------------------------------------------------------------------------
def test_flat_params_round_trip_and_layout():
    conv, fc = tms.init_net(3)
    assert [w.shape for w, _ in conv] == so.CONV_SHAPES and [w.shape for w, _ in fc] == so.FC_SHAPES
    assert len(conv) == 5 and len(fc) == 4
    for layers in (conv, fc):      # the ranges of the two reset()s
        for w, b in layers:
            bound = 1 / np.sqrt(np.prod(w.shape[1:]))
            assert np.abs(w).max() <= bound and np.abs(b).max() <= bound and np.abs(w).max() > 0.9 * bound
    wide, _ = tms.init_net(3, gain=2.0)
    assert np.abs(wide[1][0]).max() > 1.8 / np.sqrt(112 * 9)
    v = tms.flat_params(conv, fc)
    assert v.size == 835617 == tms.tmsl.NPARAMS == tms.tmsl.NCONV + tms.tmsl.NFC and v.dtype == np.float32
    assert tms.tmsl.NCONV == 453152 == 112 * 9 + 112 + 4 * (112 * 112 * 9 + 112)
    assert tms.tmsl.NFC == 382465 == 384 * 224 + 384 + 2 * (384 * 384 + 384) + 384 + 1
    np.testing.assert_array_equal(v, so.flat(conv, fc))
    names = tms.tensor_names()
    assert len(names) == 18 and sum(n for _, n in names) == 835617 and [n for n, _ in names] == so.NAMES
    # the header's order: w1 b1 .. w5 b5 fw1 fb1 .. fw4 fb4
    np.testing.assert_array_equal(v[:1008], conv[0][0].ravel())
    np.testing.assert_array_equal(v[1008:1120], conv[0][1])
    np.testing.assert_array_equal(v[1120:1120 + 112 * 112 * 9], conv[1][0].ravel())
    np.testing.assert_array_equal(v[453152 - 112:453152], conv[4][1])
    np.testing.assert_array_equal(v[453152:453152 + 384 * 224], fc[0][0].ravel())
    np.testing.assert_array_equal(v[-385:-1], fc[3][0].ravel())
    assert v[-1] == fc[3][1][0]
    o = 0
    for name, n in names:             # every fw offset is a multiple of 4 (float4 loads)
        assert not name.startswith("fw") or o % 4 == 0, name
        o += n
    conv2, fc2 = tms.unflat_params(v)
    for a, b in zip(conv + fc, conv2 + fc2):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        tms.flat_params(conv[:4], fc)
    with pytest.raises(ValueError):
        tms.flat_params(*ts.init_net(3))          # the KITTI accurate net: 4 + 5 layers
    with pytest.raises(ValueError):
        tms.unflat_params(v[:-1])


def test_saved_net_round_trips_into_the_readers(tmp_path):
    from mc_cnn_amd import t7
    conv, fc = tms.init_net(5)
    argv = ["-a", "train_tr", "-seed", "5"]
    _, _, opt, _ = tms.parse(["mb", "slow"] + argv)
    fname = tms.net_fname_of("mb", "slow", argv)
    assert fname == os.path.join("net", "net_mb_slow_-a_train_tr_-seed_5.t7")     # main.lua:344-347, 594
    path = tms.save_net(str(tmp_path / fname), conv, fc, opt)
    got_conv, got_fc = t7.load_reference_net(path, "slow")
    assert len(got_conv) == 5 and len(got_fc) == 4
    for want, got in ((conv, got_conv), (fc, got_fc), (conv, mcmain.load_net(path, "mb", "slow")), (fc, mcmain.load_fc(path, "mb"))):
        assert len(want) == len(got)
        for (w, b), (w2, b2) in zip(want, got):
            assert w2.shape == w.shape and b2.shape == b.shape
            np.testing.assert_array_equal(w, w2)
            np.testing.assert_array_equal(b, b2)
    obj = t7.load(path)
    assert obj[3]["seed"] == 5 and obj[3]["a"] == "train_tr" and obj[3]["lr"] == 0.003 and obj[3]["false2"] == 18
    assert [m.cls for m in t7._modules(obj[1])] == ["cudnn.SpatialConvolution", "cudnn.ReLU"] * 5
    mods2 = t7._modules(obj[2])
    assert [m.cls for m in mods2] == ["nn.SpatialConvolution1_fw", "cudnn.ReLU"] * 3 + ["nn.SpatialConvolution1_fw", "cudnn.Sigmoid"]
    assert np.asarray(mods2[0]["weight"]).shape == (384, 224) and np.asarray(mods2[6]["weight"]).shape == (1, 384)


def test_oracle_forward_pairs_left_with_positive_then_negative():
    import torch
    conv, fc = so.wide_nets(1)
    rng = np.random.default_rng(0)
    p = torch.tensor(rng.standard_normal((3, 3, 11, 11)))
    o = so.forward(so.as_f64(conv), so.as_f64(fc), p)
    assert o.shape == (6,)
    swapped = p.clone()
    swapped[:, 1], swapped[:, 2] = p[:, 2], p[:, 1]
    o2 = so.forward(so.as_f64(conv), so.as_f64(fc), swapped)
    np.testing.assert_allclose(o2.numpy().reshape(3, 2), o.numpy().reshape(3, 2)[:, ::-1], rtol=1e-12)
    assert so.fragile(conv, fc, p.numpy()).shape == (3,) and so.fragile(conv, fc, p.numpy(), eps=1e3).all()


# ---- the library -------------------------------------------------------------------------------------------------------
HEADER = os.path.join(ROOT, "include", "mc_train_mb_slow.h")


def test_library_loads_without_a_gpu_and_exports_the_headers_symbols():
    """what only libmctrainmbslow.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    assert tms.tmsl.load().mc_train_mb_slow_version() == 1 and len(L.exported_abi(tms.tmsl.LIB_PATH)) == 5     # no sampler entry point
    built = L.built_kernels(tms.tmsl.LIB_PATH)
    # the FC kernels are the KITTI accurate net's (one header, compiled into both libraries); the rest is this library's own,
    # and there is no sampler kernel: libmctrainmb.so's draws the same patches
    assert built == L.SHARED_KERNELS | {"mb_tower_forward_kernel<true>", "mb_tower_forward_kernel<false>", "mb_tower_backward_kernel", "mb_slow_sgd_kernel"}
    assert len(built) == 8 and built & set(L.read_inventory("kernel_inventory_train_slow.txt")) == L.SHARED_KERNELS
    assert L.SHARED_KERNELS == {"fc_forward_kernel", "fc_head_kernel", "fc_backward_kernel<true>", "fc_backward_kernel<false>"}
    assert not any("sample" in k for k in built)


def test_loader_constants_equal_the_headers_defines():
    text = open(HEADER).read()
    t = tms.tmsl
    defines = dict(re.findall(r"#define MC_TRAIN_MB_SLOW_(\w+) (-?\d+)\b", text))
    mirrored = dict(ABI_VERSION=t.ABI_VERSION, WS=t.WS, FM=t.FM, L1=t.L1, L2=t.L2, NH2=t.NH2, NPRM=t.NPRM, NCONV=t.NCONV, NFC=t.NFC,
                    NPARAMS=t.NPARAMS, MAX_PAIRS=t.MAX_PAIRS)
    assert {k: int(v) for k, v in defines.items()} == mirrored
    assert (t.WS, t.FM, t.L1, t.L2, t.NH2, t.NPRM, t.MAX_PAIRS) == (11, 112, 5, 3, 384, 18, 256)
    assert t.EINVAL == -22 and re.search(r"#define MC_EINVAL \(-22\)", text)
    assert (t.WS, t.NPRM) == (tm.tml.WS, tm.tml.NPRM)        # the sampler's, shared with libmctrainmb.so


def test_workspace_bytes():
    wb = tms.tmsl.load().mc_train_mb_slow_workspace_bytes
    M = tms.tmsl.MAX_PAIRS
    assert wb(0) == 0 and wb(-1) == 0 and wb(M + 1) == 0
    sizes = [wb(n) for n in (1, 2, 3, 64, 65, M)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # at least one slab row per PATCH and the FC parameters' gradient; 348 MB of slab at 64 pairs, about 1.4 GB at the cap
    assert wb(64) >= 4 * (3 * 64 * tms.tmsl.NCONV + tms.tmsl.NFC) and 3 * 64 * tms.tmsl.NCONV * 4 == 348020736
    assert wb(1) < 4 * (3 * tms.tmsl.NCONV + tms.tmsl.NFC) + (1 << 20)
    assert 1.39e9 < wb(M) < 1.41e9


def test_argument_checks_return_einval_with_a_message_before_any_launch():
    lib = tms.tmsl.load()
    P = 1 << 20                      # never dereferenced: every check precedes the first launch
    need = lib.mc_train_mb_slow_workspace_bytes(4)

    def step(patches=P, n=4, params=P, moms=P, loss=P, ws=P, ws_bytes=need):
        return lib.mc_train_mb_slow_step_batch(patches, n, params, moms, 0.003, 0.9, loss, ws, ws_bytes, None)

    def run(planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, src=P, prm=P, params=P, moms=P,
            losses=P, ws=P, ws_bytes=need):
        return lib.mc_train_mb_slow_run(planes, table, n_planes, nnz, n_nnz, perm, n_perm, t0, n_steps, n, src, prm, params, moms, 0.003,
                                        0.9, losses, ws, ws_bytes, None)

    bad = [("n_pairs 0", lambda: step(n=0), "n_pairs"), ("n_pairs above the maximum", lambda: step(n=tms.tmsl.MAX_PAIRS + 1), "n_pairs"),
           ("null patches", lambda: step(patches=None), "null"), ("null params", lambda: step(params=None), "null"),
           ("null moms", lambda: step(moms=None), "null"), ("null loss", lambda: step(loss=None), "null"),
           ("null workspace", lambda: step(ws=None), "workspace"), ("workspace one byte short", lambda: step(ws_bytes=need - 1), "workspace"),
           ("misaligned params", lambda: step(params=P + 4), "aligned"), ("misaligned workspace", lambda: step(ws=P + 4), "aligned"),
           ("run: null planes", lambda: run(planes=None), "null"), ("run: null table", lambda: run(table=None), "null"),
           ("run: null nnz", lambda: run(nnz=None), "null"), ("run: null perm", lambda: run(perm=None), "null"),
           ("run: null src", lambda: run(src=None), "null"), ("run: null prm", lambda: run(prm=None), "null"),
           ("run: null losses", lambda: run(losses=None), "null"), ("run: n_pairs 0", lambda: run(n=0), "n_pairs"),
           ("run: n_pairs above the maximum", lambda: run(n=tms.tmsl.MAX_PAIRS + 1), "n_pairs"),
           ("run: workspace one byte short", lambda: run(ws_bytes=need - 1), "workspace"),
           ("run: steps past the permutation", lambda: run(t0=93), "permutation"), ("run: negative t0", lambda: run(t0=-1), "permutation"),
           ("run: negative n_steps", lambda: run(n_steps=-1), "n_steps"), ("run: no planes", lambda: run(n_planes=0), "n_planes"),
           ("run: empty nnz", lambda: run(n_nnz=0), "nnz")]
    for what, call, word in bad:
        rc = call()
        assert rc == tms.tmsl.EINVAL, (what, rc)
        assert word in tms.tmsl.last_error(), (what, tms.tmsl.last_error())
    with pytest.raises(tms.tmsl.TrainMbSlowError, match="n_pairs"):
        tms.tmsl.check(step(n=0), "mc_train_mb_slow_step_batch")


# ---- the host loop -------------------------------------------------------------------------------------------------------
N_TR, N_TE = 21, 5      # bs 4 (2 pairs per step): `for t = 1, 21 - 2, 2` is a 10-step epoch
INDEX = np.array([[0, 2, 2], [8, 1, 1], [10, 3, 3], [28, 2, 1], [32, 1, 2]], np.int64)   # (first plane, lights, exposures) of 5 images


class Recorder:
    """Stands in for train_mb_slow.Trainer: stores the constructor's arguments and every run() call; a step's loss is its
    index in the whole run."""
    made = []

    def __init__(self, planes, table, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        self.nnz, self.perm, self.n_pairs = np.array(nnz), np.asarray(perm), n_pairs
        self.conv, self.fc = conv_layers, fc_layers
        self.calls, self.steps_done = [], 0
        Recorder.made.append(self)

    def run(self, t0, src, prm, lr, mom, losses):
        k = prm.shape[0]
        self.calls.append(dict(t0=t0, n_steps=k, src=src.numpy().copy(), prm_shape=tuple(prm.shape), lr=lr, mom=mom,
                               offset=losses.storage_offset()))
        for s in range(k):
            losses[s] = float(self.steps_done)
            self.steps_done += 1

    def nets(self):
        return self.conv, self.fc


def test_host_loop_chunks_sources_learning_rate_drop_and_init(monkeypatch, tmp_path):
    import torch
    from mc_cnn_amd import t7
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(tms, "Trainer", Recorder)
    monkeypatch.setattr(tms, "CHUNK_STEPS", 4)
    Recorder.made = []
    rng = np.random.default_rng(0)
    nnz = lambda n, first: np.stack([rng.integers(1, 6, n), rng.integers(0, 8, n), rng.integers(0, 10, n), first + np.arange(n)],
                                    1).astype(np.float32)
    data = dict(nnz_tr=nnz(N_TR, 100), nnz_te=nnz(N_TE, 200), planes=np.zeros(16, np.float32), table=np.zeros(36, tm.PLANE_DTYPE),
                index=INDEX)
    argv = ["-a", "train_tr", "-bs", "4", "-seed", "5", "-epochs", "13", "-lr", "0.004"]
    _, _, opt, _ = tms.parse(["mb", "slow"] + argv)
    fname = tms.train(opt, argv, torch.device("cpu"), data=data)
    rec, = Recorder.made
    assert [(c["t0"], c["n_steps"]) for c in rec.calls] == [(0, 4), (8, 4), (16, 2)] * 13 and tms.last_run["epochs"] == 13
    assert sorted(rec.perm.tolist()) == list(range(N_TR)) and rec.perm.dtype == np.int32 and rec.n_pairs == 2
    np.testing.assert_array_equal(rec.nnz, data["nnz_tr"])
    for e, c in enumerate(rec.calls):
        assert c["prm_shape"] == (c["n_steps"], 2, 18) and c["src"].shape == (c["n_steps"], 2, 2) and c["src"].dtype == np.int32
        assert c["lr"] == (0.004 if e < 33 else 0.004 / 10) and c["mom"] == 0.9 and c["offset"] == c["t0"] // 2
        # every pair's planes belong to the image of its nnz row, left view then right view
        img = rec.nnz[rec.perm[c["t0"]:c["t0"] + 2 * c["n_steps"]], 0].astype(np.int64).reshape(c["n_steps"], 2)
        k = c["src"].astype(np.int64) - INDEX[img - 1, 0][..., None]
        assert (k >= 0).all() and (k < (2 * INDEX[img - 1, 1] * INDEX[img - 1, 2])[..., None]).all() and (k % 2 == [0, 1]).all()
    assert opt.lr == 0.004 / 10
    np.testing.assert_array_equal(tms.last_run["losses"], np.arange(130, dtype=np.float32))
    assert fname == os.path.join("net", "net_mb_slow_-a_train_tr_-bs_4_-seed_5_-epochs_13_-lr_0.004.t7") == tms.last_run["net_fname"]
    # started from init_net(-seed), saved what the Trainer holds
    want_conv, want_fc = tms.init_net(5)
    np.testing.assert_array_equal(rec.conv[1][0], want_conv[1][0])
    got_conv, got_fc = t7.load_reference_net(fname, "slow")
    assert len(got_conv) == 5 and len(got_fc) == 4
    np.testing.assert_array_equal(got_fc[3][0], want_fc[3][0])
    # train_all adds nnz_te; -max_steps; init; fewer pairs than a batch is refused
    Recorder.made = []
    init = so.wide_nets(9)
    argv = ["-a", "train_all", "-bs", "4", "-epochs", "1", "-max_steps", "7"]
    tms.train(tms.parse(["mb", "slow"] + argv)[2], argv, torch.device("cpu"), data=data, init=init)
    rec, = Recorder.made
    np.testing.assert_array_equal(rec.nnz, np.concatenate([data["nnz_tr"], data["nnz_te"]], 0))
    assert [(c["t0"], c["n_steps"]) for c in rec.calls] == [(0, 4), (8, 3)]
    assert rec.conv is init[0] and rec.fc is init[1]
    with pytest.raises(SystemExit, match="fewer than a batch"):
        argv = ["-a", "train_tr", "-bs", "64"]
        tms.train(tms.parse(["mb", "slow"] + argv)[2], argv, torch.device("cpu"), data=data)
