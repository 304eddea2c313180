"""CPU: the host side of `{kitti|kitti2015} slow -a train_tr | train_all | test_te | test_all` (main.lua:663-677, 753-875):
flags, the flat parameter layout and the saved net, the criterion's oracle, libmctrainslow.so's symbols, argument checks
and kernel inventory, and the host loop of `train_slow.train` with a recording stand-in for its Trainer."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libraries as L  # noqa: E402
import train_slow_oracle as so  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402
from mc_cnn_amd import train_slow as ts  # noqa: E402


# ---- parse ------------------------------------------------------------------------------------------------------------
def test_parse_defaults_are_main_luas_for_arch_slow():
    for a in ("train_tr", "train_all", "test_te", "test_all"):
        for ds in ("kitti", "kitti2015"):
            dataset, arch, opt, prm = ts.parse([ds, "slow", "-a", a])
            assert (dataset, arch, opt.a) == (ds, "slow", a)
    _, _, opt, prm = ts.parse(["kitti", "slow", "-a", "train_tr"])
    want = dict(seed=42, lr=0.003, mom=0.9, bs=128, true1=1, false1=4, false2=10, rotate=7, hscale=0.9, scale=1, trans=0,
                hshear=0.1, brightness=0.7, contrast=1.3, d_vtrans=0, d_rotate=0, d_hscale=1, d_hshear=0, d_brightness=0.3,
                d_contrast=1, hflip=0, vflip=0, epochs=14, max_steps=0, disp_max=228, at=0, data_dir="", gpu=1)
    for k, v in want.items():
        assert getattr(opt, k) == v, k
    assert not hasattr(opt, "m") and not hasattr(opt, "pow")
    # the hyper-parameters of main.lua:86-99, as main.parse builds them for -a predict
    _, _, _, want_prm = mcmain.parse(["kitti", "slow", "-a", "predict"])
    assert prm == want_prm and prm["L1"] == 5 and prm["cbca_i2"] == 0
    assert ts.parse(["kitti2015", "slow", "-a", "test_te"])[3] == mcmain.parse(["kitti2015", "slow", "-a", "predict"])[3]


def test_parse_overrides():
    _, _, opt, prm = ts.parse(["kitti2015", "slow", "-a", "train_all", "-seed", "7", "-lr", "0.01", "-bs", "64", "-hflip", "1",
                               "-d_contrast", "1.2", "-max_steps", "5", "-epochs", "2", "-data_dir", "d", "-L1", "9", "-pi1", "2.5",
                               "-net_fname", "x.t7", "-disp_max", "70"])
    assert (opt.seed, opt.lr, opt.bs, opt.hflip, opt.d_contrast, opt.max_steps, opt.epochs, opt.data_dir, opt.net_fname, opt.disp_max) == \
        (7, 0.01, 64, 1, 1.2, 5, 2, "d", "x.t7", 70)
    assert prm["L1"] == 9 and prm["pi1"] == 2.5
    assert ts.parse(["kitti", "slow", "-a", "train_tr", "-at", "1"])[2].at == 1


@pytest.mark.parametrize("argv", [["kitti", "slow", "-a", "train_tr", "-at", "1", "-data_dir", "d"],
                                  ["mb", "slow", "-a", "train_tr"], ["kitti", "slow", "-a", "submit"],
                                  ["kitti", "fast", "-a", "train_tr"], ["kitti", "slow", "-a", "train_tr", "-m", "0.2"],
                                  ["kitti", "slow", "-a", "train_tr", "-subset", "0.5"], ["kitti", "slow", "-a", "train_tr", "-debug"],
                                  ["kitti", "slow", "-a", "train_tr", "-bs", "7"]])
def test_parse_refuses_what_is_out_of_scope(argv):
    with pytest.raises(SystemExit):
        ts.parse(argv)


def test_main_routes_only_slow_training_and_main_parse_keeps_refusing():
    from mc_cnn_amd import train_mb_slow
    route = mcmain.training_module
    assert route(["kitti", "slow", "-a", "train_tr"]) is ts and route(["kitti2015", "slow", "-seed", "3", "-a", "test_all"]) is ts
    assert route(["mb", "slow", "-a", "train_tr"]) is train_mb_slow          # not train_slow's: Middlebury's own accurate net
    for argv in (["kitti", "slow", "-a", "submit"], ["kitti", "slow", "-a", "predict"], ["kitti", "fast", "-a", "train_tr"],
                 ["kitti", "slow"], ["kitti", "slow", "-a"]):
        assert route(argv) is None, argv
    for argv in (["mb", "slow", "-a", "train_tr"], ["kitti", "slow", "-a", "submit"], ["kitti", "slow", "-a", "train_tr"]):
        with pytest.raises(SystemExit, match="fast only"):
            mcmain.parse(argv)


# ---- parameters and the saved net ----------------------------------------------------------------------------------------
def test_flat_params_round_trip_and_layout():
    conv, fc = ts.init_net(3)
    assert [w.shape for w, _ in conv] == so.CONV_SHAPES and [w.shape for w, _ in fc] == so.FC_SHAPES
    for layers in (conv, fc):      # the ranges of the two reset()s
        for w, b in layers:
            bound = 1 / np.sqrt(np.prod(w.shape[1:]))
            assert np.abs(w).max() <= bound and np.abs(b).max() <= bound and np.abs(w).max() > 0.9 * bound
    v = ts.flat_params(conv, fc)
    assert v.size == 870449 == ts.tsl.NPARAMS and v.dtype == np.float32
    np.testing.assert_array_equal(v, so.flat(conv, fc))
    assert sum(n for _, n in ts.tensor_names()) == 870449 and [n for n, _ in ts.tensor_names()] == so.NAMES
    np.testing.assert_array_equal(v[:1008], conv[0][0].ravel())
    np.testing.assert_array_equal(v[340144:340144 + 384 * 224], fc[0][0].ravel())
    assert v[-1] == fc[4][1][0]
    conv2, fc2 = ts.unflat_params(v)
    for a, b in zip(conv + fc, conv2 + fc2):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    with pytest.raises(ValueError):
        ts.flat_params(conv[:3], fc)
    with pytest.raises(ValueError):
        ts.unflat_params(v[:-1])


def test_saved_net_round_trips_into_the_readers(tmp_path):
    from mc_cnn_amd import t7
    conv, fc = ts.init_net(5)
    argv = ["-a", "train_tr", "-seed", "5"]
    _, _, opt, _ = ts.parse(["kitti", "slow"] + argv)
    fname = ts.net_fname_of("kitti", "slow", argv)
    assert fname == os.path.join("net", "net_kitti_slow_-a_train_tr_-seed_5.t7")     # main.lua:344-347, 594
    path = ts.save_net(str(tmp_path / fname), conv, fc, opt)
    got_conv, got_fc = t7.load_reference_net(path, "slow")
    assert len(got_conv) == 4 and len(got_fc) == 5
    for want, got in ((conv, got_conv), (fc, got_fc), (conv, mcmain.load_net(path, "kitti", "slow")), (fc, mcmain.load_fc(path, "kitti"))):
        assert len(want) == len(got)
        for (w, b), (w2, b2) in zip(want, got):
            assert w2.shape == w.shape and b2.shape == b.shape
            np.testing.assert_array_equal(w, w2)
            np.testing.assert_array_equal(b, b2)
    obj = t7.load(path)
    assert obj[3]["seed"] == 5 and obj[3]["a"] == "train_tr" and obj[3]["lr"] == 0.003
    assert [m.cls for m in t7._modules(obj[1])] == ["cudnn.SpatialConvolution", "cudnn.ReLU"] * 4
    assert all(m["padW"] == 1 and m["padH"] == 1 for m in t7._modules(obj[1])[::2])
    mods2 = t7._modules(obj[2])
    assert [m.cls for m in mods2] == ["nn.SpatialConvolution1_fw", "cudnn.ReLU"] * 4 + ["nn.SpatialConvolution1_fw", "cudnn.Sigmoid"]
    assert np.asarray(mods2[0]["bias"]).shape == (1, 384, 1, 1) and np.asarray(mods2[8]["weight"]).shape == (1, 384)


# ---- the criterion's oracle ---------------------------------------------------------------------------------------------
def test_restated_criterion_gradient_is_autograds_away_from_saturation():
    import torch
    rng = np.random.default_rng(2)
    z = torch.tensor(rng.uniform(-10, 10, 400), requires_grad=True)
    t = so.targets(200)
    o = torch.sigmoid(z)
    o.retain_grad()
    loss = so.bce2(o, t)
    loss.backward()
    want = -(t * torch.log(o + 1e-12) + (1 - t) * torch.log(1 - o + 1e-12)).mean()
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-12
    got = so.bce2_grad(o.detach(), t)
    assert (got - o.grad).abs().max() <= 1e-12 * max(1.0, float(o.grad.abs().max()))
    # through the Sigmoid the gradient is (o - t) / n where nothing saturates, but for eps: relative eps / min(o, 1 - o)
    # = 1e-12 / 4.5e-5 at |logit| 10, of at most 1 / n = 2.5e-3
    np.testing.assert_allclose((got * o.detach() * (1 - o.detach())).numpy(), ((o.detach() - t) / 400).numpy(), rtol=0, atol=1e-10)
    # at saturation (o == 1 exactly) the reference's form gives 0 after the Sigmoid, (o - t) / n does not
    one = torch.ones(2, dtype=torch.float64)
    assert (so.bce2_grad(one, so.targets(1)) * one * (1 - one)).abs().max() == 0
    assert abs(float(so.bce2(one, so.targets(1))) + np.log(1e-12) / 2) <= 1e-9


def test_oracle_forward_pairs_left_with_positive_then_negative():
    import torch
    conv, fc = so.wide_nets(1)
    rng = np.random.default_rng(0)
    p = torch.tensor(rng.standard_normal((3, 3, 9, 9)))
    o = so.forward(so.as_f64(conv), so.as_f64(fc), p)
    assert o.shape == (6,)
    swapped = p.clone()
    swapped[:, 1], swapped[:, 2] = p[:, 2], p[:, 1]
    o2 = so.forward(so.as_f64(conv), so.as_f64(fc), swapped)
    np.testing.assert_allclose(o2.numpy().reshape(3, 2), o.numpy().reshape(3, 2)[:, ::-1], rtol=1e-12)
    frag = so.fragile(conv, fc, p.numpy())
    assert frag.shape == (3,) and frag.dtype == bool
    assert so.fragile(conv, fc, p.numpy(), eps=1e3).all()


# ---- the library -------------------------------------------------------------------------------------------------------
def test_library_loads_without_a_gpu_and_exports_the_headers_symbols():
    """what only libmctrainslow.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    assert ts.tsl.load().mc_train_slow_version() == 1
    text = open(os.path.join(ROOT, "include", "mc_train_slow.h")).read()
    for name, value in (("NPARAMS", ts.tsl.NPARAMS), ("NCONV", ts.tsl.NCONV), ("NFC", ts.tsl.NFC), ("MAX_PAIRS", ts.tsl.MAX_PAIRS),
                        ("FM", ts.tsl.FM), ("NH2", ts.tsl.NH2), ("NPRM", ts.tsl.NPRM), ("ABI_VERSION", ts.tsl.ABI_VERSION)):
        assert re.search(r"#define MC_TRAIN_SLOW_%s %d\b" % (name, value), text), name
    assert ts.tsl.MAX_PAIRS >= 256


def test_workspace_bytes():
    lib = ts.tsl.load()
    wb = lib.mc_train_slow_workspace_bytes
    assert wb(0) == 0 and wb(-1) == 0 and wb(ts.tsl.MAX_PAIRS + 1) == 0
    sizes = [wb(n) for n in (1, 2, 3, 64, 65, ts.tsl.MAX_PAIRS)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    # at least the per-pair slab of the convolutions' gradients and the FC parameters' gradient
    assert wb(64) >= 4 * (64 * ts.tsl.NCONV + ts.tsl.NFC)
    assert wb(ts.tsl.MAX_PAIRS) < 2 ** 31


def test_argument_checks_return_einval_with_a_message_before_any_launch():
    lib = ts.tsl.load()
    P = 1 << 20                      # never dereferenced: every check precedes the first launch
    need = lib.mc_train_slow_workspace_bytes(4)

    def step(patches=P, n=4, params=P, moms=P, loss=P, ws=P, ws_bytes=need):
        return lib.mc_train_slow_step_batch(patches, n, params, moms, 0.003, 0.9, loss, ws, ws_bytes, None)

    def run(x0=P, x1=P, n_img=1, H=20, W=30, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, prm=P, params=P, moms=P,
            losses=P, ws=P, ws_bytes=need):
        return lib.mc_train_slow_run(x0, x1, n_img, H, W, nnz, n_nnz, perm, n_perm, t0, n_steps, n, prm, params, moms, 0.003, 0.9,
                                     losses, ws, ws_bytes, None)

    bad = [("n_pairs 0", lambda: step(n=0), "n_pairs"), ("n_pairs above the maximum", lambda: step(n=ts.tsl.MAX_PAIRS + 1), "n_pairs"),
           ("null patches", lambda: step(patches=None), "null"), ("null params", lambda: step(params=None), "null"),
           ("null moms", lambda: step(moms=None), "null"), ("null loss", lambda: step(loss=None), "null"),
           ("null workspace", lambda: step(ws=None), "workspace"), ("workspace one byte short", lambda: step(ws_bytes=need - 1), "workspace"),
           ("misaligned params", lambda: step(params=P + 4), "aligned"), ("misaligned workspace", lambda: step(ws=P + 4), "aligned"),
           ("run: null x0", lambda: run(x0=None), "null"), ("run: null nnz", lambda: run(nnz=None), "null"),
           ("run: null perm", lambda: run(perm=None), "null"), ("run: null prm", lambda: run(prm=None), "null"),
           ("run: null losses", lambda: run(losses=None), "null"), ("run: n_pairs 0", lambda: run(n=0), "n_pairs"),
           ("run: workspace one byte short", lambda: run(ws_bytes=need - 1), "workspace"),
           ("run: steps past the permutation", lambda: run(t0=93), "permutation"), ("run: negative t0", lambda: run(t0=-1), "permutation"),
           ("run: negative n_steps", lambda: run(n_steps=-1), "n_steps"), ("run: tiny image", lambda: run(H=3), "dims"),
           ("run: empty nnz", lambda: run(n_nnz=0), "nnz")]
    for what, call, word in bad:
        rc = call()
        assert rc == ts.tsl.EINVAL, (what, rc)
        assert word in ts.tsl.last_error(), (what, ts.tsl.last_error())
    with pytest.raises(ts.tsl.TrainSlowError, match="n_pairs"):
        ts.tsl.check(step(n=0), "mc_train_slow_step_batch")


def test_the_library_has_no_sampler_kernel_of_its_own():
    from mc_cnn_amd import _train_lib
    assert "train_sample_kernel" in L.built_kernels(_train_lib.LIB_PATH)
    assert not any("sample_kernel" in k for k in L.built_kernels(ts.tsl.LIB_PATH))


# ---- the host loop -------------------------------------------------------------------------------------------------------
N_TR, N_TE = 21, 5      # bs 4 (2 pairs per step): `for t = 1, 21 - 2, 2` is a 10-step epoch


class Recorder:
    """Stands in for train_slow.Trainer: stores the constructor's arguments and every run() call; a step's loss is its
    index in the whole run."""
    made = []

    def __init__(self, x0, x1, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        self.nnz, self.perm, self.n_pairs = np.array(nnz), perm, n_pairs
        self.conv, self.fc = conv_layers, fc_layers
        self.calls, self.steps_done = [], 0
        Recorder.made.append(self)

    def run(self, t0, prm, lr, mom, losses):
        k = prm.shape[0]
        self.calls.append(dict(t0=t0, n_steps=k, prm_shape=tuple(prm.shape), lr=lr, mom=mom, offset=losses.storage_offset(),
                               room=losses.shape[0], perm=self.perm))
        for s in range(k):
            losses[s] = float(self.steps_done)
            self.steps_done += 1

    def nets(self):
        return self.conv, self.fc


def _data(rng):
    nnz = lambda n, first: np.stack([rng.integers(1, 3, n), rng.integers(0, 12, n), rng.integers(0, 16, n),
                                     first + np.arange(n)], 1).astype(np.float32)
    x = rng.standard_normal((2, 1, 12, 16)).astype(np.float32)
    return dict(x0=x, x1=x[..., ::-1].copy(), nnz_tr=nnz(N_TR, 100), nnz_te=nnz(N_TE, 200))


def _train(monkeypatch, tmp_path, extra, a="train_tr", init=None):
    import torch
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(ts, "Trainer", Recorder)
    monkeypatch.setattr(ts, "CHUNK_STEPS", 4)
    Recorder.made = []
    argv = ["-a", a, "-bs", "4", "-seed", "5"] + extra
    _, _, opt, _ = ts.parse(["kitti", "slow"] + argv)
    data = _data(np.random.default_rng(0))
    fname = ts.train("kitti", opt, argv, torch.device("cpu"), data=data, init=init)
    assert len(Recorder.made) == 1
    return Recorder.made[0], ts.last_run, opt, data, fname


def _epochs(calls):
    out = []
    for c in calls:
        if c["t0"] == 0:
            out.append([])
        out[-1].append(c)
    return out


def test_host_loop_chunks_permutation_and_learning_rate_drop(monkeypatch, tmp_path):
    from mc_cnn_amd import t7
    rec, run, opt, data, fname = _train(monkeypatch, tmp_path, ["-epochs", "13", "-lr", "0.004"])
    eps = _epochs(rec.calls)
    assert len(eps) == 13 and run["epochs"] == 13
    for e, calls in enumerate(eps, 1):
        assert [(c["t0"], c["n_steps"]) for c in calls] == [(0, 4), (8, 4), (16, 2)], e
        for c, s0 in zip(calls, (0, 4, 8)):
            assert c["offset"] == s0 and c["room"] == 10 - s0
            assert c["prm_shape"] == (c["n_steps"], 2, 18) and c["perm"] is rec.perm
            assert c["lr"] == (0.004 if e < 12 else 0.004 / 10) and c["mom"] == 0.9
    assert opt.lr == 0.004 / 10
    perm = np.asarray(rec.perm)
    assert perm.dtype == np.int32 and sorted(perm.tolist()) == list(range(N_TR)) and not np.array_equal(perm, np.arange(N_TR))
    assert rec.n_pairs == 2
    np.testing.assert_array_equal(rec.nnz, data["nnz_tr"])
    np.testing.assert_array_equal(run["losses"], np.arange(130, dtype=np.float32))
    assert os.path.exists(fname) and run["net_fname"] == fname
    assert fname == os.path.join("net", "net_kitti_slow_-a_train_tr_-bs_4_-seed_5_-epochs_13_-lr_0.004.t7")
    # started from init_net(-seed), saved what the Trainer holds
    want_conv, want_fc = ts.init_net(5)
    np.testing.assert_array_equal(rec.conv[1][0], want_conv[1][0])
    got_conv, got_fc = t7.load_reference_net(fname, "slow")
    np.testing.assert_array_equal(got_fc[4][0], want_fc[4][0])


def test_host_loop_max_steps_train_all_and_init(monkeypatch, tmp_path):
    rec, run, opt, _, _ = _train(monkeypatch, tmp_path, ["-epochs", "13", "-max_steps", "23"])
    assert [[(c["t0"], c["n_steps"]) for c in calls] for calls in _epochs(rec.calls)] == [[(0, 4), (8, 4), (16, 2)]] * 2 + [[(0, 3)]]
    assert run["epochs"] == 3 and all(c["lr"] == opt.lr == 0.003 for c in rec.calls)
    np.testing.assert_array_equal(run["losses"], np.arange(23, dtype=np.float32))
    rec, run, _, _, _ = _train(monkeypatch, tmp_path, ["-epochs", "13", "-max_steps", "20"])
    assert run["epochs"] == 2 and len(_epochs(rec.calls)) == 2
    init = so.wide_nets(9)
    rec, run, _, data, _ = _train(monkeypatch, tmp_path, ["-epochs", "1"], a="train_all", init=init)
    np.testing.assert_array_equal(rec.nnz, np.concatenate([data["nnz_tr"], data["nnz_te"]], 0))
    assert sorted(np.asarray(rec.perm).tolist()) == list(range(N_TR + N_TE))
    assert [(c["t0"], c["n_steps"]) for c in rec.calls] == [(0, 4), (8, 4), (16, 4)] and run["losses"].size == 12
    assert rec.conv is init[0] and rec.fc is init[1]
    with pytest.raises(SystemExit, match="fewer than a batch"):
        _train(monkeypatch, tmp_path, ["-bs", "64"])
