"""CPU: the host side of `{kitti|kitti2015|mb} fast -l1 N` (main.lua:212-214, 240-242, 271-273): libmctraindepth.so's symbols, sizes
and argument checks, the parameter layout per depth, the flags -l1 / -fm / -ks with their routing and refusals, the order of draws
of train_depth.train, and hs.py's -l1."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libraries as L  # noqa: E402
import train_fast_oracle as do  # noqa: E402
from mc_cnn_amd import _train_depth_lib as tdl  # noqa: E402
from mc_cnn_amd import hs, train, train_depth, train_mb  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402

# include/mc_train_depth.h's table: l1 -> (patch side, parameters)
TABLE = {1: (3, 640), 2: (5, 37568), 3: (7, 74496), 4: (9, 111424), 5: (11, 148352)}
HEADER = os.path.join(ROOT, "include", "mc_train_depth.h")


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_loads_without_a_gpu_and_exports_the_headers_symbols():
    """what only libmctraindepth.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    text = open(HEADER).read()
    assert len(L.exported_abi(tdl.LIB_PATH)) == 10
    for name, value in (("MIN_L1", tdl.MIN_L1), ("MAX_L1", tdl.MAX_L1), ("FM", tdl.FM), ("NPRM", tdl.NPRM), ("MAX_PAIRS", tdl.MAX_PAIRS)):
        assert re.search(r"#define MC_TRAIN_DEPTH_%s %d\b" % (name, value), text), name
    assert (tdl.MIN_L1, tdl.MAX_L1, tdl.FM, tdl.NPRM, tdl.MAX_PAIRS, tdl.EINVAL) == (1, 5, 64, 18, 1024, -22)
    want = {"train_depth_sgd_kernel"}
    for l1 in TABLE:
        want |= {"train_depth_sample_kernel<%d>" % l1, "train_depth_mb_sample_kernel<%d>" % l1, "train_depth_mb_step_kernel<%d>" % l1,
                 "train_depth_step_kernel<%d, true>" % l1, "train_depth_step_kernel<%d, false>" % l1}
    assert L.built_kernels(tdl.LIB_PATH) == want and len(want) == 26


def test_sizes_equal_the_headers_table_and_are_zero_outside_it():
    lib = tdl.load()
    for l1, (ws, nparams) in TABLE.items():
        assert lib.mc_train_depth_ws(l1) == ws == tdl.ws_of(l1) == do.ws_of(l1)
        assert lib.mc_train_depth_nparams(l1) == nparams == tdl.nparams_of(l1) == 640 + (l1 - 1) * 36928
        for n in (1, 3, 64, 1024):
            assert lib.mc_train_depth_workspace_bytes(l1, n) == n * (nparams + 1) * 4      # a slab row and a loss per pair
        for n in (0, 1025, -1):
            assert lib.mc_train_depth_workspace_bytes(l1, n) == 0
    assert TABLE[4][1] == train.tl.NPARAMS and TABLE[5][1] == train_mb.tml.NPARAMS
    for l1 in (0, 6, -1):
        assert lib.mc_train_depth_ws(l1) == 0 and lib.mc_train_depth_nparams(l1) == 0 and lib.mc_train_depth_workspace_bytes(l1, 4) == 0


def test_argument_checks_return_einval_with_a_message_before_any_launch():
    lib = tdl.load()
    P = 1 << 20                      # never dereferenced: every check precedes the first launch
    L = 3
    need = lib.mc_train_depth_workspace_bytes(L, 4)

    def step(l1=L, patches=P, n=4, params=P, moms=P, margin=0.2, pow_=1, loss=P, ws=P, ws_bytes=need):
        return lib.mc_train_depth_step_batch(l1, patches, n, params, moms, 0.002, 0.9, margin, pow_, loss, ws, ws_bytes, None)

    def sample(l1=L, x0=P, x1=P, n_img=2, H=10, W=12, nnz=P, n_nnz=10, rows=P, prm=P, n=4, out=P):
        return lib.mc_train_depth_sample(l1, x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, n, out, None)

    def run(l1=L, x0=P, x1=P, n_img=2, H=10, W=12, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, prm=P, params=P, moms=P,
            losses=P, ws=P, ws_bytes=need):
        return lib.mc_train_depth_run(l1, x0, x1, n_img, H, W, nnz, n_nnz, perm, n_perm, t0, n_steps, n, prm, params, moms, 0.002, 0.9, 0.2,
                                      1, losses, ws, ws_bytes, None)

    def mb_sample(l1=L, planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, rows=P, src=P, prm=P, n=4, out=P):
        return lib.mc_train_depth_mb_sample(l1, planes, table, n_planes, nnz, n_nnz, rows, src, prm, n, out, None)

    def mb_run(l1=L, planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, src=P, prm=P, params=P,
               moms=P, losses=P, ws=P, ws_bytes=need):
        return lib.mc_train_depth_mb_run(l1, planes, table, n_planes, nnz, n_nnz, perm, n_perm, t0, n_steps, n, src, prm, params, moms,
                                         0.002, 0.9, 0.2, 1, losses, ws, ws_bytes, None)

    bad = []
    for name, call in (("step", step), ("sample", sample), ("run", run), ("mb_sample", mb_sample), ("mb_run", mb_run)):
        bad += [("%s: l1 %d" % (name, l1), lambda call=call, l1=l1: call(l1=l1), "l1 %d outside [1, 5]" % l1) for l1 in (0, 6, -1)]
    bad += [("n_pairs 0", lambda: step(n=0), "n_pairs"), ("n_pairs above the maximum", lambda: step(n=tdl.MAX_PAIRS + 1), "n_pairs"),
            ("null patches", lambda: step(patches=None), "null"), ("null params", lambda: step(params=None), "null"),
            ("null moms", lambda: step(moms=None), "null"), ("null loss", lambda: step(loss=None), "null"),
            ("null workspace", lambda: step(ws=None), "workspace"), ("workspace one byte short", lambda: step(ws_bytes=need - 1), "workspace"),
            ("the workspace of a shallower net", lambda: step(ws_bytes=lib.mc_train_depth_workspace_bytes(L - 1, 4)), "workspace"),
            ("pow 3", lambda: step(pow_=3), "pow"), ("margin nan", lambda: step(margin=float("nan")), "margin"),
            ("sample: null x0", lambda: sample(x0=None), "null"), ("sample: null x1", lambda: sample(x1=None), "null"),
            ("sample: null nnz", lambda: sample(nnz=None), "null"), ("sample: null rows", lambda: sample(rows=None), "null"),
            ("sample: null prm", lambda: sample(prm=None), "null"), ("sample: null out", lambda: sample(out=None), "null"),
            ("sample: n_pairs 0", lambda: sample(n=0), "n_pairs"), ("sample: H 3", lambda: sample(H=3), "image dims"),
            ("sample: W 32768", lambda: sample(W=32768), "16-bit"), ("sample: empty nnz", lambda: sample(n_nnz=0), "nnz"),
            ("run: null x0", lambda: run(x0=None), "null"), ("run: null perm", lambda: run(perm=None), "null"),
            ("run: null prm", lambda: run(prm=None), "null"), ("run: null losses", lambda: run(losses=None), "null"),
            ("run: null params", lambda: run(params=None), "null"), ("run: n_pairs 0", lambda: run(n=0), "n_pairs"),
            ("run: n_pairs above the maximum", lambda: run(n=tdl.MAX_PAIRS + 1), "n_pairs"),
            ("run: workspace one byte short", lambda: run(ws_bytes=need - 1), "workspace"),
            ("run: steps past the permutation", lambda: run(t0=93), "permutation"), ("run: negative t0", lambda: run(t0=-1), "permutation"),
            ("run: negative n_steps", lambda: run(n_steps=-1), "n_steps"), ("run: empty nnz", lambda: run(n_nnz=0), "nnz"),
            ("mb_sample: null planes", lambda: mb_sample(planes=None), "null"), ("mb_sample: null table", lambda: mb_sample(table=None), "null"),
            ("mb_sample: null src", lambda: mb_sample(src=None), "null"), ("mb_sample: null out", lambda: mb_sample(out=None), "null"),
            ("mb_sample: n_pairs 0", lambda: mb_sample(n=0), "n_pairs"), ("mb_sample: no planes", lambda: mb_sample(n_planes=0), "n_planes"),
            ("mb_sample: empty nnz", lambda: mb_sample(n_nnz=0), "nnz"),
            ("mb_run: null planes", lambda: mb_run(planes=None), "null"), ("mb_run: null table", lambda: mb_run(table=None), "null"),
            ("mb_run: null perm", lambda: mb_run(perm=None), "null"), ("mb_run: null src", lambda: mb_run(src=None), "null"),
            ("mb_run: null prm", lambda: mb_run(prm=None), "null"), ("mb_run: null losses", lambda: mb_run(losses=None), "null"),
            ("mb_run: n_pairs 0", lambda: mb_run(n=0), "n_pairs"), ("mb_run: workspace one byte short", lambda: mb_run(ws_bytes=need - 1), "workspace"),
            ("mb_run: steps past the permutation", lambda: mb_run(t0=93), "permutation"),
            ("mb_run: negative n_steps", lambda: mb_run(n_steps=-1), "n_steps")]
    for what, call, word in bad:
        rc = call()
        assert rc == tdl.EINVAL, (what, rc)
        assert word in tdl.last_error() and tdl.last_error().startswith("train_depth"), (what, tdl.last_error())
    assert step(l1=6) == tdl.EINVAL and "254464 bytes in LDS" in tdl.last_error()      # why six layers are refused
    with pytest.raises(tdl.TrainDepthError, match="n_pairs"):
        tdl.check(step(n=0), "mc_train_depth_step_batch")


# ---- the parameter layout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l1", sorted(TABLE))
def test_net_shape_round_trips_and_refuses_another_depth(l1):
    shape = train_depth.net_shape(l1)
    assert (shape.l1, shape.fm, shape.l2, shape.nh2, shape.nparams, shape.library) == (l1, 64, 0, 0, TABLE[l1][1], "libmctraindepth.so")
    layers = do.random_layers(l1, 3)
    v = shape.flat_params(layers)
    assert v.dtype == np.float32 and v.size == TABLE[l1][1]
    np.testing.assert_array_equal(v, do.flat(layers))
    np.testing.assert_array_equal(v[:576], layers[0][0].ravel())
    np.testing.assert_array_equal(v[-64:], layers[-1][1])
    back, fc = shape.unflat_params(v)
    assert fc == [] and len(back) == l1
    for (w, b), (w2, b2) in zip(layers, back):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    for other in (l1 - 1, l1 + 1):
        if other in TABLE:
            with pytest.raises(ValueError, match="libmctraindepth.so trains l1 %d" % l1):
                shape.flat_params(do.random_layers(other, 3))
    with pytest.raises(ValueError):
        shape.unflat_params(v[:-1])


def test_net_shape_is_the_old_libraries_at_their_depths_and_nothing_outside_1_to_5():
    for l1, old in ((4, train.NET), (5, train_mb.NET)):
        shape = train_depth.net_shape(l1)
        assert shape.tensor_names() == old.tensor_names() and shape.nparams == old.nparams
        layers = do.random_layers(l1, 8)
        np.testing.assert_array_equal(shape.flat_params(layers), old.flat_params(layers))
    for l1 in (0, 6):
        with pytest.raises(ValueError, match="l1 1..5"):
            train_depth.net_shape(l1)


# ---- flags and routing -------------------------------------------------------------------------------------------------------------
def test_l1_routes_training_to_train_depth():
    """Fails without the feature: -l1 is no flag there."""
    for argv, l1 in ((["kitti", "fast", "-a", "train_tr", "-l1", "3"], 3), (["mb", "fast", "-a", "train_tr", "-l1", "2"], 2),
                     (["kitti2015", "fast", "-a", "train_all", "-l1", "5"], 5), (["mb", "fast", "-a", "train_all", "-l1", "4"], 4),
                     (["kitti", "fast", "-l1", "1", "-a", "train_tr"], 1)):
        mod, trainer, dataset, arch, opt, prm = mcmain.route(argv)
        assert trainer is train_depth and (dataset, arch, opt.l1, opt.fm, opt.ks) == (argv[0], "fast", l1, 64, 3), argv
        assert mod is (train_mb if dataset == "mb" else None)          # whose parse and evaluate still apply
        assert train_depth.net_fname_of(dataset, arch, argv[2:]).endswith("_".join(argv[2:]) + ".t7") and "-l1_%d" % l1 in \
            train_depth.net_fname_of(dataset, arch, argv[2:])


def test_the_default_depth_keeps_todays_route():
    for dataset, default, want_mod, want_trainer in (("kitti", 4, None, train), ("kitti2015", 4, None, train), ("mb", 5, train_mb, train_mb)):
        for extra in ([], ["-l1", str(default)], ["-l1", str(default), "-fm", "64", "-ks", "3"]):
            argv = [dataset, "fast", "-a", "train_tr"] + extra
            mod, trainer, _, _, opt, _ = mcmain.route(argv)
            assert mod is want_mod and trainer is want_trainer and (opt.l1, opt.fm, opt.ks) == (default, 64, 3), argv
            # the file name gains the flag only where it is written (main.lua's cmd_str)
            assert ("-l1" in train.net_fname_of(dataset, "fast", argv[2:])) == bool(extra)
    from mc_cnn_amd import train_mb_slow, train_slow
    assert mcmain.route(["kitti", "slow", "-a", "train_tr"])[:2] == (train_slow, train_slow)
    assert mcmain.route(["mb", "slow", "-a", "train_tr"])[:2] == (train_mb_slow, train_mb_slow)
    mod, trainer, _, _, opt, _ = mcmain.route(["kitti", "fast", "-a", "predict", "-l1", "2"])
    assert mod is None and trainer is None and opt.l1 == 2


def test_l1_and_the_cross_arm_length_are_two_flags():
    for parse, head in ((mcmain.parse, ["kitti", "fast"]), (train_mb.parse, ["mb", "fast"])):
        _, _, opt, prm = parse(head + ["-a", "train_tr", "-l1", "3", "-L1", "5"])
        assert opt.l1 == 3 and opt.L1 == 5 and prm["L1"] == 5 and "l1" not in prm
        _, _, opt, prm = parse(head + ["-a", "train_tr", "-L1", "7"])
        assert opt.l1 == mcmain.NET_SHAPES[(head[0], "fast")][0] and opt.L1 == 7


@pytest.mark.parametrize("argv, words", [
    (["kitti", "fast", "-a", "train_tr", "-l1", "6"], ("-l1 6", "l1 1..5")),
    (["kitti", "fast", "-a", "train_tr", "-l1", "0"], ("-l1 0", "l1 1..5")),
    (["mb", "fast", "-a", "train_tr", "-l1", "6"], ("-l1 6", "l1 1..5")),
    (["kitti", "fast", "-a", "predict", "-l1", "7"], ("-l1 7", "l1 1..5")),
    (["kitti", "fast", "-a", "train_tr", "-fm", "96"], ("-fm 96", "only -fm 64", "-l1 1..5")),
    (["mb", "fast", "-a", "train_tr", "-fm", "80"], ("-fm 80", "only -fm 64")),
    (["kitti2015", "fast", "-a", "train_tr", "-ks", "5"], ("-ks 5", "only -ks 3", "-l1 1..5")),
    (["mb", "fast", "-a", "test_te", "-ks", "2"], ("-ks 2", "only -ks 3")),
    (["kitti", "slow", "-a", "train_tr", "-l1", "3"], ("-l1", "arch slow", "GEMM family", "{kitti|kitti2015|mb} fast")),
    (["kitti", "slow", "-a", "predict", "-fm", "64"], ("-fm", "arch slow")),
    (["mb", "slow", "-a", "train_tr", "-ks", "3"], ("-ks", "arch slow")),
    (["kitti", "ad", "-a", "predict", "-l1", "4"], ("-l1", "arch ad", "no net")),
    (["mb", "census", "-a", "predict", "-fm", "64"], ("-fm", "arch census", "no net"))])
def test_what_the_kernels_do_not_serve_is_refused_naming_what_is_supported(argv, words):
    with pytest.raises(SystemExit) as e:
        mcmain.route(argv)
    for word in words:
        assert word in str(e.value), (word, str(e.value))


def test_load_net_takes_the_depth_for_random_and_npz_nets(tmp_path):
    _, _, opt, _ = mcmain.parse(["kitti", "fast", "-a", "predict", "-l1", "2"])
    layers = mcmain.load_net("random:7", "kitti", "fast", l1=opt.l1)
    assert [w.shape for w, _ in layers] == [(64, 1, 3, 3), (64, 64, 3, 3)] and [b.shape for _, b in layers] == [(64,), (64,)]
    assert np.abs(layers[0][0]).max() <= 1 / 3 and np.abs(layers[1][0]).max() <= 1 / 24      # nn.SpatialConvolution:reset's bounds
    # the first layers of a seed are the same draws at every depth, and the default is the data set's
    for (w, b), (w4, b4) in zip(layers, mcmain.load_net("random:7", "kitti", "fast")):
        np.testing.assert_array_equal(w, w4)
        np.testing.assert_array_equal(b, b4)
    assert len(mcmain.load_net("random:7", "kitti", "fast")) == 4 and len(mcmain.load_net("random:7", "mb", "fast")) == 5
    np.savez(str(tmp_path / "n.npz"), **{"%s%d" % (k, i + 1): a for i, wb in enumerate(do.random_layers(3, 1)) for k, a in zip("wb", wb)})
    assert len(mcmain.load_net(str(tmp_path / "n.npz"), "mb", "fast", l1=3)) == 3
    with pytest.raises(KeyError):
        mcmain.load_net(str(tmp_path / "n.npz"), "kitti", "fast")          # without the flag: four layers are looked for


# ---- the order of draws ----------------------------------------------------------------------------------------------------------
N_TR, N_TE = 21, 5      # bs 4 (2 pairs per step): `for t = 1, 21 - 2, 2` is a 10-step epoch
INDEX = np.array([[0, 2, 2], [8, 1, 1], [10, 3, 3], [28, 2, 1], [32, 1, 2]], np.int64)   # (first plane, lights, exposures) of 5 images


def recorder(mb):
    class Recorder:
        """Stands in for a Trainer: keeps the permutation and net it is given and every prm (and src) passed to run()."""
        made = []

        def __init__(self, store0, store1, nnz, perm, layers, n_pairs, device):
            self.perm, self.net, self.prm, self.src = np.array(perm), layers, [], []
            Recorder.made.append(self)

        def run(self, t0, *args):
            if mb:
                self.src.append(args[0].numpy().copy())
            self.prm.append(args[1 if mb else 0].numpy().copy())
            args[-1][:args[1 if mb else 0].shape[0]] = 0.5

        def layers(self):
            return self.net
    return Recorder


def nnz_rows(rng, n, first, n_img):
    return np.stack([rng.integers(1, n_img + 1, n), rng.integers(0, 8, n), rng.integers(0, 10, n), first + np.arange(n)], 1).astype(np.float32)


@pytest.mark.parametrize("dataset", ["kitti", "mb"])
def test_a_seed_draws_the_same_pixels_and_augmentations_at_every_depth(dataset, monkeypatch, tmp_path):
    """train_depth.train at l1 = 2 hands its Trainer the arrays that train.train / train_mb.train hand theirs for the same -seed:
    the same Generator draws in the same order (permutation, each chunk's parameters, on Middlebury its sources)."""
    import torch
    mb = dataset == "mb"
    old = train_mb if mb else train
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    data = dict(nnz_tr=nnz_rows(rng, N_TR, 100, 5 if mb else 2), nnz_te=nnz_rows(rng, N_TE, 200, 5 if mb else 2))
    if mb:
        data.update(planes=np.zeros(16, np.float32), table=np.zeros(36, train_mb.PLANE_DTYPE), index=INDEX)
    argv = ["-a", "train_tr", "-bs", "4", "-seed", "5", "-epochs", "2"]
    if not mb:                                            # KITTI: through the loader, from a data.kitti directory
        from mc_cnn_amd import binio
        x = rng.standard_normal((2, 1, 12, 16)).astype(np.float32)
        data.update(x0=x, x1=x[..., ::-1].copy(), metadata=np.array([[12, 16, 0], [12, 16, 1]], np.int32), tr=np.array([1], np.int32),
                    te=np.array([2], np.int32))
        os.makedirs("d")
        for k, a in data.items():
            binio.tofile(os.path.join("d", k + ".bin"), a)
        argv, data = argv + ["-data_dir", "d"], None
    dev = torch.device("cpu")
    recs = {}
    for mod, attr, extra in ((old, "Trainer", []), (train_depth, "MbTrainer" if mb else "Trainer", ["-l1", "2"])):
        Recorder = recorder(mb)
        monkeypatch.setattr(mod, attr, Recorder)
        monkeypatch.setattr(mod, "CHUNK_STEPS", 4)
        _, trainer, _, _, opt, _ = mcmain.route([dataset, "fast"] + argv + extra)
        assert trainer is mod
        lead = () if mod is train_mb else (dataset, "fast")
        fname = mod.train(*lead, opt, argv + extra, dev, data=data)
        recs[mod], = Recorder.made
        assert mod.last_run["epochs"] == 2 and mod.last_run["losses"].size == 20 and os.path.exists(fname)
    a, b = recs[old], recs[train_depth]
    np.testing.assert_array_equal(a.perm, b.perm)
    np.testing.assert_array_equal(a.perm, np.random.default_rng(5).permutation(N_TR))
    assert len(a.prm) == len(b.prm) == 6 and len(a.src) == len(b.src) == (6 if mb else 0) and a.prm[0].shape == (4, 2, 18)
    for x, y in zip(a.prm + a.src, b.prm + b.src):
        np.testing.assert_array_equal(x, y)
    # the initial net is load_net("random:<seed>") with l1 layers, and the saved one has them
    want = mcmain.load_net("random:5", dataset, "fast", l1=2)
    assert len(b.net) == 2 and len(a.net) == (5 if mb else 4)
    for (w, bias), (w2, bias2) in zip(b.net, want):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(bias, bias2)
    saved = mcmain.load_net(train_depth.last_run["net_fname"], dataset, "fast")
    assert [w.shape for w, _ in saved] == [(64, 1, 3, 3), (64, 64, 3, 3)] and "-l1_2" in train_depth.last_run["net_fname"]


# ---- hs.py -------------------------------------------------------------------------------------------------------------------------
def test_hs_takes_the_depth_of_a_trained_net(tmp_path):
    _, _, opt, _ = mcmain.parse(["kitti", "fast", "-a", "train_tr", "-l1", "3"])
    layers = do.random_layers(3, 2)
    path = train.save_net(str(tmp_path / "net3.t7"), layers, opt)
    o = hs.parse(["random", "kitti", "fast", "test_te", path, "-l1", "3"])
    assert o.l1 == 3
    got, fc = hs.check_net(path, "kitti", "fast", o.l1)
    assert fc is None and len(got) == 3
    for (w, b), (w2, b2) in zip(layers, got):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    assert hs.parse(["random", "kitti", "fast", "test_te", path]).l1 is None
    with pytest.raises(SystemExit, match="does not fit kitti fast"):
        hs.check_net(path, "kitti", "fast")                    # without the flag the check is the data set's four layers
    with pytest.raises(SystemExit, match="does not fit kitti fast"):
        hs.check_net(path, "kitti", "fast", 2)
    for argv in (["random", "kitti", "fast", "test_te", path, "-l1", "6"], ["random", "kitti", "slow", "test_te", path, "-l1", "4"]):
        with pytest.raises(SystemExit, match="-l1 1..5"):
            hs.parse(argv)
    for action in ("train_tr", "da"):
        with pytest.raises(SystemExit) as e:
            hs.parse(["random", "kitti", "fast", action, path])
        assert "only test_te" in str(e.value) and "fm 64 only" in str(e.value) and "-l1 1..5" in str(e.value)
