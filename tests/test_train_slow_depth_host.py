"""CPU: the host side of `{kitti|kitti2015|mb} slow -l2 N` (main.lua:73-78, 120-124, 663-695): libmctrainslowdepth.so's symbols,
sizes and argument checks, the parameter layout per depth, the flags -l2 / -nh2 with their routing and refusals, the order of draws
of train_slow_depth.train, load_fc's and hs.py's -l2, and the depth a saved .t7 carries."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libraries as L  # noqa: E402
import train_slow_oracle as so  # noqa: E402
from mc_cnn_amd import _train_slow_depth_lib as tsdl  # noqa: E402
from mc_cnn_amd import hs, train_mb, train_mb_slow, train_slow, train_slow_depth  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402

HEADER = os.path.join(ROOT, "include", "mc_train_slow_depth.h")
NCONV = {tsdl.KITTI: 340144, tsdl.MB: 453152}
ORACLE = {tsdl.KITTI: lambda l2: so.Net(9, 4, l2), tsdl.MB: lambda l2: so.Net(11, 5, l2)}
DEPTHS = range(1, 8)


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_library_loads_without_a_gpu_and_exports_the_headers_symbols():
    """what only libmctrainslowdepth.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    text = open(HEADER).read()
    assert len(L.exported_abi(tsdl.LIB_PATH)) == 7
    for name, value in (("KITTI", tsdl.KITTI), ("MB", tsdl.MB), ("MIN_L2", tsdl.MIN_L2), ("MAX_L2", tsdl.MAX_L2), ("NH2", tsdl.NH2), ("NPRM", tsdl.NPRM),
                        ("NFC1", tsdl.NFC1), ("NFC_STEP", tsdl.NFC_STEP), ("MAX_PAIRS", tsdl.MAX_PAIRS[tsdl.KITTI]),
                        ("MB_MAX_PAIRS", tsdl.MAX_PAIRS[tsdl.MB])):
        assert re.search(r"#define MC_TRAIN_SLOW_DEPTH_%s %d\b" % (name, value), text), name
    assert (tsdl.MIN_L2, tsdl.MAX_L2, tsdl.NH2, tsdl.NPRM, tsdl.EINVAL) == (1, 7, 384, 18, -22)
    assert tsdl.MAX_PAIRS == {tsdl.KITTI: train_slow.tsl.MAX_PAIRS, tsdl.MB: train_mb_slow.tmsl.MAX_PAIRS} == {0: 1024, 1: 256}
    # train_slow_fc.h's four, the towers once per tower, never once per l2, and one update kernel
    want = L.SHARED_KERNELS | {"depth_tower_forward_kernel<true>", "depth_tower_forward_kernel<false>", "depth_mb_tower_forward_kernel<true>",
                               "depth_mb_tower_forward_kernel<false>", "depth_tower_backward_kernel<KittiTower>",
                               "depth_tower_backward_kernel<MbTower>", "train_slow_depth_sgd_kernel"}
    assert L.built_kernels(tsdl.LIB_PATH) == want and len(want) == 11


def test_sizes_equal_the_headers_table_and_the_parents_constants():
    lib = tsdl.load()
    text = open(HEADER).read()
    for store in (tsdl.KITTI, tsdl.MB):
        for l2 in DEPTHS:
            nfc = 86785 + (l2 - 1) * 147840
            want = NCONV[store] + nfc
            net = ORACLE[store](l2)
            assert lib.mc_train_slow_depth_nparams(store, l2) == want == tsdl.nparams_of(store, l2) == net.NPARAMS and net.NCONV == NCONV[store]
            assert tsdl.nfc_of(l2) == nfc
            row = re.search(r"^ \*\s+%d\s+([\d ]+?)\s{2,}([\d ]+?)\s{2,}([\d ]+?)\s{2,}(\d+)\s*$" % l2, text, re.M)      # the header prints the table
            assert [int(g.replace(" ", "")) for g in row.groups()] == [nfc, NCONV[tsdl.KITTI] + nfc, NCONV[tsdl.MB] + nfc, 2 * l2 + 4]
            top = tsdl.MAX_PAIRS[store]
            sizes = [lib.mc_train_slow_depth_workspace_bytes(store, l2, n) for n in (1, 3, 64, top)]
            assert all(s > 0 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
            for n in (0, top + 1, -1):
                assert lib.mc_train_slow_depth_workspace_bytes(store, l2, n) == 0
            if l2 > 1:      # one more hidden Linear: 2 n rows of 384 activations (64-float granules) and its 147 840 gradients
                more = lib.mc_train_slow_depth_workspace_bytes(store, l2, 3) - lib.mc_train_slow_depth_workspace_bytes(store, l2 - 1, 3)
                assert more == 4 * (6 * 384 + 147840)
    assert lib.mc_train_slow_depth_nparams(tsdl.KITTI, 1) == 426929
    assert lib.mc_train_slow_depth_nparams(tsdl.KITTI, 4) == 870449 == train_slow.tsl.NPARAMS
    assert lib.mc_train_slow_depth_nparams(tsdl.MB, 3) == 835617 == train_mb_slow.tmsl.NPARAMS
    # at the parents' depths the workspace is the parents'
    for n in (1, 5, 64, 256):
        assert lib.mc_train_slow_depth_workspace_bytes(tsdl.KITTI, 4, n) == train_slow.tsl.load().mc_train_slow_workspace_bytes(n)
        assert lib.mc_train_slow_depth_workspace_bytes(tsdl.MB, 3, n) == train_mb_slow.tmsl.load().mc_train_mb_slow_workspace_bytes(n)
    for store, l2 in ((0, 0), (0, 8), (1, 0), (1, 8), (0, -1), (2, 3), (-1, 3)):
        assert lib.mc_train_slow_depth_nparams(store, l2) == 0 and lib.mc_train_slow_depth_workspace_bytes(store, l2, 4) == 0


def test_argument_checks_return_einval_with_a_message_before_any_launch():
    lib = tsdl.load()
    P = 1 << 20                      # never dereferenced: every check precedes the first launch
    L = 2
    need = {s: lib.mc_train_slow_depth_workspace_bytes(s, L, 4) for s in (tsdl.KITTI, tsdl.MB)}

    def step(store=tsdl.KITTI, l2=L, patches=P, n=4, params=P, moms=P, loss=P, ws=P, ws_bytes=None):
        return lib.mc_train_slow_depth_step_batch(store, l2, patches, n, params, moms, 0.003, 0.9, loss, ws, need[store] if ws_bytes is None else ws_bytes,
                                                  None)

    def run(l2=L, x0=P, x1=P, n_img=2, H=10, W=12, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, prm=P, params=P, moms=P, losses=P,
            ws=P, ws_bytes=need[tsdl.KITTI]):
        return lib.mc_train_slow_depth_run(l2, x0, x1, n_img, H, W, nnz, n_nnz, perm, n_perm, t0, n_steps, n, prm, params, moms, 0.003, 0.9, losses, ws,
                                           ws_bytes, None)

    def mb_run(l2=L, planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, src=P, prm=P, params=P, moms=P,
               losses=P, ws=P, ws_bytes=need[tsdl.MB]):
        return lib.mc_train_slow_depth_mb_run(l2, planes, table, n_planes, nnz, n_nnz, perm, n_perm, t0, n_steps, n, src, prm, params, moms, 0.003, 0.9,
                                              losses, ws, ws_bytes, None)

    mb_step = lambda **k: step(store=tsdl.MB, **k)  # noqa: E731
    bad = []
    for name, call in (("step", step), ("mb step", mb_step), ("run", run), ("mb_run", mb_run)):
        bad += [("%s: l2 %d" % (name, l2), lambda call=call, l2=l2: call(l2=l2), "l2 %d outside [1, 7]" % l2) for l2 in (0, 8, -1)]
    bad += [("another store", lambda: step(store=2, ws_bytes=need[tsdl.KITTI]), "store 2"),
            ("n_pairs 0", lambda: step(n=0), "n_pairs 0 outside [1, 1024]"), ("n_pairs above the maximum", lambda: step(n=1025), "n_pairs 1025 outside [1, 1024]"),
            ("mb: n_pairs 0", lambda: mb_step(n=0), "n_pairs 0 outside [1, 256]"), ("mb: n_pairs above the maximum", lambda: mb_step(n=257), "n_pairs 257 outside [1, 256]"),
            ("null patches", lambda: step(patches=None), "null"), ("null params", lambda: step(params=None), "null"),
            ("null moms", lambda: step(moms=None), "null"), ("null loss", lambda: step(loss=None), "null"),
            ("null workspace", lambda: step(ws=None), "workspace"), ("misaligned params", lambda: step(params=P + 4), "aligned"),
            ("workspace one byte short", lambda: step(ws_bytes=need[tsdl.KITTI] - 1), "workspace"),
            ("mb: workspace one byte short", lambda: mb_step(ws_bytes=need[tsdl.MB] - 1), "workspace"),
            ("the workspace of a shallower net", lambda: step(ws_bytes=lib.mc_train_slow_depth_workspace_bytes(tsdl.KITTI, L - 1, 4)), "workspace"),
            ("mb: null patches", lambda: mb_step(patches=None), "null"),
            ("run: null x0", lambda: run(x0=None), "null"), ("run: null perm", lambda: run(perm=None), "null"),
            ("run: null prm", lambda: run(prm=None), "null"), ("run: null losses", lambda: run(losses=None), "null"),
            ("run: null params", lambda: run(params=None), "null"), ("run: n_pairs 0", lambda: run(n=0), "n_pairs"),
            ("run: n_pairs above the maximum", lambda: run(n=1025), "n_pairs"), ("run: H 3", lambda: run(H=3), "image dims"),
            ("run: workspace one byte short", lambda: run(ws_bytes=need[tsdl.KITTI] - 1), "workspace"),
            ("run: steps past the permutation", lambda: run(t0=93), "permutation"), ("run: negative n_steps", lambda: run(n_steps=-1), "n_steps"),
            ("run: empty nnz", lambda: run(n_nnz=0), "nnz"),
            ("mb_run: null planes", lambda: mb_run(planes=None), "null"), ("mb_run: null table", lambda: mb_run(table=None), "null"),
            ("mb_run: null src", lambda: mb_run(src=None), "null"), ("mb_run: null losses", lambda: mb_run(losses=None), "null"),
            ("mb_run: n_pairs 0", lambda: mb_run(n=0), "n_pairs"), ("mb_run: n_pairs above the maximum", lambda: mb_run(n=257), "n_pairs"),
            ("mb_run: workspace one byte short", lambda: mb_run(ws_bytes=need[tsdl.MB] - 1), "workspace"),
            ("mb_run: steps past the permutation", lambda: mb_run(t0=93), "permutation"), ("mb_run: no planes", lambda: mb_run(n_planes=0), "n_planes")]
    for what, call, word in bad:
        rc = call()
        assert rc == tsdl.EINVAL, (what, rc)
        assert word in tsdl.last_error() and tsdl.last_error().startswith("train_slow_depth"), (what, tsdl.last_error())
    assert step(l2=0) == tsdl.EINVAL and "384 activations" in tsdl.last_error()       # why no hidden Linear is refused
    assert step(l2=8) == tsdl.EINVAL and "mc_fc_stack takes 8 layers" in tsdl.last_error()
    with pytest.raises(tsdl.TrainSlowDepthError, match="n_pairs"):
        tsdl.check(step(n=0), "mc_train_slow_depth_step_batch")


# ---- the parameter layout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset, l2", [(d, l2) for d in ("kitti", "mb") for l2 in (1, 2, 7)])
def test_net_shape_round_trips_and_refuses_another_depth(dataset, l2):
    store = tsdl.STORE_OF[dataset]
    net = ORACLE[store](l2)
    shape = train_slow_depth.net_shape(dataset, l2)
    assert (shape.l1, shape.fm, shape.l2, shape.nh2, shape.nparams, shape.library) == (net.L1, 112, l2, 384, net.NPARAMS, "libmctrainslowdepth.so")
    assert [n for n, _ in shape.tensor_names()] == net.NAMES
    conv, fc = net.random_nets(3, 1.0)
    v = shape.flat_params(conv, fc)
    assert v.dtype == np.float32 and v.size == net.NPARAMS
    np.testing.assert_array_equal(v, net.flat(conv, fc))
    c2, f2 = shape.unflat_params(v)
    assert len(c2) == net.L1 and len(f2) == l2 + 1 and f2[-1][0].shape == (1, 384) and f2[0][0].shape == (384, 224)
    for (w, b), (w2, b2) in zip(conv + fc, c2 + f2):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    # the initial net is the parents' rule at this shape: the convolutions' draws first, then the Linears', +-1 / sqrt(fan_in)
    ic, ifc = shape.init_net(3)
    for (w, b), (w2, b2) in zip(conv + fc, ic + ifc):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    _, other = ORACLE[store](l2 + 1 if l2 < 7 else l2 - 1).random_nets(3, 1.0)
    with pytest.raises(ValueError, match="libmctrainslowdepth.so trains l1 %d, fm 112, l2 %d" % (net.L1, l2)):
        shape.flat_params(conv, other)


def test_net_shape_is_the_parents_at_their_depths_and_nothing_outside_1_to_7():
    for dataset, l2, old in (("kitti", 4, train_slow.NET), ("kitti2015", 4, train_slow.NET), ("mb", 3, train_mb_slow.NET)):
        shape = train_slow_depth.net_shape(dataset, l2)
        assert shape.tensor_names() == old.tensor_names() and shape.nparams == old.nparams
        conv, fc = old.init_net(8)
        np.testing.assert_array_equal(shape.flat_params(conv, fc), old.flat_params(conv, fc))
        c2, f2 = shape.init_net(8)
        np.testing.assert_array_equal(shape.flat_params(c2, f2), old.flat_params(conv, fc))
    for l2 in (0, 8):
        with pytest.raises(ValueError, match="l2 1..7"):
            train_slow_depth.net_shape("kitti", l2)
    at = tsdl.at_depth(tsdl.MB, 5)
    assert (at.PREFIX, at.MAX_PAIRS, at.WS, at.L1, at.L2, at.NPARAMS, at.LIB_PATH) == ("mc_train_slow_depth", 256, 11, 5, 5, 453152 + 678145, tsdl.LIB_PATH)
    lib = at.load()            # (store, l2) bound to the calls that take them
    assert lib.mc_train_slow_depth_nparams() == at.NPARAMS and lib.mc_train_slow_depth_workspace_bytes(257) == 0
    assert lib.mc_train_slow_depth_workspace_bytes(2) == tsdl.load().mc_train_slow_depth_workspace_bytes(tsdl.MB, 5, 2) > 0


# ---- flags and routing -------------------------------------------------------------------------------------------------------------
def test_l2_routes_training_to_train_slow_depth():
    """Fails without the feature: -l2 is no flag there."""
    for argv, l2, mod_want in ((["kitti", "slow", "-a", "train_tr", "-l2", "2"], 2, train_slow), (["mb", "slow", "-a", "train_tr", "-l2", "1"], 1, train_mb_slow),
                               (["kitti2015", "slow", "-a", "train_all", "-l2", "7"], 7, train_slow), (["mb", "slow", "-a", "train_all", "-l2", "4"], 4, train_mb_slow),
                               (["kitti", "slow", "-l2", "3", "-nh2", "384", "-a", "train_tr"], 3, train_slow)):
        mod, trainer, dataset, arch, opt, prm = mcmain.route(argv)
        assert trainer is train_slow_depth and (dataset, arch, opt.l2, opt.nh2) == (argv[0], "slow", l2, 384), argv
        assert mod is mod_want                                           # whose parse and evaluate still apply
        fname = train_slow_depth.net_fname_of(dataset, arch, argv[2:])
        assert fname.endswith("_".join(argv[2:]) + ".t7") and "-l2_%d" % l2 in fname


def test_the_default_depth_keeps_todays_route():
    for dataset, default, want in (("kitti", 4, train_slow), ("kitti2015", 4, train_slow), ("mb", 3, train_mb_slow)):
        for extra in ([], ["-l2", str(default)], ["-l2", str(default), "-nh2", "384"]):
            argv = [dataset, "slow", "-a", "train_tr"] + extra
            mod, trainer, _, _, opt, _ = mcmain.route(argv)
            assert mod is want and trainer is want and (opt.l2, opt.nh2) == (default, 384), argv
    # testing and predicting never train: the flag sizes the net there
    mod, trainer, _, _, opt, _ = mcmain.route(["kitti", "slow", "-a", "test_te", "-l2", "2"])
    assert mod is train_slow and trainer is train_slow and opt.l2 == 2
    mod, trainer, _, _, opt, _ = mcmain.route(["mb", "slow", "-a", "predict", "-l2", "5"])
    assert mod is None and trainer is None and opt.l2 == 5
    assert mcmain.route(["kitti", "slow", "-a", "time"])[4].l2 == 4 and mcmain.route(["mb", "slow", "-a", "time"])[4].l2 == 3
    for argv in (["kitti", "fast", "-a", "train_tr"], ["mb", "fast", "-a", "train_tr"], ["kitti", "ad", "-a", "predict"]):
        assert not hasattr(mcmain.route(argv)[4], "l2")                  # no FC flag where there is no FC stack


@pytest.mark.parametrize("argv, words", [
    (["kitti", "slow", "-a", "train_tr", "-l2", "8"], ("-l2 8", "l2 1..7")),
    (["kitti", "slow", "-a", "train_tr", "-l2", "0"], ("-l2 0", "l2 1..7", "384 activations")),
    (["mb", "slow", "-a", "train_tr", "-l2", "8"], ("-l2 8", "l2 1..7")),
    (["mb", "slow", "-a", "test_te", "-l2", "0"], ("-l2 0", "l2 1..7")),
    (["kitti", "slow", "-a", "predict", "-l2", "9"], ("-l2 9", "l2 1..7", "2..8 layers")),
    (["kitti", "slow", "-a", "train_tr", "-nh2", "256"], ("-nh2 256", "only -nh2 384", "384 wide", "mc_fc_stack", "mc_fc_split_stack", "-l2 1..7")),
    (["mb", "slow", "-a", "train_tr", "-nh2", "512"], ("-nh2 512", "only -nh2 384")),
    (["kitti2015", "slow", "-a", "predict", "-nh2", "128"], ("-nh2 128", "only -nh2 384")),
    (["kitti", "fast", "-a", "train_tr", "-l2", "2"], ("-l2", "arch fast", "no FC stack", "{kitti|kitti2015|mb} slow", "-l2 1..7")),
    (["mb", "fast", "-a", "train_tr", "-l2", "3"], ("-l2", "arch fast", "no FC stack")),
    (["kitti", "fast", "-a", "predict", "-nh2", "384"], ("-nh2", "arch fast", "no FC stack")),
    (["kitti", "ad", "-a", "predict", "-l2", "4"], ("-l2", "arch ad", "no FC stack", "image pair")),
    (["mb", "census", "-a", "predict", "-l2", "3"], ("-l2", "arch census", "no FC stack")),
    # what was refused stays refused, in its words
    (["kitti", "slow", "-a", "train_tr", "-l2", "2", "-l1", "3"], ("-l1", "arch slow", "GEMM family")),
    (["mb", "slow", "-a", "train_tr", "-l2", "2", "-fm", "96"], ("-fm", "arch slow"))])
def test_what_the_kernels_do_not_serve_is_refused_naming_what_is_supported(argv, words):
    with pytest.raises(SystemExit) as e:
        mcmain.route(argv)
    for word in words:
        assert word in str(e.value), (word, str(e.value))


def test_every_parser_of_arch_slow_takes_the_flags():
    for parse, head in ((mcmain.parse, ["kitti", "slow", "-a", "predict"]), (mcmain.parse, ["mb", "slow", "-a", "time"]),
                        (train_slow.parse, ["kitti2015", "slow", "-a", "test_all"]), (train_mb_slow.parse, ["mb", "slow", "-a", "test_te"])):
        _, _, opt, prm = parse(head + ["-l2", "6", "-nh2", "384", "-fc_mode", "bf16x3", "-conv_mode", "bf16x3"])
        assert (opt.l2, opt.nh2, opt.fc_mode, opt.conv_mode) == (6, 384, "bf16x3", "bf16x3") and "l2" not in prm
        assert parse(head)[2].l2 == mcmain.FC_SHAPES[head[0]][0]
    with pytest.raises(SystemExit, match="only -nh2 384"):
        train_mb.parse_mb(["mb", "slow", "-a", "train_tr", "-nh2", "256"], "slow", train_mb_slow.MB_SLOW_TRAIN_DEFAULTS, "train_mb_slow")


def test_load_fc_takes_the_depth_for_random_and_npz_nets(tmp_path):
    _, _, opt, _ = mcmain.parse(["kitti", "slow", "-a", "predict", "-l2", "2"])
    fc = mcmain.load_fc("random:7", "kitti", l2=opt.l2)
    assert [w.shape for w, _ in fc] == [(384, 224), (384, 384), (1, 384)] and [b.shape for _, b in fc] == [(384,), (384,), (1,)]
    assert np.abs(fc[0][0]).max() <= 1 / np.sqrt(224) and np.abs(fc[1][0]).max() <= 1 / np.sqrt(384)
    # the first layers of a seed are the same draws at every depth, and the default is the data set's
    deep = mcmain.load_fc("random:7", "kitti")
    assert len(deep) == 5 and len(mcmain.load_fc("random:7", "mb")) == 4 and len(mcmain.load_fc("random:7", "mb", l2=7)) == 8
    assert [w.shape for w, _ in mcmain.load_fc("random:7", "mb", l2=1)] == [(384, 224), (1, 384)]
    for (w, b), (w4, b4) in zip(fc[:2], deep):
        np.testing.assert_array_equal(w, w4)
        np.testing.assert_array_equal(b, b4)
    _, fcl = so.Net(9, 4, 2).random_nets(1, 1.0)
    np.savez(str(tmp_path / "n.npz"), **{"f%s%d" % (k, i + 1): a for i, wb in enumerate(fcl) for k, a in zip("wb", wb)})
    got = mcmain.load_fc(str(tmp_path / "n.npz"), "kitti", l2=2)
    assert len(got) == 3
    np.testing.assert_array_equal(got[2][0], fcl[2][0])
    with pytest.raises(KeyError):
        mcmain.load_fc(str(tmp_path / "n.npz"), "kitti")          # without the flag: five Linears are looked for


# ---- the order of draws ----------------------------------------------------------------------------------------------------------
N_TR, N_TE = 21, 5      # bs 4 (2 pairs per step): `for t = 1, 21 - 2, 2` is a 10-step epoch
INDEX = np.array([[0, 2, 2], [8, 1, 1], [10, 3, 3], [28, 2, 1], [32, 1, 2]], np.int64)   # (first plane, lights, exposures) of 5 images


def recorder(mb):
    class Recorder:
        """Stands in for a Trainer: keeps the permutation and nets it is given and every prm (and src) passed to run()."""
        made = []

        def __init__(self, store0, store1, nnz, perm, conv_layers, fc_layers, n_pairs, device):
            self.perm, self.conv, self.fc, self.prm, self.src = np.array(perm), conv_layers, fc_layers, [], []
            Recorder.made.append(self)

        def run(self, t0, *args):
            if mb:
                self.src.append(args[0].numpy().copy())
            self.prm.append(args[1 if mb else 0].numpy().copy())
            args[-1][:args[1 if mb else 0].shape[0]] = 0.5

        def nets(self):
            return self.conv, self.fc
    return Recorder


def nnz_rows(rng, n, first, n_img):
    return np.stack([rng.integers(1, n_img + 1, n), rng.integers(0, 8, n), rng.integers(0, 10, n), first + np.arange(n)], 1).astype(np.float32)


@pytest.mark.parametrize("dataset", ["kitti", "mb"])
def test_a_seed_draws_the_same_pixels_and_augmentations_at_every_depth(dataset, monkeypatch, tmp_path):
    """train_slow_depth.train at l2 = 2 hands its Trainer the arrays that train_slow.train / train_mb_slow.train hand theirs for the
    same -seed: the same Generator draws in the same order (permutation, each chunk's parameters, on Middlebury its sources).  The
    saved .t7 carries its depth: it loads back with 3 Linears."""
    import torch
    mb = dataset == "mb"
    old = train_mb_slow if mb else train_slow
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(0)
    data = dict(nnz_tr=nnz_rows(rng, N_TR, 100, 5 if mb else 2), nnz_te=nnz_rows(rng, N_TE, 200, 5 if mb else 2))
    if mb:
        data.update(planes=np.zeros(16, np.float32), table=np.zeros(36, train_mb.PLANE_DTYPE), index=INDEX)
    else:
        x = rng.standard_normal((2, 1, 12, 16)).astype(np.float32)
        data.update(x0=x, x1=x[..., ::-1].copy())
    argv = ["-a", "train_tr", "-bs", "4", "-seed", "5", "-epochs", "2"]
    dev = torch.device("cpu")
    recs = {}
    for mod, attr, extra in ((old, "Trainer", []), (train_slow_depth, "MbTrainer" if mb else "Trainer", ["-l2", "2"])):
        Recorder = recorder(mb)
        monkeypatch.setattr(mod, attr, Recorder)
        monkeypatch.setattr(mod, "CHUNK_STEPS", 4)
        _, trainer, _, _, opt, _ = mcmain.route([dataset, "slow"] + argv + extra)
        assert trainer is mod
        lead = () if mod is train_mb_slow else (dataset,)
        fname = mod.train(*lead, opt, argv + extra, dev, data=data)
        recs[mod], = Recorder.made
        assert mod.last_run["epochs"] == 2 and mod.last_run["losses"].size == 20 and os.path.exists(fname)
    a, b = recs[old], recs[train_slow_depth]
    np.testing.assert_array_equal(a.perm, b.perm)
    np.testing.assert_array_equal(a.perm, np.random.default_rng(5).permutation(N_TR))
    assert len(a.prm) == len(b.prm) == 6 and len(a.src) == len(b.src) == (6 if mb else 0) and a.prm[0].shape == (4, 2, 18)
    for x, y in zip(a.prm + a.src, b.prm + b.src):
        np.testing.assert_array_equal(x, y)
    # the initial net is the parents' init_net rule at the new shape; its convolutions are the parents' own draws
    want_conv, want_fc = train_slow_depth.net_shape(dataset, 2).init_net(5)
    assert len(b.fc) == 3 and len(a.fc) == (4 if mb else 5) and len(b.conv) == len(a.conv) == (5 if mb else 4)
    for (w, bias), (w2, bias2) in zip(b.conv + b.fc, want_conv + want_fc):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(bias, bias2)
    for (w, bias), (w2, bias2) in zip(b.conv + b.fc[:1], a.conv + a.fc[:1]):
        np.testing.assert_array_equal(w, w2)
    fname = train_slow_depth.last_run["net_fname"]
    assert "-l2_2" in fname
    saved_fc = mcmain.load_fc(fname, dataset)                     # a .t7 carries its own depth
    assert [w.shape for w, _ in saved_fc] == [(384, 224), (384, 384), (1, 384)] and len(mcmain.load_net(fname, dataset, "slow")) == len(b.conv)
    for (w, bias), (w2, bias2) in zip(saved_fc, b.fc):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(bias.ravel(), bias2)
    with pytest.raises(ValueError, match="hidden Linears for -l2 2"):
        train_slow_depth.train(dataset, opt, argv, dev, data=data, init=old.init_net(1))


# ---- the planned batches of the GPU comparison ---------------------------------------------------------------------------------------
def test_the_planned_batches_stay_within_the_parents_share_under_the_oracle_alone():
    """tests/test_gpu_train_slow_depth.py's float64 comparison runs on batches from which the oracle's selector dropped the pairs with
    a pre-activation within 3e-6 of 0.  At every case's depth, tower and seed it drops at most the 20 % the parents' tests allow
    (measured: 0 .. 12 %), and leaves the case its n_pairs."""
    import train_slow_depth_cases as cases
    assert sorted(set((d, l2) for d, l2, _ in cases.ORACLE_CASES)) == [("kitti", 1), ("kitti", 2), ("kitti", 7), ("mb", 1), ("mb", 5)]
    assert sorted(set(n for _, _, n in cases.ORACLE_CASES)) == [1, 3, 17] and len(cases.ORACLE_CASES) == 15 and cases.MAX_FRAGILE == 0.2
    for dataset, l2, n_pairs in cases.ORACLE_CASES:
        patches, share = cases.sturdy_pairs(dataset, l2, n_pairs)
        assert share <= cases.MAX_FRAGILE and patches.shape == (n_pairs, 3) + (cases.TOWER[dataset][0],) * 2, (dataset, l2, n_pairs, share)


# ---- hs.py -------------------------------------------------------------------------------------------------------------------------
def test_hs_takes_the_depth_of_a_trained_net(tmp_path):
    net = so.Net(9, 4, 2)
    conv, fc = net.random_nets(2, 1.0)
    path = str(tmp_path / "net2.npz")
    arrays = {"%s%d" % (k, i + 1): a for i, wb in enumerate(conv) for k, a in zip("wb", wb)}
    arrays.update({"f%s%d" % (k, i + 1): a for i, wb in enumerate(fc) for k, a in zip("wb", wb)})
    np.savez(path, **arrays)
    o = hs.parse(["random", "kitti", "slow", "test_te", path, "-l2", "2", "-n", "2"])
    assert o.l2 == 2 and o.nh2 == 384
    got, got_fc = hs.check_net(path, "kitti", "slow", l2=o.l2)
    assert len(got) == 4 and len(got_fc) == 3
    for (w, b), (w2, b2) in zip(fc, got_fc):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    assert hs.parse(["random", "kitti", "slow", "test_te", path]).l2 is None
    with pytest.raises(SystemExit, match="does not fit kitti slow"):
        hs.check_net(path, "kitti", "slow")                    # without the flag the check is the data set's four hidden Linears
    with pytest.raises(SystemExit, match="does not fit kitti slow"):
        hs.check_net(path, "kitti", "slow", l2=3)
    # a .t7 of depth 2 carries its depth, and is checked against the flag all the same
    _, _, opt, _ = train_slow.parse(["kitti", "slow", "-a", "train_tr", "-l2", "2"])
    t7 = train_slow.save_net(str(tmp_path / "net2.t7"), conv, fc, opt)
    assert len(hs.check_net(t7, "kitti", "slow", l2=2)[1]) == 3
    with pytest.raises(SystemExit, match="Linears of"):
        hs.check_net(t7, "kitti", "slow")
    assert len(hs.check_net("random:3", "mb", "slow", l2=1)[1]) == 2 and len(hs.check_net("random:3", "mb", "slow")[1]) == 4
    for argv, word in ((["random", "kitti", "slow", "test_te", path, "-l2", "8"], "-l2 1..7"), (["random", "kitti", "slow", "test_te", path, "-l2", "0"], "-l2 1..7"),
                       (["random", "kitti", "fast", "test_te", path, "-l2", "4"], "-l2 1..7"), (["random", "mb", "census", "test_te", path, "-l2", "3"], "no FC stack"),
                       (["random", "kitti", "slow", "test_te", path, "-nh2", "256"], "only -nh2 384")):
        with pytest.raises(SystemExit) as e:
            hs.parse(argv)
        assert word in str(e.value), (argv, str(e.value))
