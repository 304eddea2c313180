"""CPU: the host side of `mb fast -a train_tr | train_all | test_te` (main.lua:455-490, 602-890, 1121-1131): flags and
routing, the loader of a ragged data.mb.* directory and its plane store, the source draws, the test examples, the flat
parameter layout and the saved net, and libmctrainmb.so's symbols and argument checks."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libraries as L  # noqa: E402
import train_mb_oracle as mo  # noqa: E402
from mc_cnn_amd import binio  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402
from mc_cnn_amd import train_mb as tm  # noqa: E402


# ---- parse and routing -----------------------------------------------------------------------------------------------------
def test_parse_defaults_are_main_luas_for_mb_fast():
    for a in ("train_tr", "train_all", "test_te"):
        dataset, arch, opt, prm = tm.parse(["mb", "fast", "-a", a])
        assert (dataset, arch, opt.a) == ("mb", "fast", a)
    want = dict(seed=42, m=0.2, pow=1, lr=0.002, bs=128, mom=0.9, true1=0.5, false1=1.5, false2=6, d_exp=0.2, d_light=0.2, ds=2001,
                hflip=0, vflip=0, rotate=28, hscale=0.8, scale=0.8, trans=0, hshear=0.1, brightness=1.3, contrast=1.1,   # main.lua:51-65
                d_vtrans=1, d_rotate=3, d_hscale=0.9, d_hshear=0.3, d_brightness=0.7, d_contrast=1.1,
                rect="imperfect", color="gray", data_dir="", epochs=14, max_steps=0, gpu=1, net_fname="random:42")
    for k, v in want.items():
        assert getattr(opt, k) == v, k
    assert tm.data_dir_of(opt) == "data.mb.imperfect_gray"
    # the hyper-parameters of main.lua:281-293, as main.parse builds them for -a predict, and direction -1 only
    _, _, _, want_prm = mcmain.parse(["mb", "fast", "-a", "predict"])
    assert prm.pop("left_only") == 1 and want_prm.get("left_only", 0) == 0
    want_prm.pop("left_only", None)
    assert prm == want_prm and prm["pi2"] == 24.3 and prm["blur_sigma"] == 6


def test_parse_overrides():
    _, _, opt, prm = tm.parse(["mb", "fast", "-a", "train_all", "-seed", "7", "-lr", "0.01", "-bs", "64", "-d_exp", "0.5", "-d_light", "0",
                               "-ds", "5", "-rect", "perfect", "-max_steps", "5", "-epochs", "2", "-pi1", "2.5", "-net_fname", "x.t7",
                               "-m", "0.3", "-pow", "2", "-false2", "8"])
    assert (opt.seed, opt.lr, opt.bs, opt.d_exp, opt.d_light, opt.ds, opt.max_steps, opt.epochs, opt.net_fname, opt.m, opt.pow, opt.false2) == \
        (7, 0.01, 64, 0.5, 0, 5, 5, 2, "x.t7", 0.3, 2, 8)
    assert prm["pi1"] == 2.5 and tm.data_dir_of(opt) == "data.mb.perfect_gray"
    assert tm.data_dir_of(tm.parse(["mb", "fast", "-a", "test_te", "-data_dir", "d"])[2]) == "d"


def test_main_routes_mb_fast_training_and_main_parse_keeps_refusing():
    from mc_cnn_amd import train_mb_slow
    route = mcmain.training_module
    for a in ("train_tr", "train_all", "test_te"):
        assert route(["mb", "fast", "-a", a]) is tm and route(["mb", "fast", "-seed", "3", "-a", a, "-bs", "64"]) is tm
    assert route(["mb", "slow", "-a", "train_tr"]) is train_mb_slow
    for argv in (["mb", "fast", "-a", "predict"], ["mb", "fast", "-a", "time"], ["kitti", "fast", "-a", "train_tr"],
                 ["mb", "fast", "-a", "test_all"], ["mb", "fast", "-a", "submit"], ["mb", "fast"], ["mb", "fast", "-a"]):
        assert route(argv) is None, argv
    with pytest.raises(SystemExit, match="fast only"):
        mcmain.parse(["mb", "fast", "-a", "train_tr"])
    with pytest.raises(SystemExit, match="train_mb.parse"):
        mcmain.parse(["mb", "fast", "-a", "train_tr"])


@pytest.mark.parametrize("argv, word", [
    (["mb", "fast", "-a", "train_tr", "-color", "rgb"], "one input plane"),
    (["mb", "slow", "-a", "train_tr"], "221 KB"),
    (["mb", "fast", "-a", "test_all"], "main.lua:1136"),
    (["mb", "fast", "-a", "submit"], "submit is out of scope"),
    (["mb", "fast", "-a", "train_tr", "-subset", "0.5"], "-subset"),
    (["mb", "fast", "-a", "train_tr", "-debug"], "-debug"),
    (["mb", "fast", "-a", "predict"], "not a training or testing action"),
    (["kitti", "fast", "-a", "train_tr"], "mb fast"),
    (["mb", "fast", "-a", "train_tr", "-bs", "7"], "pairs of samples")])
def test_parse_refuses_what_is_out_of_scope_and_says_why(argv, word):
    with pytest.raises(SystemExit) as e:
        tm.parse(argv)
    assert word in str(e.value), str(e.value)


# ---- the loader ------------------------------------------------------------------------------------------------------------
# (H, W, lights >= 2, exposures, test views, dispnoc) of a ragged set: image 2 has one training light and one exposure,
# image 3 three lights x three exposures, images 5 and 6 are test-only without ground truth (6 without training lights)
RAGGED = ((12, 20, 2, 2, 2, True), (9, 31, 1, 1, 0, True), (17, 14, 3, 3, 4, True), (10, 10, 2, 1, 0, True), (8, 25, 1, 2, 2, False),
          (11, 13, 0, 0, 2, False))


def write_ragged(d, spec=RAGGED, nnz_imgs=(1, 2, 3, 4), te=(3,), seed=0):
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    files = {}
    for n, (H, W, n_light, n_exp, n_test, has_disp) in enumerate(spec, 1):
        files[(n, 1)] = rng.standard_normal((n_test, 1, H, W)).astype(np.float32) if n_test else np.zeros((0,), np.float32)
        for l in range(2, 2 + n_light):
            files[(n, l)] = rng.standard_normal((n_exp, 2, 1, H, W)).astype(np.float32)
        if has_disp:
            binio.tofile(os.path.join(d, "dispnoc%d.bin" % n), rng.uniform(0, 5, (1, 1, H, W)).astype(np.float32))
    for (n, l), a in files.items():
        binio.tofile(os.path.join(d, "x_%d_%d.bin" % (n, l)), a)
    nnz = lambda ids: np.array([[i, 3, 4, 2] for i in ids for _ in range(3)], np.float32)
    binio.tofile(os.path.join(d, "meta.bin"), np.array([[s[0], s[1], 16] for s in spec], np.int32))
    binio.tofile(os.path.join(d, "te.bin"), np.array(te, np.int32))
    binio.tofile(os.path.join(d, "nnz_tr.bin"), nnz([i for i in nnz_imgs if i not in te]))
    binio.tofile(os.path.join(d, "nnz_te.bin"), nnz([i for i in nnz_imgs if i in te]))
    return files


def test_loader_builds_the_plane_store_of_a_ragged_set(tmp_path):
    d = str(tmp_path / "data.mb.imperfect_gray")
    files = write_ragged(d)
    # a light past a gap is never read: image 4 has lights 2 and 3, so light 5 lies behind the missing light 4
    binio.tofile(os.path.join(d, "x_4_5.bin"), np.zeros((1, 2, 1, 10, 10), np.float32))
    data = tm.load_mb_data(d, "train_all")
    assert [len(x) for x in data["X"]] == [3, 2, 4, 3, 2, 1]
    assert data["X"][1][0].size == 0 and data["X"][1][0].ndim == 1          # the 0-element light-1 file of the older sets
    assert data["X"][2][0].shape == (4, 1, 17, 14) and data["X"][0][0].shape == (2, 1, 12, 20)
    assert sorted(data["dispnoc"]) == [1, 2, 3, 4]
    assert data["meta"].shape == (6, 3) and list(data["te"]) == [3]
    assert data["nnz_tr"].shape == (9, 4) and data["nnz_te"].shape == (3, 4)
    planes, table, index = data["planes"], data["table"], data["index"]
    assert planes.dtype == np.float32 and table.dtype == tm.PLANE_DTYPE and table.dtype.itemsize == tm.tml.PLANE_BYTES == 16
    np.testing.assert_array_equal(index[:, 1:], [[2, 2], [1, 1], [3, 3], [2, 1], [1, 2], [0, 0]])
    assert table.shape[0] == sum(2 * s[2] * s[3] for s in RAGGED) == 8 + 2 + 18 + 4 + 4
    # plane by plane against the files: offset, H, W and content
    k, end = 0, 0
    for n, (H, W, n_light, n_exp, _, _) in enumerate(RAGGED, 1):
        assert index[n - 1, 0] == k
        for l in range(n_light):
            for e in range(n_exp):
                for v in range(2):
                    rec = table[index[n - 1, 0] + (l * n_exp + e) * 2 + v]
                    assert (rec["offset"], rec["H"], rec["W"]) == (end, H, W), (n, l, e, v)
                    np.testing.assert_array_equal(planes[end:end + H * W].reshape(H, W), files[(n, l + 2)][e, v, 0])
                    end += H * W
                    k += 1
    assert end == planes.size and k == table.shape[0]
    # test_te reads light 1 only and builds no store
    te = tm.load_mb_data(d, "test_te")
    assert [len(x) for x in te["X"]] == [1] * 6 and "planes" not in te
    # train_tr needs training lights for the images of nnz_tr only
    assert tm.load_mb_data(d, "train_tr")["table"].shape[0] == table.shape[0]


def test_loader_refuses_unusable_sets_naming_the_image(tmp_path):
    d = str(tmp_path / "a")
    write_ragged(d, nnz_imgs=(1, 2, 6))                     # image 6 has no light >= 2
    with pytest.raises(ValueError, match=r"image 6 .*no light >= 2"):
        tm.load_mb_data(d, "train_tr")
    assert tm.load_mb_data(d, "test_te")["nnz_tr"].shape == (9, 4)
    d = str(tmp_path / "b")
    write_ragged(d)
    binio.tofile(os.path.join(d, "x_3_3.bin"), np.zeros((2, 2, 1, 17, 14), np.float32))     # two exposures beside three
    with pytest.raises(ValueError, match=r"image 3: light 3 .*must agree"):
        tm.load_mb_data(d, "train_tr")
    binio.tofile(os.path.join(d, "x_3_3.bin"), np.zeros((3, 2, 1, 17, 15), np.float32))     # another width
    with pytest.raises(ValueError, match=r"image 3: light 3 .*must agree"):
        tm.load_mb_data(d, "train_all")
    d = str(tmp_path / "c")
    write_ragged(d, spec=RAGGED[:3] + ((3, 10, 2, 1, 0, True),) + RAGGED[4:])
    with pytest.raises(ValueError, match=r"image 4: planes of 3 x 10 .*sampler's range"):
        tm.load_mb_data(d, "train_tr")
    with pytest.raises(ValueError, match="sampler's range"):
        import torch
        tm.device_table(np.array([(0, 16, 3)], tm.PLANE_DTYPE), torch.device("cpu"))


# ---- the source draws ------------------------------------------------------------------------------------------------------
INDEX = np.array([[0, 2, 2], [8, 1, 1], [10, 3, 3], [28, 2, 1], [32, 1, 2]], np.int64)   # RAGGED's, images 1..5


def decode(src, img):
    """plane ids -> (light, exp, view) of each, 0-based, light 0 the file's light 2"""
    first, n_exp = INDEX[img - 1, 0], INDEX[img - 1, 2]
    k = src - first[..., None]
    return k // 2 // n_exp[..., None], k // 2 % n_exp[..., None], k % 2


def opt_of(*extra):
    return tm.parse(["mb", "fast", "-a", "train_tr"] + list(extra))[2]


def test_draw_sources_without_d_exp_and_d_light_pairs_the_views_of_one_plane():
    rng = np.random.default_rng(1)
    img = rng.integers(1, 6, (50, 40))
    src = tm.draw_sources(rng, opt_of("-d_exp", "0", "-d_light", "0"), img, INDEX)
    assert src.shape == (50, 40, 2) and src.dtype == np.int32
    np.testing.assert_array_equal(src[..., 1], src[..., 0] + 1)
    light, exp, view = decode(src.astype(np.int64), img)
    assert (view[..., 0] == 0).all() and (view[..., 1] == 1).all()


def test_draw_sources_stay_within_each_images_counts_and_follow_the_reference_rules():
    rng = np.random.default_rng(2)
    img = rng.integers(1, 6, 100000)
    n_light, n_exp = INDEX[img - 1, 1], INDEX[img - 1, 2]
    src = tm.draw_sources(rng, opt_of(), img, INDEX).astype(np.int64)
    light, exp, view = decode(src, img)
    for a, n in ((light, n_light), (exp, n_exp)):
        assert (a >= 0).all() and (a < n[:, None]).all()
    assert (view == [0, 1]).all()
    assert ((src >= INDEX[img - 1, 0][:, None]) & (src < (INDEX[img - 1, 0] + 2 * n_light * n_exp)[:, None])).all()
    # every (light, exposure) of an image is drawn, uniformly: image 3 has 9, each 1/9 of its draws within 5 sigma
    m = img == 3
    counts = np.bincount(light[m, 0] * 3 + exp[m, 0], minlength=9)
    assert np.abs(counts - m.sum() / 9).max() < 5 * np.sqrt(m.sum() * (1 / 9) * (8 / 9))
    # defaults: exp_ redrawn with probability 0.2 (and equal by chance 1 / n_exp of those), light_ lowered with 0.2
    same_exp = (exp[m, 0] == exp[m, 1]).mean()
    assert abs(same_exp - (0.8 + 0.2 / 3)) < 0.02
    lowered = (light[m, 1] != light[m, 0]).mean()                  # light 0 cannot go lower: 0.2 * 2/3
    assert abs(lowered - 0.2 * 2 / 3) < 0.02
    # d_light = 1: light_ == max(2, light - 1) always
    src = tm.draw_sources(rng, opt_of("-d_light", "1", "-d_exp", "0"), img, INDEX).astype(np.int64)
    light, exp, _ = decode(src, img)
    np.testing.assert_array_equal(light[:, 1], np.maximum(0, light[:, 0] - 1))
    np.testing.assert_array_equal(exp[:, 1], exp[:, 0])
    # d_exp = 1: exp_ is uniform and independent of exp (image 3: every (exp, exp_) cell 1/9 of its draws)
    src = tm.draw_sources(rng, opt_of("-d_exp", "1", "-d_light", "0"), img, INDEX).astype(np.int64)
    light, exp, _ = decode(src, img)
    np.testing.assert_array_equal(light[:, 1], light[:, 0])
    cells = np.bincount(exp[m, 0] * 3 + exp[m, 1], minlength=9)
    assert np.abs(cells - m.sum() / 9).max() < 5 * np.sqrt(m.sum() * (1 / 9) * (8 / 9))
    assert (exp[:, 1] < n_exp).all()
    with pytest.raises(ValueError, match="image 6 has no light"):
        tm.draw_sources(rng, opt_of(), np.array([6]), np.concatenate([INDEX, [[36, 0, 0]]]))


def test_test_te_examples_are_te_then_the_two_extra_views_of_image_5():
    assert tm.test_examples(np.array([1, 5], np.int32)) == [(1, 2), (5, 2), (5, 3), (5, 4)]
    assert tm.test_examples(np.array([[7], [9], [12]])) == [(7, 2), (9, 2), (12, 2), (5, 3), (5, 4)]


# ---- parameters and the saved net --------------------------------------------------------------------------------------------
def test_flat_params_round_trip_and_layout():
    layers = mcmain.load_net("random:3", "mb", "fast")
    assert [w.shape for w, _ in layers] == mo.SHAPES
    v = tm.flat_params(layers)
    assert v.size == 148352 == tm.tml.NPARAMS == 64 * 9 + 64 + 4 * (64 * 64 * 9 + 64) and v.dtype == np.float32
    np.testing.assert_array_equal(v, mo.flat(layers))
    np.testing.assert_array_equal(v[:576], layers[0][0].ravel())
    np.testing.assert_array_equal(v[576:640], layers[0][1])
    np.testing.assert_array_equal(v[640:640 + 36864], layers[1][0].ravel())
    np.testing.assert_array_equal(v[-64:], layers[4][1])
    for (w, b), (w2, b2) in zip(layers, tm.unflat_params(v)):
        np.testing.assert_array_equal(w, w2)
        np.testing.assert_array_equal(b, b2)
    with pytest.raises(ValueError):
        tm.flat_params(layers[:4])
    with pytest.raises(ValueError):
        tm.unflat_params(v[:-1])


def test_saved_net_round_trips_into_the_readers(tmp_path):
    from mc_cnn_amd import t7
    layers = mo.random_layers(5)
    argv = ["-a", "train_tr", "-seed", "5"]
    _, _, opt, _ = tm.parse(["mb", "fast"] + argv)
    fname = tm.net_fname_of("mb", "fast", argv)
    assert fname == os.path.join("net", "net_mb_fast_-a_train_tr_-seed_5.t7")     # main.lua:344-347, 594
    path = tm.save_net(str(tmp_path / fname), layers, opt)
    for got in (t7.load_reference_net(path, "fast")[0], mcmain.load_net(path, "mb", "fast")):
        assert len(got) == 5
        for (w, b), (w2, b2) in zip(layers, got):
            assert w2.shape == w.shape and b2.shape == b.shape
            np.testing.assert_array_equal(w, w2)
            np.testing.assert_array_equal(b, b2)
    obj = t7.load(path)
    assert [m.cls for m in t7._modules(obj[1])] == ["cudnn.SpatialConvolution", "cudnn.ReLU"] * 4 + [
        "cudnn.SpatialConvolution", "nn.Normalize2", "nn.StereoJoin"]
    assert all(m["padW"] == 1 and m["padH"] == 1 for m in t7._modules(obj[1])[:9:2])
    assert obj[2]["seed"] == 5 and obj[2]["a"] == "train_tr" and obj[2]["d_exp"] == 0.2 and obj[2]["false2"] == 6


# ---- the library -------------------------------------------------------------------------------------------------------------
def test_library_loads_without_a_gpu_and_exports_the_headers_symbols():
    """what only libmctrainmb.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    assert tm.tml.load().mc_train_mb_version() == 1 and len(L.exported_abi(tm.tml.LIB_PATH)) == 6
    text = open(os.path.join(ROOT, "include", "mc_train_mb.h")).read()
    for name, value in (("NPARAMS", tm.tml.NPARAMS), ("MAX_PAIRS", tm.tml.MAX_PAIRS), ("FM", tm.tml.FM), ("L1", tm.tml.L1), ("WS", tm.tml.WS),
                        ("NPRM", tm.tml.NPRM), ("ABI_VERSION", tm.tml.ABI_VERSION)):
        assert re.search(r"#define MC_TRAIN_MB_%s %d\b" % (name, value), text), name
    assert (tm.tml.WS, tm.tml.L1, tm.tml.FM, tm.tml.NPRM) == (11, 5, 64, 18) and tm.tml.MAX_PAIRS >= 64
    assert L.built_kernels(tm.tml.LIB_PATH) == {"train_mb_sample_kernel", "train_mb_step_kernel<true>", "train_mb_step_kernel<false>", "train_mb_sgd_kernel"}


def test_workspace_bytes():
    wb = tm.tml.load().mc_train_mb_workspace_bytes
    assert wb(0) == 0 and wb(-1) == 0 and wb(tm.tml.MAX_PAIRS + 1) == 0
    for n in (1, 3, 64, tm.tml.MAX_PAIRS):
        assert wb(n) == n * (tm.tml.NPARAMS + 1) * 4      # a slab row and a loss per pair


def test_argument_checks_return_einval_with_a_message_before_any_launch():
    lib = tm.tml.load()
    P = 1 << 20                      # never dereferenced: every check precedes the first launch
    need = lib.mc_train_mb_workspace_bytes(4)

    def step(patches=P, n=4, params=P, moms=P, margin=0.2, pow_=1, loss=P, ws=P, ws_bytes=need):
        return lib.mc_train_mb_step_batch(patches, n, params, moms, 0.002, 0.9, margin, pow_, loss, ws, ws_bytes, None)

    def sample(planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, rows=P, src=P, prm=P, n=4, out=P):
        return lib.mc_train_mb_sample(planes, table, n_planes, nnz, n_nnz, rows, src, prm, n, out, None)

    def run(planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, src=P, prm=P, params=P, moms=P,
            losses=P, ws=P, ws_bytes=need):
        return lib.mc_train_mb_run(planes, table, n_planes, nnz, n_nnz, perm, n_perm, t0, n_steps, n, src, prm, params, moms, 0.002, 0.9,
                                   0.2, 1, losses, ws, ws_bytes, None)

    bad = [("n_pairs 0", lambda: step(n=0), "n_pairs"), ("n_pairs above the maximum", lambda: step(n=tm.tml.MAX_PAIRS + 1), "n_pairs"),
           ("null patches", lambda: step(patches=None), "null"), ("null params", lambda: step(params=None), "null"),
           ("null moms", lambda: step(moms=None), "null"), ("null loss", lambda: step(loss=None), "null"),
           ("null workspace", lambda: step(ws=None), "workspace"), ("workspace one byte short", lambda: step(ws_bytes=need - 1), "workspace"),
           ("pow 3", lambda: step(pow_=3), "pow"), ("margin nan", lambda: step(margin=float("nan")), "margin"),
           ("sample: null planes", lambda: sample(planes=None), "null"), ("sample: null table", lambda: sample(table=None), "null"),
           ("sample: null nnz", lambda: sample(nnz=None), "null"), ("sample: null rows", lambda: sample(rows=None), "null"),
           ("sample: null src", lambda: sample(src=None), "null"), ("sample: null out", lambda: sample(out=None), "null"),
           ("sample: n_pairs 0", lambda: sample(n=0), "n_pairs"), ("sample: no planes", lambda: sample(n_planes=0), "n_planes"),
           ("sample: empty nnz", lambda: sample(n_nnz=0), "nnz"),
           ("run: null planes", lambda: run(planes=None), "null"), ("run: null table", lambda: run(table=None), "null"),
           ("run: null perm", lambda: run(perm=None), "null"), ("run: null src", lambda: run(src=None), "null"),
           ("run: null prm", lambda: run(prm=None), "null"), ("run: null losses", lambda: run(losses=None), "null"),
           ("run: n_pairs 0", lambda: run(n=0), "n_pairs"), ("run: workspace one byte short", lambda: run(ws_bytes=need - 1), "workspace"),
           ("run: steps past the permutation", lambda: run(t0=93), "permutation"), ("run: negative t0", lambda: run(t0=-1), "permutation"),
           ("run: negative n_steps", lambda: run(n_steps=-1), "n_steps"), ("run: empty nnz", lambda: run(n_nnz=0), "nnz")]
    for what, call, word in bad:
        rc = call()
        assert rc == tm.tml.EINVAL, (what, rc)
        assert word in tm.tml.last_error(), (what, tm.tml.last_error())
    with pytest.raises(tm.tml.TrainMbError, match="n_pairs"):
        tm.tml.check(step(n=0), "mc_train_mb_step_batch")


# ---- the host loop -----------------------------------------------------------------------------------------------------------
N_TR, N_TE = 21, 5      # bs 4 (2 pairs per step): `for t = 1, 21 - 2, 2` is a 10-step epoch


class Recorder:
    """Stands in for train_mb.Trainer: stores the constructor's arguments and every run() call; a step's loss is its index
    in the whole run."""
    made = []

    def __init__(self, planes, table, nnz, perm, layers, n_pairs, device):
        self.nnz, self.perm, self.n_pairs, self.net = np.array(nnz), np.asarray(perm), n_pairs, layers
        self.calls, self.steps_done = [], 0
        Recorder.made.append(self)

    def run(self, t0, src, prm, lr, mom, margin, pow_, losses):
        k = prm.shape[0]
        self.calls.append(dict(t0=t0, n_steps=k, src=src.numpy().copy(), prm_shape=tuple(prm.shape), lr=lr, mom=mom, margin=margin,
                               pow=pow_, offset=losses.storage_offset()))
        for s in range(k):
            losses[s] = float(self.steps_done)
            self.steps_done += 1

    def layers(self):
        return self.net


def test_host_loop_draws_each_chunks_sources_from_the_images_of_its_pairs(monkeypatch, tmp_path):
    import torch
    from mc_cnn_amd import t7
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(tm, "Trainer", Recorder)
    monkeypatch.setattr(tm, "CHUNK_STEPS", 4)
    Recorder.made = []
    rng = np.random.default_rng(0)
    nnz = lambda n, first: np.stack([rng.integers(1, 6, n), rng.integers(0, 8, n), rng.integers(0, 10, n), first + np.arange(n)],
                                    1).astype(np.float32)
    data = dict(nnz_tr=nnz(N_TR, 100), nnz_te=nnz(N_TE, 200), planes=np.zeros(16, np.float32), table=np.zeros(36, tm.PLANE_DTYPE),
                index=INDEX)
    argv = ["-a", "train_tr", "-bs", "4", "-seed", "5", "-epochs", "13", "-lr", "0.004", "-m", "0.3", "-pow", "2"]
    _, _, opt, _ = tm.parse(["mb", "fast"] + argv)
    fname = tm.train(opt, argv, torch.device("cpu"), data=data)
    rec, = Recorder.made
    assert [(c["t0"], c["n_steps"]) for c in rec.calls] == [(0, 4), (8, 4), (16, 2)] * 13 and tm.last_run["epochs"] == 13
    assert sorted(rec.perm.tolist()) == list(range(N_TR)) and rec.perm.dtype == np.int32 and rec.n_pairs == 2
    np.testing.assert_array_equal(rec.nnz, data["nnz_tr"])
    for e, c in enumerate(rec.calls):
        assert c["prm_shape"] == (c["n_steps"], 2, 18) and c["src"].shape == (c["n_steps"], 2, 2) and c["src"].dtype == np.int32
        assert c["lr"] == (0.004 if e < 33 else 0.004 / 10) and (c["mom"], c["margin"], c["pow"]) == (0.9, 0.3, 2)
        assert c["offset"] == c["t0"] // 2
        # every pair's planes belong to the image of its nnz row, left view then right view
        img = rec.nnz[rec.perm[c["t0"]:c["t0"] + 2 * c["n_steps"]], 0].astype(np.int64).reshape(c["n_steps"], 2)
        light, exp, view = decode(c["src"].astype(np.int64), img)
        assert (light >= 0).all() and (light < INDEX[img - 1, 1][..., None]).all() and (exp < INDEX[img - 1, 2][..., None]).all()
        assert (view == [0, 1]).all()
    assert any((c["src"] != rec.calls[0]["src"]).any() for c in rec.calls[3::3])       # redrawn every epoch
    np.testing.assert_array_equal(tm.last_run["losses"], np.arange(130, dtype=np.float32))
    assert fname == os.path.join("net", "net_mb_fast_-a_train_tr_-bs_4_-seed_5_-epochs_13_-lr_0.004_-m_0.3_-pow_2.t7")
    got = t7.load_reference_net(fname, "fast")[0]
    want = mcmain.load_net("random:5", "mb", "fast")         # started from the seeded net, saved what the Trainer holds
    assert len(got) == 5
    np.testing.assert_array_equal(got[4][0], want[4][0])
    # train_all adds nnz_te; fewer pairs than a batch is refused
    Recorder.made = []
    argv = ["-a", "train_all", "-bs", "4", "-epochs", "1", "-max_steps", "7"]
    tm.train(tm.parse(["mb", "fast"] + argv)[2], argv, torch.device("cpu"), data=data)
    rec, = Recorder.made
    np.testing.assert_array_equal(rec.nnz, np.concatenate([data["nnz_tr"], data["nnz_te"]], 0))
    assert [(c["t0"], c["n_steps"]) for c in rec.calls] == [(0, 4), (8, 3)]
    with pytest.raises(SystemExit, match="fewer than a batch"):
        argv = ["-a", "train_tr", "-bs", "64"]
        tm.train(tm.parse(["mb", "fast"] + argv)[2], argv, torch.device("cpu"), data=data)
