"""CPU: `python -m mc_cnn_amd.preprocess_kitti` (preprocess_kitti.lua) with its GPU stages replaced by the numpy
restatement of tests/preprocess_oracle.py -- torch7's generator and randperm, the crop, normalisation, padding, metadata
and file format of the written sets, the refusals -- and the index arithmetic of `-at 1` (main.lua:403-426)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import preprocess_oracle as po  # noqa: E402
from mc_cnn_amd import binio  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402
from mc_cnn_amd import preprocess_kitti as pk  # noqa: E402
from mc_cnn_amd import train  # noqa: E402


def test_generator_is_mt19937():
    g = pk.MT19937(42)
    assert [g.genrand_int32(), g.genrand_int32()] == [1608637542, 3421126067]
    g = pk.MT19937()
    assert [g.genrand_int32() for _ in range(10000)][-1] == 4123659995     # std::mt19937, default seed 5489
    bg = np.random.MT19937(0)
    bg._legacy_seeding(42)                                                   # init_genrand, like torch.manualSeed
    g = pk.MT19937(42)
    assert [g.genrand_int32() for _ in range(1500)] == [int(v) for v in bg.random_raw(1500)]


@pytest.mark.parametrize("n", [1, 2, 194, 200])
def test_randperm_is_a_one_based_permutation(n):
    p = pk.randperm(n, pk.MT19937(42))
    assert p.dtype == np.int64 and sorted(p.tolist()) == list(range(1, n + 1))


def test_randperm_restates_the_swap_loop():
    g, ref = pk.MT19937(7), pk.MT19937(7)
    r = list(range(10))
    for i in range(9):
        z = ref.genrand_int32() % (10 - i)
        r[i], r[i + z] = r[i + z], r[i]
    assert pk.randperm(10, g).tolist() == [v + 1 for v in r]


@pytest.mark.parametrize("year", [2012, 2015])
def test_split_sizes(year):
    n_tr = pk.SETS[year]["n_tr"]
    tr, te = pk.split(n_tr)
    assert (te.size, tr.size) == (40, n_tr - 40) and tr.dtype == te.dtype == np.int64
    assert sorted(np.concatenate([te, tr]).tolist()) == list(range(1, n_tr + 1))
    assert np.array_equal(np.concatenate([te, tr]), pk.randperm(n_tr, pk.MT19937(42)))


def test_cli_sets_and_usage():
    assert (pk.SETS[2012]["n_tr"], pk.SETS[2012]["n_te"], pk.SETS[2015]["n_tr"], pk.SETS[2015]["n_te"]) == (194, 195, 200, 200)
    with pytest.raises(SystemExit, match="usage"):
        pk.main(["2014"])


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    """Both sets of a small synthetic tree at KITTI's sizes, preprocessed with the numpy stages."""
    root = str(tmp_path_factory.mktemp("kitti"))
    out = {}
    for year, seed in ((2012, 1), (2015, 2)):
        po.write_tree(root, year, 3, 2, seed=seed)
        d = os.path.join(root, pk.SETS[year]["path"])
        open(os.path.join(d, "keep.txt"), "w").write("not ours")
        binio.tofile(os.path.join(d, "x0.bin"), np.ones((2, 2), np.float32))     # a stale set is overwritten
        out[year] = pk.preprocess_set(year, 3, 2, n_val=1, root=root, stages=po.stages)
    return root, out


def _load_crop(root, year, d, cnt, which):
    s = pk.SETS[year]
    img = mcmain.load_image(os.path.join(root, s["path"], "unzip", d, s[which], "%06d_10.png" % cnt))
    if year == 2015:
        assert img.shape[0] == 3
        img = mcmain.rgb2y(img)
    return img[:, img.shape[1] - pk.HEIGHT:]


@pytest.mark.parametrize("year", [2012, 2015])
def test_written_set(written, year):
    root, out = written
    d = os.path.join(root, pk.SETS[year]["path"])
    got = {k: binio.fromfile(os.path.join(d, k + ".bin")) for k in pk.OUTPUTS}
    for k in pk.OUTPUTS:
        assert np.array_equal(got[k], out[year][k]), k
    assert open(os.path.join(d, "keep.txt")).read() == "not ours"
    x0, x1, disp, meta = got["x0"], got["x1"], got["dispnoc"], got["metadata"]
    assert x0.shape == x1.shape == (5, 1, 350, 1242) and x0.dtype == np.float32
    assert disp.shape == (3, 1, 350, 1242) and disp.dtype == np.float32
    assert meta.dtype == np.int32 and meta.shape == (5, 3)
    examples = [("training", c) for c in range(3)] + [("testing", c) for c in range(2)]
    for k, (dd, cnt) in enumerate(examples):
        h, w = po.SIZES[(cnt + (dd == "testing")) % 3]
        assert meta[k].tolist() == [h, w, cnt]
        for x, which in ((x0, "image_0"), (x1, "image_1")):
            crop = _load_crop(root, year, dd, cnt, which)
            assert crop.shape == (1, 350, w)
            assert np.array_equal(x[k, :, :, :w], mcmain.normalize(crop))
            assert not x[k, :, :, w:].any()
            assert abs(float(x[k, :, :, :w].mean())) < 1e-4 and abs(float(x[k, :, :, :w].std(ddof=1)) - 1) < 1e-4
        if dd == "training":
            gt = binio.read_png16(os.path.join(root, pk.SETS[year]["path"], "unzip", "training", pk.SETS[year]["disp_noc"],
                                               "%06d_10.png" % cnt))
            assert np.array_equal(disp[k, 0, :, :w], gt[h - 350:])          # unfiltered
            assert not disp[k, 0, :, w:].any()
    tr, te = got["tr"], got["te"]
    assert tr.dtype == te.dtype == np.int64
    want_tr, want_te = pk.split(3, 1)
    assert tr.tolist() == want_tr.tolist() and te.tolist() == want_te.tolist()
    filt = po.filter_gt(disp[:, 0], x0[:3, 0])
    for key, ids in (("nnz_tr", tr), ("nnz_te", te)):
        ids = np.sort(ids)
        assert np.array_equal(got[key], po.make_dataset2(filt[ids - 1], ids)), key
        assert got[key].dtype == np.float32 and got[key].shape[1] == 4 and got[key].shape[0] > 0
    assert set(np.unique(got["nnz_te"][:, 0]).tolist()) == set(te.tolist())
    # the filters removed something, and the unfiltered map keeps it
    assert (filt > 0.5).sum() < (disp > 0.5).sum()
    for k in pk.OUTPUTS:
        f = os.path.join(d, k + ".bin")
        t = {np.float32: "float32", np.int32: "int32", np.int64: "int64"}[got[k].dtype.type]
        assert open(f + ".type").read() == t
        assert open(f + ".dim").read() == "".join("%d\n" % n for n in got[k].shape)
        assert os.path.getsize(f) == got[k].nbytes


def test_filter_restatement_rules():
    x = np.zeros((1, 8), np.float32)
    d = np.array([[3, 0.5, 1, 9, 2, 2, 1, 0]], np.float32)
    want = d.copy()                    # non-visible: col 0 (3 >= 0) and col 3 (9 >= 3); then the scalar occlusion loop
    want[0, 0] = want[0, 3] = 0
    nv = want.copy()
    for c in range(8):
        for i in range(1, 8 - c):
            if np.float32(i) - nv[0, c + i] < -nv[0, c]:
                want[0, c] = 0
                break
    assert np.array_equal(po.filter_gt(d, x), want)
    x[0, 6] = 255
    want[0, 6] = 0
    assert np.array_equal(po.filter_gt(d, x), want)


def _tree_one(tmp_path, year=2012, **kw):
    po.write_tree(str(tmp_path), year, 2, 1, seed=5, **kw)
    return os.path.join(str(tmp_path), pk.SETS[year]["path"], "unzip")


def _run(tmp_path, year=2012):
    return pk.preprocess_set(year, 2, 1, n_val=1, root=str(tmp_path), stages=po.stages)


def _save(path, a):
    from PIL import Image
    Image.fromarray(a).save(path)


def test_refuses_a_missing_file(tmp_path):
    u = _tree_one(tmp_path)
    for f in (os.path.join(u, "testing", "image_1", "000000_10.png"), os.path.join(u, "training", "disp_noc", "000001_10.png")):
        os.rename(f, f + ".away")
        with pytest.raises(SystemExit, match="%s: no such file" % f):
            _run(tmp_path)
        os.rename(f + ".away", f)
    _run(tmp_path)


def test_refuses_short_and_wide_images(tmp_path):
    u = _tree_one(tmp_path)
    f = os.path.join(u, "training", "image_0", "000001_10.png")
    _save(f, np.zeros((349, 1200), np.uint8))
    with pytest.raises(SystemExit, match="%s: 349 x 1200: the set needs at least 350 rows and at most 1242 columns" % f):
        _run(tmp_path)
    _save(f, np.zeros((375, 1243), np.uint8))
    with pytest.raises(SystemExit, match="%s: 375 x 1243" % f):
        _run(tmp_path)


def test_refuses_mismatched_sizes(tmp_path):
    u = _tree_one(tmp_path)
    f = os.path.join(u, "training", "disp_noc", "000000_10.png")
    _save(f, np.zeros((375, 1241), np.uint16))
    with pytest.raises(SystemExit, match="%s: ground truth of 375 x 1241, its image .* is 375 x 1242" % f):
        _run(tmp_path)
    _save(f, np.zeros((375, 1242), np.uint16))
    _run(tmp_path)
    f = os.path.join(u, "testing", "image_1", "000000_10.png")
    _save(f, np.zeros((370, 1200), np.uint8))
    with pytest.raises(SystemExit, match=f):
        _run(tmp_path)


def test_refuses_wrong_channel_counts(tmp_path):
    u = _tree_one(tmp_path, year=2015)
    f = os.path.join(u, "training", "image_2", "000000_10.png")
    _save(f, np.zeros((375, 1242), np.uint8))
    with pytest.raises(SystemExit, match="%s: 1 channels" % f):
        _run(tmp_path, 2015)


# ---- -at 1 ---------------------------------------------------------------------------------------------------------------
def _fake_set(d, n_tr, n_te, tag):
    """A tiny set whose arrays record where each entry came from: image k of set `tag` is filled with tag * 100 + k."""
    os.makedirs(d)
    n, H, W = n_tr + n_te, 2, 3
    img = (tag * 100 + np.arange(n, dtype=np.float32))[:, None, None, None] * np.ones((1, 1, H, W), np.float32)
    binio.tofile(os.path.join(d, "x0.bin"), img)
    binio.tofile(os.path.join(d, "x1.bin"), -img)
    binio.tofile(os.path.join(d, "dispnoc.bin"), img[:n_tr] + 0.5)
    binio.tofile(os.path.join(d, "metadata.bin"), np.array([[H, W, tag * 100 + k] for k in range(n)], np.int32))
    perm = np.arange(1, n_tr + 1, dtype=np.int64)[::-1].copy()
    binio.tofile(os.path.join(d, "te.bin"), perm[:1])
    binio.tofile(os.path.join(d, "tr.bin"), perm[1:])
    for key, ids in (("nnz_tr", perm[1:]), ("nnz_te", perm[:1])):
        binio.tofile(os.path.join(d, key + ".bin"), np.stack([ids, ids * 0 + tag, ids * 0 + 1, ids * 0 + 2], 1).astype(np.float32))


@pytest.fixture()
def at_sets(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _fake_set("data.kitti", 3, 2, 12)       # n_tr 3 in place of 194, 2 test images in place of 195
    _fake_set("data.kitti2015", 4, 3, 15)   # n_tr 4 in place of 200, 3 test images in place of 200


def _opt(ds, *extra):
    return mcmain.parse([ds, "fast", "-a", "train_tr"] + list(extra))[2]


def test_at_flag():
    assert _opt("kitti").at == 0 and _opt("kitti2015", "-at", "1").at == 1
    with pytest.raises(SystemExit, match="-at 1 .* takes no -data_dir"):
        _opt("kitti", "-at", "1", "-data_dir", "data.kitti")
    assert _opt("kitti", "-data_dir", "d").data_dir == "d"


@pytest.mark.parametrize("ds", ["kitti", "kitti2015"])
def test_at_1_index_arithmetic(at_sets, ds):
    got = train.load_data(ds, _opt(ds, "-at", "1"), train.DATA_FILES + ("dispnoc",))
    first = lambda a: np.asarray(a).reshape(a.shape[0], -1)[:, 0].tolist()
    # 2012 training images, 2015 training images, then the chosen set's test images; for kitti2015 from image n_tr
    # (1-based) on, one early: main.lua's X_15[{{200,400}}]
    tail = [1203, 1204] if ds == "kitti" else [1503, 1504, 1505, 1506]
    want = [1200, 1201, 1202, 1500, 1501, 1502, 1503] + tail
    assert first(got["x0"]) == want and first(got["x1"]) == [-v for v in want]
    assert got["metadata"][:, 2].tolist() == want
    assert first(got["dispnoc"]) == [v + 0.5 for v in [1200, 1201, 1202, 1500, 1501, 1502, 1503]]
    assert got["tr"].tolist() == [2, 1] + [3 + 3, 3 + 2, 3 + 1] and got["tr"].dtype == np.int64
    assert got["te"].tolist() == ([3] if ds == "kitti" else [3 + 4])
    assert got["nnz_tr"][:, 0].tolist() == [2, 1, 6, 5, 4] and got["nnz_tr"][:, 1].tolist() == [12, 12, 15, 15, 15]
    assert got["nnz_te"][:, 0].tolist() == [3, 7]
    # every te / tr index points at a training image of its own set
    for i in got["tr"].tolist() + got["te"].tolist():
        assert got["dispnoc"][i - 1, 0, 0, 0] - 0.5 == got["x0"][i - 1, 0, 0, 0]


def test_at_0_reads_one_set(at_sets):
    got = train.load_data("kitti2015", _opt("kitti2015"), ("x0", "te"))
    assert got["x0"].shape[0] == 7 and got["te"].tolist() == [4]
