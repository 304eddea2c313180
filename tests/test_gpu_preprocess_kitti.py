"""GPU: the dataset kernels of libmctrain.so (mc_train_filter_gt, mc_train_nnz_count / _fill) bit-compared with the
reference's own remove_nonvisible / remove_occluded / remove_white / make_dataset2 (oracle/_ref), `preprocess_kitti` on
a synthetic tree against the numpy restatement, and preprocess -> `-a train_tr` (also `-at 1`) end to end."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import preprocess_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pk():
    import torch
    from mc_cnn_amd import preprocess_kitti
    assert torch.cuda.is_available()
    return preprocess_kitti


def _maps(rng, n, H, W):
    """PNG16-quantised maps with occlusions and non-visible pixels, and raw 0..255 images with 255 in them."""
    d = np.stack([po.png16_map(rng, H, W, d_max=min(100.0, 2.0 * W)) for _ in range(n)]).astype(np.float32) / 256
    x = rng.integers(0, 256, (n, H, W)).astype(np.float32)
    x[rng.uniform(0, 1, (n, H, W)) < 0.03] = 255
    return d, x


@pytest.mark.parametrize("W", [1242, 1226, 97, 1])
@pytest.mark.parametrize("H", [350, 5, 1])
def test_filter_matches_the_reference(pk, ref, W, H):
    import torch
    rng = np.random.default_rng(W * 1000 + H)
    n = 2
    d, x = _maps(rng, n, H, W)
    got = torch.from_numpy(d).cuda()
    pk.filter_gt(got, torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    changed = np.zeros(3, np.int64)
    for k in range(n):
        y = torch.from_numpy(d[k].reshape(1, 1, H, W).copy()).cuda()
        stages = [y.cpu().numpy()]
        ref.call("remove_nonvisible", y)
        stages.append(y.cpu().numpy())
        ref.call("remove_occluded", y)
        stages.append(y.cpu().numpy())
        ref.call("remove_white", torch.from_numpy(x[k].reshape(1, 1, H, W).copy()).cuda(), y)
        stages.append(y.cpu().numpy())
        want = stages[-1].reshape(H, W)
        assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), (k, int((got[k] != want).sum()))
        changed += [int((stages[i + 1] != stages[i]).sum()) for i in range(3)]
    assert np.array_equal(got, po.filter_gt(d, x))
    if H > 1 and W > 97:
        assert (changed > 0).all(), changed     # non-visible, occluded and white pixels were all removed


def _ref_list(ref, disp, ids):
    import torch
    n, H, W = disp.shape
    buf = torch.zeros((max(1, n * H * W), 4), dtype=torch.float32)
    t = 0
    for k in range(n):
        t = int(ref.call("make_dataset2", torch.from_numpy(disp[k].reshape(1, 1, H, W).copy()), buf, int(ids[k]), t)[0])
    return buf[:t].numpy().copy()


@pytest.mark.parametrize("case", ["maps", "empty", "full", "one_row", "one_col", "none"])
def test_pixel_list_matches_make_dataset2(pk, ref, case):
    import torch
    rng = np.random.default_rng(7)
    shape = {"one_row": (3, 1, 1242), "one_col": (4, 350, 1), "none": (0, 5, 7)}.get(case, (3, 350, 1242))
    n, H, W = shape
    d = np.stack([po.png16_map(rng, H, W) for _ in range(n)] or [np.zeros((H, W))]).astype(np.float32)[:n] / 256
    if case == "empty":
        d[:] = 0
        d[1, 7, 9] = 0.5          # not > 0.5
    elif case == "full":
        d = rng.uniform(0.51, 200, shape).astype(np.float32)
    ids = np.array([5, 1, 9, 2][:n], np.int32)
    want = _ref_list(ref, d, ids) if n else np.zeros((0, 4), np.float32)
    got = pk.pixel_list(torch.from_numpy(d).cuda(), ids).cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got, po.make_dataset2(d, ids))
    if case == "full":
        assert got.shape[0] == n * H * W
    if case == "empty":
        assert got.shape[0] == 0


def _run_tree(pk, root, stages=None):
    out = {}
    for year in (2012, 2015):
        out[year] = pk.preprocess_set(year, 4, 2, n_val=2, root=root, stages=stages)
    return out


def _files(root, pk):
    got = {}
    for year in (2012, 2015):
        d = os.path.join(root, pk.SETS[year]["path"])
        for k in pk.OUTPUTS:
            for ext in ("", ".dim", ".type"):
                got[(year, k + ".bin" + ext)] = open(os.path.join(d, k + ".bin" + ext), "rb").read()
    return got


def test_full_run_matches_the_numpy_restatement(pk, tmp_path):
    import shutil
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for year, seed in ((2012, 3), (2015, 4)):
        po.write_tree(a, year, 4, 2, seed=seed)
    _run_tree(pk, a, po.stages)
    want = _files(a, pk)
    shutil.copytree(a, b)
    for root in (a, b):
        out = _run_tree(pk, root)
        assert _files(root, pk) == want
        for year in (2012, 2015):
            assert out[year]["nnz_tr"].shape[0] > 0 and out[year]["nnz_te"].shape[0] > 0
            t = pk.last_timing[year]
            assert all(t[k] >= 0 for k in ("decode", "normalize", "write", "gpu_upload", "gpu_filter", "gpu_lists"))


def test_preprocess_then_train_end_to_end(pk, tmp_path, monkeypatch, capsys):
    from mc_cnn_amd import binio, main, train
    monkeypatch.chdir(tmp_path)
    for year, seed in ((2012, 11), (2015, 12)):
        po.write_tree(".", year, 4, 1, seed=seed, textured=True, noise=1.0, block=(16, 16))
        pk.preprocess_set(year, 4, 1, n_val=1)
    te = binio.fromfile("data.kitti/te.bin")
    assert te.dtype == np.int64 and te.size == 1
    capsys.readouterr()
    steps = 1200
    assert main.main(["kitti", "fast", "-a", "train_tr", "-seed", "3", "-max_steps", str(steps), "-disp_max", "32"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    losses = train.last_run["losses"]
    assert losses.size == steps and np.isfinite(losses).all()
    n = steps // 10
    first, last = float(losses[:n].mean()), float(losses[-n:].mean())
    assert last < 0.75 * first, (first, last)
    err_trained = float(out[-1])
    assert main.main(["kitti", "fast", "-a", "test_te", "-net_fname", "random:3", "-disp_max", "32"]) == 0
    err_random = float(capsys.readouterr().out.strip().splitlines()[-1])
    print("test_te error: trained %.4f, seeded random net %.4f; loss %.4f -> %.4f" % (err_trained, err_random, first, last))
    assert err_trained < err_random
    # -at 1: both sets, 3 + 3 training images and the 2015 validation image
    assert main.main(["kitti2015", "fast", "-a", "train_tr", "-at", "1", "-seed", "3", "-max_steps", "200", "-disp_max", "32"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    assert np.isfinite(train.last_run["losses"]).all() and train.last_run["losses"].size == 200
    assert train.last_run["net_fname"].startswith(os.path.join("net", "net_kitti2015_fast_-a_train_tr_-at_1"))
    te15 = binio.fromfile("data.kitti2015/te.bin")
    assert len(out[-2].split()) == 2 and 0 <= float(out[-1]) <= 1
    data = train.load_data("kitti2015", main.parse(["kitti2015", "fast", "-a", "test_te", "-at", "1"])[2])
    assert data["te"].tolist() == (te15 + 4).tolist() and data["x0"].shape[0] == 4 + 4 + 2
