"""GPU: libmctrainmb.so (include/mc_train_mb.h) against float64 oracles -- the 11 x 11 sampler on a ragged plane store against
the numpy restatement of make_patch + OpenCV's warp, the five-layer training step against float64 torch autograd of the same
net on the CPU -- and `main.py mb fast -a train_tr` end to end on a small synthetic Middlebury directory."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_mb_oracle as mo  # noqa: E402
from train_fixtures import dev, rel, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

LR, MOM, MARGIN = 0.002, 0.9, 0.2


@pytest.fixture(scope="module")
def tm():
    import torch
    from mc_cnn_amd import train_mb
    assert torch.cuda.is_available()
    return train_mb


def opt_of(*extra):
    from mc_cnn_amd import train_mb
    return train_mb.parse(["mb", "fast", "-a", "train_tr"] + list(extra))[2]


def candidates(rng, n):
    return rng.standard_normal((n, 3, 11, 11)).astype(np.float32)


# ---- the store ----------------------------------------------------------------------------------------------------------------
PLANE_SIZES = ((30, 50), (4, 4), (11, 11), (12, 40), (37, 23), (5, 9), (16, 16), (20, 13))   # (H, W); 4 x 4 is smaller than the patch


def make_store(tm, seed=11, sizes=PLANE_SIZES):
    """Planes of different sizes with distinct content (own noise around an own level), the flat buffer and the table"""
    rng = np.random.default_rng(seed)
    planes = [(rng.standard_normal(s) + 0.25 * k).astype(np.float32) for k, s in enumerate(sizes)]
    table = np.zeros(len(planes), tm.PLANE_DTYPE)
    o = 0
    for k, p in enumerate(planes):
        table[k] = (o, p.shape[0], p.shape[1])
        o += p.size
    flat = np.concatenate([p.ravel() for p in planes])
    return planes, flat, table


def test_sampler_matches_the_warp_restatement_on_a_ragged_store(tm):
    import torch
    planes, flat, table = make_store(tm)
    n_planes = len(planes)
    rng = np.random.default_rng(5)
    n = 48
    prm = tm.draw_params(rng, opt_of(), 1, n)[0]         # the full Middlebury augmentation: rotate 28, scale 0.8, d_* all on
    plain = np.array([0.5, -3, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 1], np.float32)
    nnz, src = [], []
    for k in range(n):
        left = k % n_planes
        right = left if k % 3 == 0 else (3 * k + 1) % n_planes      # two in three pairs take their views from different planes
        H, W = planes[left].shape
        where = k % 7     # inside; straddling the top, bottom, left, right border; wholly outside below, to the right
        row, col = ((H // 2, W // 2), (1, W // 2), (H - 2, W // 2), (H // 2, 1), (H // 2, W - 2), (H + 25, W // 2), (H // 2, W + 40))[where]
        nnz.append([1 + left, row, col, [0, 2, 3.5][k % 3]])
        src.append([left, right])
        if k % 5 == 0:
            prm[k] = plain                                # no warp: the geometry alone
    nnz, src = np.array(nnz, np.float32), np.array(src, np.int32)
    assert (src == n_planes - 1).any(0).all() and (src[:, 0] != src[:, 1]).sum() >= n // 2     # the table's last plane, on both sides
    rows = np.arange(n, dtype=np.int32)
    # out of range: nnz rows -1 and n_nnz, plane ids -1 and n_planes (left, right)
    rows = np.concatenate([rows, [-1, n, 0, 7, 0, 7]]).astype(np.int32)
    src = np.concatenate([src, [[0, 0], [0, 0], [-1, 0], [n_planes, 2], [0, -1], [3, n_planes]]]).astype(np.int32)
    prm = np.concatenate([prm, prm[1:7]])
    dtable = tm.device_table(table, torch.device("cuda"))
    got = tm.sample(dev(flat), dtable, dev(nnz), dev(rows), dev(src), dev(prm)).cpu().numpy()
    assert got.shape == (n + 6, 3, 11, 11)
    nonzero = 0
    for i in range(n + 6):
        row = nnz[rows[i]] if 0 <= rows[i] < n else None
        want = mo.sample_pair(planes, row, src[i], prm[i])
        np.testing.assert_allclose(got[i], want, rtol=0, atol=1e-5, err_msg="pair %d (row %s, planes %s)" % (i, row, src[i]))
        nonzero += int(np.abs(want[0] - prm[i, 8]).max() > 0.1) + int(np.abs(want[1] - prm[i, 16]).max() > 0.1)
    assert nonzero >= n                                   # most patches do show their planes
    for i, sides in ((n, (0, 1, 2)), (n + 1, (0, 1, 2)), (n + 2, (0,)), (n + 3, (0,)), (n + 4, (1, 2)), (n + 5, (1, 2))):
        p = prm[i]
        for s in sides:                                   # 0 * contrast + brightness, exactly
            want = np.float32(0) * p[9 if s == 0 else 17] + p[8 if s == 0 else 16]
            assert (got[i, s] == want).all(), (i, s)
    assert np.abs(got[n + 2, 1] - prm[n + 2, 16]).max() > 0.1 and np.abs(got[n + 4, 0] - prm[n + 4, 8]).max() > 0.1   # the other side is drawn


# ---- one step against float64 autograd -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("n_pairs", [1, 3, 17, 64])
def test_one_step_matches_float64_autograd(tm, n_pairs, pow_):
    import torch
    rng = np.random.default_rng(1000 * pow_ + n_pairs)
    layers = mo.random_layers(5)
    b = mo.robust_patches(layers, candidates(rng, 3 * n_pairs), n_pairs, MARGIN)
    params = dev(mo.flat(layers))
    moms = torch.zeros_like(params)
    loss = float(tm.step_batch(dev(b), params, moms, LR, MOM, MARGIN, pow_).cpu())
    wp, wv, wl = mo.sgd_steps(layers, [b], LR, MOM, MARGIN, pow_)
    print("%d pairs, pow %d: loss %.6f (float64 %.6f)" % (n_pairs, pow_, loss, wl[0]))
    assert abs(loss - wl[0]) <= 1e-5
    np.testing.assert_allclose(params.cpu().numpy(), wp, rtol=0, atol=1e-5)
    np.testing.assert_allclose(moms.cpu().numpy(), wv, rtol=0, atol=1e-5)
    assert np.abs(wv).max() > 1e-6                        # the step moved something
    # the momenta are -lr * g: each of the 10 tensors within 1e-4 of its largest magnitude
    mo.check_per_tensor(moms.cpu().numpy(), wv, 1e-4, "%d pairs, pow %d" % (n_pairs, pow_))


def plan_steps(rng, layers, n_pairs, n_steps, pow_):
    """Batches for consecutive steps, each drawn as 3n candidates of which the first n non-fragile ones are kept, judged on
    the float64 oracle's own trajectory (fp32 state): no GPU involved."""
    p, v = mo.flat(layers), np.zeros(mo.NPARAMS, np.float32)
    batches = []
    for _ in range(n_steps):
        b = mo.robust_patches(mo.unflat(p), candidates(rng, 3 * n_pairs), n_pairs, MARGIN)
        p, v, _ = mo.sgd_steps(mo.unflat(p), [b], LR, MOM, MARGIN, pow_, fp32_state=True, moms=v)
        p, v = p.astype(np.float32), v.astype(np.float32)
        batches.append(b)
    return batches


def test_twenty_steps_match_float64_autograd(tm):
    import torch
    rng = np.random.default_rng(21)
    layers = mo.random_layers(6)
    n_pairs, pow_ = 16, 1
    batches = plan_steps(rng, layers, n_pairs, 20, pow_)
    params = dev(mo.flat(layers))
    moms = torch.zeros_like(params)
    ws = torch.empty(tm.tml.load().mc_train_mb_workspace_bytes(n_pairs) // 4, dtype=torch.float32, device="cuda")
    for k, b in enumerate(batches):
        p0, v0 = params.cpu().numpy(), moms.cpu().numpy()
        loss = float(tm.step_batch(dev(b), params, moms, LR, MOM, MARGIN, pow_, ws).cpu())
        wp, wv, wl = mo.sgd_steps(mo.unflat(p0), [b], LR, MOM, MARGIN, pow_, moms=v0)     # from the same fp32 state
        assert abs(loss - wl[0]) <= 1e-5, (k, loss, wl[0])
        np.testing.assert_allclose(params.cpu().numpy(), wp, rtol=0, atol=1e-5, err_msg="step %d" % k)
        np.testing.assert_allclose(moms.cpu().numpy(), wv, rtol=0, atol=1e-5, err_msg="step %d" % k)
    wp, wv, wl = mo.sgd_steps(layers, batches, LR, MOM, MARGIN, pow_, fp32_state=True)
    gp = params.cpu().numpy()
    print("20 steps: relative L2 error of the parameters %.2e, of the momenta %.2e" % (rel(gp, wp), rel(moms.cpu().numpy(), wv)))
    assert rel(gp, wp) <= 1e-4


@pytest.mark.parametrize("pow_", [1, 2])
def test_inactive_hinges_give_an_exactly_zero_gradient(tm, pow_):
    rng = np.random.default_rng(8)
    layers = mo.random_layers(9)
    b = candidates(rng, 19)
    f, _ = mo.hinge_and_fragility(layers, b, -10.0)
    assert (f < -1).all()                                 # |pos|, |neg| <= 1: with margin -10 every hinge is inactive
    p0 = mo.flat(layers)
    v0 = (rng.standard_normal(mo.NPARAMS) * 1e-3).astype(np.float32)
    params, moms = dev(p0), dev(v0)
    loss = tm.step_batch(dev(b), params, moms, LR, MOM, -10.0, pow_).cpu()
    assert float(loss) == 0
    v1 = v0 * np.float32(MOM)                             # fl(mom * v) - lr * 0, then fl(w + v), in float32
    assert v1.dtype == np.float32 and same_bits(moms, dev(v1)) and same_bits(params, dev(p0 + v1))


# ---- mc_train_mb_run ------------------------------------------------------------------------------------------------------------
def small_set(tm, seed=1):
    """Three scenes of different sizes, lights and exposures in the loader's form: planes, table, index, nnz"""
    rng = np.random.default_rng(seed)
    X, nnz = [], []
    for n, (H, W, n_light, n_exp) in enumerate(((40, 90, 2, 2), (33, 57, 1, 3), (52, 41, 3, 1)), 1):
        base = rng.standard_normal((H, W)).astype(np.float32)
        lights = [np.zeros((0,), np.float32)]
        for l in range(n_light):
            lights.append(np.stack([np.stack([base * (1 + 0.1 * e) + 0.1 * l, np.roll(base, -5, 1) * (1 + 0.1 * e) + 0.1 * l +
                                              0.1 * rng.standard_normal((H, W))])[:, None] for e in range(n_exp)]).astype(np.float32))
        X.append(lights)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        nnz.append(np.stack([np.full(H * W, n), ys.ravel(), xs.ravel(), np.full(H * W, 5)], 1))
    planes, table, index = tm.build_store(X, need={1, 2, 3})
    return planes, table, index, np.concatenate(nnz).astype(np.float32)


def run_steps(tm, seed, n_steps, n_pairs, t0=0):
    import torch
    planes, table, index, nnz = small_set(tm)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    opt = opt_of("-hflip", "1", "-d_exp", "0.5", "-d_light", "0.5")
    prm = tm.draw_params(rng, opt, n_steps, n_pairs)
    ids = nnz[perm[t0:t0 + n_steps * n_pairs], 0].reshape(n_steps, n_pairs)
    src = tm.draw_sources(rng, opt, ids, index)
    assert (src[..., 1] != src[..., 0] + 1).any()          # some pairs take their right view from another light or exposure
    t = tm.Trainer(planes, table, nnz, perm, mo.random_layers(seed), n_pairs, torch.device("cuda"))
    losses = torch.empty(n_steps, dtype=torch.float32, device="cuda")
    t.run(t0, dev(src), dev(prm), LR, MOM, MARGIN, 1, losses)
    torch.cuda.synchronize()
    return t, prm, src, perm, losses.cpu().numpy()


def test_run_equals_the_chain_of_sample_and_step(tm):
    import torch
    n_steps, n_pairs, t0 = 3, 5, 7
    t, prm, src, perm, losses = run_steps(tm, 3, n_steps, n_pairs, t0)
    params = dev(mo.flat(mo.random_layers(3)))
    moms = torch.zeros_like(params)
    for s in range(n_steps):
        rows = dev(perm[t0 + s * n_pairs:t0 + (s + 1) * n_pairs])
        patches = tm.sample(t.planes, t.table, t.nnz, rows, dev(src[s]), dev(prm[s]))
        loss = tm.step_batch(patches, params, moms, LR, MOM, MARGIN, 1).cpu().numpy()
        assert loss[0] == losses[s], s
    assert same_bits(params, t.params) and same_bits(moms, t.moms)
    assert np.isfinite(losses).all() and (losses > 0).all()


def test_runs_are_bitwise_reproducible(tm):
    a, _, _, _, la = run_steps(tm, 4, 30, 64)
    b, _, _, _, lb = run_steps(tm, 4, 30, 64)
    assert same_bits(a.params, b.params) and same_bits(a.moms, b.moms)
    np.testing.assert_array_equal(la, lb)
    assert np.isfinite(la).all()


def test_limits_are_refused_before_any_launch(tm):
    import torch
    lib = tm.tml.load()
    M = tm.tml.MAX_PAIRS
    assert lib.mc_train_mb_workspace_bytes(1) > 0 and lib.mc_train_mb_workspace_bytes(M) > 0
    assert lib.mc_train_mb_workspace_bytes(0) == 0 and lib.mc_train_mb_workspace_bytes(M + 1) == 0
    n_pairs = 4
    need = lib.mc_train_mb_workspace_bytes(n_pairs)
    rng = np.random.default_rng(0)
    params = dev(mo.flat(mo.random_layers(1)))
    moms = torch.zeros_like(params)
    p0 = params.clone()
    patches = dev(candidates(rng, n_pairs))
    ws = torch.empty(need // 4, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), -7.0, device="cuda")
    P = lambda x: x.data_ptr()
    step = lambda n, nbytes: lib.mc_train_mb_step_batch(P(patches), n, P(params), P(moms), LR, MOM, MARGIN, 1, P(loss), P(ws), nbytes, None)
    for n, nbytes, word in ((n_pairs, need - 1, "workspace"), (0, need, "n_pairs"), (M + 1, need, "n_pairs")):
        assert step(n, nbytes) == tm.tml.EINVAL and word in tm.tml.last_error()      # the message is the last call's: ask after each
    planes, table, index, nnz = small_set(tm)
    t = tm.Trainer(planes, table, nnz, np.arange(100, dtype=np.int32), mo.random_layers(1), n_pairs, torch.device("cuda"))
    prm = dev(tm.draw_params(rng, opt_of(), 3, n_pairs))
    src = torch.zeros((3, n_pairs, 2), dtype=torch.int32, device="cuda")
    losses = torch.full((3,), -7.0, device="cuda")
    with pytest.raises(tm.tml.TrainMbError, match="permutation"):
        t.run(89, src, prm, LR, MOM, MARGIN, 1, losses)     # 89 + 3 * 4 > 100
    torch.cuda.synchronize()
    assert same_bits(params, p0) and same_bits(t.params, p0) and float(loss) == -7 and (losses == -7).all()   # nothing ran
    t.run(88, src, prm, LR, MOM, MARGIN, 1, losses)          # 88 + 12 == 100 fits
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and not same_bits(t.params, p0)


# ---- end to end: main.py mb fast -a train_tr on a synthetic data.mb.* directory ----------------------------------------------------
def test_train_tr_end_to_end(tmp_path, monkeypatch, capsys, tm):
    from mc_cnn_amd import main, t7
    monkeypatch.chdir(tmp_path)
    mo.write_synthetic_mb(str(tmp_path / "mbdata"))
    steps = 600
    assert main.main(["mb", "fast", "-a", "train_tr", "-data_dir", "mbdata", "-max_steps", str(steps), "-bs", "64"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    run = tm.last_run
    losses = run["losses"]
    assert losses.size == steps and np.isfinite(losses).all()
    n = steps // 10
    first, last = float(losses[:n].mean()), float(losses[-n:].mean())
    assert last <= 0.5 * first, (first, last)
    assert run["net_fname"] == os.path.join("net", "net_mb_fast_-a_train_tr_-data_dir_mbdata_-max_steps_600_-bs_64.t7")
    assert os.path.exists(run["net_fname"])
    layers, _ = t7.load_reference_net(run["net_fname"], "fast")
    assert len(layers) == 5 and layers[4][0].shape == (64, 64, 3, 3) and layers[0][0].shape == (64, 1, 3, 3)
    # one line per epoch, then `runtime err` per example -- (1, 2), (5, 2), (5, 3), (5, 4) -- then the mean
    n_ex = len(mo.SCENE_TE) + 2
    err_trained = float(out[-1])
    pairs = [l.split() for l in out if len(l.split()) == 2]
    assert len(pairs) == n_ex and [len(l.split()) for l in out[-1 - n_ex:-1]] == [2] * n_ex
    assert abs(np.mean([float(p[1]) for p in pairs]) - err_trained) < 1e-9
    assert main.main(["mb", "fast", "-a", "test_te", "-data_dir", "mbdata", "-net_fname", "random:42"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == n_ex + 1
    err_random = float(out[-1])
    print("test_te error: trained %.4f, seeded random net %.4f; loss %.4f -> %.4f" % (err_trained, err_random, first, last))
    assert err_trained < err_random
