"""GPU: libmctrainmbslow.so (include/mc_train_mb_slow.h) against float64 torch autograd of Middlebury's accurate net on the
CPU (tests/train_mb_slow_oracle.py), its exact-zero gradient at a saturated output, `mc_train_mb_slow_run` against the chain of
libmctrainmb.so's sampler and `step_batch`, bitwise reproducibility, the limits refused on the host, learning on a small
synthetic Middlebury directory from wide initial weights, and `main.py mb slow -a train_tr` end to end from the reference's
initialisation.

The numeric tests use weights drawn from +-sqrt(6 / fan_in), as tests/test_gpu_train_slow.py does and for its reason: under
the reference's +-1 / sqrt(fan_in) the net's output is a constant and many random pairs have a pre-activation within 3e-6 of
0, where fp32 rounding flips a ReLU mask.  Bounds are the project's for the accurate net (loss 1e-5, each of the 18 momenta
tensors 1e-4 of its largest magnitude, parameters atol 1e-5): float32 CPU autograd of this net on the very batches of the
one-step test differs from float64 by at most 2.8e-7 on the loss and 1.4e-6 on the worst tensor, so the bounds leave about
70x over plain fp32 rounding."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_mb_oracle as mo  # noqa: E402
import train_mb_slow_oracle as so  # noqa: E402
from train_fixtures import dev, rel, same_bits  # noqa: E402
from test_gpu_train_mb import small_set  # noqa: E402

pytestmark = pytest.mark.gpu

LR, MOM = 0.003, 0.9


@pytest.fixture(scope="module")
def tms():
    import torch
    from mc_cnn_amd import train_mb_slow
    assert torch.cuda.is_available()
    return train_mb_slow


@pytest.fixture(scope="module")
def wide():
    return so.wide_nets(1)


def sturdy_pairs(conv, fc, seed, n_pairs):
    """The first n_pairs of 3 * n_pairs N(0, 1) candidates with no pre-activation within 3e-6 of 0 in float64 (the oracle
    alone decides, before the GPU is touched)."""
    rng = np.random.default_rng(seed)
    cand = rng.standard_normal((3 * n_pairs, 3, 11, 11)).astype(np.float32)
    frag = so.fragile(conv, fc, cand)
    print("%d of %d candidate pairs are fragile" % (frag.sum(), frag.size))
    assert frag.mean() <= 0.2, "more than 20 % of the candidates are fragile (the oracle alone gives 0/3, 1/9, 6/51, 8/99)"
    return cand[~frag][:n_pairs]


# 2 FC rows; 6; 34 rows = two full 16-row tiles and a ragged third; 66 rows, past one four-tile FC workgroup.  The tower grid
# has 3, 9, 51 and 99 workgroups.
@pytest.mark.parametrize("n_pairs", [1, 3, 17, 33])
def test_one_step_matches_float64_autograd(tms, wide, n_pairs):
    import torch
    conv, fc = wide
    patches = sturdy_pairs(conv, fc, 40 + n_pairs, n_pairs)
    assert patches.shape[0] == n_pairs
    params = dev(so.flat(conv, fc))
    moms = torch.zeros_like(params)
    loss = float(tms.step_batch(dev(patches), params, moms, LR, MOM).cpu())
    wp, wv, wl = so.sgd_steps(conv, fc, [patches], LR, MOM)
    print("n_pairs %d: loss %.7f, float64 %.7f, difference %.2e" % (n_pairs, loss, wl[0], abs(loss - wl[0])))
    got = moms.cpu().numpy()
    print("n_pairs %d: relative L2 of all momenta %.2e, worst parameter %.2e" % (n_pairs, rel(got, wv), np.abs(params.cpu().numpy() - wp).max()))
    assert abs(loss - wl[0]) <= 1e-5
    assert np.isfinite(got).all() and np.abs(wv).max() > 1e-6
    errs = so.check_per_tensor(got, wv, 1e-4, "n_pairs %d" % n_pairs)
    print("n_pairs %d: worst tensor %.2e" % (n_pairs, max(errs.values())))
    np.testing.assert_allclose(params.cpu().numpy(), wp, rtol=0, atol=1e-5)


def test_twenty_steps_match_float64_autograd(tms, wide):
    import torch
    conv, fc = wide
    rng = np.random.default_rng(101)
    n_pairs = 16
    batches = [rng.standard_normal((n_pairs, 3, 11, 11)).astype(np.float32) for _ in range(20)]
    params = dev(so.flat(conv, fc))
    moms = torch.zeros_like(params)
    ws = torch.empty(tms.tmsl.load().mc_train_mb_slow_workspace_bytes(n_pairs) // 4, dtype=torch.float32, device="cuda")
    losses = []
    worst_p = worst_v = 0.0
    for k, b in enumerate(batches):
        p0, v0 = params.cpu().numpy(), moms.cpu().numpy()
        losses.append(float(tms.step_batch(dev(b), params, moms, LR, MOM, ws).cpu()))
        # every step of the run against float64 autograd from the same (fp32) state
        c0, f0 = so.unflat(p0)
        wp, wv, wl = so.sgd_steps(c0, f0, [b], LR, MOM, moms=v0)
        worst_p = max(worst_p, float(np.abs(params.cpu().numpy() - wp).max()))
        worst_v = max(worst_v, float(np.abs(moms.cpu().numpy() - wv).max()))
        print("step %d: loss %.7f, float64 %.7f; worst params %.2e, momenta %.2e so far" % (k, losses[-1], wl[0], worst_p, worst_v))
        assert abs(losses[-1] - wl[0]) <= 1e-5, (k, losses[-1], wl[0])
        np.testing.assert_allclose(params.cpu().numpy(), wp, rtol=0, atol=1e-5)
        np.testing.assert_allclose(moms.cpu().numpy(), wv, rtol=0, atol=1e-5)
    print("20 steps: worst absolute error of a step's params %.2e, momenta %.2e" % (worst_p, worst_v))
    wp, wv, wl = so.sgd_steps(conv, fc, batches, LR, MOM, fp32_state=True)
    gp, gv = params.cpu().numpy(), moms.cpu().numpy()
    print("20 steps: losses %s; relative L2 error params %.2e, momenta %.2e" % (np.round(losses, 4).tolist(), rel(gp, wp), rel(gv, wv)))
    np.testing.assert_allclose(losses, wl, rtol=1e-4, atol=0)
    assert rel(gp, wp) <= 1e-4


def test_saturated_output_gives_an_exactly_zero_gradient(tms, wide):
    """fb4 = +40: o is exactly 1.0f.  The reference's criterion gives grad_o = 1e12 / n (target 0) or -1 / n (target 1),
    and Sigmoid's backward multiplies by o (1 - o) = 0: the gradient is exactly 0, where (o - t) / n would be 1 / n."""
    import torch
    conv, fc = wide
    rng = np.random.default_rng(5)
    n_pairs = 5
    patches = rng.standard_normal((n_pairs, 3, 11, 11)).astype(np.float32)
    p0 = so.flat(conv, fc).copy()
    p0[-1] = 40.0
    v0 = (rng.uniform(0.5, 1.5, p0.size) * rng.choice([-1, 1], p0.size) * 1e-3).astype(np.float32)
    params, moms = dev(p0), dev(v0)
    loss = float(tms.step_batch(dev(patches), params, moms, LR, MOM).cpu())
    want = -math.log(float(np.float32(1e-12))) / 2
    print("saturated: loss %.6f, -log(1e-12f) / 2 = %.6f" % (loss, want))
    assert abs(loss - want) <= 1e-5 * want
    v1, p1 = moms.cpu().numpy(), params.cpu().numpy()
    assert np.isfinite(v1).all() and np.isfinite(p1).all()
    want_v = np.float32(MOM) * v0
    np.testing.assert_array_equal(v1.view(np.uint32), want_v.view(np.uint32))
    np.testing.assert_array_equal(p1.view(np.uint32), (p0 + want_v).view(np.uint32))


# ---- mc_train_mb_slow_run --------------------------------------------------------------------------------------------------
def run_steps(tms, nets, seed, n_steps, n_pairs, t0=0):
    """n_steps of mc_train_mb_slow_run on test_gpu_train_mb.small_set's ragged store with -hflip 1 -d_exp 0.5 -d_light 0.5"""
    import torch
    from mc_cnn_amd import train_mb
    planes, table, index, nnz = small_set(train_mb)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    opt = tms.parse(["mb", "slow", "-a", "train_tr", "-hflip", "1", "-d_exp", "0.5", "-d_light", "0.5"])[2]
    prm = tms.draw_params(rng, opt, n_steps, n_pairs)
    ids = nnz[perm[t0:t0 + n_steps * n_pairs], 0].reshape(n_steps, n_pairs)
    src = tms.draw_sources(rng, opt, ids, index)
    assert (src[..., 1] != src[..., 0] + 1).any()          # some pairs take their right view from another light or exposure
    t = tms.Trainer(planes, table, nnz, perm, nets[0], nets[1], n_pairs, torch.device("cuda"))
    losses = torch.empty(n_steps, dtype=torch.float32, device="cuda")
    t.run(t0, dev(src), dev(prm), LR, MOM, losses)
    torch.cuda.synchronize()
    return t, prm, src, perm, losses.cpu().numpy()


def test_run_equals_the_chain_of_sample_and_step(tms, wide):
    import torch
    from mc_cnn_amd import train_mb
    n_steps, n_pairs, t0 = 3, 5, 7
    t, prm, src, perm, losses = run_steps(tms, wide, 3, n_steps, n_pairs, t0)
    params = dev(so.flat(*wide))
    moms = torch.zeros_like(params)
    for s in range(n_steps):
        rows = dev(perm[t0 + s * n_pairs:t0 + (s + 1) * n_pairs])
        patches = train_mb.sample(t.planes, t.table, t.nnz, rows, dev(src[s]), dev(prm[s]))      # libmctrainmb.so's sampler
        loss = tms.step_batch(patches, params, moms, LR, MOM).cpu().numpy()
        assert loss.view(np.uint32)[0] == losses.view(np.uint32)[s], s
    assert same_bits(params, t.params) and same_bits(moms, t.moms)
    assert np.isfinite(losses).all() and (losses > 0).all() and not same_bits(params, dev(so.flat(*wide)))


def test_runs_are_bitwise_reproducible(tms, wide):
    import torch
    a, _, _, _, la = run_steps(tms, wide, 4, 30, 64)
    b, _, _, _, lb = run_steps(tms, wide, 4, 30, 64)
    assert same_bits(a.params, b.params) and same_bits(a.moms, b.moms)
    np.testing.assert_array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert np.isfinite(la).all() and bool(torch.isfinite(a.params).all()) and bool(torch.isfinite(a.moms).all())


def test_limits_are_refused_before_any_launch(tms, wide):
    import torch
    from mc_cnn_amd import train_mb
    lib = tms.tmsl.load()
    M = tms.tmsl.MAX_PAIRS
    wb = lib.mc_train_mb_slow_workspace_bytes
    assert M == 256 and wb(1) > 0 and wb(M) > 0 and wb(0) == 0 and wb(M + 1) == 0
    n_pairs = 4
    need = wb(n_pairs)
    rng = np.random.default_rng(0)
    params = dev(so.flat(*wide))
    moms = torch.zeros_like(params)
    p0 = params.clone()
    patches = dev(rng.standard_normal((n_pairs, 3, 11, 11)).astype(np.float32))
    ws = torch.empty(need // 4, dtype=torch.float32, device="cuda")
    loss = torch.full((1,), -7.0, device="cuda")
    P = lambda x: x.data_ptr()
    step = lambda n, nbytes: lib.mc_train_mb_slow_step_batch(P(patches), n, P(params), P(moms), LR, MOM, P(loss), P(ws), nbytes, None)
    for n, nbytes, word in ((n_pairs, need - 1, "workspace"), (0, need, "n_pairs"), (M + 1, need, "n_pairs")):
        assert step(n, nbytes) == tms.tmsl.EINVAL and word in tms.tmsl.last_error()      # the message is the last call's: ask after each
    torch.cuda.synchronize()
    assert same_bits(params, p0) and not moms.any() and float(loss) == -7
    planes, table, index, nnz = small_set(train_mb)
    t = tms.Trainer(planes, table, nnz, np.arange(100, dtype=np.int32), wide[0], wide[1], n_pairs, torch.device("cuda"))
    prm = dev(tms.draw_params(rng, tms.parse(["mb", "slow", "-a", "train_tr"])[2], 3, n_pairs))
    src = torch.zeros((3, n_pairs, 2), dtype=torch.int32, device="cuda")
    losses = torch.full((3,), -7.0, device="cuda")
    with pytest.raises(tms.tmsl.TrainMbSlowError, match="permutation"):
        t.run(89, src, prm, LR, MOM, losses)     # 89 + 3 * 4 > 100
    t.n_pairs = M + 1
    with pytest.raises(tms.tmsl.TrainMbSlowError, match="n_pairs"):
        t.run(0, src.new_zeros((1, M + 1, 2)), prm.new_zeros((1, M + 1, 18)), LR, MOM, losses)
    t.n_pairs = n_pairs
    torch.cuda.synchronize()
    assert same_bits(t.params, p0) and not t.moms.any() and (losses == -7).all()   # nothing ran: parameters, momenta, sentinels
    t.run(88, src, prm, LR, MOM, losses)          # 88 + 12 == 100 fits
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and not same_bits(t.params, p0)


# ---- learning and end to end on a synthetic data.mb.* directory ---------------------------------------------------------------
def test_it_learns_from_wide_weights(tms, tmp_path, monkeypatch, capsys):
    """600 steps at bs 64 from +-sqrt(6 / fan_in) weights on scenes with noise 0.5, the mb augmentation defaults: the loss
    halves and the trained nets match better than the initial ones.  (From the reference's initialisation the loss stays
    at ln 2 on such a set: test_train_tr_end_to_end_from_the_references_initialisation.)  A float32 CPU torch run of the
    same net on the restated sampler, same set, distributions and seed-3 weights, draws made in one chunk: 0.688 -> 0.254,
    0.37x."""
    import torch
    from mc_cnn_amd import main
    monkeypatch.chdir(tmp_path)
    mo.write_synthetic_mb(str(tmp_path / "mbdata"), noise=0.5)
    steps = 600
    argv = ["-a", "train_tr", "-data_dir", "mbdata", "-seed", "3", "-bs", "64", "-max_steps", str(steps)]
    _, _, opt, _ = tms.parse(["mb", "slow"] + argv)
    init = so.wide_nets(3)
    fname = tms.train(opt, argv, torch.device("cuda"), init=init)
    losses = tms.last_run["losses"]
    assert losses.size == steps and np.isfinite(losses).all()
    n = steps // 10
    first, last = float(losses[:n].mean()), float(losses[-n:].mean())
    _, _, opt0, _ = tms.parse(["mb", "slow"] + argv)
    init_fname = tms.save_net(os.path.join("net", "init.t7"), init[0], init[1], opt0)
    capsys.readouterr()
    errs = []
    for f in (fname, init_fname):
        assert main.main(["mb", "slow", "-a", "test_te", "-data_dir", "mbdata", "-net_fname", f]) == 0
        errs.append(float(capsys.readouterr().out.strip().splitlines()[-1]))
    print("loss: first tenth %.4f, last tenth %.4f (%.2f x); test_te error: trained %.4f, initial wide nets %.4f"
          % (first, last, last / first, errs[0], errs[1]))
    assert last <= 0.5 * first, (first, last)
    assert errs[0] < errs[1], errs


def test_train_tr_end_to_end_from_the_references_initialisation(tms, tmp_path, monkeypatch, capsys):
    """`main.py mb slow -a train_tr` from init_net(-seed), the ranges of nn.SpatialConvolution:reset and nn.Linear:reset.
    As for the KITTI accurate net, the net sits on a plateau from there on this small set: float64 on N(0, 1) patches gives
    logits of 1e-4 ... 1.5e-3, and 40 steps stay in 0.69314 ... 0.69323.  That is expected, and what this test asserts: every
    loss within 0.01 of ln 2; learning is test_it_learns_from_wide_weights."""
    from PIL import Image
    from mc_cnn_amd import binio, main
    monkeypatch.chdir(tmp_path)
    written = mo.write_synthetic_mb(str(tmp_path / "mbdata"))
    steps = 200
    assert main.main(["mb", "slow", "-a", "train_tr", "-data_dir", "mbdata", "-seed", "3", "-max_steps", str(steps), "-bs", "64"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    run = tms.last_run
    losses = run["losses"]
    assert losses.size == steps and np.isfinite(losses).all()
    print("losses %.5f .. %.5f, ln 2 = %.5f" % (losses.min(), losses.max(), math.log(2)))
    assert np.abs(losses - math.log(2)).max() <= 0.01
    # the epoch line (epoch, mean loss, lr, seconds), then `runtime err` per example -- (1, 2), (5, 2), (5, 3), (5, 4) --, then the mean
    n_ex = len(mo.SCENE_TE) + 2
    assert len(out) == 1 + n_ex + 1 and len(out[0].split()) == 4 and out[0].split()[0] == "1" and float(out[0].split()[2]) == 0.003
    assert abs(float(out[0].split()[1]) - math.log(2)) <= 0.01
    assert [len(l.split()) for l in out[1:1 + n_ex]] == [2] * n_ex
    errs = [float(l.split()[1]) for l in out[1:1 + n_ex]]
    assert all(0 <= e <= 1 for e in errs) and abs(np.mean(errs) - float(out[-1])) < 1e-9
    fname = run["net_fname"]
    assert fname == os.path.join("net", "net_mb_slow_-a_train_tr_-data_dir_mbdata_-seed_3_-max_steps_200_-bs_64.t7") and os.path.exists(fname)
    conv, fc = main.load_net(fname, "mb", "slow"), main.load_fc(fname, "mb")      # t7.load_reference_net, parsed once
    assert len(conv) == 5 and len(fc) == 4 and conv[4][0].shape == (112, 112, 3, 3) and fc[0][0].shape == (384, 224) and fc[3][0].shape == (1, 384)
    init_conv, _ = tms.init_net(3)
    assert not np.array_equal(conv[0][0], init_conv[0][0])        # the step moved the weights
    capsys.readouterr()
    assert main.main(["mb", "slow", "-a", "test_te", "-data_dir", "mbdata", "-net_fname", fname]) == 0
    out2 = capsys.readouterr().out.strip().splitlines()
    assert len(out2) == n_ex + 1 and 0 <= float(out2[-1]) <= 1
    x = written[1][1]                                              # image 1's test views (2, 1, 60, 90)
    for name, a in (("l.png", x[0, 0, :32, :80]), ("r.png", x[1, 0, :32, :80])):
        Image.fromarray(np.clip(a * 40 + 128, 0, 255).astype(np.uint8)).save(name)
    assert main.main(["mb", "slow", "-a", "predict", "-net_fname", fname, "-left", "l.png", "-right", "r.png", "-disp_max", "16"]) == 0
    disp = binio.read_bin("disp.bin", (32, 80))
    assert np.isfinite(disp).all() and os.path.getsize("left.bin") == 16 * 32 * 80 * 4
