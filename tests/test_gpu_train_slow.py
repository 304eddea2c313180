"""GPU: libmctrainslow.so (include/mc_train_slow.h) against float64 torch autograd of the accurate net on the CPU
(tests/train_slow_oracle.py), its exact-zero gradient at a saturated output, `mc_train_slow_run` against the chain of
libmctrain.so's sampler and `step_batch`, bitwise reproducibility, learning on a small synthetic stereo set from wide
initial weights, and `main.py kitti slow -a train_tr` end to end from the reference's initialisation.

The numeric tests use weights drawn from +-sqrt(6 / fan_in): under the reference's +-1 / sqrt(fan_in) the net's output is a
constant and a third of random pairs have a pre-activation within 3e-6 of 0, where fp32 rounding flips a ReLU mask."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_slow_oracle as so  # noqa: E402
from train_fixtures import dev, rel, small_images, write_synthetic_kitti  # noqa: E402

pytestmark = pytest.mark.gpu

LR, MOM = 0.003, 0.9


@pytest.fixture(scope="module")
def ts():
    import torch
    from mc_cnn_amd import train_slow
    assert torch.cuda.is_available()
    return train_slow


@pytest.fixture(scope="module")
def wide():
    return so.wide_nets(1)


def sturdy_pairs(conv, fc, seed, n_pairs):
    """The first n_pairs of 3 * n_pairs N(0, 1) candidates with no pre-activation within 3e-6 of 0 in float64 (the oracle
    alone decides, before the GPU is touched)."""
    rng = np.random.default_rng(seed)
    cand = rng.standard_normal((3 * n_pairs, 3, 9, 9)).astype(np.float32)
    frag = so.fragile(conv, fc, cand)
    print("%d of %d candidate pairs are fragile" % (frag.sum(), frag.size))
    assert frag.mean() <= 0.2, "more than 20 % of the candidates are fragile (the oracle alone gives 5 %)"
    return cand[~frag][:n_pairs]


@pytest.mark.parametrize("n_pairs", [1, 3, 17, 64])   # 2 rows; odd; 34 rows cross a 32-row tile; the workload's
def test_one_step_matches_float64_autograd(ts, wide, n_pairs):
    import torch
    conv, fc = wide
    patches = sturdy_pairs(conv, fc, 20 + n_pairs, n_pairs)
    assert patches.shape[0] == n_pairs
    params = dev(so.flat(conv, fc))
    moms = torch.zeros_like(params)
    loss = float(ts.step_batch(dev(patches), params, moms, LR, MOM).cpu())
    wp, wv, wl = so.sgd_steps(conv, fc, [patches], LR, MOM)
    print("n_pairs %d: loss %.7f, float64 %.7f, difference %.2e" % (n_pairs, loss, wl[0], abs(loss - wl[0])))
    assert abs(loss - wl[0]) <= 1e-5
    got = moms.cpu().numpy()
    assert np.isfinite(got).all() and np.abs(wv).max() > 1e-6
    errs = so.check_per_tensor(got, wv, 1e-4, "n_pairs %d" % n_pairs)
    print("n_pairs %d: worst tensor %.2e, relative L2 of all momenta %.2e" % (n_pairs, max(errs.values()), rel(got, wv)))
    np.testing.assert_allclose(params.cpu().numpy(), wp, rtol=0, atol=1e-5)


def test_twenty_steps_match_float64_autograd(ts, wide):
    import torch
    conv, fc = wide
    rng = np.random.default_rng(101)
    n_pairs = 16
    batches = [rng.standard_normal((n_pairs, 3, 9, 9)).astype(np.float32) for _ in range(20)]
    params = dev(so.flat(conv, fc))
    moms = torch.zeros_like(params)
    ws = torch.empty(ts.tsl.load().mc_train_slow_workspace_bytes(n_pairs) // 4, dtype=torch.float32, device="cuda")
    losses = []
    worst_p = worst_v = 0.0
    for k, b in enumerate(batches):
        p0, v0 = params.cpu().numpy(), moms.cpu().numpy()
        losses.append(float(ts.step_batch(dev(b), params, moms, LR, MOM, ws).cpu()))
        # every step of the run against float64 autograd from the same (fp32) state
        c0, f0 = so.unflat(p0)
        wp, wv, wl = so.sgd_steps(c0, f0, [b], LR, MOM, moms=v0)
        assert abs(losses[-1] - wl[0]) <= 1e-5, (k, losses[-1], wl[0])
        worst_p = max(worst_p, float(np.abs(params.cpu().numpy() - wp).max()))
        worst_v = max(worst_v, float(np.abs(moms.cpu().numpy() - wv).max()))
        np.testing.assert_allclose(params.cpu().numpy(), wp, rtol=0, atol=1e-5)
        np.testing.assert_allclose(moms.cpu().numpy(), wv, rtol=0, atol=1e-5)
    print("20 steps: worst absolute error of a step's params %.2e, momenta %.2e" % (worst_p, worst_v))
    wp, wv, wl = so.sgd_steps(conv, fc, batches, LR, MOM, fp32_state=True)
    gp, gv = params.cpu().numpy(), moms.cpu().numpy()
    print("20 steps: losses %s; relative L2 error params %.2e, momenta %.2e" % (np.round(losses, 4).tolist(), rel(gp, wp), rel(gv, wv)))
    np.testing.assert_allclose(losses, wl, rtol=1e-4, atol=0)
    assert rel(gp, wp) <= 1e-4


def test_saturated_output_gives_an_exactly_zero_gradient(ts, wide):
    """fb5 = +40: o is exactly 1.0f.  The reference's criterion gives grad_o = 1e12 / n (target 0) or -1 / n (target 1),
    and Sigmoid's backward multiplies by o (1 - o) = 0: the gradient is exactly 0, where (o - t) / n would be 1 / n."""
    import torch
    conv, fc = wide
    rng = np.random.default_rng(5)
    n_pairs = 5
    patches = rng.standard_normal((n_pairs, 3, 9, 9)).astype(np.float32)
    p0 = so.flat(conv, fc).copy()
    p0[-1] = 40.0
    v0 = (rng.uniform(0.5, 1.5, p0.size) * rng.choice([-1, 1], p0.size) * 1e-3).astype(np.float32)
    params, moms = dev(p0), dev(v0)
    loss = float(ts.step_batch(dev(patches), params, moms, LR, MOM).cpu())
    want = -math.log(float(np.float32(1e-12))) / 2
    print("saturated: loss %.6f, -log(1e-12f) / 2 = %.6f" % (loss, want))
    assert abs(loss - want) <= 1e-5 * want
    v1, p1 = moms.cpu().numpy(), params.cpu().numpy()
    assert np.isfinite(v1).all() and np.isfinite(p1).all()
    want_v = np.float32(MOM) * v0
    np.testing.assert_array_equal(v1.view(np.uint32), want_v.view(np.uint32))
    np.testing.assert_array_equal(p1.view(np.uint32), (p0 + want_v).view(np.uint32))


def make_trainer(ts, nets, seed, n_steps, n_pairs, images=(1,)):
    import torch
    x0, x1, nnz = small_images(*images)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    _, _, opt, _ = ts.parse(["kitti", "slow", "-a", "train_tr", "-hflip", "1"])
    prm = dev(ts.draw_params(rng, opt, n_steps, n_pairs))
    t = ts.Trainer(x0, x1, nnz, perm, nets[0], nets[1], n_pairs, torch.device("cuda"))
    return t, prm, perm, (x0, x1, nnz)


def test_run_equals_the_chain_of_sample_and_step(ts, wide):
    import torch
    from mc_cnn_amd import train
    n_steps, n_pairs, t0 = 3, 5, 7
    t, prm, perm, (x0, x1, nnz) = make_trainer(ts, wide, 3, n_steps, n_pairs)      # 3 x 40 x 90
    assert (t.n_img, t.H, t.W) == (3, 40, 90)
    losses = torch.empty(n_steps, dtype=torch.float32, device="cuda")
    t.run(t0, prm, LR, MOM, losses)
    params = dev(so.flat(*wide))
    moms = torch.zeros_like(params)
    chain = []
    for s in range(n_steps):
        rows = perm[t0 + s * n_pairs:t0 + (s + 1) * n_pairs]
        patches = train.sample(dev(x0), dev(x1), dev(nnz), dev(rows), prm[s])
        chain.append(ts.step_batch(patches, params, moms, LR, MOM).cpu().numpy()[0])
    np.testing.assert_array_equal(losses.cpu().numpy().view(np.uint32), np.array(chain, np.float32).view(np.uint32))
    assert torch.equal(params, t.params) and torch.equal(moms, t.moms)
    assert np.isfinite(chain).all() and not torch.equal(params, dev(so.flat(*wide)))


def test_runs_are_bitwise_reproducible(ts, wide):
    import torch
    out = []
    for _ in range(2):
        t, prm, _, _ = make_trainer(ts, wide, 4, 30, 64)
        losses = torch.empty(30, dtype=torch.float32, device="cuda")
        t.run(0, prm, LR, MOM, losses)
        out.append((t.params.clone(), t.moms.clone(), losses.cpu().numpy()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])
    assert np.isfinite(out[0][2]).all() and bool(torch.isfinite(out[0][0]).all()) and bool(torch.isfinite(out[0][1]).all())


def test_it_learns_from_wide_weights(ts, tmp_path, monkeypatch, capsys):
    """800 steps from +-sqrt(6 / fan_in) weights on scenes with noise 0.5, KITTI augmentation defaults: the loss halves and
    the trained nets match better than the initial ones.  (From the reference's initialisation the loss stays at ln 2 on
    such a set: test_train_tr_end_to_end_from_the_references_initialisation.)"""
    import torch
    from mc_cnn_amd import main, train
    monkeypatch.chdir(tmp_path)
    write_synthetic_kitti(str(tmp_path / "data.kitti"), noise=0.5)
    steps = 800
    argv = ["-a", "train_tr", "-seed", "3", "-max_steps", str(steps), "-disp_max", "32"]
    _, _, opt, _ = ts.parse(["kitti", "slow"] + argv)
    init = so.wide_nets(3)
    fname = ts.train("kitti", opt, argv, torch.device("cuda"), data=train.load_data("kitti", opt), init=init)
    losses = ts.last_run["losses"]
    assert losses.size == steps and np.isfinite(losses).all()
    n = steps // 10
    first, last = float(losses[:n].mean()), float(losses[-n:].mean())
    _, _, opt0, _ = ts.parse(["kitti", "slow"] + argv)
    init_fname = ts.save_net(os.path.join("net", "init.t7"), init[0], init[1], opt0)
    capsys.readouterr()
    errs = []
    for f in (fname, init_fname):
        assert main.main(["kitti", "slow", "-a", "test_te", "-net_fname", f, "-disp_max", "32"]) == 0
        errs.append(float(capsys.readouterr().out.strip().splitlines()[-1]))
    print("loss: first tenth %.4f, last tenth %.4f (%.2f x); test_te error: trained %.4f, initial wide nets %.4f"
          % (first, last, last / first, errs[0], errs[1]))
    assert last <= 0.5 * first, (first, last)
    assert errs[0] < errs[1], errs


def test_train_tr_end_to_end_from_the_references_initialisation(ts, tmp_path, monkeypatch, capsys):
    """`main.py kitti slow -a train_tr` from init_net(-seed), the ranges of nn.SpatialConvolution:reset and nn.Linear:reset.
    On this small set the accurate net sits on a plateau from there: its output is a constant and the loss stays within
    0.01 of ln 2 (float32 CPU torch does the same for 5000 steps).  That is expected, and what this test asserts; learning
    is test_it_learns_from_wide_weights."""
    from PIL import Image
    from mc_cnn_amd import binio, main
    monkeypatch.chdir(tmp_path)
    write_synthetic_kitti(str(tmp_path / "data.kitti"))
    steps = 200
    assert main.main(["kitti", "slow", "-a", "train_tr", "-seed", "3", "-max_steps", str(steps), "-disp_max", "32"]) == 0
    out = capsys.readouterr().out.strip().splitlines()
    run = ts.last_run
    losses = run["losses"]
    assert losses.size == steps and np.isfinite(losses).all()
    print("losses %.5f .. %.5f, ln 2 = %.5f" % (losses.min(), losses.max(), math.log(2)))
    assert np.abs(losses - math.log(2)).max() <= 0.01
    # the epoch line (epoch, mean loss, lr, seconds), then `runtime err` per test pair, then the mean
    assert len(out) == 4 and len(out[0].split()) == 4 and out[0].split()[0] == "1" and float(out[0].split()[2]) == 0.003
    assert len(out[1].split()) == 2 and len(out[2].split()) == 2 and 0 <= float(out[3]) <= 1
    fname = run["net_fname"]
    assert fname == os.path.join("net", "net_kitti_slow_-a_train_tr_-seed_3_-max_steps_200_-disp_max_32.t7") and os.path.exists(fname)
    conv, fc = main.load_net(fname, "kitti", "slow"), main.load_fc(fname, "kitti")      # t7.load_reference_net, parsed once
    assert len(conv) == 4 and len(fc) == 5 and conv[1][0].shape == (112, 112, 3, 3) and fc[0][0].shape == (384, 224)
    init_conv, _ = ts.init_net(3)
    assert not np.array_equal(conv[0][0], init_conv[0][0])        # the step moved the weights
    x0 = binio.fromfile(str(tmp_path / "data.kitti" / "x0.bin"))[4, 0, :32, :96]
    x1 = binio.fromfile(str(tmp_path / "data.kitti" / "x1.bin"))[4, 0, :32, :96]
    for name, x in (("l.png", x0), ("r.png", x1)):
        Image.fromarray(np.clip(x * 40 + 128, 0, 255).astype(np.uint8)).save(name)
    assert main.main(["kitti", "slow", "-a", "predict", "-net_fname", fname, "-left", "l.png", "-right", "r.png", "-disp_max", "16"]) == 0
    disp = binio.read_bin("disp.bin", (32, 96))
    assert np.isfinite(disp).all() and os.path.getsize("left.bin") == 16 * 32 * 96 * 4
