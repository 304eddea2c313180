"""GPU: libmctrainslowdepth.so (include/mc_train_slow_depth.h), the accurate net's training step at -l2 1..7 on both image stores:
bit for bit against libmctrainslow.so at (KITTI, 4) and libmctrainmbslow.so at (Middlebury, 3); against float64 torch autograd of
`Net(9, 4, l2)` / `Net(11, 5, l2)` (tests/train_slow_oracle.py) at the shallowest, a middle and the deepest net; `run` against the
chain of the samplers and `step_batch`; bitwise reproducibility; the exact-zero gradient at a saturated output with ONE hidden
Linear; depths and stores interleaved in one process; prediction with 2 and 8 Linears in both -fc_mode; and main.py / hs.py end
to end with -l2.

The numeric tests use the parents' set-up (tests/test_gpu_train_slow.py, tests/test_gpu_train_mb_slow.py): weights from
+-sqrt(6 / fan_in), batches planned by the oracle's selector (tests/train_slow_depth_cases.py), and their bounds: loss 1e-5, each
momenta tensor 1e-4 of its largest magnitude, parameters atol 1e-5."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_slow_depth_cases as cases  # noqa: E402
from train_fixtures import dev, rel, same_bits, small_images, write_synthetic_kitti, write_synthetic_mb  # noqa: E402
from test_gpu_train_mb import small_set  # noqa: E402

pytestmark = pytest.mark.gpu

LR, MOM = 0.003, 0.9


@pytest.fixture(scope="module")
def tsd():
    import torch
    from mc_cnn_amd import train_slow_depth
    assert torch.cuda.is_available()
    return train_slow_depth


def patches_of(dataset, seed, n_pairs):
    ws = cases.TOWER[dataset][0]
    return np.random.default_rng(seed).standard_normal((n_pairs, 3, ws, ws)).astype(np.float32)


# ---- runs on the two stores -------------------------------------------------------------------------------------------------------
def kitti_run(trainer_cls, nets, seed, n_steps, n_pairs, t0=0):
    """n_steps of a Trainer's run on train_fixtures.small_images' store with -hflip 1, as test_gpu_train_slow.make_trainer sets it up."""
    import torch
    from mc_cnn_amd import train_slow
    x0, x1, nnz = small_images(1)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    opt = train_slow.parse(["kitti", "slow", "-a", "train_tr", "-hflip", "1"])[2]
    prm = train_slow.draw_params(rng, opt, n_steps, n_pairs)
    t = trainer_cls(x0, x1, nnz, perm, nets[0], nets[1], n_pairs, torch.device("cuda"))
    losses = torch.empty(n_steps, dtype=torch.float32, device="cuda")
    t.run(t0, dev(prm), LR, MOM, losses)
    torch.cuda.synchronize()
    return t, dict(prm=prm, perm=perm, x0=x0, x1=x1, nnz=nnz), losses.cpu().numpy()


def mb_run(trainer_cls, nets, seed, n_steps, n_pairs, t0=0):
    """n_steps of a Trainer's run on test_gpu_train_mb.small_set's ragged store with -hflip 1 -d_exp 0.5 -d_light 0.5, as
    test_gpu_train_mb_slow.run_steps sets it up."""
    import torch
    from mc_cnn_amd import train_mb, train_mb_slow
    planes, table, index, nnz = small_set(train_mb)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    opt = train_mb_slow.parse(["mb", "slow", "-a", "train_tr", "-hflip", "1", "-d_exp", "0.5", "-d_light", "0.5"])[2]
    prm = train_mb_slow.draw_params(rng, opt, n_steps, n_pairs)
    ids = nnz[perm[t0:t0 + n_steps * n_pairs], 0].reshape(n_steps, n_pairs)
    src = train_mb_slow.draw_sources(rng, opt, ids, index)
    t = trainer_cls(planes, table, nnz, perm, nets[0], nets[1], n_pairs, torch.device("cuda"))
    losses = torch.empty(n_steps, dtype=torch.float32, device="cuda")
    t.run(t0, dev(src), dev(prm), LR, MOM, losses)
    torch.cuda.synchronize()
    return t, dict(prm=prm, src=src, perm=perm), losses.cpu().numpy()


def run_of(tsd, dataset, nets, seed, n_steps, n_pairs, t0=0):
    return (mb_run(tsd.MbTrainer, nets, seed, n_steps, n_pairs, t0) if dataset == "mb" else
            kitti_run(tsd.Trainer, nets, seed, n_steps, n_pairs, t0))


# ---- bit for bit against the parents ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset, l2", [("kitti", 4), ("mb", 3)])
def test_the_parents_depths_equal_the_parents_libraries_bit_for_bit(tsd, dataset, l2):
    """3 steps at n_pairs 5, t0 = 7: parameters, momenta and losses of step_batch and of run."""
    import torch
    from mc_cnn_amd import train_mb_slow, train_slow
    old = train_mb_slow if dataset == "mb" else train_slow
    assert old.NET.l2 == l2
    net, nets = cases.net_of(dataset, l2)
    n_steps, n_pairs, t0 = 3, 5, 7
    state = {}
    for who, step in (("old", old.step_batch), ("new", lambda *a: tsd.step_batch(dataset, l2, *a))):
        params = dev(net.flat(*nets))
        moms = torch.zeros_like(params)
        losses = [step(dev(patches_of(dataset, 50 + s, n_pairs)), params, moms, LR, MOM).cpu().numpy()[0] for s in range(n_steps)]
        state[who] = (params, moms, np.array(losses, np.float32))
    (p0, v0, l0), (p1, v1, l1) = state["old"], state["new"]
    assert same_bits(p0, p1) and same_bits(v0, v1) and np.array_equal(l0.view(np.uint32), l1.view(np.uint32))
    assert np.isfinite(l0).all() and not same_bits(p0, dev(net.flat(*nets))) and bool(v0.any())
    if dataset == "mb":
        a, _, la = mb_run(old.Trainer, nets, 3, n_steps, n_pairs, t0)
        b, _, lb = mb_run(tsd.MbTrainer, nets, 3, n_steps, n_pairs, t0)
    else:
        a, _, la = kitti_run(old.Trainer, nets, 3, n_steps, n_pairs, t0)
        b, _, lb = kitti_run(tsd.Trainer, nets, 3, n_steps, n_pairs, t0)
    assert b.LIB.PREFIX == "mc_train_slow_depth" and a.LIB.PREFIX != b.LIB.PREFIX and a.ws_bytes == b.ws_bytes
    assert same_bits(a.params, b.params) and same_bits(a.moms, b.moms) and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert np.isfinite(la).all() and (la > 0).all() and not same_bits(a.params, dev(net.flat(*nets)))


# ---- against float64 autograd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset, l2, n_pairs", cases.ORACLE_CASES)
def test_one_step_matches_float64_autograd(tsd, dataset, l2, n_pairs):
    import torch
    net, (conv, fc) = cases.net_of(dataset, l2)
    patches, share = cases.sturdy_pairs(dataset, l2, n_pairs)
    print("%s l2 %d n_pairs %d: %.0f %% of the candidates are fragile" % (dataset, l2, n_pairs, 100 * share))
    assert share <= cases.MAX_FRAGILE and patches.shape[0] == n_pairs
    params = dev(net.flat(conv, fc))
    moms = torch.zeros_like(params)
    loss = float(tsd.step_batch(dataset, l2, dev(patches), params, moms, LR, MOM).cpu())
    wp, wv, wl = net.sgd_steps(conv, fc, [patches], LR, MOM)
    got = moms.cpu().numpy()
    print("%s l2 %d n_pairs %d: loss %.7f, float64 %.7f, difference %.2e; relative L2 of all momenta %.2e, worst parameter %.2e"
          % (dataset, l2, n_pairs, loss, wl[0], abs(loss - wl[0]), rel(got, wv), np.abs(params.cpu().numpy() - wp).max()))
    assert abs(loss - wl[0]) <= 1e-5
    assert np.isfinite(got).all() and np.abs(wv).max() > 1e-6
    errs = net.check_per_tensor(got, wv, 1e-4, "%s l2 %d n_pairs %d" % (dataset, l2, n_pairs))
    print("%s l2 %d n_pairs %d: worst tensor %.2e" % (dataset, l2, n_pairs, max(errs.values())))
    assert len(errs) == 2 * (net.L1 + l2 + 1)
    np.testing.assert_allclose(params.cpu().numpy(), wp, rtol=0, atol=1e-5)


# ---- run ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset, l2", [(d, l2) for d in ("kitti", "mb") for l2 in (1, 7)])
def test_run_equals_the_chain_of_sample_and_step(tsd, dataset, l2):
    import torch
    from mc_cnn_amd import train, train_mb
    net, nets = cases.net_of(dataset, l2)
    n_steps, n_pairs, t0 = 3, 5, 7
    t, drawn, losses = run_of(tsd, dataset, nets, 3, n_steps, n_pairs, t0)
    params = dev(net.flat(*nets))
    moms = torch.zeros_like(params)
    for s in range(n_steps):
        rows = dev(drawn["perm"][t0 + s * n_pairs:t0 + (s + 1) * n_pairs])
        if dataset == "mb":
            patches = train_mb.sample(t.planes, t.table, t.nnz, rows, dev(drawn["src"][s]), dev(drawn["prm"][s]))     # libmctrainmb.so's sampler
        else:
            patches = train.sample(t.x0, t.x1, t.nnz, rows, dev(drawn["prm"][s]))                                    # libmctrain.so's sampler
        loss = tsd.step_batch(dataset, l2, patches, params, moms, LR, MOM).cpu().numpy()
        assert loss.view(np.uint32)[0] == losses.view(np.uint32)[s], s
    assert same_bits(params, t.params) and same_bits(moms, t.moms)
    assert np.isfinite(losses).all() and (losses > 0).all() and not same_bits(params, dev(net.flat(*nets)))


@pytest.mark.parametrize("dataset, l2", [("kitti", 7), ("mb", 1)])
def test_runs_are_bitwise_reproducible(tsd, dataset, l2):
    import torch
    _, nets = cases.net_of(dataset, l2)
    a, _, la = run_of(tsd, dataset, nets, 4, 30, 16)
    b, _, lb = run_of(tsd, dataset, nets, 4, 30, 16)
    assert same_bits(a.params, b.params) and same_bits(a.moms, b.moms)
    np.testing.assert_array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert np.isfinite(la).all() and bool(torch.isfinite(a.params).all()) and bool(torch.isfinite(a.moms).all())


# ---- the edges of the depth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dataset", ["kitti", "mb"])
def test_saturated_output_with_one_hidden_linear_gives_an_exactly_zero_gradient(tsd, dataset):
    """l2 = 1, fb2 = +40: o is exactly 1.0f, so Sigmoid's backward gives gh = 0 and the one hidden Linear -- the first, whose
    backward pass is the unmasked one fed by the head -- every gradient after it.  The loss is -log(1e-12f) / 2 and the update is
    v = mom * v, w += v exactly, as in the parents' test."""
    net, (conv, fc) = cases.net_of(dataset, 1)
    rng = np.random.default_rng(5)
    patches = patches_of(dataset, 5, 5)
    p0 = net.flat(conv, fc).copy()
    p0[-1] = 40.0
    v0 = (rng.uniform(0.5, 1.5, p0.size) * rng.choice([-1, 1], p0.size) * 1e-3).astype(np.float32)
    params, moms = dev(p0), dev(v0)
    loss = float(tsd.step_batch(dataset, 1, dev(patches), params, moms, LR, MOM).cpu())
    want = -math.log(float(np.float32(1e-12))) / 2
    print("saturated: loss %.6f, -log(1e-12f) / 2 = %.6f" % (loss, want))
    assert abs(loss - want) <= 1e-5 * want
    v1, p1 = moms.cpu().numpy(), params.cpu().numpy()
    assert np.isfinite(v1).all() and np.isfinite(p1).all()
    want_v = np.float32(MOM) * v0
    np.testing.assert_array_equal(v1.view(np.uint32), want_v.view(np.uint32))
    np.testing.assert_array_equal(p1.view(np.uint32), (p0 + want_v).view(np.uint32))


def test_depths_and_stores_interleaved_give_each_its_own_result(tsd):
    """l2 1, 7, 1 on KITTI's store, then the ragged store between them: every call gives what that (store, depth) gives alone --
    no state of a depth (offsets, workspace layout, a tower's LDS limit) leaks into the next call."""
    import torch

    def step(dataset, l2):
        net, nets = cases.net_of(dataset, l2)
        params = dev(net.flat(*nets))
        moms = torch.zeros_like(params)
        loss = tsd.step_batch(dataset, l2, dev(patches_of(dataset, 9, 3)), params, moms, LR, MOM)
        return params, moms, loss

    alone = {k: step(*k) for k in (("kitti", 7), ("kitti", 1), ("mb", 7), ("mb", 1))}
    assert alone[("kitti", 1)][0].numel() == 426929 and alone[("kitti", 7)][0].numel() == 1313969
    for k in (("kitti", 1), ("kitti", 7), ("kitti", 1), ("mb", 7), ("kitti", 1), ("mb", 1), ("kitti", 7), ("mb", 7)):
        got = step(*k)
        assert all(same_bits(g, w) for g, w in zip(got, alone[k])), k
    assert float(alone[("kitti", 1)][2]) != float(alone[("kitti", 7)][2]) and all(bool(torch.isfinite(v[2]).all()) for v in alone.values())


# ---- prediction ---------------------------------------------------------------------------------------------------------------------
def fc_stack_float64(f, layers, D):
    """main.lua:958-983 in float64: (left, right) volumes (D, H, W), NaN where a disparity has no voxel."""
    C, H, W = f[0].shape
    vl, vr = np.full((D, H, W), np.nan), np.full((D, H, W), np.nan)
    for d in range(min(D, W)):
        n = W - d
        x = np.concatenate([f[0][:, :, d:], f[1][:, :, :n]], 0).reshape(2 * C, H * n).astype(np.float64)
        for i, (w, b) in enumerate(layers):
            x = w.astype(np.float64) @ x + b.astype(np.float64)[:, None]
            x = np.maximum(x, 0) if i < len(layers) - 1 else 1 / (1 + np.exp(-x))
        vl[d, :, d:] = vr[d, :, :n] = x.reshape(H, n)
    return vl, vr


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("l2", [1, 7])
def test_prediction_serves_the_shallowest_and_the_deepest_net(mc, l2, mode):
    """fc.fc_cost_volumes with 2 and 8 Linears at the smallest shape of the FC tests (tests/test_gpu_fc_split.py: C 5, 2 x 60, D 3)
    against a float64 FC stack, with those tests' bars: NaN masks identical, values within 1e-4, outputs not saturated.  With 2
    Linears -fc_mode bf16x3 has no 384 x 384 layer to split.  The hidden layers of the deepest net are drawn from +-sqrt(6 / fan_in),
    as that file's six-hidden-layer case, so that they keep their spread."""
    import torch
    from test_gpu_fc_split import make_layers
    from util import features
    from mc_cnn_amd.fc import fc_cost_volumes
    C, H, W, D = 5, 2, 60, 3
    f = np.maximum(features(C, H, W, seed=C + W), 0) * 3.0
    layers = make_layers(C, l2 - 1, seed=W, hidden_gain=6.0 if l2 > 4 else 1.0)
    assert len(layers) == l2 + 1
    want = fc_stack_float64(f, layers, D)
    dl = [(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()) for w, b in layers]
    got = fc_cost_volumes(torch.from_numpy(f).cuda(), dl, D, mode=mode)
    torch.cuda.synchronize()
    for g, w, name in ((got[0], want[0], "left"), (got[1], want[1], "right")):
        g = g.cpu().numpy()[0]
        assert np.array_equal(np.isnan(g), np.isnan(w)), "%s: NaN mask differs" % name
        ok = ~np.isnan(w)
        err = np.abs(g[ok] - w[ok]).max()
        print("l2 %d %s %s: max |kernel - float64| %.3g, std %.3g" % (l2, mode, name, err, w[ok].std()))
        assert err <= 1e-4, "%s: max |diff| = %g" % (name, err)
        assert w[ok].std() > 1e-3, w[ok].std()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def test_kitti_train_tr_and_the_parameter_search_at_l2_2(tsd, tmp_path, monkeypatch, capsys):
    """`main.py kitti slow -a train_tr -l2 2` trains through libmctrainslowdepth.so, saves a net whose net_te2 has 3 Linears and runs
    test_te on it; `hs.py random kitti slow test_te NET -l2 2 -n 2` then scores two candidates with it.  No learning threshold: from
    the reference's initialisation the accurate net sits on the ln 2 plateau on such a set (README.md)."""
    from mc_cnn_amd import hs, main
    monkeypatch.chdir(tmp_path)
    write_synthetic_kitti(str(tmp_path / "data.kitti"))
    argv = ["kitti", "slow", "-a", "train_tr", "-l2", "2", "-bs", "16", "-epochs", "1", "-max_steps", "40", "-disp_max", "32"]
    assert main.route(argv)[1] is tsd
    assert main.main(argv) == 0
    out = capsys.readouterr().out.strip().splitlines()
    run = tsd.last_run
    assert run["losses"].size == 40 and np.isfinite(run["losses"]).all() and run["epochs"] == 1
    assert len(out) == 4 and out[0].split()[0] == "1" and 0 <= float(out[3]) <= 1          # the epoch line, two test pairs, their mean
    fname = run["net_fname"]
    assert fname == os.path.join("net", "net_kitti_slow_-a_train_tr_-l2_2_-bs_16_-epochs_1_-max_steps_40_-disp_max_32.t7") and os.path.exists(fname)
    conv, fc = main.load_net(fname, "kitti", "slow"), main.load_fc(fname, "kitti")
    assert len(conv) == 4 and [w.shape for w, _ in fc] == [(384, 224), (384, 384), (1, 384)]
    init_conv, init_fc = tsd.net_shape("kitti", 2).init_net(42)
    assert not np.array_equal(conv[0][0], init_conv[0][0]) and not np.array_equal(fc[1][0], init_fc[1][0])      # the steps moved the weights
    assert main.main(["kitti", "slow", "-a", "test_te", "-net_fname", fname, "-disp_max", "32", "-fc_mode", "bf16x3", "-conv_mode", "bf16x3"]) == 0
    assert 0 <= float(capsys.readouterr().out.strip().splitlines()[-1]) <= 1
    assert hs.main(["random", "kitti", "slow", "test_te", fname, "-l2", "2", "-n", "2", "-disp_max", "32", "-log", "hs.log"]) == 0
    lines = [l for l in capsys.readouterr().out.strip().splitlines() if not l.startswith("evalset:")]      # one result line per candidate
    assert len(lines) == 2 and all(l.endswith("-net_fname " + fname) and 0 <= float(l.split()[0]) <= 1 for l in lines)
    assert open("hs.log").read().strip().splitlines() == lines


def test_mb_train_tr_at_l2_1(tsd, tmp_path, monkeypatch, capsys):
    """`main.py mb slow -a train_tr -l2 1 -data_dir mbdata`: the shallowest net on the ragged store, saved with 2 Linears, then
    test_te on it."""
    from mc_cnn_amd import main
    import train_mb_oracle as mo
    monkeypatch.chdir(tmp_path)
    write_synthetic_mb(str(tmp_path / "mbdata"))
    argv = ["mb", "slow", "-a", "train_tr", "-l2", "1", "-bs", "16", "-epochs", "1", "-max_steps", "40", "-data_dir", "mbdata"]
    assert main.route(argv)[1] is tsd
    assert main.main(argv) == 0
    out = capsys.readouterr().out.strip().splitlines()
    run = tsd.last_run
    assert run["losses"].size == 40 and np.isfinite(run["losses"]).all() and run["epochs"] == 1
    n_ex = len(mo.SCENE_TE) + 2
    assert len(out) == 1 + n_ex + 1 and out[0].split()[0] == "1" and 0 <= float(out[-1]) <= 1
    fname = run["net_fname"]
    assert fname == os.path.join("net", "net_mb_slow_-a_train_tr_-l2_1_-bs_16_-epochs_1_-max_steps_40_-data_dir_mbdata.t7") and os.path.exists(fname)
    conv, fc = main.load_net(fname, "mb", "slow"), main.load_fc(fname, "mb")
    assert len(conv) == 5 and [w.shape for w, _ in fc] == [(384, 224), (1, 384)]
    init_conv, init_fc = tsd.net_shape("mb", 1).init_net(42)
    assert not np.array_equal(conv[0][0], init_conv[0][0]) and not np.array_equal(fc[0][0], init_fc[0][0])
    assert main.main(["mb", "slow", "-a", "test_te", "-data_dir", "mbdata", "-net_fname", fname, "-fc_mode", "bf16x3"]) == 0
    assert 0 <= float(capsys.readouterr().out.strip().splitlines()[-1]) <= 1
