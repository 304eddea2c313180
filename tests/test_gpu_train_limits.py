"""GPU: libmctrain.so's training entry points (include/mc_train.h) at their edges -- run offsets into the permutation and
the parameter draws, batch sizes from 1 to MC_TRAIN_MAX_PAIRS, the fixed-order reduction, exact and degenerate states, the
sampler at image borders and past 2^31 elements, every refusal -- against the float64 oracles of tests/train_oracle.py, and
the oracle's tail (Normalize2, StereoJoin1, Margin2) against the reference's own kernels.

Per-tensor gradient checks at every step need pairs on which fp32 and float64 agree about every ReLU mask: pairs with a
pre-activation (or hinge argument) within 3e-6 of 0 in the FLOAT64 forward pass are left out before the GPU is touched
(`select`); the kernel's output never takes part in the selection."""
import functools
import math
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_oracle as to  # noqa: E402
import train_fixtures  # noqa: E402
from train_fixtures import bits, dev, same_bits  # noqa: E402

small_images = functools.partial(train_fixtures.small_images, noise=1.5)   # strong enough to leave most hinges of a random net active

pytestmark = pytest.mark.gpu

MC_EINVAL = -22
NAN = float("nan")
AUGMENT = ["-hflip", "1", "-vflip", "1", "-trans", "2", "-scale", "0.8", "-d_vtrans", "1", "-d_rotate", "3", "-d_hscale", "0.9",
           "-d_hshear", "0.3", "-d_contrast", "1.1"]


@pytest.fixture(scope="module")
def tr():
    import torch
    from mc_cnn_amd import train
    assert torch.cuda.is_available()
    return train


def opt_of(*flags):
    from mc_cnn_amd import main
    return main.parse(["kitti", "fast", "-a", "train_tr"] + list(flags))[2]


def poisoned_workspace(tr, n_pairs):
    """exactly mc_train_workspace_bytes(n_pairs) bytes of NaN"""
    import torch
    need = tr.tl.load().mc_train_workspace_bytes(n_pairs)
    assert need == (n_pairs * tr.tl.NPARAMS + n_pairs) * 4
    return torch.full((need // 4,), NAN, dtype=torch.float32, device="cuda")


# ---- (a) mc_train_run is the chain sample -> step_batch at every step, for any offset ------------------------------------
def raw_run(t, t0, n_steps, prm, losses, n_perm=None):
    """mc_train_run with n_steps and n_perm given explicitly (Trainer.run derives them); returns rc"""
    from mc_cnn_amd.train import _p, _stream
    return t.lib.mc_train_run(_p(t.x0), _p(t.x1), t.n_img, t.H, t.W, _p(t.nnz), t.nnz.shape[0], _p(t.perm),
                              t.perm.shape[0] if n_perm is None else n_perm, t0, n_steps, t.n_pairs, _p(prm), _p(t.params), _p(t.moms),
                              0.002, 0.9, 0.2, 1, _p(losses), t.ws.data_ptr(), t.ws_bytes, _stream())


@pytest.mark.parametrize("n_pairs", [1, 3, 64])
def test_run_equals_the_chain_of_sample_and_step(tr, n_pairs):
    import torch
    x0, x1, nnz = small_images(1)
    rng = np.random.default_rng(40 + n_pairs)
    n_steps, t0 = 5, 7
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    prm = dev(tr.draw_params(rng, opt_of("-hflip", "1", "-vflip", "1", "-d_vtrans", "1", "-d_hshear", "0.2"), n_steps, n_pairs))
    assert (prm[..., 2] < 0).any() and (prm[..., 3] < 0).any()
    layers = to.random_layers(8)
    t = tr.Trainer(x0, x1, nnz, perm, layers, n_pairs, torch.device("cuda"))
    t.ws = poisoned_workspace(tr, n_pairs)
    losses = torch.full((n_steps + 1,), -123.25, dtype=torch.float32, device="cuda")
    t.run(t0, prm, 0.002, 0.9, 0.2, 1, losses)
    torch.cuda.synchronize()
    # the chain, with tensors of its own
    x0d, x1d, nnzd, permd = dev(x0), dev(x1), dev(nnz), dev(perm)
    params, moms = dev(to.flat(layers)), torch.zeros(tr.tl.NPARAMS, device="cuda")
    want = []
    for s in range(n_steps):
        rows = permd[t0 + s * n_pairs: t0 + (s + 1) * n_pairs].contiguous()
        patches = tr.sample(x0d, x1d, nnzd, rows, prm[s].contiguous())
        want.append(tr.step_batch(patches, params, moms, 0.002, 0.9, 0.2, 1, poisoned_workspace(tr, n_pairs)))
    want = torch.cat(want)
    got = losses.cpu().numpy()
    print("n_pairs %d: losses of the run %s, of the chain %s" % (n_pairs, got[:n_steps], want.cpu().numpy()))
    assert np.isfinite(got).all()
    assert same_bits(losses[:n_steps], want)
    assert got[n_steps] == -123.25                       # one loss per step, nothing after them
    assert same_bits(t.params, params) and same_bits(t.moms, moms)
    assert len(set(got[:n_steps][got[:n_steps] > 0].tolist())) >= 3   # the steps differ, so an offset error cannot hide

    # n_steps = 0 changes nothing
    p0, v0, l0 = t.params.clone(), t.moms.clone(), losses.clone()
    assert raw_run(t, t0, 0, prm, losses) == 0
    torch.cuda.synchronize()
    assert same_bits(t.params, p0) and same_bits(t.moms, v0) and same_bits(losses, l0)


def test_run_takes_the_last_legal_offset_and_refuses_one_more(tr):
    import torch
    x0, x1, nnz = small_images(2, n_img=1, H=12, W=20)
    n_pairs, n_steps = 3, 2
    n_perm = 17
    perm = np.random.default_rng(0).permutation(nnz.shape[0]).astype(np.int32)[:n_perm]
    t = tr.Trainer(x0, x1, nnz, perm, to.random_layers(8), n_pairs, torch.device("cuda"))
    prm = dev(tr.draw_params(np.random.default_rng(1), opt_of(), n_steps, n_pairs))
    losses = torch.full((n_steps,), NAN, dtype=torch.float32, device="cuda")
    t0 = n_perm - n_steps * n_pairs
    assert raw_run(t, t0, n_steps, prm, losses) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and torch.isfinite(t.params).all()
    # the same steps through the chain: rows perm[11:14], perm[14:17]
    params, moms = dev(to.flat(to.random_layers(8))), torch.zeros(tr.tl.NPARAMS, device="cuda")
    for s in range(n_steps):
        rows = t.perm[t0 + s * n_pairs: t0 + (s + 1) * n_pairs].contiguous()
        loss = tr.step_batch(tr.sample(t.x0, t.x1, t.nnz, rows, prm[s].contiguous()), params, moms, 0.002, 0.9, 0.2, 1)
        assert same_bits(loss, losses[s:s + 1])
    assert same_bits(params, t.params)
    p0 = t.params.clone()
    losses.fill_(NAN)
    assert raw_run(t, t0 + 1, n_steps, prm, losses) == MC_EINVAL
    msg = t.lib.mc_train_last_error().decode()
    assert "permutation" in msg and "[12, 18)" in msg and "17 rows" in msg, msg
    torch.cuda.synchronize()
    assert torch.isnan(losses).all() and same_bits(t.params, p0)


# ---- (b) the fragile-pair filter ----------------------------------------------------------------------------------------------
def select(pool, layers, n, margin, what):
    """The first n pairs of `pool` (m, 3, 9, 9) that are not fragile in the float64 forward pass with `layers`
    (to.hinge_and_fragility: some |pre-activation| of layers 1-3, or the hinge argument, below 3e-6).  Fails if more than a
    quarter of the pool is fragile.  Returns the pairs, their hinge arguments and their places in the pool."""
    f, fragile = to.hinge_and_fragility(layers, pool, margin)
    share = float(fragile.mean())
    print("%s: %d of %d candidate pairs fragile (%.1f %%)" % (what, int(fragile.sum()), pool.shape[0], 100 * share))
    assert share <= 0.25, "%s: %.1f %% of the candidates discarded" % (what, 100 * share)
    keep = np.nonzero(~fragile)[0][:n]
    assert keep.size == n
    return pool[keep], f[keep], keep


def pool_size(n):
    return max(256, int(math.ceil(n / 0.75)))


def plan_steps(draw, layers, n_pairs, n_steps, lr, mom, margin, pow_, what, moms=None):
    """Batches for n_steps consecutive steps, each selected against the float64 oracle's own trajectory (fp32 state):
    no GPU involved.  draw(m) -> (m, 3, 9, 9) float32 candidates."""
    p = to.flat(layers)
    v = np.zeros_like(p) if moms is None else np.asarray(moms, np.float32)
    batches = []
    for k in range(n_steps):
        b, _, _ = select(draw(pool_size(n_pairs)), to.unflat(p), n_pairs, margin, "%s step %d" % (what, k))
        batches.append(b)
        p, v, _ = to.sgd_steps(to.unflat(p), [b], lr, mom, margin, pow_, fp32_state=True, moms=v)
        p, v = p.astype(np.float32), v.astype(np.float32)
    return batches


def check_step(params, moms, ws, loss, p0, v0, b, lr, mom, margin, pow_, what):
    """The state a kernel step left against float64 autograd of one step on batch b from the fp32 state (p0, v0): loss,
    parameters and momenta to 1e-5 absolute, the momenta of each tensor to 1e-4 of that tensor's largest; everything,
    the NaN-filled workspace included, finite."""
    import torch
    gp, gv = params.cpu().numpy(), moms.cpu().numpy()
    wp, wv, wl = to.sgd_steps(to.unflat(p0), [b], lr, mom, margin, pow_, moms=v0)
    print("%s: loss %.7f (float64 %.7f), max |params - float64| %.2e, max |momenta - float64| %.2e" % (
        what, loss, wl[0], np.abs(gp - wp).max(), np.abs(gv - wv).max()))
    assert math.isfinite(loss) and np.isfinite(gp).all() and np.isfinite(gv).all(), what
    assert bool(torch.isfinite(ws).all()), "%s: the step left part of its workspace unwritten" % what
    assert abs(loss - wl[0]) <= 1e-5, (what, loss, wl[0])
    np.testing.assert_allclose(gp, wp, rtol=0, atol=1e-5)
    np.testing.assert_allclose(gv, wv, rtol=0, atol=1e-5)
    to.check_per_tensor(gv, wv, 1e-4, what)


def run_checked_steps(tr, layers, batches, lr, mom, margin, pow_, what):
    """Every batch through mc_train_step_batch on a NaN-filled workspace of exactly the documented size, each step checked
    by check_step."""
    import torch
    params = dev(to.flat(layers))
    moms = torch.zeros_like(params)
    ws = poisoned_workspace(tr, batches[0].shape[0])
    for k, b in enumerate(batches):
        p0, v0 = params.cpu().numpy(), moms.cpu().numpy()
        ws.fill_(NAN)
        loss = float(tr.step_batch(dev(b), params, moms, lr, mom, margin, pow_, ws).cpu())
        check_step(params, moms, ws, loss, p0, v0, b, lr, mom, margin, pow_, "%s step %d" % (what, k))


def normal_patches(rng):
    return lambda m: rng.standard_normal((m, 3, 9, 9)).astype(np.float32)


# ---- (c) batch sizes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("n_pairs", [1, 2, 3, 65, 257])
def test_batch_sizes_match_autograd_per_tensor_at_every_step(tr, n_pairs, pow_):
    rng = np.random.default_rng(1000 * pow_ + n_pairs)
    layers = to.random_layers(5)
    what = "%d pairs, pow %d" % (n_pairs, pow_)
    batches = plan_steps(normal_patches(rng), layers, n_pairs, 3, 0.002, 0.9, 0.2, pow_, what)
    run_checked_steps(tr, layers, batches, 0.002, 0.9, 0.2, pow_, what)


# ---- (d) the reduction over the pairs runs in pair order --------------------------------------------------------------------
@pytest.mark.parametrize("N,pow_", [(64, 1), (64, 2), (4096, 1)])
def test_gradients_are_summed_in_pair_order(tr, N, pow_):
    """With lr = 1, mom = 0 and zero momenta a step leaves moms = -g.  Each pair alone gives g_i; the N-pair step scales each
    pair's gradient by 1/N (exact for a power of two) and must give the float32 sum of g_i / N over i = 0, 1, ... in that
    order, bit for bit."""
    import torch
    assert N & (N - 1) == 0
    rng = np.random.default_rng(N + pow_)
    layers = to.random_layers(21)
    b = rng.standard_normal((N, 3, 9, 9)).astype(np.float32)
    bd = dev(b)
    fresh = dev(to.flat(layers))
    NP = tr.tl.NPARAMS
    G = torch.empty((N, NP), dtype=torch.float32, device="cuda")
    params, moms, ws1 = fresh.clone(), torch.zeros(NP, device="cuda"), poisoned_workspace(tr, 1)
    t_start = time.perf_counter()
    for i in range(N):
        params.copy_(fresh)
        moms.zero_()
        tr.step_batch(bd[i:i + 1], params, moms, 1.0, 0.0, 0.2, pow_, ws1)
        torch.neg(moms, out=G[i])
    torch.cuda.synchronize()
    t_single = time.perf_counter() - t_start
    assert torch.isfinite(G).all()
    params.copy_(fresh)
    moms.zero_()
    ws = poisoned_workspace(tr, N)
    loss = float(tr.step_batch(bd, params, moms, 1.0, 0.0, 0.2, pow_, ws).cpu())
    assert torch.isfinite(ws).all()
    inv = 1.0 / N
    acc = torch.zeros(NP, device="cuda")
    tiny = torch.zeros(NP, dtype=torch.bool, device="cuda")
    for i in range(N):
        gi = G[i] * inv                                   # exact: a power of two
        tiny |= (gi != 0) & (gi.abs() < 2.0 ** -100)
        acc = acc + gi                                    # one float32 add per pair, in pair order
    want = torch.zeros(NP, device="cuda") - acc           # the kernel's 0 * 0 - 1 * g
    share = float(tiny.float().mean())
    differ = (bits(moms) != bits(want)) & ~tiny
    n_differ = int(differ.sum())
    err = float((moms - want).abs().max())
    print("N %d pow %d: %d of %d elements differ from the ordered float32 sum (max |difference| %.3e); %.2e of the elements "
          "have a term below 2^-100; %d single-pair steps took %.1f s" % (N, pow_, n_differ, NP, err, share, N, t_single))
    assert share < 1e-4
    assert float((moms - want)[tiny].abs().max()) <= 1e-12 if bool(tiny.any()) else True
    assert n_differ == 0
    assert same_bits(params, fresh + moms)
    assert float(moms.abs().max()) > 1e-4                 # a gradient was there to be summed
    # the same sum in any other order is a different float32 number somewhere: the comparison can tell orders apart
    rev = torch.zeros(NP, device="cuda")
    for i in reversed(range(N)):
        rev = rev + G[i] * inv
    assert int((bits(rev) != bits(acc)).sum()) > 0
    # the loss of the large batch against float64
    with torch.no_grad():
        chunk = min(N, 512)
        want_loss = float(np.mean([float(to.loss_of(to.as_f64(layers), torch.tensor(b[i:i + chunk].astype(np.float64)), 0.2, pow_))
                                   for i in range(0, N, chunk)]))
    print("N %d pow %d: loss %.7f, float64 %.7f" % (N, pow_, loss, want_loss))
    assert abs(loss - want_loss) <= 1e-5


# ---- (e) exact and degenerate states -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pow_", [1, 2])
def test_inactive_hinges_leave_only_the_momentum(tr, pow_):
    """positive = left for every pair and negatives whose score is below the positive's by more than the margin (chosen by
    the float64 forward pass): every hinge is inactive, the gradient is exactly 0, so v = fl(mom * v), w = fl(w + v)."""
    import torch
    rng = np.random.default_rng(70 + pow_)
    layers = to.random_layers(9)
    n_pairs, mom = 32, 0.9
    pool = rng.standard_normal((256, 3, 9, 9)).astype(np.float32)
    pool[:, 1] = pool[:, 0]
    f, _ = to.hinge_and_fragility(layers, pool, 0.2)
    keep = np.nonzero(f < -1e-3)[0][:n_pairs]
    print("pow %d: %d of %d candidates have f < -1e-3 (f in [%.3f, %.3f])" % (pow_, int((f < -1e-3).sum()), f.size, f.min(), f.max()))
    assert keep.size == n_pairs
    b = pool[keep]
    params = dev(to.flat(layers))
    moms = dev((rng.standard_normal(tr.tl.NPARAMS) * 1e-3).astype(np.float32))
    p0, v0 = params.clone(), moms.clone()
    ws = poisoned_workspace(tr, n_pairs)
    loss = tr.step_batch(dev(b), params, moms, 0.002, mom, 0.2, pow_, ws).cpu().numpy()
    assert torch.isfinite(ws).all()
    assert loss[0] == 0.0
    want_v = v0 * torch.tensor(mom, dtype=torch.float32, device="cuda")
    assert same_bits(moms, want_v) and same_bits(params, p0 + want_v)
    assert not same_bits(params, p0)


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("case", ["zero_patches", "positive_is_negative", "zero_last_layer"])
def test_states_whose_gradient_vanishes(tr, case, pow_):
    """Three states where pos == neg identically, so the loss is the margin's (0.2, or 0.02 for pow 2) and the gradient is
    0 in exact arithmetic (float64 autograd leaves its own rounding, up to 1.3e-17 measured)."""
    import torch
    rng = np.random.default_rng(80)
    layers = to.random_layers(10)
    n_pairs = 16
    b = rng.standard_normal((n_pairs, 3, 9, 9)).astype(np.float32)
    if case == "zero_patches":
        b[:] = 0
    elif case == "positive_is_negative":
        b[:, 2] = b[:, 1]
    else:
        layers = layers[:3] + [(np.zeros_like(layers[3][0]), np.zeros_like(layers[3][1]))]
    _, wv, wl = to.sgd_steps(layers, [b], 0.002, 0.9, 0.2, pow_)
    want_loss = 0.2 if pow_ == 1 else 0.02
    # float64 itself: the loss is the margin's, and what autograd leaves of the gradient is float64 rounding of O(1) terms
    print("%s pow %d: float64 loss %.17g, largest float64 gradient %.2e" % (case, pow_, wl[0], np.abs(wv).max() / 0.002))
    assert abs(wl[0] - want_loss) <= 1e-15 and np.abs(wv).max() <= 0.002 * 1e-14
    params = dev(to.flat(layers))
    moms = torch.zeros_like(params)
    ws = poisoned_workspace(tr, n_pairs)
    loss = float(tr.step_batch(dev(b), params, moms, 0.002, 0.9, 0.2, pow_, ws).cpu())
    worst = float(moms.abs().max())
    print("%s pow %d: loss %.8f, max |momentum| %.3e" % (case, pow_, loss, worst))
    assert torch.isfinite(ws).all() and torch.isfinite(params).all() and torch.isfinite(moms).all()
    assert abs(loss - want_loss) <= 1e-6
    assert worst <= 1e-7


@pytest.mark.parametrize("margin", [0.0, -0.5, 5.0])
def test_margins_match_autograd(tr, margin):
    rng = np.random.default_rng(90)
    layers = to.random_layers(11)
    for pow_ in (1, 2):
        what = "margin %g, pow %d" % (margin, pow_)
        batches = plan_steps(normal_patches(rng), layers, 24, 3, 0.002, 0.9, margin, pow_, what)
        run_checked_steps(tr, layers, batches, 0.002, 0.9, margin, pow_, what)


def textured_images(seed, n_img=2, H=40, W=80, d=5, noise=0.3):
    """Smooth textures (a pixel's neighbours a few columns away still resemble it); the right view is the left one shifted
    by d, plus noise.  nnz lists the pixels whose patches lie inside both views."""
    rng = np.random.default_rng(seed)
    k = np.ones(3) / 3
    r = rng.standard_normal((n_img, H, W))
    for axis in (1, 2):
        r = np.apply_along_axis(lambda v: np.convolve(v, k, "same"), axis, r)
    x0 = (r / r.std()).astype(np.float32)
    x1 = (np.roll(x0, -d, axis=2) + noise * rng.standard_normal(x0.shape)).astype(np.float32)
    ys, xs = np.meshgrid(np.arange(8, H - 8), np.arange(d + 12, W - 12), indexing="ij")
    nnz = np.concatenate([np.stack([np.full(ys.size, i + 1), ys.ravel(), xs.ravel(), np.full(ys.size, d)], 1) for i in range(n_img)])
    return x0, x1, nnz.astype(np.float32)


FALSE, NOISE = (1, 1), 0.5     # the negatives' distance from the match in columns; the right view's noise


def plan_trained_state(draw_params, n_pairs, n_steps, lr, mom, margin):
    """No GPU here.  200 float64 steps (fp32 state) on windows cut from textured images -- left, its match in the right view,
    and the right view 2 or 3 columns off the match -- then, from that state, n_steps batches of pairs for the sampler,
    selected against the oracle's own trajectory on the restatement's patches."""
    rng = np.random.default_rng(123)
    layers = to.random_layers(12)
    x0, x1, nnz = textured_images(5, noise=NOISE)
    d = 5

    def windows(m):
        out = np.empty((m, 3, 9, 9), np.float32)
        for j, r in enumerate(rng.integers(0, nnz.shape[0], m)):
            i, y, x = int(nnz[r, 0]) - 1, int(nnz[r, 1]), int(nnz[r, 2])
            off = int(rng.choice([-1, 1])) * int(rng.integers(FALSE[0], FALSE[1] + 1))
            out[j, 0] = x0[i, y - 4:y + 5, x - 4:x + 5]
            out[j, 1] = x1[i, y - 4:y + 5, x - d - 4:x - d + 5]
            out[j, 2] = x1[i, y - 4:y + 5, x - d + off - 4:x - d + off + 5]
        return out
    p, v, wl = to.sgd_steps(layers, [windows(n_pairs) for _ in range(200)], lr, mom, margin, 1, fp32_state=True)
    p, v = p.astype(np.float32), v.astype(np.float32)
    print("200 float64 steps: mean loss of the first ten %.4f, of the last ten %.4f" % (np.mean(wl[:10]), np.mean(wl[-10:])))
    trained = (p.copy(), v.copy())
    m = 2 * n_pairs                                        # candidates per step: the restatement's sampler is slow
    cand = rng.permutation(nnz.shape[0])[:n_steps * m].astype(np.int32)
    prm_all = draw_params(rng, opt_of("-rotate", "0", "-hshear", "0", "-trans", "1", "-false1", str(FALSE[0]), "-false2", str(FALSE[1])),
                          n_steps, m)
    assert (prm_all[..., 4] == 0).all() and (prm_all[..., 12] == 0).all()     # no rotation: the sampler is exact
    perm, prm, batches, inactive = [], [], [], 0
    for k in range(n_steps):
        rows = cand[k * m:(k + 1) * m]
        pool = np.stack([to.sample_pair(x0, x1, nnz[r], prm_all[k, i]) for i, r in enumerate(rows)])
        b, f, keep = select(pool, to.unflat(p), n_pairs, margin, "trained state, step %d" % k)
        inactive += int((f <= 0).sum())
        perm.append(rows[keep])
        prm.append(prm_all[k, keep])
        batches.append(b)
        p, v, _ = to.sgd_steps(to.unflat(p), [b], lr, mom, margin, 1, fp32_state=True, moms=v)
        p, v = p.astype(np.float32), v.astype(np.float32)
    share = inactive / float(n_steps * n_pairs)
    print("trained state: %.1f %% of the chosen pairs' hinges are inactive" % (100 * share))
    assert 0.25 <= share <= 0.75
    return (x0, x1, nnz), trained, np.concatenate(perm), np.stack(prm), batches


def test_a_trained_state_on_sampled_patches(tr):
    """A state in which part of the hinges is inactive, and from it three steps of mc_train_run -- which samples its
    patches itself -- against float64 autograd on the restatement's patches."""
    import torch
    n_pairs, n_steps, lr, mom, margin = 32, 3, 0.002, 0.9, 0.2
    (x0, x1, nnz), (p_tr, v_tr), perm, prm, batches = plan_trained_state(tr.draw_params, n_pairs, n_steps, lr, mom, margin)
    t = tr.Trainer(x0, x1, nnz, perm, to.unflat(p_tr), n_pairs, torch.device("cuda"))
    t.moms.copy_(dev(v_tr))
    t.ws = poisoned_workspace(tr, n_pairs)
    prm_d = dev(prm)
    losses = torch.full((n_steps,), NAN, dtype=torch.float32, device="cuda")
    for k in range(n_steps):
        p0, v0 = t.params.cpu().numpy(), t.moms.cpu().numpy()
        t.ws.fill_(NAN)
        t.run(k * n_pairs, prm_d[k:k + 1].contiguous(), lr, mom, margin, 1, losses[k:])
        check_step(t.params, t.moms, t.ws, float(losses[k].cpu()), p0, v0, batches[k], lr, mom, margin, 1, "trained state step %d" % k)


# ---- (f) the sampler ---------------------------------------------------------------------------------------------------------------
def ulps(a, b):
    """distance in float32 steps, per element"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def check_sampler(tr, x0, x1, nnz, prm, what, x0_host=None, x1_host=None, nnz_host=None):
    """mc_train_sample on every row of nnz with prm against the restatement: 1e-5 everywhere, bit for bit where neither
    patch is rotated (phi == phi_ == 0: then kernel and restatement run the same IEEE operations in the same order)."""
    n = nnz.shape[0]
    got = tr.sample(x0, x1, dev(nnz), dev(np.arange(n, dtype=np.int32)), dev(prm)).cpu().numpy()
    x0h, x1h, nnzh = (x0.cpu().numpy() if x0_host is None else x0_host, x1.cpu().numpy() if x1_host is None else x1_host,
                      nnz if nnz_host is None else nnz_host)
    exact = (prm[:, 4] == 0) & (prm[:, 12] == 0)
    worst, worst_ulp, n_differ = 0.0, 0, 0
    bad = []
    for i in range(n):
        want = to.sample_pair(x0h, x1h, nnzh[i], prm[i])
        worst = max(worst, float(np.abs(got[i] - want).max()))
        if exact[i]:
            u = int(ulps(got[i], want).max())
            differ = not np.array_equal(got[i].view(np.uint32), want.view(np.uint32))
            worst_ulp, n_differ = max(worst_ulp, u), n_differ + differ
            if differ:
                bad.append(i)
    print("%s: %d pairs, max |kernel - restatement| %.3e; of the %d unrotated pairs %d differ in some bit (largest distance %d ulp)" % (
        what, n, worst, int(exact.sum()), n_differ, worst_ulp))
    assert np.isfinite(got).all()
    assert worst <= 1e-5, what
    assert n_differ == 0, (what, bad[:10])
    return got


def augmented_params(tr, rng, n):
    prm = tr.draw_params(rng, opt_of(*AUGMENT), 1, n)[0]
    prm[::3, 4] = prm[::3, 12] = 0                       # a third of the pairs unrotated
    assert (prm[:, 2] < 0).any() and (prm[:, 3] < 0).any() and (prm[:, 1] < 0).any() and (prm[:, 1] > 0).any()
    assert (prm[:, 10] != prm[:, 2]).all() and (prm[:, 14] != prm[:, 6]).any() and (prm[:, 15] != prm[:, 7]).all()
    assert (prm[:, 17] != prm[:, 9]).all() and (prm[1::3, 12] != prm[1::3, 4]).all() and (prm[:, 5] != 0).all()
    return prm


def test_sampler_at_the_borders_of_full_size_images(tr):
    import torch
    rng = np.random.default_rng(31)
    n_img, H, W = 3, 350, 1242
    x0 = torch.from_numpy(rng.standard_normal((n_img, H, W)).astype(np.float32)).cuda()
    x1 = torch.from_numpy(rng.standard_normal((n_img, H, W)).astype(np.float32)).cuda()
    n = 510
    rows = []
    for k in range(n):
        kind = k % 10
        y, x = int(rng.integers(5, H - 5)), int(rng.integers(5, W - 5))
        d = float(rng.uniform(0.6, 228))
        if kind < 4:                                      # the corners
            y, x = (0, H - 1)[kind & 1], (0, W - 1)[kind >> 1]
        elif kind < 8:                                    # the edges
            if kind < 6:
                y = (0, H - 1)[kind & 1]
            else:
                x = (0, W - 1)[kind & 1]
        elif kind == 9:                                   # a disparity larger than the column: the right patches leave the image
            d = x + float(rng.uniform(3, 60))
        rows.append((1 + k % n_img, y, x, d))
    nnz = np.array(rows, np.float32)
    assert (nnz[:, 3] > nnz[:, 2]).sum() >= 50
    prm = augmented_params(tr, rng, n)
    got = check_sampler(tr, x0, x1, nnz, prm, "350 x 1242")
    far = (nnz[:, 3] > nnz[:, 2] + 30)
    # right patches far outside the image are 0 * contrast + brightness; left ones inside are not constant
    for i in np.nonzero(far)[0]:
        assert (got[i, 1] == np.float32(0) * prm[i, 17] + prm[i, 16]).all() and got[i, 0].std() > 0


def test_sampler_reads_zero_for_rows_and_images_out_of_range(tr):
    rng = np.random.default_rng(32)
    n_img, H, W = 2, 20, 30
    x0 = rng.standard_normal((n_img, H, W)).astype(np.float32)
    x1 = rng.standard_normal((n_img, H, W)).astype(np.float32)
    nnz = np.array([[1, 10, 15, 3], [0, 10, 15, 3], [n_img + 1, 10, 15, 3], [2, 9, 14, 2], [-1, 10, 15, 3]], np.float32)
    rows = np.array([0, -1, nnz.shape[0], 1, 2, 3, 4, -2 ** 31, 2 ** 31 - 1], np.int32)
    prm = augmented_params(tr, rng, rows.size)
    got = tr.sample(dev(x0), dev(x1), dev(nnz), dev(rows), dev(prm)).cpu().numpy()
    for i, r in enumerate(rows):
        if r in (0, 3):
            np.testing.assert_allclose(got[i], to.sample_pair(x0, x1, nnz[r], prm[i]), rtol=0, atol=1e-5)
            assert got[i, 0].std() > 0
        else:
            assert (got[i, 0] == np.float32(0) * prm[i, 9] + prm[i, 8]).all(), (i, r)
            assert (got[i, 1:] == np.float32(0) * prm[i, 17] + prm[i, 16]).all(), (i, r)


def test_sampler_on_the_smallest_images(tr):
    rng = np.random.default_rng(33)
    x0 = rng.standard_normal((2, 4, 4)).astype(np.float32)
    x1 = rng.standard_normal((2, 4, 4)).astype(np.float32)
    nnz = np.array([(1 + k % 2, y, x, d) for k, (y, x) in enumerate((y, x) for y in range(4) for x in range(4)) for d in (0.75, 2)],
                   np.float32)
    prm = augmented_params(tr, rng, nnz.shape[0])
    prm[:, 5:7] = rng.uniform(-0.9, 0.9, (nnz.shape[0], 2))       # keep the 4 x 4 image under the patch
    prm[:, 13] = prm[:, 5]
    got = check_sampler(tr, dev(x0), dev(x1), nnz, prm, "4 x 4")
    assert (got[:, 0].std((1, 2)) > 0).all()


def test_sampler_past_2_to_the_31_elements(tr):
    """9 images of 17000 x 17000 (10.4 GB, generated on the device, x0 and x1 the same tensor); the pairs lie in the last
    image, whose first element is 2.3e9 floats in."""
    import torch
    n_img, H, W = 9, 17000, 17000
    assert (n_img - 1) * H * W > 2 ** 31
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.empty((n_img, H, W), dtype=torch.float32, device="cuda")
    for i in range(n_img):
        x[i].normal_(generator=g)
    last = x[n_img - 1].cpu().numpy()
    rng = np.random.default_rng(34)
    pos = [(0, 0), (H - 1, W - 1), (H - 1, 0), (0, W - 1), (H - 1, 9000), (8000, W - 1)] + \
        [(int(rng.integers(0, H)), int(rng.integers(300, W))) for _ in range(18)]
    nnz = np.array([(n_img, y, x_, float(rng.uniform(0.6, 228))) for y, x_ in pos], np.float32)
    prm = augmented_params(tr, rng, nnz.shape[0])
    host_rows = nnz.copy()
    host_rows[:, 0] = 1
    got = check_sampler(tr, x, x, nnz, prm, "9 x 17000 x 17000", x0_host=last[None], x1_host=last[None], nnz_host=host_rows)
    assert (got[6:, 0].std((1, 2)) > 0).all()
    del x


# ---- (g) refusals -------------------------------------------------------------------------------------------------------------------
SIG = {
    "mc_train_sample": ["x0", "x1", "n_img", "H", "W", "nnz", "n_nnz", "rows", "prm", "n_pairs", "out", "stream"],
    "mc_train_step_batch": ["patches", "n_pairs", "params", "moms", "lr", "mom", "margin", "pow", "loss", "ws", "ws_bytes", "stream"],
    "mc_train_run": ["x0", "x1", "n_img", "H", "W", "nnz", "n_nnz", "perm", "n_perm", "t0", "n_steps", "n_pairs", "prm", "params",
                     "moms", "lr", "mom", "margin", "pow", "losses", "ws", "ws_bytes", "stream"],
    "mc_train_filter_gt": ["disp", "img", "n", "mH", "mW", "stream"],
    "mc_train_nnz_count": ["disp", "n", "mH", "mW", "count", "nws", "nws_bytes", "stream"],
    "mc_train_nnz_fill": ["disp", "ids", "n", "mH", "mW", "list", "n_list", "nws", "nws_bytes", "stream"],
}
STEP_ARGS = [("n_pairs", 0, "n_pairs 0"), ("n_pairs", 4097, "n_pairs 4097"), ("n_pairs", -1, "n_pairs -1"), ("params", None, "null params"),
             ("moms", None, "null params"), ("pow", 3, "pow 3"), ("pow", 0, "pow 0"), ("margin", NAN, "margin"),
             ("margin", float("inf"), "margin"), ("margin", float("-inf"), "margin"), ("ws", None, "workspace"),
             ("ws_bytes", -1, "workspace")]
IMAGE_ARGS = [("x0", None, "null image"), ("x1", None, "null image"), ("nnz", None, "null image"), ("n_img", 0, "bad image dims 0"),
              ("H", 3, "x 3 x"), ("W", 3, "x 3"), ("H", 32768, "32768 x"), ("W", 32768, "x 32768"), ("n_nnz", 0, "empty nnz"),
              ("n_nnz", -5, "empty nnz"), (("n_img", "H", "W"), (1025, 32767, 32767), "bad image dims 1025")]
MAP_ARGS = [("n", -1, "bad map dims -1"), ("mH", 0, "bad map dims"), ("mW", 0, "bad map dims"), ("disp", None, "null map"),
            (("n", "mH", "mW"), (65536, 32768, 1), "too many"), (("n", "mH", "mW"), (1024, 1024, 1 << 20), "too many")]
REFUSALS = (
    [("mc_train_step_batch",) + c for c in STEP_ARGS + [("patches", None, "null pointer"), ("loss", None, "null pointer")]] +
    [("mc_train_run",) + c for c in STEP_ARGS + IMAGE_ARGS + [
        ("perm", None, "null pointer"), ("prm", None, "null pointer"), ("losses", None, "null pointer"), ("n_steps", -1, "n_steps -1"),
        ("t0", -1, "permutation"), ("t0", 5, "permutation"), ("n_perm", 3, "permutation"), ("n_steps", 5, "permutation")]] +
    [("mc_train_sample",) + c for c in IMAGE_ARGS + [
        ("n_pairs", 0, "n_pairs 0"), ("n_pairs", (1 << 24) + 1, "n_pairs"), ("rows", None, "null pointer"), ("prm", None, "null pointer"),
        ("out", None, "null pointer")]] +
    [("mc_train_filter_gt",) + c for c in MAP_ARGS + [("mW", 8193, "width 8193"), ("img", None, "null image")]] +
    [("mc_train_nnz_count",) + c for c in MAP_ARGS + [("count", None, "null count"), ("nws", None, "null count"),
                                                       ("nws_bytes", -1, "workspace")]] +
    [("mc_train_nnz_fill",) + c for c in MAP_ARGS + [("ids", None, "null ids"), ("nws", None, "null ids"), ("nws_bytes", -1, "workspace"),
                                                      ("n_list", -1, "-1 rows"), ("list", None, "null output"),
                                                      ("list", "misaligned", "16-byte aligned")]])


@pytest.fixture(scope="module")
def refusal_buffers(tr):
    """Small valid arguments for every entry point; every buffer a call writes is filled with NaN (-7 for the integers)."""
    import torch
    lib = tr.tl.load()
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(0)
    t = dict(x0=dev(rng.standard_normal((1, 8, 8)).astype(np.float32)), x1=dev(rng.standard_normal((1, 8, 8)).astype(np.float32)),
             nnz=dev(np.array([[1, 4, 4, 1], [1, 3, 5, 2], [1, 5, 3, 1]], np.float32)), rows=dev(np.array([0, 1], np.int32)),
             perm=dev(np.array([0, 1, 2, 0, 1, 2, 0, 1], np.int32)), prm=dev(tr.draw_params(rng, opt_of(), 2, 2)),
             patches=dev(rng.standard_normal((2, 3, 9, 9)).astype(np.float32)), out=nan(2, 3, 9, 9), params=nan(tr.tl.NPARAMS),
             moms=nan(tr.tl.NPARAMS), loss=nan(1), losses=nan(4), ws=nan(lib.mc_train_workspace_bytes(2) // 4),
             disp=nan(2, 4, 16), img=dev(np.zeros((2, 4, 16), np.float32)), ids=dev(np.array([1, 2], np.int32)),
             count=torch.full((1,), -7, dtype=torch.int64, device="cuda"),
             nws=torch.full((lib.mc_train_nnz_workspace_bytes(2, 4) // 8,), -7, dtype=torch.int64, device="cuda"), list=nan(2 * 4 * 16 + 1, 4))
    assert lib.mc_train_nnz_workspace_bytes(2, 4) % 8 == 0
    scalars = dict(n_img=1, H=8, W=8, n_nnz=3, n_pairs=2, n_perm=8, t0=0, n_steps=2, lr=0.002, mom=0.9, margin=0.2, pow=1,
                   ws_bytes=lib.mc_train_workspace_bytes(2), n=2, mH=4, mW=16, nws_bytes=lib.mc_train_nnz_workspace_bytes(2, 4),
                   n_list=8, stream=None)
    return t, scalars


@pytest.mark.parametrize("fn,arg,value,names", REFUSALS, ids=["%s-%s-%s" % (c[0][9:], "+".join(c[1]) if isinstance(c[1], tuple) else c[1], c[2])
                                                              for c in REFUSALS])
def test_refusals_are_loud_and_touch_nothing(tr, refusal_buffers, fn, arg, value, names):
    """One case per MC_REQUIRE that train.hip (with train_net.h and train_conv.h, which hold its shared checks) and dataset.hip can reach: MC_EINVAL, a message that names the argument, and no buffer
    written.  All of them are refused on the host before any launch."""
    import torch
    lib = tr.tl.load()
    tensors, scalars = refusal_buffers
    vals = dict(scalars)
    vals.update({k: v.data_ptr() for k, v in tensors.items()})
    for a, v in zip(arg, value) if isinstance(arg, tuple) else [(arg, value)]:
        if v == "misaligned":
            vals[a] += 4
        elif a in ("ws_bytes", "nws_bytes"):
            vals[a] += v                                   # one byte short
        else:
            vals[a] = v
    torch.cuda.synchronize()
    rc = getattr(lib, fn)(*[vals[k] for k in SIG[fn]])
    msg = lib.mc_train_last_error().decode()
    torch.cuda.synchronize()
    print("%s(%s = %s): rc %d, %r" % (fn, arg, value, rc, msg))
    assert rc == MC_EINVAL
    assert msg and names in msg, msg
    for k in ("out", "params", "moms", "loss", "losses", "ws", "disp", "list"):
        assert bool(torch.isnan(tensors[k]).all()), k
    assert bool((tensors["count"] == -7).all()) and bool((tensors["nws"] == -7).all())


def test_the_refusal_baseline_is_accepted(tr, refusal_buffers):
    """The arguments the refusal cases start from are valid: each refusal is due to the one argument it changes.  Runs on
    copies of the NaN-filled buffers, so that it does not disturb them."""
    import torch
    lib = tr.tl.load()
    tensors, scalars = refusal_buffers
    copies = {k: v.clone() for k, v in tensors.items()}
    copies["params"] = dev(to.flat(to.random_layers(1)))
    copies["moms"].zero_()
    copies["disp"] = dev(np.random.default_rng(1).uniform(0, 8, (2, 4, 16)).astype(np.float32))
    vals = dict(scalars)
    vals.update({k: v.data_ptr() for k, v in copies.items()})
    for fn in ("mc_train_sample", "mc_train_step_batch", "mc_train_run", "mc_train_filter_gt", "mc_train_nnz_count", "mc_train_nnz_fill"):
        assert getattr(lib, fn)(*[vals[k] for k in SIG[fn]]) == 0, (fn, lib.mc_train_last_error())
    torch.cuda.synchronize()
    assert torch.isfinite(copies["out"]).all() and torch.isfinite(copies["losses"][:2]).all() and torch.isnan(copies["losses"][2:]).all()
    assert 0 <= int(copies["count"]) <= 8 * 16


def test_workspace_sizes_are_zero_where_documented(tr):
    lib = tr.tl.load()
    for n in (0, -1, 4097, -2 ** 31):
        assert lib.mc_train_workspace_bytes(n) == 0
    assert lib.mc_train_workspace_bytes(1) == (tr.tl.NPARAMS + 1) * 4
    assert lib.mc_train_workspace_bytes(4096) == 4096 * (tr.tl.NPARAMS + 1) * 4
    for n, H in ((-1, 5), (1, 0), (1, -3), (65536, 32768), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.mc_train_nnz_workspace_bytes(n, H) == 0, (n, H)
    assert lib.mc_train_nnz_workspace_bytes(0, 5) == 8                  # no rows: the offset of row 0
    assert lib.mc_train_nnz_workspace_bytes(3, 5) == 64 + 16 * 8       # 15 int32 counts rounded up to 16 bytes, 16 int64 offsets


# ---- (h) the reference's kernels pin the oracle's tail ---------------------------------------------------------------------
@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("N", [1, 16])
def test_the_references_kernels_agree_with_the_oracles_tail(ref, N, pow_):
    """Normalize_forward, Margin2 (followed by Margin2.lua's division by the number of pairs) and Normalize_backward_input
    of the reference on features (4N, 64, 1, 1), against float64 autograd of train_oracle.tail_parts.  Bound: the fp32
    worst case of a 64-term sum, 66 * 2^-24 = 3.9e-6, times the quantity's scale (1 for the normalised features, the scores
    and the loss; 1 / sqrt(norm) for the backward pass, whose incoming gradient is at most 1 in magnitude)."""
    import torch
    bound = 66 * 2.0 ** -24
    margin = 0.2
    rng = np.random.default_rng(50 + N + pow_)
    x = rng.standard_normal((4 * N, 64, 1, 1)).astype(np.float32)
    x[0::4] = x[2::4]                                                # patches 4i-3 and 4i-1 are the same left patch
    x[1::4] = (x[0::4] + 3 * rng.standard_normal((N, 64, 1, 1))).astype(np.float32)      # a positive that resembles it
    if N == 1:
        x[3] = (x[0] + 0.5 * rng.standard_normal((64, 1, 1))).astype(np.float32)         # and a negative that does: an active hinge
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    hn, s, per_pair = to.tail_parts(xt, margin, pow_)
    hn.retain_grad()
    s.retain_grad()
    loss = per_pair.mean()
    loss.backward()
    f = (s[1::2] - s[0::2] + margin).detach().numpy()
    assert (np.abs(f) > 1e-4).all()                                  # no hinge at its kink
    assert (f > 0).any() and (N == 1 or (f < 0).any())               # active and (among 16) inactive hinges
    # forward: Normalize2
    xd = torch.from_numpy(x).cuda()
    norm = torch.full((4 * N, 1, 1, 1), NAN, device="cuda")
    out = torch.full((4 * N, 64, 1, 1), NAN, device="cuda")
    ref.call("Normalize_forward", xd, norm, out)
    e_norm = float((norm.cpu().double() - ((xt.detach() ** 2).sum(1, keepdim=True) + 1e-5)).abs().max())
    e_out = float((out.cpu().double() - hn.detach()).abs().max())
    # StereoJoin1.lua's forward on the reference's normalised features, in fp32 on the device
    sd = (out[0::2] * out[1::2]).sum(1).reshape(2 * N, 1, 1, 1).contiguous()
    e_s = float((sd.cpu().double().ravel() - s.detach()).abs().max())
    tmp = torch.full((N,), NAN, device="cuda")
    gs = torch.full((2 * N, 1, 1, 1), NAN, device="cuda")
    ref.call("Margin2", sd, tmp, gs, margin, pow_)
    ref_loss = float(tmp.double().mean().cpu())
    gs = gs / N                                                      # Margin2.lua: self.gradInput:div(self.tmp:size(1))
    e_loss = abs(ref_loss - float(loss))
    e_gs = float((gs.cpu().double().ravel() - s.grad).abs().max())
    # StereoJoin1.lua's backward, then Normalize2's
    g_out = torch.empty_like(out)
    g_out[0::2] = out[1::2] * gs
    g_out[1::2] = out[0::2] * gs
    e_gout = float((g_out.cpu().double() - hn.grad).abs().max())
    g_in = torch.full((4 * N, 64, 1, 1), NAN, device="cuda")
    ref.call("Normalize_backward_input", g_out, xd, norm, g_in)
    scale = 1 / np.sqrt(norm.cpu().double().numpy())
    e_gin = float(((g_in.cpu().double() - xt.grad).abs() / scale).max())
    print("N %d pow %d: errors norm %.2e (of ~64), normalised %.2e, scores %.2e, loss %.2e, d/dscores %.2e, d/dnormalised %.2e, "
          "d/dfeatures %.2e of 1/sqrt(norm); bound %.2e" % (N, pow_, e_norm, e_out, e_s, e_loss, e_gs, e_gout, e_gin, bound))
    assert float(xt.grad.abs().max()) > 0
    assert e_norm <= bound * float(norm.max())
    assert e_out <= bound and e_s <= bound and e_loss <= bound and e_gs <= bound and e_gout <= bound
    assert e_gin <= bound
