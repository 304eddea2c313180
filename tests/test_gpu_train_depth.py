"""GPU: libmctraindepth.so (include/mc_train_depth.h), the fast net's training step at -l1 1..5 on both image stores.

  1. where it overlaps the older libraries it equals them bit for bit: l1 = 4 against libmctrain.so on a KITTI store, l1 = 5
     against libmctrainmb.so on a ragged one (the same inline code, instantiated with the same constants under the same flags);
  2. every depth the older libraries do not have, and l1 = 5 through this one, against float64 autograd;
  3. l1 = 1 at its edges: GEMMs of 3 columns, a first layer whose 5 K steps split unevenly, no data gradient;
  4. the sampler at the new patch sides against the warp restatement;
  5. runs are bitwise reproducible and equal sample -> step_batch chained;
  6. `main.py kitti fast -l1 2` and `mb fast -l1 3` end to end: train, save, test_te, predict.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_fast_oracle as do  # noqa: E402
from train_fixtures import bits, dev, rel, same_bits, small_images, write_synthetic_kitti  # noqa: E402
from train_mb_oracle import write_synthetic_mb  # noqa: E402

pytestmark = pytest.mark.gpu
LR, MOM, MARGIN = 0.002, 0.9, 0.2


@pytest.fixture(scope="module")
def td():
    import torch
    from mc_cnn_amd import train_depth
    assert torch.cuda.is_available()
    return train_depth


def patches_of(rng, n, l1):
    return rng.standard_normal((n, 3, do.ws_of(l1), do.ws_of(l1))).astype(np.float32)


def kitti_opt(*extra):
    from mc_cnn_amd import main
    return main.parse(["kitti", "fast", "-a", "train_tr", "-hflip", "1"] + list(extra))[2]


def mb_opt(*extra):
    from mc_cnn_amd import train_mb
    return train_mb.parse(["mb", "fast", "-a", "train_tr", "-hflip", "1", "-d_exp", "0.5", "-d_light", "0.5"] + list(extra))[2]


# ---- the two stores ---------------------------------------------------------------------------------------------------------------
RAGGED = ((23, 37, 2, 2), (4, 4, 1, 1))     # (H, W, lights >= 2, exposures) of two images; 4 x 4 is smaller than every patch but 3 x 3


def ragged_set(seed=2):
    """Two images of different sizes in the loader's form (planes, table, index), nnz of every pixel at disparity 1, and the
    planes as a list of 2-D arrays in the table's order."""
    from mc_cnn_amd import train_mb
    rng = np.random.default_rng(seed)
    X, nnz = [], []
    for n, (H, W, n_light, n_exp) in enumerate(RAGGED, 1):
        base = rng.standard_normal((H, W)).astype(np.float32)
        lights = [np.zeros((0,), np.float32)]
        for l in range(n_light):
            lights.append(np.stack([np.stack([base * (1 + 0.1 * e) + 0.1 * l, np.roll(base, -1, 1) * (1 + 0.1 * e) + 0.1 * l +
                                              0.1 * rng.standard_normal((H, W))])[:, None] for e in range(n_exp)]).astype(np.float32))
        X.append(lights)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        nnz.append(np.stack([np.full(H * W, n), ys.ravel(), xs.ravel(), np.full(H * W, 1)], 1))
    planes, table, index = train_mb.build_store(X, need={1, 2})
    as_list = [planes[r["offset"]:r["offset"] + r["H"] * r["W"]].reshape(r["H"], r["W"]) for r in table]
    return planes, table, index, np.concatenate(nnz).astype(np.float32), as_list


def draws(store, seed, n_steps, n_pairs, t0):
    """(nnz, perm, prm, src or None) of a run on `store` ("kitti" | "mb"), drawn in train()'s order"""
    from mc_cnn_amd import train_common, train_mb
    rng = np.random.default_rng(seed)
    if store == "kitti":
        nnz = small_images(1)[2]
        perm = rng.permutation(nnz.shape[0]).astype(np.int32)
        return nnz, perm, train_common.draw_params(rng, kitti_opt(), n_steps, n_pairs), None
    _, _, index, nnz, _ = ragged_set()
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    perm[t0 + 1] = nnz.shape[0] - 1                      # a pixel of the 4 x 4 image is among the first step's pairs
    prm = train_common.draw_params(rng, mb_opt(), n_steps, n_pairs)
    ids = nnz[perm[t0:t0 + n_steps * n_pairs], 0].reshape(n_steps, n_pairs)
    src = train_mb.draw_sources(rng, mb_opt(), ids, index)
    assert (ids == 2).any() and (ids == 1).any() and (src[..., 1] != src[..., 0] + 1).any()
    return nnz, perm, prm, src


def run_on(store, mod, layers, seed, n_steps, n_pairs, t0):
    """A run of `mod`'s Trainer for `store` (train / train_mb, or train_depth at the depth of layers) from row t0 of the
    permutation: (trainer, losses, perm, prm, src)."""
    import torch
    from mc_cnn_amd import train_depth
    nnz, perm, prm, src = draws(store, seed, n_steps, n_pairs, t0)
    cuda = torch.device("cuda")
    losses = torch.full((n_steps,), -7.0, dtype=torch.float32, device="cuda")
    if store == "kitti":
        x0, x1, _ = small_images(1)
        t = mod.Trainer(x0, x1, nnz, perm, layers, n_pairs, cuda)
        t.run(t0, dev(prm), LR, MOM, MARGIN, 1, losses)
    else:
        planes, table = ragged_set()[:2]
        t = (mod.MbTrainer if mod is train_depth else mod.Trainer)(planes, table, nnz, perm, layers, n_pairs, cuda)
        t.run(t0, dev(src), dev(prm), LR, MOM, MARGIN, 1, losses)
    torch.cuda.synchronize()
    return t, losses, perm, prm, src


def sample_on(store, td, l1, t, rows, prm, src):
    """The patches of pairs `rows` through the depth library's sampler for `store`, from trainer t's device store"""
    if store == "kitti":
        return td.sample(l1, t.x0, t.x1, t.nnz, dev(rows), dev(prm))
    return td.mb_sample(l1, t.planes, t.table, t.nnz, dev(rows), dev(src), dev(prm))


# ---- 1. the new library equals the old ones where they overlap, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("store, l1", [("kitti", 4), ("mb", 5)])
def test_run_and_sample_equal_the_older_library_bit_for_bit(td, store, l1):
    from mc_cnn_amd import train, train_mb
    old = train if store == "kitti" else train_mb
    n_steps, n_pairs, t0 = 3, 5, 7
    layers = do.random_layers(l1, 3)
    a, la, perm, prm, src = run_on(store, old, layers, 3, n_steps, n_pairs, t0)
    b, lb, _, _, _ = run_on(store, td, layers, 3, n_steps, n_pairs, t0)
    assert b.LIB.PREFIX == "mc_train_depth" and a.LIB.PREFIX != b.LIB.PREFIX      # two libraries did run
    assert same_bits(a.params, b.params) and same_bits(a.moms, b.moms) and same_bits(la, lb)
    assert np.isfinite(la.cpu().numpy()).all() and float(la.min()) > 0 and not same_bits(a.params, dev(do.flat(layers)))
    rows = perm[t0:t0 + n_pairs]
    if store == "kitti":
        want = old.sample(a.x0, a.x1, a.nnz, dev(rows), dev(prm[0]))
    else:
        want = old.sample(a.planes, a.table, a.nnz, dev(rows), dev(src[0]), dev(prm[0]))
    got = sample_on(store, td, l1, b, rows, prm[0], None if src is None else src[0])
    assert got.shape == (n_pairs, 3, 2 * l1 + 1, 2 * l1 + 1) and same_bits(got, want)
    assert float(got.abs().max()) > 0.1


@pytest.mark.parametrize("n_pairs", [1, 64, 65])
@pytest.mark.parametrize("l1", [4, 5])
def test_step_batch_equals_the_older_library_bit_for_bit(td, l1, n_pairs):
    import torch
    from mc_cnn_amd import train, train_mb
    old = train if l1 == 4 else train_mb
    rng = np.random.default_rng(10 * l1 + n_pairs)
    b = dev(patches_of(rng, n_pairs, l1))
    start = do.flat(do.random_layers(l1, 4))
    v0 = (rng.standard_normal(start.size) * 1e-3).astype(np.float32)
    state = []
    for step in (old.step_batch, lambda *a: td.step_batch(l1, *a)):
        params, moms = dev(start), dev(v0)
        loss = step(b, params, moms, LR, MOM, MARGIN, 2)
        torch.cuda.synchronize()
        state.append((params, moms, loss))
    for x, y in zip(*state):
        assert same_bits(x, y)
    assert float(state[0][2]) > 0 and not same_bits(state[0][0], dev(start))


# ---- 2. every new depth against float64 autograd ----------------------------------------------------------------------------------
# Seeds whose first batch of 16 pairs the float64 oracle alone calls non-fragile under the net of random_layers(l1, 5): no
# pre-activation before a ReLU and no hinge argument within 3e-6 of 0 (train_oracle.hinge_and_fragility's rule), found on the CPU.
FIRST_BATCH_SEED = {1: 100, 2: 200, 3: 300, 5: 594}


def batches_of(rng, layers, l1, n_pairs, n_steps, pow_):
    """n_steps batches of n_pairs pairs.  The first is the seed's first draw, whole.  At l1 <= 3 so are the others, as in
    test_gpu_train.py.  At l1 = 5 the others are planned as test_gpu_train_mb.py::plan_steps plans its own: 3 n candidates of which
    the first n non-fragile ones are kept, judged on the float64 oracle's own trajectory (fp32 state), no GPU involved -- five
    layers put 670 000 pre-activations of a batch in front of a ReLU, some of them within 3e-6 of 0, and one mask that
    fp32 rounding flips sends a float32 and a float64 trajectory apart (see the docstring below)."""
    first = patches_of(rng, n_pairs, l1)
    if l1 <= 3:
        return [first] + [patches_of(rng, n_pairs, l1) for _ in range(n_steps - 1)]
    batches, p, v = [first], do.flat(layers), np.zeros(do.nparams_of(l1), np.float32)
    for _ in range(n_steps - 1):
        p, v, _ = do.sgd_steps(do.unflat(l1, p), [batches[-1]], LR, MOM, MARGIN, pow_, fp32_state=True, moms=v)
        p, v = p.astype(np.float32), v.astype(np.float32)
        cand = patches_of(rng, 3 * n_pairs, l1)
        keep = np.nonzero(~do.hinge_and_fragility(do.unflat(l1, p), cand, MARGIN)[1])[0]
        assert keep.size >= n_pairs, "only %d of %d candidate pairs are non-fragile" % (keep.size, cand.shape[0])
        batches.append(cand[keep[:n_pairs]])
    return batches


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("l1", sorted(FIRST_BATCH_SEED))
def test_step_matches_float64_autograd(td, l1, pow_):
    """The bounds of test_gpu_train.py::test_step_matches_float64_autograd (l1 = 4) at l1 = 1, 2, 3 -- a shallower chain sums fewer
    products -- and those of test_gpu_train_mb.py's step tests at l1 = 5.  For the first step and for each of 20 steps from the
    same fp32 state they are the same numbers: loss, parameters and momenta within 1e-5, at the first step each tensor within
    1e-4 of its largest magnitude.  For the 20-step trajectory l1 = 4's are the losses to rtol 1e-4 / atol 1e-6, Middlebury's the
    parameters to 1e-4 relative L2 on planned batches; l1 = 5 is held to both.
    Measured at l1 = 5, pow 1 on 20 unplanned batches: the kernel's losses within 1e-6 of the float64 trajectory for four steps,
    then up to 2.4e-4 apart, its parameters 1.4e-4 relative.  Float32 torch autograd on the CPU leaves the float64 trajectory on
    those batches by as much (1.6e-4, 1.5e-4): the distance is float32's where a ReLU mask can flip, not the kernel's, whose step
    equals libmctrainmb.so's bit for bit (above).  Hence batches_of's plan at that depth."""
    import torch
    rng = np.random.default_rng(FIRST_BATCH_SEED[l1])
    layers = do.random_layers(l1, 5)
    n_pairs = 16
    batches = batches_of(rng, layers, l1, n_pairs, 20, pow_)
    f, fragile = do.hinge_and_fragility(layers, batches[0], MARGIN)
    assert not fragile.any() and (f > 0).sum() >= 8       # a property of the input: every one of the 16 pairs is compared
    params = dev(do.flat(layers))
    moms = torch.zeros_like(params)
    _, ws = td.common.new_workspace(td.tdl.at_depth(l1), "test", n_pairs, torch.device("cuda"))
    losses, worst = [], [0.0, 0.0, 0.0]
    for k, b in enumerate(batches):
        p0, v0 = params.cpu().numpy(), moms.cpu().numpy()
        losses.append(float(td.step_batch(l1, dev(b), params, moms, LR, MOM, MARGIN, pow_, ws).cpu()))
        gp, gv = params.cpu().numpy(), moms.cpu().numpy()
        wp, wv, wl = do.sgd_steps(do.unflat(l1, p0), [b], LR, MOM, MARGIN, pow_, moms=v0)     # from the same fp32 state
        if k == 0:
            print("l1 %d pow %d, first step: loss %.7f (float64 %.7f), max |error| params %.2e momenta %.2e"
                  % (l1, pow_, losses[0], wl[0], np.abs(gp - wp).max(), np.abs(gv - wv).max()))
            assert np.abs(wv).max() > 1e-6                # the step moved something
            do.check_per_tensor(l1, gv, wv, 1e-4, "l1 %d pow %d" % (l1, pow_))     # the momenta are -lr * g
        worst = [max(a, float(e)) for a, e in zip(worst, (abs(losses[-1] - wl[0]), np.abs(gp - wp).max(), np.abs(gv - wv).max()))]
        assert abs(losses[-1] - wl[0]) <= 1e-5, (k, losses[-1], wl[0])
        np.testing.assert_allclose(gp, wp, rtol=0, atol=1e-5, err_msg="step %d" % k)
        np.testing.assert_allclose(gv, wv, rtol=0, atol=1e-5, err_msg="step %d" % k)
    print("l1 %d pow %d, each of 20 steps from its fp32 state: max |error| loss %.2e params %.2e momenta %.2e" % ((l1, pow_) + tuple(worst)))
    wp, wv, wl = do.sgd_steps(layers, batches, LR, MOM, MARGIN, pow_, fp32_state=True)
    gp, gv = params.cpu().numpy(), moms.cpu().numpy()
    print("l1 %d pow %d, 20 steps: max relative loss error %.2e; relative L2 error params %.2e, momenta %.2e"
          % (l1, pow_, np.max(np.abs(np.array(losses) - wl) / np.abs(wl)), rel(gp, wp), rel(gv, wv)))
    np.testing.assert_allclose(losses, wl, rtol=1e-4, atol=1e-6)
    assert rel(gp, wp) <= 1e-4


# ---- 3. l1 = 1 at its edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, pow_", [(1, 1), (2, 1), (2, 2)])
def test_one_layer_sums_its_gradients_in_pair_order(td, N, pow_):
    """test_gpu_train_limits.py::test_gradients_are_summed_in_pair_order's construction on the one-layer net, whose only GEMMs have
    3 columns (forward, K = 9 taps in 5 steps over four slices) and K = 3 (weight gradient): with lr = 1, mom = 0 and zero
    momenta a step leaves moms = -g; the N-pair step must give the float32 sum of the single pairs' g_i / N in pair order."""
    import torch
    l1 = 1
    rng = np.random.default_rng(34)                       # a seed whose first two pairs have active hinges under this net (found on the CPU)
    layers = do.random_layers(l1, 21)
    b = patches_of(rng, N, l1)
    f, _ = do.hinge_and_fragility(layers, b, MARGIN)
    assert (f > 0.05).all()                               # every pair has a gradient to sum
    bd, fresh, NP = dev(b), dev(do.flat(layers)), do.nparams_of(l1)
    G = torch.empty((N, NP), dtype=torch.float32, device="cuda")
    for i in range(N):
        params, moms = fresh.clone(), torch.zeros(NP, device="cuda")
        td.step_batch(l1, bd[i:i + 1], params, moms, 1.0, 0.0, MARGIN, pow_)
        torch.neg(moms, out=G[i])
    params, moms = fresh.clone(), torch.zeros(NP, device="cuda")
    nbytes, ws = td.common.new_workspace(td.tdl.at_depth(l1), "test", N, torch.device("cuda"))
    assert nbytes == N * (NP + 1) * 4
    ws.fill_(float("nan"))                                # exactly the bytes asked for, poisoned: all of it is written before it is read
    loss = float(td.step_batch(l1, bd, params, moms, 1.0, 0.0, MARGIN, pow_, ws).cpu())
    assert torch.isfinite(ws).all() and torch.isfinite(G).all()
    acc = torch.zeros(NP, device="cuda")
    for i in range(N):
        acc = acc + G[i] * (1.0 / N)                      # exact scaling by a power of two, one float32 add per pair, in pair order
    want = torch.zeros(NP, device="cuda") - acc           # the kernel's 0 * 0 - 1 * g
    assert float((G * (1.0 / N)).abs()[G != 0].min()) > 2.0 ** -100      # no term near the subnormals, where the scaling would round
    print("l1 1, N %d pow %d: %d of %d elements differ from the ordered float32 sum" % (N, pow_, int((bits(moms) != bits(want)).sum()), NP))
    assert same_bits(moms, want) and same_bits(params, fresh + moms)
    assert float(moms.abs().max()) > 1e-4 and (moms.view(-1)[:576] != 0).any() and (moms.view(-1)[576:] != 0).any()
    want_loss = float(do.loss_of(do.as_f64(layers), torch.tensor(b.astype(np.float64)), MARGIN, pow_))
    assert abs(loss - want_loss) <= 1e-5


# ---- 4. the sampler at the new patch sides -----------------------------------------------------------------------------------------
def sampler_prm(rng, opt, n):
    """n pairs' parameters: the data set's full augmentation, every fifth pair without any warp (the geometry alone)"""
    from mc_cnn_amd import train_common
    prm = train_common.draw_params(rng, opt, 1, n)[0]
    prm[::5] = np.array([0.5, -3, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 1], np.float32)
    return prm


@pytest.mark.parametrize("l1", [1, 2, 3])
def test_sampler_matches_the_warp_restatement_on_a_kitti_store(td, l1):
    x0, x1, nnz = small_images(11, n_img=2, H=21, W=34)
    H, W = x0.shape[1:]
    at = lambda img, y, x: (img - 1) * H * W + y * W + x
    # the four corners, the borders, the inside
    rows = np.array([at(1, 0, 0), at(2, 0, W - 1), at(1, H - 1, 0), at(2, H - 1, W - 1), at(1, 1, W // 2), at(2, H // 2, 1),
                     at(1, H // 2, W - 2), at(2, H - 2, W // 2), at(1, H // 2, W // 2), at(2, 7, 9), at(1, 0, 0), at(2, H - 1, W - 1)], np.int32)
    prm = sampler_prm(np.random.default_rng(l1), kitti_opt(), rows.size)
    assert (nnz[rows[0], 1:3] == 0).all() and (nnz[rows[10], 1:3] == 0).all()     # a corner without a warp (pair 0, 10) and with one
    got = td.sample(l1, dev(x0), dev(x1), dev(nnz), dev(rows), dev(prm)).cpu().numpy()
    assert got.shape == (rows.size, 3, 2 * l1 + 1, 2 * l1 + 1)
    worst = 0.0
    for i in range(rows.size):
        want = do.sample_pair(l1, x0, x1, nnz[rows[i]], prm[i])
        worst = max(worst, float(np.abs(got[i] - want).max()))
        np.testing.assert_allclose(got[i], want, rtol=0, atol=1e-5, err_msg="pair %d" % i)
    print("l1 %d, KITTI store: max |error| %.2e" % (l1, worst))
    c = l1                                               # the unwarped corner patch: its centre is the pixel, everything above and left of it reads 0
    assert got[0, 0, c, c] == x0[0, 0, 0] and (got[0, 0, :c] == 0).all() and (got[0, 0, :, :c] == 0).all()


@pytest.mark.parametrize("l1", [1, 2, 3])
def test_sampler_matches_the_warp_restatement_on_a_ragged_store(td, l1):
    import torch
    from mc_cnn_amd import train_mb
    planes, table, index, nnz, as_list = ragged_set()
    H, W = RAGGED[0][:2]
    n1 = H * W
    small = int(index[1, 0])                             # the 4 x 4 image's first plane
    # image 1: corners, borders, inside, views from different lights and exposures; image 2 (4 x 4): every kind of pixel
    rows = np.array([0, W - 1, n1 - W, n1 - 1, W // 2, (H // 2) * W + 1, (H // 2) * W + W // 2, 5 * W + 7, n1, n1 + 5, n1 + 15, n1 + 10], np.int32)
    src = np.array([[0, 1], [2, 3], [4, 5], [6, 7], [0, 3], [2, 5], [4, 7], [6, 1]] + [[small, small + 1]] * 4, np.int32)
    assert (nnz[rows[8:], 0] == 2).all() and (nnz[rows[:8], 0] == 1).all() and table["H"][small] == 4
    prm = sampler_prm(np.random.default_rng(10 + l1), mb_opt(), rows.size)
    dtable = train_mb.device_table(table, torch.device("cuda"))
    got = td.mb_sample(l1, dev(planes), dtable, dev(nnz), dev(rows), dev(src), dev(prm)).cpu().numpy()
    assert got.shape == (rows.size, 3, 2 * l1 + 1, 2 * l1 + 1)
    worst, shown = 0.0, 0
    for i in range(rows.size):
        want = do.sample_mb_pair(l1, as_list, nnz[rows[i]], src[i], prm[i])
        worst = max(worst, float(np.abs(got[i] - want).max()))
        np.testing.assert_allclose(got[i], want, rtol=0, atol=1e-5, err_msg="pair %d (planes %s)" % (i, src[i]))
        shown += int(np.abs(want[0] - prm[i, 8]).max() > 0.1)
    print("l1 %d, ragged store: max |error| %.2e" % (l1, worst))
    assert shown == rows.size                            # every left patch shows its plane, those of the 4 x 4 image too
    assert got[10, 0, l1, l1] == as_list[small][3, 3]   # pair 10 is unwarped: the centre of the patch is the pixel


# ---- 5. runs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["kitti", "mb"])
@pytest.mark.parametrize("l1", [1, 2, 3, 4, 5])             # every depth on both stores: each instantiation of the run's kernels
def test_runs_are_bitwise_reproducible_and_equal_the_chain_of_sample_and_step(td, l1, store):
    import torch
    n_steps, n_pairs, t0 = 4, 6, 9
    layers = do.random_layers(l1, 4)
    a, la, perm, prm, src = run_on(store, td, layers, 4, n_steps, n_pairs, t0)
    b, lb, _, _, _ = run_on(store, td, layers, 4, n_steps, n_pairs, t0)
    assert same_bits(a.params, b.params) and same_bits(a.moms, b.moms) and same_bits(la, lb)
    assert a.params.numel() == do.nparams_of(l1) and torch.isfinite(la).all() and float(la.min()) > 0
    params = dev(do.flat(layers))
    moms = torch.zeros_like(params)
    for s in range(n_steps):
        rows = perm[t0 + s * n_pairs:t0 + (s + 1) * n_pairs]
        patches = sample_on(store, td, l1, a, rows, prm[s], None if src is None else src[s])
        loss = td.step_batch(l1, patches, params, moms, LR, MOM, MARGIN, 1)
        assert same_bits(loss, la[s:s + 1]), s
    assert same_bits(params, a.params) and same_bits(moms, a.moms)


def test_depths_keep_their_own_lds_limit_in_one_process(td):
    """Each depth's kernels get their own dynamic-LDS limit: a deep net after a shallow one (and back) still launches and gives
    what it gave alone."""
    import torch
    out = {}
    for l1 in (1, 5, 2, 4, 3, 5, 1):
        params = dev(do.flat(do.random_layers(l1, 1)))
        moms = torch.zeros_like(params)
        loss = td.step_batch(l1, dev(patches_of(np.random.default_rng(l1), 3, l1)), params, moms, LR, MOM, MARGIN, 1)
        torch.cuda.synchronize()
        assert torch.isfinite(loss).all() and float(loss) > 0
        if l1 in out:
            assert same_bits(out[l1], params)
        out[l1] = params
    assert len(out) == 5


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------------
def write_png_pair(left, right):
    from PIL import Image
    for name, a in (("l.png", left), ("r.png", right)):
        a = (a - a.min()) / (a.max() - a.min()) * 255
        Image.fromarray(a.astype(np.uint8)).save(name)


def check_saved_net_and_rerun(main, head, fname, l1, mean, n_examples, capsys, disp_max):
    """The saved .t7 has l1 convolutions 1 -> 64 -> .. -> 64; test_te on it prints the mean that followed the training; predict runs."""
    from mc_cnn_amd import t7
    layers, _ = t7.load_reference_net(fname, "fast")
    assert [w.shape for w, _ in layers] == [(64, 1 if i == 0 else 64, 3, 3) for i in range(l1)]
    assert main.main(head + ["-a", "test_te", "-net_fname", fname]) == 0          # a .t7 carries its own depth: no -l1
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == n_examples + 1 and float(out[-1]) == mean
    assert main.main(head[:2] + ["-a", "predict", "-net_fname", fname, "-left", "l.png", "-right", "r.png", "-disp_max", str(disp_max)]) == 0
    out = capsys.readouterr().out
    assert "Writing disp.bin" in out
    disp = np.fromfile("disp.bin", np.float32)             # raw float32, as the reference writes it
    assert disp.size > 0 and np.isfinite(disp).all()


def test_kitti_fast_l1_2_trains_saves_tests_and_predicts(tmp_path, monkeypatch, capsys, td):
    from mc_cnn_amd import main
    monkeypatch.chdir(tmp_path)
    x0, x1 = write_synthetic_kitti(str(tmp_path / "data.kitti"))
    write_png_pair(x0[5, 0], x1[5, 0])
    args = ["kitti", "fast", "-a", "train_tr", "-l1", "2", "-bs", "16", "-epochs", "1", "-max_steps", "40", "-disp_max", "32"]
    assert main.main(args) == 0
    out = capsys.readouterr().out.strip().splitlines()
    run = td.last_run
    assert run["losses"].size == 40 and np.isfinite(run["losses"]).all() and run["epochs"] == 1
    assert run["net_fname"] == os.path.join("net", "net_kitti_fast_-a_train_tr_-l1_2_-bs_16_-epochs_1_-max_steps_40_-disp_max_32.t7")
    mean = float(out[-1])                                 # one line for the epoch, `runtime err` per test pair, the mean
    assert np.isfinite(mean) and [len(l.split()) for l in out[-3:]] == [2, 2, 1]
    check_saved_net_and_rerun(main, ["kitti", "fast", "-disp_max", "32"], run["net_fname"], 2, mean, 2, capsys, 32)
    # a seeded random net of that depth through the flag
    assert main.main(["kitti", "fast", "-a", "test_te", "-net_fname", "random:3", "-l1", "2", "-disp_max", "32"]) == 0
    assert np.isfinite(float(capsys.readouterr().out.strip().splitlines()[-1]))


# (H, W, lights >= 2, exposures, test views): test_te always predicts views 3 and 4 of image 5 besides te (main.lua:1124-1130), so
# the smallest set that can be tested has five images; two of them (2 and 3) carry the training pixels used here
MB_SCENES = ((40, 72, 1, 1, 2), (36, 80, 2, 2, 0), (44, 66, 1, 1, 0), (32, 64, 1, 1, 0), (38, 70, 1, 1, 4))


def test_mb_fast_l1_3_trains_saves_tests_and_predicts(tmp_path, monkeypatch, capsys, td):
    from mc_cnn_amd import main
    monkeypatch.chdir(tmp_path)
    written = write_synthetic_mb(str(tmp_path / "mbdata"), scenes=MB_SCENES, te=(1, 5))
    write_png_pair(written[1][1][0, 0], written[1][1][1, 0])
    args = ["mb", "fast", "-a", "train_tr", "-l1", "3", "-bs", "16", "-epochs", "1", "-max_steps", "40", "-data_dir", "mbdata"]
    assert main.main(args) == 0
    out = capsys.readouterr().out.strip().splitlines()
    run = td.last_run
    assert run["losses"].size == 40 and np.isfinite(run["losses"]).all() and run["epochs"] == 1
    assert run["net_fname"] == os.path.join("net", "net_mb_fast_-a_train_tr_-l1_3_-bs_16_-epochs_1_-max_steps_40_-data_dir_mbdata.t7")
    mean = float(out[-1])                                 # (1, 2), (5, 2), (5, 3), (5, 4), then the mean
    assert np.isfinite(mean) and [len(l.split()) for l in out[-5:]] == [2, 2, 2, 2, 1]
    check_saved_net_and_rerun(main, ["mb", "fast", "-data_dir", "mbdata"], run["net_fname"], 3, mean, 4, capsys, 24)
