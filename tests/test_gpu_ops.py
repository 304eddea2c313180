"""GPU: libmcops.so's operators (include/mc_ops.h) bit-compared with the reference's own kernels of the same name (oracle/_ref through
`ref.call`), signs of zeros included, and -- so that something holds them where oracle/_ref is absent and the `ref` fixture skips --
with their float64 formulas (the device operators within 1e-4 of the tensor's largest magnitude, the bound
tests/train_fast_oracle.check_per_tensor puts on a gradient tensor; the remove_* operators exactly against a numpy restatement).
Then three routes: the fused KITTI preprocessing against the operators, the fast net's fused tail (train_conv.h's hinge_tail) against
modules.py's chain, and BCECriterion2 / StereoJoin1 against float64."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_fast_oracle as do  # noqa: E402
from train_fixtures import dev, same_bits, write_synthetic_kitti  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ad(mc):
    import torch
    assert torch.cuda.is_available()
    return mc.adcensus


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- Normalize_backward_input ------------------------------------------------------------------------------------------------------
# the training shape; an empty sum; odd sizes; C above a wave with pixels across a workgroup (64 pixels), twice
NB_SHAPES = [(3, 64, 1, 1), (1, 1, 1, 1), (2, 5, 3, 7), (1, 112, 2, 65), (1, 128, 1, 130)]
_nb_cache = {}


def nb_case(ad, shape):
    """Random normal input and grad_output (so that every contraction rounds), the norm Normalize_forward leaves, and this
    library's grad_input: computed once per shape and left unchanged."""
    import torch
    if shape not in _nb_cache:
        rng = np.random.default_rng(sum(shape))
        x, go = (dev(rng.standard_normal(shape).astype(np.float32)) for _ in range(2))
        norm = torch.empty((shape[0], 1) + shape[2:], device="cuda")
        ad.Normalize_forward(x, norm, torch.empty_like(x))
        gi = torch.full_like(x, float("nan"))
        ad.Normalize_backward_input(go, x, norm, gi)
        torch.cuda.synchronize()
        _nb_cache[shape] = (x, go, norm, gi)
    return _nb_cache[shape]


@pytest.mark.parametrize("shape", NB_SHAPES)
def test_normalize_backward_equals_the_reference_bit_for_bit(ad, ref, shape):
    import torch
    x, go, norm, gi = nb_case(ad, shape)
    want = torch.full_like(x, float("nan"))
    ref.call("Normalize_backward_input", go, x, norm, want)
    assert torch.isfinite(want).all()
    print("%s: %d of %d elements differ" % (shape, int((gi.view(torch.int32) != want.view(torch.int32)).sum()), gi.numel()))
    assert same_bits(gi, want)


@pytest.mark.parametrize("shape", NB_SHAPES)
def test_normalize_backward_matches_its_float64_formula(ad, shape):
    x, go, norm, gi = (t.cpu().numpy().astype(np.float64) for t in nb_case(ad, shape))
    denom = norm ** 1.5
    others = (x * go).sum(1, keepdims=True) - x * go          # exact enough in float64: the sum without the own channel
    want = (norm - x * x) / denom * go - others * x / denom
    assert np.isfinite(gi).all()
    err = np.abs(gi - want).max() / np.abs(want).max()
    print("%s: max error %.2e of the largest magnitude %.2e" % (shape, err, np.abs(want).max()))
    assert err <= 1e-4
    if shape[1] == 1:                                         # the empty sum: nothing but (norm - x^2) / denom * go, and norm - x^2 = 1e-5
        assert np.abs(others).max() == 0


def test_normalize2_is_the_gradient_of_its_forward_pass(mc):
    """modules.Normalize2 through its autograd wrapper against float64 autograd of x / sqrt(sum x^2 + 1e-5)."""
    import torch
    from mc_cnn_amd import modules
    rng = np.random.default_rng(5)
    x = dev(rng.standard_normal((4, 64, 1, 1)).astype(np.float32)).requires_grad_()
    go = dev(rng.standard_normal((4, 64, 1, 1)).astype(np.float32))
    modules.normalize2_fn(x).backward(go)
    xd = x.detach().double().requires_grad_()
    (xd / torch.sqrt((xd * xd).sum(1, keepdim=True) + 1e-5)).backward(go.double())
    err = float((x.grad.double() - xd.grad).abs().max() / xd.grad.abs().max())
    print("max error %.2e of the largest magnitude" % err)
    assert err <= 1e-4


# ---- Margin2 -------------------------------------------------------------------------------------------------------------------------
MARGIN = 0.2


def margin_input(n, rot):
    """n (pos, neg) pairs; pair i is of kind (i + rot) % 3: f < 0, f > 0, f == 0 exactly (neg 0, pos the float32 margin)."""
    rng = np.random.default_rng(n)
    x = np.zeros((n, 2), np.float32)
    kind = (np.arange(n) + rot) % 3
    pos = rng.uniform(-1, 1, n).astype(np.float32)
    gap = rng.uniform(0.25, 1, n).astype(np.float32)
    x[:, 0] = pos
    x[:, 1] = np.where(kind == 0, pos - gap - np.float32(1), pos + gap)          # f < 0: neg far below pos; f > 0: neg above pos
    x[kind == 2] = (np.float32(MARGIN), 0)
    f = (x[:, 1] - x[:, 0]) + np.float32(MARGIN)
    assert ((f < 0) == (kind == 0)).all() and ((f > 0) == (kind == 1)).all() and ((f == 0) == (kind == 2)).all()
    return x.reshape(2 * n, 1, 1, 1), f


def run_margin2(ad, x, n, pow_):
    import torch
    tmp, gi = torch.full((n,), float("nan"), device="cuda"), torch.full((2 * n, 1, 1, 1), float("nan"), device="cuda")
    ad.Margin2(dev(x), tmp, gi, MARGIN, pow_)
    torch.cuda.synchronize()
    return tmp, gi


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("n", [1, 64, 257])
def test_margin2_equals_the_reference_bit_for_bit(ad, ref, n, pow_):
    import torch
    for rot in range(3 if n == 1 else 1):                     # a single pair is each kind in turn
        x, _ = margin_input(n, rot)
        tmp, gi = run_margin2(ad, x, n, pow_)
        wtmp, wgi = torch.full_like(tmp, float("nan")), torch.full_like(gi, float("nan"))
        ref.call("Margin2", dev(x), wtmp, wgi, MARGIN, pow_)
        assert same_bits(tmp, wtmp) and same_bits(gi, wgi), (n, pow_, rot)


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("n", [1, 64, 257])
def test_margin2_matches_its_float64_formula_and_the_signs_of_zero(ad, n, pow_):
    for rot in range(3 if n == 1 else 1):
        x, f32 = margin_input(n, rot)
        tmp, gi = (t.cpu().numpy() for t in run_margin2(ad, x, n, pow_))
        gi = gi.reshape(n, 2)
        xd = x.reshape(n, 2).astype(np.float64)
        f = xd[:, 1] - xd[:, 0] + np.float64(np.float32(MARGIN))
        f[f32 == 0] = 0                                       # exactly 0 in float32 by construction; float64 agrees to 1e-17
        d = np.maximum(f, 0)
        on = (f > 0).astype(np.float64)
        want_tmp = d if pow_ == 1 else 0.5 * d * d
        want_gi = np.stack([-on, on], 1) if pow_ == 1 else np.stack([-f * on, f * on], 1)
        for got, want in ((tmp, want_tmp), (gi, want_gi)):
            top = np.abs(want).max()
            assert (np.abs(got - want).max() <= 1e-4 * top) if top else (np.abs(got).max() == 0)
        # the reference's zeros.  pow 1: -1. * (f > 0) is -0.0 for an inactive pair, f > 0 alone +0.0.  pow 2: -f * (f > 0) is
        # -0.0 at f == 0 and +0.0 for f < 0, f * (f > 0) the other way round
        off, neg, zero = f32 <= 0, f32 < 0, f32 == 0
        assert (gi[off] == 0).all()
        if pow_ == 1:
            assert np.signbit(gi[off, 0]).all() and not np.signbit(gi[off, 1]).any()
        else:
            assert np.signbit(gi[zero, 0]).all() and not np.signbit(gi[zero, 1]).any()
            assert not np.signbit(gi[neg, 0]).any() and np.signbit(gi[neg, 1]).all()
        assert not np.signbit(tmp).any()


def test_margin2_module_keeps_the_mean_and_the_division(mc):
    import torch
    from mc_cnn_amd import modules
    n = 64
    x, f = margin_input(n, 0)
    for pow_ in (1, 2):
        m = modules.Margin2(MARGIN, pow_)
        out = m.forward(dev(x))
        tmp, gi = run_margin2(mc.adcensus, x, n, pow_)
        assert same_bits(out, tmp.mean()) and same_bits(m.backward(dev(x)), gi / n)
        xs = dev(x).requires_grad_()
        modules.margin2_fn(xs, MARGIN, pow_).backward()
        assert same_bits(xs.grad, gi / n)


# ---- remove_nonvisible, remove_occluded, remove_white --------------------------------------------------------------------------------
def np_nonvisible(d):
    return np.where(d >= np.arange(d.shape[-1], dtype=np.float32), np.float32(0), d)


def np_occluded(d):
    """Every pixel against the row as it was: i - y[id + i] < -y[id] in float32."""
    W = d.shape[-1]
    occ = np.zeros(d.shape, bool)
    for i in range(1, W):
        occ[..., :W - i] |= (np.float32(i) - d[..., i:]) < -d[..., :W - i]
    return np.where(occ, np.float32(0), d)


def np_white(x, d):
    return np.where(x == 255, np.float32(0), d)


def remove_case(shape):
    """Maps of multiples of 1/256 and their images.  Row 0 of every first map is planted, with keys x - y (a pixel is occluded by
    one further right with a smaller key): column 2 a y == x tie; 3 (key 2.5) and 5 (key 3) occluded; 7 (key 2.5) an occluder
    of 5 that is itself occluded by 8; 8 (key 2) stays; 6 (key 2) ties with 8, which does not occlude it; zeros between them.
    The image is 255 over column 8 and 254.999 over column 6.  Row 1: y = x - 1/256 at column 1 is visible, y == x at 2 is not."""
    rng = np.random.default_rng(shape[-1])
    N, _, H, W = shape
    d = (rng.integers(0, 256 * min(W, 40), shape) / 256).astype(np.float32)
    d[rng.uniform(0, 1, shape) < 0.3] = 0
    row = d[0, 0, 0]
    row[:9] = (0, 0, 2, 0.5, 0, 2, 4, 4.5, 6)
    row[9:] = np.where(np.arange(9, W) - row[9:] < 2, 0, row[9:])        # nothing further right has a key below 2
    d[0, 0, 1, :3] = (0, 1 - 1 / 256, 2)
    x = rng.integers(0, 255, shape).astype(np.float32)
    x[rng.uniform(0, 1, shape) < 0.1] = 255
    x[0, 0, 0, 8], x[0, 0, 0, 6] = 255, np.float32(254.999)
    assert (d * 256 == np.round(d * 256)).all() and (d >= 0).all() and d.max() < 65536
    return d, x


@pytest.mark.parametrize("shape", [(1, 1, 3, 130), (2, 1, 2, 9)])
def test_remove_operators_equal_the_reference_and_numpy(ad, ref, shape):
    import torch
    d, x = remove_case(shape)
    got, want = dev(d), dev(d)
    stages = []
    for name, args in (("remove_nonvisible", ()), ("remove_occluded", ()), ("remove_occluded", ()), ("remove_white", (dev(x),))):
        getattr(ad, name)(*args, got)
        ref.call(name, *args, want)
        torch.cuda.synchronize()
        assert same_bits(got, want), name
        stages.append(got.cpu().numpy())
    assert bits_equal(stages[1], stages[2])                   # remove_occluded run twice is bitwise stable
    _check_remove_stages(d, x, stages)


@pytest.mark.parametrize("shape", [(1, 1, 3, 130), (2, 1, 2, 9)])
def test_remove_operators_equal_numpy_exactly(ad, shape):
    import torch
    d, x = remove_case(shape)
    got = dev(d)
    stages = []
    for name, args in (("remove_nonvisible", ()), ("remove_occluded", ()), ("remove_occluded", ()), ("remove_white", (dev(x),))):
        getattr(ad, name)(*args, got)
        torch.cuda.synchronize()
        stages.append(got.cpu().numpy())
    _check_remove_stages(d, x, stages)


def _check_remove_stages(d, x, stages):
    want = np_nonvisible(d)
    assert bits_equal(stages[0], want)
    want = np_occluded(want)
    assert bits_equal(stages[1], want) and bits_equal(stages[2], want) and bits_equal(np_occluded(want), want)
    assert bits_equal(stages[3], np_white(x, want))
    vis, occ, out = stages[0][0, 0, 0], stages[1][0, 0, 0], stages[3][0, 0, 0]
    assert d[0, 0, 0, 2] == 2 and vis[2] == 0                 # the tie y == x is not visible
    assert stages[0][0, 0, 1, 1] == np.float32(1 - 1 / 256) and stages[0][0, 0, 1, 2] == 0
    assert vis[3] == 0.5 and occ[3] == 0 and vis[5] == 2 and occ[5] == 0        # occluded
    assert vis[7] == 4.5 and occ[7] == 0                      # the occluder that is itself occluded
    assert occ[8] == 6 and occ[6] == 4                        # the one that stays, and the tie beside it
    assert out[8] == 0 and out[6] == 4 and x[0, 0, 0, 6] != 255                 # 255 beside 254.999
    for a, b in zip([d] + stages[:1] + stages[2:3], stages[:2] + stages[3:]):
        assert (a != b).any()                                 # every operator removed something


# ---- the host pair against the reference ------------------------------------------------------------------------------------------
def test_make_dataset2_equals_the_reference(ad, ref):
    import torch
    rng = np.random.default_rng(3)
    maps = (rng.integers(0, 400, (2, 1, 1, 7, 11)) / 256).astype(np.float32)     # around the 0.5 threshold (128 / 256)
    maps[0, 0, 0, 0, :3] = (0.5, np.float32(0.5) + np.float32(2.0 ** -24), 129 / 256)
    got, want = torch.zeros((200, 4)), torch.zeros((200, 4))
    t = tr = 0
    for k, img in enumerate((7, 3)):                          # t is carried across two images
        t = ad.make_dataset2(torch.from_numpy(maps[k]), got, img, t)
        tr = int(ref.call("make_dataset2", torch.from_numpy(maps[k]), want, img, tr)[0])
        assert t == tr
    assert 0 < t < 200 and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_subset_dataset_equals_the_reference(ad, ref):
    import torch
    rng = np.random.default_rng(4)
    rows = np.stack([rng.integers(0, 200, 300), rng.integers(0, 50, 300), rng.integers(0, 60, 300), rng.uniform(1, 90, 300)], 1).astype(np.float32)
    for index in ([0, 199, 17, 17, 60], [], [5]):
        idx = torch.tensor(index, dtype=torch.int64)
        got, want = torch.zeros((300, 4)), torch.zeros((300, 4))
        n = ad.subset_dataset(idx, torch.from_numpy(rows), got)
        nr = int(ref.call("subset_dataset", idx, torch.from_numpy(rows), want)[0])
        assert n == nr == int(np.isin(rows[:, 0], index).sum()) and torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- route 1: the fused KITTI preprocessing against the operators ----------------------------------------------------------------
def test_fused_kitti_preprocessing_equals_the_operators(ad, tmp_path):
    """preprocess_kitti.filter_gt (dataset.hip's one kernel) + pixel_list on the synthetic set of tests/train_fixtures equal
    remove_nonvisible, remove_occluded, remove_white + make_dataset2 image by image (preprocess_kitti.lua:97-112), bit for bit."""
    import torch
    from mc_cnn_amd import binio
    from mc_cnn_amd import preprocess_kitti as pk
    d = str(tmp_path / "data.kitti")
    x0, _ = write_synthetic_kitti(d, n_img=3, H=24, W=160, seed=2)
    dispnoc = binio.fromfile(os.path.join(d, "dispnoc.bin")).astype(np.float32)
    x0 = np.round(np.clip(x0 * 40 + 200, 0, 255)).astype(np.float32)          # 8-bit images, as the archives' are, with 255 among them
    n, _, H, W = dispnoc.shape
    assert (x0 == 255).any() and (dispnoc > 0.5).any()
    fused = torch.from_numpy(dispnoc.reshape(n, H, W).copy()).cuda()
    pk.filter_gt(fused, torch.from_numpy(x0.reshape(n, H, W)).cuda())
    ids = np.arange(1, n + 1)
    fused_list = pk.pixel_list(fused, ids).cpu()
    nnz = torch.zeros((n * H * W, 4))
    t = 0
    for i in range(n):
        disp = torch.from_numpy(dispnoc[i:i + 1].copy()).cuda()
        ad.remove_nonvisible(disp)
        ad.remove_occluded(disp)
        ad.remove_white(torch.from_numpy(x0[i:i + 1]).cuda(), disp)
        assert same_bits(disp[0, 0], fused[i]), i
        t = ad.make_dataset2(disp.cpu(), nnz, int(ids[i]), t)
    assert t == fused_list.shape[0] > 0 and torch.equal(nnz[:t].view(torch.int32), fused_list.view(torch.int32))
    assert int((fused.cpu() != torch.from_numpy(dispnoc.reshape(n, H, W))).sum()) > 0       # the filters removed something


# ---- route 2: the fast net's fused tail against the modules -------------------------------------------------------------------------
@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("n_pairs", [1, 3])
def test_fused_tail_of_the_fast_trainer_matches_the_modules(mc, n_pairs, pow_):
    """train_depth.step_batch at l1 = 1 (one valid 3x3 convolution, then train_conv.h's hinge_tail) from zero momenta, lr 1 and
    mom 0 -- so that the momenta are -g -- against valid F.conv2d -> Normalize2 -> StereoJoin1 -> Margin2 of modules.py and their
    backward passes.  The convolution and its backward run in float64 (the features are rounded to float32 for Normalize2), so
    that the distance is the tail's.  The bounds are tests/test_gpu_train_depth.py's: 1e-5 on the loss, 1e-4 of each momentum
    tensor's largest magnitude.  Bit-equality is not expected: hinge_tail forms dot - x * go where the operator folds C - 1 terms."""
    import torch
    import torch.nn.functional as F
    from mc_cnn_amd import modules, train_depth
    rng = np.random.default_rng(34)                           # tests/test_gpu_train_depth.py's pairs with active hinges under this net
    layers = do.random_layers(1, 21)
    patches = rng.standard_normal((n_pairs, 3, 3, 3)).astype(np.float32)
    params = dev(do.flat(layers))
    moms = torch.zeros_like(params)
    loss = float(train_depth.step_batch(1, dev(patches), params, moms, 1.0, 0.0, MARGIN, pow_).cpu())
    w = dev(layers[0][0]).double().requires_grad_()
    b = dev(layers[0][1]).double().requires_grad_()
    p = dev(patches)
    batch = torch.stack([p[:, 0], p[:, 1], p[:, 0], p[:, 2]], 1).reshape(4 * n_pairs, 1, 3, 3)
    h = F.conv2d(batch.double(), w, b).float()
    want = modules.margin2_fn(modules.stereo_join1_fn(modules.normalize2_fn(h)), MARGIN, pow_)
    want.backward()
    g = torch.cat([w.grad.reshape(-1), b.grad]).cpu().numpy()
    got = moms.cpu().numpy().astype(np.float64)
    print("n_pairs %d pow %d: loss %.7f, modules %.7f (apart %.2e); momenta relative L2 %.2e" %
          (n_pairs, pow_, loss, float(want), abs(loss - float(want)), np.linalg.norm(got + g) / np.linalg.norm(g)))
    assert np.abs(g).max() > 1e-6                              # a hinge is active: the step moved something
    assert abs(loss - float(want)) <= 1e-5
    do.check_per_tensor(1, got, -g, 1e-4, "n_pairs %d pow %d" % (n_pairs, pow_))


# ---- route 3: BCECriterion2 and StereoJoin1 against float64 --------------------------------------------------------------------------
RTOL = 2.0 ** -20   # one rounding (2^-24) per operation of a five-operation chain, plus the device log


def test_bce_criterion2_matches_float64_and_the_saturated_loss(mc):
    import torch
    from mc_cnn_amd import modules
    rng = np.random.default_rng(6)
    x = rng.uniform(0.02, 0.98, 8).astype(np.float32)
    t = (np.arange(8) % 2).astype(np.float32)                 # targets 0 / 1, as the trainer's: one of the two terms is exactly 0
    eps = np.float64(np.float32(1e-12))
    xd, td = x.astype(np.float64), t.astype(np.float64)
    want = -np.mean(np.log(xd + eps) * td + np.log(1 - xd + eps) * (1 - td))
    want_g = -(td / (xd + eps) - (1 - td) / (1 - xd + eps)) / 8
    m = modules.BCECriterion2()
    xs = dev(x).requires_grad_()
    loss = m.forward(xs.detach(), dev(t))
    np.testing.assert_allclose(float(loss), want, rtol=RTOL)
    np.testing.assert_allclose(m.backward(xs.detach(), dev(t)).cpu().numpy(), want_g, rtol=RTOL)
    modules.bce_criterion2_fn(xs, dev(t)).backward()
    assert same_bits(xs.grad, m.gradInput)
    # the saturated net of DESIGN.md section 9.1: both outputs 1, targets (1, 0)
    sat = float(m.forward(dev(np.ones(2, np.float32)), dev(np.array([1, 0], np.float32))))
    np.testing.assert_allclose(sat, -np.log(eps) / 2, rtol=RTOL)
    assert "%.6f" % sat == "13.815512"
    assert torch.isfinite(m.backward(dev(np.ones(2, np.float32)), dev(np.array([1, 0], np.float32)))).all()


def test_stereo_join1_matches_float64(mc):
    from mc_cnn_amd import modules
    rng = np.random.default_rng(7)
    x = rng.uniform(0.5, 1.5, (6, 5, 2, 3)).astype(np.float32)            # positive: no cancellation in the sum over 5 channels
    go = rng.standard_normal((3, 1, 2, 3)).astype(np.float32)
    m = modules.StereoJoin1()
    out = m.forward(dev(x))
    xd = x.astype(np.float64)
    assert tuple(out.shape) == (3, 1, 2, 3)
    np.testing.assert_allclose(out.cpu().numpy(), (xd[0::2] * xd[1::2]).sum(1, keepdims=True), rtol=RTOL)
    gi = m.backward(dev(x), dev(go)).cpu().numpy()
    np.testing.assert_allclose(gi[0::2], xd[1::2] * go.astype(np.float64), rtol=RTOL)
    np.testing.assert_allclose(gi[1::2], xd[0::2] * go.astype(np.float64), rtol=RTOL)
    xs = dev(x).requires_grad_()
    modules.stereo_join1_fn(xs).backward(dev(go))
    assert bits_equal(xs.grad.cpu().numpy(), gi)
