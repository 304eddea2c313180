"""GPU: libmcops.so's operators (include/mc_ops.h) at their limits -- every width class of the remove_* operators on piecewise-linear
scenes, the loops that only a large tensor makes iterate, Normalize_backward_input over channel counts, tiles, seven decades of
magnitude and element offsets past 2^31, Margin2 at block edges and on non-finite scores, the bindings' size checks and the autograd
wrapper off the 1x1 case.  Every device result is compared bit for bit with the reference's own kernel (`ref.call`, oracle/_ref) and,
in a test of its own that needs no oracle/_ref, with a restatement: numpy or torch exactly for the remove_* operators, float64 for
the arithmetic ones.  The helpers are tests/test_gpu_ops.py's and tests/train_fixtures.py's."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_ops import bits_equal, margin_input, nb_case, np_nonvisible, np_occluded, np_white  # noqa: E402
from train_fixtures import dev, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ad(mc):
    import torch
    assert torch.cuda.is_available()
    return mc.adcensus


def n_differ(a, b):
    import torch
    return int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())


# ---- 1. remove_nonvisible, remove_occluded, remove_white at every width class -------------------------------------------------------
# W: rows.  Below, at and above one pass of the 256-thread workgroup, two and five passes, the widest row; rows enough for several
# of the reference's 128-thread blocks (a block of the reference spans rows at every width but 256)
SCENE_ROWS = {1: 3000, 2: 3000, 9: 200, 255: 40, 256: 40, 257: 40, 513: 40, 1242: 40, 8192: 3}
SEQUENCE = ("remove_nonvisible", "remove_occluded", "remove_occluded", "remove_white")


@functools.lru_cache(maxsize=None)
def scene_case(W):
    """A map (1, 1, rows, W) of multiples of 1/256 in [0, 2^16) and its image.  Every row is a piecewise-linear scene: segments of
    random length up to W / 6, each with a random base below min(W, 256) pixels and a slope in [-64, 64] / 256 per pixel, then 30 %
    zeros; a segment's occluders lie up to 256 pixels away.  The image is 0 .. 254 with 10 % exactly 255.  From W = 9 on row 0 is
    planted: zero except y[1] = 0.5 and y[W - 1] = W - 1 - 1 / 256, so that pixel 1 is occluded by the row's last pixel alone."""
    rng = np.random.default_rng(1000 + W)
    H = SCENE_ROWS[W]
    q = np.zeros((H, W), np.int64)                            # in units of 1 / 256
    for r in range(H):
        c = 0
        while c < W:
            n = min(int(rng.integers(1, max(1, W // 6) + 1)), W - c)
            q[r, c:c + n] = int(rng.integers(0, 256 * min(W, 256))) + int(rng.integers(-64, 65)) * np.arange(n)
            c += n
    q = np.clip(q, 0, 65536 * 256 - 1)
    q[rng.uniform(0, 1, q.shape) < 0.3] = 0
    d = (q / 256).astype(np.float32)
    x = rng.integers(0, 255, (H, W)).astype(np.float32)
    x[rng.uniform(0, 1, x.shape) < 0.1] = 255
    if W >= 9:
        d[0] = 0
        d[0, 1], d[0, W - 1] = 0.5, W - 1 - 1 / 256
        x[0, 1] = x[0, W - 1] = 0
    assert (d * 256 == np.round(d * 256)).all() and (d >= 0).all() and d.max() < 65536
    return d.reshape(1, 1, H, W), x.reshape(1, 1, H, W)


@functools.lru_cache(maxsize=None)
def scene_expected(W):
    """the numpy restatements' four stages, computed once"""
    d, x = scene_case(W)
    vis = np_nonvisible(d)
    occ = np_occluded(vis)
    return vis, occ, np_occluded(occ), np_white(x, occ)


_scene_cache = {}


def scene_stages(ad, W):
    """this library's four stages as device tensors: computed once per width and left unchanged"""
    import torch
    if W not in _scene_cache:
        d, x = scene_case(W)
        got, stages = dev(d), []
        for name in SEQUENCE:
            getattr(ad, name)(*((dev(x), got) if name == "remove_white" else (got,)))
            torch.cuda.synchronize()
            stages.append(got.clone())
        _scene_cache[W] = stages
    return _scene_cache[W]


@pytest.mark.parametrize("W", sorted(SCENE_ROWS))
def test_remove_operators_equal_the_reference_at_every_width_class(ad, ref, W):
    d, x = scene_case(W)
    got, want = scene_stages(ad, W), dev(d)
    for k, name in enumerate(SEQUENCE):
        ref.call(name, *((dev(x), want) if name == "remove_white" else (want,)))
        print("W %d, %s: %d of %d elements differ from the reference" % (W, name, n_differ(got[k], want), want.numel()))
        assert same_bits(got[k], want), (W, k, name)


@pytest.mark.parametrize("W", sorted(SCENE_ROWS))
def test_remove_operators_equal_numpy_at_every_width_class(ad, W):
    d, x = scene_case(W)
    want = scene_expected(W)
    got = [t.cpu().numpy() for t in scene_stages(ad, W)]
    for k, name in enumerate(SEQUENCE):
        assert bits_equal(got[k], want[k]), (W, k, name)
    assert bits_equal(got[1], got[2])                         # the second remove_occluded changes nothing
    if W < 9:                                                 # y >= x removes nearly everything there: equality only
        return
    counts = []
    for a, b in ((d, want[0]), (want[0], want[1]), (want[1], want[3])):      # decided by the restatement, not by the library
        counts.append((int(((a != 0) & (b == 0)).sum()), int((b != 0).sum())))
        assert counts[-1][0] >= 1 and counts[-1][1] >= 1      # every operator removes a pixel and leaves one: a no-op cannot pass
    print("W %d: (removed, left) by nonvisible %s, occluded %s, white %s" % ((W,) + tuple(counts)))
    row = [g[0, 0, 0] for g in got]
    last = np.float32(W - 1 - 1 / 256)
    assert row[0][1] == 0.5 and row[0][W - 1] == last         # both visible
    assert row[1][1] == 0 and row[1][W - 1] == last and row[3][W - 1] == last            # the inner loop reached the row's end
    assert not row[3][:W - 1].any()


@functools.lru_cache(maxsize=None)
def _occluded_alone_case():
    d, _ = scene_case(513)
    return d, np_occluded(d)


def _occluded_alone(ad):
    import torch
    got = dev(_occluded_alone_case()[0])
    ad.remove_occluded(got)
    torch.cuda.synchronize()
    return got


def test_remove_occluded_alone_equals_the_reference_on_an_unfiltered_scene(ad, ref):
    """DESIGN.md section 13's argument does not need remove_nonvisible first: maps with y >= x in them, keys x - y below 0."""
    d, _ = _occluded_alone_case()
    assert (d >= np.arange(513, dtype=np.float32)).sum() > 100
    want = dev(d)
    ref.call("remove_occluded", want)
    got = _occluded_alone(ad)
    print("%d of %d elements differ from the reference" % (n_differ(got, want), want.numel()))
    assert same_bits(got, want)


def test_remove_occluded_alone_equals_numpy_on_an_unfiltered_scene(ad):
    d, want = _occluded_alone_case()
    assert (want != d).any() and want.any()
    assert bits_equal(_occluded_alone(ad).cpu().numpy(), want)


# ---- 2. the loops that have never iterated ---------------------------------------------------------------------------------------------
def test_remove_occluded_row_loop_takes_a_second_row_per_workgroup(ad):
    """2^20 + 3 rows of W = 2: the grid is capped at 2^20 workgroups, so workgroups 0, 1, 2 take rows 2^20, 2^20 + 1, 2^20 + 2 as
    their second.  Pixel 0 of a row of two is removed where 1 - y[1] < -y[0].  The first three rows are occluded, the last three
    are not (and hold other values), so a workgroup that tests its second row against its first row's copy removes them."""
    import torch
    rows = (1 << 20) + 3
    g = torch.Generator(device="cuda").manual_seed(20)
    y = torch.randint(0, 8 * 256, (rows, 2), device="cuda", generator=g, dtype=torch.int32).float() / 256
    y[:3] = torch.tensor([0.5, 2.0], device="cuda")           # 1 - 2 < -0.5: removed
    y[-3:] = torch.tensor([0.75, 1.5], device="cuda")         # 1 - 1.5 < -0.75 is false: stays
    want = y.clone()
    want[:, 0] = torch.where(1 - y[:, 1] < -y[:, 0], torch.zeros_like(y[:, 0]), y[:, 0])
    assert (want[:3, 0] == 0).all() and (want[-3:, 0] == 0.75).all()
    removed = int(((want == 0) & (y != 0)).sum())
    assert 0 < removed < rows // 2 and int((want[:, 0] != 0).sum()) > rows // 4
    got = y.clone()
    ad.remove_occluded(got)
    torch.cuda.synchronize()
    print("%d of %d pixels removed; %d elements differ from torch" % (removed, y.numel(), n_differ(got, want)))
    assert same_bits(got[-3:], want[-3:]) and same_bits(got[:3], want[:3])
    assert same_bits(got, want)


def test_remove_occluded_row_loop_with_rows_of_three_waves(ad):
    """2^20 + 4096 rows of W = 130, for what the rows of two above cannot show: a row of two is one wave's, so the barrier between a
    workgroup's rows has nothing to order there.  Here a row takes three waves, the third with two pixels and little to do, and 4096
    workgroups take a second row; a library without that barrier had 71 wrong elements here.  Against the copy-based rule restated
    in torch on the device."""
    import torch
    W, rows = 130, (1 << 20) + 4096
    g = torch.Generator(device="cuda").manual_seed(21)
    y = torch.randint(0, 8 * 256, (rows, W), device="cuda", generator=g, dtype=torch.int32).float().div_(256)
    y[torch.randint(0, 10, (rows, W), device="cuda", generator=g, dtype=torch.int32) < 3] = 0
    occluded = torch.zeros((rows, W), dtype=torch.bool, device="cuda")
    for i in range(1, W):
        occluded[:, :W - i] |= (i - y[:, i:]) < -y[:, :W - i]
    want = torch.where(occluded, torch.zeros((), device="cuda"), y)
    tail = slice(1 << 20, None)
    removed, left = int(((want[tail] == 0) & (y[tail] != 0)).sum()), int((want[tail] != 0).sum())
    assert removed > 4096 and left > 4096
    got = y.clone()
    ad.remove_occluded(got)
    torch.cuda.synchronize()
    print("second rows: %d pixels removed, %d left; %d elements differ from torch" % (removed, left, n_differ(got, want)))
    assert same_bits(got[tail], want[tail]) and same_bits(got[:4096], want[:4096])
    assert same_bits(got, want)


BIG_W = 1242
BIG_ROWS = -(-(1 << 28) // BIG_W) + 2    # the first whole number of rows past 2^28 elements, and two more: 2^28 + 2972 elements


@pytest.fixture(scope="module")
def big(ad):
    """remove_nonvisible, then remove_white, on 2^28 + 2972 elements (1 GiB a tensor): the grid is capped at 2^20 workgroups of 256
    threads, so the elements past 2^28 are a second step of the grid-stride loop.  Maps are random multiples of 1 / 256 below
    2 * W, images 0 .. 254 with 10 % exactly 255, all made on the device.  Freed when the module's tests are over."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(28)
    shape = (1, 1, BIG_ROWS, BIG_W)
    assert (1 << 28) < BIG_ROWS * BIG_W < (1 << 28) + 3 * BIG_W
    case = {"d": torch.randint(0, 2 * BIG_W * 256, shape, device="cuda", generator=g, dtype=torch.int32).float().div_(256)}
    x = torch.randint(0, 255, shape, device="cuda", generator=g, dtype=torch.int32).float()
    x[torch.randint(0, 10, shape, device="cuda", generator=g, dtype=torch.int32) == 0] = 255
    case["x"] = x
    case["vis"] = case["d"].clone()
    ad.remove_nonvisible(case["vis"])
    case["white"] = case["vis"].clone()
    ad.remove_white(x, case["white"])
    torch.cuda.synchronize()
    yield case
    case.clear()
    del x
    torch.cuda.empty_cache()


def test_elementwise_grid_stride_loops_take_a_second_step(big):
    import torch
    d, x = big["d"], big["x"]
    col = torch.arange(BIG_W, device="cuda", dtype=torch.float32)
    zero = torch.zeros((), device="cuda")
    want = torch.where(d >= col, zero, d)
    tail = slice(1 << 28, None)
    for name, before, got in (("remove_nonvisible", d, big["vis"]), ("remove_white", big["vis"], big["white"])):
        if name == "remove_white":
            want = torch.where(x == 255, zero, want)
        removed = int(((before.reshape(-1)[tail] != 0) & (want.reshape(-1)[tail] == 0)).sum())
        left = int((want.reshape(-1)[tail] != 0).sum())
        print("%s: past element 2^28, %d removed and %d left of %d; %d elements differ from torch.where" %
              (name, removed, left, want.numel() - (1 << 28), n_differ(got, want)))
        assert removed >= 1 and left >= 1
        assert same_bits(got.reshape(-1)[tail], want.reshape(-1)[tail])
        assert same_bits(got, want)


def test_elementwise_grid_stride_loops_equal_the_reference(big, ref):
    """the reference's int indices still hold at 2^28 + 2972 elements"""
    want = big["d"].clone()
    ref.call("remove_nonvisible", want)
    print("remove_nonvisible: %d elements differ from the reference" % n_differ(big["vis"], want))
    assert same_bits(big["vis"], want)
    ref.call("remove_white", big["x"], want)
    print("remove_white: %d elements differ from the reference" % n_differ(big["white"], want))
    assert same_bits(big["white"], want)


# ---- 3. Normalize_backward_input: channels, tiles, magnitudes, offsets ----------------------------------------------------------------
# a 64-pixel tile over four images with a part-filled second sweep of 8 channels; H * W = 63, 64, 65 with C that ends a sweep
# part-way; the training layout over more than two tiles; the smallest sum; one full sweep of one wave over four tiles
NB_LIMIT_SHAPES = [(5, 9, 3, 7), (3, 63, 1, 63), (1, 65, 1, 64), (2, 100, 5, 13), (1, 127, 2, 33), (130, 64, 1, 1), (130, 7, 1, 1),
                   (1, 2, 1, 1), (1, 8, 1, 200)]
NB_MAGNITUDE_SHAPES = [(1, 64, 1, 70 * 64), (1, 128, 1, 70 * 8)]
PER_PIXEL = 1e-4    # tests/train_fast_oracle.check_per_tensor's bound on a gradient tensor, applied to each pixel's C results


def nb_float64(x, go, norm):
    """the formula in float64 on torch tensors (N, C, H, W) and norm (N, 1, H, W), on whichever device they are"""
    x, go, norm = x.double(), go.double(), norm.double()
    denom = norm ** 1.5
    xg = x * go
    others = xg.sum(1, keepdim=True) - xg                     # exact enough in float64: the sum without the own channel
    return (norm - x * x) / denom * go - others * x / denom


def per_pixel_ratio(gi, want):
    """the largest, over the pixels, of max_c |gi - want| / max_c |want|"""
    err, top = (gi.double() - want).abs().amax(1), want.abs().amax(1)
    assert bool((top > 0).all())
    return float((err / top).max())


@pytest.mark.parametrize("shape", NB_LIMIT_SHAPES)
def test_normalize_backward_equals_the_reference_at_channel_and_tile_edges(ad, ref, shape):
    import torch
    x, go, norm, gi = nb_case(ad, shape)
    want = torch.full_like(x, NAN)
    ref.call("Normalize_backward_input", go, x, norm, want)
    assert torch.isfinite(want).all()
    print("%s: %d of %d elements differ from the reference" % (shape, n_differ(gi, want), gi.numel()))
    assert same_bits(gi, want)


@pytest.mark.parametrize("shape", NB_LIMIT_SHAPES)
def test_normalize_backward_matches_float64_at_channel_and_tile_edges(ad, shape):
    import torch
    x, go, norm, gi = nb_case(ad, shape)
    want = nb_float64(x, go, norm)
    assert torch.isfinite(gi).all()
    err = float((gi.double() - want).abs().max() / want.abs().max())
    print("%s: max error %.2e of the largest magnitude; largest per-pixel ratio %.2e" % (shape, err, per_pixel_ratio(gi, want)))
    assert err <= 1e-4


_mag_cache = {}


def magnitude_case(ad, shape):
    """Pixel p's input is standard normal times 2^k, k = -14 + p % 35, so norm = sum x^2 + 1e-5 runs from 1e-5 to 1e14; every
    41st pixel is all zero (norm the float32 1e-5 exactly), every 37th has one non-zero channel (37 and 35 are coprime: at every
    k in turn).  grad_output is standard normal, norm is Normalize_forward's.  Computed once per shape and left unchanged."""
    import torch
    if shape not in _mag_cache:
        N, C, H, W = shape
        assert N == 1 and H == 1 and W % 35 == 0
        rng = np.random.default_rng(sum(shape) + 1)
        p = np.arange(W)
        x = rng.standard_normal(shape).astype(np.float32) * (2.0 ** (-14 + p % 35)).astype(np.float32)
        zero = p % 41 == 7
        single = (p % 37 == 5) & ~zero
        x[0, :, 0] *= (np.arange(C)[:, None] == (p % C)[None, :]) | ~single[None, :]
        x[..., zero] = 0
        live = (x[0, :, 0] != 0).sum(0)
        assert (live[zero] == 0).all() and (live[single] == 1).all() and (live[~single & ~zero] == C).all() and zero.sum() > 9 < single.sum()
        x, go = dev(x), dev(rng.standard_normal(shape).astype(np.float32))
        norm = torch.empty((1, 1, 1, W), device="cuda")
        ad.Normalize_forward(x, norm, torch.empty_like(x))
        gi = torch.full_like(x, NAN)
        ad.Normalize_backward_input(go, x, norm, gi)
        torch.cuda.synchronize()
        nn = norm.cpu().numpy().reshape(-1)
        assert (nn[zero].view(np.uint32) == np.float32(1e-5).view(np.uint32)).all()
        assert nn.min() == np.float32(1e-5) and (nn < 2e-5).sum() > W // 35 and nn.max() > 1e13 and np.isfinite(nn.astype(np.float32) ** 1.5).all()
        for lo in 10.0 ** np.arange(-5, 13):                  # every decade of the range holds a pixel
            assert ((nn >= lo) & (nn < 10 * lo)).any(), lo
        _mag_cache[shape] = (x, go, norm, gi)
    return _mag_cache[shape]


@pytest.mark.parametrize("shape", NB_MAGNITUDE_SHAPES)
def test_normalize_backward_equals_the_reference_over_the_range_of_norms(ad, ref, shape):
    """pins ops_normalize.hip's -ffp-contract=fast over powf(norm, 1.5f)'s range, not only around norm = C"""
    import torch
    x, go, norm, gi = magnitude_case(ad, shape)
    want = torch.full_like(x, NAN)
    ref.call("Normalize_backward_input", go, x, norm, want)
    assert torch.isfinite(want).all()
    differ = (gi.view(torch.int32) != want.view(torch.int32)).any(1).reshape(-1)
    print("%s: %d of %d elements differ from the reference, in %d pixels with norms %s" %
          (shape, n_differ(gi, want), gi.numel(), int(differ.sum()), norm.reshape(-1)[differ][:8].tolist()))
    assert same_bits(gi, want)


@pytest.mark.parametrize("shape", NB_MAGNITUDE_SHAPES)
def test_normalize_backward_matches_float64_per_pixel_over_the_range_of_norms(ad, shape):
    """A per-tensor maximum would let the pixels of small norm (large results) hide all others; the formula is scale-invariant per
    pixel, so check_per_tensor's 1e-4 is applied to each pixel's C results against that pixel's largest |expected| value."""
    import torch
    x, go, norm, gi = magnitude_case(ad, shape)
    assert torch.isfinite(gi).all()
    want = nb_float64(x, go, norm)
    ratio = per_pixel_ratio(gi, want)
    worst = int(((gi.double() - want).abs().amax(1) / want.abs().amax(1)).argmax())
    print("%s: largest per-pixel ratio %.2e, at pixel %d of norm %.3e with %d non-zero channels" %
          (shape, ratio, worst, float(norm.reshape(-1)[worst]), int((x[0, :, 0, worst] != 0).sum())))
    assert ratio <= PER_PIXEL


def test_normalize_backward_addresses_elements_past_two_to_the_31(ad):
    """(1, 128, 1, 2^24 + 67): 2^31 + 8576 elements, 8.6 GB a tensor, above the reference's int range (no ref.call).  All 128 channels
    of the first 130 pixels, the last 130, and 130 around the pixel where channel 127's element offset crosses 2^31 are gathered
    on the device and held to float64 per pixel, and bitwise to the operator run on the gathered pixels as a tensor of their own --
    the one comparison of the library with itself; the small shapes above pin that tensor to the reference.  The output is NaN
    before the launch and finite everywhere after it."""
    import torch
    C, HW = 128, (1 << 24) + 67
    free, total = torch.cuda.mem_get_info()
    print("free device memory %.1f GiB of %.1f GiB" % (free / 2.0 ** 30, total / 2.0 ** 30))
    if free < 40 << 30:
        pytest.skip("three tensors of 8.6 GB and their temporaries need 40 GiB of free device memory; %.1f GiB are free" % (free / 2.0 ** 30))
    cross = (1 << 31) - 127 * HW                              # channel 127's element 127 * HW + p reaches 2^31 at this pixel
    assert C * HW == (1 << 31) + 8576 and 65 <= cross < HW - 65
    idx = torch.cat([torch.arange(0, 130), torch.arange(HW - 130, HW), torch.arange(cross - 65, cross + 65)]).cuda()
    g = torch.Generator(device="cuda").manual_seed(31)
    x = torch.randn((1, C, 1, HW), device="cuda", generator=g)
    go = torch.randn((1, C, 1, HW), device="cuda", generator=g)
    gi = torch.empty_like(x)
    norm = torch.empty((1, 1, 1, HW), device="cuda")
    ad.Normalize_forward(x, norm, gi)
    gi.fill_(NAN)
    ad.Normalize_backward_input(go, x, norm, gi)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gi).all())
    sx, sgo, snorm, sgi = (t[:, :, :, idx].contiguous() for t in (x, go, norm, gi))
    del x, go, gi, norm
    torch.cuda.empty_cache()
    ratio = per_pixel_ratio(sgi, nb_float64(sx, sgo, snorm))
    small = torch.full_like(sx, NAN)
    ad.Normalize_backward_input(sgo, sx, snorm, small)
    torch.cuda.synchronize()
    print("largest per-pixel ratio %.2e over %d gathered pixels; %d elements differ from the operator on the gathered tensor" %
          (ratio, idx.numel(), n_differ(sgi, small)))
    assert ratio <= PER_PIXEL
    assert same_bits(sgi, small)


# ---- 4. Margin2 at block edges and with special values -------------------------------------------------------------------------------
MARGINS = [0.2, 0.0, -0.5]
MARGIN_N = [255, 256, 257, 65537]


def margin_pairs(n, margin):
    """tests/test_gpu_ops.margin_input's pairs (pair i of kind i % 3: f < 0, f > 0, f == 0 exactly) for another margin: the f == 0
    pairs become (the float32 margin, 0), and the f > 0 pairs move up by the part of the margin below 0.  f is derived in float32."""
    x, _ = margin_input(n, 0)
    x = x.reshape(n, 2).copy()
    kind = np.arange(n) % 3
    x[kind == 2] = (np.float32(margin), 0)
    x[kind == 1, 1] += np.float32(max(-margin, 0.0))
    f = (x[:, 1] - x[:, 0]) + np.float32(margin)
    assert f.dtype == np.float32
    assert ((f < 0) == (kind == 0)).all() and ((f > 0) == (kind == 1)).all() and ((f == 0) == (kind == 2)).all()
    return x.reshape(2 * n, 1, 1, 1), f


INF = np.float32(np.inf)
TINY = np.float32(2.0 ** -140)
SPECIAL_PAIRS = np.array([(-INF, INF), (INF, -INF), (INF, INF), (-INF, -INF), (0, INF), (0, -INF), (INF, 0), (-INF, 0),    # f = +-inf or NaN
                          (NAN, 0), (0, NAN), (NAN, NAN), (NAN, INF),                                                # a NaN score
                          (0, 1e-40), (TINY, 3 * TINY), (1e-40, 0), (3 * TINY, TINY)], np.float32)                    # neg - pos a denormal


def special_input(n):
    """margin_pairs at margin 0 with the special pairs planted at the start, across the first block's edge and at the end"""
    x, _ = margin_pairs(n, 0.0)
    x = x.reshape(n, 2).copy()
    k = len(SPECIAL_PAIRS)
    for at in (0, 256 - k // 2, n - k):
        x[at:at + k] = SPECIAL_PAIRS
    with np.errstate(invalid="ignore"):
        f = x[:, 1] - x[:, 0] + np.float32(0)
    sub = np.abs(f[np.isfinite(f) & (f != 0)]) < np.finfo(np.float32).tiny
    assert sub.sum() == 12 and np.isnan(f).sum() == 18 and np.isinf(f).sum() == 18
    return x.reshape(2 * n, 1, 1, 1), f


def run_margin2(ad, x, n, margin, pow_):
    import torch
    tmp, gi = torch.full((n,), NAN, device="cuda"), torch.full((2 * n, 1, 1, 1), NAN, device="cuda")
    ad.Margin2(dev(x), tmp, gi, margin, pow_)
    torch.cuda.synchronize()
    return tmp, gi


def margin_float64(x, f32, margin, pow_):
    """Margin2.lua's formulas in float64, C's fmax (which drops a NaN) included; f == 0 pairs are exactly 0 in float32 by construction"""
    n = f32.size
    xd = x.reshape(n, 2).astype(np.float64)
    with np.errstate(invalid="ignore"):
        f = xd[:, 1] - xd[:, 0] + np.float64(np.float32(margin))
        f[f32 == 0] = 0
        d = np.fmax(f, 0)
        on = (f > 0).astype(np.float64)
        tmp = d if pow_ == 1 else 0.5 * d * d
        gi = np.stack([-on, on], 1) if pow_ == 1 else np.stack([-f * on, f * on], 1)
    return tmp, gi


def check_against_float64(got, want):
    """NaN where the formula has NaN, the formula's infinity where it has one, every other element within 1e-4 of the largest
    finite magnitude (tests/test_gpu_ops.py's bound)"""
    got = got.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    top = np.abs(want[fin]).max()
    assert (np.abs(got[fin] - want[fin]).max() <= 1e-4 * top) if top else (np.abs(got[fin]).max() == 0)


def check_zero_signs(tmp, gi, f32, pow_):
    """include/mc_ops.h's zeros: pow 1 -1. * (f > 0) is -0.0 for an inactive pair, f > 0 alone +0.0; pow 2 -f * (f > 0) is -0.0 at
    f == 0 and +0.0 for f < 0, f * (f > 0) the other way round.  Finite f only."""
    fin = np.isfinite(f32)
    off, neg, zero = fin & (f32 <= 0), fin & (f32 < 0), fin & (f32 == 0)
    assert off.any() and neg.any() and zero.any() and (gi[off] == 0).all()
    if pow_ == 1:
        assert np.signbit(gi[off, 0]).all() and not np.signbit(gi[off, 1]).any()
    else:
        assert np.signbit(gi[zero, 0]).all() and not np.signbit(gi[zero, 1]).any()
        assert not np.signbit(gi[neg, 0]).any() and np.signbit(gi[neg, 1]).all()
    assert not np.signbit(tmp[~np.isnan(tmp)]).any()


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("n", MARGIN_N)
def test_margin2_equals_the_reference_at_block_edges_and_other_margins(ad, ref, n, margin, pow_):
    import torch
    x, _ = margin_pairs(n, margin)
    tmp, gi = run_margin2(ad, x, n, margin, pow_)
    wtmp, wgi = torch.full_like(tmp, NAN), torch.full_like(gi, NAN)
    ref.call("Margin2", dev(x), wtmp, wgi, margin, pow_)
    assert torch.isfinite(wtmp).all() and torch.isfinite(wgi).all()
    assert same_bits(tmp, wtmp) and same_bits(gi, wgi), (n, margin, pow_)


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("n", MARGIN_N)
def test_margin2_matches_float64_and_the_signs_of_zero_at_block_edges_and_other_margins(ad, n, margin, pow_):
    x, f32 = margin_pairs(n, margin)
    tmp, gi = (t.cpu().numpy() for t in run_margin2(ad, x, n, margin, pow_))
    gi = gi.reshape(n, 2)
    assert np.isfinite(tmp).all() and np.isfinite(gi).all()   # the last pair of the last block was written
    want_tmp, want_gi = margin_float64(x, f32, margin, pow_)
    check_against_float64(tmp, want_tmp)
    check_against_float64(gi, want_gi)
    check_zero_signs(tmp, gi, f32, pow_)


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("n", [1000, 65537])
def test_margin2_equals_the_reference_on_special_scores(ad, ref, n, pow_):
    """NaN in the same places, every other element bit for bit (the bits of a NaN are not the operator's to keep)"""
    import torch
    x, _ = special_input(n)
    tmp, gi = run_margin2(ad, x, n, 0.0, pow_)
    wtmp, wgi = torch.full_like(tmp, 7.0), torch.full_like(gi, 7.0)         # a NaN of the reference's is written, not left over
    ref.call("Margin2", dev(x), wtmp, wgi, 0.0, pow_)
    for got, want in ((tmp, wtmp), (gi, wgi)):
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        assert same_bits(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want)), (n, pow_)
    assert int(torch.isnan(wgi).sum()) == (0 if pow_ == 1 else 2 * 3 * 9)


@pytest.mark.parametrize("pow_", [1, 2])
@pytest.mark.parametrize("n", [1000, 65537])
def test_margin2_matches_float64_on_special_scores(ad, n, pow_):
    """f = +-inf, NaN and denormal: pow 1 has no NaN result (fmaxf drops it, f > 0 is false); pow 2 has -f * (f > 0) = NaN for f
    NaN and for f = -inf (inf * 0).  A denormal f > 0 is an active pair: gradient (-1, 1) at pow 1, (-f, f) at pow 2."""
    x, f32 = special_input(n)
    tmp, gi = (t.cpu().numpy() for t in run_margin2(ad, x, n, 0.0, pow_))
    gi = gi.reshape(n, 2)
    want_tmp, want_gi = margin_float64(x, f32, 0.0, pow_)
    check_against_float64(tmp, want_tmp)
    check_against_float64(gi, want_gi)
    check_zero_signs(tmp, gi, f32, pow_)
    sub = np.isfinite(f32) & (f32 > 0) & (f32 < np.finfo(np.float32).tiny)
    assert sub.sum() == 6
    if pow_ == 1:
        assert not np.isnan(tmp).any() and not np.isnan(gi).any()
        assert (tmp[sub] == f32[sub]).all() and (gi[sub] == (-1, 1)).all()
        assert (tmp[np.isnan(f32)] == 0).all() and (tmp[f32 == INF] == INF).all() and (tmp[f32 == -INF] == 0).all()
    else:
        assert (gi[sub, 1] == f32[sub]).all() and (gi[sub, 0] == -f32[sub]).all() and (tmp[sub] == 0).all()
        assert np.isnan(gi[np.isnan(f32) | (f32 == -INF)]).all() and (gi[f32 == INF] == (-INF, INF)).all()


# ---- 5. the bindings refuse wrong sizes before any launch -----------------------------------------------------------------------------
def test_bindings_refuse_wrong_sizes_and_write_nothing(ad):
    """Every call below would read or write outside a tensor if it reached the launcher; each raises ValueError first, with the
    sizes in its message, and the outputs keep what they held."""
    import torch

    def filled(*shape):
        return torch.full(shape, 3.0, device="cuda")

    x, go, norm, gi = filled(2, 4, 3, 5), filled(2, 4, 3, 5), filled(2, 1, 3, 5), filled(2, 4, 3, 5)
    outputs = [gi]
    bad_nb = [("a 3-D input", (filled(8, 3, 5), filled(8, 3, 5), norm, filled(8, 3, 5)), r"\(8, 3, 5\)"),
              ("a short grad_output", (filled(2, 3, 3, 5), x, norm, gi), r"\(2, 3, 3, 5\)"),
              ("a short grad_input", (go, x, norm, filled(1, 4, 3, 5)), r"\(1, 4, 3, 5\)"),
              ("a transposed grad_output", (filled(2, 4, 5, 3), x, norm, gi), r"\(2, 4, 5, 3\)"),
              ("a short norm", (go, x, filled(1, 1, 3, 5), gi), "15 elements"),
              ("a norm per element", (go, x, filled(2, 4, 3, 5), gi), "120 elements")]
    for what, args, word in bad_nb:
        outputs.append(args[3])
        with pytest.raises(ValueError, match="Normalize_backward_input: .*" + word):
            ad.Normalize_backward_input(*args)
    tmp, mgi = filled(4), filled(8, 1, 1, 1)
    outputs += [tmp, mgi]
    bad_margin = [("a short input", (filled(6, 1, 1, 1), tmp, mgi), "4 pairs, input 6 elements, gradInput 8"),
                  ("a short gradInput", (filled(8, 1, 1, 1), tmp, filled(4, 1, 1, 1)), "4 pairs, input 8 elements, gradInput 4"),
                  ("a long tmp", (filled(8, 1, 1, 1), filled(5), mgi), "5 pairs, input 8 elements, gradInput 8")]
    for what, args, word in bad_margin:
        outputs += [args[1], args[2]]
        with pytest.raises(ValueError, match="Margin2: .*" + word):
            ad.Margin2(*args, 0.2, 1)
    scalar = torch.tensor(3.0, device="cuda")
    outputs.append(scalar)
    for fn in (ad.remove_nonvisible, ad.remove_occluded):
        with pytest.raises(ValueError, match=r"%s: .*\(\)" % fn.__name__):
            fn(scalar)
    with pytest.raises(ValueError, match="remove_white: the image holds 4 elements, the map 8"):
        ad.remove_white(filled(4), mgi)
    torch.cuda.synchronize()
    for t in outputs:
        assert bool((t == 3.0).all())
    # what has the right sizes is taken whatever its number of dimensions: norm (N, H, W), pairs as (n, 2)
    ad.Normalize_backward_input(go, x, filled(2, 3, 5), gi)
    ad.Margin2(filled(4, 2), tmp, filled(4, 2), 0.2, 1)
    torch.cuda.synchronize()
    assert bool((gi != 3.0).any()) and bool((tmp != 3.0).all())


# ---- 6. the autograd wrappers off the 1x1 case ---------------------------------------------------------------------------------------
def _float64_autograd(x, go):
    import torch
    xd = x.detach().double().requires_grad_()
    (xd / torch.sqrt((xd * xd).sum(1, keepdim=True) + 1e-5)).backward(go.double())
    return xd.grad


@pytest.mark.parametrize("which", ["a permuted input", "a permuted upstream gradient"])
def test_normalize2_fn_takes_non_contiguous_tensors(mc, which):
    """modules.normalize2_fn on (2, 9, 5, 13) against float64 autograd of x / sqrt(sum x^2 + 1e-5), each pixel's 9 results within
    1e-4 of that pixel's largest |expected| value, where the input or the upstream gradient is a channels-last tensor permuted
    to (N, C, H, W): the wrapper has to copy it, not read its storage in the wrong order."""
    from mc_cnn_amd import modules
    rng = np.random.default_rng(6)
    shape, last = (2, 9, 5, 13), (2, 5, 13, 9)
    if which == "a permuted input":
        leaf = dev(rng.standard_normal(last).astype(np.float32)).requires_grad_()
        x, go = leaf.permute(0, 3, 1, 2), dev(rng.standard_normal(shape).astype(np.float32))
    else:
        leaf = dev(rng.standard_normal(shape).astype(np.float32)).requires_grad_()
        x, go = leaf, dev(rng.standard_normal(last).astype(np.float32)).permute(0, 3, 1, 2)
    assert tuple(x.shape) == tuple(go.shape) == shape and not (x.is_contiguous() and go.is_contiguous())
    modules.normalize2_fn(x).backward(go)
    got = leaf.grad.permute(0, 3, 1, 2) if which == "a permuted input" else leaf.grad
    ratio = per_pixel_ratio(got, _float64_autograd(x, go))
    print("%s: largest per-pixel ratio %.2e" % (which, ratio))
    assert ratio <= PER_PIXEL


def test_normalize2_backward_refuses_a_non_contiguous_input(mc):
    import torch
    from mc_cnn_amd import modules
    rng = np.random.default_rng(7)
    x = dev(rng.standard_normal((2, 5, 13, 9)).astype(np.float32)).permute(0, 3, 1, 2)
    go = dev(rng.standard_normal((2, 9, 5, 13)).astype(np.float32))
    m = modules.Normalize2()
    m.forward(x.contiguous())
    with pytest.raises(TypeError, match="contiguous float32 CUDA tensor expected"):
        m.backward(x, go)
    torch.cuda.synchronize()
    want = _float64_autograd(x.contiguous(), go)
    assert per_pixel_ratio(m.backward(x.contiguous(), go), want) <= PER_PIXEL
