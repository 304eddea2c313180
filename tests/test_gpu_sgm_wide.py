"""-m gpu: disparity ranges 513..1024 -- the line walk at 16 values per lane (sgm.hip, VPL = 16) and the operators around it.

mc_sgm2 against tests/sgm2_restatement.py run on the GPU, bit for bit, NaN masks included (the C oracle's sgm2 stops at 512;
tests/test_sgm_wide_host.py holds the restatement to that oracle where both run).  D = 513 (one value in the last lane but 31), 514, 516
(the first D % 4 == 0), 640, 1000, 1023, 1024 (every lane full); shapes where the direction's NaN triangle covers most of the volume (5 x 37),
where lines run complete with W > D (3 x 1100) and a portrait (40 x 9).  A (1,H,W,D) tensor is 16-byte aligned with a pixel stride D: D % 4 == 0
runs the vector forms of the walk, every other D and every volume on an odd base the per-element ones.  Volumes of 2 GiB run the FAR forms:
that test makes, restates and compares its 2 GiB on the device in about 2 s (the restatement's 50 000 small launches: 1.0 s; it prints both times).

The other operators of the op-by-op chain at D = 513 and 1024 against cpu_oracle: they never had a limit at 512, and
tests/test_gpu_predict_wide.py leans on them."""
import functools
import time

import numpy as np
import pytest

from sgm2_restatement import PRM, assert_same_bits_dev, quantised_case, sgm2 as restated_sgm2
from util import diff_report, features, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DS = [513, 514, 516, 640, 1000, 1023, 1024]
SHAPES = [(5, 37), (3, 1100), (40, 9)]


def prm_of(tau):
    return PRM[:2] + (tau,) + PRM[3:]


@functools.lru_cache(None)
def case(H, W, D, direction):
    """the inputs on the device and what sgm2 adds to a zeroed output, restated: computed once, shared, never written to"""
    x0, x1, vol, tau = quantised_case(H, W, D, direction, seed=7 * D + H)
    x0, x1, vol = (torch.from_numpy(a).cuda() for a in (x0, x1, vol))
    want = restated_sgm2(x0, x1, vol, torch.zeros_like(vol), *prm_of(tau), direction)
    assert bool(torch.isnan(want).any()) and bool(torch.isfinite(want[:, :, 0]).all())
    return x0, x1, vol, tau, want


def odd_based(t):
    """a contiguous copy of t one float behind a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=t.device)
    assert buf.data_ptr() % 16 == 0
    o = buf[1:].view(t.shape)
    o.copy_(t)
    return o


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("D", DS)
def test_sgm2_wide(mc, H, W, D, direction):
    x0, x1, vol, tau, want = case(H, W, D, direction)
    out = torch.zeros((1, H, W, D), device="cuda")
    assert vol.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    mc.adcensus.sgm2(x0, x1, vol[None], out, None, *prm_of(tau), direction)
    assert_same_bits_dev(out, want, "sgm2 %dx%dx%d direction %d" % (H, W, D, direction))


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("D", [513, 514, 1023])
def test_sgm2_wide_on_an_odd_base(mc, H, W, D, direction):
    """D % 4 != 0 on volumes that start one float behind a 16-byte boundary: the per-element forms"""
    x0, x1, vol, tau, want = case(H, W, D, direction)
    vin = odd_based(vol[None])
    out = odd_based(torch.zeros((1, H, W, D), device="cuda"))
    assert vin.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    mc.adcensus.sgm2(x0, x1, vin, out, None, *prm_of(tau), direction)
    assert_same_bits_dev(out, want, "sgm2 on an odd base %dx%dx%d direction %d" % (H, W, D, direction))


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("H,W,D", [(5, 37, 516), (40, 9, 1023), (3, 1100, 1024)])
def test_sgm2_wide_adds_to_its_output(mc, H, W, D, direction):
    """adcensus.sgm2 ADDS the four directional costs (adcensus.cu:569,616): ((((base + L0) + L1) + L2) + L3)"""
    x0, x1, vol, tau, _ = case(H, W, D, direction)
    base = torch.from_numpy(np.random.default_rng(D).integers(1, 64, (H, W, D)).astype(np.float32) / 32).cuda()
    want = restated_sgm2(x0, x1, vol, base.clone(), *prm_of(tau), direction)
    out = base.clone()[None]
    mc.adcensus.sgm2(x0, x1, vol[None], out, None, *prm_of(tau), direction)
    assert_same_bits_dev(out, want, "sgm2 into a filled output %dx%dx%d direction %d" % (H, W, D, direction))


@pytest.mark.parametrize("D", [1024, 1023])   # the vector and the per-element FAR forms
def test_sgm2_wide_volume_of_two_gib(mc, D):
    """a volume of 2 GiB: 64-bit pixel addresses in every step.  Made, restated (about 50 000 small launches) and compared on the device.
    Measured on an MI355X: 1.8 s for D = 1024 (the file's first use of the device; inputs and mc_sgm2 0.7 s, restatement 1.0 s), 0.6 s for 1023."""
    H, W, direction = 512, 1040, -1
    assert H * W * D * 4 >= 1 << 31
    t0 = time.time()
    g = torch.Generator(device="cuda").manual_seed(D)
    x0, x1 = torch.randint(0, 4, (2, H, W), device="cuda", generator=g).float() / 8
    vol = (torch.floor(torch.rand((H, W, D), device="cuda", generator=g) * 16) + 1) / 16
    vol.masked_fill_(torch.arange(D, device="cuda")[None, None, :] > torch.arange(W, device="cuda")[None, :, None], float("nan"))
    out = torch.zeros((1, H, W, D), device="cuda")
    mc.adcensus.sgm2(x0, x1, vol[None], out, None, *prm_of(0.125), direction)
    torch.cuda.synchronize()
    t1 = time.time()
    want = restated_sgm2(x0, x1, vol, torch.zeros_like(vol), *prm_of(0.125), direction)
    torch.cuda.synchronize()
    print("2 GiB case D=%d: inputs and mc_sgm2 %.1f s, restatement %.1f s" % (D, t1 - t0, time.time() - t1))
    assert_same_bits_dev(out, want, "sgm2 on a volume of 2 GiB, D = %d" % D)


def test_sgm2_fallback_scratch_is_one_area_per_stream(mc):
    """without a usable `tmp` the Python mirror takes its cached scratch, whose size follows D above 512: one area per (device, size, stream),
    so that calls on two streams do not share the edge-class maps"""
    H, W, D, direction = 5, 37, 640, -1
    x0, x1, vol, tau, want = case(H, W, D, direction)
    need = mc._lib.lib.mc_sgm2_tmp_bytes(H, W, D)
    assert need > mc._lib.lib.mc_sgm2_tmp_bytes(H, W, 512)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    outs = []
    for stream in (torch.cuda.current_stream(), side):
        with torch.cuda.stream(stream):
            out = torch.zeros((1, H, W, D), device="cuda")
            mc.adcensus.sgm2(x0, x1, vol[None], out, torch.empty(1, device="cuda"), *prm_of(tau), direction)   # (a `tmp` that is too small)
            outs.append(out)
    torch.cuda.synchronize()
    areas = {k: v for k, v in mc.adcensus._scratch.items() if k[1] == need}
    assert {k[2] for k in areas} >= {torch.cuda.current_stream().cuda_stream, side.cuda_stream} and all(len(k) == 3 for k in mc.adcensus._scratch)
    assert len({v.data_ptr() for v in areas.values()}) == len(areas)
    for out in outs:
        assert_same_bits_dev(out, want, "sgm2 on its cached scratch")


# ---- the operators around it ---------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def assert_same(got, want, name):
    got = got.detach().cpu().numpy()
    assert same_bits(got, want), diff_report(got, want, name)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("D", [513, 1024])
def test_stereo_join_wide(mc, oracle, H, W, D):
    f = features(7, H, W, seed=D + H)
    want_l, want_r = oracle.stereo_join(f[0], f[1], D)
    fd = dev(f)
    vl = mc.adcensus.fill_nan(torch.empty((1, D, H, W), device="cuda"))
    vr = mc.adcensus.fill_nan(torch.empty((1, D, H, W), device="cuda"))
    mc.adcensus.StereoJoin(fd[0], fd[1], vl, vr)
    assert_same(vl, want_l, "StereoJoin left %dx%dx%d" % (D, H, W))
    assert_same(vr, want_r, "StereoJoin right %dx%dx%d" % (D, H, W))


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("D", [513, 1024])
def test_cbca_argmin_subpixel_wide(mc, oracle, H, W, D, direction):
    x0, x1, vol_hwd, _ = quantised_case(H, W, D, direction, seed=D + W)
    vol = np.ascontiguousarray(vol_hwd.transpose(2, 0, 1))          # (D,H,W)
    x0c, x1c = oracle.cross(x0, 5, 0.2), oracle.cross(x1, 5, 0.2)
    want = oracle.cbca(x0c, x1c, vol, direction)
    out = torch.empty((1, D, H, W), device="cuda")
    mc.adcensus.cbca(dev(x0c), dev(x1c), dev(vol), out, direction)
    assert_same(out, want, "cbca %dx%dx%d direction %d" % (D, H, W, direction))
    # (the quantised volume: ties, the first index wins; an all-NaN pixel gives index 0)
    vol[:, 0, 0] = np.nan
    xe, top = (W - 1, min(D, W) - 1) if direction == -1 else (0, min(D, W) - 1)   # the last live disparity of the pixel that has the most
    vol[top, H - 1, xe] = 1 / 64
    d0 = mc.adcensus.argmin(dev(vol)[None])
    want_d0 = oracle.argmin(vol)
    assert_same(d0, want_d0, "argmin %dx%dx%d" % (D, H, W))
    assert want_d0[H - 1, xe] == top and want_d0[0, 0] == 0
    # sub-pixel refinement at every disparity of the range, the two ends (no refinement) included
    pick = (np.arange(H * W).reshape(H, W) * 37 % D).astype(np.float32)
    pick[0, :3] = (0, D - 1, D - 2)
    sub = mc.adcensus.subpixel_enchancement(dev(pick)[None, None], dev(vol)[None], D)
    assert_same(sub, oracle.subpixel_enchancement(pick, vol), "subpixel %dx%dx%d" % (D, H, W))


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("D", [513, 1024])
def test_outlier_detection_wide(mc, oracle, H, W, D):
    rng = np.random.default_rng(D + H)
    d0 = rng.integers(0, D, (H, W)).astype(np.float32)
    d1 = rng.integers(0, D, (H, W)).astype(np.float32)
    xs = np.arange(W)[None, :]
    agree = rng.random((H, W)) < 0.4                                  # matches: d1 at the partner pixel equals d0
    for y, x in zip(*np.nonzero(agree & (xs - d0 >= 0))):
        d1[y, int(x - d0[y, x])] = d0[y, x]
    outl = torch.empty((1, 1, H, W), device="cuda")
    mc.adcensus.outlier_detection(dev(d0)[None, None], dev(d1)[None, None], outl, D)
    want = oracle.outlier_detection(d0, d1, D)
    assert_same(outl, want, "outlier_detection %dx%d disp_max %d" % (H, W, D))
    assert len(np.unique(want)) >= 2
