"""-m gpu: parity AT THE BENCHMARKED SHAPES.  The fused mc_predict -- exactly the call bench.py times, on
exactly bench.py's inputs (bench.make_inputs) -- against main.lua's stereo_predict run over the
REFERENCE'S OWN kernels (oracle/_ref, tests/ref_pipeline.py) on the same GPU:

  kitti_fast  370x1226x228 from 64-channel features        (BASELINE.json configs[1])
  kitti_slow  370x1226x228 from raw volumes, CBCA 2+0       (configs[2])
  mb_slow     1000x1500x256 from raw volumes, CBCA 2+16     (configs[3], the north-star shape)

left.bin / right.bin volumes, both arg-min maps and disp.bin, bit for bit, NaN masks included.  The
comparison runs on the device (the volumes are 0.4 - 1.5 GB each).  These are the launches whose
geometry depends on the problem size (rows per CBCA strip, non-temporal instantiations, SGM line
counts), which no small-shape test reaches (main.lua:929-1082, 1144-1148)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def assert_same_bits_dev(got, want, name):
    """bit-exact equality on the device, NaN == NaN, NaN masks identical"""
    got = got.reshape(-1)
    want = want.reshape(-1)
    assert got.shape == want.shape, "%s: shape %s vs %s" % (name, tuple(got.shape), tuple(want.shape))
    ng, nw = torch.isnan(got), torch.isnan(want)
    bad = (ng != nw) | (~ng & (got.view(torch.int32) != want.view(torch.int32)))
    n = int(bad.sum().item())
    if n:
        idx = torch.nonzero(bad)[:5, 0]
        raise AssertionError("%s: %d of %d elements differ; first idx=%s got=%s want=%s" % (
            name, n, got.numel(), idx.tolist(), got[idx].tolist(), want[idx].tolist()))


@pytest.mark.parametrize("config", ["kitti_fast", "kitti_slow", "mb_slow"])
def test_fused_predict_at_benchmarked_shape(ref, mc, config):
    import bench
    from ref_pipeline import ref_stereo_predict
    from mc_cnn_amd.predict import Workspace
    cfg = bench.CONFIGS[config]
    preset, H, W, D, C, _ = cfg
    prm = dict(mc.PRESETS[preset])
    device = torch.device("cuda", 0)
    xb, kw, _ = bench.make_inputs(cfg, 0, device)
    ws = Workspace(prm, D, H, W, device)
    got = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
    torch.cuda.synchronize()
    want = ref_stereo_predict(ref, prm, xb, D, **kw)
    torch.cuda.synchronize()
    for key, label in (("volL", "left.bin"), ("volR", "right.bin"), ("dispL0", "left argmin"),
                       ("dispR0", "right argmin"), ("disp", "disp.bin")):
        assert_same_bits_dev(got[key], want[key], "%s %s: hip fused vs reference kernels" % (config, label))
    # the timed call (no volume export) must produce the same disp.bin
    out = torch.empty((1, 1, H, W), dtype=torch.float32, device=device)
    mc.stereo_predict_fused(xb, prm, D, workspace=ws, out=out, **kw)
    assert_same_bits_dev(out, want["disp"], "%s disp.bin (timed call form)" % config)
    # sanity on the reference side: the arg-min maps are integers in [0, D)
    for k in ("dispL0", "dispR0"):
        d = want[k]
        assert float(d.min()) >= 0 and float(d.max()) <= D - 1 and bool((d == d.round()).all())


@pytest.mark.parametrize("preset,H,W,D", [("mb_slow", 260, 700, 48), ("kitti2015_slow", 200, 640, 64), ("mb_census", 130, 500, 40)])
def test_fused_predict_on_real_scene_arm_statistics(ref, mc, preset, H, W, D):
    """the regime real images are in (tests/util.natural_pair): cbca by the tile kernel (short-arm instance for L1 <= 5, long-arm
    instance for L1 <= 14, picked by the pair's route word), both aggregation blocks, through mc_predict, against the reference's kernels"""
    from ref_pipeline import ref_stereo_predict
    from mc_cnn_amd.predict import Workspace
    from util import natural_pair, raw_volumes
    prm = dict(mc.PRESETS[preset])
    device = torch.device("cuda", 0)
    x0, x1 = natural_pair(H, W, D, seed=7, sigma=25.0)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).to(device)
    vl, vr = raw_volumes(D, H, W, seed=11)
    kw = dict(raw=(torch.from_numpy(vl).to(device), torch.from_numpy(vr).to(device)))
    ws = Workspace(prm, D, H, W, device)
    got = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
    torch.cuda.synchronize()
    want = ref_stereo_predict(ref, prm, xb, D, **kw)
    torch.cuda.synchronize()
    for key, label in (("volL", "left.bin"), ("volR", "right.bin"), ("dispL0", "left argmin"), ("dispR0", "right argmin"), ("disp", "disp.bin")):
        assert_same_bits_dev(got[key], want[key], "%s %s on the realistic pair" % (preset, label))


def _device_pair(H, W, seed):
    """a textured pair made on the device (no multi-GB host arrays): smoothed noise, the right image the left shifted by 9 pixels"""
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(seed)
    x0 = F.avg_pool2d(torch.rand((1, 1, H, W + 16), device="cuda", generator=g), 3, 1, 1)
    x1 = torch.roll(x0, -9, dims=3) + 0.02 * torch.rand(x0.shape, device="cuda", generator=g)
    return torch.cat([x0, x1])[:, :, :, :W].contiguous()


def _device_raw_volumes(D, H, W, seed):
    """tests/util.raw_volumes on the device: uniform [0, 1) with the NaN triangles (left d > x, right x + d >= W)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.arange(D, device="cuda")[:, None, None]
    x = torch.arange(W, device="cuda")[None, None, :]
    vl = torch.rand((1, D, H, W), device="cuda", generator=g).masked_fill_((d > x)[None], float("nan"))
    vr = torch.rand((1, D, H, W), device="cuda", generator=g).masked_fill_((x + d >= W)[None], float("nan"))
    return vl, vr


def _device_features(C, H, W, seed):
    """tests/util.features on the device: N(0, 1) L2-normalised over C, the right view the left shifted by 9 pixels plus noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f0 = torch.randn((1, C, H, W), device="cuda", generator=g)
    f1 = torch.roll(f0, -9, dims=3) + 0.3 * torch.randn(f0.shape, device="cuda", generator=g)
    f = torch.cat([f0, f1])
    return (f / torch.sqrt((f.double() ** 2).sum(1, keepdim=True) + 1e-5).float()).contiguous()


@pytest.mark.parametrize("preset,over,H,W,D,C", [
    # the fused sweeps on volumes of 2 GiB or more (sgm.hip: the FAR = 64-bit-address instances), 4 and 8 disparities per lane:
    # the two horizontal directions at once (MODE 0, DUAL), the down sweep (MODE 3), the up sweep with the arg-min folded in
    # (MODE 2, ARGMIN: cbca_i2 = 0) and without it (cbca_i2 > 0: CBCA-2 and the arg-min follow)
    ("kitti_fast", {}, 1400, 1536, 256, 16),
    ("kitti_ad", {"cbca_i2": 2}, 1400, 1536, 256, 0),
    ("kitti_fast", {}, 1000, 1500, 360, 16),
    ("kitti_ad", {"cbca_i2": 2}, 1000, 1500, 360, 0),
])
def test_fused_predict_on_volumes_of_two_gib(ref, mc, preset, over, H, W, D, C):
    """mc_predict where every (H,W,Dp) volume spans 2 GiB or more, against main.lua's stereo_predict over the reference's kernels,
    compared on the device"""
    from ref_pipeline import ref_stereo_predict
    from mc_cnn_amd.predict import Workspace
    assert H * W * ((D + 3) // 4 * 4) * 4 >= 1 << 31
    prm = dict(mc.PRESETS[preset])
    prm.update(over)
    xb = _device_pair(H, W, seed=H + D)
    kw = dict(feat=_device_features(C, H, W, seed=D)) if C else dict(raw=_device_raw_volumes(D, H, W, seed=D))
    ws = Workspace(prm, D, H, W, xb.device)
    got = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
    torch.cuda.synchronize()
    del ws
    want = ref_stereo_predict(ref, prm, xb, D, **kw)
    torch.cuda.synchronize()
    for key, label in (("volL", "left.bin"), ("volR", "right.bin"), ("dispL0", "left argmin"),
                       ("dispR0", "right argmin"), ("disp", "disp.bin")):
        assert_same_bits_dev(got[key], want[key], "%s %dx%dx%d %s: hip fused vs reference kernels" % (preset, H, W, D, label))
