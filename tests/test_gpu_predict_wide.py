"""-m gpu: mc_predict at disparity ranges 513..1024.  predict.stereo_predict_fused -- one mc_predict call: StereoJoin into (H,W,Dp) volumes, the
fused SGM schedule at 16 values per lane, the post-processing -- against predict.stereo_predict, the op-by-op chain over the same library.
That chain's operators are pinned one by one at these ranges by tests/test_gpu_sgm_wide.py (cpu_oracle; sgm2: the restatement), so equality
here carries the fused path to the same ground.  disp, both exported volumes and both arg-min maps, bit for bit, NaN masks included; every
case with a workspace of mc_predict_workspace_bytes and with one of mc_predict_workspace_bytes_full (the checkpoint slots behind it, which a
range above 256 leaves unused: the two must not differ)."""
import os

import numpy as np
import pytest

from sgm2_restatement import assert_same_bits_dev, device_features, device_pair, device_raw_volumes
from util import features, raw_volumes, smooth_pair

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class PlainWorkspace:
    """a workspace of exactly mc_predict_workspace_bytes: no checkpoint slots behind it"""

    def __init__(self, mc, prm, D, H, W):
        from mc_cnn_amd.predict import workspace_bytes
        self.nbytes = workspace_bytes(prm, D, H, W)
        assert self.nbytes < workspace_bytes(prm, D, H, W, full=True)
        self.buf = torch.empty(self.nbytes + 256, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + (-self.buf.data_ptr()) % 256


CASES = [
    # preset, overrides, H, W, D, C (0: raw volumes)
    ("kitti_fast", {}, 6, 1100, 1024, 64),     # every lane full, lines longer than the range; the two lanes
    ("kitti_fast", {}, 6, 1100, 1024, 7),      # join_owner_kernel<8>
    ("kitti_fast", {}, 9, 70, 600, 64),        # the NaN triangle covers most of both volumes
    ("kitti_fast", {}, 9, 70, 600, 7),
    ("kitti_slow", {}, 9, 70, 516, 0),         # CBCA 2 + 0 on (D,H,W), transposes, the up sweep's arg-min
    ("mb_slow", {}, 9, 70, 520, 0),            # no LR check, CBCA 2 + 16: the up sweep without the arg-min
]


@pytest.mark.parametrize("full", [False, True], ids=["nbytes", "nbytes_full"])
@pytest.mark.parametrize("preset,over,H,W,D,C", CASES)
def test_fused_predict_wide(mc, preset, over, H, W, D, C, full):
    from mc_cnn_amd.predict import Workspace
    prm = dict(mc.PRESETS[preset])
    prm.update(over)
    x0, x1 = smooth_pair(H, W, 8, seed=H + D)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    if C:
        kw = dict(feat=torch.from_numpy(features(C, H, W, seed=D + C)).cuda())
    else:
        vl, vr = raw_volumes(D, H, W, seed=D)
        kw = dict(raw=(torch.from_numpy(vl).cuda(), torch.from_numpy(vr).cuda()))
    ws = Workspace(prm, D, H, W, xb.device) if full else PlainWorkspace(mc, prm, D, H, W)
    got = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
    want = mc.stereo_predict(xb, prm, D, return_all=True, **kw)
    torch.cuda.synchronize()
    for key in ("volL", "volR", "dispL0", "dispR0", "disp"):
        assert_same_bits_dev(got[key], want[key], "%s %dx%dx%d C=%d %s: fused vs op by op" % (preset, H, W, D, C, key))
    assert bool(torch.isnan(want["volL"]).any()) and float(want["dispL0"].max()) <= D - 1
    # the call as the benchmark makes it (no exports: the right volume's final costs are dropped)
    out = torch.empty((1, 1, H, W), device="cuda")
    mc.stereo_predict_fused(xb, prm, D, workspace=ws, out=out, **kw)
    assert_same_bits_dev(out, want["disp"], "%s %dx%dx%d C=%d disp without exports" % (preset, H, W, D, C))


@pytest.mark.parametrize("preset,over,C", [("kitti_fast", {}, 7), ("kitti_ad", {"cbca_i2": 1}, 0)])
def test_fused_predict_wide_on_volumes_of_two_gib(mc, preset, over, C):
    """every (H,W,Dp) volume of the workspace spans 2 GiB: the fused schedule's FAR forms of the walk at 16 values per lane -- the two horizontal
    directions at once, the down sweep, the up sweep with the arg-min (kitti_fast) and without it (a CBCA-2 pass follows).  Inputs made and
    outputs compared on the device."""
    from mc_cnn_amd.predict import Workspace
    H, W, D = 512, 1040, 1024
    assert H * W * D * 4 >= 1 << 31
    prm = dict(mc.PRESETS[preset])
    prm.update(over)
    xb = device_pair(H, W, seed=H + D)
    kw = dict(feat=device_features(C, H, W, seed=D)) if C else dict(raw=device_raw_volumes(D, H, W, seed=D))
    ws = Workspace(prm, D, H, W, xb.device)
    got = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
    torch.cuda.synchronize()
    del ws
    want = mc.stereo_predict(xb, prm, D, return_all=True, **kw)
    torch.cuda.synchronize()
    for key in ("volL", "volR", "dispL0", "dispR0", "disp"):
        assert_same_bits_dev(got[key], want[key], "%s %dx%dx%d %s: fused vs op by op at 2 GiB" % (preset, H, W, D, key))


def test_main_predict_at_disp_max_600(mc, tmp_path, monkeypatch):
    """`main.py kitti fast -a predict -net_fname random:1 -disp_max 600`: the three .bin files at the sizes of D = 600, and what they hold"""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    from mc_cnn_amd import main as mcmain
    H, W, D = 16, 96, 600
    rng = np.random.default_rng(5)
    base = gaussian_filter(rng.random((H, W + 6)), 2.0)
    base = ((base - base.min()) / np.ptp(base) * 255).astype(np.uint8)
    Image.fromarray(base[:, 6:]).save(tmp_path / "L.png")
    Image.fromarray(base[:, :W]).save(tmp_path / "R.png")
    monkeypatch.chdir(tmp_path)
    assert mcmain.main(["kitti", "fast", "-a", "predict", "-net_fname", "random:1", "-left", "L.png", "-right", "R.png",
                        "-disp_max", str(D)]) == 0
    assert os.path.getsize("left.bin") == os.path.getsize("right.bin") == 4 * D * H * W
    assert os.path.getsize("disp.bin") == 4 * H * W
    left = mc.read_bin("left.bin", (1, D, H, W))
    right = mc.read_bin("right.bin", (1, D, H, W))
    disp = mc.read_bin("disp.bin", (1, 1, H, W))
    d, x = np.arange(D)[:, None, None], np.arange(W)[None, None, :]
    # the triangles of a range six times the width (fix_border copies a shorter column's vector into the four border columns: left out here)
    assert np.array_equal(np.isnan(left[0])[:, :, :W - 4], np.broadcast_to(d > x, (D, H, W))[:, :, :W - 4])
    assert np.array_equal(np.isnan(right[0])[:, :, 4:], np.broadcast_to(x + d >= W, (D, H, W))[:, :, 4:])
    assert np.isfinite(disp).all() and disp.min() >= 0 and disp.max() < W
