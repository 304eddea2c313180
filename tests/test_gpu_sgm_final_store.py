"""-m gpu: mc_predict does not store the right volume's final SGM costs unless right.bin is asked for.

Where no CBCA-2 follows the SGM, the last up sweep gives the right volume's output descriptor zero records: only the
arg-min map of that volume (the LR check's input) is written.  These cases run the same inputs with and without a
right.bin output and require disp, both arg-min maps and left.bin to be bit-identical between the two runs and to the
CPU oracle, and right.bin (when asked for) to match the oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _run(mc, prm, xb, D, feat=None, raw=None, volL=True, volR=True):
    """mc_predict with a chosen subset of the volume outputs (stereo_predict_fused always asks for both)."""
    from mc_cnn_amd._lib import check, lib
    from mc_cnn_amd.predict import Workspace

    p = mc.make_params(prm)
    H, W = xb.shape[-2:]
    x = xb.reshape(2, H, W)
    x0, x1 = x[0].contiguous(), x[1].contiguous()
    dev = xb.device
    ws = Workspace(p, D, H, W, dev)
    ws.buf.fill_(0xFF)   # NaN everywhere: a later read of costs the up sweep did not store cannot go unnoticed
    res = {k: torch.empty((1, 1, H, W), dtype=torch.float32, device=dev) for k in ("disp", "dispL0", "dispR0")}
    if volL:
        res["volL"] = torch.empty((1, D, H, W), dtype=torch.float32, device=dev)
    if volR:
        res["volR"] = torch.empty((1, D, H, W), dtype=torch.float32, device=dev)
    fl = fr = rl = rr = None
    Cn = 0
    if feat is not None:
        Cn = feat.shape[-3]
        fl, fr = feat[0].data_ptr(), feat[1].data_ptr()
    else:
        rl, rr = raw[0].data_ptr(), raw[1].data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda k: res[k].data_ptr() if k in res else None
    check(lib.mc_predict(C.byref(p), x0.data_ptr(), x1.data_ptr(), fl, fr, Cn, rl, rr, D, H, W, ws.ptr, ws.nbytes,
                         ptr("volL"), ptr("volR"), ptr("dispL0"), ptr("dispR0"), res["disp"].data_ptr(), st), "mc_predict")
    torch.cuda.synchronize()
    return res


def _same_dev(got, want, name):
    """bit-exact on the device, NaN == NaN"""
    got, want = got.reshape(-1), want.reshape(-1)
    ng, nw = torch.isnan(got), torch.isnan(want)
    bad = (ng != nw) | (~ng & (got.view(torch.int32) != want.view(torch.int32)))
    n = int(bad.sum().item())
    assert n == 0, "%s: %d of %d elements differ" % (name, n, got.numel())


def _check_subsets(mc, prm, xb, D, **kw):
    """the same call with both volumes, left.bin only and no volume: every output the runs share is the same bits"""
    both = _run(mc, prm, xb, D, volL=True, volR=True, **kw)
    for volL in (True, False):
        got = _run(mc, prm, xb, D, volL=volL, volR=False, **kw)
        for k, v in got.items():
            _same_dev(v, both[k], "%s (left.bin %s, no right.bin)" % (k, "asked" if volL else "not asked"))
        del got
    return both


CASES = [
    # preset, H, W, D, C (0: raw volumes)
    ("kitti_fast", 24, 96, 20, 16),
    ("kitti_fast", 7, 45, 70, 24),
    ("kitti_slow", 16, 80, 24, 0),
]


@pytest.mark.parametrize("preset,H,W,D,Cn", CASES)
def test_right_volume_store_skip(preset, H, W, D, Cn):
    import mc_cnn_amd as mc
    from oracle import cpu_oracle
    from util import diff_report, features, same_bits, smooth_pair

    prm = dict(mc.PRESETS[preset])
    assert prm["cbca_i2"] == 0
    x0, x1 = smooth_pair(H, W, min(D, 10), seed=11)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    kw = {}
    okw = {}
    if Cn:
        f = features(Cn, H, W, seed=12)
        kw["feat"] = torch.from_numpy(f).cuda()
        okw = dict(featL=f[0], featR=f[1])
    else:
        rng = np.random.default_rng(13)
        raw = rng.random((2, D, H, W)).astype(np.float32)
        kw["raw"] = torch.from_numpy(raw).cuda()
        okw = dict(rawL=raw[0], rawR=raw[1])
    want = cpu_oracle.stereo_predict(prm, x0, x1, D, **okw)
    both = {k: v.cpu().numpy() for k, v in _check_subsets(mc, prm, xb, D, **kw).items()}
    for k in ("volL", "volR", "dispL0", "dispR0", "disp"):
        g = both[k].reshape(want[k].shape)
        assert same_bits(g, want[k]), diff_report(g, want[k], k)


def test_right_volume_store_skip_on_volumes_of_two_gib():
    """the FAR (64-bit address) up sweep drops the same stores: 1400x1536x256 spans 2 GiB per volume"""
    import mc_cnn_amd as mc
    H, W, D, Cn = 1400, 1536, 256, 16
    assert H * W * D * 4 >= 1 << 31
    prm = dict(mc.PRESETS["kitti_fast"])
    g = torch.Generator(device="cuda").manual_seed(5)
    xb = torch.randn((2, 1, H, W), device="cuda", generator=g)
    f0 = torch.randn((1, Cn, H, W), device="cuda", generator=g)
    f = torch.cat([f0, torch.roll(f0, -9, dims=3) + 0.3 * torch.randn(f0.shape, device="cuda", generator=g)])
    f = (f / torch.sqrt((f.double() ** 2).sum(1, keepdim=True) + 1e-5).float()).contiguous()
    _check_subsets(mc, prm, xb, D, feat=f)
