"""-m gpu: mc_predict stays inside the workspace mc_predict_workspace_bytes asks for.  The workspace lies between two guard
areas of one allocation; after the call both still hold their fill pattern and every output is bit-equal to the oracle."""
import numpy as np
import pytest

from util import diff_report, features, raw_volumes, same_bits, smooth_pair

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD, FILL = 4096, 0xA5
H, W, D = 20, 72, 20

CASES = [
    # name, preset overrides, C (0 = from raw volumes), outputs compared
    ("kitti_fast", {}, 16, ("volL", "volR", "dispL0", "dispR0", "disp")),           # fast join path, no plan
    ("kitti_slow", {}, 0, ("volL", "volR", "dispL0", "dispR0", "disp")),            # two plans, the planned route
    ("mb_slow", {"cbca_i2": 2}, 0, ("volL", "volR", "dispL0", "dispR0", "disp")),
    ("kitti_slow", {"left_only": 1, "lr_check": 0}, 0, ("volL", "dispL0", "disp")),  # one plan
]


class GuardedWorkspace:
    """[guard | exactly nbytes, 256-byte aligned | guard] in one byte tensor filled with FILL"""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((GUARD + 256 + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.ptr = self.buf.data_ptr() + self.off

    def guards(self):
        return self.buf[:self.off], self.buf[self.off + self.nbytes:]


@pytest.mark.parametrize("name,over,C,compared", CASES, ids=["fast", "slow", "mb", "left_only"])
def test_predict_stays_inside_its_workspace(mc, oracle, name, over, C, compared):
    prm = dict(mc.PRESETS[name])
    prm.update(over)
    x0, x1 = smooth_pair(H, W, 10, seed=31)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    if C:
        f = features(C, H, W, seed=5)
        want = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
        kw = dict(feat=torch.from_numpy(f).cuda())
    else:
        vl, vr = raw_volumes(D, H, W, seed=7)
        want = oracle.stereo_predict(prm, x0, x1, D, rawL=vl, rawR=vr)
        kw = dict(raw=(torch.from_numpy(vl).cuda(), torch.from_numpy(vr).cuda()))
    ws = GuardedWorkspace(mc.predict.workspace_bytes(prm, D, H, W, C))
    assert ws.ptr % 256 == 0 and len(ws.guards()[0]) >= GUARD and len(ws.guards()[1]) >= GUARD
    got = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
    torch.cuda.synchronize()
    for side, g in zip(("below", "above"), ws.guards()):
        assert bool((g == FILL).all()), "mc_predict wrote %d bytes %s its workspace" % (int((g != FILL).sum()), side)
    for k in compared:
        g = got[k].cpu().numpy()
        assert same_bits(g, want[k]), diff_report(g, want[k], k)
