"""-m gpu: the fused SGM schedule's recomputing vertical launches (mc-cnn_amd/csrc/sgm.hip: MODE 4 and sgm_updown_line).

Where D <= 256 the down sweep no longer writes (out + out2) + L_down for the up sweep to read: a first launch keeps L_down at every
B-th row (B = SGM_CK_ROWS = 8) in a checkpoint area of the workspace, and a second one walks each column's blocks of B rows from the
bottom, recomputes L_down inside the block and runs the up recurrence over it.  Every output of mc_predict must keep its bits.  Each case
runs the same call with the two-launch form and with the recomputing one out of one library (mc_test_sgm_vertical 1 / 2) and compares
every output bit for bit, NaN masks included, with the CPU oracle and the two forms with each other:
  heights 1, 2, B-1, B, B+1, 2B, 2B+1, 3B+5 (no checkpoint at all, a bottom block of one row, exact multiples);
  W x D 20x36 (W < D: every column trimmed), 36x36, 70x36, 70x35 (D % 4 != 0);
  volumes from features (the NaN-triangle promise) and raw volumes with finite costs in the triangle (no promise);
  all exports, left.bin only and none (the last two drop the right volume's final costs), one lane and two;
  the workspace, checkpoint area included, pre-filled with NaN and with 1e3;
  with and without a border, one and two SGM iterations; caller streams; graph capture with three replays;
  at KITTI's size, where a late wave's first rows showed a store-data hazard that small shapes do not reach: the accurate path on raw volumes whose
  triangle is NaN (both volumes in one launch, no arg-min) and the fast path on one lane with two iterations, each run three times."""
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

B = 8   # SGM_CK_ROWS (mc-cnn_amd/csrc/launchers.h)
HEIGHTS = [1, 2, B - 1, B, B + 1, 2 * B, 2 * B + 1, 3 * B + 5]
WD = [(20, 36), (36, 36), (70, 36), (70, 35)]
SPLIT, RECOMPUTE = 1, 2
FORMS = [
    ("all exports", ("volL", "volR", "dispL0", "dispR0")),
    ("left.bin only", ("volL", "dispL0", "dispR0")),
    ("no export", ()),
]


@pytest.fixture(autouse=True)
def switches(mc):
    vertical, lanes = mc._lib.lib.mc_test_sgm_vertical, mc._lib.lib.mc_test_predict_lanes
    for fn in (vertical, lanes):
        fn.argtypes, fn.restype = [C.c_int], C.c_int
    assert vertical(-1) == RECOMPUTE   # the default
    yield vertical, lanes
    vertical(0)
    lanes(0)


class FilledWorkspace:
    """mc_predict's workspace, every float of it `fill` before the call"""

    def __init__(self, nbytes, fill):
        self.nbytes = nbytes
        self.buf = torch.full(((nbytes + 256) // 4 + 1,), fill, dtype=torch.float32, device="cuda")
        self.ptr = self.buf.data_ptr() + (-self.buf.data_ptr()) % 256


def run(mc, prm, xb, D, outs, fill, feat=None, raw=None):
    """mc_predict on a filled workspace writing `disp` and the outputs named in `outs`; host arrays"""
    from mc_cnn_amd._lib import check, lib

    p = mc.make_params(prm)
    H, W = xb.shape[-2:]
    x = xb.reshape(2, H, W)
    x0, x1 = x[0].contiguous(), x[1].contiguous()
    need = mc.predict.workspace_bytes(prm, D, H, W)
    ws = FilledWorkspace(mc.predict.workspace_bytes(prm, D, H, W, full=True), fill)   # with the checkpoint slots, filled like the rest
    assert ws.nbytes > need
    res = {"disp": torch.empty((1, 1, H, W), dtype=torch.float32, device="cuda")}
    for k in outs:
        res[k] = torch.empty((1, D if k.startswith("vol") else 1, H, W), dtype=torch.float32, device="cuda")
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
    slots = ws.buf.view(torch.uint8)[ws.ptr - ws.buf.data_ptr() + need:ws.ptr - ws.buf.data_ptr() + ws.nbytes].view(torch.float32)
    written = bool((slots != fill).any().item()) if fill == fill else bool((~torch.isnan(slots)).any().item())
    return {k: v.cpu().numpy() for k, v in res.items()}, written


def check_all(mc, switches, prm, xb, D, want, lanes_list, applies=True, **kw):
    """export forms x workspace fills x lanes x the two vertical forms: each output against the oracle and against the two-launch form"""
    from util import diff_report, same_bits

    vertical, lanes = switches
    for form, outs in FORMS:
        for fill in (float("nan"), 1e3):
            for nl in lanes_list:
                assert lanes(nl) == nl
                got = {}
                for mode in (SPLIT, RECOMPUTE):
                    assert vertical(mode) == mode
                    got[mode], written = run(mc, prm, xb, D, outs, fill, **kw)
                    # the form that ran: only the recomputing one writes the checkpoint slots, and only where the image has a checkpoint row
                    assert written == (applies and mode == RECOMPUTE and xb.shape[-2] >= B), (form, fill, nl, mode)
                what = "%s, workspace pre-filled with %g, %d lane(s)" % (form, fill, nl)
                for k, g in got[RECOMPUTE].items():
                    w = want[k]
                    assert same_bits(g.reshape(w.shape), w), diff_report(g.reshape(w.shape), w, "%s (%s) against the oracle" % (k, what))
                    s = got[SPLIT][k]
                    assert same_bits(g, s), diff_report(g, s, "%s (%s) against the two-launch form" % (k, what))


def feature_case(H, W, D, seed):
    from util import features, smooth_pair
    x0, x1 = smooth_pair(H, W, min(D, 10), seed=seed)
    return x0, x1, features(4, H, W, seed=seed + 1)


@pytest.mark.parametrize("W,D", WD, ids=["%dx%d" % wd for wd in WD])
@pytest.mark.parametrize("H", HEIGHTS)
def test_feature_path_keeps_its_bits(mc, oracle, switches, H, W, D):
    """the triangle promise: in a trimmed column the lanes at d >= Dv neither store nor load a checkpoint"""
    prm = dict(mc.PRESETS["kitti_fast"])
    x0, x1, f = feature_case(H, W, D, seed=71)
    want = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    check_all(mc, switches, prm, xb, D, want, (1, 2), feat=torch.from_numpy(f).cuda())


@pytest.mark.parametrize("W,D", WD, ids=["%dx%d" % wd for wd in WD])
@pytest.mark.parametrize("H", HEIGHTS)
def test_raw_volumes_keep_their_bits(mc, oracle, switches, H, W, D):
    """a caller's volumes with finite costs in the triangle: no promise, every lane below D takes part in both recurrences"""
    from util import raw_volumes, smooth_pair

    prm = dict(mc.PRESETS["kitti_fast"])
    x0, x1 = smooth_pair(H, W, 10, seed=73)
    vl, vr = raw_volumes(D, H, W, seed=74)
    rng = np.random.default_rng(75)
    for v in (vl, vr):
        n = np.isnan(v)
        v[n] = rng.random(int(n.sum()), dtype=np.float32)
    want = oracle.stereo_predict(prm, x0, x1, D, rawL=vl, rawR=vr)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    check_all(mc, switches, prm, xb, D, want, (1,), raw=(torch.from_numpy(vl).cuda(), torch.from_numpy(vr).cuda()))   # (raw volumes run on one lane)


@pytest.mark.parametrize("sgm_i", [1, 2])
@pytest.mark.parametrize("border_n", [0, 4])
@pytest.mark.parametrize("H", [B + 1, 3 * B + 5])
def test_border_and_second_iteration(mc, oracle, switches, H, border_n, sgm_i):
    """a second iteration reads the first one's output (whose triangle the promise covers) and writes the checkpoints again"""
    W, D = 70, 35
    prm = dict(mc.PRESETS["kitti_fast"])
    prm["border_n"], prm["sgm_i"] = border_n, sgm_i
    x0, x1, f = feature_case(H, W, D, seed=81)
    want = oracle.stereo_predict(prm, x0, x1, D, featL=f[0], featR=f[1])
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    check_all(mc, switches, prm, xb, D, want, (1, 2), feat=torch.from_numpy(f).cuda())


KEYS = ("disp", "dispL0", "dispR0", "volL", "volR")


def same_bits_dev(a, b):
    a, b = a.reshape(-1), b.reshape(-1)
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and not bool(((na != nb) | (~na & (a.view(torch.int32) != b.view(torch.int32)))).any().item())


def test_caller_streams_and_graph_replays(mc, switches):
    """two caller streams in turn on a workspace each, then one call captured into a graph and replayed three times over a poisoned
    workspace: the recomputing form gives what the two-launch form gave eagerly"""
    from mc_cnn_amd.predict import Workspace
    from util import features, natural_pair

    vertical, lanes = switches
    H, W, D = 3 * B + 5, 72, 20
    prm = dict(mc.PRESETS["kitti_fast"])
    dev = torch.device("cuda", 0)
    pairs = []
    for k in range(2):
        x0, x1 = natural_pair(H, W, D, seed=91 + 2 * k)
        pairs.append((torch.from_numpy(np.stack([x0, x1])[:, None]).cuda(), torch.from_numpy(features(16, H, W, seed=92 + 2 * k)).cuda()))

    def predict(k, **kw):
        return mc.stereo_predict_fused(pairs[k][0], prm, D, feat=pairs[k][1], want_volumes=True, want_disp0=True, **kw)

    def assert_same(got, want, what):
        for key in KEYS:
            assert same_bits_dev(got[key], want[key]), "%s %s differs from the two-launch form's" % (what, key)

    assert lanes(2) == 2 and vertical(SPLIT) == SPLIT
    want = [predict(k) for k in range(2)]
    torch.cuda.synchronize()
    assert vertical(RECOMPUTE) == RECOMPUTE
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    spaces = [Workspace(prm, D, H, W, dev) for _ in range(2)]
    got = [None, None]
    for rnd in range(3):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                got[k] = predict((k + rnd) % 2, workspace=spaces[k])
    torch.cuda.synchronize()
    for k in range(2):
        assert_same(got[k], want[k % 2], "stream %d in turn:" % k)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=streams[0]):
        out = predict(0, workspace=spaces[0])
    for rep in range(3):
        for key in KEYS:
            out[key].fill_(-7.0)
        spaces[0].buf.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert_same(out, want[0], "replay %d:" % rep)


@pytest.mark.parametrize("config,over,nl", [("kitti_slow", {}, 1), ("kitti_fast", {"sgm_i": 2}, 1), ("kitti_fast", {}, 2)],
                         ids=["accurate-raw-volumes", "fast-one-lane-two-iterations", "fast-two-lanes"])
def test_full_size_repeats_agree_with_the_two_launch_form(mc, switches, config, over, nl):
    """370 x 1226 x 228: 2 452 (or 1 226) columns a launch, more than the chip holds at once on the checkpoint launch.  On raw volumes every lane of the
    NaN triangle stores, NaN in its first element: where the 128-bit store's data register was overwritten too early the volume held +INF there,
    differently from run to run.  Three runs of the recomputing form, each bit-equal to the two-launch form in every output."""
    import bench
    from mc_cnn_amd.predict import Workspace

    vertical, lanes = switches
    cfg = bench.CONFIGS[config]
    preset, H, W, D = cfg[:4]
    prm = dict(mc.PRESETS[preset])
    prm.update(over)
    dev = torch.device("cuda", 0)
    xb, kw, _ = bench.make_inputs(cfg, 0, dev)
    ws = Workspace(prm, D, H, W, dev)
    assert lanes(nl) == nl and vertical(SPLIT) == SPLIT
    want = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(want["volR"]).any())   # the triangle is there to be compared
    assert vertical(RECOMPUTE) == RECOMPUTE
    for rep in range(3):
        off = ws.ptr - ws.buf.data_ptr()
        ws.buf[off + ws.nbytes:off + ws.nbytes_full].zero_()
        got = mc.stereo_predict_fused(xb, prm, D, workspace=ws, want_volumes=True, want_disp0=True, **kw)
        torch.cuda.synchronize()
        assert bool(ws.buf[off + ws.nbytes:off + ws.nbytes_full].any().item()), "the recomputing form did not run"
        for key in KEYS:
            assert same_bits_dev(got[key], want[key]), "run %d: %s differs from the two-launch form's" % (rep, key)
