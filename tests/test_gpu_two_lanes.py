"""-m gpu: the fast path's two lanes.  mc_predict runs the right volume's chain (StereoJoin, border, SGM sweeps, exports) on a side
stream one stage behind the left volume's and joins in front of the LR check.  Every case runs the same call under the serial schedule
and under the two-lane one out of one library (mc_test_predict_lanes, the in-process form of MC_PREDICT_LANES) and compares disp, dispL0,
dispR0, volL and volR bit for bit, NaN masks included.  The shapes are the smallest at which a lane can go wrong: one row, rows beyond
the eight XCD slots, D no multiple of 4 or 32, every k-step instance of the owner kernel, with and without a border."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("disp", "dispL0", "dispR0", "volL", "volR")


@pytest.fixture(autouse=True)
def lanes(mc):
    fn = mc._lib.lib.mc_test_predict_lanes
    fn.argtypes, fn.restype = [C.c_int], C.c_int
    yield fn
    fn(0)   # back to what the environment says


def same_bits_dev(a, b):
    """bit-exact equality on the device with NaN == NaN, as bench.same_bits_dev"""
    a, b = a.reshape(-1), b.reshape(-1)
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    bad = (na != nb) | (~na & (a.view(torch.int32) != b.view(torch.int32)))
    return not bool(bad.any().item())


def inputs(H, W, D, Cn, seed):
    from util import features, natural_pair
    x0, x1 = natural_pair(H, W, D, seed=seed)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None]).cuda()
    return xb, torch.from_numpy(features(Cn, H, W, seed=seed + 1)).cuda()


def params(mc, border_n=4, sgm_i=1):
    prm = dict(mc.PRESETS["kitti_fast"])
    prm["border_n"], prm["sgm_i"] = border_n, sgm_i
    return prm


def predict(mc, lanes, n, xb, feat, prm, D, want_volumes=True, **kw):
    assert lanes(n) == n
    return mc.stereo_predict_fused(xb, prm, D, feat=feat, want_volumes=want_volumes, want_disp0=True, **kw)


def assert_same(got, want, what=""):
    assert set(got) == set(want)
    for k in KEYS:
        if k in want:
            assert same_bits_dev(got[k], want[k]), "%s %s differs from the serial schedule's" % (what, k)


@pytest.mark.parametrize("border_n", [0, 4])
@pytest.mark.parametrize("H,W,D,Cn", [(1, 33, 16, 16), (9, 40, 20, 16), (20, 72, 20, 26), (17, 100, 36, 3), (17, 100, 36, 64)])
def test_two_lanes_reproduce_the_serial_schedule(mc, lanes, H, W, D, Cn, border_n):
    xb, feat = inputs(H, W, D, Cn, seed=11)
    prm = params(mc, border_n)
    want = predict(mc, lanes, 1, xb, feat, prm, D)
    got = predict(mc, lanes, 2, xb, feat, prm, D)
    torch.cuda.synchronize()
    assert_same(got, want)
    assert bool(torch.isnan(want["volR"]).any())   # the triangle is there to be compared


@pytest.mark.parametrize("sgm_i", [1, 2])
@pytest.mark.parametrize("want_volumes", [False, True])
def test_options_that_change_the_right_lane(mc, lanes, want_volumes, sgm_i):
    """the right lane's exports exist only where they are asked for (without them the up sweep drops the right volume's stores), and a
    second SGM iteration swaps each lane's buffers once more"""
    H, W, D = 9, 40, 20
    xb, feat = inputs(H, W, D, 16, seed=21)
    prm = params(mc, 4, sgm_i)
    want = predict(mc, lanes, 1, xb, feat, prm, D, want_volumes=want_volumes)
    got = predict(mc, lanes, 2, xb, feat, prm, D, want_volumes=want_volumes)
    torch.cuda.synchronize()
    assert ("volR" in got) == want_volumes
    assert_same(got, want)


def test_caller_streams_and_reuse(mc, lanes):
    """a caller stream of its own; two caller streams in turn, a workspace each, nothing waiting in between; one caller stream fifty times on
    one workspace with the input changing from call to call: a join that is missing shows as the call before's right arg-min"""
    from mc_cnn_amd.predict import Workspace
    H, W, D = 20, 72, 20
    prm = params(mc)
    dev = torch.device("cuda", 0)
    pairs = [inputs(H, W, D, 16, seed=31 + 2 * k) for k in range(2)]
    want = [predict(mc, lanes, 1, xb, feat, prm, D) for xb, feat in pairs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    spaces = [Workspace(prm, D, H, W, dev) for _ in range(2)]
    with torch.cuda.stream(streams[0]):
        got = predict(mc, lanes, 2, *pairs[0], prm, D, workspace=spaces[0])
    torch.cuda.synchronize()
    assert_same(got, want[0], "own stream:")
    got = [None, None]
    for rnd in range(3):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                got[k] = predict(mc, lanes, 2, *pairs[(k + rnd) % 2], prm, D, workspace=spaces[k])
    torch.cuda.synchronize()
    for k in range(2):
        assert_same(got[k], want[k % 2], "stream %d in turn:" % k)   # the last round is rnd = 2
    with torch.cuda.stream(streams[1]):
        for i in range(50):
            got = predict(mc, lanes, 2, *pairs[i % 2], prm, D, workspace=spaces[1])
    torch.cuda.synchronize()
    assert_same(got, want[1], "fiftieth call:")
    assert not same_bits_dev(want[0]["dispR0"], want[1]["dispR0"])   # (a stale arg-min would have been seen)


def test_nothing_of_the_right_lane_runs_past_the_join(mc, lanes):
    """behind a two-lane call the caller's stream overwrites the whole workspace, and a second call follows on a second workspace: what the
    first call copied out must be the serial schedule's.  A right lane still running would read the sentinel or write its exports late."""
    from mc_cnn_amd.predict import Workspace
    H, W, D = 17, 100, 36
    prm = params(mc)
    dev = torch.device("cuda", 0)
    xb, feat = inputs(H, W, D, 64, seed=41)
    xb2, feat2 = inputs(H, W, D, 64, seed=43)
    want = predict(mc, lanes, 1, xb, feat, prm, D)
    want2 = predict(mc, lanes, 1, xb2, feat2, prm, D)
    torch.cuda.synchronize()
    ws, ws2 = Workspace(prm, D, H, W, dev), Workspace(prm, D, H, W, dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        got = predict(mc, lanes, 2, xb, feat, prm, D, workspace=ws)
        ws.buf.fill_(0xA5)
        got2 = predict(mc, lanes, 2, xb2, feat2, prm, D, workspace=ws2)
        ws2.buf.fill_(0x5A)
    torch.cuda.synchronize()
    assert_same(got, want, "first call:")
    assert_same(got2, want2, "second call:")


@pytest.mark.parametrize("H,W,D,Cn,ds,n", [(1, 33, 16, 16, 16, 4), (9, 40, 20, 16, 20, 0), (9, 40, 20, 3, 20, 4), (17, 100, 36, 64, 36, 4), (20, 72, 20, 26, 24, 4)])
def test_stereo_join_hwd_one_side_at_a_time(mc, H, W, D, Cn, ds, n):
    """the side selector: the left volume alone, then the right one alone, into NaN-poisoned volumes, against one launch for both; after
    the first of the two the other volume is still poison (a payload no kernel writes)"""
    from util import features
    fn = mc._lib.lib.mc_test_stereo_join_hwd
    vp, i = C.c_void_p, C.c_int
    fn.argtypes, fn.restype = [vp, vp, vp, vp, i, i, i, i, i, i, i, vp], i
    feat = torch.from_numpy(features(Cn, H, W, seed=51)).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def vols():
        return [torch.full((H, W, ds), 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32) for _ in range(2)]   # NaN with a payload

    def join(v, sides):
        mc._lib.check(fn(feat[0].data_ptr(), feat[1].data_ptr(), v[0].data_ptr(), v[1].data_ptr(), Cn, D, ds, H, W, n, sides, st), "mc_test_stereo_join_hwd")

    def untouched(t):
        return bool((t.view(torch.int32) == 0x7FC0BEEF).all().item())

    def live(t):   # the D disparities of every pixel: the padding up to ds is nobody's (the owner kernel stores whole 16-byte runs out of its ring)
        return t[..., :D].contiguous()

    both, one = vols(), vols()
    join(both, 3)
    join(one, 1)
    assert untouched(one[1]) and same_bits_dev(live(one[0]), live(both[0]))
    join(one, 2)
    assert same_bits_dev(live(one[0]), live(both[0])) and same_bits_dev(live(one[1]), live(both[1]))
    right_first = vols()
    join(right_first, 2)
    assert untouched(right_first[0]) and same_bits_dev(live(right_first[1]), live(both[1]))
    assert not untouched(live(both[0])) and not untouched(live(both[1]))
    assert fn(feat[0].data_ptr(), feat[1].data_ptr(), one[0].data_ptr(), one[1].data_ptr(), Cn, D, ds, H, W, n, 0, st) == -22   # no side at all


def test_a_two_lane_call_is_capturable(mc, lanes):
    """the fork and the join are events: a graph captured on the caller's stream holds both lanes, and its replays give the eager result"""
    from mc_cnn_amd.predict import Workspace
    H, W, D = 20, 72, 20
    prm = params(mc)
    dev = torch.device("cuda", 0)
    xb, feat = inputs(H, W, D, 16, seed=61)
    want = predict(mc, lanes, 1, xb, feat, prm, D)
    torch.cuda.synchronize()
    ws = Workspace(prm, D, H, W, dev)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):   # the stream's first call makes its side stream and events, and the process's first one the Gaussian table
        eager = predict(mc, lanes, 2, xb, feat, prm, D, workspace=ws)
    torch.cuda.synchronize()
    assert_same(eager, want, "eager:")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        got = predict(mc, lanes, 2, xb, feat, prm, D, workspace=ws)
    for rep in range(3):
        for k in KEYS:
            got[k].fill_(-7.0)
        ws.buf.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert_same(got, want, "replay %d:" % rep)
