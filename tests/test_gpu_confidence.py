"""-m gpu: mc_cost_margins (the margins form of argmin_dhw_kernel / argmin_dhw4_kernel), want_margins of stereo_predict_fused, and
confidence.sparsification on the device.

What the four maps are is the double loop of tests/confidence_cases.py (margins_oracle).  The scan applies no arithmetic to a cost, so
every comparison is exact: bit patterns (view(int32)) for c1 / c2 / c2l, equality for d1.  The shapes are the smallest at which each
form of the launch can go wrong (confidence_cases.SHAPES), each with the planted curves of confidence_cases._curves at its first and
last pixels, at two seeds."""
import functools
import itertools

import numpy as np
import pytest

import confidence_cases as cc
from util import features, random_pair

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EINVAL = -22
NAMES = ("d1", "c1", "c2", "c2l")
SENTINEL = -12345.0
IDS = ["x".join(map(str, s)) for s in cc.SHAPES]


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.int32).reshape(a.shape[-2:])


def assert_maps(got, want, what):
    for name in NAMES:
        if name in got:
            g, w = bits(got[name]), bits(want[NAMES.index(name)])
            assert np.array_equal(g, w), "%s: %s differs at %s" % (what, name, np.argwhere(g != w)[:4].tolist())


@functools.lru_cache(maxsize=None)
def on_device(shape, seed):
    return torch.from_numpy(cc.volume(*shape, seed).copy()).cuda()


def margins(mc, vol, which=NAMES, outs=None):
    """mc_cost_margins through ctypes with the outputs named in `which` (the others NULL), each filled with SENTINEL first"""
    D, H, W = vol.shape[-3:]
    outs = outs if outs is not None else {k: torch.full((H, W), SENTINEL, dtype=torch.float32, device="cuda") for k in which}
    rc = mc._lib.lib.mc_cost_margins(vol.data_ptr(), D, H, W, *(outs[k].data_ptr() if k in outs else None for k in NAMES),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize("seed", (0, 1))
@pytest.mark.parametrize("shape", cc.SHAPES, ids=IDS)
def test_the_four_maps_are_the_oracles(mc, shape, seed):
    vol = on_device(shape, seed)
    rc, got = margins(mc, vol)
    assert rc == 0, mc._lib.lib.mc_last_error()
    assert_maps(got, cc.wanted(*shape, seed), "mc_cost_margins %s seed %d" % (shape, seed))
    # the binding: the same maps, (1,1,H,W) each, and an arg-min that is mc_argmin's
    bound = mc.adcensus.cost_margins(vol[None])
    torch.cuda.synchronize()
    assert all(tuple(t.shape) == (1, 1) + shape[1:] for t in bound)
    assert_maps(dict(zip(NAMES, bound)), cc.wanted(*shape, seed), "adcensus.cost_margins")
    assert torch.equal(bound[0], mc.adcensus.argmin(vol[None]))


@pytest.mark.parametrize("shape", cc.SHAPES, ids=IDS)
def test_every_subset_of_the_outputs_gives_the_same_maps(mc, shape):
    vol = on_device(shape, 0)
    want = cc.wanted(*shape, 0)
    for r in range(1, 5):
        for which in itertools.combinations(NAMES, r):
            rc, got = margins(mc, vol, which)
            assert rc == 0 and sorted(got) == sorted(which)
            assert_maps(got, want, "outputs %s" % (which,))
    # d1_out alone is the arg-min loop itself: what mc_argmin writes
    rc, got = margins(mc, vol, ("d1",))
    assert torch.equal(got["d1"].reshape(1, 1, *shape[1:]), mc.adcensus.argmin(vol[None]))


def test_misaligned_bases_take_the_one_pixel_kernel(mc):
    """a (9,4,6) volume that starts one float into its allocation, then aligned with each output in turn one float into its own: H*W is
    a multiple of 4, so only the bases keep the launch from 16-byte accesses, which would fault or write the wrong floats"""
    shape = (9, 4, 6)
    D, H, W = shape
    want = cc.wanted(*shape, 0)
    flat = torch.from_numpy(cc.volume(*shape, 0).copy()).reshape(-1)
    room = torch.full((D * H * W + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    assert room.data_ptr() % 16 == 0
    for vol_off, out_off in ((1, {}), (1, dict.fromkeys(NAMES, 1)), (0, {"d1": 1}), (0, {"c1": 1}), (0, {"c2": 2}), (0, {"c2l": 3}), (3, {"c2": 1})):
        room.fill_(SENTINEL)
        vol = room[vol_off:vol_off + D * H * W].copy_(flat).reshape(D, H, W)
        assert vol.data_ptr() % 16 == 4 * vol_off
        back = {k: torch.full((H * W + 8,), SENTINEL, dtype=torch.float32, device="cuda") for k in NAMES}
        outs = {k: back[k][out_off.get(k, 0):out_off.get(k, 0) + H * W].reshape(H, W) for k in NAMES}
        rc, got = margins(mc, vol, outs=outs)
        assert rc == 0
        assert_maps(got, want, "volume at +%d floats, outputs at %s" % (vol_off, out_off))
        for k in NAMES:   # nothing outside a map was written
            o = out_off.get(k, 0)
            assert (back[k][:o] == SENTINEL).all() and (back[k][o + H * W:] == SENTINEL).all(), k
        assert (room[:vol_off] == SENTINEL).all() and (room[vol_off + D * H * W:] == SENTINEL).all()


def test_refusals_launch_nothing(mc):
    shape = (9, 4, 6)
    D, H, W = shape
    lib = mc._lib.lib
    vol = on_device(shape, 0)
    big = torch.full((D * H * W + H * W,), SENTINEL, dtype=torch.float32, device="cuda")   # a volume and a map in one allocation
    big[:D * H * W].copy_(vol.reshape(-1))
    inside = big[:D * H * W].reshape(D, H, W)
    outs = {k: torch.full((H, W), SENTINEL, dtype=torch.float32, device="cuda") for k in NAMES}
    p = {k: t.data_ptr() for k, t in outs.items()}
    st = torch.cuda.current_stream().cuda_stream
    step = 4 * H * W
    calls = [
        ("D < 1", (vol.data_ptr(), 0, H, W, p["d1"], p["c1"], p["c2"], p["c2l"])),
        ("H < 1", (vol.data_ptr(), D, 0, W, p["d1"], p["c1"], p["c2"], p["c2l"])),
        ("W < 1", (vol.data_ptr(), D, H, -1, p["d1"], p["c1"], p["c2"], p["c2l"])),
        ("all outputs null", (vol.data_ptr(), D, H, W, None, None, None, None)),
        ("null volume", (None, D, H, W, p["d1"], p["c1"], p["c2"], p["c2l"])),
        ("an output inside the volume", (inside.data_ptr(), D, H, W, p["d1"], inside.data_ptr() + 3 * step, p["c2"], p["c2l"])),
        ("an output on the volume's last float", (inside.data_ptr(), D, H, W, p["d1"], p["c1"], inside.data_ptr() + D * step - 4, p["c2l"])),
        ("two outputs on each other", (vol.data_ptr(), D, H, W, p["d1"], p["c1"], p["c2"], p["c2"])),
        ("two outputs one float apart", (vol.data_ptr(), D, H, W, p["d1"], p["d1"] + 4, None, None)),
    ]
    for what, args in calls:
        assert lib.mc_cost_margins(*args, st) == EINVAL, what
        assert lib.mc_last_error().decode().startswith("mc_cost_margins: "), what
        torch.cuda.synchronize()
        for k in NAMES:
            assert (outs[k] == SENTINEL).all(), (what, k)
        assert torch.equal(inside.view(torch.int32), vol.view(torch.int32)) and (big[D * H * W:] == SENTINEL).all(), what   # (NaNs: by bits)
    # ... and the same buffers are taken once the call is right
    rc, got = margins(mc, inside, outs=outs)
    assert rc == 0
    assert_maps(got, cc.wanted(*shape, 0), "after the refusals")


# ---- the fused route ---------------------------------------------------------------------------------------------------------------

FUSED = ("kitti_fast", "mb_fast")
Cf, Hf, Wf, Df = 64, 6, 40, 12
SIX = ("c1", "c2", "c2l", "c1_right", "c2_right", "c2l_right")


@functools.lru_cache(maxsize=None)
def fused_inputs():
    x0, x1 = random_pair(Hf, Wf, seed=5)
    xb = torch.from_numpy(np.stack([x0, x1])[:, None].astype(np.float32)).cuda()
    return xb, torch.from_numpy(features(Cf, Hf, Wf, seed=6)).cuda()


@pytest.mark.parametrize("preset", FUSED)
def test_fused_margins_are_the_oracles_of_the_exported_volumes(mc, preset):
    xb, feat = fused_inputs()
    prm = dict(mc.PRESETS[preset])
    res = mc.stereo_predict_fused(xb, prm, Df, feat=feat, want_margins=True, want_right=True, want_volumes=True)
    torch.cuda.synchronize()
    for side, suffix in (("volL", ""), ("volR", "_right")):
        vol = res[side].cpu().numpy()[0]
        assert np.isnan(vol).any() and np.isfinite(vol).any()          # the NaN triangle is part of what is scanned
        want = cc.margins_oracle(vol)
        got = {k: res[k + suffix] for k in ("c1", "c2", "c2l")}
        assert all(tuple(t.shape) == (1, 1, Hf, Wf) for t in got.values())
        assert_maps(got, want, "%s, %s" % (preset, side))
    # one candidate only: column 0 of the left view, column W-1 of the right one
    assert torch.isinf(res["c2"][..., 0]).all() and torch.isinf(res["c2_right"][..., Wf - 1]).all()
    assert torch.isfinite(res["c2"][..., 1:]).all() and torch.isfinite(res["c1"]).all()
    # disp and the volumes are what a call without the flag gives
    plain = mc.stereo_predict_fused(xb, prm, Df, feat=feat, want_right=True, want_volumes=True)
    torch.cuda.synchronize()
    assert sorted(set(res) - set(plain)) == sorted(SIX)
    for k in plain:
        assert np.array_equal(bits(res[k].reshape(-1, Wf)), bits(plain[k].reshape(-1, Wf))), k
    # without want_volumes the maps are the same and no volume is returned; without want_right the left three alone
    lean = mc.stereo_predict_fused(xb, prm, Df, feat=feat, want_margins=True, want_right=True)
    left = mc.stereo_predict_fused(xb, prm, Df, feat=feat, want_margins=True)
    torch.cuda.synchronize()
    assert sorted(lean) == sorted(SIX + ("disp", "disp_right", "outlier_right")) and sorted(left) == ["c1", "c2", "c2l", "disp"]
    for k in SIX:
        assert np.array_equal(bits(lean[k]), bits(res[k])), k
    for k in ("c1", "c2", "c2l", "disp"):
        assert np.array_equal(bits(left[k]), bits(res[k])), k


@pytest.mark.parametrize("preset", FUSED)
def test_fused_margins_against_op_by_op(mc, preset):
    xb, feat = fused_inputs()
    prm = dict(mc.PRESETS[preset])
    res = mc.stereo_predict_fused(xb, prm, Df, feat=feat, want_margins=True, want_right=True, want_volumes=True)
    ops = mc.stereo_predict(xb, prm, Df, feat=feat, return_all=True)
    torch.cuda.synchronize()
    for k in SIX:
        assert tuple(ops[k].shape) == (1, 1, Hf, Wf)
        assert np.array_equal(bits(res[k]), bits(ops[k])), "%s: %s, fused against op by op" % (preset, k)
    # and the measures read the same from either route, for both views
    from mc_cnn_amd import confidence
    full = mc.stereo_predict_fused(xb, prm, Df, feat=feat, want_margins=True, want_right=True, want_disp0=True, want_outlier=True,
                                   want_confidence=True)
    for view in ("left", "right"):
        a, b = confidence.measures(full, Df, view=view), confidence.measures(ops, Df, view=view)
        assert tuple(a) == tuple(b) == tuple(k for k in confidence.NAMES if view == "left" or k != "cur")
        for k in a:
            assert a[k].is_cuda and np.array_equal(bits(a[k]), bits(b[k])), (view, k)


# ---- the ranking, on the device ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cc.RANKING_CASES)
def test_sparsification_and_keep_mask_on_the_device(mc, name):
    from mc_cnn_amd import confidence
    conf, pred, actual, err_at, n = cc.ranking_case(name)
    want = cc.sparsification_oracle(conf, pred, actual, err_at, n)
    got = confidence.sparsification(*(torch.from_numpy(a.copy()).cuda() for a in (conf, pred, actual)), err_at, n=n)
    for g, w, what in zip(got, want, ("bad", "bad_oracle", "m")):
        assert g.is_cuda and g.dtype == torch.int64 and np.array_equal(g.cpu().numpy(), w), (name, what)
    assert confidence.area(got[1], got[2]) <= confidence.area(got[0], got[2])
    for fraction in (1.0, 0.5, 1.0 / 3.0):
        mask = confidence.keep_mask(torch.from_numpy(conf.copy()).cuda(), fraction)
        assert mask.is_cuda and np.array_equal(mask.cpu().numpy(), cc.keep_mask_oracle(conf, fraction)), (name, fraction)
