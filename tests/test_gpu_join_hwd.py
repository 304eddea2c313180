"""-m gpu: the (H,W,ds) StereoJoin kernels -- join_owner_kernel<8|16|32, 2>, join_mfma_kernel<56|64>, fix_border_hwd_kernel -- held to
the CPU oracle voxel by voxel.  Every call goes through the test hook mc_test_stereo_join_hwd into volumes poisoned with a NaN payload
that no kernel writes: every (pixel, d < D) voxel has to be written on every call, the NaN triangle included (the SGM sweeps leave it
untouched in a reused workspace), bit for bit the oracle's fmaf chain, and nothing outside the volume.  Each case runs once for both
volumes and once for either volume alone (C > 64: both only).  The tables, what they are after and the helpers are in
tests/join_cases.py; tests/test_join_cases_host.py shows on the oracle alone that the value-range cases are in their ranges."""
import pytest

import join_cases as jc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("W", jc.OWNER_W)
def test_owner_geometry(mc, oracle, W):
    """ring and line writer: D around the multiples of 32 x every class of ds mod 32, rows in the second group of eight, the volume's
    base 16-byte but not always 128-byte aligned"""
    for H, W, D, ds, lead in jc.owner_cases(W):
        jc.check_case(mc, oracle, "unit", jc.OWNER_C, H, W, D, ds, lead=lead)


@pytest.mark.parametrize("H,W,D,ds", jc.OWNER_ROWS)
def test_owner_rows(mc, oracle, H, W, D, ds):
    for lead in (0, 12):
        jc.check_case(mc, oracle, "unit", jc.OWNER_C, H, W, D, ds, lead=lead)


@pytest.mark.parametrize("W", jc.MFMA_W)
@pytest.mark.parametrize("C", jc.MFMA_C)
def test_mfma_geometry(mc, oracle, C, W):
    """the wide-C kernel: tiles on the image's edges, D > W (virtual tiles that write only the right volume's triangle)"""
    for H, W, D, ds, lead in jc.mfma_cases(W):
        jc.check_case(mc, oracle, "unit", C, H, W, D, ds, lead=lead)


@pytest.mark.parametrize("C", jc.CHANNELS)
def test_channel_edges(mc, oracle, C):
    """both sides of every instance's k-step count: odd C and C below the instance's 2 * KSTEPS run zero-padded k-steps"""
    for H, W, D, ds in jc.CHANNEL_SHAPES:
        jc.check_case(mc, oracle, "unit", C, H, W, D, ds)


@pytest.mark.parametrize("H,W,D", jc.BORDER_SHAPES)
@pytest.mark.parametrize("C", jc.BORDER_C)
def test_border(mc, oracle, C, H, W, D):
    for n in jc.border_ns(W):
        jc.check_case(mc, oracle, "unit", C, H, W, D, jc.r4(D), n=n)


@pytest.mark.parametrize("C", jc.VALUE_C)
@pytest.mark.parametrize("recipe", jc.RECIPES)
def test_value_ranges(mc, oracle, recipe, C):
    """sums that overflow while no product does on its own and the reverse, subnormal products and sums, zeros of both signs, +-inf and
    NaN operands: the matrix cores' chain is the oracle's fmaf chain there too"""
    H, W, D = jc.VALUE_SHAPE
    jc.check_case(mc, oracle, recipe, C, H, W, D, jc.r4(D))


def test_refusals(mc):
    """a call that the hook or the launcher refuses returns MC_REQUIRE's code and writes nothing"""
    H, W, D, ds, C = 3, 40, 20, 20, 16
    fn = jc.bind(mc)
    f = torch.from_numpy(jc.feats("unit", 128, H, W).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    (bl, vl), (br, vr) = jc.poisoned_volume(H, W, 24), jc.poisoned_volume(H, W, 24)   # (room for every ds below)
    fl, fr, pl, pr = f[0].data_ptr(), f[1].data_ptr(), vl.data_ptr(), vr.data_ptr()
    good = dict(fl=fl, fr=fr, pl=pl, pr=pr, C=C, D=D, ds=ds, H=H, W=W, n=4, sides=3)
    cases = [("no side", dict(sides=0)), ("sides = 4", dict(sides=4)),
             ("left alone, C = 65", dict(sides=1, C=65)), ("right alone, C = 65", dict(sides=2, C=65)),
             ("ds % 4 != 0", dict(ds=22)), ("ds < D", dict(ds=16)),
             ("left volume 4 bytes off", dict(pl=pl + 4)), ("right volume 4 bytes off", dict(pr=pr + 4)),
             ("n = W", dict(n=W)), ("C = 0", dict(C=0)), ("C = 129", dict(C=129)),
             ("featL null", dict(fl=None)), ("featR null", dict(fr=None)), ("volL null", dict(pl=None)), ("volR null", dict(pr=None))]
    for what, change in cases:
        a = dict(good, **change)
        rc = fn(a["fl"], a["fr"], a["pl"], a["pr"], a["C"], a["D"], a["ds"], a["H"], a["W"], a["n"], a["sides"], st)
        assert rc == jc.EINVAL, "%s: returned %d" % (what, rc)
        assert mc._lib.lib.mc_last_error(), what
    torch.cuda.synchronize()
    assert jc.all_poison(bl.cpu().numpy()) and jc.all_poison(br.cpu().numpy())
    a = good   # (and the call they all differ from is taken)
    assert fn(a["fl"], a["fr"], a["pl"], a["pr"], a["C"], a["D"], a["ds"], a["H"], a["W"], a["n"], a["sides"], st) == 0
    torch.cuda.synchronize()
    assert not jc.all_poison(bl.cpu().numpy()) and not jc.all_poison(br.cpu().numpy())
