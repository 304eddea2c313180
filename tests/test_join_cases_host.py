"""CPU: the oracle alone over the tables of tests/join_cases.py -- what tests/test_gpu_join_hwd.py and the (D,H,W) cases of
tests/test_gpu_parity.py compare the StereoJoin kernels with.  A comparison of value ranges says something only if the oracle's
voxels are in the range that the recipe is named after; a table of channel counts or shapes only if it has a value on either side
of every point at which the kernels take another path."""
import numpy as np
import pytest

import join_cases as jc


def left_live(oracle, recipe, C):
    """the left volume's voxels that have a partner pixel (d <= x), of the value-range shape"""
    H, W, D = jc.VALUE_SHAPE
    return jc.want_of(oracle, recipe, C, H, W, D)[0][:, jc.live_left(D, W)]


@pytest.mark.parametrize("C", jc.VALUE_C)
def test_huge_overflows_without_nan(oracle, C):
    """about half of the voxels overflow, and no inf - inf forms: the product inside an fma is exact.  A multiply-then-add chain over
    the same features overflows (or gives NaN) in voxels that the fused chain keeps finite, which is what tells the two apart."""
    H, W, D = jc.VALUE_SHAPE
    k = jc.classes(left_live(oracle, "huge", C))
    print("huge C=%d: %.3f infinite, %.3f NaN" % (C, k["inf"], k["nan"]))
    assert 0.2 <= k["inf"] <= 0.8 and k["nan"] == 0
    f = jc.feats("huge", C, H, W)
    want = jc.want_of(oracle, "huge", C, H, W, D)[0]
    lost = nans = 0
    with np.errstate(all="ignore"):
        for d in range(D):
            acc = np.zeros((H, W - d), np.float32)
            for c in range(C):   # sum -= L * R with the product rounded on its own
                acc = acc - f[0, c, :, d:] * f[1, c, :, :W - d]
            nans += int(np.isnan(acc).sum())
            lost += int((~np.isfinite(acc) & np.isfinite(want[:, d:, d])).sum())
    print("        a multiply-then-add chain: %d NaN, %d voxels not finite that the fused chain keeps finite" % (nans, lost))
    if C <= 64:   # a product is about 2^128 n1 n2 / sqrt(C): in wider features it is the sums that overflow, hardly ever a product alone
        assert lost >= 10


@pytest.mark.parametrize("C", jc.VALUE_C)
def test_edge_straddles_the_smallest_normal_number(oracle, C):
    k = jc.classes(left_live(oracle, "edge", C))
    print("edge C=%d: %.3f subnormal, %.3f normal" % (C, k["subnormal"], k["normal"]))
    assert 0.2 <= k["subnormal"] <= 0.8
    assert k["nan"] == 0 and k["inf"] == 0 and k["pos_zero"] == 0 and k["neg_zero"] == 0   # the rest is normal


@pytest.mark.parametrize("C", jc.VALUE_C)
def test_tiny_is_subnormal_with_zeros_of_both_signs(oracle, C):
    k = jc.classes(left_live(oracle, "tiny", C))
    print("tiny C=%d: %.3f subnormal, %d of +0, %d of -0" % (C, k["subnormal"], k["pos_zero"], k["neg_zero"]))
    assert k["pos_zero"] >= 10 and k["neg_zero"] >= 10 and k["subnormal"] >= 0.9


@pytest.mark.parametrize("C", jc.VALUE_C)
def test_specials_reach_every_class(oracle, C):
    H, W, D = jc.VALUE_SHAPE
    k = jc.classes(left_live(oracle, "specials", C))
    print("specials C=%d: %.3f NaN, %.3f infinite, %.3f normal" % (C, k["nan"], k["inf"], k["normal"]))
    assert k["nan"] >= 0.05 and k["inf"] >= 0.05 and k["normal"] >= 0.05
    f = jc.feats("specials", C, H, W)
    for value, _ in jc.SPECIALS:   # every special value is there, in both feature maps
        for side in (0, 1):
            hit = np.isnan(f[side]) if value != value else (f[side] == value) & (np.signbit(f[side]) == np.signbit(value))
            assert hit.sum() >= 10, (value, side)


def test_the_dhw_value_cases_are_in_their_range(oracle):
    for recipe, C, (H, W, D) in jc.DHW_VALUES:
        k = jc.classes(jc.want_of(oracle, recipe, C, H, W, D)[0][:, jc.live_left(D, W)])
        print("dhw %s C=%d: %.3f infinite, %.3f subnormal, %.3f NaN" % (recipe, C, k["inf"], k["subnormal"], k["nan"]))
        assert k["nan"] == 0 and 0.2 <= k["inf" if recipe == "huge" else "subnormal"] <= 0.8


def test_the_channels_sit_on_both_sides_of_every_instance(oracle):
    """the boundaries are the launcher's own: a new instance of either kernel wants a channel count on either side of it here"""
    edges, top = jc.join_boundaries()
    print("k-step boundaries", edges, "largest", top)
    assert edges and edges == sorted(edges) and top > edges[-1]
    ks = set((C + 1) // 2 for C in jc.CHANNELS)
    for e in edges:
        assert e in ks and e + 1 in ks, e
    assert top in ks and 2 * top in jc.CHANNELS and 1 in jc.CHANNELS
    assert any(C % 2 for C in jc.CHANNELS) and any(C % 2 == 0 for C in jc.CHANNELS)   # a zero-padded last k-step, and none
    owner_top = max(e for e in edges if e < top and 2 * e <= 64)
    for group in (jc.VALUE_C, jc.BORDER_C):   # both kernel families
        assert any((C + 1) // 2 <= owner_top for C in group) and any((C + 1) // 2 > owner_top for C in group)
    assert jc.OWNER_C <= 2 * edges[0] and sorted((C + 1) // 2 > edges[-1] for C in jc.MFMA_C) == [False, True]
    assert all((C + 1) // 2 > owner_top for C in jc.MFMA_C)


def test_the_geometry_tables_reach_every_path():
    for name, cases, widths, depths in (("owner", jc.owner_cases, jc.OWNER_W, jc.OWNER_D), ("mfma", jc.mfma_cases, jc.MFMA_W, jc.MFMA_D)):
        assert any(W < 32 for W in widths) and any(32 < W <= 64 for W in widths) and any(W > 64 for W in widths)
        assert any(((W + 31) // 32) % 2 == 1 and W > 32 for W in widths), name       # an odd tile count: the second own tile is outside the image
        for edge in (32, 64):
            assert any(D < edge for D in depths) and any(D > edge for D in depths) and (edge in depths or name == "mfma" and edge == 64)
        assert any(D > W for W in widths for D in depths) and 1 in widths and 1 in depths
        for W in widths:
            for H, W_, D, ds, lead in cases(W):
                assert W_ == W and ds % 4 == 0 and ds >= D and lead % 4 == 0
    owner = [c for W in jc.OWNER_W for c in jc.owner_cases(W)]
    assert len(owner) == len(jc.OWNER_W) * len(jc.OWNER_D) * len(jc.OWNER_DS_EXTRA)
    assert set(ds % 32 for _, _, _, ds, _ in owner) == set(range(0, 32, 4))           # every class of ds mod 32
    assert set(lead for _, _, _, _, lead in owner) == set(jc.LEADS) and any(lead % 32 for lead in jc.LEADS) and 0 in jc.LEADS
    assert any(ds > jc.r4(D) for _, _, D, ds, _ in owner) and any(ds == jc.r4(D) for _, _, D, ds, _ in owner)
    for W in jc.OWNER_W:    # every D of a width meets a base that is 128-byte aligned and one that is not
        by_d = {}
        for _, _, D, _, lead in jc.owner_cases(W):
            by_d.setdefault(D, set()).add(lead % 32 != 0)
        assert all(v == {False, True} for v in by_d.values())
    assert jc.OWNER_H > 8 and jc.MFMA_H > 8                                              # rows in the second group of eight
    assert sorted(H for H, _, _, _ in jc.OWNER_ROWS) == [1, 17]
    for H, W, D in jc.BORDER_SHAPES:
        ns = jc.border_ns(W)
        assert ns[0] == 0 and ns[-1] == W - 1 and all(0 <= n < W for n in ns)
    assert any(D > W and D > 64 for _, W, D in jc.BORDER_SHAPES)


def test_want_hwd_is_the_oracles_join_and_border(oracle):
    """the triangle is NaN, the border pixels repeat the (n+1)-th pixel, D > W leaves NaNs in the copied column"""
    H, W, D, n = 5, 33, 70, 4
    wl, wr = jc.want_of(oracle, "unit", 16, H, W, D, n)
    pl, pr = jc.want_of(oracle, "unit", 16, H, W, D, 0)
    assert wl.shape == wr.shape == (H, W, D)
    assert np.isnan(pl[:, ~jc.live_left(D, W)]).all() and not np.isnan(pl[:, jc.live_left(D, W)]).any()
    assert np.isnan(pr[:, ~jc.live_right(D, W)]).all() and not np.isnan(pr[:, jc.live_right(D, W)]).any()
    for i in range(n):
        assert jc.same_bits(wl[:, W - 1 - i], pl[:, W - 1 - n]) and jc.same_bits(wr[:, i], pr[:, n])
    assert jc.same_bits(wl[:, :W - n], pl[:, :W - n]) and jc.same_bits(wr[:, n:], pr[:, n:])
    assert np.isnan(wl[:, W - 1]).any() and np.isnan(wr[:, 0]).any()


def test_check_volume_sees_what_it_is_there_for(oracle):
    """a voxel left unwritten, a wrong bit, a wrong NaN, a store outside the volume: each fails; the padding is free"""
    H, W, D, ds = 3, 33, 34, 44
    want = jc.want_of(oracle, "unit", 3, H, W, D)[0]
    poison = np.array([jc.POISON], np.int32).view(np.float32)[0]

    def good():
        got = np.full((H, W, ds), poison, np.float32)
        got[..., :D] = want
        return got, (np.full(jc.GUARD, jc.POISON, np.int32), np.full(jc.GUARD, jc.POISON, np.int32))

    got, guards = good()
    jc.check_volume(got, want, D, guards)
    got[1, 2, D:] = 7.0                                     # nobody's
    jc.check_volume(got, want, D, guards)
    for y, x, d in ((0, 0, D - 1), (2, 5, 20), (1, W - 1, 0)):   # the triangle (NaN in the oracle) and live voxels alike
        got, guards = good()
        got[y, x, d] = poison
        with pytest.raises(AssertionError, match="never written"):
            jc.check_volume(got, want, D, guards)
    got, guards = good()
    got[2, 20, 3] = np.nextafter(got[2, 20, 3], np.float32(1))
    with pytest.raises(AssertionError, match="first at"):
        jc.check_volume(got, want, D, guards)
    got, guards = good()
    got[2, 20, 30] = 0.0                                    # a number in the triangle
    with pytest.raises(AssertionError, match="nan-mask"):
        jc.check_volume(got, want, D, guards)
    for k in (0, 1):
        got, guards = good()
        guards[k][-1 if k == 0 else 0] = 0
        with pytest.raises(AssertionError, match="wrote"):
            jc.check_volume(got, want, D, guards)
