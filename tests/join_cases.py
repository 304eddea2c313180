"""The case tables and helpers of tests/test_gpu_join_hwd.py (GPU: the (H,W,ds) StereoJoin kernels -- join_owner_kernel, join_mfma_kernel,
fix_border_hwd_kernel -- through the test hook mc_test_stereo_join_hwd, against the CPU oracle voxel by voxel), of the (D,H,W) cases
in tests/test_gpu_parity.py and of tests/test_join_cases_host.py (CPU: the oracle alone over the same tables, so that no GPU
comparison is vacuous).  A plain module, imported as it is; torch is imported only by the helpers that touch the device.

What the tables are after (mc-cnn_amd/csrc/stereo_join.hip):
  owner kernel   a wave owns two 32-pixel tiles of one volume; per tile step it parks 32 disparities per pixel in a 64-float ring and
                 writes the 128-byte line that became complete.  The line offset of a pixel's run is a_o = (y*W*ds + x*ds) mod 32, so
                 every class of ds mod 32 is here, with rows y > 0; D sits around the multiples of 32 (nJ = (D+30)/32 + 1 tile steps,
                 the `interior` branch, the `last` line), W around 32 and 64 (pairs of tiles, a second own tile wholly outside the
                 image), W < D, and the volume's base 16-byte but not 128-byte aligned (`lead`).
  wide-C kernel  D > W: the virtual tiles that write only the right volume's NaN triangle.
  channels       both sides of every instantiation boundary of stereo_join_hwd: odd C and C below 2*KSTEPS are the zero-padded k-steps.
  values         products and sums that are subnormal, that overflow, +-0, +-inf and NaN operands: whether the matrix cores'
                 v_mfma_f32_32x32x2_f32 is the reference's fmaf chain there too."""
import ctypes
import functools

import numpy as np

from util import diff_report, features, same_bits

POISON = 0x7FC0BEEF        # a NaN with a payload that no kernel writes
GUARD = 64                 # floats in front of a volume (plus `lead`) and behind it
EINVAL = -22               # MC_REQUIRE's code, as tests/test_gpu_two_lanes.py asserts it


def r4(D):
    return (D + 3) // 4 * 4


# ---- owner geometry: C = 3, n = 0; one test per W, each looping over D x ds --------------------------------------------------
OWNER_C = 3
OWNER_H = 9                # rows in the second group of eight
OWNER_W = (1, 2, 31, 32, 33, 63, 64, 65, 97, 130)
OWNER_D = (1, 2, 4, 21, 31, 32, 33, 34, 63, 64, 65, 70, 100)   # (21: without it no ds of the table is 24 mod 32)
OWNER_DS_EXTRA = (0, 4, 12, 28)
LEADS = (0, 4, 12, 20)
OWNER_ROWS = ((17, 65, 34, 48), (1, 97, 33, 40))      # (H, W, D, ds): three groups of eight rows; one row alone


def owner_cases(W):
    """[(H, W, D, ds, lead)] of one width, `lead` cycling"""
    out = [(OWNER_H, W, D, r4(D) + e) for D in OWNER_D for e in OWNER_DS_EXTRA]
    return [c + (LEADS[(i + i // len(LEADS)) % len(LEADS)],) for i, c in enumerate(out)]   # (a D later, each ds meets the next lead)


# ---- wide-C geometry: C = 65 is join_mfma_kernel<56>, C = 113 join_mfma_kernel<64> -------------------------------------------
MFMA_C = (65, 113)
MFMA_H = 9
MFMA_W = (1, 31, 32, 33, 64, 97, 130)
MFMA_D = (1, 2, 32, 33, 34, 65, 100)
MFMA_DS_EXTRA = (0, 4)


def mfma_cases(W):
    out = [(MFMA_H, W, D, r4(D) + e) for D in MFMA_D for e in MFMA_DS_EXTRA]
    return [c + (LEADS[(i + i // len(LEADS)) % len(LEADS)],) for i, c in enumerate(out)]   # (a D later, each ds meets the next lead)


# ---- channel edges ------------------------------------------------------------------------------------------------------------
CHANNELS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 111, 112, 113, 127, 128)
CHANNEL_SHAPES = ((9, 70, 40, 40), (3, 33, 34, 44))   # (H, W, D, ds)

# ---- border -------------------------------------------------------------------------------------------------------------------
BORDER_C = (16, 65)
BORDER_SHAPES = ((9, 40, 20), (5, 33, 70), (3, 130, 100))   # (5, 33, 70): D > W, the source column carries NaNs; D > 64, a second copy step


def border_ns(W):
    return (0, 1, 4, W - 1)


# ---- value ranges -------------------------------------------------------------------------------------------------------------
VALUE_SHAPE = (9, 70, 40)
VALUE_C = (2, 3, 17, 64, 65, 128)
RECIPES = ("huge", "edge", "tiny", "specials")
# `specials`: the shares of a feature's values that become +inf, -inf, NaN, +0 and -0 at C = SPECIALS_C.  A voxel is a sum over C
# products, so at these shares per value nearly every voxel of a wide feature would be NaN or infinite and none normal: the shares are
# scaled by SPECIALS_C / C, which keeps the number of special values per pixel, and with it the voxels' classes, alike for every C.
SPECIALS = ((np.inf, 0.02), (-np.inf, 0.02), (np.nan, 0.01), (0.0, 0.10), (-0.0, 0.05))
SPECIALS_C = 6

# ---- the (D,H,W) kernel ------------------------------------------------------------------------------------------------------
DHW_C = (1, 2, 15, 16, 17, 33, 128)
DHW_SHAPES = ((3, 1, 1), (3, 63, 31), (3, 64, 32), (3, 65, 33), (2, 129, 65))   # (H, W, D)
DHW_VALUES = (("edge", 17, (3, 65, 33)), ("huge", 17, (3, 65, 33)))


def seed_of(C, H, W):
    return 1000 * C + 10 * W + H


@functools.lru_cache(None)
def feats(recipe, C, H, W, seed=None):
    """The (2,C,H,W) float32 features of a recipe ("unit": util.features as they are), made once and never written to."""
    f = features(C, H, W, seed_of(C, H, W) if seed is None else seed)
    if recipe != "unit":
        f64 = f.astype(np.float64)
        if recipe == "huge":      # half of the sums overflow, and for C <= 64 products that overflow on their own sit in finite sums:
            #                       the fused chain's product is exact, so it stays finite there and inf - inf never forms
            f = (f64 * (2.0 ** 64 * C ** 0.25)).astype(np.float32)
        elif recipe == "edge":    # products and sums on both sides of the smallest normal number, 2^-126
            f = (f64 * (2.0 ** -63 * C ** 0.25)).astype(np.float32)
        elif recipe == "tiny":    # products around the smallest subnormal, 2^-149: sums of a few units, zeros of both signs
            f = (f64 * (2.0 ** -73 * C ** 0.5)).astype(np.float32)
        elif recipe == "specials":
            f = f.copy()
            r = np.random.default_rng(1).random(f.shape)
            lo, scale = 0.0, SPECIALS_C / C
            for value, share in SPECIALS:
                f[(r >= lo) & (r < lo + share * scale)] = value
                lo += share * scale
        else:
            raise ValueError(recipe)
    f.setflags(write=False)
    return f


def want_hwd(oracle, f, D, n):
    """(volL, volR) as (H,W,D): oracle.stereo_join, fix_border on either volume where n > 0, transposed"""
    with np.errstate(all="ignore"):
        vl, vr = oracle.stereo_join(f[0], f[1], D)
        if n > 0:
            vl, vr = oracle.fix_border(vl, n, -1), oracle.fix_border(vr, n, +1)
        return oracle.dhw_to_hwd(vl), oracle.dhw_to_hwd(vr)


_wants = {}


def want_of(oracle, recipe, C, H, W, D, n=0):
    """want_hwd of a recipe's features, computed once per case and shared (ds and lead do not enter); read-only"""
    key = (recipe, C, H, W, D, n)
    if key not in _wants:
        _wants[key] = want_hwd(oracle, feats(recipe, C, H, W), D, n)
        for a in _wants[key]:
            a.setflags(write=False)
    return _wants[key]


def live_left(D, W):
    """(W, D) mask of the left volume's voxels that have a partner pixel: d <= x"""
    return np.arange(D)[None, :] <= np.arange(W)[:, None]


def live_right(D, W):
    """... of the right volume's: x + d < W"""
    return np.arange(W)[:, None] + np.arange(D)[None, :] < W


# ---- the device side ----------------------------------------------------------------------------------------------------------
def bind(mc):
    """mc_test_stereo_join_hwd(featL, featR, volL, volR, C, D, ds, H, W, border_n, sides, stream)"""
    fn = mc._lib.lib.mc_test_stereo_join_hwd
    vp, i = ctypes.c_void_p, ctypes.c_int
    fn.argtypes, fn.restype = [vp, vp, vp, vp, i, i, i, i, i, i, i, vp], i
    return fn


def poisoned_volume(H, W, ds, lead=0):
    """(buffer, volume): an int32 device buffer filled with POISON, and the (H,W,ds) float32 view of it that starts GUARD + lead floats
    in -- lead a multiple of 4, so the volume's base is 16-byte aligned and, for lead % 32 != 0, not 128-byte aligned; GUARD floats
    follow the volume's end."""
    import torch
    assert lead % 4 == 0 and lead >= 0
    n = H * W * ds
    buf = torch.full((GUARD + lead + n + GUARD,), POISON, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 128 == 0
    vol = buf[GUARD + lead:GUARD + lead + n].view(torch.float32).view(H, W, ds)
    assert vol.data_ptr() % 16 == 0 and (vol.data_ptr() % 128 != 0) == (lead % 32 != 0)
    return buf, vol


def fetch(buf, H, W, ds, lead=0):
    """(volume as (H,W,ds) float32, (front guard, back guard) as int32) of a poisoned_volume's buffer, on the host"""
    a = buf.cpu().numpy()
    n = H * W * ds
    at = GUARD + lead
    return a[at:at + n].view(np.float32).reshape(H, W, ds), (a[:at], a[at + n:])


def all_poison(a):
    return bool((np.ascontiguousarray(a).view(np.int32) == POISON).all())


def check_volume(got, want, D, guards, what=""):
    """got (H,W,ds) against the oracle's (H,W,D): no voxel of [..., :D] is still poison (as int32, in front of any comparison that
    takes one NaN for another), [..., :D] equals the oracle bit for bit with its NaN mask, and both guards are untouched.  [..., D:ds]
    is nobody's (the owner kernel stores whole 16-byte runs out of its ring): nothing is asserted about it."""
    live = np.ascontiguousarray(got[..., :D])
    stale = live.view(np.int32) == POISON
    assert not stale.any(), "%s: %d of %d voxels were never written, first (y, x, d) = %s" % (
        what, int(stale.sum()), stale.size, tuple(int(v) for v in np.argwhere(stale)[0]))
    assert same_bits(live, want), diff_report(live, want, what) + first_difference(live, want)
    assert all_poison(guards[0]), "%s: wrote in front of the volume" % what
    assert all_poison(guards[1]), "%s: wrote behind the volume" % what


def first_difference(got, want):
    """the first differing voxel and both bit patterns, for a message"""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    ng, nw = np.isnan(g), np.isnan(w)
    bad = np.argwhere((ng != nw) | (~ng & ~nw & (g.view(np.uint32) != w.view(np.uint32))))
    if not len(bad):
        return ""
    i = tuple(int(v) for v in bad[0])
    return "; first at %s: got 0x%08X, want 0x%08X" % (i, int(g.view(np.uint32)[i]), int(w.view(np.uint32)[i]))


def run_join(mc, f_dev, C, D, ds, H, W, n, sides, lead=0):
    """One call of the hook into fresh poisoned volumes: ((volL, guardsL), (volR, guardsR)) on the host."""
    import torch
    fn = bind(mc)
    (bl, vl), (br, vr) = poisoned_volume(H, W, ds, lead), poisoned_volume(H, W, ds, lead)
    st = torch.cuda.current_stream().cuda_stream
    mc._lib.check(fn(f_dev[0].data_ptr(), f_dev[1].data_ptr(), vl.data_ptr(), vr.data_ptr(), C, D, ds, H, W, n, sides, st),
                  "mc_test_stereo_join_hwd")
    return fetch(bl, H, W, ds, lead), fetch(br, H, W, ds, lead)


def check_case(mc, oracle, recipe, C, H, W, D, ds, n=0, lead=0):
    """A case under sides 3, 1 and 2 (C > 64: the wide-C kernel computes both volumes from one product and takes 3 only), each into
    fresh poisoned volumes; with one side the other volume stays all poison, guards and padding included."""
    import torch
    want = want_of(oracle, recipe, C, H, W, D, n)
    f_dev = torch.from_numpy(feats(recipe, C, H, W).copy()).cuda()   # (a copy: the shared features are read-only)
    for sides in (3, 1, 2) if C <= 64 else (3,):
        what = "%s C=%d H=%d W=%d D=%d ds=%d n=%d lead=%d sides=%d" % (recipe, C, H, W, D, ds, n, lead, sides)
        got = run_join(mc, f_dev, C, D, ds, H, W, n, sides, lead)
        for k, name in enumerate(("volL", "volR")):
            vol, guards = got[k]
            if sides >> k & 1:
                check_volume(vol, want[k], D, guards, "%s %s" % (what, name))
            else:
                assert all_poison(vol) and all_poison(guards[0]) and all_poison(guards[1]), "%s: %s was written" % (what, name)


# ---- what keeps the value-range cases from being vacuous (tests/test_join_cases_host.py) --------------------------------------
TINY_NORMAL = np.float32(2.0 ** -126)


def classes(v):
    """shares of a float32 array's values that are NaN / infinite / subnormal / normal, and the counts of +0 and -0"""
    v = np.ascontiguousarray(v, np.float32).ravel()
    a = np.abs(v)
    zero = v == 0
    neg = np.signbit(v)
    n = float(v.size)
    return dict(nan=np.isnan(v).sum() / n, inf=np.isinf(v).sum() / n, subnormal=((a > 0) & (a < TINY_NORMAL)).sum() / n,
                normal=((a >= TINY_NORMAL) & np.isfinite(v)).sum() / n, pos_zero=int((zero & ~neg).sum()), neg_zero=int((zero & neg).sum()))


def join_boundaries():
    """The k-step counts (ks = ceil(C / 2)) at which stereo_join_hwd changes the kernel it launches, read from the launcher's own
    conditions in csrc/stereo_join.hip, and the largest one it takes (MC_JOIN_MAX_C): ([8, 16, 32, 56], 64) today."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mc-cnn_amd", "csrc")
    src = open(os.path.join(csrc, "stereo_join.hip")).read()
    body = src[src.index("int stereo_join_hwd("):]
    body = body[:body.index("\n}\n")]
    assert "const int ks = (C + 1) / 2;" in body
    launches = re.findall(r"ks <= (\d+)\) hipLaunchKernelGGL\(\(join_(?:owner|mfma)_kernel<(\d+)>\)", body)
    assert launches and all(a == b for a, b in launches), launches     # an instance takes what fills its k-steps
    edges = sorted(set(int(a) for a, _ in launches) | set(int(v) for v in re.findall(r"if \(ks <= (\d+)\) \{", body)))
    header = open(os.path.join(os.path.dirname(os.path.dirname(csrc)), "include", "mc_adcensus.h")).read()
    max_c = int(re.search(r"#define\s+MC_JOIN_MAX_C\s+(\d+)", header).group(1))
    return edges, (max_c + 1) // 2
