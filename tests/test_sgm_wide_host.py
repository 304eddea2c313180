"""CPU: the ground the disparity ranges 513..1024 stand on.  (1) tests/sgm2_restatement.py -- the yardstick of tests/test_gpu_sgm_wide.py, where
the C oracle's sgm2 stops -- equals that oracle bit for bit wherever both run.  (2) What the library says about the range without a GPU:
the scratch size mc_sgm2 asks for is what it always was up to D = 512 and larger above, the limit is 1024 and named in both refusals,
and mc_predict's workspace grows with it."""
import ctypes as C

import numpy as np
import pytest

from sgm2_restatement import PRM, quantised_case, sgm2 as restated_sgm2
from util import diff_report, same_bits

torch = pytest.importorskip("torch")

EINVAL = -22


def all_three_classes_occur(x0, x1, tau):
    """at d = 0 of the first direction: both differences below tau_so, both above, and one of each"""
    a, b = np.abs(np.diff(x0, axis=1)), np.abs(np.diff(x1, axis=1))
    lo, hi = (a < tau) & (b < tau), (a > tau) & (b > tau)
    return lo.any() and hi.any() and (~lo & ~hi).any()


@pytest.mark.parametrize("direction", [-1, 1])
@pytest.mark.parametrize("H,W", [(5, 9), (9, 5)])
@pytest.mark.parametrize("D", [1, 7, 64, 300, 512])
def test_restatement_is_the_oracles_sgm2(oracle, H, W, D, direction):
    x0, x1, vol, tau = quantised_case(H, W, D, direction, seed=5 * D + H)
    assert all_three_classes_occur(x0, x1, tau)
    prm = PRM[:2] + (tau,) + PRM[3:]
    want = oracle.sgm2(x0, x1, vol, *prm, direction)
    assert np.isnan(want).any() == (D > 1) and np.isfinite(want[:, :, 0]).all()
    got = restated_sgm2(torch.from_numpy(x0), torch.from_numpy(x1), torch.from_numpy(vol), torch.zeros((H, W, D)), *prm, direction).numpy()
    assert same_bits(got, want), diff_report(got, want, "restated sgm2 %dx%dx%d direction %d" % (H, W, D, direction))


def test_restatement_adds_to_its_output(oracle):
    H, W, D = 6, 11, 20
    x0, x1, vol, tau = quantised_case(H, W, D, -1, seed=9)
    prm = PRM[:2] + (tau,) + PRM[3:]
    base = np.random.default_rng(0).random((H, W, D), dtype=np.float32)
    want = oracle.sgm2(x0, x1, vol, *prm, -1, out=base.copy())
    got = restated_sgm2(torch.from_numpy(x0), torch.from_numpy(x1), torch.from_numpy(vol), torch.from_numpy(base.copy()), *prm, -1).numpy()
    assert same_bits(got, want), diff_report(got, want, "restated sgm2 into a filled output")


# mc_sgm2_tmp_bytes(H, W, D <= 512) as the build of the commit before the range grew returned it
TMP_BYTES = {(8, 8): 67584, (370, 1226): 8521984}


def test_sgm2_scratch_size_follows_d_only_above_512(mc):
    lib = mc._lib.lib
    for (H, W), want in TMP_BYTES.items():
        assert lib.mc_sgm2_tmp_bytes(H, W, 1) == lib.mc_sgm2_tmp_bytes(H, W, 512) == want
        assert lib.mc_sgm2_tmp_bytes(H, W, 228) == want
        wide = lib.mc_sgm2_tmp_bytes(H, W, 513)
        assert wide > want and wide == lib.mc_sgm2_tmp_bytes(H, W, 1024)
        assert wide - want <= 8 * H * 1024 + 256          # the eight window planes' rows, 2 x 512 bytes longer each


def test_the_limit_is_1024_and_both_refusals_name_it(mc):
    lib = mc._lib.lib
    assert lib.mc_sgm2(1, 1, 1, 2, 1, 1 << 30, 8, 8, 1025, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1, None) == EINVAL
    assert lib.mc_last_error() == b"mc_sgm2: D=1025 exceeds 1024"
    p = mc.make_params("kitti_fast")
    assert lib.mc_predict(C.byref(p), 1, 1, 1, 1, 64, None, None, 1025, 8, 8, 256, 1 << 40, None, None, None, None, 1, None) == EINVAL
    assert lib.mc_last_error() == b"mc_predict: D=1025 exceeds 1024"


def test_d_600_is_refused_for_its_scratch_not_for_its_range(mc):
    lib = mc._lib.lib
    need = lib.mc_sgm2_tmp_bytes(8, 8, 600)
    for tmp_bytes in (0, TMP_BYTES[(8, 8)], need - 1):      # (the middle one: what D <= 512 needs is not enough)
        assert lib.mc_sgm2(1, 1, 1, 2, 1, tmp_bytes, 8, 8, 600, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1, None) == EINVAL
        msg = lib.mc_last_error()
        assert msg == b"mc_sgm2: tmp holds %d bytes, needs %d" % (tmp_bytes, need) and b"exceeds" not in msg


def test_predict_workspace_grows_with_the_range(mc):
    lib = mc._lib.lib
    for preset in ("kitti_fast", "mb_slow"):
        p = mc.make_params(preset)
        for fn in (lib.mc_predict_workspace_bytes, lib.mc_predict_workspace_bytes_full):
            sizes = [fn(C.byref(p), 64, D, 40, 90) for D in (512, 513, 1024)]
            assert sizes[0] > 0 and sizes[0] <= sizes[1] <= sizes[2], (preset, sizes)
        assert lib.mc_predict_workspace_bytes(C.byref(p), 64, 1025, 40, 90) > 0    # a size, not a verdict: mc_predict itself refuses D = 1025
