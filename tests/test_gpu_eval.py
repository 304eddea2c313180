"""GPU: mc_eval_error (libmceval.so, include/mc_eval.h) against `train.error_rate` and numpy's NaN count.  The three counts are
integers, so everything here is equality."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(a, ld, fill):
    """(H, W) -> (H, ld) with `fill` in the padding: a kernel that reads past a row's W counts it."""
    out = np.full((a.shape[0], ld), fill, np.float32)
    out[:, :a.shape[1]] = a
    return out


def want_counts(pred, actual, err_at):
    """The reference's arithmetic (main.lua:1224-1236) as train.error_rate states it, and numpy's NaN count."""
    from mc_cnn_amd.train import error_rate
    mask = actual != 0
    with np.errstate(invalid="ignore"):
        bad = (np.abs(actual - pred) > err_at) & mask
        want = [int(mask.sum()), int(bad.sum()), int(np.isnan(pred).sum())]
        if want[0]:
            assert float(want[1]) / float(want[0]) == error_rate(pred, actual, err_at)
    return want


def device_counts(pred, actual, err_at, pred_ld=None, actual_ld=None, counts=None):
    import torch
    from mc_cnn_amd.evalset import eval_error
    H, W = pred.shape
    pred_ld, actual_ld = pred_ld or W, actual_ld or W
    p, a = dev(strided(pred, pred_ld, np.nan)), dev(strided(actual, actual_ld, 1e9))
    if counts is None:
        counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    eval_error(p, pred_ld, a, actual_ld, H, W, err_at, counts)
    torch.cuda.synchronize()
    return counts.cpu().numpy().tolist()


def random_maps(H, W, seed, err_at):
    """A third of the ground truth unknown (0), differences spread around err_at, a few NaNs in the prediction."""
    rng = np.random.default_rng(seed)
    actual = rng.uniform(1, 200, (H, W)).astype(np.float32)
    actual[rng.uniform(size=(H, W)) < 0.33] = 0
    pred = (actual + rng.normal(0, err_at, (H, W))).astype(np.float32)
    pred[actual == 0] = rng.uniform(0, 200, int((actual == 0).sum())).astype(np.float32)
    pred[rng.uniform(size=(H, W)) < 0.01] = np.nan
    return pred, actual


# the issue's shapes, then three of this file's own: every row misaligned against a 16-byte boundary in the same way (heads of 1..3
# dwords in front of more than one workgroup's worth of 16-byte loads), and a base pointer that is itself off the boundary
SHAPES = [(1, 1, 0, 0), (1, 63, 0, 0), (1, 64, 0, 0), (1, 65, 0, 0), (3, 257, 0, 0), (5, 1026, 0, 0), (48, 160, 163, 170),
          (350, 1226, 0, 1242), (3, 9000, 9001, 9005), (2, 4100, 4101, 4101), (7, 4097, 4099, 4103)]


@pytest.mark.parametrize("H, W, pred_ld, actual_ld", SHAPES)
def test_counts_equal_numpys(H, W, pred_ld, actual_ld):
    for err_at in (3, 1):
        pred, actual = random_maps(H, W, H * 10007 + W + err_at, err_at)
        want = want_counts(pred, actual, err_at)
        got = device_counts(pred, actual, err_at, pred_ld, actual_ld)
        print(H, W, pred_ld, actual_ld, err_at, got, want)
        assert got == want
    if H * W > 1000:
        assert want[0] > 0 and 0 < want[1] < want[0] and want[2] > 0


def test_a_base_pointer_off_the_16_byte_boundary():
    import torch
    from mc_cnn_amd.evalset import eval_error
    H, W = 6, 301
    pred, actual = random_maps(H, W, 77, 3)
    for off_p, off_a in ((1, 1), (3, 3), (1, 2), (0, 3)):
        p = torch.full((H * W + 4,), float("nan"), device="cuda")
        a = torch.full((H * W + 4,), 1e9, device="cuda")
        p[off_p:off_p + H * W] = dev(pred).ravel()
        a[off_a:off_a + H * W] = dev(actual).ravel()
        counts = torch.zeros(3, dtype=torch.int32, device="cuda")
        eval_error(p[off_p:], W, a[off_a:], W, H, W, 3, counts)
        assert counts.cpu().numpy().tolist() == want_counts(pred, actual, 3), (off_p, off_a)


def test_value_cases():
    f = np.float32
    one_ulp_past = np.nextafter(f(7), f(-np.inf))            # 10 - it = 3 + 2^-21, representable: just over err_at
    rows = [  # (pred, actual) -> valid, bad, nan
        (f(7), f(10)),                # |diff| exactly err_at: not bad
        (one_ulp_past, f(10)),        # one ulp above: bad
        (f(13), f(10)),               # exactly err_at the other way
        (f(50), f(-0.0)),             # -0.0 is zero: not valid
        (f(50), f(1e-40)),            # a denormal is non-zero: valid and bad
        (f(0), f(1e-40)),             # ... valid and not bad
        (f(np.nan), f(10)),           # NaN difference is not bad; counted as NaN
        (f(np.nan), f(0)),            # NaN is counted where the ground truth is unknown too
        (f(np.inf), f(10)), (f(-np.inf), f(10)),    # bad
        (f(np.inf), f(np.inf)),       # inf - inf = NaN: not bad, and the prediction is no NaN
        (f(5), f(np.nan)),            # NaN != 0: valid; NaN difference: not bad
    ]
    pred = np.array([[p for p, _ in rows]], f)
    actual = np.array([[a for _, a in rows]], f)
    want = want_counts(pred, actual, 3)
    assert want == [10, 4, 2]         # what numpy gives on float32, spelled out
    assert device_counts(pred, actual, 3) == want
    # each case alone as well, so that no two errors cancel
    for k in range(len(rows)):
        assert device_counts(pred[:, k:k + 1], actual[:, k:k + 1], 3) == want_counts(pred[:, k:k + 1], actual[:, k:k + 1], 3), k


def test_all_zero_ground_truth_counts_no_valid_pixel():
    pred, _ = random_maps(9, 130, 5, 3)
    actual = np.zeros_like(pred)
    got = device_counts(pred, actual, 3, 133, 131)
    assert got == [0, 0, int(np.isnan(pred).sum())] and got[2] > 0


def test_two_calls_accumulate_into_counts_that_are_not_zero():
    pred1, actual1 = random_maps(17, 200, 1, 3)
    pred2, actual2 = random_maps(5, 1026, 2, 3)
    counts = dev(np.array([5, 6, 7], np.int32))
    device_counts(pred1, actual1, 3, counts=counts)
    got = device_counts(pred2, actual2, 3, 1030, 1027, counts=counts)
    w1, w2 = want_counts(pred1, actual1, 3), want_counts(pred2, actual2, 3)
    assert got == [5 + w1[0] + w2[0], 6 + w1[1] + w2[1], 7 + w1[2] + w2[2]]


def test_two_streams_into_two_rows_at_once():
    import torch
    from mc_cnn_amd.evalset import eval_error
    maps = [random_maps(350, 1226, 11, 3), random_maps(350, 1226, 12, 3)]
    tensors = [(dev(p), dev(strided(a, 1242, 1e9))) for p, a in maps]
    counts = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    for _ in range(3):      # three rounds each, interleaved: the rows take three times the counts
        for i, s in enumerate(streams):
            with torch.cuda.stream(s):
                eval_error(tensors[i][0], 1226, tensors[i][1], 1242, 350, 1226, 3, counts[i])
    torch.cuda.synchronize()
    got = counts.cpu().numpy().tolist()
    assert got == [[3 * v for v in want_counts(p, a, 3)] for p, a in maps]
