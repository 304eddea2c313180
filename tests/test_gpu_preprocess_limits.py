"""GPU: the dataset kernels of libmctrain.so (csrc/dataset.hip) at their limits -- map widths around the 64-lane ballot, the
256-thread row loop and MC_TRAIN_GT_MAX_W, row counts around the scan's 1024 chunks, mc_train_nnz_fill with fewer rows than
the count, and a workspace used twice -- against the numpy restatements of tests/preprocess_oracle.py and the reference's own
kernels (oracle/_ref)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import preprocess_oracle as po  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def pk():
    import torch
    from mc_cnn_amd import preprocess_kitti
    assert torch.cuda.is_available()
    return preprocess_kitti


def maps(rng, n, H, W):
    """PNG16-quantised maps with occlusions and non-visible pixels"""
    return np.stack([po.png16_map(rng, H, W, d_max=min(100.0, 2.0 * W)) for _ in range(n)]).astype(np.float32) / 256


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("W", [63, 64, 65, 127, 128, 129, 255, 256, 257, 8192])
def test_filters_at_width_limits(pk, ref, W):
    import torch
    rng = np.random.default_rng(W)
    n, H = 2, 3
    d = maps(rng, n, H, W)
    d[0, 1, W - 1] = 3.5                                   # the last column holds a value: visible, nothing right of it
    d[1, 2, :] = np.minimum(d[1, 2, :], 2.0)
    x = rng.integers(0, 256, (n, H, W)).astype(np.float32)
    x[rng.uniform(0, 1, (n, H, W)) < 0.03] = 255
    x[0, 0, W - 1] = 255
    got = torch.from_numpy(d).cuda()
    pk.filter_gt(got, torch.from_numpy(x).cuda())
    got = got.cpu().numpy()
    want = po.filter_gt(d, x)
    print("W %d: %d of %d pixels kept, %d removed" % (W, int((got > 0).sum()), got.size, int(((d > 0) & (got == 0)).sum())))
    assert same_bits(got, want), int((got != want).sum())
    assert (got > 0).any() and ((d > 0) & (got == 0)).any()
    for k in range(n):                                     # the reference's three kernels, one map at a time as the Lua script runs them
        y = torch.from_numpy(d[k].reshape(1, 1, H, W).copy()).cuda()
        ref.call("remove_nonvisible", y)
        ref.call("remove_occluded", y)
        ref.call("remove_white", torch.from_numpy(x[k].reshape(1, 1, H, W).copy()).cuda(), y)
        assert same_bits(got[k], y.cpu().numpy().reshape(H, W)), k


def ref_list(ref, disp, ids):
    import torch
    n, H, W = disp.shape
    buf = torch.zeros((max(1, n * H * W), 4), dtype=torch.float32)
    t = 0
    for k in range(n):
        t = int(ref.call("make_dataset2", torch.from_numpy(disp[k].reshape(1, 1, H, W).copy()), buf, int(ids[k]), t)[0])
    return buf[:t].numpy().copy()


@pytest.mark.parametrize("n,H", [(1, 1023), (1, 1024), (5, 205), (3, 683), (8, 625)])
def test_pixel_list_at_scan_chunk_edges(pk, ref, n, H):
    """n * H = 1023, 1024, 1025, 2049, 5000 rows for the scan's 1024 threads: one row per thread or none, exactly one, two for
    the first thread only, and uneven chunks.  W = 70: one full ballot and one of 6 lanes."""
    import torch
    W = 70
    rng = np.random.default_rng(n * H)
    d = maps(rng, n, H, W)
    d[:, ::7] = 0                                          # empty rows among the others
    d[-1, -1, :] = 9.25                                    # and a full last row
    ids = (np.arange(n) * 3 + 2).astype(np.int32)
    got = pk.pixel_list(torch.from_numpy(d).cuda(), ids).cpu().numpy()
    want = po.make_dataset2(d, ids)
    print("%d x %d rows: %d pixels listed" % (n, H, got.shape[0]))
    assert got.shape == want.shape and same_bits(got, want)
    assert same_bits(got, ref_list(ref, d, ids))
    assert (got[-W:, 2] == np.arange(W)).all() and (got[-W:, 1] == H - 1).all()


class Lister:
    """mc_train_nnz_count / _fill on one workspace, called directly"""

    def __init__(self, n, H):
        import torch
        from mc_cnn_amd import _train_lib as tl
        self.tl, self.lib = tl, tl.load()
        self.bytes = self.lib.mc_train_nnz_workspace_bytes(n, H)
        assert self.bytes > 0 and self.bytes % 8 == 0
        self.ws = torch.full((self.bytes // 8,), -1, dtype=torch.int64, device="cuda")
        self.count_d = torch.full((1,), -1, dtype=torch.int64, device="cuda")

    def count(self, d):
        n, H, W = d.shape
        assert self.lib.mc_train_nnz_workspace_bytes(n, H) <= self.bytes
        self.tl.check(self.lib.mc_train_nnz_count(d.data_ptr(), n, H, W, self.count_d.data_ptr(), self.ws.data_ptr(), self.bytes, None),
                      "mc_train_nnz_count")
        return int(self.count_d.item())

    def fill(self, d, ids, out, n_nnz):
        n, H, W = d.shape
        assert 0 <= n_nnz <= out.shape[0]
        self.tl.check(self.lib.mc_train_nnz_fill(d.data_ptr(), ids.data_ptr(), n, H, W, out.data_ptr(), n_nnz, self.ws.data_ptr(),
                                                 self.bytes, None), "mc_train_nnz_fill")
        return out.cpu().numpy()


def test_fill_stops_at_n_nnz():
    """Rows past n_nnz are not written: into a NaN-filled buffer longer than the whole list, for n_nnz = count - 1, count - 65,
    1 and 0 the first n_nnz rows are the full list's and every later row is still NaN; with n_nnz above the count exactly
    count rows are written."""
    import torch
    rng = np.random.default_rng(5)
    n, H, W = 3, 37, 200
    d = maps(rng, n, H, W)
    ids = np.array([4, 9, 1], np.int32)
    full = po.make_dataset2(d, ids)
    dd, idd = torch.from_numpy(d).cuda(), torch.from_numpy(ids).cuda()
    ls = Lister(n, H)
    count = ls.count(dd)
    assert count == full.shape[0] and count > 1000
    for n_nnz in (count - 1, count - 65, 1, 0, count, count + 69):
        out = torch.full((count + 70, 4), NAN, dtype=torch.float32, device="cuda")
        got = ls.fill(dd, idd, out, n_nnz)
        k = min(n_nnz, count)
        written = int((~np.isnan(got)).any(1).sum())
        print("n_nnz %d of %d: %d rows written" % (n_nnz, count, written))
        assert same_bits(got[:k], full[:k]), n_nnz
        assert np.isnan(got[k:]).all(), (n_nnz, np.nonzero(~np.isnan(got[k:]).all(1))[0][:5] + k)


def test_a_second_count_leaves_no_stale_offsets():
    """One workspace, counted for a large set of maps and then for smaller, other ones: the second list is the second set's."""
    import torch
    rng = np.random.default_rng(6)
    big = rng.uniform(0.51, 200, (4, 300, 130)).astype(np.float32)          # every pixel listed: large counts and offsets
    small = maps(rng, 3, 101, 70)
    small[1] = 0                                                             # a map without pixels in the middle
    ls = Lister(4, 300)
    assert ls.count(torch.from_numpy(big).cuda()) == big.size
    for d, ids in ((small, np.array([7, 8, 9], np.int32)), (big[:2, :50], np.array([1, 2], np.int32)), (small[:1, :1], np.array([3], np.int32))):
        d = np.ascontiguousarray(d)
        want = po.make_dataset2(d, ids)
        dd = torch.from_numpy(d).cuda()
        count = ls.count(dd)
        assert count == want.shape[0]
        out = torch.full((count + 1, 4), NAN, dtype=torch.float32, device="cuda")
        got = ls.fill(dd, torch.from_numpy(ids).cuda(), out, count)
        assert same_bits(got[:count], want) and np.isnan(got[count:]).all()
