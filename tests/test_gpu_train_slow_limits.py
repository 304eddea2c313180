"""GPU: libmctrainslow.so (include/mc_train_slow.h) and libmctrainmbslow.so (include/mc_train_mb_slow.h) at their edges, as
tests/test_gpu_train_limits.py has libmctrain.so: batch sizes at the FC kernels' 16-row tile edges and at MAX_PAIRS, the
order in which the convolutions' gradient is summed, `run` against the chain sample -> step_batch with the sampler at the
image borders and the offset at its last legal value, and one refusal per MC_REQUIRE.

Every workspace here is a slice of a larger tensor (`Guarded`): 16-byte aligned, exactly `*_workspace_bytes(n)` bytes, filled
with NaN, with 4096 sentinel words before and after it.  After every call the sentinels must be bit-identical; after a
completed step every area the step computes (`areas`, the libraries' carve restated) must be finite, and what no kernel may
write -- the 64-float alignment pads, and the sampled patches' area on the step_batch path -- must still be NaN.

(b), the bit-exact pair-order sum, covers libmctrainslow.so only: its slab holds one row per pair, which a single-pair step
supplies.  libmctrainmbslow.so sums 3 N per-PATCH rows (3 * pair + p), which single-pair steps cannot supply one by one; its
summation is left to (a), where a wrong row or a dropped one misses the float64 gradient.

Bounds are the existing tests' (tests/test_gpu_train_slow.py, tests/test_gpu_train_mb_slow.py): loss 1e-5, each of the 18
momenta tensors 1e-4 of its largest magnitude, parameters atol 1e-5."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_mb_slow_oracle as mso  # noqa: E402
import train_slow_oracle as so  # noqa: E402
import test_gpu_train_mb_slow as base_mb_slow  # noqa: E402
import test_gpu_train_slow as base_slow  # noqa: E402
from test_gpu_train_mb import small_set  # noqa: E402
from train_fixtures import bits, dev, same_bits, small_images  # noqa: E402

pytestmark = pytest.mark.gpu

LR, MOM = 0.003, 0.9
NAN = float("nan")
MC_EINVAL = -22
GUARD = 4096                   # sentinel words on either side of a workspace
SENTINEL = 0x4B1D5EED          # their bit pattern (a finite float, 1.03e7: a kernel that read it would not turn it into NaN)
LOSS_SENTINEL = -123.25


class Guarded:
    """nbytes of NaN at a 16-byte aligned address inside a larger tensor, GUARD sentinel words on either side."""

    def __init__(self, nbytes):
        import torch
        assert nbytes > 0 and nbytes % 4 == 0
        self.n = nbytes // 4
        self.buf = torch.empty(2 * GUARD + self.n, dtype=torch.int32, device="cuda")
        self.buf.fill_(SENTINEL)
        self.ws = self.buf[GUARD:GUARD + self.n].view(torch.float32)
        self.ws.fill_(NAN)
        assert self.ws.data_ptr() % 16 == 0 and self.ws.numel() * 4 == nbytes
        assert self.ws.data_ptr() == self.buf.data_ptr() + 4 * GUARD

    def poison(self):
        self.ws.fill_(NAN)

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


# ---- the two libraries behind one face ----------------------------------------------------------------------------------------
class SlowLib:
    """libmctrainslow.so: KITTI's accurate net, 9 x 9 patches, one slab row per pair, images (n_img, H, W)"""
    name, PS, L2, rows_per_pair = "slow", 9, 4, 1
    oracle = so
    sturdy_pairs = staticmethod(base_slow.sturdy_pairs)
    RUN_SIG = ["x0", "x1", "n_img", "H", "W", "nnz", "n_nnz", "perm", "n_perm", "t0", "n_steps", "n_pairs", "prm", "params", "moms", "lr",
               "mom", "losses", "ws", "ws_bytes", "stream"]

    def __init__(self):
        from mc_cnn_amd import train_slow
        self.mod, self.tl = train_slow, train_slow.tsl

    def opt(self, *flags):
        return self.mod.parse(["kitti", "slow", "-a", "train_tr"] + list(flags))[2]

    def trainer(self, store, nnz, perm, nets, n_pairs):
        import torch
        return self.mod.Trainer(store[0], store[1], nnz, perm, nets[0], nets[1], n_pairs, torch.device("cuda"))

    def store_values(self, t):
        return dict(x0=t.x0.data_ptr(), x1=t.x1.data_ptr(), n_img=t.n_img, H=t.H, W=t.W)

    def sample(self, t, rows, src, prm):
        from mc_cnn_amd import train
        return train.sample(t.x0, t.x1, t.nnz, rows, prm)         # libmctrain.so's sampler, which libmctrainslow.so's kernel restates


class MbSlowLib:
    """libmctrainmbslow.so: Middlebury's accurate net, 11 x 11 patches, three slab rows per pair, the ragged plane store"""
    name, PS, L2, rows_per_pair = "mb_slow", 11, 3, 3
    oracle = mso
    sturdy_pairs = staticmethod(base_mb_slow.sturdy_pairs)
    RUN_SIG = ["planes", "table", "n_planes", "nnz", "n_nnz", "perm", "n_perm", "t0", "n_steps", "n_pairs", "src", "prm", "params", "moms",
               "lr", "mom", "losses", "ws", "ws_bytes", "stream"]

    def __init__(self):
        from mc_cnn_amd import train_mb_slow
        self.mod, self.tl = train_mb_slow, train_mb_slow.tmsl

    def opt(self, *flags):
        return self.mod.parse(["mb", "slow", "-a", "train_tr"] + list(flags))[2]

    def trainer(self, store, nnz, perm, nets, n_pairs):
        import torch
        return self.mod.Trainer(store[0], store[1], nnz, perm, nets[0], nets[1], n_pairs, torch.device("cuda"))

    def store_values(self, t):
        return dict(planes=t.planes.data_ptr(), table=t.table.data_ptr(), n_planes=t.table.shape[0])

    def sample(self, t, rows, src, prm):
        from mc_cnn_amd import train_mb
        return train_mb.sample(t.planes, t.table, t.nnz, rows, src, prm)   # libmctrainmb.so's sampler


STEP_SIG = ["patches", "n_pairs", "params", "moms", "lr", "mom", "loss", "ws", "ws_bytes", "stream"]
LIBS = {"slow": SlowLib, "mb_slow": MbSlowLib}
_libs, _wide, _reference = {}, {}, {}


def lib_of(name):
    import torch
    assert torch.cuda.is_available()
    if name not in _libs:
        _libs[name] = LIBS[name]()
        L = _libs[name]
        L.lib = L.tl.load()
        L.MAX, L.NCONV, L.NFC, L.NPARAMS = L.tl.MAX_PAIRS, L.tl.NCONV, L.tl.NFC, L.tl.NPARAMS
        L.fn = lambda what, L=L: getattr(L.lib, "%s_%s" % (L.tl.PREFIX, what))
        assert L.oracle.NPARAMS == L.NPARAMS and L.oracle.WS == L.PS and (L.MAX, L.PS) in ((1024, 9), (256, 11))
    return _libs[name]


def wide_of(L):
    if L.name not in _wide:
        _wide[L.name] = L.oracle.wide_nets(1)
    return _wide[L.name]


def reference(L, n_pairs):
    """Sturdy pairs and, from the wide nets, their float64 loss and gradient: computed once per (library, batch size) and
    left unchanged.  The float64 step with lr 1 and no momentum leaves momenta = -gradient."""
    key = (L.name, n_pairs)
    if key not in _reference:
        conv, fc = wide_of(L)
        t_start = time.perf_counter()
        patches = L.sturdy_pairs(conv, fc, 7000 + n_pairs, n_pairs)
        assert patches.shape[0] == n_pairs
        _, wv, wl = L.oracle.sgd_steps(conv, fc, [patches], 1.0, 0.0)
        print("%s, %d pairs: float64 selection and gradient took %.1f s" % (L.name, n_pairs, time.perf_counter() - t_start))
        grad = -wv
        grad.setflags(write=False)
        _reference[key] = (patches, grad, wl[0])
    return _reference[key]


def areas(L, n_pairs):
    """The libraries' workspace (carve in train_slow_fc.h) restated: (name, first float, floats) of every
    area, each rounded up to 64 floats, and the total."""
    R, NIN, NH = 2 * n_pairs, 224, 384
    sizes = [("xs", n_pairs * 3 * L.PS * L.PS), ("a0", R * NIN)] + [("a%d" % l, R * NH) for l in range(1, L.L2 + 1)] + \
        [("g0", R * NH), ("g1", R * NH), ("dfeat", R * NIN), ("gfc", L.NFC), ("slab", L.rows_per_pair * n_pairs * L.NCONV)]
    out, o = [], 0
    for name, n in sizes:
        out.append((name, o, n))
        o += -(-n // 64) * 64
    return out, o


def guarded_ws(L, n_pairs):
    need = L.fn("workspace_bytes")(n_pairs)
    assert need == areas(L, n_pairs)[1] * 4, "the workspace is not the sum of the documented areas"
    return Guarded(need)


def check_workspace(L, g, n_pairs, sampled, what):
    """After a completed step: sentinels intact, every computed area finite, pads (and xs where the patches were given) NaN."""
    import torch
    assert g.guards_intact(), "%s: a kernel wrote outside its workspace" % what
    layout, total = areas(L, n_pairs)
    assert total == g.n
    end = 0
    for name, o, n in layout:
        assert bool(torch.isnan(g.ws[end:o]).all()), "%s: the pad before %s was written" % (what, name)
        if name == "xs" and not sampled:
            assert bool(torch.isnan(g.ws[o:o + n]).all()), "%s: xs written though the patches were given" % what
        else:
            assert bool(torch.isfinite(g.ws[o:o + n]).all()), "%s: the step left part of %s unwritten" % (what, name)
        end = o + n
    assert bool(torch.isnan(g.ws[end:]).all()), "%s: the pad at the end was written" % what


# ---- (a) batch sizes at the 16-row tile edges, and the largest -------------------------------------------------------------
# R = 2 n rows: 4; 14 (one pair short of a tile); 16 (exactly one); 18 (one pair past); 30; 32 (exactly two).  The weight
# gradient takes rows four at a time: 14, 18 and 30 leave two.
EDGES = [("slow", n) for n in (2, 7, 8, 9, 15, 16)] + [("mb_slow", n) for n in (2, 7, 8, 9, 15, 16)] + [("slow", 1024), ("mb_slow", 256)]


@pytest.mark.parametrize("name,n_pairs", EDGES, ids=["%s-%d" % e for e in EDGES])
def test_tile_edges_and_the_largest_batch_match_float64_autograd(name, n_pairs):
    """One step from wide weights on sturdy pairs, on a poisoned and guarded workspace, against float64 autograd.
    Measured on an MI355X, worst of the cases (each case prints its own): libmctrainslow.so loss difference 2.4e-7 (9 pairs;
    2.3e-7 at 1024), worst tensor 7.8e-6 of its largest magnitude (7 pairs; 1.7e-6 at 1024); libmctrainmbslow.so 6.4e-7
    (256 pairs) and 2.0e-6 (8 pairs; 1.3e-6 at 256).  The bounds of 64 pairs hold at MAX_PAIRS with a factor of 15 to
    spare, so none had to be derived anew."""
    import torch
    L = lib_of(name)
    assert n_pairs <= L.MAX and (n_pairs < 64 or n_pairs == L.MAX)
    patches, grad, want_loss = reference(L, n_pairs)
    p0 = L.oracle.flat(*wide_of(L))
    params = dev(p0)
    moms = torch.zeros_like(params)
    g = guarded_ws(L, n_pairs)
    loss = float(L.mod.step_batch(dev(patches), params, moms, LR, MOM, g.ws).cpu())
    what = "%s, %d pairs" % (name, n_pairs)
    check_workspace(L, g, n_pairs, False, what)
    want_v = -LR * grad                                   # float64: v = 0.9 * 0 - lr * g, w += v
    want_p = p0.astype(np.float64) + want_v
    got_v, got_p = moms.cpu().numpy(), params.cpu().numpy()
    print("%s: loss %.7f, float64 %.7f, difference %.2e" % (what, loss, want_loss, abs(loss - want_loss)))
    assert np.isfinite(got_v).all() and np.isfinite(got_p).all() and np.abs(want_v).max() > 1e-6
    assert abs(loss - want_loss) <= 1e-5
    errs = L.oracle.check_per_tensor(got_v, want_v, 1e-4, what)
    print("%s: worst tensor %.2e, worst parameter %.2e" % (what, max(errs.values()), np.abs(got_p - want_p).max()))
    np.testing.assert_allclose(got_p, want_p, rtol=0, atol=1e-5)


# ---- (b) the convolutions' gradient is summed in pair order -------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1024])
def test_convolution_gradients_are_summed_in_pair_order(N):
    """libmctrainslow.so.  With lr = 1, mom = 0 and zero momenta a step leaves moms = -g.  Each pair alone gives g_i (its
    head divides by R = 2); in the N-pair step the head divides by 2 N, exact for a power of two, and the FC data
    gradients and the tower are linear in that factor row by row: slab row i is g_i / N, and the update must leave in the
    first NCONV momenta the float32 sum of g_i / N over i = 0, 1, ... in that order, bit for bit.  The FC part of the same
    step is summed inside MFMA instructions and is held to float64 per tensor instead."""
    import torch
    assert N & (N - 1) == 0
    L = lib_of("slow")
    NC, NP = L.NCONV, L.NPARAMS
    patches, grad, want_loss = reference(L, N)
    bd = dev(patches)
    fresh = dev(L.oracle.flat(*wide_of(L)))
    G = torch.empty((N, NC), dtype=torch.float32, device="cuda")
    params, moms, g1 = fresh.clone(), torch.zeros(NP, device="cuda"), guarded_ws(L, 1)
    t_start = time.perf_counter()
    for i in range(N):
        params.copy_(fresh)
        moms.zero_()
        L.mod.step_batch(bd[i:i + 1], params, moms, 1.0, 0.0, g1.ws)
        torch.neg(moms[:NC], out=G[i])
    torch.cuda.synchronize()
    t_single = time.perf_counter() - t_start
    assert torch.isfinite(G).all()
    check_workspace(L, g1, 1, False, "single pairs")
    params.copy_(fresh)
    moms.zero_()
    g = guarded_ws(L, N)
    loss = float(L.mod.step_batch(bd, params, moms, 1.0, 0.0, g.ws).cpu())
    check_workspace(L, g, N, False, "%d pairs" % N)
    inv = 1.0 / N
    acc = torch.zeros(NC, device="cuda")
    tiny = torch.zeros(NC, dtype=torch.bool, device="cuda")
    for i in range(N):
        gi = G[i] * inv                                   # exact: a power of two
        tiny |= (gi != 0) & (gi.abs() < 2.0 ** -100)
        acc = acc + gi                                    # one float32 add per pair, in pair order
    want = torch.zeros(NC, device="cuda") - acc           # the kernel's 0 * 0 - 1 * g
    got = moms[:NC]
    share = float(tiny.float().mean())
    differ = (bits(got) != bits(want)) & ~tiny
    n_differ = int(differ.sum())
    err = float((got - want).abs().max())
    print("N %d: %d of %d convolution elements differ from the ordered float32 sum (max |difference| %.3e); %.2e of the elements "
          "have a term below 2^-100; %d single-pair steps took %.1f s" % (N, n_differ, NC, err, share, N, t_single))
    assert share < 1e-4
    assert float((got - want)[tiny].abs().max()) <= 1e-12 if bool(tiny.any()) else True
    assert n_differ == 0
    assert same_bits(params, fresh + moms)
    assert float(got.abs().max()) > 1e-4                  # a gradient was there to be summed
    # the same sum in any other order is a different float32 number somewhere: the comparison can tell orders apart
    rev = torch.zeros(NC, device="cuda")
    for i in reversed(range(N)):
        rev = rev + G[i] * inv
    assert int((bits(rev) != bits(acc)).sum()) > 0
    # the FC part (and, more loosely than above, the convolutions) and the loss against float64
    print("N %d: loss %.7f, float64 %.7f, difference %.2e" % (N, loss, want_loss, abs(loss - want_loss)))
    assert abs(loss - want_loss) <= 1e-5
    errs = L.oracle.check_per_tensor(moms.cpu().numpy(), -grad, 1e-4, "N %d" % N)
    print("N %d: worst tensor %.2e, worst FC tensor %.2e" % (N, max(errs.values()), max(v for k, v in errs.items() if k.startswith("f"))))


# ---- (c) run equals the chain sample -> step_batch where the sampler is at its limits -------------------------------------------
def border_rows(img, H, W):
    """nnz rows of image `img` (1-based) on its four corners, its four borders and one inside, each with a small disparity and
    with one that puts both right patches wholly outside the image."""
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1), (H // 2, W // 2)]
    return [(img, y, x, d) for y, x in pos for d in (1.0, x + 60.5)]


def slow_case():
    x0, x1, _ = small_images(3, n_img=2, H=14, W=23)
    nnz = np.array(border_rows(1, 14, 23) + border_rows(2, 14, 23), np.float32)
    return (x0, x1), nnz, None


def mb_slow_case():
    """small_set's ragged store: planes of 40 x 90, 33 x 57 and 52 x 41.  Left planes are even ids, right ones odd; pair k of
    an image takes the right view of plane pair k + 1 (another exposure or light) where k is odd, and image 3's pairs reach
    the table's last plane."""
    from mc_cnn_amd import train_mb
    planes, table, index, _ = small_set(train_mb)
    nnz, src = [], []
    for img in range(1, 4):
        first, n_light, n_exp = (int(v) for v in index[img - 1])
        n_views = n_light * n_exp
        H, W = int(table["H"][first]), int(table["W"][first])
        for k, row in enumerate(border_rows(img, H, W)):
            left = k % n_views
            right = (left + (k & 1)) % n_views if img < 3 else n_views - 1 - (k % 2)
            nnz.append(row)
            src.append((first + 2 * left, first + 2 * right + 1))
    src = np.array(src, np.int32)
    assert (src[:, 1] == len(table) - 1).any() and (src[:, 1] != src[:, 0] + 1).sum() >= 10
    assert len(set((int(table["H"][k]), int(table["W"][k])) for k in src.ravel())) == 3
    return (planes, table), np.array(nnz, np.float32), src


def raw_run(L, t, t0, n_steps, src, prm, losses, g):
    from mc_cnn_amd.train_common import _stream
    vals = dict(L.store_values(t), nnz=t.nnz.data_ptr(), n_nnz=t.nnz.shape[0], perm=t.perm.data_ptr(), n_perm=t.perm.shape[0], t0=t0,
                n_steps=n_steps, n_pairs=t.n_pairs, src=None if src is None else src.data_ptr(), prm=prm.data_ptr(),
                params=t.params.data_ptr(), moms=t.moms.data_ptr(), lr=LR, mom=MOM, losses=losses.data_ptr(), ws=g.ws.data_ptr(),
                ws_bytes=g.n * 4, stream=_stream())
    return L.fn("run")(*[vals[k] for k in L.RUN_SIG])


@pytest.mark.parametrize("n_pairs", [1, 8])
@pytest.mark.parametrize("name", ["slow", "mb_slow"])
def test_run_equals_the_chain_at_the_samplers_limits_and_the_last_offset(name, n_pairs):
    import torch
    L = lib_of(name)
    store, nnz, src_of_row = slow_case() if name == "slow" else mb_slow_case()
    rng = np.random.default_rng(50 + n_pairs)
    n_steps, t0 = 4, 3
    n_perm = t0 + n_steps * n_pairs                       # t0 is the last legal offset
    far = nnz[:, 3] > nnz[:, 2] + 20                      # rows whose right patches leave the image, and the others, in turn
    perm = np.stack([rng.permutation(np.nonzero(far)[0]), rng.permutation(np.nonzero(~far)[0])], 1).ravel().astype(np.int32)[:n_perm]
    used = nnz[perm[t0:]]
    assert perm.size == n_perm and far[perm[t0:]].sum() == n_steps * n_pairs // 2 and np.unique(perm).size == n_perm
    prm = dev(L.mod.draw_params(rng, L.opt("-hflip", "1", "-vflip", "1", "-trans", "1"), n_steps, n_pairs))
    src = None if src_of_row is None else dev(src_of_row[perm[t0:]].reshape(n_steps, n_pairs, 2))
    nets = wide_of(L)
    t = L.trainer(store, nnz, perm, nets, n_pairs)
    g = guarded_ws(L, n_pairs)
    losses = torch.full((n_steps + 1,), LOSS_SENTINEL, dtype=torch.float32, device="cuda")
    fresh = t.params.clone()

    # n_steps = 0 changes nothing and launches nothing
    assert raw_run(L, t, t0, 0, src, prm, losses, g) == 0
    torch.cuda.synchronize()
    assert same_bits(t.params, fresh) and not t.moms.any() and bool((losses == LOSS_SENTINEL).all())
    assert bool(torch.isnan(g.ws).all()) and g.guards_intact()

    # one row past the last legal offset: refused with the message's three numbers, nothing touched
    assert raw_run(L, t, t0 + 1, n_steps, src, prm, losses, g) == MC_EINVAL
    msg = L.fn("last_error")().decode()
    assert "permutation" in msg and "[%d, %d)" % (t0 + 1, n_perm + 1) in msg and "%d rows" % n_perm in msg, msg
    torch.cuda.synchronize()
    assert same_bits(t.params, fresh) and not t.moms.any() and bool((losses == LOSS_SENTINEL).all())
    assert bool(torch.isnan(g.ws).all()) and g.guards_intact()

    # the last legal offset runs
    assert raw_run(L, t, t0, n_steps, src, prm, losses, g) == 0, L.fn("last_error")()
    torch.cuda.synchronize()
    what = "%s run, %d pairs" % (name, n_pairs)
    check_workspace(L, g, n_pairs, True, what)
    # the chain, with tensors of its own
    params, moms, gc = dev(L.oracle.flat(*nets)), torch.zeros_like(fresh), guarded_ws(L, n_pairs)
    assert same_bits(params, fresh)
    want = []
    for s in range(n_steps):
        rows = t.perm[t0 + s * n_pairs:t0 + (s + 1) * n_pairs].contiguous()
        patches = L.sample(t, rows, None if src is None else src[s].contiguous(), prm[s].contiguous())
        if s == 0:
            outside = (used[:n_pairs, 3] > used[:n_pairs, 2] + 20)
            for i in np.nonzero(outside)[0]:              # right patches wholly outside the image: 0 * contrast + brightness
                for side in (1, 2):
                    assert bool((patches[i, side] == patches[i, side, 0, 0]).all()), (i, side)
                assert float(patches[i, 0].std()) > 0
        gc.poison()
        want.append(L.mod.step_batch(patches, params, moms, LR, MOM, gc.ws))
        check_workspace(L, gc, n_pairs, False, "%s chain step %d" % (what, s))
    want = torch.cat(want)
    got = losses.cpu().numpy()
    print("%s: losses of the run %s, of the chain %s" % (what, got[:n_steps], want.cpu().numpy()))
    assert np.isfinite(got).all()
    assert same_bits(losses[:n_steps], want)
    assert got[n_steps] == LOSS_SENTINEL                 # one loss per step, nothing after them
    assert same_bits(t.params, params) and same_bits(t.moms, moms) and not same_bits(params, fresh)
    assert len(set(got[:n_steps].tolist())) >= 3         # the steps differ, so an offset error cannot hide


# ---- (d) refusals -------------------------------------------------------------------------------------------------------------------
STEP_ARGS = [("n_pairs", 0, "n_pairs 0"), ("n_pairs", "MAX+1", "n_pairs %d"), ("params", None, "null params"), ("moms", None, "null params"),
             ("params", "misaligned", "params not 16-byte aligned"), ("ws", None, "workspace of"), ("ws_bytes", -1, "workspace of"),
             ("ws", "misaligned", "workspace not 16-byte aligned")]
RUN_ARGS = [("perm", None, "null pointer"), ("prm", None, "null pointer"), ("losses", None, "null pointer"), ("n_steps", -1, "n_steps -1"),
            ("t0", -1, "steps [-1, 3)"), ("t0", 5, "steps [5, 9)"), ("n_nnz", 0, "empty nnz"), ("nnz", None, "nnz pointer")]
IMAGE_ARGS = [("x0", None, "null image"), ("x1", None, "null image"), ("n_img", 0, "bad image dims 0"), ("H", 3, "x 3 x"), ("W", 3, "x 3"),
              ("H", 32768, "32768 x"), ("W", 32768, "x 32768"), (("n_img", "H", "W"), (1025, 32767, 32767), "bad image dims 1025"),
              (("n_img", "H", "W"), (1 << 20, 1024, 1024), "bad image dims 1048576")]
STORE_ARGS = [("planes", None, "null planes"), ("table", None, "null planes"), ("n_planes", 0, "n_planes 0"), ("n_planes", -1, "n_planes -1"),
              ("src", None, "null pointer")]
REFUSALS = (
    [(name, "step_batch") + c for name in ("slow", "mb_slow") for c in STEP_ARGS + [("patches", None, "null pointer"), ("loss", None, "null pointer")]] +
    [("slow", "run") + c for c in STEP_ARGS + RUN_ARGS + IMAGE_ARGS] +
    [("mb_slow", "run") + c for c in STEP_ARGS + RUN_ARGS + STORE_ARGS])


def refusal_buffers(L):
    """Small valid arguments for both entry points; every buffer a call writes is NaN (the losses a sentinel), the workspace
    guarded.  Built once per library."""
    import torch
    if hasattr(L, "refusal"):
        return L.refusal
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(0)
    n_pairs = 2
    g = guarded_ws(L, n_pairs)
    t = dict(nnz=dev(np.array([[1, 4, 4, 1], [1, 3, 5, 2], [1, 5, 3, 1]], np.float32)), perm=dev(np.array([0, 1, 2, 0, 1, 2, 0, 1], np.int32)),
             prm=dev(L.mod.draw_params(rng, L.opt(), 2, n_pairs)), src=torch.zeros((2, n_pairs, 2), dtype=torch.int32, device="cuda"),
             patches=dev(rng.standard_normal((n_pairs, 3, L.PS, L.PS)).astype(np.float32)), params=nan(L.NPARAMS), moms=nan(L.NPARAMS),
             loss=torch.full((1,), LOSS_SENTINEL, device="cuda"), losses=torch.full((4,), LOSS_SENTINEL, device="cuda"), ws=g.ws)
    scalars = dict(n_nnz=3, n_pairs=n_pairs, n_perm=8, t0=0, n_steps=2, lr=LR, mom=MOM, ws_bytes=g.n * 4, stream=None)
    if L.name == "slow":
        t.update(x0=dev(rng.standard_normal((1, 8, 8)).astype(np.float32)), x1=dev(rng.standard_normal((1, 8, 8)).astype(np.float32)))
        scalars.update(n_img=1, H=8, W=8)
    else:
        t.update(planes=dev(rng.standard_normal(2 * 8 * 8).astype(np.float32)), table=dev(np.array([[0, 8 | 8 << 32], [64, 8 | 8 << 32]], np.int64)))
        scalars.update(n_planes=2)
        t["src"][..., 1] = 1
    L.refusal = (t, scalars, g)
    return L.refusal


def call_with(L, fn, tensors, scalars, arg=(), value=()):
    vals = dict(scalars)
    vals.update({k: v.data_ptr() for k, v in tensors.items()})
    for a, v in zip(arg, value) if isinstance(arg, tuple) else [(arg, value)]:
        if v == "misaligned":
            vals[a] += 4
        elif v == "MAX+1":
            vals[a] = L.MAX + 1
        elif a == "ws_bytes":
            vals[a] += v                                   # one byte short
        else:
            vals[a] = v
    return L.fn(fn)(*[vals[k] for k in (STEP_SIG if fn == "step_batch" else L.RUN_SIG)])


@pytest.mark.parametrize("name,fn,arg,value,names", REFUSALS, ids=["%s-%s-%s-%s" % (c[0], c[1], "+".join(c[2]) if isinstance(c[2], tuple) else c[2], c[3])
                                                                   for c in REFUSALS])
def test_refusals_are_loud_and_touch_nothing(name, fn, arg, value, names):
    """One case per MC_REQUIRE that train_slow.hip and train_mb_slow.hip can reach (their shared checks are train_net.h's and train_slow_fc.h's): MC_EINVAL, a message that names the argument, and no
    buffer written.  All of them are refused on the host before any launch."""
    import torch
    L = lib_of(name)
    tensors, scalars, g = refusal_buffers(L)
    torch.cuda.synchronize()
    rc = call_with(L, fn, tensors, scalars, arg, value)
    msg = L.fn("last_error")().decode()
    torch.cuda.synchronize()
    print("%s_%s(%s = %s): rc %d, %r" % (L.tl.PREFIX, fn, arg, value, rc, msg))
    assert rc == MC_EINVAL
    if "%d" in names:
        names = names % (L.MAX + 1)
    assert msg and names in msg and L.tl.PREFIX[3:] in msg, msg
    for k in ("params", "moms", "ws"):
        assert bool(torch.isnan(tensors[k]).all()), k
    assert bool((tensors["loss"] == LOSS_SENTINEL).all()) and bool((tensors["losses"] == LOSS_SENTINEL).all())
    assert g.guards_intact()


@pytest.mark.parametrize("name", ["slow", "mb_slow"])
def test_the_refusal_baseline_is_accepted(name):
    """The arguments the refusal cases start from are valid: each refusal is due to the one argument it changes.  Runs on
    copies of the written buffers, so that it does not disturb them."""
    import torch
    L = lib_of(name)
    tensors, scalars, g = refusal_buffers(L)
    copies = dict(tensors)
    g2 = guarded_ws(L, scalars["n_pairs"])
    copies.update(params=dev(L.oracle.flat(*wide_of(L))), moms=torch.zeros(L.NPARAMS, device="cuda"), loss=tensors["loss"].clone(),
                  losses=tensors["losses"].clone(), ws=g2.ws)
    for fn in ("step_batch", "run"):
        assert call_with(L, fn, copies, scalars) == 0, (fn, L.fn("last_error")())
        torch.cuda.synchronize()
        check_workspace(L, g2, scalars["n_pairs"], fn == "run", "%s baseline %s" % (name, fn))
        g2.poison()
    assert torch.isfinite(copies["loss"]).all() and float(copies["loss"]) != LOSS_SENTINEL
    assert torch.isfinite(copies["losses"]).all() and bool((copies["losses"][:2] != LOSS_SENTINEL).all())
    assert bool((copies["losses"][2:] == LOSS_SENTINEL).all())
    assert torch.isfinite(copies["params"]).all() and torch.isfinite(copies["moms"]).all()


@pytest.mark.parametrize("name", ["slow", "mb_slow"])
def test_workspace_sizes_are_zero_where_documented(name):
    L = lib_of(name)
    wb = L.fn("workspace_bytes")
    for n in (0, -1, L.MAX + 1, -2 ** 31, 2 ** 31 - 1):
        assert wb(n) == 0, n
    for n in (1, 2, 63, L.MAX):
        assert wb(n) == areas(L, n)[1] * 4 > 0, n
