"""GPU: libmctrainmb.so (include/mc_train_mb.h) at its edges, as tests/test_gpu_train_limits.py has libmctrain.so: small and
the largest batch sizes, the order in which the pairs' gradients are summed, `run` against the chain sample -> step_batch on
the ragged store at plane borders (a 4 x 4 plane and plane ids outside the table among them) with the offset at its last
legal value, and one refusal per MC_REQUIRE that train_mb.hip can reach.

Every workspace is tests/test_gpu_train_slow_limits.py's `Guarded`: a 16-byte aligned slice of exactly
`mc_train_mb_workspace_bytes(n)` bytes of NaN with 4096 sentinel words on either side.  The workspace is one gradient row
per pair and one loss per pair, so after a completed step all of it must be finite, and the sentinels must be bit-identical
after every call.  Bounds are tests/test_gpu_train_mb.py's: loss, parameters and momenta 1e-5 absolute, each of the 10
momenta tensors 1e-4 of its largest magnitude."""
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_mb_oracle as mo  # noqa: E402
from test_gpu_train_mb import candidates, make_store, opt_of  # noqa: E402
from test_gpu_train_slow_limits import LOSS_SENTINEL, MC_EINVAL, NAN, Guarded  # noqa: E402
from train_fixtures import bits, dev, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

LR, MOM, MARGIN = 0.002, 0.9, 0.2
_reference = {}


@pytest.fixture(scope="module")
def tm():
    import torch
    from mc_cnn_amd import train_mb
    assert torch.cuda.is_available()
    return train_mb


def guarded_ws(tm, n_pairs):
    need = tm.tml.load().mc_train_mb_workspace_bytes(n_pairs)
    assert need == (n_pairs * tm.tml.NPARAMS + n_pairs) * 4
    return Guarded(need)


def check_workspace(g, what):
    import torch
    assert g.guards_intact(), "%s: a kernel wrote outside its workspace" % what
    assert bool(torch.isfinite(g.ws).all()), "%s: the step left part of its workspace unwritten" % what


def reference(n_pairs, pow_):
    """Non-fragile pairs (the float64 oracle alone chooses them among 3 n candidates) and the float64 step on them from
    random_layers(5): computed once per (batch size, pow) and left unchanged."""
    key = (n_pairs, pow_)
    if key not in _reference:
        t_start = time.perf_counter()
        layers = mo.random_layers(5)
        b = mo.robust_patches(layers, candidates(np.random.default_rng(3000 * pow_ + n_pairs), 3 * n_pairs), n_pairs, MARGIN)
        wp, wv, wl = mo.sgd_steps(layers, [b], LR, MOM, MARGIN, pow_)
        print("%d pairs, pow %d: float64 selection and step took %.1f s" % (n_pairs, pow_, time.perf_counter() - t_start))
        for a in (wp, wv):
            a.setflags(write=False)
        _reference[key] = (layers, b, wp, wv, wl[0])
    return _reference[key]


# ---- (a) batch sizes ------------------------------------------------------------------------------------------------------------
SIZES = [(n, p) for p in (1, 2) for n in (2, 7, 8, 9)] + [(1024, 1)]


@pytest.mark.parametrize("n_pairs,pow_", SIZES)
def test_small_and_the_largest_batch_match_float64_autograd(tm, n_pairs, pow_):
    """One step on a poisoned and guarded workspace against float64 autograd.  Measured on an MI355X, worst of the cases
    (each prints its own): loss difference 3.5e-8 (7 pairs, pow 1; 4.2e-10 at 1024), worst tensor 4.0e-6 of its largest
    magnitude (1.2e-6 at 1024)."""
    import torch
    assert n_pairs <= tm.tml.MAX_PAIRS == 1024
    layers, b, wp, wv, want_loss = reference(n_pairs, pow_)
    params = dev(mo.flat(layers))
    moms = torch.zeros_like(params)
    g = guarded_ws(tm, n_pairs)
    loss = float(tm.step_batch(dev(b), params, moms, LR, MOM, MARGIN, pow_, g.ws).cpu())
    what = "%d pairs, pow %d" % (n_pairs, pow_)
    check_workspace(g, what)
    got_p, got_v = params.cpu().numpy(), moms.cpu().numpy()
    print("%s: loss %.7f, float64 %.7f, difference %.2e; max |params - float64| %.2e, max |momenta - float64| %.2e" % (
        what, loss, want_loss, abs(loss - want_loss), np.abs(got_p - wp).max(), np.abs(got_v - wv).max()))
    assert abs(loss - want_loss) <= 1e-5
    np.testing.assert_allclose(got_p, wp, rtol=0, atol=1e-5)
    np.testing.assert_allclose(got_v, wv, rtol=0, atol=1e-5)
    assert np.abs(wv).max() > 1e-6                        # the step moved something
    mo.check_per_tensor(got_v, wv, 1e-4, what)


# ---- (b) the reduction over the pairs runs in pair order ------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1024])
def test_gradients_are_summed_in_pair_order(tm, N):
    """tests/test_gpu_train_limits.py's statement for libmctrainmb.so, whose workspace also holds one gradient row per pair:
    with lr = 1, mom = 0 and zero momenta a step leaves moms = -g; the N-pair step scales each pair's gradient by 1 / N
    (exact for a power of two) and must give the float32 sum of g_i / N over i = 0, 1, ... in that order, bit for bit, in
    all NPARAMS elements."""
    import torch
    assert N & (N - 1) == 0
    pow_ = 1
    layers, b, _, _, want_loss = reference(N, pow_)
    bd = dev(b)
    fresh = dev(mo.flat(layers))
    NP = tm.tml.NPARAMS
    G = torch.empty((N, NP), dtype=torch.float32, device="cuda")
    params, moms, g1 = fresh.clone(), torch.zeros(NP, device="cuda"), guarded_ws(tm, 1)
    t_start = time.perf_counter()
    for i in range(N):
        params.copy_(fresh)
        moms.zero_()
        tm.step_batch(bd[i:i + 1], params, moms, 1.0, 0.0, MARGIN, pow_, g1.ws)
        torch.neg(moms, out=G[i])
    torch.cuda.synchronize()
    t_single = time.perf_counter() - t_start
    assert torch.isfinite(G).all()
    check_workspace(g1, "single pairs")
    params.copy_(fresh)
    moms.zero_()
    g = guarded_ws(tm, N)
    loss = float(tm.step_batch(bd, params, moms, 1.0, 0.0, MARGIN, pow_, g.ws).cpu())
    check_workspace(g, "%d pairs" % N)
    inv = 1.0 / N
    acc = torch.zeros(NP, device="cuda")
    tiny = torch.zeros(NP, dtype=torch.bool, device="cuda")
    for i in range(N):
        gi = G[i] * inv                                   # exact: a power of two
        tiny |= (gi != 0) & (gi.abs() < 2.0 ** -100)
        acc = acc + gi                                    # one float32 add per pair, in pair order
    want = torch.zeros(NP, device="cuda") - acc           # the kernel's 0 * 0 - 1 * g
    share = float(tiny.float().mean())
    differ = (bits(moms) != bits(want)) & ~tiny
    n_differ = int(differ.sum())
    err = float((moms - want).abs().max())
    print("N %d: %d of %d elements differ from the ordered float32 sum (max |difference| %.3e); %.2e of the elements have a term "
          "below 2^-100; %d single-pair steps took %.1f s" % (N, n_differ, NP, err, share, N, t_single))
    assert share < 1e-4
    assert float((moms - want)[tiny].abs().max()) <= 1e-12 if bool(tiny.any()) else True
    assert n_differ == 0
    assert same_bits(params, fresh + moms)
    assert float(moms.abs().max()) > 1e-4                 # a gradient was there to be summed
    # the same sum in any other order is a different float32 number somewhere: the comparison can tell orders apart
    rev = torch.zeros(NP, device="cuda")
    for i in reversed(range(N)):
        rev = rev + G[i] * inv
    assert int((bits(rev) != bits(acc)).sum()) > 0
    print("N %d: loss %.7f, float64 %.7f, difference %.2e" % (N, loss, want_loss, abs(loss - want_loss)))
    assert abs(loss - want_loss) <= 1e-5


# ---- (c) run equals the chain on the ragged store ----------------------------------------------------------------------------------
def border_case(tm):
    """test_gpu_train_mb.make_store's eight planes, 4 x 4 among them.  nnz rows on every plane's corners and borders, each
    with a small disparity and with one that puts both right patches outside the plane; odd rows take their right view from
    the next plane.  The last four rows have a plane id outside the table: left -1, left n_planes, right -1, right n_planes."""
    planes, flat, table = make_store(tm)
    n = len(planes)
    nnz, src = [], []
    for k, p in enumerate(planes):
        H, W = p.shape
        pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1)]
        for j, (y, x) in enumerate(pos):
            nnz.append((1 + k, y, x, 1.0 if j % 2 else x + 60.5))
            src.append((k, (k + (j >> 1 & 1)) % n))
    out_of_range = len(nnz)
    for left, right in ((-1, 0), (n, 2), (0, -1), (3, n)):
        nnz.append((1, 5, 7, 1.0))
        src.append((left, right))
    nnz, src = np.array(nnz, np.float32), np.array(src, np.int32)
    assert (src[:out_of_range] == n - 1).any(0).all() and (planes[1].shape == (4, 4))
    return flat, table, nnz, src, out_of_range


RUN_SIG = ["planes", "table", "n_planes", "nnz", "n_nnz", "perm", "n_perm", "t0", "n_steps", "n_pairs", "src", "prm", "params", "moms", "lr",
           "mom", "margin", "pow", "losses", "ws", "ws_bytes", "stream"]
STEP_SIG = ["patches", "n_pairs", "params", "moms", "lr", "mom", "margin", "pow", "loss", "ws", "ws_bytes", "stream"]
SAMPLE_SIG = ["planes", "table", "n_planes", "nnz", "n_nnz", "rows", "src", "prm", "n_pairs", "out", "stream"]
SIG = {"mc_train_mb_run": RUN_SIG, "mc_train_mb_step_batch": STEP_SIG, "mc_train_mb_sample": SAMPLE_SIG}


def raw_run(tm, t, t0, n_steps, src, prm, losses, g):
    from mc_cnn_amd.train_common import _stream
    vals = dict(planes=t.planes.data_ptr(), table=t.table.data_ptr(), n_planes=t.table.shape[0], nnz=t.nnz.data_ptr(), n_nnz=t.nnz.shape[0],
                perm=t.perm.data_ptr(), n_perm=t.perm.shape[0], t0=t0, n_steps=n_steps, n_pairs=t.n_pairs, src=src.data_ptr(),
                prm=prm.data_ptr(), params=t.params.data_ptr(), moms=t.moms.data_ptr(), lr=LR, mom=MOM, margin=MARGIN, pow=1,
                losses=losses.data_ptr(), ws=g.ws.data_ptr(), ws_bytes=g.n * 4, stream=_stream())
    return t.lib.mc_train_mb_run(*[vals[k] for k in RUN_SIG])


@pytest.mark.parametrize("n_pairs", [1, 8])
def test_run_equals_the_chain_at_plane_borders_and_the_last_offset(tm, n_pairs):
    import torch
    flat, table, nnz, src_of_row, out_of_range = border_case(tm)
    rng = np.random.default_rng(60 + n_pairs)
    n_steps, t0 = 6, 3
    n_perm = t0 + n_steps * n_pairs                       # t0 is the last legal offset
    far = nnz[:, 3] > nnz[:, 2] + 20                      # rows whose right patches leave the plane, and the others, in turn
    perm = np.stack([rng.permutation(np.nonzero(far)[0]), rng.permutation(np.nonzero(~far)[0][:far.sum()])], 1).ravel().astype(np.int32)[:n_perm]
    bad = list(range(out_of_range, out_of_range + 4)) if n_pairs >= 4 else [out_of_range]
    perm[t0 + 1:t0 + 1 + len(bad)] = bad                  # plane ids outside the table, inside the run
    perm[t0] = 9                                          # the 4 x 4 plane takes part: its top right corner
    assert perm.size == n_perm and nnz[perm[t0], 0] == 2 and table["H"][1] == table["W"][1] == 4
    layers = mo.random_layers(3)
    prm = dev(tm.draw_params(rng, opt_of("-hflip", "1", "-vflip", "1", "-trans", "1"), n_steps, n_pairs))
    src = dev(src_of_row[perm[t0:]].reshape(n_steps, n_pairs, 2))
    t = tm.Trainer(flat, table, nnz, perm, layers, n_pairs, torch.device("cuda"))
    g = guarded_ws(tm, n_pairs)
    losses = torch.full((n_steps + 1,), LOSS_SENTINEL, dtype=torch.float32, device="cuda")
    fresh = t.params.clone()

    def untouched():
        torch.cuda.synchronize()
        return (same_bits(t.params, fresh) and not bool(t.moms.any()) and bool((losses == LOSS_SENTINEL).all()) and
                bool(torch.isnan(g.ws).all()) and g.guards_intact())

    assert raw_run(tm, t, t0, 0, src, prm, losses, g) == 0 and untouched()             # n_steps = 0 changes nothing
    assert raw_run(tm, t, t0 + 1, n_steps, src, prm, losses, g) == MC_EINVAL           # one row past the last legal offset
    msg = t.lib.mc_train_mb_last_error().decode()
    assert "permutation" in msg and "[%d, %d)" % (t0 + 1, n_perm + 1) in msg and "%d rows" % n_perm in msg, msg
    assert untouched()
    assert raw_run(tm, t, t0, n_steps, src, prm, losses, g) == 0, t.lib.mc_train_mb_last_error()
    torch.cuda.synchronize()
    what = "mb run, %d pairs" % n_pairs
    check_workspace(g, what)
    # the chain, with tensors of its own
    params, moms, gc = dev(mo.flat(layers)), torch.zeros_like(fresh), guarded_ws(tm, n_pairs)
    want, n_constant = [], 0
    for s in range(n_steps):
        rows_h = perm[t0 + s * n_pairs:t0 + (s + 1) * n_pairs]
        patches = tm.sample(t.planes, t.table, t.nnz, dev(rows_h), src[s].contiguous(), prm[s].contiguous())
        for i, r in enumerate(rows_h):                    # 0 * contrast + brightness where the plane id is outside the table
            sides = [k for k in (0, 1, 2) if not 0 <= src_of_row[r, min(k, 1)] < len(table)]
            for k in sides:
                p = prm[s, i].cpu().numpy()
                assert bool((patches[i, k] == float(np.float32(0) * p[9 if k == 0 else 17] + p[8 if k == 0 else 16])).all()), (s, i, k)
                n_constant += 1
        gc.poison()
        want.append(tm.step_batch(patches, params, moms, LR, MOM, MARGIN, 1, gc.ws))
        check_workspace(gc, "%s chain step %d" % (what, s))
    assert n_constant >= 1
    want = torch.cat(want)
    got = losses.cpu().numpy()
    print("%s: losses of the run %s, of the chain %s" % (what, got[:n_steps], want.cpu().numpy()))
    assert np.isfinite(got).all()
    assert same_bits(losses[:n_steps], want)
    assert got[n_steps] == LOSS_SENTINEL                 # one loss per step, nothing after them
    assert same_bits(t.params, params) and same_bits(t.moms, moms) and not same_bits(params, fresh)
    assert len(set(got[:n_steps].tolist())) >= 3         # the steps differ, so an offset error cannot hide


# ---- (d) refusals -------------------------------------------------------------------------------------------------------------------
STEP_ARGS = [("n_pairs", 0, "n_pairs 0"), ("n_pairs", 1025, "n_pairs 1025"), ("n_pairs", -1, "n_pairs -1"), ("params", None, "null params"),
             ("moms", None, "null params"), ("pow", 3, "pow 3"), ("pow", 0, "pow 0"), ("margin", NAN, "margin"),
             ("margin", float("inf"), "margin"), ("ws", None, "workspace"), ("ws_bytes", -1, "workspace")]
STORE_ARGS = [("planes", None, "null planes"), ("table", None, "null planes"), ("nnz", None, "null planes"), ("n_planes", 0, "n_planes 0"),
              ("n_planes", -3, "n_planes -3"), ("n_nnz", 0, "empty nnz"), ("n_nnz", -5, "empty nnz")]
REFUSALS = (
    [("mc_train_mb_step_batch",) + c for c in STEP_ARGS + [("patches", None, "null pointer"), ("loss", None, "null pointer")]] +
    [("mc_train_mb_run",) + c for c in STORE_ARGS + STEP_ARGS + [
        ("perm", None, "null pointer"), ("src", None, "null pointer"), ("prm", None, "null pointer"), ("losses", None, "null pointer"),
        ("n_steps", -1, "n_steps -1"), ("t0", -1, "steps [-1, 3)"), ("t0", 5, "steps [5, 9)"), ("n_perm", 3, "its 3 rows"),
        ("n_steps", 5, "steps [0, 10)")]] +
    [("mc_train_mb_sample",) + c for c in STORE_ARGS + [
        ("n_pairs", 0, "n_pairs 0"), ("n_pairs", (1 << 24) + 1, "n_pairs"), ("rows", None, "null pointer"), ("src", None, "null pointer"),
        ("prm", None, "null pointer"), ("out", None, "null pointer")]])


@pytest.fixture(scope="module")
def refusal_buffers(tm):
    """Small valid arguments for the three entry points; every buffer a call writes is NaN (the losses a sentinel), the
    workspace guarded."""
    import torch
    nan = lambda *shape: torch.full(shape, NAN, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(0)
    g = guarded_ws(tm, 2)
    table = np.zeros(2, tm.PLANE_DTYPE)
    table[0], table[1] = (0, 8, 8), (64, 8, 8)
    src = torch.zeros((2, 2, 2), dtype=torch.int32, device="cuda")
    src[..., 1] = 1
    t = dict(planes=dev(rng.standard_normal(128).astype(np.float32)), table=tm.device_table(table, torch.device("cuda")),
             nnz=dev(np.array([[1, 4, 4, 1], [1, 3, 5, 2], [1, 5, 3, 1]], np.float32)), rows=dev(np.array([0, 1], np.int32)),
             perm=dev(np.array([0, 1, 2, 0, 1, 2, 0, 1], np.int32)), src=src, prm=dev(tm.draw_params(rng, opt_of(), 2, 2)),
             patches=dev(candidates(rng, 2)), out=nan(2, 3, 11, 11), params=nan(tm.tml.NPARAMS), moms=nan(tm.tml.NPARAMS),
             loss=torch.full((1,), LOSS_SENTINEL, device="cuda"), losses=torch.full((4,), LOSS_SENTINEL, device="cuda"), ws=g.ws)
    scalars = dict(n_planes=2, n_nnz=3, n_pairs=2, n_perm=8, t0=0, n_steps=2, lr=LR, mom=MOM, margin=MARGIN, pow=1, ws_bytes=g.n * 4,
                   stream=None)
    return t, scalars, g


def call_with(lib, fn, tensors, scalars, arg=(), value=()):
    vals = dict(scalars)
    vals.update({k: v.data_ptr() for k, v in tensors.items()})
    for a, v in [(arg, value)] if arg else []:
        vals[a] = vals[a] + v if a == "ws_bytes" else v   # the workspace: one byte short
    return getattr(lib, fn)(*[vals[k] for k in SIG[fn]])


@pytest.mark.parametrize("fn,arg,value,names", REFUSALS, ids=["%s-%s-%s" % (c[0][12:], c[1], c[2]) for c in REFUSALS])
def test_refusals_are_loud_and_touch_nothing(tm, refusal_buffers, fn, arg, value, names):
    """One case per MC_REQUIRE that train_mb.hip can reach (its shared checks are train_net.h's and train_conv.h's),
    mc_train_mb_sample's included: MC_EINVAL, a message that names the argument, and no buffer written.  All of them are
    refused on the host before any launch."""
    import torch
    lib = tm.tml.load()
    tensors, scalars, g = refusal_buffers
    torch.cuda.synchronize()
    rc = call_with(lib, fn, tensors, scalars, arg, value)
    msg = lib.mc_train_mb_last_error().decode()
    torch.cuda.synchronize()
    print("%s(%s = %s): rc %d, %r" % (fn, arg, value, rc, msg))
    assert rc == MC_EINVAL
    assert msg and names in msg and msg.startswith("train_mb"), msg
    for k in ("out", "params", "moms", "ws"):
        assert bool(torch.isnan(tensors[k]).all()), k
    assert bool((tensors["loss"] == LOSS_SENTINEL).all()) and bool((tensors["losses"] == LOSS_SENTINEL).all())
    assert g.guards_intact()


def test_the_refusal_baseline_is_accepted(tm, refusal_buffers):
    """The arguments the refusal cases start from are valid: each refusal is due to the one argument it changes.  Runs on
    copies of the written buffers, so that it does not disturb them."""
    import torch
    lib = tm.tml.load()
    tensors, scalars, _ = refusal_buffers
    g2 = guarded_ws(tm, 2)
    copies = dict(tensors)
    copies.update(params=dev(mo.flat(mo.random_layers(1))), moms=torch.zeros(tm.tml.NPARAMS, device="cuda"), out=tensors["out"].clone(),
                  loss=tensors["loss"].clone(), losses=tensors["losses"].clone(), ws=g2.ws)
    for fn in ("mc_train_mb_sample", "mc_train_mb_step_batch", "mc_train_mb_run"):
        assert call_with(lib, fn, copies, scalars) == 0, (fn, lib.mc_train_mb_last_error())
        torch.cuda.synchronize()
        if fn != "mc_train_mb_sample":
            check_workspace(g2, fn)
            g2.poison()
    assert torch.isfinite(copies["out"]).all() and torch.isfinite(copies["loss"]).all() and float(copies["loss"]) != LOSS_SENTINEL
    assert torch.isfinite(copies["losses"]).all() and bool((copies["losses"][:2] != LOSS_SENTINEL).all())
    assert bool((copies["losses"][2:] == LOSS_SENTINEL).all())
    assert torch.isfinite(copies["params"]).all() and torch.isfinite(copies["moms"]).all()


def test_workspace_sizes_are_zero_where_documented(tm):
    lib = tm.tml.load()
    M = tm.tml.MAX_PAIRS
    for n in (0, -1, M + 1, -2 ** 31, 2 ** 31 - 1):
        assert lib.mc_train_mb_workspace_bytes(n) == 0, n
    for n in (1, 2, M):
        assert lib.mc_train_mb_workspace_bytes(n) == n * (tm.tml.NPARAMS + 1) * 4 > 0, n
