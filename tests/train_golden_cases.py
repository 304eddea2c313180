"""The cases of tests/test_gpu_train_golden.py, shared with tests/golden/make_train_bitwise.py, which records them: small runs
of the four training libraries whose parameters, momenta and losses are compared bit for bit (as SHA-256 of their bytes)
with what the libraries gave before their layer chains and host code were stated once, and of libmctraindepth.so at l1 1, 2
and 3 on both stores (one run with pow 1, one step with pow 2, one sample each) with what it gave before the fast net's
kernels were stated once in csrc/train_fast.h.

Every case has n_pairs = 9: 18 FC rows are a ragged last 16-row tile, and 9 (27 for libmctrainmbslow.so) slab rows are summed
in order.  `run` is mc_train*_run with n_steps = 3 from t0 = 5, `step` one mc_train*_step_batch on given patches (the
SAMPLE = false kernels), `sample` the fast libraries' sampler entry.  The fast libraries run with pow 1 and 2.  Weights are
init_net(seed, gain = sqrt(6)): ReLUs and hinges are about half active.

run_all() needs a GPU and the package it finds as `mc_cnn_amd` -- the recorder puts another tree first on sys.path."""
import hashlib

import numpy as np

N_PAIRS, N_STEPS, T0 = 9, 3, 5
GAIN = 6 ** 0.5
MARGIN = 0.2


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


def kitti_set():
    """Two 24 x 40 images; the first twelve nnz rows sit on the images' borders and corners, the rest anywhere."""
    rng = np.random.default_rng(11)
    n_img, H, W = 2, 24, 40
    x0 = rng.standard_normal((n_img, H, W)).astype(np.float32)
    x1 = (np.roll(x0, -3, axis=2) + 0.1 * rng.standard_normal((n_img, H, W))).astype(np.float32)
    border = [(1, 0, 0), (1, 0, W - 1), (1, H - 1, 0), (2, H - 1, W - 1), (2, 0, 17), (1, H - 1, 20), (2, 11, 0), (1, 12, W - 1),
              (2, 1, 1), (1, H - 2, W - 2), (2, 0, 3), (1, 2, W - 1)]
    n = 60
    rest = np.stack([rng.integers(1, n_img + 1, n), rng.integers(0, H, n), rng.integers(0, W, n)], 1)
    nnz = np.concatenate([np.array(border), rest]).astype(np.float32)
    nnz = np.concatenate([nnz, rng.integers(1, 6, (nnz.shape[0], 1)).astype(np.float32)], 1)      # the disparity
    # the steps read rows T0 .. T0 + 27 of perm: the border rows come first among them
    others = rng.permutation(np.arange(12, nnz.shape[0]))
    perm = np.concatenate([others[:T0], rng.permutation(12), others[T0:]]).astype(np.int32)
    return x0, x1, nnz, perm


def mb_set(tm):
    """Three scenes whose planes are 20 x 28, 24 x 36 and 32 x 24, with (lights >= 2, exposures) = (1, 2), (2, 1), (1, 1)."""
    rng = np.random.default_rng(12)
    X, nnz = [], []
    for n, (H, W, n_light, n_exp) in enumerate(((20, 28, 1, 2), (24, 36, 2, 1), (32, 24, 1, 1)), 1):
        base = rng.standard_normal((H, W)).astype(np.float32)
        lights = [np.zeros((0,), np.float32)]
        for l in range(n_light):
            lights.append(np.stack([np.stack([base * (1 + 0.1 * e) + 0.1 * l, np.roll(base, -3, 1) * (1 + 0.1 * e) + 0.1 * l +
                                              0.1 * rng.standard_normal((H, W))])[:, None] for e in range(n_exp)]).astype(np.float32))
        X.append(lights)
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        nnz.append(np.stack([np.full(H * W, n), ys.ravel(), xs.ravel(), np.full(H * W, 3)], 1)[::7])   # borders among them
    planes, table, index = tm.build_store(X, need={1, 2, 3})
    nnz = np.concatenate(nnz).astype(np.float32)
    perm = np.random.default_rng(13).permutation(nnz.shape[0]).astype(np.int32)
    return planes, table, index, nnz, perm


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _result(shape, p0, params, moms, losses):
    import torch
    torch.cuda.synchronize()
    return dict(shape=shape, params0=p0, params=params.cpu().numpy(), moms=moms.cpu().numpy(), losses=losses.cpu().numpy().reshape(-1))


def _kitti_cases(mod, parse, seed, scalars_list):
    import torch
    x0, x1, nnz, perm = kitti_set()
    shape = mod.NET
    conv, fc = shape.init_net(seed, gain=GAIN)
    nets = (conv, fc) if fc else (conv,)
    p0 = shape.flat_params(conv, fc)
    opt = parse(["kitti", "slow" if fc else "fast", "-a", "train_tr", "-hflip", "1"])[2]
    out = {}
    for tag, scalars in scalars_list:
        rng = np.random.default_rng(seed + 1)
        prm = mod.draw_params(rng, opt, N_STEPS, N_PAIRS)
        t = mod.Trainer(x0, x1, nnz, perm, *nets, N_PAIRS, torch.device("cuda"))
        losses = torch.empty(N_STEPS, dtype=torch.float32, device="cuda")
        t.run(T0, _dev(prm), *scalars, losses)
        out["run" + tag] = _result(shape, p0, t.params, t.moms, losses)
        patches = rng.standard_normal((N_PAIRS, 3, 9, 9)).astype(np.float32)
        params, moms = _dev(p0), torch.zeros(p0.size, dtype=torch.float32, device="cuda")
        loss = mod.step_batch(_dev(patches), params, moms, *scalars)
        out["step" + tag] = _result(shape, p0, params, moms, loss)
    if not fc:
        got = mod.sample(_dev(x0), _dev(x1), _dev(nnz), _dev(perm[T0:T0 + N_PAIRS]), _dev(prm[0]))
        torch.cuda.synchronize()
        out["sample"] = dict(patches=got.cpu().numpy())
    return out


def _mb_cases(mod, tm, seed, scalars_list):
    import torch
    planes, table, index, nnz, perm = mb_set(tm)
    shape = mod.NET
    conv, fc = shape.init_net(seed, gain=GAIN)
    nets = (conv, fc) if fc else (conv,)
    p0 = shape.flat_params(conv, fc)
    opt = mod.parse(["mb", "slow" if fc else "fast", "-a", "train_tr", "-hflip", "1", "-d_exp", "0.5", "-d_light", "0.5"])[2]
    out = {}
    for tag, scalars in scalars_list:
        rng = np.random.default_rng(seed + 1)
        prm = mod.draw_params(rng, opt, N_STEPS, N_PAIRS)
        ids = nnz[perm[T0:T0 + N_STEPS * N_PAIRS], 0].reshape(N_STEPS, N_PAIRS)
        src = mod.draw_sources(rng, opt, ids, index)
        t = mod.Trainer(planes, table, nnz, perm, *nets, N_PAIRS, torch.device("cuda"))
        losses = torch.empty(N_STEPS, dtype=torch.float32, device="cuda")
        t.run(T0, _dev(src), _dev(prm), *scalars, losses)
        out["run" + tag] = _result(shape, p0, t.params, t.moms, losses)
        patches = rng.standard_normal((N_PAIRS, 3, 11, 11)).astype(np.float32)
        params, moms = _dev(p0), torch.zeros(p0.size, dtype=torch.float32, device="cuda")
        loss = mod.step_batch(_dev(patches), params, moms, *scalars)
        out["step" + tag] = _result(shape, p0, params, moms, loss)
    if not fc:
        got = mod.sample(t.planes, t.table, t.nnz, _dev(perm[T0:T0 + N_PAIRS]), _dev(src[0]), _dev(prm[0]))
        torch.cuda.synchronize()
        out["sample"] = dict(patches=got.cpu().numpy())
    return out


def _depth_cases(td, main, tm, l1, store, seed):
    """libmctraindepth.so at depth l1 on `store` ("kitti" | "mb"): a run with pow 1, a step on given patches with pow 2, the
    sampler.  The shallow depths have no older library to be compared with (tests/test_gpu_train_depth.py)."""
    import torch
    shape = td.net_shape(l1)
    conv, _ = shape.init_net(seed, gain=GAIN)
    p0 = shape.flat_params(conv)
    rng = np.random.default_rng(seed + 1)
    cuda = torch.device("cuda")
    losses = torch.empty(N_STEPS, dtype=torch.float32, device="cuda")
    if store == "kitti":
        x0, x1, nnz, perm = kitti_set()
        prm = tm.draw_params(rng, main.parse(["kitti", "fast", "-a", "train_tr", "-hflip", "1"])[2], N_STEPS, N_PAIRS)
        t = td.Trainer(x0, x1, nnz, perm, conv, N_PAIRS, cuda)
        t.run(T0, _dev(prm), 0.002, 0.9, MARGIN, 1, losses)
        got = td.sample(l1, t.x0, t.x1, t.nnz, _dev(perm[T0:T0 + N_PAIRS]), _dev(prm[0]))
    else:
        planes, table, index, nnz, perm = mb_set(tm)
        opt = tm.parse(["mb", "fast", "-a", "train_tr", "-hflip", "1", "-d_exp", "0.5", "-d_light", "0.5"])[2]
        prm = tm.draw_params(rng, opt, N_STEPS, N_PAIRS)
        src = tm.draw_sources(rng, opt, nnz[perm[T0:T0 + N_STEPS * N_PAIRS], 0].reshape(N_STEPS, N_PAIRS), index)
        t = td.MbTrainer(planes, table, nnz, perm, conv, N_PAIRS, cuda)
        t.run(T0, _dev(src), _dev(prm), 0.002, 0.9, MARGIN, 1, losses)
        got = td.mb_sample(l1, t.planes, t.table, t.nnz, _dev(perm[T0:T0 + N_PAIRS]), _dev(src[0]), _dev(prm[0]))
    out = {"run_pow1": _result(shape, p0, t.params, t.moms, losses)}
    patches = rng.standard_normal((N_PAIRS, 3, 2 * l1 + 1, 2 * l1 + 1)).astype(np.float32)
    params, moms = _dev(p0), torch.zeros(p0.size, dtype=torch.float32, device="cuda")
    loss = td.step_batch(l1, _dev(patches), params, moms, 0.002, 0.9, MARGIN, 2)
    out["step_pow2"] = _result(shape, p0, params, moms, loss)
    out["sample"] = dict(patches=got.cpu().numpy())
    return {"l1_%d_%s_%s" % (l1, store, name): r for name, r in out.items()}


def run_all():
    """{"<library>/<case>": result}: a result has the flat `params`, `moms` and `losses` after the case (and `params0`, the
    NetShape `shape`), the sampler's has `patches`."""
    from mc_cnn_amd import main, train, train_depth, train_mb, train_mb_slow, train_slow
    fast = [("_pow1", (0.002, 0.9, MARGIN, 1)), ("_pow2", (0.002, 0.9, MARGIN, 2))]
    slow = [("", (0.003, 0.9))]
    out = {}
    for lib, cases in (("libmctrain.so", _kitti_cases(train, main.parse, 21, fast)), ("libmctrainslow.so", _kitti_cases(train_slow, train_slow.parse, 22, slow)),
                       ("libmctrainmb.so", _mb_cases(train_mb, train_mb, 23, fast)),
                       ("libmctrainmbslow.so", _mb_cases(train_mb_slow, train_mb, 24, slow))):
        for name, r in cases.items():
            out["%s/%s" % (lib, name)] = r
    for l1 in (1, 2, 3):
        for store in ("kitti", "mb"):
            for name, r in _depth_cases(train_depth, main, train_mb, l1, store, 30 + 2 * l1).items():
                out["libmctraindepth.so/" + name] = r
    return out


def hashes(result):
    """What the golden file keeps of a result"""
    return {k: sha(v) for k, v in result.items() if k in ("params", "moms", "losses", "patches")}


def vacuous(result):
    """Why a result proves nothing, or None: a loss that is zero or not finite, a parameter or momentum tensor that the case
    left as it was, a sampler output that is constant."""
    if "patches" in result:
        return "constant patches" if np.ptp(result["patches"]) == 0 or not np.isfinite(result["patches"]).all() else None
    if not (np.isfinite(result["losses"]).all() and (result["losses"] != 0).all()):
        return "losses %s" % result["losses"]
    o = 0
    for name, n in result["shape"].tensor_names():
        for what, before in (("params", result["params0"][o:o + n]), ("moms", np.zeros(n, np.float32))):
            if result[what][o:o + n].tobytes() == before.tobytes():
                return "%s of %s unchanged" % (what, name)
        o += n
    assert o == result["params"].size
    return None
