"""`main.lua mb slow -a train_tr | train_all | test_te` (main.lua:116-130, 455-490, 602-890, 1121-1131, 1183-1238) on the
MI355X.

Middlebury's accurate net is `-l1 5 -fm 112 -l2 3 -nh2 384` (main.lua:116-130): five valid 3x3 convolutions
1 -> 112 -> 112 -> 112 -> 112 -> 112 on 11 x 11 patches with ReLU after every one, Reshape(bs, 224), Linear
224 -> 384 -> 384 -> 384 -> 1 with ReLUs, Sigmoid, BCECriterion2.  It is trained by libmctrainmbslow.so
(include/mc_train_mb_slow.h): ten kernels a step, the towers one workgroup per PATCH (a pair's 221 KB of activations do not
fit a CU's LDS, one patch's 74 KB do), enqueued chunk by chunk through `mc_train_mb_slow_run`.

Nothing here is new but the net's shapes: the ragged store, its loader, the source draws and `test_te` are train_mb.py's
(`load_mb_data`, `build_store`, `device_table`, `draw_sources`, `data_dir_of`, `evaluate`), the augmentation draws and the
epoch schedule train.py's (`draw_params`, `n_steps_per_epoch`, `net_fname_of`), the saved net train_slow.py's (`save_net`,
generic in the layer count).  `init_net` has the ranges of nn.SpatialConvolution:reset and nn.Linear:reset; as for the KITTI
accurate net, small synthetic sets keep the net on the ln 2 plateau from there, and `train(..., init=(conv, fc))` starts
from given nets instead.

Not covered: -color rgb, -subset, -debug, -a submit, -a test_all (main.lua:1136 asserts it away itself), multi-GPU training.
"""
import argparse
import time

import numpy as np

from . import _train_mb_slow_lib as tmsl
from .train import draw_params, n_steps_per_epoch, net_fname_of
from .train_mb import ACTIONS, build_store, data_dir_of, device_table, draw_sources, evaluate, load_mb_data  # noqa: F401
from .train_slow import save_net

CHUNK_STEPS = 256           # steps enqueued per mc_train_mb_slow_run call (one chunk of parameter and source draws)
MB_SLOW_TRAIN_DEFAULTS = dict(lr=0.003, bs=128, mom=0.9, true1=0.5, false1=1.5, false2=18.0, d_exp=0.2,
                              d_light=0.2)   # main.lua:116-130
FC_DIMS = [2 * tmsl.FM] + [tmsl.NH2] * tmsl.L2 + [1]


def conv_shapes():
    return [(tmsl.FM, 1 if i == 0 else tmsl.FM, 3, 3) for i in range(tmsl.L1)]


def fc_shapes():
    return [(FC_DIMS[i + 1], FC_DIMS[i]) for i in range(len(FC_DIMS) - 1)]


def flat_params(conv_layers, fc_layers):
    """[(w, b)] of the convolutions and [(w (out,in), b)] of the Linears -> one float32 vector in
    include/mc_train_mb_slow.h's order (w1 b1 .. w5 b5 fw1 fb1 .. fw4 fb4)."""
    conv_layers, fc_layers = list(conv_layers), list(fc_layers)
    got = [tuple(np.shape(w)) for w, _ in conv_layers], [tuple(np.shape(w)) for w, _ in fc_layers]
    if got != (conv_shapes(), fc_shapes()):
        raise ValueError("slow net of shapes %s, libmctrainmbslow.so trains l1 5, fm 112, l2 3, nh2 384 on 1 input plane" % (got,))
    if [tuple(np.shape(b)) for _, b in conv_layers + fc_layers] != [(s[0],) for s in conv_shapes() + fc_shapes()]:
        raise ValueError("slow net with biases of shapes %s" % ([tuple(np.shape(b)) for _, b in conv_layers + fc_layers],))
    out = np.concatenate([np.asarray(a, np.float32).ravel() for wb in conv_layers + fc_layers for a in wb])
    assert out.size == tmsl.NPARAMS
    return out


def unflat_params(v):
    """The inverse of flat_params: (conv_layers, fc_layers)."""
    v = np.asarray(v, np.float32)
    if v.size != tmsl.NPARAMS:
        raise ValueError("%d floats, Middlebury's slow net has %d" % (v.size, tmsl.NPARAMS))
    out, o = [], 0
    for shape in conv_shapes() + fc_shapes():
        n = int(np.prod(shape))
        out.append((v[o:o + n].reshape(shape).copy(), v[o + n:o + n + shape[0]].copy()))
        o += n + shape[0]
    return out[:tmsl.L1], out[tmsl.L1:]


def tensor_names():
    """The 18 tensors of the flat buffer with their sizes, in order."""
    names = []
    for i, s in enumerate(conv_shapes()):
        names += [("w%d" % (i + 1), int(np.prod(s))), ("b%d" % (i + 1), s[0])]
    for i, s in enumerate(fc_shapes()):
        names += [("fw%d" % (i + 1), int(np.prod(s))), ("fb%d" % (i + 1), s[0])]
    return names


def init_net(seed, gain=1.0):
    """(conv_layers, fc_layers) drawn uniformly from +-gain/sqrt(fan_in): gain 1 is the range of
    nn.SpatialConvolution:reset and nn.Linear:reset (the draws are numpy's, not Torch's stream)."""
    rng = np.random.default_rng(seed)
    nets = []
    for shapes in (conv_shapes(), fc_shapes()):
        layers = []
        for s in shapes:
            bound = gain / np.sqrt(np.prod(s[1:]))
            layers.append((rng.uniform(-bound, bound, s).astype(np.float32), rng.uniform(-bound, bound, (s[0],)).astype(np.float32)))
        nets.append(layers)
    return nets[0], nets[1]


def parse(argv):
    """The flags of `main.lua mb slow -a train_tr | train_all | test_te` with main.lua's names and defaults: train_mb.parse's,
    with arch slow's optimiser values (main.lua:116-130) and no -m / -pow.  Returns (dataset, arch, opt, prm) as main.parse
    does; prm has left_only = 1 (outside -a predict dataset mb runs direction -1 only, main.lua:953-955)."""
    from .main import AUG_DEFAULTS
    from .params import SM_SKIP, SM_TERMINATE, TABLES
    if len(argv) < 2 or argv[0] != "mb" or argv[1] != "slow":
        raise SystemExit("train_mb_slow: training and testing of Middlebury's accurate net cover mb slow -a %s (mb fast trains "
                         "through train_mb.parse, {kitti|kitti2015} slow through train_slow.parse)" % " | ".join(ACTIONS))
    t = TABLES[("mb", "slow")]
    ap = argparse.ArgumentParser(prog="main.py mb slow", prefix_chars="-")
    ap.add_argument("-a", required=True)
    ap.add_argument("-net_fname", default="random:42")
    ap.add_argument("-gpu", type=int, default=1, help="1-based, as cutorch.setDevice (main.lua:16,342)")
    for k in ("L1", "cbca_i1", "cbca_i2", "sgm_i"):
        ap.add_argument("-" + k, type=int, default=t[k])
    for k in ("tau1", "pi1", "pi2", "sgm_q1", "sgm_q2", "alpha1", "tau_so", "blur_sigma", "blur_t"):
        ap.add_argument("-" + k, type=float, default=t[k])
    ap.add_argument("-sm_terminate", default="", choices=sorted(SM_TERMINATE), help="main.lua:25")
    ap.add_argument("-sm_skip", default="", choices=sorted(SM_SKIP), help="main.lua:26")
    ap.add_argument("-seed", type=int, default=42)
    for k, v in MB_SLOW_TRAIN_DEFAULTS.items():
        ap.add_argument("-" + k, type=type(v), default=v)
    ap.add_argument("-ds", type=int, default=2001, help="parsed and ignored: main.lua declares it and never reads it")
    for k, v in AUG_DEFAULTS["mb"].items():
        ap.add_argument("-" + k, type=int if k in ("hflip", "vflip") else float, default=float(v) if k not in ("hflip", "vflip") else v)
    ap.add_argument("-rect", default="imperfect", help="main.lua:68")
    ap.add_argument("-color", default="gray", help="main.lua:69")
    ap.add_argument("-data_dir", default="", help="default data.mb.<rect>_<color> (main.lua:456)")
    ap.add_argument("-subset", type=float, default=1.0, help="main.lua:28; only 1 is supported")
    ap.add_argument("-debug", action="store_true", help="main.lua:18; not supported")
    ap.add_argument("-epochs", type=int, default=14, help="main.lua:777 runs 14")
    ap.add_argument("-max_steps", type=int, default=0, help="stop training after this many steps in all (0: no limit)")
    opt = ap.parse_args(argv[2:])
    if opt.a == "test_all":
        raise SystemExit("train_mb_slow: -a test_all is not supported on Middlebury (main.lua:1136 asserts the same)")
    if opt.a == "submit":
        raise SystemExit("train_mb_slow: -a submit is out of scope (it writes the Middlebury evaluation's PFM files)")
    if opt.a not in ACTIONS:
        raise SystemExit("train_mb_slow: -a %s is not a training or testing action; mb slow covers -a %s" % (opt.a, " | ".join(ACTIONS)))
    if opt.color != "gray":
        raise SystemExit("train_mb_slow: -color %s: the nets here have one input plane, only -color gray is supported" % opt.color)
    if opt.subset != 1:
        raise SystemExit("train_mb_slow: -subset %g is not supported (the whole training set is used)" % opt.subset)
    if opt.debug:
        raise SystemExit("train_mb_slow: -debug (main.lua:1240-1260 writes images of every prediction) is not supported")
    if opt.bs < 2 or opt.bs % 2:
        raise SystemExit("train_mb_slow: -bs %d: a batch is pairs of samples (main.lua:789)" % opt.bs)
    prm = dict(t)
    prm["sm_terminate"], prm["sm_skip"] = opt.sm_terminate, opt.sm_skip
    for k in ("L1", "cbca_i1", "cbca_i2", "sgm_i", "tau1", "pi1", "pi2", "sgm_q1", "sgm_q2", "alpha1", "tau_so", "blur_sigma",
              "blur_t"):
        prm[k] = getattr(opt, k)
    prm["left_only"] = 1
    return "mb", "slow", opt, prm


# ---- the device side -----------------------------------------------------------------------------------------------------
def _p(t):
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Trainer:
    """Device state of a training run: planes, table, nnz, permutation, parameters, momenta, workspace."""

    def __init__(self, planes, table, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        import torch
        self.lib = tmsl.load()
        self.dev = device
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
        self.table = device_table(table, device)
        self.planes = f32(planes)
        self.nnz = f32(np.asarray(nnz).reshape(-1, 4))
        self.perm = torch.from_numpy(np.ascontiguousarray(perm, np.int32)).to(device)
        self.params = f32(flat_params(conv_layers, fc_layers))
        self.moms = torch.zeros_like(self.params)
        self.n_pairs = n_pairs
        self.ws_bytes = self.lib.mc_train_mb_slow_workspace_bytes(n_pairs)
        if self.ws_bytes == 0:
            raise ValueError("train_mb_slow: %d pairs per batch is outside libmctrainmbslow.so's range [1, %d]" % (n_pairs, tmsl.MAX_PAIRS))
        self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=device)

    def run(self, t0, src, prm, lr, mom, losses):
        """mc_train_mb_slow_run: src (n_steps, n_pairs, 2) int32 and prm (n_steps, n_pairs, 18) on the device; losses
        (>= n_steps) device float32."""
        n_steps = prm.shape[0]
        assert tuple(src.shape) == (n_steps, self.n_pairs, 2) and tuple(prm.shape) == (n_steps, self.n_pairs, tmsl.NPRM)
        tmsl.check(self.lib.mc_train_mb_slow_run(_p(self.planes), _p(self.table), self.table.shape[0], _p(self.nnz), self.nnz.shape[0],
                                                 _p(self.perm), self.perm.shape[0], t0, n_steps, self.n_pairs, _p(src), _p(prm),
                                                 _p(self.params), _p(self.moms), lr, mom, _p(losses), self.ws.data_ptr(),
                                                 self.ws_bytes, _stream()), "mc_train_mb_slow_run")

    def nets(self):
        return unflat_params(self.params.cpu().numpy())


def step_batch(patches, params, moms, lr, mom, workspace=None):
    """mc_train_mb_slow_step_batch: one SGD step on patches (n_pairs, 3, 11, 11); params / moms (835617,) updated in place.
    Returns the device scalar of the batch's loss."""
    import torch
    lib = tmsl.load()
    n_pairs = patches.shape[0]
    if workspace is None:
        nbytes = lib.mc_train_mb_slow_workspace_bytes(n_pairs)
        if nbytes == 0:
            raise ValueError("train_mb_slow: %d pairs per batch is outside libmctrainmbslow.so's range [1, %d]" % (n_pairs, tmsl.MAX_PAIRS))
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=patches.device)
    loss = torch.empty(1, dtype=torch.float32, device=patches.device)
    tmsl.check(lib.mc_train_mb_slow_step_batch(_p(patches), n_pairs, _p(params), _p(moms), lr, mom, _p(loss), workspace.data_ptr(),
                                               workspace.numel() * 4, _stream()), "mc_train_mb_slow_step_batch")
    return loss


# ---- training ------------------------------------------------------------------------------------------------------------
last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def train(opt, argv, device, data=None, init=None):
    """main.lua:602-890 for mb slow, -a train_tr / train_all: returns the saved net's file name.  init:
    (conv_layers, fc_layers) to start from instead of init_net(opt.seed).  The loop is train_mb.train's (one permutation,
    drawn once; chunks of CHUNK_STEPS steps with the pairs' sources drawn beside their augmentation parameters; lr / 10 from
    epoch 12; -max_steps), restated for the slow Trainer's signature."""
    global last_run
    import torch
    if data is None:
        data = load_mb_data(data_dir_of(opt), opt.a)
    nnz = data["nnz_tr"] if opt.a == "train_tr" else np.concatenate([data["nnz_tr"], data["nnz_te"]], 0)
    nnz = np.asarray(nnz, np.float32).reshape(-1, 4)
    n_pairs = opt.bs // 2
    rng = np.random.default_rng(opt.seed)
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    img_of = nnz[perm, 0].astype(np.int64)      # the image of every pair of an epoch, in the permutation's order
    conv_layers, fc_layers = init if init is not None else init_net(opt.seed)
    tr = Trainer(data["planes"], data["table"], nnz, perm, conv_layers, fc_layers, n_pairs, device)
    steps = n_steps_per_epoch(nnz.shape[0], opt.bs)
    if steps < 1:
        raise SystemExit("train: %d training pairs, fewer than a batch of %d" % (nnz.shape[0], n_pairs))
    budget = opt.max_steps if opt.max_steps > 0 else None
    lr = opt.lr
    all_losses = []
    t_start = time.perf_counter()
    losses = torch.empty(steps, dtype=torch.float32, device=device)
    for epoch in range(1, opt.epochs + 1):
        if budget is not None and budget <= 0:
            break
        if epoch == 12:
            lr = lr / 10
        n = steps if budget is None else min(steps, budget)
        for s0 in range(0, n, CHUNK_STEPS):
            k = min(CHUNK_STEPS, n - s0)
            prm = torch.from_numpy(draw_params(rng, opt, k, n_pairs)).to(device)
            ids = img_of[s0 * n_pairs:(s0 + k) * n_pairs].reshape(k, n_pairs)
            src = torch.from_numpy(draw_sources(rng, opt, ids, data["index"])).to(device)
            tr.run(s0 * n_pairs, src, prm, lr, opt.mom, losses[s0:])
        ep = losses[:n].cpu().numpy().copy()   # synchronises: the epoch's steps are done
        all_losses.append(ep)
        ok = (ep >= 0) & (ep < 100)           # main.lua:861-866
        for e in ep[~ok]:
            print("WARNING! err=%f" % e)
        print(epoch, float(ep[ok].mean()) if ok.any() else float("nan"), lr, time.perf_counter() - t_start)
        if budget is not None:
            budget -= n
    opt.lr = lr
    conv_layers, fc_layers = tr.nets()
    fname = save_net(net_fname_of("mb", "slow", argv), conv_layers, fc_layers, opt)
    last_run = {"net_fname": fname, "losses": np.concatenate(all_losses) if all_losses else np.zeros(0, np.float32),
                "epochs": len(all_losses)}
    return fname
