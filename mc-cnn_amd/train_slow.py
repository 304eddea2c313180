"""`main.lua -a train_tr | train_all` for arch slow on kitti / kitti2015 (main.lua:663-677, 753-875) on the MI355X.

The accurate net -- four valid 3x3 convolutions 1 -> 112 -> 112 -> 112 -> 112 with ReLU after every one, Reshape(bs, 224),
Linear 224 -> 384 -> 384 -> 384 -> 384 -> 1 with ReLUs, Sigmoid, BCECriterion2 -- is trained by libmctrainslow.so
(include/mc_train_slow.h): twelve kernels a step, enqueued chunk by chunk through `mc_train_slow_run` with no host round
trip inside a chunk.  The data, the sampler, the augmentation draws, the permutation and the epoch schedule are those of
train.py (`load_data`, `draw_params`, `n_steps_per_epoch`, `net_fname_of`, `evaluate`), which was written dataset-wide.

The initial weights (`init_net`) have the ranges of nn.SpatialConvolution:reset and nn.Linear:reset, +-1/sqrt(fan_in).  On
small synthetic sets the net sits on a plateau from there (its output is a constant, the loss stays at ln 2 for thousands
of steps: README.md); `train(..., init=(conv_layers, fc_layers))` starts from given nets instead.

Middlebury's accurate net (l1 5, l2 3) trains through train_mb_slow.py, `mb fast` through train_mb.py.  Not covered:
-subset, -debug, -a submit.
"""
import argparse
import os
import time

import numpy as np

from . import _train_slow_lib as tsl
from .train import draw_params, load_data, n_steps_per_epoch, net_fname_of

CHUNK_STEPS = 256           # steps enqueued per mc_train_slow_run call (one chunk of parameter draws)
SLOW_TRAIN_DEFAULTS = dict(lr=0.003, bs=128, mom=0.9, true1=1, false1=4, false2=10)   # main.lua:79-84
ACTIONS = ("train_tr", "train_all", "test_te", "test_all")
FC_DIMS = [2 * tsl.FM] + [tsl.NH2] * tsl.L2 + [1]


def conv_shapes():
    return [(tsl.FM, 1 if i == 0 else tsl.FM, 3, 3) for i in range(tsl.L1)]


def fc_shapes():
    return [(FC_DIMS[i + 1], FC_DIMS[i]) for i in range(len(FC_DIMS) - 1)]


def flat_params(conv_layers, fc_layers):
    """[(w, b)] of the convolutions and [(w (out,in), b)] of the Linears -> one float32 vector in
    include/mc_train_slow.h's order (w1 b1 .. w4 b4 fw1 fb1 .. fw5 fb5)."""
    conv_layers, fc_layers = list(conv_layers), list(fc_layers)
    got = [tuple(np.shape(w)) for w, _ in conv_layers], [tuple(np.shape(w)) for w, _ in fc_layers]
    if got != (conv_shapes(), fc_shapes()):
        raise ValueError("slow net of shapes %s, libmctrainslow.so trains l1 4, fm 112, l2 4, nh2 384 on 1 input plane" % (got,))
    out = np.concatenate([np.asarray(a, np.float32).ravel() for wb in conv_layers + fc_layers for a in wb])
    assert out.size == tsl.NPARAMS
    return out


def unflat_params(v):
    """The inverse of flat_params: (conv_layers, fc_layers)."""
    v = np.asarray(v, np.float32)
    if v.size != tsl.NPARAMS:
        raise ValueError("%d floats, a slow net has %d" % (v.size, tsl.NPARAMS))
    out, o = [], 0
    for shape in conv_shapes() + fc_shapes():
        n = int(np.prod(shape))
        out.append((v[o:o + n].reshape(shape).copy(), v[o + n:o + n + shape[0]].copy()))
        o += n + shape[0]
    return out[:tsl.L1], out[tsl.L1:]


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


def _p(t):
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Trainer:
    """Device state of a training run: images, nnz, permutation, parameters, momenta, workspace."""

    def __init__(self, x0, x1, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        import torch
        self.lib = tsl.load()
        self.dev = device
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)
        x0, x1 = np.asarray(x0), np.asarray(x1)
        self.n_img, self.H, self.W = x0.shape[0], x0.shape[-2], x0.shape[-1]
        self.x0 = f32(x0.reshape(self.n_img, self.H, self.W))
        self.x1 = f32(x1.reshape(self.n_img, self.H, self.W))
        self.nnz = f32(np.asarray(nnz).reshape(-1, 4))
        self.perm = torch.from_numpy(np.ascontiguousarray(perm, np.int32)).to(device)
        self.params = f32(flat_params(conv_layers, fc_layers))
        self.moms = torch.zeros_like(self.params)
        self.n_pairs = n_pairs
        self.ws_bytes = self.lib.mc_train_slow_workspace_bytes(n_pairs)
        if self.ws_bytes == 0:
            raise ValueError("train_slow: %d pairs per batch is outside libmctrainslow.so's range [1, %d]" % (n_pairs, tsl.MAX_PAIRS))
        self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=device)

    def run(self, t0, prm, lr, mom, losses):
        """mc_train_slow_run: prm (n_steps, n_pairs, 18) on the device; losses (>= n_steps) device float32."""
        n_steps = prm.shape[0]
        tsl.check(self.lib.mc_train_slow_run(_p(self.x0), _p(self.x1), self.n_img, self.H, self.W, _p(self.nnz), self.nnz.shape[0],
                                             _p(self.perm), self.perm.shape[0], t0, n_steps, self.n_pairs, _p(prm), _p(self.params),
                                             _p(self.moms), lr, mom, _p(losses), self.ws.data_ptr(), self.ws_bytes, _stream()),
                  "mc_train_slow_run")

    def nets(self):
        return unflat_params(self.params.cpu().numpy())


def step_batch(patches, params, moms, lr, mom, workspace=None):
    """mc_train_slow_step_batch: one SGD step on patches (n_pairs, 3, 9, 9); params / moms (870449,) updated in place.
    Returns the device scalar of the batch's loss."""
    import torch
    lib = tsl.load()
    n_pairs = patches.shape[0]
    if workspace is None:
        workspace = torch.empty(lib.mc_train_slow_workspace_bytes(n_pairs) // 4, dtype=torch.float32, device=patches.device)
    loss = torch.empty(1, dtype=torch.float32, device=patches.device)
    tsl.check(lib.mc_train_slow_step_batch(_p(patches), n_pairs, _p(params), _p(moms), lr, mom, _p(loss), workspace.data_ptr(),
                                           workspace.numel() * 4, _stream()), "mc_train_slow_step_batch")
    return loss


def save_net(fname, conv_layers, fc_layers, opt):
    """torch.save(fname, {clean_net(net_te), clean_net(net_te2), opt}, 'ascii') of arch slow (main.lua:587-600, 679-695):
    net_te is the convolutions with padding 1, each followed by cudnn.ReLU; net_te2 the Linears as
    nn.SpatialConvolution1_fw (weight (out, in), bias (1, out, 1, 1)), each followed by cudnn.ReLU, the last by
    cudnn.Sigmoid."""
    from . import t7
    mods = []
    for w, b in conv_layers:
        mods.append(t7.T7Object("cudnn.SpatialConvolution", {
            "weight": np.ascontiguousarray(w, np.float32), "bias": np.ascontiguousarray(b, np.float32),
            "nInputPlane": int(w.shape[1]), "nOutputPlane": int(w.shape[0]), "kW": 3, "kH": 3, "dW": 1, "dH": 1,
            "padW": 1, "padH": 1, "train": False}))
        mods.append(t7.T7Object("cudnn.ReLU", {"inplace": True, "train": False}))
    net_te = t7.T7Object("nn.Sequential", {"modules": mods, "train": False})
    mods2 = []
    for i, (w, b) in enumerate(fc_layers):
        mods2.append(t7.T7Object("nn.SpatialConvolution1_fw", {
            "weight": np.ascontiguousarray(w, np.float32),
            "bias": np.ascontiguousarray(b, np.float32).reshape(1, -1, 1, 1), "train": False}))
        last = i == len(fc_layers) - 1
        mods2.append(t7.T7Object("cudnn.Sigmoid" if last else "cudnn.ReLU", {"inplace": True, "train": False}))
    net_te2 = t7.T7Object("nn.Sequential", {"modules": mods2, "train": False})
    opt_t = {k: v for k, v in sorted(vars(opt).items()) if isinstance(v, (bool, int, float, str))}
    d = os.path.dirname(fname)
    if d:
        os.makedirs(d, exist_ok=True)
    t7.save(fname, [net_te, net_te2, opt_t])
    return fname


def parse(argv):
    """The flags of `main.lua {kitti|kitti2015} slow -a train_tr|train_all|test_te|test_all`: main.parse's
    hyper-parameter and augmentation flags, with arch slow's optimiser values (main.lua:79-84) and no -m / -pow.
    Returns (dataset, "slow", opt, prm) as main.parse does."""
    from .main import AUG_DEFAULTS
    from .params import SM_SKIP, SM_TERMINATE, TABLES
    if len(argv) < 2 or argv[0] not in ("kitti", "kitti2015") or argv[1] != "slow":
        raise SystemExit("train_slow: training and testing of arch slow cover {kitti|kitti2015} slow -a %s "
                         "(mb slow's l1 5 / l2 3 net trains through train_mb_slow.parse, mb fast through train_mb.parse; -a submit is out of scope)" % " | ".join(ACTIONS))
    dataset = argv[0]
    t = TABLES[(dataset, "slow")]
    ap = argparse.ArgumentParser(prog="main.py %s slow" % dataset, prefix_chars="-")
    ap.add_argument("-a", required=True)
    ap.add_argument("-net_fname", default="random:42")
    ap.add_argument("-disp_max", type=int, default=228)
    ap.add_argument("-gpu", type=int, default=1, help="1-based, as cutorch.setDevice (main.lua:16,342)")
    for k in ("L1", "cbca_i1", "cbca_i2", "sgm_i"):
        ap.add_argument("-" + k, type=int, default=t[k])
    for k in ("tau1", "pi1", "pi2", "sgm_q1", "sgm_q2", "alpha1", "tau_so", "blur_sigma", "blur_t"):
        ap.add_argument("-" + k, type=float, default=t[k])
    ap.add_argument("-sm_terminate", default="", choices=sorted(SM_TERMINATE), help="main.lua:25")
    ap.add_argument("-sm_skip", default="", choices=sorted(SM_SKIP), help="main.lua:26")
    ap.add_argument("-seed", type=int, default=42)
    for k, v in SLOW_TRAIN_DEFAULTS.items():
        ap.add_argument("-" + k, type=type(v), default=v)
    for k, v in AUG_DEFAULTS[dataset].items():
        ap.add_argument("-" + k, type=int if k in ("hflip", "vflip") else float, default=float(v) if k not in ("hflip", "vflip") else v)
    ap.add_argument("-data_dir", default="", help="default data.kitti / data.kitti2015 (main.lua:427-445)")
    ap.add_argument("-at", type=int, default=0, choices=(0, 1), help="1: KITTI 2012 and 2015 together (main.lua:403-426)")
    ap.add_argument("-epochs", type=int, default=14, help="main.lua:777 runs 14")
    ap.add_argument("-max_steps", type=int, default=0, help="stop training after this many steps in all (0: no limit)")
    opt = ap.parse_args(argv[2:])
    if opt.a not in ACTIONS:
        raise SystemExit("train_slow: -a %s is not supported for %s slow; training and testing cover -a %s (-a submit is out "
                         "of scope)" % (opt.a, dataset, " | ".join(ACTIONS)))
    if opt.at == 1 and opt.data_dir:
        raise SystemExit("main.py: -at 1 reads data.kitti and data.kitti2015 together (main.lua:403-426) and takes no -data_dir")
    if opt.bs < 2 or opt.bs % 2:
        raise SystemExit("train_slow: -bs %d: a batch is pairs of samples (main.lua:787)" % opt.bs)
    prm = dict(t)
    prm["sm_terminate"], prm["sm_skip"] = opt.sm_terminate, opt.sm_skip
    for k in ("L1", "cbca_i1", "cbca_i2", "sgm_i", "tau1", "pi1", "pi2", "sgm_q1", "sgm_q2", "alpha1", "tau_so", "blur_sigma",
              "blur_t"):
        prm[k] = getattr(opt, k)
    return dataset, "slow", opt, prm


last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def train(dataset, opt, argv, device, data=None, init=None):
    """main.lua:602-890 for arch slow, -a train_tr / train_all: returns the saved net's file name.  init:
    (conv_layers, fc_layers) to start from instead of init_net(opt.seed).  The loop is train.train's (one permutation,
    drawn once; chunks of CHUNK_STEPS steps; lr / 10 from epoch 12; -max_steps), restated for the slow Trainer's
    signature."""
    global last_run
    import torch
    if data is None:
        data = load_data(dataset, opt)
    nnz = data["nnz_tr"] if opt.a == "train_tr" else np.concatenate([data["nnz_tr"], data["nnz_te"]], 0)
    nnz = np.asarray(nnz, np.float32).reshape(-1, 4)
    n_pairs = opt.bs // 2
    rng = np.random.default_rng(opt.seed)
    perm = rng.permutation(nnz.shape[0]).astype(np.int32)
    conv_layers, fc_layers = init if init is not None else init_net(opt.seed)
    tr = Trainer(data["x0"], data["x1"], nnz, perm, conv_layers, fc_layers, n_pairs, device)
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
            tr.run(s0 * n_pairs, prm, lr, opt.mom, losses[s0:])
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
    fname = save_net(net_fname_of(dataset, "slow", argv), conv_layers, fc_layers, opt)
    last_run = {"net_fname": fname, "losses": np.concatenate(all_losses) if all_losses else np.zeros(0, np.float32),
                "epochs": len(all_losses)}
    return fname
