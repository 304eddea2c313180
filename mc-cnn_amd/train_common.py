"""The host side that the four trainable nets share: train.py (KITTI fast), train_slow.py (KITTI slow), train_mb.py
(Middlebury fast) and train_mb_slow.py (Middlebury slow) keep what is theirs -- data, image store, `Trainer.run`'s argument
list, the saved net -- and take from here

  * the parser blocks (`new_parser`, `pipeline_prm`, `check_bs`) and the augmentation defaults,
  * the augmentation draws and the epoch schedule (`draw_params`, `n_steps_per_epoch`, `training_rows`, `run_epochs`),
  * the flat parameter layout of a net of l1 convolutions and, for arch slow, l2 + 1 Linears (`NetShape`),
  * the device state common to every `Trainer` (`TrainerBase`) and the one-step wrapper (`step_batch`).

Randomness: ONE `numpy.random.Generator(-seed)` draws the permutation (`training_rows`; once, the same every epoch) and
then, chunk by chunk, the augmentation parameters (`run_epochs`) and whatever the chunk callback draws after them
(Middlebury's sources).  That order is what makes a run bitwise reproducible for a given -seed.
"""
import argparse
import math
import os
import time

import numpy as np

from .params import NET_SHAPES, SM_SKIP, SM_TERMINATE

# ---- flags -------------------------------------------------------------------------------------------------------------
PIPELINE_FLAGS = (("L1", "cbca_i1", "cbca_i2", "sgm_i"),                                                      # int
                  ("tau1", "pi1", "pi2", "sgm_q1", "sgm_q2", "alpha1", "tau_so", "blur_sigma", "blur_t"))     # float

# main.lua:33-64: the augmentation, per dataset
AUG_DEFAULTS = {
    "kitti": dict(hflip=0, vflip=0, rotate=7, hscale=0.9, scale=1, trans=0, hshear=0.1, brightness=0.7, contrast=1.3,
                  d_vtrans=0, d_rotate=0, d_hscale=1, d_hshear=0, d_brightness=0.3, d_contrast=1),
    "mb": dict(hflip=0, vflip=0, rotate=28, hscale=0.8, scale=0.8, trans=0, hshear=0.1, brightness=1.3, contrast=1.1,
               d_vtrans=1, d_rotate=3, d_hscale=0.9, d_hshear=0.3, d_brightness=0.7, d_contrast=1.1),
}
AUG_DEFAULTS["kitti2015"] = AUG_DEFAULTS["kitti"]


def new_parser(dataset, arch, t, train_defaults):
    """An ArgumentParser with the flags every command line of `main.py <dataset> <arch>` has: -net_fname, -gpu, the 13
    pipeline flags with the defaults of table t, -sm_terminate / -sm_skip, -seed, the optimiser's flags with
    train_defaults, the dataset's augmentation flags, -epochs and -max_steps.  The caller adds -a and its own."""
    ap = argparse.ArgumentParser(prog="main.py %s %s" % (dataset, arch), prefix_chars="-")
    ap.add_argument("-net_fname", default="random:42")
    ap.add_argument("-gpu", type=int, default=1, help="1-based, as cutorch.setDevice (main.lua:16,342)")
    for keys, kind in zip(PIPELINE_FLAGS, (int, float)):
        for k in keys:
            ap.add_argument("-" + k, type=kind, default=t[k])
    ap.add_argument("-sm_terminate", default="", choices=sorted(SM_TERMINATE), help="main.lua:25")
    ap.add_argument("-sm_skip", default="", choices=sorted(SM_SKIP), help="main.lua:26")
    ap.add_argument("-seed", type=int, default=42)
    for k, v in train_defaults.items():
        ap.add_argument("-" + k, type=type(v), default=v)
    for k, v in AUG_DEFAULTS[dataset].items():
        ap.add_argument("-" + k, type=int if k in ("hflip", "vflip") else float, default=float(v) if k not in ("hflip", "vflip") else v)
    ap.add_argument("-epochs", type=int, default=14, help="main.lua:777 runs 14")
    ap.add_argument("-max_steps", type=int, default=0, help="stop training after this many steps in all (0: no limit)")
    return ap


NET_FLAGS = ("-l1", "-fm", "-ks")   # main.lua:212-214, 240-242, 271-273: what the reference builds the net from
L1_TRAINABLE = (1, 5)               # include/mc_train_depth.h


def add_net_flags(ap, dataset, arch):
    """-l1 (3x3 convolutions; not -L1, the cross arm length: the flags are case-sensitive), -fm (feature maps) and -ks (kernel
    size) with the defaults of (dataset, arch)."""
    l1, fm = NET_SHAPES.get((dataset, arch), (0, 0))
    ap.add_argument("-l1", type=int, default=l1, help="convolution layers of the fast net, %d..%d" % L1_TRAINABLE)
    ap.add_argument("-fm", type=int, default=fm, help="feature maps per layer; only 64 is supported")
    ap.add_argument("-ks", type=int, default=3, help="kernel size; only 3 is supported")


def refuse_net_flags(argv, who):
    """-l1 / -fm / -ks on a command line whose arch is not fast: arch slow has the shape its libraries are compiled for, ad and
    census have no net."""
    given = [a for a in argv[2:] if a in NET_FLAGS]
    if given and len(argv) >= 2 and argv[1] != "fast":
        why = ("its towers (fm 112) run on another GEMM family, compiled for the data set's l1" if argv[1] == "slow" else "it has no net")
        raise SystemExit("%s: %s is not supported for arch %s: %s; -l1 %d..%d (with -fm 64 -ks 3) builds {kitti|kitti2015|mb} fast"
                         % ((who, given[0], argv[1], why) + L1_TRAINABLE))


def check_net_flags(opt, who):
    """What of -l1 / -fm / -ks the fast net's kernels serve; names it where they do not."""
    if not L1_TRAINABLE[0] <= opt.l1 <= L1_TRAINABLE[1]:
        raise SystemExit("%s: -l1 %d is not supported: l1 %d..%d are (a pair's step keeps every activation in a CU's 160 KiB of LDS, "
                         "which six layers on 13 x 13 patches exceed)" % ((who, opt.l1) + L1_TRAINABLE))
    if opt.fm != 64:
        raise SystemExit("%s: -fm %d is not supported: only -fm 64 is (the training GEMMs tile 64 output maps as two 32 x 32 tiles and "
                         "the hinge gives each of a wave's 64 lanes a channel); -l1 %d..%d is" % ((who, opt.fm) + L1_TRAINABLE))
    if opt.ks != 3:
        raise SystemExit("%s: -ks %d is not supported: only -ks 3 is (every convolution kernel here is 3 x 3); -l1 %d..%d is"
                         % ((who, opt.ks) + L1_TRAINABLE))


FC_FLAGS = ("-l2", "-nh2")          # main.lua:76-77, 123-124: what the reference builds the accurate net's FC stack from
L2_TRAINABLE = (1, 7)               # include/mc_train_slow_depth.h; with the last Linear, the 2..8 layers mc_fc_stack takes
NH2 = 384                           # the one hidden width of mc_fc_stack, mc_fc_split_stack and the training GEMMs


def add_fc_flags(ap, dataset):
    """-l2 (hidden Linears of arch slow's FC stack, default the data set's) and -nh2 (their units)."""
    from .main import FC_SHAPES
    l2, nh2 = FC_SHAPES[dataset]
    ap.add_argument("-l2", type=int, default=l2, help="hidden Linears of the accurate net, %d..%d" % L2_TRAINABLE)
    ap.add_argument("-nh2", type=int, default=nh2, help="units per hidden Linear; only %d is supported" % NH2)


def refuse_fc_flags(argv, who):
    """-l2 / -nh2 on a command line whose arch is not slow: the fast net, ad and census have no FC stack."""
    given = [a for a in argv[2:] if a in FC_FLAGS]
    if given and len(argv) >= 2 and argv[1] != "slow":
        why = "the fast net's cost is StereoJoin's dot product" if argv[1] == "fast" else "its cost is computed from the image pair"
        raise SystemExit("%s: %s is not supported for arch %s: it has no FC stack (%s); -l2 %d..%d (with -nh2 %d) builds "
                         "{kitti|kitti2015|mb} slow" % ((who, given[0], argv[1], why) + L2_TRAINABLE + (NH2,)))


def check_fc_flags(opt, who):
    """What of -l2 / -nh2 the accurate net's kernels serve; names it where they do not."""
    if not L2_TRAINABLE[0] <= opt.l2 <= L2_TRAINABLE[1]:
        raise SystemExit("%s: -l2 %d is not supported: l2 %d..%d are (the training step's head reads a hidden Linear's %d activations, "
                         "and mc_fc_stack / mc_fc_split_stack take 2..8 layers, the last Linear among them)"
                         % ((who, opt.l2) + L2_TRAINABLE + (NH2,)))
    if opt.nh2 != NH2:
        raise SystemExit("%s: -nh2 %d is not supported: only -nh2 %d is (mc_fc_stack and mc_fc_split_stack are %d wide, and so are "
                         "the training step's GEMMs); -l2 %d..%d is" % ((who, opt.nh2, NH2, NH2) + L2_TRAINABLE))


FC_MODES = ("fp32", "bf16x3")      # fc.fc_cost_volumes: mc_fc_stack | mc_fc_split_stack (include/mc_fc_split.h)


def add_fc_mode_flag(ap):
    """-fc_mode: how arch slow's FC stack takes its products wherever a command line predicts (-a predict | time | test_te | test_all,
    the test_te after train_tr included).  Not a flag of main.lua; the default is today's fp32 kernel."""
    ap.add_argument("-fc_mode", default="fp32", choices=FC_MODES,
                    help="arch slow's FC stack: fp32 (mc_fc_stack, exact products) or bf16x3 (mc_fc_split_stack, three bf16 products each)")


def check_fc_mode(opt, arch, who):
    """-fc_mode bf16x3 where there is no FC stack: refused, naming where it applies.  -fc_mode fp32 is taken there and means nothing, so
    it leaves opt as it is without the flag."""
    if arch == "slow":
        return
    mode = opt.__dict__.pop("fc_mode", "fp32")
    if mode != "fp32":
        opt.fc_mode = mode
        raise SystemExit("%s: -fc_mode %s is not supported for arch %s: it has no FC stack (%s); -fc_mode fp32 | bf16x3 is a flag of "
                         "arch slow" % (who, opt.fc_mode, arch, "the fast net's cost is StereoJoin's dot product" if arch == "fast"
                                        else "its cost is computed from the image pair"))


CONV_MODES = ("fp32", "bf16x3")    # adcensus.conv3x3: mc_conv3x3 | mc_conv_split for the layers it takes (include/mc_conv_split.h)


def add_conv_mode_flag(ap):
    """-conv_mode: how the feature net's 3x3 convolutions take their products wherever a command line predicts with arch fast or arch
    slow (-a predict | time | test_te | test_all, the test_te after train_tr included).  Not a flag of main.lua; the default is today's
    fp32 kernel, and training never reads it."""
    ap.add_argument("-conv_mode", default="fp32", choices=CONV_MODES,
                    help="the feature net's convolutions: fp32 (mc_conv3x3, exact products) or bf16x3 (mc_conv_split, three bf16 products "
                         "each, for the layers with 16n input channels; about 1e-5 of the output scale less exact)")


def check_conv_mode(opt, arch, who):
    """-conv_mode bf16x3 where there is no net: refused, naming where it applies.  opt keeps conv_mode only where it is bf16x3, so a
    command line without the flag (or with -conv_mode fp32) parses to the namespace it parsed to before the flag existed; readers use
    getattr(opt, "conv_mode", "fp32")."""
    mode = opt.__dict__.pop("conv_mode", "fp32")
    if mode == "fp32":
        return
    opt.conv_mode = mode
    if arch not in ("fast", "slow"):
        raise SystemExit("%s: -conv_mode %s is not supported for arch %s: it has no net (its cost is computed from the image pair); "
                         "-conv_mode fp32 | bf16x3 is a flag of arch fast and arch slow" % (who, mode, arch))


def pipeline_prm(t, opt):
    """The hyper-parameter table of the post-CNN pipeline: t with the 13 flags and the stage switches of opt."""
    prm = dict(t)
    prm["sm_terminate"], prm["sm_skip"] = opt.sm_terminate, opt.sm_skip   # make_params maps the stage names
    for k in PIPELINE_FLAGS[0] + PIPELINE_FLAGS[1]:
        prm[k] = getattr(opt, k)
    return prm


def check_bs(opt, who, where):
    if opt.bs < 2 or opt.bs % 2:
        raise SystemExit("%s: -bs %d: a batch is pairs of samples (%s)" % (who, opt.bs, where))


# ---- draws and schedule ------------------------------------------------------------------------------------------------
def n_steps_per_epoch(n, bs):
    """`for t = 1, n - bs/2, bs/2` (main.lua:787)."""
    return len(range(1, n - bs // 2 + 1, bs // 2))


def draw_params(rng, opt, n_steps, n_pairs):
    """The augmentation parameters of main.lua:790-814 for n_steps x n_pairs pairs, (n_steps, n_pairs, 18) float32 in the
    order of include/mc_train.h.  Vectorised numpy draws: the distributions and flags of the reference, not its stream."""
    sh = (n_steps, n_pairs)
    u = lambda a, b: rng.uniform(a, b, sh)
    assert opt.hscale <= 1 and opt.scale <= 1
    assert opt.contrast >= 1 and opt.d_contrast >= 1
    d_pos = u(-opt.true1, opt.true1)
    d_neg = u(opt.false1, opt.false2)
    d_neg = np.where(rng.uniform(0, 1, sh) < 0.5, -d_neg, d_neg)
    s = u(opt.scale, 1)
    sx, sy = s * u(opt.hscale, 1), s
    if opt.hflip == 1:
        sx = np.where(rng.uniform(0, 1, sh) < 0.5, -sx, sx)
    if opt.vflip == 1:
        sy = np.where(rng.uniform(0, 1, sh) < 0.5, -sy, sy)
    hshear = u(-opt.hshear, opt.hshear)
    tx, ty = u(-opt.trans, opt.trans), u(-opt.trans, opt.trans)
    rot = opt.rotate * math.pi / 180
    phi = u(-rot, rot)
    brightness = u(-opt.brightness, opt.brightness)
    contrast = u(1 / opt.contrast, opt.contrast)
    sx_ = sx * u(opt.d_hscale, 1)
    hshear_ = hshear + u(-opt.d_hshear, opt.d_hshear)
    ty_ = ty + u(-opt.d_vtrans, opt.d_vtrans)
    drot = opt.d_rotate * math.pi / 180
    phi_ = phi + u(-drot, drot)
    brightness_ = brightness + u(-opt.d_brightness, opt.d_brightness)
    contrast_ = contrast * u(1 / opt.d_contrast, opt.d_contrast)
    return np.stack([d_pos, d_neg, sx, sy, phi, tx, ty, hshear, brightness, contrast,
                     sx_, sy, phi_, tx, ty_, hshear_, brightness_, contrast_], axis=-1).astype(np.float32)


def training_rows(opt, data):
    """(nnz, rng, perm): the pixel list of -a train_tr (nnz_tr) or train_all (nnz_tr .. nnz_te), the run's Generator(-seed)
    and its first draw, the permutation of the rows (main.lua:657: drawn once, the same every epoch)."""
    nnz = data["nnz_tr"] if opt.a == "train_tr" else np.concatenate([data["nnz_tr"], data["nnz_te"]], 0)
    nnz = np.asarray(nnz, np.float32).reshape(-1, 4)
    rng = np.random.default_rng(opt.seed)
    return nnz, rng, rng.permutation(nnz.shape[0]).astype(np.int32)


def run_epochs(trainer, rng, opt, steps, n_pairs, device, chunk_steps, run_chunk):
    """main.lua:777-875: -epochs epochs of `steps` steps, enqueued in chunks of chunk_steps; lr / 10 from epoch 12; at most
    -max_steps steps in all.  Per chunk the augmentation parameters are drawn from rng, then
    `run_chunk(s0, prm, lr, losses)` draws what else the net needs and calls `trainer.run` for steps s0 .. s0 + len(prm) - 1
    of the epoch, rows s0 * n_pairs on of the permutation, writing their losses to losses[0:].  Leaves the last learning
    rate in opt.lr, as main.lua does.  Returns (every step's loss in order, float32; the number of epochs run)."""
    import torch
    if steps < 1:
        raise SystemExit("train: %d training pairs, fewer than a batch of %d" % (len(trainer.perm), n_pairs))
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
        for s0 in range(0, n, chunk_steps):
            k = min(chunk_steps, n - s0)
            prm = torch.from_numpy(draw_params(rng, opt, k, n_pairs)).to(device)
            run_chunk(s0, prm, lr, losses[s0:])
        ep = losses[:n].cpu().numpy().copy()   # synchronises: the epoch's steps are done
        all_losses.append(ep)
        ok = (ep >= 0) & (ep < 100)           # main.lua:861-866
        for e in ep[~ok]:
            print("WARNING! err=%f" % e)
        print(epoch, float(ep[ok].mean()) if ok.any() else float("nan"), lr, time.perf_counter() - t_start)
        if budget is not None:
            budget -= n
    opt.lr = lr
    return np.concatenate(all_losses) if all_losses else np.zeros(0, np.float32), len(all_losses)


# ---- the net's parameters ----------------------------------------------------------------------------------------------
class NetShape:
    """The flat parameter buffer of a training library: l1 3x3 convolutions 1 -> fm -> .. -> fm and, where l2 > 0, the
    Linears 2 fm -> nh2 (l2 times) -> 1, every tensor followed by its bias (w1 b1 .. fw1 fb1 ..: the order of the
    library's header).  The fast nets have l2 = 0 and no Linear at all."""

    def __init__(self, l1, fm, l2, nh2, nparams, library):
        self.l1, self.fm, self.l2, self.nh2, self.nparams, self.library = l1, fm, l2, nh2, nparams, library

    def conv_shapes(self):
        return [(self.fm, 1 if i == 0 else self.fm, 3, 3) for i in range(self.l1)]

    def fc_shapes(self):
        dims = [2 * self.fm] + [self.nh2] * self.l2 + [1] if self.l2 else []
        return [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)]

    def flat_params(self, conv_layers, fc_layers=()):
        """[(w, b)] of the convolutions and [(w (out,in), b)] of the Linears -> one float32 vector."""
        layers = list(conv_layers) + list(fc_layers)
        want = self.conv_shapes() + self.fc_shapes()
        got = [tuple(np.shape(w)) for w, _ in layers], [tuple(np.shape(b)) for _, b in layers]
        if got != (want, [(s[0],) for s in want]):
            fc = ", l2 %d, nh2 %d" % (self.l2, self.nh2) if self.l2 else ""
            raise ValueError("net of weights %s and biases %s, %s trains l1 %d, fm %d%s on 1 input plane"
                             % (got + (self.library, self.l1, self.fm, fc)))
        out = np.concatenate([np.asarray(a, np.float32).ravel() for wb in layers for a in wb])
        assert out.size == self.nparams
        return out

    def unflat_params(self, v):
        """The inverse of flat_params: (conv_layers, fc_layers)."""
        v = np.asarray(v, np.float32)
        if v.size != self.nparams:
            raise ValueError("%d floats, %s's net has %d" % (v.size, self.library, self.nparams))
        out, o = [], 0
        for shape in self.conv_shapes() + self.fc_shapes():
            n = int(np.prod(shape))
            out.append((v[o:o + n].reshape(shape).copy(), v[o + n:o + n + shape[0]].copy()))
            o += n + shape[0]
        return out[:self.l1], out[self.l1:]

    def tensor_names(self):
        """The tensors of the flat buffer with their sizes, in order."""
        names = []
        for prefix, shapes in (("", self.conv_shapes()), ("f", self.fc_shapes())):
            for i, s in enumerate(shapes):
                names += [("%sw%d" % (prefix, i + 1), int(np.prod(s))), ("%sb%d" % (prefix, i + 1), s[0])]
        return names

    def init_net(self, seed, gain=1.0):
        """(conv_layers, fc_layers) drawn uniformly from +-gain/sqrt(fan_in): gain 1 is the range of
        nn.SpatialConvolution:reset and nn.Linear:reset (the draws are numpy's, not Torch's stream)."""
        rng = np.random.default_rng(seed)
        nets = []
        for shapes in (self.conv_shapes(), self.fc_shapes()):
            layers = []
            for s in shapes:
                bound = gain / np.sqrt(np.prod(s[1:]))
                layers.append((rng.uniform(-bound, bound, s).astype(np.float32), rng.uniform(-bound, bound, (s[0],)).astype(np.float32)))
            nets.append(layers)
        return nets[0], nets[1]


# ---- the device side ---------------------------------------------------------------------------------------------------
def _p(t):
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def new_workspace(tlib, who, n_pairs, device):
    """(bytes, float32 tensor of exactly that size) of `<prefix>_workspace_bytes(n_pairs)`, which answers 0 outside the
    library's range of n_pairs."""
    import torch
    nbytes = getattr(tlib.load(), tlib.PREFIX + "_workspace_bytes")(n_pairs)
    if nbytes == 0:
        top = " [1, %d]" % tlib.MAX_PAIRS if hasattr(tlib, "MAX_PAIRS") else ""
        raise ValueError("%s: %d pairs per batch is outside %s's range%s" % (who, n_pairs, os.path.basename(tlib.LIB_PATH), top))
    return nbytes, torch.empty(nbytes // 4, dtype=torch.float32, device=device)


class TrainerBase:
    """Device state of a training run that every net has: nnz, permutation, parameters, momenta, workspace.  A subclass
    names its library module (LIB), itself for the messages (WHO) and its NetShape (SHAPE), uploads its image store and
    defines `run`."""
    LIB = WHO = SHAPE = None

    def __init__(self, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        import torch
        self.lib = self.LIB.load()
        self.dev = device
        self.nnz = self.f32(np.asarray(nnz).reshape(-1, 4))
        self.perm = torch.from_numpy(np.ascontiguousarray(perm, np.int32)).to(device)
        self.params = self.f32(self.SHAPE.flat_params(conv_layers, fc_layers))
        self.moms = torch.zeros_like(self.params)
        self.n_pairs = n_pairs
        self.ws_bytes, self.ws = new_workspace(self.LIB, self.WHO, n_pairs, device)

    def f32(self, a):
        import torch
        return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(self.dev)

    def call(self, name, *args):
        """`<prefix>_<name>(*args, workspace, its bytes, the current stream)`, checked."""
        name = "%s_%s" % (self.LIB.PREFIX, name)
        self.LIB.check(getattr(self.lib, name)(*args, self.ws.data_ptr(), self.ws_bytes, _stream()), name)

    def nets(self):
        return self.SHAPE.unflat_params(self.params.cpu().numpy())

    def layers(self):
        return self.nets()[0]


def step_batch(tlib, who, patches, params, moms, scalars, workspace=None):
    """`<prefix>_step_batch`: one SGD step on patches (n_pairs, 3, ws, ws) with the library's scalars (lr, mom and, for the
    fast nets, margin and pow); params / moms updated in place.  Returns the device scalar of the batch's loss."""
    import torch
    n_pairs = patches.shape[0]
    if workspace is None:
        _, workspace = new_workspace(tlib, who, n_pairs, patches.device)
    loss = torch.empty(1, dtype=torch.float32, device=patches.device)
    name = tlib.PREFIX + "_step_batch"
    tlib.check(getattr(tlib.load(), name)(_p(patches), n_pairs, _p(params), _p(moms), *scalars, _p(loss), workspace.data_ptr(),
                                          workspace.numel() * 4, _stream()), name)
    return loss
