"""`main.lua -a train_tr | train_all` for arch slow on kitti / kitti2015 (main.lua:663-677, 753-875) on the MI355X.

The accurate net -- four valid 3x3 convolutions 1 -> 112 -> 112 -> 112 -> 112 with ReLU after every one, Reshape(bs, 224),
Linear 224 -> 384 -> 384 -> 384 -> 384 -> 1 with ReLUs, Sigmoid, BCECriterion2 -- is trained by libmctrainslow.so
(include/mc_train_slow.h): twelve kernels a step, enqueued chunk by chunk through `mc_train_slow_run` with no host round
trip inside a chunk.  The data, the image store, the sampler and the evaluation are train.py's (`load_data`,
`KittiTrainer`, `net_fname_of`, `evaluate`); the flags, the draws, the epoch loop, the parameter layout and `step_batch` are
train_common.py's, shared by all four nets.

The initial weights (`init_net`) have the ranges of nn.SpatialConvolution:reset and nn.Linear:reset, +-1/sqrt(fan_in).  On
small synthetic sets the net sits on a plateau from there (its output is a constant, the loss stays at ln 2 for thousands
of steps: README.md); `train(..., init=(conv_layers, fc_layers))` starts from given nets instead.

Middlebury's accurate net (l1 5, l2 3) trains through train_mb_slow.py, `mb fast` through train_mb.py, and a -l2 other than 4
through train_slow_depth.py (libmctrainslowdepth.so; main.route decides).  Not covered:
-subset, -debug, -a submit.
"""
import os

import numpy as np

from . import _train_slow_lib as tsl
from . import train_common as common
from .train import KittiTrainer, evaluate, load_data, net_fname_of  # noqa: F401
from .train_common import _p, draw_params, n_steps_per_epoch, run_epochs, training_rows  # noqa: F401

CHUNK_STEPS = 256           # steps enqueued per mc_train_slow_run call (one chunk of parameter draws)
SLOW_TRAIN_DEFAULTS = dict(lr=0.003, bs=128, mom=0.9, true1=1, false1=4, false2=10)   # main.lua:79-84
ACTIONS = ("train_tr", "train_all", "test_te", "test_all")
NET = common.NetShape(tsl.L1, tsl.FM, tsl.L2, tsl.NH2, tsl.NPARAMS, "libmctrainslow.so")
# include/mc_train_slow.h's order: w1 b1 .. w4 b4 fw1 fb1 .. fw5 fb5, 18 tensors
conv_shapes, fc_shapes, flat_params, unflat_params = NET.conv_shapes, NET.fc_shapes, NET.flat_params, NET.unflat_params
tensor_names, init_net = NET.tensor_names, NET.init_net


class Trainer(KittiTrainer):
    """Device state of a training run: images, nnz, permutation, parameters, momenta, workspace."""
    LIB, WHO, SHAPE = tsl, "train_slow", NET

    def run(self, t0, prm, lr, mom, losses):
        """mc_train_slow_run: prm (n_steps, n_pairs, 18) on the device; losses (>= n_steps) device float32."""
        self.call("run", _p(self.x0), _p(self.x1), self.n_img, self.H, self.W, _p(self.nnz), self.nnz.shape[0], _p(self.perm),
                  self.perm.shape[0], t0, prm.shape[0], self.n_pairs, _p(prm), _p(self.params), _p(self.moms), lr, mom, _p(losses))


def step_batch(patches, params, moms, lr, mom, workspace=None):
    """mc_train_slow_step_batch: one SGD step on patches (n_pairs, 3, 9, 9); params / moms (870449,) updated in place.
    Returns the device scalar of the batch's loss."""
    return common.step_batch(tsl, "train_slow", patches, params, moms, (lr, mom), workspace)


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
    opt_t = {k: v for k, v in sorted(vars(opt).items()) if isinstance(v, (bool, int, float, str)) and k not in ("fc_mode", "conv_mode")}   # -fc_mode / -conv_mode are how a run predicts, not the net's
    d = os.path.dirname(fname)
    if d:
        os.makedirs(d, exist_ok=True)
    t7.save(fname, [net_te, net_te2, opt_t])
    return fname


def parse(argv):
    """The flags of `main.lua {kitti|kitti2015} slow -a train_tr|train_all|test_te|test_all`: main.parse's
    hyper-parameter and augmentation flags, with arch slow's optimiser values (main.lua:79-84) and no -m / -pow.
    Returns (dataset, "slow", opt, prm) as main.parse does."""
    from .params import TABLES
    if len(argv) < 2 or argv[0] not in ("kitti", "kitti2015") or argv[1] != "slow":
        raise SystemExit("train_slow: training and testing of arch slow cover {kitti|kitti2015} slow -a %s "
                         "(mb slow's l1 5 / l2 3 net trains through train_mb_slow.parse, mb fast through train_mb.parse; -a submit is out of scope)" % " | ".join(ACTIONS))
    common.refuse_net_flags(argv, "train_slow")
    dataset = argv[0]
    t = TABLES[(dataset, "slow")]
    ap = common.new_parser(dataset, "slow", t, SLOW_TRAIN_DEFAULTS)
    ap.add_argument("-a", required=True)
    ap.add_argument("-disp_max", type=int, default=228)
    ap.add_argument("-data_dir", default="", help="default data.kitti / data.kitti2015 (main.lua:427-445)")
    ap.add_argument("-at", type=int, default=0, choices=(0, 1), help="1: KITTI 2012 and 2015 together (main.lua:403-426)")
    common.add_fc_flags(ap, dataset)  # -l2 other than 4 trains through train_slow_depth.py: main.route
    common.add_fc_mode_flag(ap)       # the test_te / test_all it runs, the one after train_tr included (main.main's run)
    common.add_conv_mode_flag(ap)     # likewise, the feature net's convolutions
    opt = ap.parse_args(argv[2:])
    common.check_conv_mode(opt, "slow", "train_slow")
    common.check_fc_flags(opt, "train_slow")
    if opt.a not in ACTIONS:
        raise SystemExit("train_slow: -a %s is not supported for %s slow; training and testing cover -a %s (-a submit is out "
                         "of scope)" % (opt.a, dataset, " | ".join(ACTIONS)))
    if opt.at == 1 and opt.data_dir:
        raise SystemExit("main.py: -at 1 reads data.kitti and data.kitti2015 together (main.lua:403-426) and takes no -data_dir")
    common.check_bs(opt, "train_slow", "main.lua:787")
    return dataset, "slow", opt, common.pipeline_prm(t, opt)


last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def train(dataset, opt, argv, device, data=None, init=None):
    """main.lua:602-890 for arch slow, -a train_tr / train_all: returns the saved net's file name.  init:
    (conv_layers, fc_layers) to start from instead of init_net(opt.seed)."""
    global last_run
    if data is None:
        data = load_data(dataset, opt)
    nnz, rng, perm = training_rows(opt, data)
    n_pairs = opt.bs // 2
    conv_layers, fc_layers = init if init is not None else init_net(opt.seed)
    tr = Trainer(data["x0"], data["x1"], nnz, perm, conv_layers, fc_layers, n_pairs, device)
    losses, epochs = run_epochs(tr, rng, opt, n_steps_per_epoch(nnz.shape[0], opt.bs), n_pairs, device, CHUNK_STEPS,
                                lambda s0, prm, lr, out: tr.run(s0 * n_pairs, prm, lr, opt.mom, out))
    conv_layers, fc_layers = tr.nets()
    fname = save_net(net_fname_of(dataset, "slow", argv), conv_layers, fc_layers, opt)
    last_run = {"net_fname": fname, "losses": losses, "epochs": epochs}
    return fname
