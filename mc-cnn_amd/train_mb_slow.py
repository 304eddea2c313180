"""`main.lua mb slow -a train_tr | train_all | test_te` (main.lua:116-130, 455-490, 602-890, 1121-1131, 1183-1238) on the
MI355X.

Middlebury's accurate net is `-l1 5 -fm 112 -l2 3 -nh2 384` (main.lua:116-130): five valid 3x3 convolutions
1 -> 112 -> 112 -> 112 -> 112 -> 112 on 11 x 11 patches with ReLU after every one, Reshape(bs, 224), Linear
224 -> 384 -> 384 -> 384 -> 1 with ReLUs, Sigmoid, BCECriterion2.  It is trained by libmctrainmbslow.so
(include/mc_train_mb_slow.h): ten kernels a step, the towers one workgroup per PATCH (a pair's 221 KB of activations do not
fit a CU's LDS, one patch's 74 KB do), enqueued chunk by chunk through `mc_train_mb_slow_run`.

Nothing here is new but the net's shapes: the flags (`parse_mb`), the ragged store and its Trainer base, the loader, the
source draws and `test_te` are train_mb.py's (`MbTrainer`, `load_mb_data`, `build_store`, `device_table`, `chunk_sources`,
`data_dir_of`, `evaluate`); the augmentation draws, the epoch loop, the parameter layout (`NetShape`) and `step_batch` are
train_common.py's, shared by all four nets; the saved net is train_slow.py's (`save_net`, generic in the layer count).
`init_net` has the ranges of nn.SpatialConvolution:reset and nn.Linear:reset; as for the KITTI accurate net, small synthetic
sets keep the net on the ln 2 plateau from there, and `train(..., init=(conv, fc))` starts from given nets instead.

Not covered: -color rgb, -subset, -debug, -a submit, -a test_all (main.lua:1136 asserts it away itself), multi-GPU training.
"""
from . import _train_mb_slow_lib as tmsl
from . import train_common as common
from .train import net_fname_of
from .train_common import _p, draw_params, n_steps_per_epoch, run_epochs, training_rows  # noqa: F401
from .train_mb import (ACTIONS, MbTrainer, build_store, chunk_sources, data_dir_of, device_table, draw_sources, evaluate,  # noqa: F401
                       load_mb_data, parse_mb)
from .train_slow import save_net

CHUNK_STEPS = 256           # steps enqueued per mc_train_mb_slow_run call (one chunk of parameter and source draws)
MB_SLOW_TRAIN_DEFAULTS = dict(lr=0.003, bs=128, mom=0.9, true1=0.5, false1=1.5, false2=18.0, d_exp=0.2,
                              d_light=0.2)   # main.lua:116-130
NET = common.NetShape(tmsl.L1, tmsl.FM, tmsl.L2, tmsl.NH2, tmsl.NPARAMS, "libmctrainmbslow.so")
# include/mc_train_mb_slow.h's order: w1 b1 .. w5 b5 fw1 fb1 .. fw4 fb4, 18 tensors
conv_shapes, fc_shapes, flat_params, unflat_params = NET.conv_shapes, NET.fc_shapes, NET.flat_params, NET.unflat_params
tensor_names, init_net = NET.tensor_names, NET.init_net


def parse(argv):
    """`main.lua mb slow -a train_tr | train_all | test_te`: train_mb.parse_mb with arch slow's optimiser values
    (main.lua:116-130) and no -m / -pow."""
    if len(argv) < 2 or argv[0] != "mb" or argv[1] != "slow":
        raise SystemExit("train_mb_slow: training and testing of Middlebury's accurate net cover mb slow -a %s (mb fast trains "
                         "through train_mb.parse, {kitti|kitti2015} slow through train_slow.parse)" % " | ".join(ACTIONS))
    return parse_mb(argv, "slow", MB_SLOW_TRAIN_DEFAULTS, "train_mb_slow")


# ---- the device side -----------------------------------------------------------------------------------------------------
class Trainer(MbTrainer):
    """Device state of a training run: planes, table, nnz, permutation, parameters, momenta, workspace."""
    LIB, WHO, SHAPE = tmsl, "train_mb_slow", NET

    def run(self, t0, src, prm, lr, mom, losses):
        """mc_train_mb_slow_run: src (n_steps, n_pairs, 2) int32 and prm (n_steps, n_pairs, 18) on the device; losses
        (>= n_steps) device float32."""
        n_steps = prm.shape[0]
        assert tuple(src.shape) == (n_steps, self.n_pairs, 2) and tuple(prm.shape) == (n_steps, self.n_pairs, tmsl.NPRM)
        self.call("run", _p(self.planes), _p(self.table), self.table.shape[0], _p(self.nnz), self.nnz.shape[0], _p(self.perm),
                  self.perm.shape[0], t0, n_steps, self.n_pairs, _p(src), _p(prm), _p(self.params), _p(self.moms), lr, mom,
                  _p(losses))


def step_batch(patches, params, moms, lr, mom, workspace=None):
    """mc_train_mb_slow_step_batch: one SGD step on patches (n_pairs, 3, 11, 11); params / moms (835617,) updated in place.
    Returns the device scalar of the batch's loss."""
    return common.step_batch(tmsl, "train_mb_slow", patches, params, moms, (lr, mom), workspace)


# ---- training ------------------------------------------------------------------------------------------------------------
last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def train(opt, argv, device, data=None, init=None):
    """main.lua:602-890 for mb slow, -a train_tr / train_all: returns the saved net's file name.  init:
    (conv_layers, fc_layers) to start from instead of init_net(opt.seed).  Every chunk's sources are drawn after its
    augmentation parameters, as in train_mb.train."""
    global last_run
    if data is None:
        data = load_mb_data(data_dir_of(opt), opt.a)
    nnz, rng, perm = training_rows(opt, data)
    n_pairs = opt.bs // 2
    src_of = chunk_sources(rng, opt, nnz, perm, data["index"], n_pairs, device)
    conv_layers, fc_layers = init if init is not None else init_net(opt.seed)
    tr = Trainer(data["planes"], data["table"], nnz, perm, conv_layers, fc_layers, n_pairs, device)
    losses, epochs = run_epochs(tr, rng, opt, n_steps_per_epoch(nnz.shape[0], opt.bs), n_pairs, device, CHUNK_STEPS,
                                lambda s0, prm, lr, out: tr.run(s0 * n_pairs, src_of(s0, prm.shape[0]), prm, lr, opt.mom, out))
    conv_layers, fc_layers = tr.nets()
    fname = save_net(net_fname_of("mb", "slow", argv), conv_layers, fc_layers, opt)
    last_run = {"net_fname": fname, "losses": losses, "epochs": epochs}
    return fname
