"""`main.lua {kitti|kitti2015|mb} slow -a train_tr | train_all -l2 N` for N = 1..7 (main.lua:73-78, 120-124, 663-695) on the
MI355X: the accurate net with another number of hidden Linears than its data set's.

The reference builds the accurate net from -l1, -fm, -l2 (hidden Linears) and -nh2 (their units).  libmctrainslow.so is that net
at -l2 4 on KITTI's tower and libmctrainmbslow.so at -l2 3 on Middlebury's; libmctrainslowdepth.so
(include/mc_train_slow_depth.h) runs the same step with l2 as an argument, 1..7, on either tower.  -nh2 stays 384 (prediction's
mc_fc_stack and mc_fc_split_stack are 384 wide), and -l1 / -fm keep the data set's: see DESIGN.md 9.7.

Everything but the depth is the parents': the data, the stores and `run`'s argument lists (train_slow.py, train_mb_slow.py), the
draws and the epoch loop (train_common.py), the saved net (`train_slow.save_net`, whose net_te2 carries the depth) and the
evaluation.  The order of draws from the ONE Generator(-seed) is train_slow.train's and train_mb_slow.train's -- permutation,
then on Middlebury the sources' generator state, then per chunk the augmentation parameters and the sources -- so a -seed picks
the same pixels and augmentations at every depth.  The initial net is the parents' `init_net` rule at the new shape.  main.py
routes here when -l2 differs from the data set's; with the default it keeps the libraries above.
"""
from . import _train_slow_depth_lib as tsdl
from . import train_common as common
from . import train_mb_slow, train_slow
from .train import net_fname_of
from .train_common import _p, n_steps_per_epoch, run_epochs, training_rows
from .train_slow import save_net  # noqa: F401

CHUNK_STEPS = 256           # steps enqueued per run call (one chunk of parameter and source draws), as the parents'
L2_RANGE = (tsdl.MIN_L2, tsdl.MAX_L2)


def net_shape(dataset, l2):
    """The flat parameter layout of the accurate net of `dataset`'s tower with l2 hidden Linears; at the data set's own depth
    train_slow.NET's (kitti, kitti2015: 4) and train_mb_slow.NET's (mb: 3) with another library's name."""
    if dataset not in tsdl.STORE_OF:
        raise ValueError("train_slow_depth: data set %r: libmctrainslowdepth.so trains %s" % (dataset, " | ".join(tsdl.STORE_OF)))
    if not L2_RANGE[0] <= l2 <= L2_RANGE[1]:
        raise ValueError("train_slow_depth: -l2 %d: libmctrainslowdepth.so trains l2 %d..%d" % ((l2,) + L2_RANGE))
    store = tsdl.STORE_OF[dataset]
    tower = tsdl.TOWERS[store]
    return common.NetShape(tower.L1, tower.FM, l2, tsdl.NH2, tsdl.nparams_of(store, l2), "libmctrainslowdepth.so")


def _depth_of(fc_layers):
    return len(fc_layers) - 1


class Trainer(train_slow.Trainer):
    """train_slow.Trainer on libmctrainslowdepth.so at the depth of `fc_layers`: `run` is mc_train_slow_depth_run with l2 first."""
    WHO = "train_slow_depth"

    def __init__(self, x0, x1, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        self.LIB, self.SHAPE = tsdl.at_depth(tsdl.KITTI, _depth_of(fc_layers)), net_shape("kitti", _depth_of(fc_layers))
        super().__init__(x0, x1, nnz, perm, conv_layers, fc_layers, n_pairs, device)


class MbTrainer(train_mb_slow.Trainer):
    """train_mb_slow.Trainer on libmctrainslowdepth.so at the depth of `fc_layers`: `run` is mc_train_slow_depth_mb_run with l2
    first."""
    WHO = "train_slow_depth"

    def __init__(self, planes, table, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        self.LIB, self.SHAPE = tsdl.at_depth(tsdl.MB, _depth_of(fc_layers)), net_shape("mb", _depth_of(fc_layers))
        super().__init__(planes, table, nnz, perm, conv_layers, fc_layers, n_pairs, device)

    def run(self, t0, src, prm, lr, mom, losses):
        n_steps = prm.shape[0]
        assert tuple(src.shape) == (n_steps, self.n_pairs, 2) and tuple(prm.shape) == (n_steps, self.n_pairs, tsdl.NPRM)
        self.call("mb_run", _p(self.planes), _p(self.table), self.table.shape[0], _p(self.nnz), self.nnz.shape[0], _p(self.perm),
                  self.perm.shape[0], t0, n_steps, self.n_pairs, _p(src), _p(prm), _p(self.params), _p(self.moms), lr, mom,
                  _p(losses))


def step_batch(dataset, l2, patches, params, moms, lr, mom, workspace=None):
    """mc_train_slow_depth_step_batch: one SGD step on patches (n_pairs, 3, ws, ws) of `dataset`'s tower (ws 9 or 11) at depth
    l2; params / moms updated in place.  Returns the device scalar of the batch's loss."""
    return common.step_batch(tsdl.at_depth(tsdl.STORE_OF[dataset], l2), "train_slow_depth", patches, params, moms, (lr, mom), workspace)


last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def train(dataset, opt, argv, device, data=None, init=None):
    """train_slow.train (kitti, kitti2015) or train_mb_slow.train (mb) with opt.l2 hidden Linears: returns the saved net's file
    name.  init: (conv_layers, fc_layers) to start from instead of net_shape(dataset, opt.l2).init_net(opt.seed)."""
    global last_run
    shape = net_shape(dataset, opt.l2)
    mb = dataset == "mb"
    if data is None:
        data = train_mb_slow.load_mb_data(train_mb_slow.data_dir_of(opt), opt.a) if mb else train_slow.load_data(dataset, opt)
    nnz, rng, perm = training_rows(opt, data)
    n_pairs = opt.bs // 2
    if mb:
        src_of = train_mb_slow.chunk_sources(rng, opt, nnz, perm, data["index"], n_pairs, device)
    conv_layers, fc_layers = init if init is not None else shape.init_net(opt.seed)
    if _depth_of(fc_layers) != opt.l2:
        raise ValueError("train_slow_depth: a net of %d hidden Linears for -l2 %d" % (_depth_of(fc_layers), opt.l2))
    if mb:
        tr = MbTrainer(data["planes"], data["table"], nnz, perm, conv_layers, fc_layers, n_pairs, device)
        run_chunk = lambda s0, prm, lr, out: tr.run(s0 * n_pairs, src_of(s0, prm.shape[0]), prm, lr, opt.mom, out)  # noqa: E731
    else:
        tr = Trainer(data["x0"], data["x1"], nnz, perm, conv_layers, fc_layers, n_pairs, device)
        run_chunk = lambda s0, prm, lr, out: tr.run(s0 * n_pairs, prm, lr, opt.mom, out)  # noqa: E731
    losses, epochs = run_epochs(tr, rng, opt, n_steps_per_epoch(nnz.shape[0], opt.bs), n_pairs, device, CHUNK_STEPS, run_chunk)
    conv_layers, fc_layers = tr.nets()
    fname = save_net(net_fname_of(dataset, "slow", argv), conv_layers, fc_layers, opt)
    last_run = {"net_fname": fname, "losses": losses, "epochs": epochs}
    return fname
