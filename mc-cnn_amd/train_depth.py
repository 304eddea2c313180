"""`main.lua {kitti|kitti2015|mb} fast -a train_tr | train_all -l1 N` for N = 1..5 (main.lua:212-214, 240-242, 271-273, 726-746)
on the MI355X: the fast net at a depth other than its data set's default.

The reference builds the fast net from -l1 (3x3 convolutions), -fm (feature maps) and -ks (kernel size).  libmctrain.so is that
net at -l1 4 and libmctrainmb.so at -l1 5; libmctraindepth.so (include/mc_train_depth.h) holds the same step instantiated for
-l1 1..5 on patches of side 2 l1 + 1, for KITTI's image store and for Middlebury's ragged one.  -fm stays 64 and -ks 3: see
DESIGN.md 9.6 for what the GEMMs would need.  l1 = 6 does not fit a CU's LDS.

Everything but the depth is the other trainers': the data, the stores and `run`'s argument lists (train.py, train_mb.py), the
draws and the epoch loop (train_common.py), the saved net and the evaluation.  The order of draws from the ONE Generator(-seed) is
train.train's and train_mb.train's -- permutation, then per chunk the augmentation parameters, then on Middlebury the sources --
so a -seed picks the same pixels and augmentations at every depth.  The initial net is `load_net("random:<seed>")` with l1
layers.  main.py routes here when -l1 differs from the data set's default; with the default it keeps the libraries above.
"""
from . import _train_depth_lib as tdl
from . import train as train_kitti, train_common as common, train_mb
from .params import NET_SHAPES
from .train import net_fname_of, save_net  # noqa: F401
from .train_common import _p, _stream, n_steps_per_epoch, run_epochs, training_rows

CHUNK_STEPS = 256           # steps enqueued per run call (one chunk of parameter and source draws), as train.py's
L1_RANGE = (tdl.MIN_L1, tdl.MAX_L1)


def net_shape(l1):
    """The flat parameter layout of the fast net of depth l1 (w1 b1 .. w_l1 b_l1); at 4 and 5 train.NET's and train_mb.NET's."""
    if not L1_RANGE[0] <= l1 <= L1_RANGE[1]:
        raise ValueError("train_depth: -l1 %d: libmctraindepth.so trains l1 %d..%d" % ((l1,) + L1_RANGE))
    return common.NetShape(l1, tdl.FM, 0, 0, tdl.nparams_of(l1), "libmctraindepth.so")


class Trainer(train_kitti.Trainer):
    """train.Trainer on libmctraindepth.so at the depth of `layers`: `run` is mc_train_depth_run with l1 first."""
    WHO = "train_depth"

    def __init__(self, x0, x1, nnz, perm, layers, n_pairs, device):
        self.LIB, self.SHAPE = tdl.at_depth(len(layers)), net_shape(len(layers))
        super().__init__(x0, x1, nnz, perm, layers, n_pairs, device)


class MbTrainer(train_mb.Trainer):
    """train_mb.Trainer on libmctraindepth.so at the depth of `layers`: `run` is mc_train_depth_mb_run with l1 first."""
    WHO = "train_depth"

    def __init__(self, planes, table, nnz, perm, layers, n_pairs, device):
        self.LIB, self.SHAPE = tdl.at_depth(len(layers)), net_shape(len(layers))
        super().__init__(planes, table, nnz, perm, layers, n_pairs, device)

    def run(self, t0, src, prm, lr, mom, margin, pow_, losses):
        n_steps = prm.shape[0]
        assert tuple(src.shape) == (n_steps, self.n_pairs, 2) and tuple(prm.shape) == (n_steps, self.n_pairs, tdl.NPRM)
        self.call("mb_run", _p(self.planes), _p(self.table), self.table.shape[0], _p(self.nnz), self.nnz.shape[0], _p(self.perm),
                  self.perm.shape[0], t0, n_steps, self.n_pairs, _p(src), _p(prm), _p(self.params), _p(self.moms), lr, mom, margin,
                  pow_, _p(losses))


def sample(l1, x0, x1, nnz, rows, prm):
    """mc_train_depth_sample: train.sample's arguments -> (n_pairs, 3, ws, ws) with ws = 2 l1 + 1."""
    import torch
    n_img, H, W = x0.shape
    out = torch.empty((rows.shape[0], 3, tdl.ws_of(l1), tdl.ws_of(l1)), dtype=torch.float32, device=x0.device)
    tdl.check(tdl.load().mc_train_depth_sample(l1, _p(x0), _p(x1), n_img, H, W, _p(nnz), nnz.shape[0], _p(rows), _p(prm), rows.shape[0],
                                               _p(out), _stream()), "mc_train_depth_sample")
    return out


def mb_sample(l1, planes, table, nnz, rows, src, prm):
    """mc_train_depth_mb_sample: train_mb.sample's arguments -> (n_pairs, 3, ws, ws)."""
    import torch
    out = torch.empty((rows.shape[0], 3, tdl.ws_of(l1), tdl.ws_of(l1)), dtype=torch.float32, device=planes.device)
    tdl.check(tdl.load().mc_train_depth_mb_sample(l1, _p(planes), _p(table), table.shape[0], _p(nnz), nnz.shape[0], _p(rows), _p(src),
                                                  _p(prm), rows.shape[0], _p(out), _stream()), "mc_train_depth_mb_sample")
    return out


def step_batch(l1, patches, params, moms, lr, mom, margin, pow_, workspace=None):
    """mc_train_depth_step_batch: one SGD step on patches (n_pairs, 3, ws, ws); params / moms updated in place.  Returns the
    device scalar of the batch's mean loss."""
    return common.step_batch(tdl.at_depth(l1), "train_depth", patches, params, moms, (lr, mom, margin, pow_), workspace)


last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def train(dataset, arch, opt, argv, device, data=None):
    """train.train (kitti, kitti2015) or train_mb.train (mb) with a net of opt.l1 layers: returns the saved net's file name."""
    global last_run
    from .main import load_net
    if arch != "fast":
        raise SystemExit("train_depth: -l1 builds the fast net only; arch %s keeps its data set's l1 %d" % (arch, NET_SHAPES[(dataset, arch)][0]))
    mb = dataset == "mb"
    if data is None:
        data = train_mb.load_mb_data(train_mb.data_dir_of(opt), opt.a) if mb else train_kitti.load_data(dataset, opt)
    nnz, rng, perm = training_rows(opt, data)
    n_pairs = opt.bs // 2
    net = load_net("random:%d" % opt.seed, dataset, arch, l1=opt.l1)
    if mb:
        src_of = train_mb.chunk_sources(rng, opt, nnz, perm, data["index"], n_pairs, device)
        tr = MbTrainer(data["planes"], data["table"], nnz, perm, net, n_pairs, device)
        run_chunk = lambda s0, prm, lr, out: tr.run(s0 * n_pairs, src_of(s0, prm.shape[0]), prm, lr, opt.mom, opt.m, opt.pow, out)  # noqa: E731
    else:
        tr = Trainer(data["x0"], data["x1"], nnz, perm, net, n_pairs, device)
        run_chunk = lambda s0, prm, lr, out: tr.run(s0 * n_pairs, prm, lr, opt.mom, opt.m, opt.pow, out)  # noqa: E731
    losses, epochs = run_epochs(tr, rng, opt, n_steps_per_epoch(nnz.shape[0], opt.bs), n_pairs, device, CHUNK_STEPS, run_chunk)
    fname = save_net(net_fname_of(dataset, arch, argv), tr.layers(), opt)
    last_run = {"net_fname": fname, "losses": losses, "epochs": epochs}
    return fname
