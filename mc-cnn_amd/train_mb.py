"""`main.lua mb fast -a train_tr | train_all | test_te` (main.lua:455-490, 602-890, 1121-1131, 1183-1238) on the MI355X.

Middlebury's fast net is `-l1 5 -fm 64` (main.lua:271-272): five valid 3x3 convolutions on 11 x 11 patches, trained by
libmctrainmb.so (include/mc_train_mb.h) in two kernels a step, enqueued chunk by chunk through `mc_train_mb_run`.  The
flags' common blocks, the augmentation draws, the permutation, the epoch loop, the parameter layout and `step_batch` are
train_common.py's, shared by all four nets; the saved net and the error measure are train.py's (`net_fname_of`, `save_net`,
`error_rate`).

What is Middlebury's own:
  * the image store is ragged: `x_<n>_<light>.bin` holds (n_exp, 2, 1, H_n, W_n) for light >= 2, every image with its own
    size, number of lights and number of exposures (preprocess_mb.py).  `build_store` lays every (light, exposure, view)
    plane into ONE flat float32 buffer with a table (offset, H, W) per plane and an index (first plane, lights, exposures)
    per image;
  * the left patch of a pair comes from X[img][light][exp, 1], the right ones from X[img][light_][exp_, 2], where exp_ is
    redrawn with probability -d_exp and light_ = max(2, light - 1) with probability -d_light (main.lua:828-841):
    `draw_sources` draws them, vectorised per chunk, and resolves them to the two plane ids of each pair (`chunk_sources`:
    after the chunk's augmentation parameters, from the same Generator);
  * `test_te` predicts (te[i], 2) for every te, then (5, 3) and (5, 4), from light 1 of each image with that image's own
    disp_max (meta.bin), direction -1 only, err_at 1.

The draws are the reference's distributions from one numpy Generator(-seed), not Torch's Mersenne-Twister stream (see
train.py).  `preprocess_mb.py` is not part of this project: `-data_dir` (default data.mb.<rect>_<color>) has to hold its
output.  `mb slow` trains through train_mb_slow.py, which shares this module's flags (`parse_mb`), data, store
(`MbTrainer`), source draws and `evaluate`.  Not covered: -color rgb, -a submit, -a test_all (main.lua:1136 asserts it
away itself), -subset, -debug.
"""
import os
import time

import numpy as np

from . import _train_mb_lib as tml
from . import train_common as common
from .binio import fromfile
from .train import error_rate, net_fname_of, save_net
from .train_common import _p, _stream, draw_params, n_steps_per_epoch, run_epochs, training_rows  # noqa: F401

CHUNK_STEPS = 256           # steps enqueued per mc_train_mb_run call (one chunk of parameter and source draws)
ACTIONS = ("train_tr", "train_all", "test_te")
MB_TRAIN_DEFAULTS = dict(m=0.2, pow=1, lr=0.002, bs=128, mom=0.9, true1=0.5, false1=1.5, false2=6.0, d_exp=0.2,
                         d_light=0.2)   # main.lua:264-279
PLANE_DTYPE = np.dtype([("offset", "<i8"), ("H", "<i4"), ("W", "<i4")])   # mc_train_mb_plane


def parse_mb(argv, arch, train_defaults, who):
    """The flags of `main.lua mb <arch> -a train_tr | train_all | test_te` with main.lua's names and defaults, for
    train_mb.parse (who = "train_mb") and train_mb_slow.parse.  Returns (dataset, arch, opt, prm) as main.parse does; prm has
    left_only = 1 (outside -a predict dataset mb runs direction -1 only, main.lua:953-955)."""
    from .params import TABLES
    t = TABLES[("mb", arch)]
    ap = common.new_parser("mb", arch, t, train_defaults)
    ap.add_argument("-a", required=True)
    ap.add_argument("-ds", type=int, default=2001, help="parsed and ignored: main.lua declares it (267 for arch fast) and never reads it")
    ap.add_argument("-rect", default="imperfect", help="main.lua:68")
    ap.add_argument("-color", default="gray", help="main.lua:69")
    ap.add_argument("-data_dir", default="", help="default data.mb.<rect>_<color> (main.lua:456)")
    ap.add_argument("-subset", type=float, default=1.0, help="main.lua:28; only 1 is supported")
    ap.add_argument("-debug", action="store_true", help="main.lua:18; not supported")
    common.add_fc_mode_flag(ap)       # arch slow: the test_te it runs, the one after train_tr included (main.main's run)
    common.add_conv_mode_flag(ap)     # either arch: the feature net's convolutions in that test_te
    common.refuse_net_flags(argv, who)
    common.refuse_fc_flags(argv, who)
    if arch == "fast":
        common.add_net_flags(ap, "mb", arch)       # -l1 other than 5 trains through train_depth.py: main.route
    if arch == "slow":
        common.add_fc_flags(ap, "mb")              # -l2 other than 3 trains through train_slow_depth.py: main.route
    opt = ap.parse_args(argv[2:])
    if arch == "fast":
        common.check_net_flags(opt, who)
    if arch == "slow":
        common.check_fc_flags(opt, who)
    common.check_fc_mode(opt, arch, who)
    common.check_conv_mode(opt, arch, who)
    if opt.a == "test_all":
        raise SystemExit("%s: -a test_all is not supported on Middlebury (main.lua:1136 asserts the same)" % who)
    if opt.a == "submit":
        raise SystemExit("%s: -a submit is out of scope (it writes the Middlebury evaluation's PFM files)" % who)
    if opt.a not in ACTIONS:
        raise SystemExit("%s: -a %s is not a training or testing action; mb %s covers -a %s" % (who, opt.a, arch, " | ".join(ACTIONS)))
    if opt.color != "gray":
        raise SystemExit("%s: -color %s: the nets here have one input plane, only -color gray is supported" % (who, opt.color))
    if opt.subset != 1:
        raise SystemExit("%s: -subset %g is not supported (the whole training set is used)" % (who, opt.subset))
    if opt.debug:
        raise SystemExit("%s: -debug (main.lua:1240-1260 writes images of every prediction) is not supported" % who)
    common.check_bs(opt, who, "main.lua:789")
    prm = common.pipeline_prm(t, opt)
    prm["left_only"] = 1
    return "mb", arch, opt, prm


def parse(argv):
    """`main.lua mb fast -a train_tr | train_all | test_te`: parse_mb with the fast net's optimiser values."""
    if len(argv) >= 2 and argv[0] == "mb" and argv[1] == "slow":
        raise SystemExit("train_mb: mb slow is not trained here: its net (l1 5, fm 112, l2 3) keeps 221 KB of activations per "
                         "pair, more than the one-workgroup-per-pair step of libmctrainmb.so can hold in a CU's LDS; "
                         "train_mb_slow.parse takes these command lines (libmctrainmbslow.so, one workgroup per patch)")
    if len(argv) < 2 or argv[0] != "mb" or argv[1] != "fast":
        raise SystemExit("train_mb: training and testing on Middlebury cover mb fast -a %s" % " | ".join(ACTIONS))
    return parse_mb(argv, "fast", MB_TRAIN_DEFAULTS, "train_mb")


def data_dir_of(opt):
    return opt.data_dir or "data.mb.%s_%s" % (opt.rect, opt.color)


# ---- the data ----------------------------------------------------------------------------------------------------------
def build_store(X, need=()):
    """X[img][light] (light 1 first) -> (planes, table, index): every (light >= 2, exposure, view) plane of every image in
    one flat float32 buffer; table[id] = (offset in floats, H, W) (PLANE_DTYPE); index[img] = (first plane id, number of
    lights >= 2, number of exposures).  The plane of (light, exp, view), 0-based with light 0 = the file's light 2, is
    first + ((light * n_exp) + exp) * 2 + view.  need: 1-based image numbers that must have a light >= 2.
    Raises ValueError, naming the image, where an image's lights differ in exposures or size (exp_ is drawn from light's
    count and used on light_, main.lua:834-840) or a plane is outside the sampler's limits."""
    index = np.zeros((len(X), 3), np.int64)
    recs, total = [], 0
    for n, lights in enumerate(X, 1):
        tr = [np.asarray(a) for a in lights[1:]]
        index[n - 1, 0] = len(recs)
        if not tr:
            if n in need:
                raise ValueError("image %d is listed in the training nnz but has no x_%d_2.bin (no light >= 2)" % (n, n))
            continue
        for k, a in enumerate(tr, 2):
            if a.ndim != 5 or a.shape[1] != 2 or a.shape[2] != 1 or a.shape[0] < 1:
                raise ValueError("image %d: x_%d_%d.bin has shape %s, not (n_exp, 2, 1, H, W)" % (n, n, k, a.shape))
            if a.shape != tr[0].shape:
                raise ValueError("image %d: light %d is %s but light 2 is %s: the lights of an image must agree in exposures "
                                 "and size" % (n, k, a.shape, tr[0].shape))
        n_exp, H, W = tr[0].shape[0], tr[0].shape[3], tr[0].shape[4]
        if not (tml.MIN_SIDE <= H <= tml.MAX_SIDE and tml.MIN_SIDE <= W <= tml.MAX_SIDE):
            raise ValueError("image %d: planes of %d x %d are outside the sampler's range [%d, %d]" % (n, H, W, tml.MIN_SIDE, tml.MAX_SIDE))
        index[n - 1, 1:] = (len(tr), n_exp)
        for _ in range(len(tr) * n_exp * 2):
            recs.append((total, H, W))
            total += H * W
    planes = np.empty(total, np.float32)
    for n, lights in enumerate(X, 1):
        o = recs[index[n - 1, 0]][0] if index[n - 1, 1] else 0
        for a in lights[1:]:
            a = np.asarray(a, np.float32)
            planes[o:o + a.size] = a.ravel()
            o += a.size
    return planes, np.array(recs, PLANE_DTYPE).reshape(-1), index


def load_mb_data(data_dir, action):
    """main.lua:455-490: te, meta (H, W, ndisp per image), nnz_tr, nnz_te, X[img] = [x_<n>_1, x_<n>_2, ...] up to the first
    missing light (light 1 only for test_te), dispnoc {image number: map}; for the training actions also the store
    (planes, table, index) of build_store.  The reference appends the dispnoc files it finds to a list and indexes it by
    image number, which is the same thing for preprocess_mb.py's sets, whose images with ground truth come first."""
    f = lambda name: fromfile(os.path.join(data_dir, name))
    d = dict(te=np.asarray(f("te.bin")).ravel().astype(np.int64), meta=np.asarray(f("meta.bin")).reshape(-1, 3),
             nnz_tr=np.asarray(f("nnz_tr.bin"), np.float32).reshape(-1, 4), nnz_te=np.asarray(f("nnz_te.bin"), np.float32).reshape(-1, 4))
    X, dispnoc = [], {}
    for n in range(1, d["meta"].shape[0] + 1):
        lights, light = [], 1
        while os.path.exists(os.path.join(data_dir, "x_%d_%d.bin" % (n, light))):
            lights.append(f("x_%d_%d.bin" % (n, light)))
            light += 1
            if action == "test_te":
                break                      # main.lua:479-481: the training data is not needed
        X.append(lights)
        if os.path.exists(os.path.join(data_dir, "dispnoc%d.bin" % n)):
            dispnoc[n] = f("dispnoc%d.bin" % n)
    d["X"], d["dispnoc"] = X, dispnoc
    if action != "test_te":
        nnz = d["nnz_tr"] if action == "train_tr" else np.concatenate([d["nnz_tr"], d["nnz_te"]], 0)
        need = set(int(v) for v in np.unique(nnz[:, 0]))
        bad = [n for n in need if not 1 <= n <= len(X)]
        if bad:
            raise ValueError("%s: the nnz lists image %d, meta.bin has %d images" % (data_dir, bad[0], len(X)))
        try:
            d["planes"], d["table"], d["index"] = build_store(X, need)
        except ValueError as e:
            raise ValueError("%s: %s" % (data_dir, e)) from None
    return d


def draw_sources(rng, opt, img_ids, index):
    """main.lua:829-840 for pairs of images img_ids (1-based, any shape): light uniform over the image's lights >= 2, exp
    uniform over its exposures, exp_ = exp redrawn uniformly with probability d_exp, light_ = light or, with
    probability d_light, max(2, light - 1).  Returns the plane ids, int32 of shape img_ids.shape + (2,): [..., 0] the
    left view of (light, exp), [..., 1] the right view of (light_, exp_)."""
    img = np.asarray(img_ids).astype(np.int64) - 1
    first, n_light, n_exp = index[img, 0], index[img, 1], index[img, 2]
    if (n_light < 1).any():
        raise ValueError("draw_sources: image %d has no light >= 2" % (int(img[n_light < 1].ravel()[0]) + 1))
    light = rng.integers(0, n_light)           # 0 is the file's light 2
    exp = rng.integers(0, n_exp)
    exp_ = np.where(rng.uniform(0, 1, img.shape) < opt.d_exp, rng.integers(0, n_exp), exp)
    light_ = np.where(rng.uniform(0, 1, img.shape) < opt.d_light, np.maximum(0, light - 1), light)
    return np.stack([first + (light * n_exp + exp) * 2, first + (light_ * n_exp + exp_) * 2 + 1], -1).astype(np.int32)


# ---- the net's parameters ----------------------------------------------------------------------------------------------
NET = common.NetShape(tml.L1, tml.FM, 0, 0, tml.NPARAMS, "libmctrainmb.so")
flat_params = NET.flat_params     # [(w, b)] of the five-layer net -> one float32 vector in include/mc_train_mb.h's order (w1 b1 .. w5 b5)


def unflat_params(v):
    return NET.unflat_params(v)[0]


# ---- the device side -----------------------------------------------------------------------------------------------------
def device_table(table, device):
    """PLANE_DTYPE records -> the device tensor mc_train_mb_* take (two int64 words per record)."""
    import torch
    table = np.ascontiguousarray(table, PLANE_DTYPE)
    bad = (table["H"] < tml.MIN_SIDE) | (table["W"] < tml.MIN_SIDE) | (table["H"] > tml.MAX_SIDE) | (table["W"] > tml.MAX_SIDE)
    if bad.any():
        k = int(np.nonzero(bad)[0][0])
        raise ValueError("plane %d of %d x %d is outside the sampler's range [%d, %d]" % (k, table["H"][k], table["W"][k], tml.MIN_SIDE,
                                                                                         tml.MAX_SIDE))
    return torch.from_numpy(table.view(np.int64).reshape(-1, 2).copy()).to(device)


class MbTrainer(common.TrainerBase):
    """TrainerBase and Middlebury's image store: the flat planes and their device_table."""

    def __init__(self, planes, table, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        super().__init__(nnz, perm, conv_layers, fc_layers, n_pairs, device)
        self.table = device_table(table, device)
        self.planes = self.f32(planes)


class Trainer(MbTrainer):
    """Device state of a training run: planes, table, nnz, permutation, parameters, momenta, workspace."""
    LIB, WHO, SHAPE = tml, "train_mb", NET

    def __init__(self, planes, table, nnz, perm, layers, n_pairs, device):
        super().__init__(planes, table, nnz, perm, layers, (), n_pairs, device)

    def run(self, t0, src, prm, lr, mom, margin, pow_, losses):
        """mc_train_mb_run: src (n_steps, n_pairs, 2) int32 and prm (n_steps, n_pairs, 18) on the device; losses
        (>= n_steps) device float32."""
        n_steps = prm.shape[0]
        assert tuple(src.shape) == (n_steps, self.n_pairs, 2) and tuple(prm.shape) == (n_steps, self.n_pairs, tml.NPRM)
        self.call("run", _p(self.planes), _p(self.table), self.table.shape[0], _p(self.nnz), self.nnz.shape[0], _p(self.perm),
                  self.perm.shape[0], t0, n_steps, self.n_pairs, _p(src), _p(prm), _p(self.params), _p(self.moms), lr, mom, margin,
                  pow_, _p(losses))


def sample(planes, table, nnz, rows, src, prm):
    """mc_train_mb_sample on device tensors: planes (flat), table (device_table's), nnz (n, 4), rows (n_pairs,) int32,
    src (n_pairs, 2) int32, prm (n_pairs, 18) -> (n_pairs, 3, 11, 11): left, positive, negative patch of each pair."""
    import torch
    lib = tml.load()
    out = torch.empty((rows.shape[0], 3, tml.WS, tml.WS), dtype=torch.float32, device=planes.device)
    tml.check(lib.mc_train_mb_sample(_p(planes), _p(table), table.shape[0], _p(nnz), nnz.shape[0], _p(rows), _p(src), _p(prm),
                                     rows.shape[0], _p(out), _stream()), "mc_train_mb_sample")
    return out


def step_batch(patches, params, moms, lr, mom, margin, pow_, workspace=None):
    """mc_train_mb_step_batch: one SGD step on patches (n_pairs, 3, 11, 11); params / moms (148352,) updated in place.
    Returns the device scalar of the batch's mean loss."""
    return common.step_batch(tml, "train_mb", patches, params, moms, (lr, mom, margin, pow_), workspace)


# ---- training and testing ------------------------------------------------------------------------------------------------
last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def chunk_sources(rng, opt, nnz, perm, index, n_pairs, device):
    """src_of(s0, k): the sources of steps s0 .. s0 + k - 1 of an epoch, drawn from rng for the images of those steps' pairs
    in the permutation's order, as the (k, n_pairs, 2) int32 device tensor `run` takes."""
    import torch
    img_of = nnz[perm, 0].astype(np.int64)

    def src_of(s0, k):
        ids = img_of[s0 * n_pairs:(s0 + k) * n_pairs].reshape(k, n_pairs)
        return torch.from_numpy(draw_sources(rng, opt, ids, index)).to(device)
    return src_of


def train(opt, argv, device, data=None):
    """main.lua:602-890 for mb fast, -a train_tr / train_all: returns the saved net's file name.  Every chunk's sources are
    drawn after its augmentation parameters."""
    global last_run
    from .main import load_net
    if data is None:
        data = load_mb_data(data_dir_of(opt), opt.a)
    nnz, rng, perm = training_rows(opt, data)
    n_pairs = opt.bs // 2
    src_of = chunk_sources(rng, opt, nnz, perm, data["index"], n_pairs, device)
    tr = Trainer(data["planes"], data["table"], nnz, perm, load_net("random:%d" % opt.seed, "mb", "fast"), n_pairs, device)
    losses, epochs = run_epochs(tr, rng, opt, n_steps_per_epoch(nnz.shape[0], opt.bs), n_pairs, device, CHUNK_STEPS,
                                lambda s0, prm, lr, out: tr.run(s0 * n_pairs, src_of(s0, prm.shape[0]), prm, lr, opt.mom, opt.m,
                                                                opt.pow, out))
    fname = save_net(net_fname_of("mb", "fast", argv), tr.layers(), opt)
    last_run = {"net_fname": fname, "losses": losses, "epochs": epochs}
    return fname


def test_examples(te):
    """main.lua:1124-1130: (te[i], 2) for every te, then (5, 3) and (5, 4): (image number, 1-based view of light 1)."""
    return [(int(i), 2) for i in np.asarray(te).ravel()] + [(5, 3), (5, 4)]


def evaluate(opt, prm, run, device, data=None):
    """main.lua:1172-1238, 1290-1292 for mb test_te: predict each example through `run(x_batch, D, workspace=...)` with the
    image's own disp_max, print `runtime err` per example (err_at 1, against dispnoc) and the mean error.  Returns the
    mean."""
    import torch
    from .predict import Workspace
    if data is None:
        data = load_mb_data(data_dir_of(opt), "test_te")
    err_at = 1
    errs, shape, ws = [], None, None     # one Workspace per shape; consecutive examples of one image share theirs
    for i, right in test_examples(data["te"]):
        if not 1 <= i <= len(data["X"]) or not data["X"][i - 1] or np.asarray(data["X"][i - 1][0]).ndim != 4:
            raise SystemExit("test_te: image %d has no test views (x_%d_1.bin is missing or empty)" % (i, i))
        x = np.asarray(data["X"][i - 1][0], np.float32)
        if right > x.shape[0]:
            raise SystemExit("test_te: image %d has %d test views, view %d is asked for" % (i, x.shape[0], right))
        if i not in data["dispnoc"]:
            raise SystemExit("test_te: image %d has no dispnoc%d.bin" % (i, i))
        D = int(data["meta"][i - 1, 2])
        if D <= 0:
            raise SystemExit("test_te: meta.bin gives image %d a disp_max of %d" % (i, D))
        H, W = x.shape[-2:]
        xb = torch.from_numpy(np.ascontiguousarray(np.stack([x[0], x[right - 1]]).reshape(2, 1, H, W))).to(device)
        if (D, H, W) != shape:
            ws = None                          # release the previous shape's before taking the next
            shape, ws = (D, H, W), Workspace(prm, D, H, W, device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = run(xb, D, workspace=ws)["disp"]
        torch.cuda.synchronize()
        runtime = time.perf_counter() - t0
        pred = pred.cpu().numpy().reshape(H, W)
        assert not np.isnan(pred.sum())
        err = error_rate(pred, np.asarray(data["dispnoc"][i], np.float32).reshape(H, W), err_at)
        errs.append(err)
        print(runtime, err)
    mean = sum(errs) / len(errs)
    print(mean)
    return mean
