"""`main.lua -a train_tr | train_all` for arch fast on kitti / kitti2015 (main.lua:602-890) on the MI355X.

The data (`x0, x1, metadata, tr, te, nnz_tr, nnz_te` of `-data_dir`, main.lua:427-445) is uploaded once; every step --
sampling the pairs' patches (make_patch + OpenCV's bicubic warpAffine), the forward and backward pass of the Siamese net
(four valid 3x3 convolutions, ReLU between them, Normalize2, StereoJoin1, the Margin2 hinge) and the momentum-SGD update --
runs on the GPU in two kernels of libmctrain.so (include/mc_train.h), enqueued chunk by chunk through `mc_train_run` with
no host round trip inside a chunk.

Randomness: ONE `numpy.random.Generator(-seed)` draws the permutation (once, before the first epoch, main.lua:657; the
same permutation every epoch) and then, vectorised per chunk of steps, every augmentation parameter of main.lua:790-814
with the reference's distributions.  Torch's Mersenne-Twister stream is NOT reproduced, so a run does not draw the
reference's numbers for the same -seed; it is bitwise reproducible for a given -seed on this implementation (gradients
are reduced in a fixed order, no float atomics).  The initial weights are those of `load_net("random:<seed>")`
(nn.SpatialConvolution:reset's range).

`-at 1` (main.lua:403-426) reads data.kitti and data.kitti2015 together: the 2012 training images, the 2015 training
images, then the chosen set's test images (for kitti2015 from 2015 image n_tr on: main.lua's X_15[{{200,400}}]); the 2015
indices and nnz image ids are shifted by 2012's n_tr.  main.lua hard-codes the two n_tr (194, 200); here each is the
length of its set's dispnoc.bin.  The sets come from `python -m mc_cnn_amd.preprocess_kitti`.

What the four trainable nets have in common is train_common.py's: the draws and the epoch loop (`draw_params`,
`run_epochs`), the flat parameter layout (`NetShape`), the Trainer's common device state (`TrainerBase`) and `step_batch`.
This module adds the KITTI data, the image store (`KittiTrainer`), libmctrain.so's `run` and `sample`, the saved fast net
and the evaluation; train_slow.py (libmctrainslow.so) reuses the data, the store and the evaluation, train_mb.py
(libmctrainmb.so) and train_mb_slow.py the saved net and the error.
Not covered: -subset, -debug, -a submit, multi-GPU.
"""
import os
import time

import numpy as np

from . import _train_lib as tl
from . import train_common as common
from .binio import dims, fromfile
from .train_common import NetShape, TrainerBase, _p, _stream, draw_params, n_steps_per_epoch, run_epochs, training_rows  # noqa: F401

CHUNK_STEPS = 256           # steps enqueued per mc_train_run call (one chunk of parameter draws)
DATA_FILES = ("x0", "x1", "metadata", "tr", "te", "nnz_tr", "nnz_te")


def data_dir_of(dataset, opt):
    return getattr(opt, "data_dir", "") or ("data.kitti" if dataset == "kitti" else "data.kitti2015")


AT_DIRS = ("data.kitti", "data.kitti2015")


def load_data(dataset, opt, names=DATA_FILES):
    """main.lua:403-445: the arrays of `data.kitti` / `data.kitti2015` (binio.fromfile), as numpy; both sets with -at 1."""
    if getattr(opt, "at", 0) == 1:
        return load_data_at(dataset, names)
    d = data_dir_of(dataset, opt)
    return {k: fromfile(os.path.join(d, k + ".bin")) for k in names}


def load_data_at(dataset, names=DATA_FILES, dirs=AT_DIRS):
    """main.lua:403-426 (-at 1): data.kitti and data.kitti2015 combined.  n12 / n15, main.lua's 194 / 200, are the
    lengths of the sets' dispnoc.bin."""
    n12, n15 = (dims(os.path.join(d, "dispnoc.bin"))[0] for d in dirs)
    out = {}
    for k in names:
        a12, a15 = (fromfile(os.path.join(d, k + ".bin")) for d in dirs)
        if k in ("x0", "x1", "metadata"):      # load(): X_12[1..194], X_15[1..200], X_12[195..389] | X_15[200..400]
            out[k] = np.concatenate([a12[:n12], a15[:n15], a12[n12:] if dataset == "kitti" else a15[n15 - 1:]], 0)
        elif k == "dispnoc":
            out[k] = np.concatenate([a12, a15], 0)
        elif k == "tr":
            out[k] = np.concatenate([a12, a15 + n12], 0)
        elif k == "te":
            out[k] = a12 if dataset == "kitti" else a15 + n12
        elif k in ("nnz_tr", "nnz_te"):        # load_nnz(): X_15[{{},1}]:add(194)
            a15 = np.array(a15).reshape(-1, 4)
            a15[:, 0] += n12
            out[k] = np.concatenate([np.asarray(a12).reshape(-1, 4), a15], 0)
        else:
            raise KeyError("-at 1: no rule to combine %s" % k)
    return out


NET = NetShape(tl.L1, tl.FM, 0, 0, tl.NPARAMS, "libmctrain.so")
flat_params = NET.flat_params     # [(w, b)] of the fast net -> one float32 vector in include/mc_train.h's order (w1 b1 .. w4 b4)


def unflat_params(v):
    return NET.unflat_params(v)[0]


class KittiTrainer(TrainerBase):
    """TrainerBase and the image store of a KITTI set: x0, x1 as (n_img, H, W) on the device."""

    def __init__(self, x0, x1, nnz, perm, conv_layers, fc_layers, n_pairs, device):
        super().__init__(nnz, perm, conv_layers, fc_layers, n_pairs, device)
        x0, x1 = np.asarray(x0), np.asarray(x1)
        self.n_img, self.H, self.W = x0.shape[0], x0.shape[-2], x0.shape[-1]
        self.x0 = self.f32(x0.reshape(self.n_img, self.H, self.W))
        self.x1 = self.f32(x1.reshape(self.n_img, self.H, self.W))


class Trainer(KittiTrainer):
    """Device state of a training run: images, nnz, permutation, parameters, momenta, workspace."""
    LIB, WHO, SHAPE = tl, "train", NET

    def __init__(self, x0, x1, nnz, perm, layers, n_pairs, device):
        super().__init__(x0, x1, nnz, perm, layers, (), n_pairs, device)

    def run(self, t0, prm, lr, mom, margin, pow_, losses):
        """mc_train_run: prm (n_steps, n_pairs, 18) on the device; losses (>= n_steps) device float32."""
        self.call("run", _p(self.x0), _p(self.x1), self.n_img, self.H, self.W, _p(self.nnz), self.nnz.shape[0], _p(self.perm),
                  self.perm.shape[0], t0, prm.shape[0], self.n_pairs, _p(prm), _p(self.params), _p(self.moms), lr, mom, margin,
                  pow_, _p(losses))


def sample(x0, x1, nnz, rows, prm):
    """mc_train_sample on device tensors: x0, x1 (n_img, H, W), nnz (n, 4), rows (n_pairs,) int32, prm (n_pairs, 18)
    -> (n_pairs, 3, 9, 9): left, positive, negative patch of each pair."""
    import torch
    lib = tl.load()
    n_img, H, W = x0.shape
    out = torch.empty((rows.shape[0], 3, tl.WS, tl.WS), dtype=torch.float32, device=x0.device)
    tl.check(lib.mc_train_sample(_p(x0), _p(x1), n_img, H, W, _p(nnz), nnz.shape[0], _p(rows), _p(prm), rows.shape[0], _p(out),
                                 _stream()), "mc_train_sample")
    return out


def step_batch(patches, params, moms, lr, mom, margin, pow_, workspace=None):
    """mc_train_step_batch: one SGD step on patches (n_pairs, 3, 9, 9); params / moms updated in place.  Returns the
    device scalar of the batch's mean loss."""
    return common.step_batch(tl, "train", patches, params, moms, (lr, mom, margin, pow_), workspace)


def net_fname_of(dataset, arch, argv):
    """main.lua:344-347, 587-600: net/net_<dataset>_<arch>_<arg>_<arg>....t7."""
    cmd_str = "_".join([dataset, arch] + [a.replace(os.sep, "_") for a in argv])
    return os.path.join("net", "net_%s.t7" % cmd_str)


def save_net(fname, layers, opt):
    """torch.save(fname, {clean_net(net_te), opt}, 'ascii') of arch fast (main.lua:587-600): net_te is net_tr with
    padding 1 and StereoJoin(1) in place of StereoJoin1 (main.lua:739-746)."""
    from . import t7
    mods = []
    for i, (w, b) in enumerate(layers):
        mods.append(t7.T7Object("cudnn.SpatialConvolution", {
            "weight": np.ascontiguousarray(w, np.float32), "bias": np.ascontiguousarray(b, np.float32),
            "nInputPlane": int(w.shape[1]), "nOutputPlane": int(w.shape[0]), "kW": 3, "kH": 3, "dW": 1, "dH": 1,
            "padW": 1, "padH": 1, "train": False}))
        if i < len(layers) - 1:
            mods.append(t7.T7Object("cudnn.ReLU", {"inplace": True, "train": False}))
    mods.append(t7.T7Object("nn.Normalize2", {"train": False}))
    mods.append(t7.T7Object("nn.StereoJoin", {"disp_max": 1, "train": False}))
    net_te = t7.T7Object("nn.Sequential", {"modules": mods, "train": False})
    opt_t = {k: v for k, v in sorted(vars(opt).items()) if isinstance(v, (bool, int, float, str)) and k not in ("fc_mode", "conv_mode")}   # -fc_mode / -conv_mode are how a run predicts, not the net's
    d = os.path.dirname(fname)
    if d:
        os.makedirs(d, exist_ok=True)
    t7.save(fname, [net_te, opt_t])
    return fname


last_run = None   # the latest train() result: {"net_fname", "losses" (per step, float32), "epochs"}


def train(dataset, arch, opt, argv, device, data=None):
    """main.lua:602-890 for -a train_tr / train_all: returns the saved net's file name."""
    global last_run
    from .main import load_net
    if data is None:
        data = load_data(dataset, opt)
    nnz, rng, perm = training_rows(opt, data)
    n_pairs = opt.bs // 2
    tr = Trainer(data["x0"], data["x1"], nnz, perm, load_net("random:%d" % opt.seed, dataset, arch), n_pairs, device)
    losses, epochs = run_epochs(tr, rng, opt, n_steps_per_epoch(nnz.shape[0], opt.bs), n_pairs, device, CHUNK_STEPS,
                                lambda s0, prm, lr, out: tr.run(s0 * n_pairs, prm, lr, opt.mom, opt.m, opt.pow, out))
    fname = save_net(net_fname_of(dataset, arch, argv), tr.layers(), opt)
    last_run = {"net_fname": fname, "losses": losses, "epochs": epochs}
    return fname


def test_examples(opt, data):
    """main.lua:1121-1138: test_te -> te, test_all -> tr .. te (1-based image indices)."""
    te = np.asarray(data["te"]).ravel().astype(np.int64)
    if opt.a == "test_te":
        return list(te)
    return list(np.asarray(data["tr"]).ravel().astype(np.int64)) + list(te)


def error_rate(pred, actual, err_at):
    """main.lua:1224-1234: bad pixels (|actual - pred| > err_at) over pixels with actual != 0."""
    mask = actual != 0
    bad = (np.abs(actual - pred) > err_at) & mask
    return float(bad.sum()) / float(mask.sum())


def evaluate(dataset, opt, run, device, data=None):
    """main.lua:1172-1238, 1290-1292 for test_te / test_all: predict each listed pair through `run(x_batch, D)`, print
    `runtime err` per pair and the mean error.  Returns the mean."""
    import torch
    if data is None:
        data = load_data(dataset, opt, ("x0", "x1", "metadata", "tr", "te", "dispnoc"))
    x0, x1, meta, dispnoc = data["x0"], data["x1"], np.asarray(data["metadata"]), data["dispnoc"]
    H, W = x0.shape[-2], x0.shape[-1]
    err_at = 3
    errs = []
    for i in test_examples(opt, data):
        w = int(meta[i - 1, 1])
        xb = torch.from_numpy(np.ascontiguousarray(np.stack([x0[i - 1].reshape(1, H, W)[..., :w],
                                                              x1[i - 1].reshape(1, H, W)[..., :w]]), np.float32)).to(device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pred = run(xb, opt.disp_max)["disp"]
        torch.cuda.synchronize()
        runtime = time.perf_counter() - t0
        pred = pred.cpu().numpy().reshape(H, w)
        assert not np.isnan(pred.sum())
        err = error_rate(pred, np.asarray(dispnoc[i - 1], np.float32).reshape(H, W)[:, :w], err_at)
        errs.append(err)
        print(runtime, err)
    mean = sum(errs) / len(errs)
    print(mean)
    return mean
