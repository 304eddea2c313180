"""`predict_kitti.lua` on one node of MI355Xs: the 3-pixel error over the KITTI 2012 training pairs (action `test`) or the
disparity maps of the test pairs as 16-bit PNGs for the evaluation server (action `submit`).

The reference spawns `./main.lua kitti fast -a predict ...` once per pair and reads `disp.bin` back
(`predict_kitti.lua:40-43, 53-63`); here the net is loaded once per process and the pairs are SHARDED over the ranks
(pair i -> rank i % world, `batch.shard`), every pair staying on its GPU; the only exchange is one all-reduce of
(error sum, pair count) at the end, or none at all for `submit` (each rank writes its own files).

    python -m mc_cnn_amd.predict_kitti test   [-path data.kitti/unzip] [-net_fname net/net_kitti_fast_-a_train_all.t7]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m mc_cnn_amd.predict_kitti submit

Within a rank `-pairs_in_flight K` (default 2) pairs are in flight: the PNGs of the next pairs are decoded and normalised by a worker
thread while the GPU runs the current ones, and the pairs alternate between K slots (stream, pinned staging buffers, workspace), so a
pair's upload / feature net / mc_predict / download overlap its neighbours' (bench.py's `pipelined` record: 2.63 -> 2.3-2.5 ms per pair
on the GPU side at KITTI size).  Results do not depend on K.

`-sparse` (no counterpart in the reference) keeps only the pixels that passed the left-right check, class 0 of `mc_predict_ex`'s outlier
map, i.e. those that were measured and not filled in by the two interpolation stages: `submit -sparse` writes 0, KITTI's "no estimate",
everywhere else; `test -sparse` prints `i err density` per pair -- the 3-pixel error over the ground-truth pixels of class 0 and their
share of all ground-truth pixels -- and then the two means.

`-sparse_by NAME -keep F` replaces that one operating point by a dial: per image the fraction F of the pixels that the confidence measure
NAME (confidence.py: msm | mmn | mlm | cur | cls | lrc) ranks highest is kept, `test` prints `i err density` and `submit` writes 0 elsewhere,
as with `-sparse`.  `test -roc` scores the measures themselves: per pair, behind `i err`, the area under the sparsification curve of every
measure and of the ranking by the error itself (`oracle`, the floor) at the 3-pixel threshold, and at the end the mean of each.

Same file layout as the reference: <path>/{training,testing}/image_{0,1}/%06d_10.png, ground truth
<path>/training/disp_noc/%06d_10.png (PNG16, value/256, 0 = no ground truth), output out/%06d_10.png.
"""
import argparse
import os
import sys

import numpy as np

from .batch import shard
from .binio import read_png16, write_png16
from .params import SM_SKIP

N_PAIRS = {"test": 194, "submit": 195}   # predict_kitti.lua:47-52


def pair_paths(path, action, i):
    d = "training" if action == "test" else "testing"
    return ("%s/%s/image_0/%06d_10.png" % (path, d, i), "%s/%s/image_1/%06d_10.png" % (path, d, i))


def three_pixel_error(disp, ground_truth):
    """predict_kitti.lua:70-73: share of the pixels WITH ground truth whose |disp - gt| exceeds 3."""
    mask = ground_truth != 0
    bad = (np.abs(disp - ground_truth) > 3) & mask
    return float(bad.sum()) / float(mask.sum())


def kept_error(disp, ground_truth, keep):
    """(3-pixel error over the ground-truth pixels of the bool map keep, their share of all ground-truth pixels); an error of 0 where
    there is no such pixel."""
    mask = ground_truth != 0
    kept = mask & keep
    bad = (np.abs(disp - ground_truth) > 3) & kept
    n_kept, n_gt = float(kept.sum()), float(mask.sum())
    return (float(bad.sum()) / n_kept if n_kept else 0.0), (n_kept / n_gt if n_gt else 0.0)


def sparse_error(disp, ground_truth, outlier):
    """-sparse: kept_error over the pixels of outlier class 0"""
    return kept_error(disp, ground_truth, outlier == 0)


ERR_AT = 3.0   # the set's error threshold (predict_kitti.lua:72)


def roc_areas(disp, ground_truth, conf):
    """-roc: ({name: area under the sparsification curve of conf[name]}, the oracle ranking's area) for one pair at ERR_AT"""
    import torch
    from . import confidence
    pred, actual = torch.from_numpy(np.ascontiguousarray(disp)), torch.from_numpy(np.ascontiguousarray(ground_truth))
    areas, floor = {}, None
    for name, c in conf.items():
        bad, bad_oracle, m = confidence.sparsification(torch.from_numpy(np.ascontiguousarray(c)), pred, actual, ERR_AT)
        areas[name], floor = confidence.area(bad, m), confidence.area(bad_oracle, m)
    return areas, floor


def run(action, path, predict_pair, world=1, rank=0, out_dir="out", n_pairs=None, log=print, in_flight=1, sparse=False, roc=None,
        sparse_by=None, keep=None):
    """predict_pair(left_png, right_png) -> (H,W) float32 disparity.  Returns (error sum, pairs done) of this rank.
    sparse: predict_pair gives (disparity, outlier classes), both (H,W); `submit` writes 0 where the class is not 0, `test` scores the
    pixels of class 0 alone, logs (i, err, density) and returns (error sum, pairs done, density sum).
    A predict_pair object with .submit(left_png, right_png) -> ticket and .result(ticket) -> disparity is driven with up to
    `in_flight` pairs submitted ahead of the one whose result is being scored / written (same order, same results).
    roc (test; a tuple of measure names) or sparse_by (a measure name, with keep, the fraction): predict_pair gives (disparity, {name:
    (H,W) confidence}).  roc logs (i, err, one area per name, the oracle ranking's area) and returns (error sum, pairs done, the area
    sums in that order); sparse_by keeps confidence.keep_mask(measure, keep) per image and logs and returns what sparse does."""
    n = N_PAIRS[action] if n_pairs is None else n_pairs
    err_sum, done, density_sum, area_sums = 0.0, 0, 0.0, []
    todo = list(shard(n, world, rank))
    staged = hasattr(predict_pair, "submit") and in_flight > 1
    tickets = {}
    ahead = 0
    for k, i in enumerate(todo):
        if staged:
            while ahead < len(todo) and ahead < k + in_flight:
                tickets[todo[ahead]] = predict_pair.submit(*pair_paths(path, action, todo[ahead]))
                ahead += 1
            disp = predict_pair.result(tickets.pop(i))
        else:
            im0, im1 = pair_paths(path, action, i)
            disp = predict_pair(im0, im1)
        if sparse:
            disp, outlier = disp
            outlier = np.asarray(outlier, np.float32)
        elif roc or sparse_by:
            disp, conf = disp
        disp = np.asarray(disp, np.float32)
        if sparse_by:
            import torch
            from . import confidence
            kept = confidence.keep_mask(torch.from_numpy(np.ascontiguousarray(conf[sparse_by], np.float32)), keep).numpy()
        if action == "test":
            gt = read_png16("%s/training/disp_noc/%06d_10.png" % (path, i))
            if sparse:
                err, density = sparse_error(disp, gt, outlier)
                density_sum += density
                log(i, err, density)
            elif sparse_by:
                err, density = kept_error(disp, gt, kept)
                density_sum += density
                log(i, err, density)
            elif roc:
                err = three_pixel_error(disp, gt)
                areas, floor = roc_areas(disp, gt, {name: conf[name] for name in roc})
                row = [areas[name] for name in roc] + [floor]
                area_sums = [a + b for a, b in zip(area_sums, row)] if area_sums else row
                log(i, err, *row)
            else:
                err = three_pixel_error(disp, gt)
                log(i, err)
            err_sum += err
        else:
            if sparse:
                disp = np.where(outlier == 0, disp, np.float32(0))
            elif sparse_by:
                disp = np.where(kept, disp, np.float32(0))
            os.makedirs(out_dir, exist_ok=True)
            write_png16(disp, "%s/%06d_10.png" % (out_dir, i))
            log(i)
        done += 1
    if roc:
        return (err_sum, done) + tuple(area_sums if area_sums else [0.0] * (len(roc) + 1))
    return (err_sum, done, density_sum) if sparse or sparse_by else (err_sum, done)


class PairPipeline:
    """K pairs in flight on one GPU: a pair is handled start to finish by a worker thread on its slot (stream, pinned staging buffers,
    workspace) -- decode + normalise (host side of main.lua:1085-1096), upload, feature net, mc_predict, download -- so that the host
    work of one pair and the GPU work of another overlap, and so do the kernels of two pairs (different streams).  The library is
    re-entrant: one workspace and one scratch area per stream."""

    def __init__(self, prm, layers, disp_max, dev, slots=2, conv_mode="fp32", sparse=False, confidence=()):
        import concurrent.futures
        import torch
        self.prm, self.layers, self.disp_max, self.dev = prm, layers, disp_max, dev
        self.conv_mode = conv_mode          # main.features_fast's: mc_conv3x3 (fp32) or mc_conv_split (bf16x3) for the inner layers
        self.sparse = sparse                # -sparse: a pair's result is (disparity, outlier classes), through mc_predict_ex
        self.confidence = tuple(confidence)  # -roc / -sparse_by: measure names; a pair's result is (disparity, {name: (H,W) map})
        self.slots = [dict(stream=torch.cuda.Stream(device=dev), shape=None) for _ in range(max(1, slots))]
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=len(self.slots))
        self.next = 0

    @staticmethod
    def stage(im0, im1):
        from . import main as mcmain
        x0, x1 = mcmain.load_image(im0), mcmain.load_image(im1)
        if x0.shape[0] == 3:
            x0, x1 = mcmain.rgb2y(x0), mcmain.rgb2y(x1)
        return np.stack([mcmain.normalize(x0), mcmain.normalize(x1)]).astype(np.float32)

    def _work(self, sl, im0, im1):
        import torch
        from . import main as mcmain
        from .predict import Workspace, stereo_predict_fused
        torch.cuda.set_device(self.dev)
        host = self.stage(im0, im1)
        if sl["shape"] != host.shape:   # (KITTI pairs come in a few sizes)
            H, W = host.shape[-2:]
            sl.update(shape=host.shape, pin_in=torch.empty(host.shape, dtype=torch.float32).pin_memory(),
                      pin_out=torch.empty((H, W), dtype=torch.float32).pin_memory(),
                      pin_outlier=torch.empty((H, W), dtype=torch.float32).pin_memory() if self.sparse else None,
                      ws=Workspace(self.prm, self.disp_max, H, W, self.dev))
        sl["pin_in"].copy_(torch.from_numpy(host))
        with torch.cuda.stream(sl["stream"]):
            xb = sl["pin_in"].to(self.dev, non_blocking=True)
            want = dict(want_outlier=self.sparse)
            if self.confidence:   # every map the measures read; they are taken on the device
                want = dict(want_outlier=True, want_disp0=True, want_margins=True, want_confidence="cur" in self.confidence)
            res = stereo_predict_fused(xb, self.prm, self.disp_max, feat=mcmain.features_fast(xb, self.layers, self.conv_mode), workspace=sl["ws"],
                                       **want)
            if self.confidence:
                from . import confidence
                maps = confidence.measures(res, self.disp_max)
                conf = {name: maps[name].cpu().numpy() for name in self.confidence}
            sl["pin_out"].copy_(res["disp"].reshape(xb.shape[2:]), non_blocking=True)
            if self.sparse:
                sl["pin_outlier"].copy_(res["outlier"].reshape(xb.shape[2:]), non_blocking=True)
        sl["stream"].synchronize()
        if self.sparse:
            return sl["pin_out"].numpy().copy(), sl["pin_outlier"].numpy().copy()
        if self.confidence:
            return sl["pin_out"].numpy().copy(), conf
        return sl["pin_out"].numpy().copy()

    def submit(self, im0, im1):
        """Queue a pair on the next slot.  The caller takes results in submission order and keeps at most len(slots) pairs submitted
        (run() does), so a slot's previous pair has been collected before the slot is used again."""
        sl = self.slots[self.next % len(self.slots)]
        self.next += 1
        return self.pool.submit(self._work, sl, im0, im1)

    def result(self, ticket):
        return ticket.result()

    def __call__(self, im0, im1):
        return self.result(self.submit(im0, im1))


def parse(argv=None):
    from .train_common import add_conv_mode_flag, check_conv_mode
    ap = argparse.ArgumentParser(prog="predict_kitti")
    ap.add_argument("action", choices=["test", "submit"])
    ap.add_argument("-path", default="data.kitti/unzip")
    ap.add_argument("-net_fname", default="net/net_kitti_fast_-a_train_all.t7")
    ap.add_argument("-disp_max", type=int, default=228)
    ap.add_argument("-n", type=int, default=None, help="number of pairs (default: the reference's 194 / 195)")
    ap.add_argument("-pairs_in_flight", type=int, default=2, help="pairs staged / queued ahead per rank (1: one at a time)")
    ap.add_argument("-sparse", action="store_true",
                    help="keep the pixels that passed the left-right check only: submit writes 0 elsewhere, test prints i err density")
    ap.add_argument("-roc", action="store_true",
                    help="test: print per pair, and as means, the area under the sparsification curve of every confidence measure and of the oracle ranking")
    ap.add_argument("-sparse_by", default=None, metavar="NAME",
                    help="with -keep F: keep the fraction F of each image that the confidence measure NAME (%s) ranks highest" % " | ".join(MEASURES))
    ap.add_argument("-keep", type=float, default=None, metavar="F", help="with -sparse_by NAME: the fraction of each image to keep, in (0, 1]")
    ap.add_argument("-sm_skip", default="", choices=sorted(SM_SKIP), help="main.lua:26")
    add_conv_mode_flag(ap)           # main.py's flag: the fast net's convolutions
    opt = ap.parse_args(argv)
    check_conv_mode(opt, "fast", "predict_kitti")
    check_confidence_flags(opt)
    return opt


MEASURES = ("msm", "mmn", "mlm", "cur", "cls", "lrc")   # confidence.NAMES (that module imports torch; tests/test_confidence_host.py holds the two equal)


def available_measures(sm_skip):
    """the measures the command line's pipeline can give: `cur` is the sub-pixel stage's"""
    return tuple(name for name in MEASURES if name != "cur" or sm_skip != "subpixel_enchancement")


def check_confidence_flags(opt):
    """-roc, -sparse_by NAME -keep F: refused with what is supported"""
    if opt.roc and opt.action != "test":
        raise SystemExit("predict_kitti: -roc scores the confidence measures against ground truth and goes with the action test only")
    if opt.roc and opt.sparse:
        raise SystemExit("predict_kitti: -roc scores every measure over all ground-truth pixels and does not go with -sparse")
    if (opt.sparse_by is None) != (opt.keep is None):
        raise SystemExit("predict_kitti: -sparse_by NAME and -keep F go together (NAME one of %s, F in (0, 1])" % " | ".join(MEASURES))
    if opt.sparse_by is None:
        return
    if opt.sparse or opt.roc:
        raise SystemExit("predict_kitti: -sparse_by NAME -keep F goes with neither -sparse (the one operating point of the left-right check; "
                         "-sparse_by cls is its measure) nor -roc")
    if opt.sparse_by not in MEASURES:
        raise SystemExit("predict_kitti: -sparse_by %s is not a confidence measure; supported: %s" % (opt.sparse_by, " | ".join(MEASURES)))
    if not 0 < opt.keep <= 1:
        raise SystemExit("predict_kitti: -keep %r is outside (0, 1]: the fraction of each image to keep" % (opt.keep,))
    if opt.sparse_by not in available_measures(opt.sm_skip):
        raise SystemExit("predict_kitti: -sparse_by cur reads the sub-pixel stage's curvature, which -sm_skip subpixel_enchancement skips; "
                         "supported there: %s" % " | ".join(available_measures(opt.sm_skip)))


def main(argv=None):
    opt = parse(argv)
    import torch
    import torch.distributed as dist
    from . import main as mcmain
    from .params import TABLES
    world, rank = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=dev)
    layers = mcmain.device_layers(mcmain.load_net(opt.net_fname, "kitti", "fast"), dev)   # resident: uploaded once
    prm = dict(TABLES[("kitti", "fast")])
    prm["border_n"] = len(layers)
    prm["sm_skip"] = opt.sm_skip
    roc = available_measures(opt.sm_skip) if opt.roc else None
    wanted = roc or ((opt.sparse_by,) if opt.sparse_by else ())
    predict_pair = PairPipeline(prm, layers, opt.disp_max, dev, slots=opt.pairs_in_flight, conv_mode=getattr(opt, "conv_mode", "fp32"),
                               sparse=opt.sparse, confidence=wanted)
    if roc and rank == 0:
        print("i", "err", *(roc + ("oracle",)))
    sums = run(opt.action, opt.path, predict_pair, world, rank, n_pairs=opt.n, in_flight=opt.pairs_in_flight, sparse=opt.sparse, roc=roc,
               sparse_by=opt.sparse_by, keep=opt.keep)
    if opt.action == "test":
        err_sum, done = sums[:2]
        t = torch.tensor([err_sum, float(done)] + list(sums[2:]), dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(t)
        if rank == 0:
            print(t[0].item() / max(t[1].item(), 1.0))   # predict_kitti.lua:83
            if opt.sparse or opt.sparse_by:
                print(t[2].item() / max(t[1].item(), 1.0))   # the mean density
            for k, name in enumerate(roc + ("oracle",) if roc else ()):
                print(name, t[2 + k].item() / max(t[1].item(), 1.0))   # -roc: the mean area of each ranking
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
