"""Step time of the accurate architecture's training at -l2 1..7 (libmctrainslowdepth.so) on either image store, at the shapes of
scripts/train_slow_bench.py (KITTI) and scripts/train_mb_slow_bench.py (Middlebury), and the cost of the run-time depth against the
library compiled for the data set's own depth.

    python scripts/train_slow_depth_bench.py [--store kitti|mb] [--steps 400] [--warmup 50] [--bs 128] [--runs 5] [--skip-sweep] [--skip-ab]

* the sweep: `mc_train_slow_depth_run` / `mc_train_slow_depth_mb_run` at l2 = 1 .. 7 -- sampling from a resident synthetic store (389
  pairs of 350 x 1242, or 24 ragged scenes of Middlebury-like sizes), forward, BCECriterion2, backward and momentum SGD, 2 l2 + 4
  kernels per step -- timed with HIP events over --steps steps after --warmup steps, from wide weights (the ReLUs half active).
* the comparison: at the data set's own depth (kitti 4, mb 3) the new library against libmctrainslow.so / libmctrainmbslow.so on the
  same store, permutation and draws, --runs runs of each, alternating (old, new, old, new, ...).  Both print the same last loss.  The
  difference of the medians is held against the parent library's own spread (max - min) over its runs.

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from train_mb_bench import synthetic_store, time_fn  # noqa: E402  (the same store, the same clock)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", default="kitti", choices=("kitti", "mb"))
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--skip-sweep", action="store_true")
    ap.add_argument("--skip-ab", action="store_true")
    args = ap.parse_args()
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import train_mb, train_mb_slow, train_slow, train_slow_depth

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n_pairs = args.bs // 2
    n_steps = args.warmup + args.steps
    w = args.warmup
    rng = np.random.default_rng(0)
    n_nnz = 1_000_000
    mb = args.store == "mb"
    dataset = "mb" if mb else "kitti"
    old = train_mb_slow if mb else train_slow
    if mb:
        table, index, total = synthetic_store(rng)
        img = rng.integers(1, index.shape[0] + 1, n_nnz)
        size = np.array([(table[index[i - 1, 0]]["H"], table[index[i - 1, 0]]["W"]) for i in range(1, index.shape[0] + 1)])
        nnz = np.stack([img, rng.integers(0, 1 << 30, n_nnz) % size[img - 1, 0], rng.integers(0, 1 << 30, n_nnz) % size[img - 1, 1],
                        rng.uniform(1, 200, n_nnz)], 1).astype(np.float32)
        perm = rng.permutation(n_nnz).astype(np.int32)
        planes, dtable = torch.randn(total, device=dev), train_mb.device_table(table, dev)      # the store, resident
        opt = old.parse(["mb", "slow", "-a", "train_tr"])[2]
        prm = torch.from_numpy(old.draw_params(rng, opt, n_steps, n_pairs)).to(dev)
        src = torch.from_numpy(old.draw_sources(rng, opt, img[perm[:n_steps * n_pairs]].reshape(n_steps, n_pairs), index)).to(dev)
    else:
        n_img, H, W = 389, 350, 1242
        nnz = np.stack([rng.integers(1, n_img + 1, n_nnz), rng.integers(0, H, n_nnz), rng.integers(0, W, n_nnz),
                        rng.uniform(1, 200, n_nnz)], 1).astype(np.float32)
        perm = rng.permutation(n_nnz).astype(np.int32)
        x0, x1 = torch.randn((n_img, H, W), device=dev), torch.randn((n_img, H, W), device=dev)   # KITTI-sized images, resident
        opt = old.parse(["kitti", "slow", "-a", "train_tr"])[2]
        prm = torch.from_numpy(old.draw_params(rng, opt, n_steps, n_pairs)).to(dev)
    losses = torch.empty(n_steps, dtype=torch.float32, device=dev)

    def measure(lib, l2):
        """(us per step, the last loss) of a fresh trainer of `lib` ("old" | "new") at depth l2 from the same wide weights."""
        conv, fc = train_slow_depth.net_shape(dataset, l2).init_net(1, gain=np.sqrt(6.0))
        if mb:
            cls = old.Trainer if lib == "old" else train_slow_depth.MbTrainer
            t = cls(np.zeros(16, np.float32), table[:1], nnz, perm, conv, fc, n_pairs, dev)
            t.planes, t.table = planes, dtable
            run = lambda t0, a, out: t.run(t0, src[a:], prm[a:], opt.lr, opt.mom, out)  # noqa: E731
        else:
            tiny = np.zeros((1, 4, 4), np.float32)
            cls = old.Trainer if lib == "old" else train_slow_depth.Trainer
            t = cls(tiny, tiny, nnz, perm, conv, fc, n_pairs, dev)
            t.x0, t.x1, t.n_img, t.H, t.W = x0, x1, n_img, H, W
            run = lambda t0, a, out: t.run(t0, prm[a:], opt.lr, opt.mom, out)  # noqa: E731
        if mb:                                              # the warm-up's chunk
            t.run(0, src[:w], prm[:w], opt.lr, opt.mom, losses)
        else:
            t.run(0, prm[:w], opt.lr, opt.mom, losses)
        us = time_fn(lambda n: run(w * n_pairs, w, losses[w:]), args.steps)
        return us, float(losses[-1].cpu()), t.ws_bytes

    out = {"metric": "train_slow_depth_step_us", "store": args.store, "bs": args.bs, "steps": args.steps, "warmup": args.warmup}
    if not args.skip_sweep:
        sweep = {}
        for l2 in range(train_slow_depth.L2_RANGE[0], train_slow_depth.L2_RANGE[1] + 1):
            us, last, ws_bytes = measure("new", l2)
            sweep[str(l2)] = {"us_per_step": round(us, 2), "launches": 2 * l2 + 4, "workspace_mb": round(ws_bytes * 1e-6, 1), "loss_last": last}
        out["sweep"] = sweep
    if not args.skip_ab:
        l2 = old.NET.l2
        runs = {"old": [], "new": []}
        last = {}
        for _ in range(args.runs):
            for lib in ("old", "new"):
                us, loss, _ = measure(lib, l2)
                runs[lib].append(round(us, 2))
                last[lib] = loss
        med = {k: float(np.median(v)) for k, v in runs.items()}
        spread = max(runs["old"]) - min(runs["old"])
        out["ab"] = {"l2": l2, "old_library": old.NET.library, "old_us": runs["old"], "new_us": runs["new"], "old_median": round(med["old"], 2),
                     "new_median": round(med["new"], 2), "difference_of_medians": round(med["new"] - med["old"], 2), "old_spread": round(spread, 2),
                     "inside_old_spread": bool(abs(med["new"] - med["old"]) <= spread), "same_last_loss": last["old"] == last["new"],
                     "loss_last": last["new"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
