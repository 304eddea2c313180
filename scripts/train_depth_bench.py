"""Step time of the fast architecture's training at -l1 1..5 (libmctraindepth.so) on either image store, at the shapes of
scripts/train_bench.py (KITTI) and scripts/train_mb_bench.py (Middlebury), against a torch autograd step of the same net.

    python scripts/train_depth_bench.py --l1 3 [--store kitti|mb] [--lib depth|old] [--steps 1000] [--warmup 100] [--bs 128] [--skip-torch]

* HIP: `mc_train_depth_run` / `mc_train_depth_mb_run` -- sampling from a resident synthetic store (389 pairs of 350 x 1242, or 24
  ragged scenes of Middlebury-like sizes), forward, Margin2, backward and momentum SGD -- two kernels per step, timed with HIP
  events over --steps steps.
* --lib old runs the same inputs through libmctrain.so (--store kitti, --l1 4) or libmctrainmb.so (--store mb, --l1 5): the
  comparison of the depth library with the libraries it overlaps.  The store is seeded, so both print the same hip_loss_last.
* torch: F.conv2d forward of the reference's 4-patch batch, Normalize2 / StereoJoin1 / Margin2 written in torch, autograd
  backward, momentum SGD written out, on given patches (no sampling): a lower bound of a full torch step.

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


def torch_step_fn(layers, lr, mom, margin):
    import torch
    import torch.nn.functional as F
    ps = [torch.tensor(a, device="cuda", requires_grad=True) for wb in layers for a in wb]
    vs = [torch.zeros_like(p) for p in ps]
    l1 = len(layers)

    def step(x):   # x: (4 n, 1, ws, ws) in the reference's order L, P, L, N
        for p in ps:
            p.grad = None
        h = x
        for i in range(l1):
            h = F.conv2d(h, ps[2 * i], ps[2 * i + 1])
            if i < l1 - 1:
                h = F.relu(h)
        h = h / torch.sqrt((h * h).sum(1, keepdim=True) + 1e-5)
        s = (h[0::2] * h[1::2]).sum(1).reshape(-1, 2)
        loss = torch.clamp(s[:, 1] - s[:, 0] + margin, min=0).mean()
        loss.backward()
        with torch.no_grad():
            for p, v in zip(ps, vs):
                v.mul_(mom).add_(p.grad, alpha=-lr)
                p.add_(v)
        return loss
    return step


def main():
    from train_mb_bench import synthetic_store, time_fn
    ap = argparse.ArgumentParser()
    ap.add_argument("--l1", type=int, required=True)
    ap.add_argument("--store", default="kitti", choices=("kitti", "mb"))
    ap.add_argument("--lib", default="depth", choices=("depth", "old"))
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    if args.lib == "old" and (args.store, args.l1) not in (("kitti", 4), ("mb", 5)):
        raise SystemExit("--lib old: libmctrain.so is --store kitti --l1 4, libmctrainmb.so --store mb --l1 5")
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import main as mcmain
    from mc_cnn_amd import train, train_depth, train_mb

    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n_pairs = args.bs // 2
    n_steps = args.warmup + args.steps
    w = args.warmup
    rng = np.random.default_rng(0)
    n_nnz = 1_000_000
    dataset = "kitti" if args.store == "kitti" else "mb"
    layers = mcmain.load_net("random:1", dataset, "fast", l1=args.l1)
    out = {"metric": "train_depth_step_us", "l1": args.l1, "store": args.store, "lib": args.lib, "bs": args.bs}
    if args.store == "kitti":
        n_img, H, W = 389, 350, 1242
        nnz = np.stack([rng.integers(1, n_img + 1, n_nnz), rng.integers(0, H, n_nnz), rng.integers(0, W, n_nnz),
                        rng.uniform(1, 200, n_nnz)], 1).astype(np.float32)
        perm = rng.permutation(n_nnz).astype(np.int32)
        tiny = np.zeros((1, 4, 4), np.float32)
        t = (train if args.lib == "old" else train_depth).Trainer(tiny, tiny, nnz, perm, layers, n_pairs, dev)
        t.x0 = torch.randn((n_img, H, W), device=dev)          # KITTI-sized images, resident
        t.x1 = torch.randn((n_img, H, W), device=dev)
        t.n_img, t.H, t.W = n_img, H, W
        _, _, opt, _ = mcmain.parse(["kitti", "fast", "-a", "train_tr"])
        prm = torch.from_numpy(train.draw_params(rng, opt, n_steps, n_pairs)).to(dev)
        run = lambda t0, a, b, losses: t.run(t0, prm[a:b], opt.lr, opt.mom, opt.m, opt.pow, losses)  # noqa: E731
    else:
        table, index, total = synthetic_store(rng)
        img = rng.integers(1, index.shape[0] + 1, n_nnz)
        size = np.array([(table[index[i - 1, 0]]["H"], table[index[i - 1, 0]]["W"]) for i in range(1, index.shape[0] + 1)])
        nnz = np.stack([img, rng.integers(0, 1 << 30, n_nnz) % size[img - 1, 0], rng.integers(0, 1 << 30, n_nnz) % size[img - 1, 1],
                        rng.uniform(1, 200, n_nnz)], 1).astype(np.float32)
        perm = rng.permutation(n_nnz).astype(np.int32)
        cls = train_mb.Trainer if args.lib == "old" else train_depth.MbTrainer
        t = cls(np.zeros(16, np.float32), table[:1], nnz, perm, layers, n_pairs, dev)
        t.planes = torch.randn(total, device=dev)               # the store, resident
        t.table = train_mb.device_table(table, dev)
        _, _, opt, _ = train_mb.parse(["mb", "fast", "-a", "train_tr"])
        prm = torch.from_numpy(train_mb.draw_params(rng, opt, n_steps, n_pairs)).to(dev)
        src = torch.from_numpy(train_mb.draw_sources(rng, opt, img[perm[:n_steps * n_pairs]].reshape(n_steps, n_pairs), index)).to(dev)
        run = lambda t0, a, b, losses: t.run(t0, src[a:b], prm[a:b], opt.lr, opt.mom, opt.m, opt.pow, losses)  # noqa: E731
        out.update(store_gb=round(total * 4e-9, 2), planes=int(table.shape[0]))
    losses = torch.empty(n_steps, dtype=torch.float32, device=dev)
    run(0, 0, w, losses)
    hip_us = time_fn(lambda n: run(w * n_pairs, w, n_steps, losses[w:]), args.steps)
    out.update(hip_us_per_step=round(hip_us, 2), hip_loss_last=float(losses[-1].cpu()), measured=["hip_us_per_step", "torch_us_per_step"])
    if not args.skip_torch:
        step = torch_step_fn(layers, opt.lr, opt.mom, opt.m)
        x = torch.randn((2 * args.bs, 1, 2 * args.l1 + 1, 2 * args.l1 + 1), device=dev)

        def run_torch(n):
            for _ in range(n):
                step(x)
        run_torch(args.warmup)
        out["torch_us_per_step"] = round(time_fn(run_torch, args.steps), 2)
        out["hip_speedup_vs_torch"] = round(out["torch_us_per_step"] / hip_us, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
