"""Step time of Middlebury's fast net's training (libmctrainmb.so, mc_train_mb_run), against a torch autograd step of the
same five-layer net on the same GPU and batch.

    python scripts/train_mb_bench.py [--steps 400] [--warmup 50] [--bs 128]

* HIP: `mc_train_mb_run` -- patch sampling from a ragged synthetic store of Middlebury-like sizes on the device (24 scenes
  between 480 x 640 and 1000 x 1500, 1 to 4 lights and 1 to 7 exposures each, two views per plane), forward, Margin2,
  backward and momentum SGD -- two kernels per step, timed with HIP events over --steps steps after --warmup steps.
* torch: F.conv2d (MIOpen) forward of the reference's 4-patch batch of 11 x 11 patches, Normalize2 / StereoJoin1 / Margin2
  written in torch, autograd backward, momentum SGD written out.  Its patches are given (no sampling): the torch number is a
  lower bound of a full torch step.

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_step_fn(layers, lr, mom, margin):
    import torch
    import torch.nn.functional as F
    ps = [torch.tensor(a, device="cuda", requires_grad=True) for wb in layers for a in wb]
    vs = [torch.zeros_like(p) for p in ps]
    n_layers = len(layers)

    def step(x):   # x: (4 n, 1, 11, 11) in the reference's order L, P, L, N
        for p in ps:
            p.grad = None
        h = x
        for i in range(n_layers):
            h = F.conv2d(h, ps[2 * i], ps[2 * i + 1])
            if i < n_layers - 1:
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


def time_fn(fn, n):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / n   # us per step


def synthetic_store(rng, n_scenes=24):
    """(table, index, total floats) of a ragged store of Middlebury-like sizes; the planes themselves are drawn on the device"""
    from mc_cnn_amd import train_mb
    recs, index, total = [], np.zeros((n_scenes, 3), np.int64), 0
    for n in range(n_scenes):
        H, W = int(rng.integers(480, 1001)), int(rng.integers(640, 1501))
        n_light, n_exp = int(rng.integers(1, 5)), int(rng.integers(1, 8))
        index[n] = (len(recs), n_light, n_exp)
        for _ in range(n_light * n_exp * 2):
            recs.append((total, H, W))
            total += H * W
    return np.array(recs, train_mb.PLANE_DTYPE), index, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import main as mcmain
    from mc_cnn_amd import train_mb

    dev = torch.device("cuda", 0)
    n_pairs = args.bs // 2
    n_steps = args.warmup + args.steps
    rng = np.random.default_rng(0)
    table, index, total = synthetic_store(rng)
    n_nnz = 1_000_000
    img = rng.integers(1, index.shape[0] + 1, n_nnz)
    size = np.array([(table[index[i - 1, 0]]["H"], table[index[i - 1, 0]]["W"]) for i in range(1, index.shape[0] + 1)])
    nnz = np.stack([img, rng.integers(0, 1 << 30, n_nnz) % size[img - 1, 0], rng.integers(0, 1 << 30, n_nnz) % size[img - 1, 1],
                    rng.uniform(1, 200, n_nnz)], 1).astype(np.float32)
    perm = rng.permutation(n_nnz).astype(np.int32)
    layers = mcmain.load_net("random:1", "mb", "fast")
    t = train_mb.Trainer(np.zeros(16, np.float32), table[:1], nnz, perm, layers, n_pairs, dev)
    t.planes = torch.randn(total, device=dev)               # the store, resident
    t.table = train_mb.device_table(table, dev)
    _, _, opt, _ = train_mb.parse(["mb", "fast", "-a", "train_tr"])
    prm = torch.from_numpy(train_mb.draw_params(rng, opt, n_steps, n_pairs)).to(dev)
    src = torch.from_numpy(train_mb.draw_sources(rng, opt, img[perm[:n_steps * n_pairs]].reshape(n_steps, n_pairs), index)).to(dev)
    losses = torch.empty(n_steps, dtype=torch.float32, device=dev)
    w = args.warmup
    t.run(0, src[:w], prm[:w], opt.lr, opt.mom, opt.m, opt.pow, losses)
    hip_us = time_fn(lambda n: t.run(w * n_pairs, src[w:], prm[w:], opt.lr, opt.mom, opt.m, opt.pow, losses[w:]), args.steps)
    out = {"metric": "train_mb_step_us", "bs": args.bs, "hip_us_per_step": round(hip_us, 2), "store_gb": round(total * 4e-9, 2),
           "planes": int(table.shape[0]), "hip_loss_last": float(losses[-1].cpu()), "measured": ["hip_us_per_step", "torch_us_per_step"]}
    if not args.skip_torch:
        step = torch_step_fn(layers, opt.lr, opt.mom, opt.m)
        x = torch.randn((2 * args.bs, 1, 11, 11), device=dev)

        def run_torch(n):
            for _ in range(n):
                step(x)
        run_torch(args.warmup)
        out["torch_us_per_step"] = round(time_fn(run_torch, args.steps), 2)
        out["hip_speedup_vs_torch"] = round(out["torch_us_per_step"] / hip_us, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
