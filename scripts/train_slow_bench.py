"""Step time of the accurate architecture's training (libmctrainslow.so, mc_train_slow_run) at KITTI shape, against a torch
autograd step of the same net on the same GPU and batch -- scripts/train_bench.py for arch slow.

    python scripts/train_slow_bench.py [--steps 200] [--warmup 20] [--bs 128]

* HIP: `mc_train_slow_run` -- patch sampling from a KITTI-sized synthetic dataset on the device (389 pairs of 350 x 1242),
  forward, BCECriterion2, backward and momentum SGD -- twelve kernels per step, timed with HIP events over --steps steps.
* torch: F.conv2d (MIOpen) and F.linear (rocBLAS / hipBLASLt) forward of the reference's 4-patch batch, BCECriterion2
  written in torch, autograd backward, momentum SGD written out.  Its patches are given (no sampling): the torch number is a
  lower bound of a full torch step.

For the per-kernel breakdown run it under `rocprofv3 --kernel-trace --stats -- python scripts/train_slow_bench.py
--skip-torch` (no counters in that run).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_step_fn(conv, fc, lr, mom):
    import torch
    import torch.nn.functional as F
    ps = [torch.tensor(a, device="cuda", requires_grad=True) for wb in conv + fc for a in wb]
    vs = [torch.zeros_like(p) for p in ps]
    eps = 1e-12

    def step(x):   # x: (4 n, 1, 9, 9) in the reference's order L, P, L, N
        for p in ps:
            p.grad = None
        h = x
        for i in range(4):
            h = F.relu(F.conv2d(h, ps[2 * i], ps[2 * i + 1]))
        h = h.reshape(x.shape[0] // 2, -1)
        for i in range(4, 9):
            h = F.linear(h, ps[2 * i], ps[2 * i + 1])
            if i < 8:
                h = F.relu(h)
        o = torch.sigmoid(h.reshape(-1))
        t = torch.arange(o.numel(), device=o.device).remainder(2).to(o.dtype)
        loss = -(torch.log(o + eps) * t + torch.log((1 - o) + eps) * (1 - t)).mean()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import train_slow as ts

    dev = torch.device("cuda", 0)
    n_img, H, W = 389, 350, 1242
    n_pairs = args.bs // 2
    n_steps = args.warmup + args.steps
    rng = np.random.default_rng(0)
    n_nnz = 1_000_000
    nnz = np.stack([rng.integers(1, n_img + 1, n_nnz), rng.integers(0, H, n_nnz), rng.integers(0, W, n_nnz),
                    rng.uniform(1, 200, n_nnz)], 1).astype(np.float32)
    perm = rng.permutation(n_nnz).astype(np.int32)
    conv, fc = ts.init_net(1, gain=6 ** 0.5)
    tiny = np.zeros((1, 4, 4), np.float32)
    t = ts.Trainer(tiny, tiny, nnz, perm, conv, fc, n_pairs, dev)
    t.x0 = torch.randn((n_img, H, W), device=dev)          # KITTI-sized images, resident
    t.x1 = torch.randn((n_img, H, W), device=dev)
    t.n_img, t.H, t.W = n_img, H, W
    _, _, opt, _ = ts.parse(["kitti", "slow", "-a", "train_tr"])
    prm = torch.from_numpy(ts.draw_params(rng, opt, n_steps, n_pairs)).to(dev)
    losses = torch.empty(n_steps, dtype=torch.float32, device=dev)
    t.run(0, prm[:args.warmup], opt.lr, opt.mom, losses)
    hip_us = time_fn(lambda n: t.run(args.warmup * n_pairs, prm[args.warmup:], opt.lr, opt.mom, losses[args.warmup:]), args.steps)
    out = {"metric": "train_slow_step_us", "bs": args.bs, "launches_per_step": 12, "hip_us_per_step": round(hip_us, 2),
           "hip_loss_last": float(losses[-1].cpu()), "measured": ["hip_us_per_step", "torch_us_per_step"]}
    if not args.skip_torch:
        step = torch_step_fn(conv, fc, opt.lr, opt.mom)
        x = torch.randn((2 * args.bs, 1, 9, 9), device=dev)

        def run_torch(n):
            for _ in range(n):
                step(x)
        run_torch(args.warmup)
        out["torch_us_per_step"] = round(time_fn(run_torch, args.steps), 2)
        out["hip_speedup_vs_torch"] = round(out["torch_us_per_step"] / hip_us, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
