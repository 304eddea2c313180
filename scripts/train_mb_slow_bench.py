"""Step time of Middlebury's accurate net's training (libmctrainmbslow.so, mc_train_mb_slow_run), against a torch autograd
step of the same net (five convolutions, four Linears) on the same GPU and batch.

    python scripts/train_mb_slow_bench.py [--steps 400] [--warmup 50] [--bs 128]

* HIP: `mc_train_mb_slow_run` -- patch sampling on the device from the ragged synthetic store of scripts/train_mb_bench.py
  (24 scenes between 480 x 640 and 1000 x 1500, 1 to 4 lights and 1 to 7 exposures each, two views per plane), forward,
  BCECriterion2, backward and momentum SGD -- ten kernels per step, timed with HIP events over --steps steps after --warmup
  steps.
* torch: F.conv2d (MIOpen) and F.linear (rocBLAS) forward of the reference's 4-patch batch of 11 x 11 patches, BCECriterion2
  written in torch, autograd backward, momentum SGD written out.  Its patches are given (no sampling): the torch number is a
  lower bound of a full torch step.

Prints one JSON line.  `--skip-torch` leaves the HIP steps alone in the process, for a kernel trace of the ten launches.
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


def torch_step_fn(conv, fc, lr, mom):
    import torch
    import torch.nn.functional as F
    ps = [torch.tensor(a, device="cuda", requires_grad=True) for wb in list(conv) + list(fc) for a in wb]
    vs = [torch.zeros_like(p) for p in ps]
    n_conv, n_fc = len(conv), len(fc)

    def step(x, target):   # x: (4 n, 1, 11, 11) in the reference's order L, P, L, N; target (2 n,): 0, 1, 0, 1, ...
        for p in ps:
            p.grad = None
        h = x
        for i in range(n_conv):
            h = F.relu(F.conv2d(h, ps[2 * i], ps[2 * i + 1]))
        h = h.reshape(x.shape[0] // 2, -1)
        for i in range(n_fc):
            h = F.linear(h, ps[2 * (n_conv + i)], ps[2 * (n_conv + i) + 1])
            if i < n_fc - 1:
                h = F.relu(h)
        o = torch.sigmoid(h.reshape(-1))
        loss = -((torch.log(o + 1e-12) * target + torch.log((1 - o) + 1e-12) * (1 - target)) / target.numel()).sum()
        loss.backward()
        with torch.no_grad():
            for p, v in zip(ps, vs):
                v.mul_(mom).add_(p.grad, alpha=-lr)
                p.add_(v)
        return loss
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--bs", type=int, default=128)
    ap.add_argument("--skip-torch", action="store_true")
    args = ap.parse_args()
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import train_mb, train_mb_slow

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
    conv, fc = train_mb_slow.init_net(1, gain=np.sqrt(6.0))   # wide weights: the ReLUs are half active, as in a trained net
    t = train_mb_slow.Trainer(np.zeros(16, np.float32), table[:1], nnz, perm, conv, fc, n_pairs, dev)
    t.planes = torch.randn(total, device=dev)               # the store, resident
    t.table = train_mb.device_table(table, dev)
    _, _, opt, _ = train_mb_slow.parse(["mb", "slow", "-a", "train_tr"])
    prm = torch.from_numpy(train_mb_slow.draw_params(rng, opt, n_steps, n_pairs)).to(dev)
    src = torch.from_numpy(train_mb_slow.draw_sources(rng, opt, img[perm[:n_steps * n_pairs]].reshape(n_steps, n_pairs), index)).to(dev)
    losses = torch.empty(n_steps, dtype=torch.float32, device=dev)
    w = args.warmup
    t.run(0, src[:w], prm[:w], opt.lr, opt.mom, losses)
    hip_us = time_fn(lambda n: t.run(w * n_pairs, src[w:], prm[w:], opt.lr, opt.mom, losses[w:]), args.steps)
    out = {"metric": "train_mb_slow_step_us", "bs": args.bs, "hip_us_per_step": round(hip_us, 2), "store_gb": round(total * 4e-9, 2),
           "planes": int(table.shape[0]), "workspace_mb": round(t.ws_bytes * 1e-6, 1), "hip_loss_last": float(losses[-1].cpu()),
           "measured": ["hip_us_per_step", "torch_us_per_step"]}
    if not args.skip_torch:
        step = torch_step_fn(conv, fc, opt.lr, opt.mom)
        x = torch.randn((2 * args.bs, 1, 11, 11), device=dev)
        target = torch.tensor([0.0, 1.0] * n_pairs, device=dev)

        def run_torch(n):
            for _ in range(n):
                step(x, target)
        run_torch(args.warmup)
        out["torch_us_per_step"] = round(time_fn(run_torch, args.steps), 2)
        out["hip_speedup_vs_torch"] = round(out["torch_us_per_step"] / hip_us, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
