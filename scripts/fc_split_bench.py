#!/usr/bin/env python3
"""mc_fc_stack (fp32 MFMA) against mc_fc_split_stack (three bf16 MFMAs per product) on one MI355X, at the two full sizes of arch slow:

    scripts/fc_split_bench.py [--out profiles/fc_split_bench.txt] [--runs 5] [--warmup 1]

Per shape: seeded features and weights, `--warmup` untimed calls of each, then the two calls alternating, `--runs` timed calls each
between device events.  Per call: the median, the spread (min .. max), TFLOP/s by the algorithmic count (the reference's 2 flops per
weight and voxel, DESIGN.md section 4: 1.06 MFLOP per voxel at three hidden layers) and that rate's
share of the fp32-MFMA peak (the fp32 call) or of 1/3 of the bf16 peak (the split call's ceiling: three bf16 products per product, 16/3 of
the fp32-MFMA peak) and of 3/16 of the bf16 peak (three times the fp32-MFMA peak).  Then the max |difference| of
the two calls' volumes, and the gate: the split call's median at the KITTI shape is at most half the fp32 call's.  Exit status 1 if
the gate is missed."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_PEAK, FP32_MFMA_PEAK = 2516.6, 157.3      # dense TFLOP/s of the MI355X matrix cores
SHAPES = (("kitti", 112, 370, 1226, 228, 3), ("mb", 112, 1000, 1500, 200, 2))   # name, C, H, W, D, n_hidden


def make_layers(C, n_hidden, seed):
    rng = np.random.default_rng(seed)
    dims = [2 * C] + [384] * (n_hidden + 1) + [1]
    layers = []
    for i in range(len(dims) - 1):
        bound = (1.0 if i < len(dims) - 2 else 6.0) / np.sqrt(dims[i])
        layers.append((rng.uniform(-bound, bound, (dims[i + 1], dims[i])).astype(np.float32),
                       rng.uniform(-bound, bound, (dims[i + 1],)).astype(np.float32)))
    return layers


def voxels(H, W, D):
    return H * sum(W - d for d in range(min(D, W)))


def flops_per_voxel(C, n_hidden):
    """the reference's count (main.lua:958-983), as bench.py takes it: 2 flops per weight of every layer, layer 1 as a 2C -> 384 product"""
    dims = [2 * C] + [384] * (n_hidden + 1) + [1]
    return 2 * sum(dims[i] * dims[i + 1] for i in range(len(dims) - 1))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_split_bench.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="kitti,mb")
    a = ap.parse_args(argv)
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import _fc_split_lib
    from mc_cnn_amd._lib import lib
    from mc_cnn_amd.fc import fc_cost_volumes
    dev = torch.device("cuda", 0)
    lines = ["fc_split_bench: %s, %d timed runs per call after %d warm-up, alternating, device events" % (
        torch.cuda.get_device_name(0), a.runs, a.warmup)]
    gate = None
    for name, C, H, W, D, n_hidden in SHAPES:
        if name not in a.shapes.split(","):
            continue
        g = torch.Generator(device="cpu").manual_seed(11)
        feat = torch.relu(torch.randn((2, C, H, W), generator=g)).mul_(0.3).to(dev)
        layers = [(torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)) for w, b in make_layers(C, n_hidden, 7)]
        need = max(lib.mc_fc_stack_workspace_bytes(C, n_hidden + 2, H, W), _fc_split_lib.load().mc_fc_split_workspace_bytes(C, n_hidden + 2, H, W))
        ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        times, out = {"fp32": [], "bf16x3": []}, {}
        for it in range(a.warmup + a.runs):
            for mode in ("fp32", "bf16x3"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                vl, vr = fc_cost_volumes(feat, layers, D, workspace=ws, mode=mode)
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[mode].append(e0.elapsed_time(e1))
                out[mode] = vl
                del vr
        ok = ~torch.isnan(out["fp32"])
        same_mask = bool(torch.equal(ok, ~torch.isnan(out["bf16x3"])))
        diff = float((out["fp32"][ok] - out["bf16x3"][ok]).abs().max())
        spread = float(out["fp32"][ok].std())
        flop = voxels(H, W, D) * flops_per_voxel(C, n_hidden)
        lines.append("%s: C %d, %d x %d x %d, n_hidden %d: %.3e voxels, %.1f TFLOP" % (name, C, H, W, D, n_hidden, voxels(H, W, D), flop / 1e12))
        med = {}
        for mode in ("fp32", "bf16x3"):
            t = times[mode]
            med[mode] = statistics.median(t)
            tf = flop / (med[mode] * 1e-3) / 1e12
            share = "%.2f of the fp32-MFMA peak %.1f" % (tf / FP32_MFMA_PEAK, FP32_MFMA_PEAK) if mode == "fp32" else \
                "%.2f of 1/3 of the bf16 peak (%.1f), %.2f of 3/16 of it (%.1f)" % (tf / (BF16_PEAK / 3), BF16_PEAK / 3, tf / (BF16_PEAK * 3 / 16),
                                                                                     BF16_PEAK * 3 / 16)
            lines.append("  %-7s median %9.3f ms  (min %9.3f, max %9.3f)  %7.1f TFLOP/s  %s" % (mode, med[mode], min(t), max(t), tf, share))
        lines.append("  fp32 / bf16x3 medians: %.2f; max |fp32 - bf16x3| = %.3g (outputs' std %.3g, NaN masks %s)" % (
            med["fp32"] / med["bf16x3"], diff, spread, "identical" if same_mask else "DIFFER"))
        if name == "kitti":
            gate = med["bf16x3"] <= 0.5 * med["fp32"]
            lines.append("  gate (bf16x3 median <= 1/2 fp32 median at the KITTI shape): %s" % ("met" if gate else "MISSED"))
        del out, ws, feat
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if gate is not False else 1


if __name__ == "__main__":
    sys.exit(main())
