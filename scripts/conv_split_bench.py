#!/usr/bin/env python3
"""mc_conv3x3 (fp32 MFMA) against mc_conv_split (three bf16 MFMAs per product) on one MI355X, at the inner layers of the four nets:

    scripts/conv_split_bench.py [--out profiles/conv_split_bench.txt] [--runs 5] [--warmup 1] [--no-pair]

Per shape: seeded inputs and weights, `--warmup` untimed calls of each, then the two calls alternating, `--runs` timed calls each
between device events.  Per call: the median, the spread (min .. max), TFLOP/s by the 2 N H W Cin Cout 9 count and that rate's share
of the fp32-MFMA peak (the fp32 call) or of 1/3 of the bf16 peak (the split call's ceiling).  Then max |fp32 - bf16x3| over the outputs.
The gate: at the 64 -> 64 KITTI shape the split call's median is below the fp32 call's minimum.  Then a KITTI pair from the images
(features_fast + stereo_predict_fused on a resident Workspace, 370 x 1226 x 228) as ms per pair under both modes, one pair at a time
and two in flight on two streams, with max |fp32 - bf16x3| over the features, and `-a test_te` on the tests' synthetic KITTI set under both
modes.  Exit status 1 if the gate is missed."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BF16_PEAK, FP32_MFMA_PEAK = 2516.6, 157.3      # dense TFLOP/s of the MI355X matrix cores
SHAPES = (("kitti fast", 2, 64, 64, 370, 1226), ("kitti slow", 2, 112, 112, 370, 1226),
          ("mb fast", 2, 64, 64, 1000, 1500), ("mb slow", 2, 112, 112, 1000, 1500))   # name, N, Cin, Cout, H, W


def pair_from_images(torch, dev, runs, warmup, lines):
    from mc_cnn_amd import main as mcmain
    from mc_cnn_amd.params import TABLES
    from mc_cnn_amd.predict import Workspace, stereo_predict_fused
    H, W, D = 370, 1226, 228
    layers = mcmain.device_layers(mcmain.load_net("random:3", "kitti", "fast"), dev)
    prm = dict(TABLES[("kitti", "fast")])
    prm["border_n"] = len(layers)
    g = torch.Generator(device="cpu").manual_seed(5)
    xs = [torch.randn((2, 1, H, W), generator=g).to(dev) for _ in range(2)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    wss = [Workspace(prm, D, H, W, dev) for _ in range(2)]
    fa, fb = mcmain.features_fast(xs[0], layers, "fp32"), mcmain.features_fast(xs[0], layers, "bf16x3")
    lines.append("KITTI pair from the images, %d x %d x %d, random:3: max |fp32 - bf16x3| over the unit-norm features %.3g" % (
        H, W, D, float((fa - fb).abs().max())))
    del fa, fb

    def one(k, mode):
        with torch.cuda.stream(streams[k]):
            stereo_predict_fused(xs[k], prm, D, feat=mcmain.features_fast(xs[k], layers, mode), workspace=wss[k])
    for K in (1, 2):
        times = {"fp32": [], "bf16x3": []}
        for it in range(warmup + runs):
            for mode in ("fp32", "bf16x3"):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for s in streams[:K]:
                    s.wait_event(e0)
                for k in range(K):
                    one(k, mode)
                for s in streams[:K]:
                    torch.cuda.current_stream().wait_stream(s)
                e1.record()
                e1.synchronize()
                if it >= warmup:
                    times[mode].append(e0.elapsed_time(e1) / K)
        for mode in ("fp32", "bf16x3"):
            t = times[mode]
            lines.append("  %d in flight, %-7s median %7.3f ms per pair  (min %7.3f, max %7.3f)" % (K, mode, statistics.median(t), min(t), max(t)))


def synthetic_test_te(torch, lines):
    """`main.py kitti fast -a test_te` on the tests' synthetic KITTI set (tests/train_fixtures.py) under both modes: the error each prints,
    and the pixels of the test images whose disparity differs by more than 0.5 px between the modes.  A record, not a bar."""
    import contextlib
    import io
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from train_fixtures import write_synthetic_kitti
    from mc_cnn_amd import main as mcmain
    from mc_cnn_amd import predict
    kept, orig = [], predict.stereo_predict_fused

    def keeping(*a, **k):
        res = orig(*a, **k)
        kept.append(res["disp"].detach().clone())
        return res
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        write_synthetic_kitti(os.path.join(d, "data.kitti"))
        os.chdir(d)
        predict.stereo_predict_fused = keeping
        try:
            errs, disps = {}, {}
            for mode in ("fp32", "bf16x3"):
                del kept[:]
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    mcmain.main(["kitti", "fast", "-a", "test_te", "-net_fname", "random:3", "-disp_max", "32", "-conv_mode", mode])
                errs[mode], disps[mode] = float(buf.getvalue().strip().splitlines()[-1]), list(kept)
        finally:
            predict.stereo_predict_fused = orig
            os.chdir(cwd)
    moved = sum(int(((a - b).abs() > 0.5).sum()) for a, b in zip(disps["fp32"], disps["bf16x3"]))
    total = sum(a.numel() for a in disps["fp32"])
    lines.append("synthetic KITTI set, kitti fast -a test_te, random:3, disp_max 32: error fp32 %r, bf16x3 %r; %d of %d pixels of the %d test "
                 "images differ by more than 0.5 px" % (errs["fp32"], errs["bf16x3"], moved, total, len(disps["fp32"])))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_split_bench.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-pair", action="store_true", help="leave out the pair from the images")
    a = ap.parse_args(argv)
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import adcensus
    dev = torch.device("cuda", 0)
    lines = ["conv_split_bench: %s, %d timed runs per call after %d warm-up, alternating, device events" % (
        torch.cuda.get_device_name(0), a.runs, a.warmup)]
    gate = None
    for name, N, Cin, Cout, H, W in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(11)
        x = torch.randn((N, Cin, H, W), generator=g).to(dev)
        bound = 1.0 / np.sqrt(9 * Cin)
        w = ((torch.rand((Cout, Cin, 3, 3), generator=g) * 2 - 1) * bound).to(dev)
        b = ((torch.rand((Cout,), generator=g) * 2 - 1) * bound).to(dev)
        out = {m: torch.empty((N, Cout, H, W), dtype=torch.float32, device=dev) for m in ("fp32", "bf16x3")}
        times = {"fp32": [], "bf16x3": []}
        for it in range(a.warmup + a.runs):
            for mode in ("fp32", "bf16x3"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                adcensus.conv3x3(x, w, b, True, out=out[mode], mode=mode)
                e1.record()
                e1.synchronize()
                if it >= a.warmup:
                    times[mode].append(e0.elapsed_time(e1))
        diff, scale = float((out["fp32"] - out["bf16x3"]).abs().max()), float(out["fp32"].abs().max())
        flop = 2.0 * N * H * W * Cin * Cout * 9
        lines.append("%s: %d x (%d -> %d) x %d x %d, ReLU: %.1f GFLOP" % (name, N, Cin, Cout, H, W, flop / 1e9))
        med = {}
        for mode in ("fp32", "bf16x3"):
            t = times[mode]
            med[mode] = statistics.median(t)
            tf = flop / (med[mode] * 1e-3) / 1e12
            share = "%.2f of the fp32-MFMA peak %.1f" % (tf / FP32_MFMA_PEAK, FP32_MFMA_PEAK) if mode == "fp32" else \
                "%.2f of 1/3 of the bf16 peak (%.1f)" % (tf / (BF16_PEAK / 3), BF16_PEAK / 3)
            lines.append("  %-7s median %8.3f ms  (min %8.3f, max %8.3f)  %7.1f TFLOP/s  %s" % (mode, med[mode], min(t), max(t), tf, share))
        lines.append("  fp32 / bf16x3 medians: %.2f; max |fp32 - bf16x3| = %.3g (output scale %.3g)" % (med["fp32"] / med["bf16x3"], diff, scale))
        if name == "kitti fast":
            gate = med["bf16x3"] < min(times["fp32"])
            lines.append("  gate (bf16x3 median below the fp32 minimum at the 64 -> 64 KITTI shape): %s" % ("met" if gate else "MISSED"))
        del out, x
        torch.cuda.empty_cache()
    if not a.no_pair:
        pair_from_images(torch, dev, a.runs, a.warmup, lines)
        synthetic_test_te(torch, lines)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if gate is not False else 1


if __name__ == "__main__":
    sys.exit(main())
