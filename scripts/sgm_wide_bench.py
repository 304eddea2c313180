#!/usr/bin/env python3
"""mc_sgm2 at a disparity range of 1024 (the line walk at 16 values per lane) beside 512 (8 per lane) on one MI355X, at KITTI's image size:

    scripts/sgm_wide_bench.py [--out profiles/sgm_wide_bench.txt] [--runs 7] [--warmup 2] [--ranges 1024 512] [--predict 400 512]

Per range: a seeded 370 x 1226 x D volume with the left volume's NaN triangle, `--warmup` untimed calls, then `--runs` timed calls between
device events, the two ranges alternating.  A call is the map kernel and the four sweeps (MODE 1: each reads the costs and the running sum
and writes the sum, 3 x 4 bytes per voxel and sweep); the line gives the median, the spread (min .. max), the bytes per second by that
count and ns per voxel.  The last line is the per-voxel ratio of the two medians (where both 1024 and 512 are timed).  A record, not a bar.
`--ranges 512` times the narrower walk alone: what a build from before the range grew can run too, for an A/B of the kernels both have.
`--predict D ...` adds the fused schedule's kernels: mc_predict at 370 x 1226 x D on a resident workspace, from 64-channel features with the
kitti fast parameters (the fused horizontal pair, the down sweep, the up sweep with the arg-min) and from raw volumes with the kitti ad
parameters and one CBCA-2 pass (the up sweep without the arg-min), ms per call in the same way."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 370, 1226
RANGES = (1024, 512)
PRM = (4.0, 55.72, 0.02, 1.5, 3.0, 2.5)   # kitti fast: pi1, pi2, tau_so, alpha1, q1, q2


def predict_lines(torch, dev, ranges, runs, warmup):
    import mc_cnn_amd as mc
    from mc_cnn_amd.predict import Workspace
    g = torch.Generator(device="cuda").manual_seed(5)
    xb = torch.randn((2, 1, H, W), device=dev, generator=g)
    lines = ["mc_predict at %d x %d, resident workspace, %d timed calls after %d warm-up, device events" % (H, W, runs, warmup)]
    for D in ranges:
        f = torch.randn((2, 64, H, W), device=dev, generator=g)
        f = (f / torch.sqrt((f * f).sum(1, keepdim=True) + 1e-5)).contiguous()
        d, x = torch.arange(D, device=dev)[:, None, None], torch.arange(W, device=dev)[None, None, :]
        raw = (torch.rand((1, D, H, W), device=dev, generator=g).masked_fill_((d > x)[None], float("nan")),
               torch.rand((1, D, H, W), device=dev, generator=g).masked_fill_((x + d >= W)[None], float("nan")))
        ad = dict(mc.PRESETS["kitti_ad"])
        ad["cbca_i2"] = 1
        for name, prm, kw in (("kitti fast from features", dict(mc.PRESETS["kitti_fast"]), dict(feat=f)), ("kitti ad, one CBCA-2 pass, from raw volumes", ad, dict(raw=raw))):
            ws = Workspace(prm, D, H, W, dev)
            out = torch.empty((1, 1, H, W), dtype=torch.float32, device=dev)
            t = []
            for it in range(warmup + runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mc.stereo_predict_fused(xb, prm, D, workspace=ws, out=out, **kw)
                e1.record()
                e1.synchronize()
                if it >= warmup:
                    t.append(e0.elapsed_time(e1))
            lines.append("  D = %4d, %-44s median %8.3f ms  (min %8.3f, max %8.3f)" % (D, name + ":", statistics.median(t), min(t), max(t)))
            del ws
        del f, raw
        torch.cuda.empty_cache()
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm_wide_bench.txt"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ranges", type=int, nargs="*", default=list(RANGES))
    ap.add_argument("--predict", type=int, nargs="*", default=[], help="ranges at which mc_predict is timed too")
    a = ap.parse_args(argv)
    ranges = tuple(a.ranges)
    import torch
    import mc_cnn_amd  # noqa: F401
    from mc_cnn_amd import adcensus
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cuda").manual_seed(3)
    x0 = torch.rand((H, W), device=dev, generator=g)
    x1 = torch.roll(x0, -9, dims=1) + 0.02 * torch.rand((H, W), device=dev, generator=g)
    vols, outs = {}, {}
    for D in ranges:
        v = torch.rand((1, H, W, D), device=dev, generator=g)
        v.masked_fill_(torch.arange(D, device=dev)[None, None, None, :] > torch.arange(W, device=dev)[None, None, :, None], float("nan"))
        vols[D], outs[D] = v, torch.zeros_like(v)
    times = {D: [] for D in ranges}
    for it in range(a.warmup + a.runs):
        for D in ranges:
            outs[D].zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            adcensus.sgm2(x0, x1, vols[D], outs[D], None, *PRM, -1)
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[D].append(e0.elapsed_time(e1))
    lines = ["sgm_wide_bench: %s, mc_sgm2 (map kernel + four sweeps) at %d x %d, %d timed calls per range after %d warm-up, alternating, device events" % (
        torch.cuda.get_device_name(0), H, W, a.runs, a.warmup)]
    med = {}
    for D in ranges:
        t = times[D]
        med[D] = statistics.median(t)
        vox = H * W * D
        lines.append("  D = %4d (%2d values per lane): median %8.3f ms  (min %8.3f, max %8.3f)  %6.2f TB/s at 48 bytes per voxel  %.4f ns per voxel" % (
            D, 16 if D > 512 else 8, med[D], min(t), max(t), 48.0 * vox / (med[D] * 1e-3) / 1e12, med[D] * 1e6 / vox))
    if 1024 in med and 512 in med:
        lines.append("  per-voxel time at D = 1024 over D = 512: %.3f" % ((med[1024] / 1024) / (med[512] / 512)))
    del vols, outs
    torch.cuda.empty_cache()
    if a.predict:
        lines += predict_lines(torch, dev, a.predict, a.runs, a.warmup)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
