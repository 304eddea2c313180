#!/usr/bin/env python3
"""Candidates per second of the parameter search (mc_cnn_amd/hs.py) on a device-resident test set, against what the search would
cost through `main.run` + `train.evaluate` per candidate.

    python scripts/hs_bench.py [--out FILE] [--pairs 40] [--arch fast slow] [--candidates 8] [--rounds 3] [--fc_mode fp32|bf16x3] [--setup_only]

The set is synthetic and KITTI-sized: --pairs test pairs of 350 x 1242 (read 1224 .. 1242 wide, as KITTI's images are), disp_max 228,
textured scenes with piecewise-constant disparity, ground truth known on two thirds of the pixels, seeded random nets.  The nets
match badly, so the SCORES mean nothing; the work per candidate is that of a real set.

Per arch, in one process:
  * EvalSet's set-up (the cost stage of every pair, once) and its resident bytes;
  * candidates per second of `EvalSet.score` at in_flight 1 / 2 / 3, interleaved over --rounds rounds (median and best), for
      full        random grid points, reuse off: 40 x (mc_predict + mc_eval_error), one synchronise, one read-back
      full+keep   the same candidates with reuse on: mc_predict ends at the median, the blur is a launch of its own
      blur-only   candidates that differ from the held one in blur_sigma / blur_t only (reuse on): 40 x (mean2d + mc_eval_error)
  * the baseline: `train.evaluate` with the `run` main.main builds for the arch (cost stage recomputed, per-pair synchronise, .cpu()
    and numpy error), for the same candidates, and that its mean equals EvalSet's bit for bit;
  * mc_eval_error's time per call at 350 x 1226 against a 1242-wide ground truth (device events around back-to-back launches).
Times are host clocks around work that ends in a device synchronise.  --fc_mode is hs.py's -fc_mode for arch slow (the cost stage's FC
stack); --setup_only stops an arch after its set-up line.
"""
import argparse
import contextlib
import io
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, D = 350, 1242, 228
WIDTHS = (1242, 1226, 1238, 1224)


def synthetic_set(n, seed=0):
    """What train.load_data returns for a set of n test pairs (and no training pair)."""
    rng = np.random.default_rng(seed)
    x0 = np.empty((n, 1, H, W), np.float32)
    x1 = np.empty_like(x0)
    disp = np.zeros((n, 1, H, W), np.float32)
    cols = np.arange(W)[None, :]
    for i in range(n):
        r = rng.standard_normal((H, W + 256)).astype(np.float32)
        r = (r + np.roll(r, 1, 0) + np.roll(r, 1, 1) + np.roll(r, (1, 1), (0, 1))) / 2
        d = np.repeat(rng.integers(8, 200, 7), H // 7)[:H][:, None] * np.ones((1, W), np.int64)
        x1[i, 0] = r[:, 256:] + 0.3 * rng.standard_normal((H, W)).astype(np.float32)
        x0[i, 0] = np.take_along_axis(r, 256 + cols - d, 1)
        known = (cols - d >= 0) & (rng.uniform(size=(H, W)) < 0.67)
        disp[i, 0] = np.where(known, d, 0)
    meta = np.array([[H, WIDTHS[i % len(WIDTHS)], i] for i in range(n)], np.int32)
    return dict(x0=x0, x1=x1, dispnoc=disp, metadata=meta, tr=np.zeros(0, np.int32), te=np.arange(1, n + 1, dtype=np.int32))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_arch(arch, data, a, say):
    import torch
    from mc_cnn_amd import hs, main, train
    from mc_cnn_amd.evalset import EvalSet
    from mc_cnn_amd.predict import stereo_predict_fused
    dev = torch.device("cuda", 0)
    net = "random:3"
    fc_mode = a.fc_mode if arch == "slow" else "fp32"
    opt = hs.parse(["random", "kitti", arch, "test_te", net, "-disp_max", str(D), "-fc_mode", fc_mode])
    layers, fc = hs.check_net(net, "kitti", arch)
    grid = hs.grid_of("kitti", arch)
    t_setup, es = timed(lambda: EvalSet("kitti", arch, opt, layers, fc, dev, 48 << 30, data=data))
    held = 4 * sum(e["H"] * e["W"] for e in es.examples)
    say("%s%s: set-up %.2f s; resident: cost stage %.2f GB (%d of %d pairs), post-median maps %.3f GB"
        % (arch, "" if fc_mode == "fp32" else " -fc_mode " + fc_mode, t_setup, es.resident_bytes / 1e9, es.n_cached, es.n, held / 1e9))
    if a.setup_only:
        return
    rng = random.Random(7)
    cands = []
    while len(cands) < a.candidates:
        ps = {name: rng.choice(values) for name, values in grid}
        if hs.valid(ps) and ps not in cands:
            cands.append(ps)
    blurs = [(s, t) for s in dict(grid)["blur_sigma"] for t in dict(grid)["blur_t"]]
    rng.shuffle(blurs)
    blurs = blurs[:a.candidates]
    es.score(dict(es.prm, **cands[0]))                 # warm-up: code objects, workspaces, the three streams
    for k in (1, 2, 3):
        es.score(dict(es.prm, **cands[1]), in_flight=k)
    for s, _ in blurs:
        es._gaussian(s)
    rates = {}

    def run_mode(mode, k):
        if mode == "blur-only":
            es.reuse = True
            es.score(dict(es.prm, **cands[0]), in_flight=k)       # holds cands[0]'s maps (not timed)
            todo = [dict(dict(es.prm, **cands[0]), blur_sigma=s, blur_t=t) for s, t in blurs]
        else:
            es.reuse = mode == "full+keep"
            todo = [dict(es.prm, **ps) for ps in cands]
            if es.reuse:
                es.score(dict(dict(es.prm, **cands[-1]), tau_so=0.5), in_flight=k)   # not timed: the held maps are no candidate's of todo
        before = es.n_predict_calls
        t, scores = timed(lambda: [es.score(p, in_flight=k) for p in todo])
        assert es.n_predict_calls - before == (0 if mode == "blur-only" else es.n * len(todo))
        rates.setdefault((mode, k), []).append(len(todo) / t)
        return scores

    ref = None
    for _ in range(a.rounds):
        for k in (1, 2, 3):
            for mode in ("full", "full+keep", "blur-only"):
                scores = run_mode(mode, k)
                if mode != "blur-only":
                    ref = ref or scores
                    assert scores == ref, "scores differ between modes"
    for mode in ("full", "full+keep", "blur-only"):
        for k in (1, 2, 3):
            r = rates[(mode, k)]
            say("%s: %-9s in_flight %d: %8.2f candidates/s median, %8.2f best of %d rounds x %d candidates"
                % (arch, mode, k, statistics.median(r), max(r), a.rounds, a.candidates))

    # the baseline: what the search costs through main.run + train.evaluate per candidate
    dl = main.device_layers(layers, dev)

    def baseline(ps):
        prm = dict(es.prm, **ps)

        def run(x_batch, Dm):
            if arch == "fast":
                return stereo_predict_fused(x_batch, prm, Dm, feat=main.features_fast(x_batch, dl))
            return stereo_predict_fused(x_batch, prm, Dm, raw=main.raw_volumes_slow(main.features_slow(x_batch, dl), fc, Dm, prm["border_n"], fc_mode=fc_mode))
        with contextlib.redirect_stdout(io.StringIO()):
            return train.evaluate("kitti", opt, run, dev, data=data)
    n_base = a.candidates if arch == "fast" else 1
    if arch == "fast":
        baseline(cands[0])                              # warm-up (arch slow's one candidate is half a minute of kernels already warm)
    t, means = timed(lambda: [baseline(ps) for ps in cands[:n_base]])
    assert means == ref[:n_base], "the baseline's means differ from EvalSet's: %r %r" % (means, ref[:n_base])
    best = max(statistics.median(rates[("full", k)]) for k in (1, 2, 3))
    say("%s: baseline (main.run + train.evaluate per candidate): %8.3f candidates/s over %d candidates; its means equal EvalSet's bit "
        "for bit; EvalSet full at its best in_flight is %.1f x that" % (arch, n_base / t, n_base, best / (n_base / t)))


def bench_kernel(say):
    import torch
    from mc_cnn_amd.evalset import eval_error
    rng = np.random.default_rng(1)
    w = 1226
    pred = torch.from_numpy(rng.uniform(0, 200, (H, w)).astype(np.float32)).cuda()
    actual = torch.from_numpy((rng.uniform(0, 200, (H, W)) * (rng.uniform(size=(H, W)) < 0.67)).astype(np.float32)).cuda()
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    reps = 500
    for _ in range(20):
        eval_error(pred, w, actual, W, H, w, 3, counts)
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            eval_error(pred, w, actual, W, H, w, 3, counts)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    say("mc_eval_error %d x %d (actual_ld %d): %.2f us per call, back-to-back launches between device events, best of 5 x %d (%.0f GB/s of "
        "the two maps)" % (H, w, W, best, reps, 2 * 4 * H * w / best / 1e3))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="")
    ap.add_argument("--pairs", type=int, default=40)
    ap.add_argument("--arch", nargs="+", default=["fast", "slow"], choices=["fast", "slow"])
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fc_mode", default="fp32", choices=["fp32", "bf16x3"], help="arch slow: hs.py's -fc_mode")
    ap.add_argument("--setup_only", action="store_true", help="per arch, the set-up line only")
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "hs_bench.py measures on the GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("hs_bench: %d pairs of %d x %d (read %s wide), disp_max %d, seeded random nets; %s"
        % (a.pairs, H, W, "/".join(map(str, WIDTHS)), D, torch.cuda.get_device_name(0)))
    data = synthetic_set(a.pairs)
    bench_kernel(say)
    for arch in a.arch:
        bench_arch(arch, data, a, say)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
