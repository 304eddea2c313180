#!/usr/bin/env python
"""What the mismatch ray walk meets on the headline workload (no GPU): the CPU oracle on bench.py's own inputs (sample_pair,
features(64, 370, 1226, seed=42), preset kitti_fast) up to the LR check, then the 16 rays of every mismatch pixel walked as
adcensus.cu:1001-1058 walks them.  Prints the outlier classes, the ray lengths and what a wave of 64 rays costs in rounds of 4
positions when it waits for its longest ray against what it costs with its lanes kept full.

  python scripts/mismatch_walk_stats.py [H W D C]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import cpu_oracle  # noqa: E402
from util import features, sample_pair  # noqa: E402
from mc_cnn_amd.params import PRESETS  # noqa: E402

H, W, D, C = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (370, 1226, 228, 64)
cpu_oracle.build()
x0, x1 = sample_pair(H, W)
f = features(C, H, W, seed=42)
o = cpu_oracle.stereo_predict(dict(PRESETS["kitti_fast"], sm_terminate="occlusion"), x0, x1, D, featL=f[0], featR=f[1])["outlier"]
print("outlier classes 0 / 1 / 2: %.1f %% / %.1f %% / %.1f %%" % tuple(100 * (o == k).mean() for k in (0, 1, 2)))
mis = np.pad(o == 2, 1)   # a border of "not a mismatch": a ray stops there at the latest
dx = [0, -.5, -1, -1, -1, -1, -1, -.5, 0, .5, 1, 1, 1, 1, 1, .5]
dy = [1, 1, 1, .5, 0, -.5, -1, -1, -1, -1, -1, -.5, 0, .5, 1, 1]
ys, xs = np.nonzero(o == 2)
steps = np.zeros((16, ys.size), np.int32)
for k in range(16):
    xx, yy = xs.astype(np.float64), ys.astype(np.float64)
    live = np.ones(ys.size, bool)
    while live.any():
        xx[live] += dx[k]
        yy[live] += dy[k]
        steps[k, live] += 1
        xi = np.clip(np.floor(np.abs(xx) + 0.5) * np.sign(xx), -1, W).astype(int)   # round half away from zero
        yi = np.clip(np.floor(np.abs(yy) + 0.5) * np.sign(yy), -1, H).astype(int)
        live &= mis[yi + 1, xi + 1]
longest = steps.max(0)
print("ray length: mean %.1f steps; a pixel's longest ray: mean %.1f, p95 %d, max %d" % (steps.mean(), longest.mean(), np.percentile(longest, 95), longest.max()))
rounds = (steps + 3) // 4
n4 = ys.size // 4 * 4       # waves of 4 pixels x 16 rays, in pixel order
wave = rounds[:, :n4].reshape(16, -1, 4).max((0, 2))
print("rounds of 4 positions per wave of 64 rays: %.2f waiting for the longest ray, %.2f with full lanes" % (wave.mean(), rounds[:, :n4].mean()))
