"""Wall time of `preprocess_kitti` (preprocess_kitti.lua) on a full-size synthetic KITTI tree: 194 + 195 grey pairs for
2012 and 200 + 200 RGB pairs for 2015 at KITTI's image sizes (textured scenes with known disparities, tests/
preprocess_oracle.py), split into the host stages (PNG decode, normalisation, writing the eight arrays) and the GPU stages
(upload, filters, pixel lists; device events).

    python scripts/preprocess_bench.py --dir /tmp/kitti_tree [--years 2012 2015] [--keep]

The tree is written once (kept if present).  The written arrays (~3 GB for both sets) are deleted after each set unless
--keep.  Prints one JSON line per set.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True)
    ap.add_argument("--years", type=int, nargs="+", default=[2012, 2015])
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()
    import torch

    import preprocess_oracle as po
    from mc_cnn_amd import preprocess_kitti as pk
    assert torch.cuda.is_available(), "preprocess_bench measures the GPU stages: it needs a GPU"
    for year in args.years:
        s = pk.SETS[year]
        marker = os.path.join(args.dir, s["path"], "unzip", "complete")
        if not os.path.exists(marker):
            t0 = time.perf_counter()
            po.write_tree(args.dir, year, s["n_tr"], s["n_te"], seed=year, textured=True, noise=1.0, block=(16, 16))
            open(marker, "w").close()
            print("wrote the %d tree in %.1f s" % (year, time.perf_counter() - t0), file=sys.stderr)
    pk.gpu_stages(*_warm())   # loads libmctrain.so and the kernels' code objects
    for year in args.years:
        s = pk.SETS[year]
        t0 = time.perf_counter()
        out = pk.preprocess_set(year, s["n_tr"], s["n_te"], root=args.dir)
        wall = time.perf_counter() - t0
        t = pk.last_timing[year]
        rec = {"set": year, "pairs": s["n_tr"] + s["n_te"], "wall_s": round(wall, 3),
               "nnz_tr": int(out["nnz_tr"].shape[0]), "nnz_te": int(out["nnz_te"].shape[0])}
        rec.update({k + "_s": round(v, 4) for k, v in t.items()})
        rec["host_s"] = round(t["decode"] + t["normalize"] + t["write"], 3)
        rec["gpu_s"] = round(t["gpu_upload"] + t["gpu_filter"] + t["gpu_lists"], 4)
        print(json.dumps(rec), flush=True)
        if not args.keep:
            for k in pk.OUTPUTS:
                for ext in ("", ".dim", ".type"):
                    os.remove(os.path.join(args.dir, s["path"], k + ".bin" + ext))


def _warm():
    import numpy as np
    d = np.zeros((2, 1, 8, 16), np.float32)
    d[:, :, :, 4:] = 2
    return d, np.zeros_like(d), np.array([1], np.int64)


if __name__ == "__main__":
    main()
