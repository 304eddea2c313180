"""What mc_predict_ex costs: ms per pair at bench.py's default workload (KITTI fast, 370 x 1226 x 228, its seeded pair and features) for
  (a) mc_predict of another build of libmcadcensus.so (--parent-lib: the commit before mc_predict_ex, built aside),
  (b) mc_predict of this tree,
  (c) mc_predict_ex of this tree with all three extra maps (outlier, cost, curvature).
--runs alternating runs of each (a, b, c, a, b, c, ...), each a warm-up and then --steps calls between two device synchronisations on
the host clock.  (b) is accepted against (a) if their medians differ by no more than the spread (max - min) of (a)'s own runs; (c) is
reported.  The three disparity maps are compared bit for bit first.  Needs a GPU; writes the report to --out and prints it.

    python scripts/predict_ex_bench.py --parent-lib /path/to/parent/libmcadcensus.so --out profiles/predict_ex_bench.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libmcadcensus.so of the commit to compare with; without it (a) is not measured")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="kitti_fast")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_ex_bench.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("predict_ex_bench: no GPU; a time measured anywhere else says nothing")
    import bench
    import mc_cnn_amd as mc
    from mc_cnn_amd.predict import Workspace

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    cfg = bench.CONFIGS[args.config]
    preset, H, W, D, Cn, name = cfg
    xb, kw, _ = bench.make_inputs(cfg, 0, device, bench.PAIR_OF[args.config])
    p = mc.make_params(dict(mc.PRESETS[preset]))
    ws = Workspace(p, D, H, W, device)
    feat = kw["feat"].contiguous()
    st = torch.cuda.current_stream().cuda_stream

    this = mc._lib.lib
    libs = {"b": this, "c": this}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        assert not hasattr(parent, "mc_predict_ex"), "--parent-lib is meant to be a build from before mc_predict_ex"
        parent.mc_predict.argtypes, parent.mc_predict.restype = this.mc_predict.argtypes, C.c_int
        parent.mc_last_error.restype = C.c_char_p
        libs["a"] = parent
    what = {"a": "mc_predict, parent build", "b": "mc_predict, this tree", "c": "mc_predict_ex with outlier, cost and curvature, this tree"}
    out = {k: torch.empty((1, 1, H, W), dtype=torch.float32, device=device) for k in libs}
    extras = [torch.empty((1, 1, H, W), dtype=torch.float32, device=device) for _ in range(3)]
    head = (C.byref(p), xb[0].data_ptr(), xb[1].data_ptr(), feat[0].data_ptr(), feat[1].data_ptr(), feat.shape[-3], None, None, D, H, W,
            ws.ptr, ws.nbytes_full, None, None, None, None)

    def call(k):
        if k == "c":
            rc = this.mc_predict_ex(*head, *(e.data_ptr() for e in extras), out[k].data_ptr(), st)
        else:
            rc = libs[k].mc_predict(*head, out[k].data_ptr(), st)
        if rc:
            raise RuntimeError("%s: rc=%d: %s" % (what[k], rc, libs[k].mc_last_error().decode()))

    def block(k, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    order = sorted(libs)
    for k in order:
        block(k, args.warmup)
    for k in order[1:]:
        assert torch.equal(out[k].view(torch.int32), out[order[0]].view(torch.int32)), "disp of (%s) differs from (%s)" % (k, order[0])
    ms = {k: [] for k in order}
    for _ in range(args.runs):
        for k in order:
            block(k, args.warmup)
            ms[k].append(block(k, args.steps))

    lines = ["predict_ex_bench: %s, %s; %d alternating runs of %d calls each (warm-up %d), host clock between device synchronisations"
             % (name, torch.cuda.get_device_name(device), args.runs, args.steps, args.warmup),
             "disparity maps of %s: bit-identical" % ", ".join("(%s)" % k for k in order)]
    for k in order:
        lines.append("(%s) %-58s ms per pair: %s  median %.4f  spread %.4f" % (
            k, what[k], " ".join("%.4f" % v for v in ms[k]), statistics.median(ms[k]), max(ms[k]) - min(ms[k])))
    if "a" in ms:
        spread = max(ms["a"]) - min(ms["a"])
        delta = statistics.median(ms["b"]) - statistics.median(ms["a"])
        lines.append("(b) - (a), medians: %+.4f ms; margin = spread of (a)'s own runs: %.4f ms -> %s" % (
            delta, spread, "inside" if abs(delta) <= spread else "OUTSIDE"))
    else:
        lines.append("(a) not measured: no --parent-lib")
    delta_c = statistics.median(ms["c"]) - statistics.median(ms["b"])
    lines.append("(c) - (b), medians: %+.4f ms (%+.2f %%), reported, not gated" % (delta_c, 100 * delta_c / statistics.median(ms["b"])))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
