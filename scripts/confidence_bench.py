"""What mc_cost_margins costs, and what the margins form of the arg-min kernels costs everyone else, at bench.py's default workload (KITTI
fast, 370 x 1226 x 228, its seeded pair and features):
  (a) mc_argmin of another build of libmcadcensus.so (--parent-lib: the commit before mc_cost_margins, built aside),
  (b) mc_argmin of this tree,
  (c) mc_predict of the parent build,
  (d) mc_predict of this tree,
  (e) .. (h) mc_cost_margins of this tree with c1_out alone, c2_out alone, c2l_out alone, and all three (d1_out NULL),
  (i) mc_cost_margins with all four outputs,
  (j) a device-to-device copy of the volume's D*H*W*4 bytes (hipMemcpyAsync through torch): what a scan that reads the volume once can
      approach; (e) .. (i) are also given as a multiple of it,
  (k) stereo_predict_fused as bench.py calls it, (l) with want_margins (volume export + scan, left view), (m) with want_right,
  (n) with want_right and want_margins (both views): (l) - (k) and (n) - (m) are what want_margins adds to a pair.
The scanned volume is the final left volume of the pair, as mc_predict exports it.  --runs alternating runs of each, each a warm-up and
then --steps calls between two device synchronisations on the host clock.  (b) is accepted against (a) and (d) against (c) if their
medians differ by no more than the spread (max - min) of the parent's own runs, printed beside the difference.  The arg-min maps and the
disparity maps of both builds are compared bit for bit first, and (i)'s maps with the torch statement (predict.cost_margins) at this
size.  Needs a GPU; writes the report to --out and prints it.

    python scripts/confidence_bench.py --parent-lib /path/to/parent/libmcadcensus.so --out profiles/confidence_bench.txt
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
    ap.add_argument("--parent-lib", default=None, help="libmcadcensus.so of the commit to compare with; without it (a) and (c) are not measured")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="kitti_fast")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confidence_bench.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("confidence_bench: no GPU; a time measured anywhere else says nothing")
    import bench
    import mc_cnn_amd as mc
    from mc_cnn_amd.predict import Workspace, cost_margins, stereo_predict_fused

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    cfg = bench.CONFIGS[args.config]
    preset, H, W, D, Cn, name = cfg
    xb, kw, _ = bench.make_inputs(cfg, 0, device, bench.PAIR_OF[args.config])
    p = mc.make_params(dict(mc.PRESETS[preset]))
    ws = Workspace(p, D, H, W, device)
    feat = kw["feat"].contiguous()
    st = torch.cuda.current_stream().cuda_stream
    vol = stereo_predict_fused(xb, p, D, feat=feat, workspace=ws, want_volumes=True)["volL"].contiguous()
    copy = torch.empty_like(vol)
    torch.cuda.synchronize()

    this = mc._lib.lib
    libs = {"b": this, "d": this}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        assert not hasattr(parent, "mc_cost_margins"), "--parent-lib is meant to be a build from before mc_cost_margins"
        for fn in ("mc_predict", "mc_argmin"):
            getattr(parent, fn).argtypes, getattr(parent, fn).restype = getattr(this, fn).argtypes, C.c_int
        parent.mc_last_error.restype = C.c_char_p
        libs["a"] = libs["c"] = parent
    what = {"a": "mc_argmin, parent build", "b": "mc_argmin, this tree", "c": "mc_predict, parent build", "d": "mc_predict, this tree",
            "e": "mc_cost_margins, c1_out alone", "f": "mc_cost_margins, c2_out alone", "g": "mc_cost_margins, c2l_out alone",
            "h": "mc_cost_margins, c1_out, c2_out and c2l_out", "i": "mc_cost_margins, all four outputs",
            "j": "device-to-device copy of the volume", "k": "stereo_predict_fused", "l": "stereo_predict_fused, want_margins",
            "m": "stereo_predict_fused, want_right", "n": "stereo_predict_fused, want_right and want_margins"}
    out = {k: torch.empty((1, 1, H, W), dtype=torch.float32, device=device) for k in "abcd"}
    maps = [torch.empty((1, 1, H, W), dtype=torch.float32, device=device) for _ in range(4)]
    head = (C.byref(p), xb[0].data_ptr(), xb[1].data_ptr(), feat[0].data_ptr(), feat[1].data_ptr(), feat.shape[-3], None, None, D, H, W,
            ws.ptr, ws.nbytes_full, None, None, None, None)
    subset = {"e": (1,), "f": (2,), "g": (3,), "h": (1, 2, 3), "i": (0, 1, 2, 3)}
    fused = {"k": {}, "l": dict(want_margins=True), "m": dict(want_right=True), "n": dict(want_right=True, want_margins=True)}

    def call(k):
        rc = 0
        if k in "ab":
            rc = libs[k].mc_argmin(vol.data_ptr(), out[k].data_ptr(), D, H, W, st)
        elif k in "cd":
            rc = libs[k].mc_predict(*head, out[k].data_ptr(), st)
        elif k in subset:
            rc = this.mc_cost_margins(vol.data_ptr(), D, H, W, *(maps[j].data_ptr() if j in subset[k] else None for j in range(4)), st)
        elif k == "j":
            copy.copy_(vol)
        else:
            stereo_predict_fused(xb, p, D, feat=feat, workspace=ws, **fused[k])
        if rc:
            raise RuntimeError("%s: rc=%d: %s" % (what[k], rc, this.mc_last_error().decode()))

    def block(k, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            call(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    order = sorted(set(libs) | set(subset) | set(fused) | {"j"})
    for k in order:
        block(k, args.warmup)
    for pair in ("ab", "cd"):
        if pair[0] in libs:
            assert torch.equal(out[pair[0]].view(torch.int32), out[pair[1]].view(torch.int32)), "(%s) differs from (%s)" % tuple(pair)
    want = cost_margins(vol)
    torch.cuda.synchronize()
    for got, ref, k in zip(maps, want, ("d1_out", "c1_out", "c2_out", "c2l_out")):
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), k
    assert torch.equal(maps[0], out["b"]), "d1_out against mc_argmin"
    inf = float("inf")
    counts = (int((want[2] == inf).sum()), int(((want[2] < inf) & (want[3] == inf)).sum()), int((want[2] == want[1]).sum()))
    del want
    ms = {k: [] for k in order}
    for _ in range(args.runs):
        for k in order:
            block(k, args.warmup)
            ms[k].append(block(k, args.steps))

    med = {k: statistics.median(v) for k, v in ms.items()}
    gb = D * H * W * 4 / 1e9
    lines = ["confidence_bench: %s, %s; %d alternating runs of %d calls each (warm-up %d), host clock between device synchronisations"
             % (name, torch.cuda.get_device_name(device), args.runs, args.steps, args.warmup),
             "scanned: the pair's final left volume, %d x %d x %d, %.1f MB" % (D, H, W, gb * 1e3),
             "arg-min maps of (a), (b) and disparity maps of (c), (d): %s" % ("bit-identical" if "a" in libs else "parent not given"),
             "(i)'s four maps: bit-identical to the torch statement (predict.cost_margins) at this size, d1_out to mc_argmin's map; pixels with "
             "one candidate (c2 = +INF): %d, unimodal curves (c2 finite, c2l = +INF): %d, c2 == c1: %d" % counts]
    for k in order:
        more = ""
        if k in subset:
            more = "  = %.2f x the copy (j)" % (med[k] / med["j"])
        if k == "j":
            more = "  = %.0f GB/s read + as much written" % (gb / (med[k] * 1e-3))
        lines.append("(%s) %-50s ms per call: %s  median %.4f  spread %.4f%s" % (
            k, what[k], " ".join("%.4f" % v for v in ms[k]), med[k], max(ms[k]) - min(ms[k]), more))
    if "a" in ms:
        for new, old in (("b", "a"), ("d", "c")):
            spread = max(ms[old]) - min(ms[old])
            delta = med[new] - med[old]
            lines.append("(%s) - (%s), medians: %+.4f ms; margin = spread of (%s)'s own runs: %.4f ms -> %s" % (
                new, old, delta, old, spread, "inside" if abs(delta) <= spread else "OUTSIDE"))
    else:
        lines.append("(a), (c) not measured: no --parent-lib")
    for new, old, text in (("l", "k", "want_margins, one view"), ("n", "m", "want_margins, both views")):
        delta = med[new] - med[old]
        lines.append("(%s) - (%s), medians: %+.4f ms (%+.2f %%): %s, reported, not gated" % (new, old, delta, 100 * delta / med[old], text))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
