"""What the right view's map costs, and what its run-time forms cost everyone else: ms per pair at bench.py's default workload (KITTI fast,
370 x 1226 x 228, its seeded pair and features) for
  (a) mc_predict of another build of libmcadcensus.so (--parent-lib: the commit before mc_predict_views, built aside),
  (b) mc_predict of this tree,
  (c) mc_predict_ex with outlier, cost and curvature of the parent build,
  (d) the same of this tree,
  (e) mc_predict_views of this tree with both right-view maps NULL,
  (f) mc_predict_views of this tree with dispR_out and outlierR_out,
  (g) mc_predict_views of this tree with outlierR_out alone (two mirrors, the LR check, one mirror back: no stage of the tail).
--runs alternating runs of each (a, b, ..., g, a, b, ...), each a warm-up and then --steps calls between two device synchronisations on
the host clock.  (b) is accepted against (a) and (d) against (c) if their medians differ by no more than the spread (max - min) of the
parent's own runs: scale_kernel and subpixel_kernel, which gained a mirrored form, are on everyone's path.  (f) - (e) is the cost of the
feature, reported, with (g) - (e) and the left view's own tail (MC_STAGE_POST of mc_predict_timed, one lane) beside it.  The disparity maps are compared bit for bit first, and (f)'s two maps with the op-by-op composition at this size.  Needs a GPU; writes the report to --out and prints it.

    python scripts/right_view_bench.py --parent-lib /path/to/parent/libmcadcensus.so --out profiles/right_view_bench.txt
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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="kitti_fast")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "right_view_bench.txt"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("right_view_bench: no GPU; a time measured anywhere else says nothing")
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
    libs = {"b": this, "d": this, "e": this, "f": this, "g": this}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        assert not hasattr(parent, "mc_predict_views"), "--parent-lib is meant to be a build from before mc_predict_views"
        for fn in ("mc_predict", "mc_predict_ex"):
            getattr(parent, fn).argtypes, getattr(parent, fn).restype = getattr(this, fn).argtypes, C.c_int
        parent.mc_last_error.restype = C.c_char_p
        libs["a"] = libs["c"] = parent
    what = {"a": "mc_predict, parent build", "b": "mc_predict, this tree",
            "c": "mc_predict_ex with outlier, cost, curvature, parent build", "d": "mc_predict_ex with outlier, cost, curvature, this tree",
            "e": "mc_predict_views, both right-view maps NULL, this tree", "f": "mc_predict_views with dispR_out and outlierR_out, this tree",
            "g": "mc_predict_views with outlierR_out alone, this tree"}
    out = {k: torch.empty((1, 1, H, W), dtype=torch.float32, device=device) for k in libs}
    maps = [torch.empty((1, 1, H, W), dtype=torch.float32, device=device) for _ in range(5)]
    head = (C.byref(p), xb[0].data_ptr(), xb[1].data_ptr(), feat[0].data_ptr(), feat[1].data_ptr(), feat.shape[-3], None, None, D, H, W,
            ws.ptr, ws.nbytes_full, None, None, None, None)

    def call(k):
        if k in "cd":
            rc = libs[k].mc_predict_ex(*head, *(e.data_ptr() for e in maps[:3]), out[k].data_ptr(), st)
        elif k == "e":
            rc = this.mc_predict_views(*head, None, None, None, None, None, out[k].data_ptr(), st)
        elif k == "f":
            rc = this.mc_predict_views(*head, None, None, None, maps[3].data_ptr(), maps[4].data_ptr(), out[k].data_ptr(), st)
        elif k == "g":
            rc = this.mc_predict_views(*head, None, None, None, None, maps[4].data_ptr(), out[k].data_ptr(), st)
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
    # the two maps at this size against the op-by-op statement (predict.right_view) on the maps and the volume the fused call exports
    from mc_cnn_amd.predict import right_view, stereo_predict_fused
    res = stereo_predict_fused(xb, p, D, feat=feat, workspace=ws, want_volumes=True, want_disp0=True, want_right=True)
    want = right_view(p, res["dispL0"], res["dispR0"], res["volR"], D)
    torch.cuda.synchronize()
    assert torch.equal(res["disp"].view(torch.int32), out["f"].view(torch.int32)), "disp with every output asked for"
    for got, ref, k in ((maps[3], want[0], "dispR_out"), (maps[4], want[1], "outlierR_out")):
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)) and torch.equal(res[{"dispR_out": "disp_right", "outlierR_out": "outlier_right"}[k]].view(torch.int32), ref.view(torch.int32)), k
    classes = [int((want[1] == c).sum()) for c in (0, 1, 2)]
    del res, want
    left = stereo_predict_fused(xb, p, D, feat=feat, workspace=ws, want_outlier=True)["outlier"]
    classes += [int((left == c).sum()) for c in (0, 1, 2)]
    post = statistics.median(stereo_predict_fused(xb, p, D, feat=feat, workspace=ws, timed=True)["stage_ms"]["post"] for _ in range(11))
    ms = {k: [] for k in order}
    for _ in range(args.runs):
        for k in order:
            block(k, args.warmup)
            ms[k].append(block(k, args.steps))

    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = ["right_view_bench: %s, %s; %d alternating runs of %d calls each (warm-up %d), host clock between device synchronisations"
             % (name, torch.cuda.get_device_name(device), args.runs, args.steps, args.warmup),
             "disparity maps of %s: bit-identical" % ", ".join("(%s)" % k for k in order),
             "(f)'s dispR_out and outlierR_out: bit-identical to the op-by-op composition (predict.right_view) at this size; right-view classes "
             "0 / 1 / 2: %d / %d / %d pixels (left view: %d / %d / %d)" % tuple(classes)]
    for k in order:
        lines.append("(%s) %-58s ms per pair: %s  median %.4f  spread %.4f" % (
            k, what[k], " ".join("%.4f" % v for v in ms[k]), med[k], max(ms[k]) - min(ms[k])))
    if "a" in ms:
        for new, old in (("b", "a"), ("d", "c")):
            spread = max(ms[old]) - min(ms[old])
            delta = med[new] - med[old]
            lines.append("(%s) - (%s), medians: %+.4f ms; margin = spread of (%s)'s own runs: %.4f ms -> %s" % (
                new, old, delta, old, spread, "inside" if abs(delta) <= spread else "OUTSIDE"))
    else:
        lines.append("(a), (c) not measured: no --parent-lib")
    delta_f = med["f"] - med["e"]
    lines.append("(f) - (e), medians: %+.4f ms (%+.2f %%): the right view's tail, reported, not gated" % (delta_f, 100 * delta_f / med["e"]))
    delta_g = med["g"] - med["e"]
    lines.append("(g) - (e), medians: %+.4f ms (%+.2f %%): the mirrors and the LR check of it" % (delta_g, 100 * delta_g / med["e"]))
    lines.append("the left view's tail, MC_STAGE_POST of mc_predict_timed (events, one lane), median of 11: %.4f ms" % post)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
