"""Time mc_normalize_backward_input (libmcops.so) against the reference's own Normalize_backward_input kernel (oracle/_ref) on the
same GPU, at the training shape of a 128-pair batch and at a full KITTI feature map:

    python scripts/ops_bench.py [--out profiles/ops_bench.txt]

Per shape: 5 warm-up runs, then the median of 20 runs, each between two HIP events on the stream both kernels use (the reference
launches on the NULL stream, which is torch's default stream).  The reference is called through oracle/_ref's entry point directly,
without ref_lib.call's device synchronisations, so that both timings are launch to completion.  Also checks that the two results
are bit-identical."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(384, 64, 1, 1), (2, 64, 370, 1226)]
WARMUP, RUNS = 5, 20


def ref_caller(ref, tensors):
    """A closure that launches the reference's Normalize_backward_input on `tensors` without synchronising."""
    from oracle.ref_lib import UDATA, _Val
    lib = ref.lib
    vals = (_Val * len(tensors))()
    keep = []
    for i, t in enumerate(tensors):
        sizes = (C.c_long * t.dim())(*t.shape)
        h = lib.mcref_tensor_new(0, C.c_void_p(t.data_ptr()), t.dim(), sizes)
        keep.append((t, sizes, h))
        vals[i] = _Val(UDATA, 0.0, b"torch.CudaTensor", h)
    rets, nret, err = (_Val * 8)(), C.c_int(0), C.create_string_buffer(512)

    def call():
        rc = lib.mcref_call(b"adcensus.Normalize_backward_input", vals, len(tensors), rets, C.byref(nret), err, 512)
        assert rc == 0, err.value.decode()
    call.keep = keep
    return call


def timed(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main(argv=None):
    import torch
    import mc_cnn_amd as mc
    from oracle.ref_lib import RefLib
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    ref = RefLib()
    lines = ["# scripts/ops_bench.py on %s: Normalize_backward_input, median (min) of %d runs after %d warm-up runs, HIP events"
             % (torch.cuda.get_device_name(0), RUNS, WARMUP),
             "# shape | libmcops.so ms | reference kernel ms | reference / ours | bytes moved once (3 tensors + norm) GB/s ours"]
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x, go = (torch.randn(shape, device="cuda", generator=g) for _ in range(2))
        norm = torch.empty((shape[0], 1) + shape[2:], device="cuda")
        mc.adcensus.Normalize_forward(x, norm, torch.empty_like(x))
        ours, theirs = torch.empty_like(x), torch.empty_like(x)
        call_ref = ref_caller(ref, (go, x, norm, theirs))
        t_ours = timed(lambda: mc.adcensus.Normalize_backward_input(go, x, norm, ours))
        t_ref = timed(call_ref)
        torch.cuda.synchronize()
        assert torch.equal(ours.view(torch.int32), theirs.view(torch.int32)), "results differ at %s" % (shape,)
        moved = (3 * x.numel() + norm.numel()) * 4
        lines.append("%s | %.4f (%.4f) | %.4f (%.4f) | %.2fx | %.0f" % ("x".join(map(str, shape)), t_ours[0], t_ours[1], t_ref[0], t_ref[1],
                                                                     t_ref[0] / t_ours[0], moved / t_ours[0] / 1e6))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
