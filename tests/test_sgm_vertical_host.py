"""The fused SGM schedule's vertical launches on the host (mc-cnn_amd/csrc/sgm.hip: sgm_sweeps; predict.hip: make_plan).
tests/sgm_vertical_check.cpp is a program of its own that includes sgm.hip, replaces every HIP call -- the kernel launch among them -- and
every launcher of the other units by a logging stub, and is built here with the host side of predict.hip and error.hip under the address and
undefined-behaviour sanitizers, non-recoverable, and run as that program alone.  It checks the order horizontal / checkpoints / recomputing
walk on one stream and on each of the two lanes, the checkpoint slot each volume gets, that the slots lie behind the maps, inside the workspace
and apart from every other area for the GPU tests' shapes and KITTI's, the fallback to the down and the up sweep for D > 256, for volumes of
2 GiB and under the test switch, and a failure injected at each launch.  No GPU and no library is involved."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mc-cnn_amd", "csrc")


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_vertical_launches_slots_fallbacks_and_error_paths(tmp_path):
    hipcc = _hipcc()
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
             "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]   # the host side only: nothing sanitized is built for a GPU
    objs = []
    for src in (os.path.join(CSRC, "predict.hip"), os.path.join(CSRC, "error.hip"), os.path.join(HERE, "sgm_vertical_check.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([hipcc] + flags + ["-x", "hip", "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "sgm_vertical_check")
    # a unit with kernels refers to its device code by a symbol the device compilation would have defined: the host side alone has none
    with open(objs[-1], "rb") as f:
        fatbin = sorted(set(re.findall(rb"__hip_fatbin_[0-9a-f]+", f.read())))
    defs = ["-Wl,--defsym=%s=0" % s.decode() for s in fatbin]
    subprocess.check_call([hipcc, "-Xarch_host", "-fsanitize=address,undefined"] + objs + defs + ["-o", exe, "-lpthread"])
    env = {k: v for k, v in os.environ.items() if k != "MC_PREDICT_LANES"}
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, universal_newlines=True, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    n_checked, n_failed = (int(v) for v in out.stdout.split())
    assert n_checked >= 1000 and n_failed == 0, (n_checked, n_failed)


def test_the_recompute_kernels_live_in_their_own_library_beside_the_one_that_needs_it():
    """libmcsgmrecompute.so holds the recomputing kernels and nothing else; libmcadcensus.so, which links against it, holds none of them, so
    its own inventory stays as it is"""
    import libraries as L
    adcensus = L.path("libmcadcensus.so")
    want = {"sgm_pass_kernel<2, 4, 4, false, true, 16, false, false>", "sgm_updown_kernel<8, true>", "sgm_updown_kernel<8, false>"}
    assert L.built_kernels(L.path("libmcsgmrecompute.so")) == want
    assert not want & L.built_kernels(adcensus) and not want & set(L.read_inventory("kernel_inventory.txt"))
    needed = subprocess.check_output(["readelf", "-d", adcensus]).decode()
    assert "libmcsgmrecompute.so" in needed and "$ORIGIN" in needed   # found beside the library that needs it
    # sgm_sweeps_ck is declared weak (the lanes' host check links predict.hip without sgm.hip): the library itself must define it
    syms = subprocess.check_output(["nm", "-C", "--defined-only", adcensus]).decode()
    assert re.search(r"^[0-9a-f]+ [TtWw] mc::sgm_sweeps_ck\(", syms, re.M)
