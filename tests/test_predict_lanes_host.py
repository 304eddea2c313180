"""mc_predict's two-lane schedule on the host (mc-cnn_amd/csrc/predict.hip): the stream and event cache, the MC_PREDICT_LANES switch, the order
of launches, records and waits on the two streams, and the way out of a failed call.  tests/predict_lanes_check.cpp is a program of its own
that replaces every launcher and every HIP call predict_impl makes by a stub writing into a log; it is built here from the host side of
predict.hip and error.hip with the address and undefined-behaviour sanitizers, non-recoverable, and run as that program alone.  It covers
cache hits and misses from eight threads on four caller streams, the switch's parsing and its read-once rule, the refusals in front of
the first launch (nothing queued, nothing created), the configurations that keep one lane, and a failure injected at every position of
a two-lane call: whenever anything was queued on the side stream, the last things queued are the side stream's record and the caller
stream's wait for it.  No GPU and no library is involved."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mc-cnn_amd", "csrc")


def _hipcc():
    return os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_two_lane_schedule_cache_switch_and_error_paths(tmp_path):
    hipcc = _hipcc()
    flags = ["--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unused-function",
             "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]   # the host side only: nothing sanitized is built for a GPU
    objs = []
    for src in (os.path.join(CSRC, "predict.hip"), os.path.join(CSRC, "error.hip"), os.path.join(HERE, "predict_lanes_check.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([hipcc] + flags + ["-x", "hip", "-c", src, "-o", obj])
        objs.append(obj)
    exe = str(tmp_path / "predict_lanes_check")
    subprocess.check_call([hipcc, "-Xarch_host", "-fsanitize=address,undefined"] + objs + ["-o", exe, "-lpthread"])
    env = {k: v for k, v in os.environ.items() if k != "MC_PREDICT_LANES"}   # the program sets it itself
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, universal_newlines=True, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    n_checked, n_failed = (int(v) for v in out.stdout.split())
    assert n_checked >= 1000 and n_failed == 0, (n_checked, n_failed)
