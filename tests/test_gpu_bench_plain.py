"""-m gpu: a plain `bench.py` run (no --full) on the tiny config: exactly --steps timed steps, the headline fields and none of the
side records, and --dump-outputs writing the last step's disparity map -- the same from run to run, and bit-identical to the fused
mc_predict on bench.make_inputs' inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--config", "tiny", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_steps_and_dumps_outputs(tmp_path, mc):
    import torch
    import bench
    j = _run(tmp_path / "a")
    assert j["steps"] == 4 and j["warmup"] == 1 and j["timed_blocks"] == 1 and j["full"] is False
    assert j["ms_per_step"] > 0 and j["value"] > 0 and j["unit"] == "MPix-disp/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    for k in ("stage_ms", "roofline", "verify", "cpu_baseline", "ops_ms_per_pair", "north_star", "multi_gpu"):
        assert j[k] is None, k
    a = np.load(tmp_path / "a" / "disp.npy")
    assert a.dtype == np.float32 and a.shape == (1, 1, 48, 160)
    _run(tmp_path / "b")                      # same arguments, same inputs: the same map
    assert a.tobytes() == np.load(tmp_path / "b" / "disp.npy").tobytes()

    preset, H, W, D, C, _ = bench.CONFIGS["tiny"]
    xb, kw, _ = bench.make_inputs(bench.CONFIGS["tiny"], 0, torch.device("cuda", 0))
    want = mc.stereo_predict_fused(xb, dict(mc.PRESETS[preset]), D, **kw)["disp"]
    torch.cuda.synchronize()
    assert want.cpu().numpy().tobytes() == a.tobytes()
