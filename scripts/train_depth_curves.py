"""Loss of a 1 200-step training run per depth on the synthetic KITTI set of tests/test_gpu_train_depth.py (6 images of 48 x 160,
the last two the test set): `main.py kitti fast -a train_tr -l1 N -seed 3 -max_steps 1200 -disp_max 32` for N = 1..5, the run
length DESIGN.md 9 reports for l1 = 4.  -l1 4 is the data set's default and trains through libmctrain.so, the others through
libmctraindepth.so.  Prints one JSON line per depth: the mean loss of the first and of the last tenth of the steps and the
test_te error that followed.

    python scripts/train_depth_curves.py [--l1 1 2 3 4 5] [--steps 1200]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--l1", type=int, nargs="+", default=[1, 2, 3, 4, 5])
    ap.add_argument("--steps", type=int, default=1200)
    args = ap.parse_args()
    from test_gpu_train_depth import write_synthetic_kitti
    from mc_cnn_amd import main as mcmain
    from mc_cnn_amd import train, train_depth
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        write_synthetic_kitti(os.path.join(d, "data.kitti"))
        for l1 in args.l1:
            argv = ["kitti", "fast", "-a", "train_tr", "-l1", str(l1), "-seed", "3", "-max_steps", str(args.steps), "-disp_max", "32"]
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                _, trainer, _, _, _, _ = mcmain.route(argv)
                assert trainer is (train if l1 == 4 else train_depth)
                mcmain.main(argv)
            losses = trainer.last_run["losses"]
            n = losses.size // 10
            print(json.dumps({"l1": l1, "library": trainer.__name__.rsplit(".", 1)[-1], "steps": int(losses.size),
                              "loss_first_tenth": round(float(losses[:n].mean()), 4), "loss_last_tenth": round(float(losses[-n:].mean()), 4),
                              "test_te_error": round(float(text.getvalue().strip().splitlines()[-1]), 4)}))
        os.chdir(ROOT)


if __name__ == "__main__":
    main()
