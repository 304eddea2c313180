"""Records tests/golden/train_bitwise.json, the hashes tests/test_gpu_train_golden.py compares with: the cases of
tests/train_golden_cases.py run on a GPU against the libraries of a tree.

    python tests/golden/make_train_bitwise.py --tree DIR [--out FILE]

DIR is a checkout of the commit whose results are the reference, built (`make -C mc-cnn_amd/csrc`), e.g. a `git worktree` of
the parent commit; its `mc_cnn_amd` package is the one imported.  The case builder is this tree's.  Refuses to write where
a case proves nothing (train_golden_cases.vacuous)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "train_bitwise.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(HERE, ".."))
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import mc_cnn_amd
    import train_golden_cases as tg
    assert os.path.samefile(os.path.dirname(os.path.dirname(mc_cnn_amd.__file__)), args.tree), mc_cnn_amd.__file__
    results = tg.run_all()
    for name, r in results.items():
        why = tg.vacuous(r)
        if why:
            raise SystemExit("%s proves nothing (%s): nothing written" % (name, why))
        if "losses" in r:
            print(name, "losses", r["losses"].tolist())
    doc = {"rocm": torch.version.hip, "torch": torch.__version__, "device": torch.cuda.get_device_name(0),
           "cases": {name: tg.hashes(r) for name, r in results.items()}}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases" % (args.out, len(doc["cases"])))


if __name__ == "__main__":
    main()
