"""What the four training libraries answer on the host, without a GPU: `mc_train*_workspace_bytes(n)` at the edges of n, and
the return code and the whole `last_error` text of every refusal that the `bad` lists of tests/test_train_slow_host.py,
test_train_mb_host.py and test_train_mb_slow_host.py provoke (restated here, with the same list for libmctrain.so, whose host
test has none).  tests/test_train_contract_host.py compares collect() with tests/golden/train_host_contract.json;

    python tests/train_host_contract.py --tree DIR [--out FILE]

records that file from the built libraries of the checkout DIR (the commit whose messages are the reference)."""
import json
import os
import sys

P = 1 << 20                      # a pointer that is never dereferenced: every check precedes the first launch


def _kitti(lib, prefix, fast):
    need = getattr(lib, prefix + "_workspace_bytes")(4)
    extra = (0.2, 1) if fast else ()

    def step(patches=P, n=4, params=P, moms=P, loss=P, ws=P, ws_bytes=need, extra=extra):
        return getattr(lib, prefix + "_step_batch")(patches, n, params, moms, 0.003, 0.9, *extra, loss, ws, ws_bytes, None)

    def run(x0=P, x1=P, n_img=1, H=20, W=30, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, prm=P, params=P, moms=P,
            losses=P, ws=P, ws_bytes=need):
        return getattr(lib, prefix + "_run")(x0, x1, n_img, H, W, nnz, n_nnz, perm, n_perm, t0, n_steps, n, prm, params, moms, 0.003, 0.9,
                                             *extra, losses, ws, ws_bytes, None)

    bad = [("run: null x0", lambda: run(x0=None)), ("run: null x1", lambda: run(x1=None)), ("run: null nnz", lambda: run(nnz=None)),
           ("run: null perm", lambda: run(perm=None)), ("run: null prm", lambda: run(prm=None)), ("run: null losses", lambda: run(losses=None)),
           ("run: tiny image", lambda: run(H=3)), ("run: wide image", lambda: run(W=32768)), ("run: no image", lambda: run(n_img=0)),
           ("run: empty nnz", lambda: run(n_nnz=0))]
    if fast:
        def sample(x0=P, x1=P, n_img=1, H=20, W=30, nnz=P, n_nnz=10, rows=P, prm=P, n=4, out=P):
            return lib.mc_train_sample(x0, x1, n_img, H, W, nnz, n_nnz, rows, prm, n, out, None)
        bad += [("sample: null x0", lambda: sample(x0=None)), ("sample: null rows", lambda: sample(rows=None)), ("sample: null out", lambda: sample(out=None)),
                ("sample: n_pairs 0", lambda: sample(n=0)), ("sample: tiny image", lambda: sample(W=3)), ("sample: empty nnz", lambda: sample(n_nnz=0))]
    return step, run, bad, need


def _mb(lib, prefix, fast):
    need = getattr(lib, prefix + "_workspace_bytes")(4)
    extra = (0.2, 1) if fast else ()

    def step(patches=P, n=4, params=P, moms=P, loss=P, ws=P, ws_bytes=need, extra=extra):
        return getattr(lib, prefix + "_step_batch")(patches, n, params, moms, 0.003, 0.9, *extra, loss, ws, ws_bytes, None)

    def run(planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, perm=P, n_perm=100, t0=0, n_steps=2, n=4, src=P, prm=P, params=P, moms=P,
            losses=P, ws=P, ws_bytes=need):
        return getattr(lib, prefix + "_run")(planes, table, n_planes, nnz, n_nnz, perm, n_perm, t0, n_steps, n, src, prm, params, moms, 0.003,
                                             0.9, *extra, losses, ws, ws_bytes, None)

    bad = [("run: null planes", lambda: run(planes=None)), ("run: null table", lambda: run(table=None)), ("run: null nnz", lambda: run(nnz=None)),
           ("run: null perm", lambda: run(perm=None)), ("run: null src", lambda: run(src=None)), ("run: null prm", lambda: run(prm=None)),
           ("run: null losses", lambda: run(losses=None)), ("run: no planes", lambda: run(n_planes=0)), ("run: empty nnz", lambda: run(n_nnz=0))]
    if fast:
        def sample(planes=P, table=P, n_planes=3, nnz=P, n_nnz=10, rows=P, src=P, prm=P, n=4, out=P):
            return lib.mc_train_mb_sample(planes, table, n_planes, nnz, n_nnz, rows, src, prm, n, out, None)
        bad += [("sample: null planes", lambda: sample(planes=None)), ("sample: null table", lambda: sample(table=None)),
                ("sample: null nnz", lambda: sample(nnz=None)), ("sample: null rows", lambda: sample(rows=None)),
                ("sample: null src", lambda: sample(src=None)), ("sample: null out", lambda: sample(out=None)),
                ("sample: n_pairs 0", lambda: sample(n=0)), ("sample: no planes", lambda: sample(n_planes=0)),
                ("sample: empty nnz", lambda: sample(n_nnz=0))]
    return step, run, bad, need


def _refusals(lib, prefix, max_pairs, fast, mb):
    step, run, bad, need = (_mb if mb else _kitti)(lib, prefix, fast)
    bad = [("n_pairs 0", lambda: step(n=0)), ("n_pairs above the maximum", lambda: step(n=max_pairs + 1)), ("null patches", lambda: step(patches=None)),
           ("null params", lambda: step(params=None)), ("null moms", lambda: step(moms=None)), ("null loss", lambda: step(loss=None)),
           ("null workspace", lambda: step(ws=None)), ("workspace one byte short", lambda: step(ws_bytes=need - 1)),
           ("run: n_pairs 0", lambda: run(n=0)), ("run: n_pairs above the maximum", lambda: run(n=max_pairs + 1)),
           ("run: workspace one byte short", lambda: run(ws_bytes=need - 1)), ("run: steps past the permutation", lambda: run(t0=93)),
           ("run: negative t0", lambda: run(t0=-1)), ("run: t0 at the end of int64", lambda: run(t0=2 ** 63 - 1)),
           ("run: negative n_steps", lambda: run(n_steps=-1))] + bad
    if fast:
        bad += [("pow 3", lambda: step(extra=(0.2, 3))), ("margin nan", lambda: step(extra=(float("nan"), 1)))]
    else:
        bad += [("misaligned params", lambda: step(params=P + 4)), ("misaligned workspace", lambda: step(ws=P + 4))]
    out = {}
    last_error = getattr(lib, prefix + "_last_error")
    for what, call in bad:
        rc = call()
        out[what] = [rc, last_error().decode()]
    return out


def collect():
    """{library: {"workspace_bytes": {n: bytes}, "refusals": {case: [rc, message]}}}"""
    from mc_cnn_amd import _train_lib, _train_mb_lib, _train_mb_slow_lib, _train_slow_lib
    out = {}
    for mod, fast, mb in ((_train_lib, True, False), (_train_slow_lib, False, False), (_train_mb_lib, True, True), (_train_mb_slow_lib, False, True)):
        lib = mod.load()
        m = mod.MAX_PAIRS if hasattr(mod, "MAX_PAIRS") else 4096     # MC_TRAIN_MAX_PAIRS, which _train_lib.py does not restate
        wb = getattr(lib, mod.PREFIX + "_workspace_bytes")
        out[os.path.basename(mod.LIB_PATH)] = {"workspace_bytes": {str(n): wb(n) for n in (0, 1, 2, 3, 64, 65, m, m + 1)},
                                               "refusals": _refusals(lib, mod.PREFIX, m, fast, mb)}
    return out


if __name__ == "__main__":
    import argparse
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True)
    ap.add_argument("--out", default=os.path.join(here, "golden", "train_host_contract.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    doc = collect()
    import mc_cnn_amd
    assert os.path.samefile(os.path.dirname(os.path.dirname(mc_cnn_amd.__file__)), args.tree), mc_cnn_amd.__file__
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %s refusals" % (args.out, [len(v["refusals"]) for v in doc.values()]))
