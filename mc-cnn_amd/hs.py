"""The reference's `hs.py ... test_te` search of the stereo method's parameters, on a test set resident on the device.

    python -m mc_cnn_amd.hs {random|hillclimb_slow|hillclimb_fast|hillclimb_dim} {kitti|kitti2015|mb} {fast|slow|ad|census} test_te
           NET_FNAME [-n N] [-seed S] [-log FILE] [-data_dir D] [-disp_max D] [-cache_gb G] [-in_flight K] [-gpu g] [-no_reuse] [-l1 N]
           [-l2 N]

hs.py starts a fresh `main.lua` per candidate; here a candidate is `EvalSet.score` (evalset.py): the cost stage of every test
pair stays on the device, and a candidate costs the post-CNN pipeline plus an error count per pair and one read-back.

GRIDS holds the values a parameter is drawn from, per (dataset, arch), for the `test_te` searches; parameters that a grid does not
name keep params.TABLES[(dataset, arch)].  A candidate is valid if pi1 <= pi2.  Candidates follow hs.py:155-201: `random` draws an
index per parameter; the hill climbs take the best result so far -- read from the files named hs.sh.* in the working directory (what
hs.sh redirects hs.py's output to) and from -log, plus this run's own -- snap each of its values to the nearest grid index, and then
redraw one random dimension (hillclimb_dim), move one random dimension to itself or a neighbour (hillclimb_slow) or move every
dimension so (hillclimb_fast).  With no result yet a hill climb starts from the defaults snapped to the grid.  Draws come from
`random.Random(-seed)`.

One line per candidate, `score dataset arch action -name value ... -net_fname NET`, goes to stdout and, appended and flushed, to
-log; hs.py's log files and these are interchangeable.  -n 0 (the default) runs until interrupted, as hs.py does.

-l1 N names the depth of a fast NET_FNAME that `main.py ... -l1 N` trained (1..5); without it the net has the data set's.
-l2 N names the hidden Linears of a slow NET_FNAME that `main.py ... -l2 N` trained (1..7), likewise.

Not covered: the `train_tr` and `da` searches (of the train_tr grid's axes the depth is trainable here, the feature maps are not:
fm 64 only), rgs*.py, and an on-disk volume cache (-make_cache / -use_cache).
"""
import argparse
import glob
import os
import random
import sys

METHODS = ("random", "hillclimb_slow", "hillclimb_fast", "hillclimb_dim")
DATASETS = ("kitti", "kitti2015", "mb")
ARCHS = ("fast", "slow", "ad", "census")

# ---- the grids ----------------------------------------------------------------------------------------------------------------
_TAU = [0.01, 0.02, 0.03, 0.05, 0.08, 0.13, 0.22, 0.36, 0.6, 1.0]
_SIGMA = [1.0, 1.29, 1.67, 2.15, 2.78, 3.59, 4.64, 5.99, 7.74, 10.0]
_SGM_TAIL = [("sgm_q1", [3, 3.5, 4, 4.5, 5]), ("sgm_q2", [2, 2.5, 3, 3.5, 4, 4.5]),
             ("alpha1", [1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 2.5, 2.75]), ("tau_so", _TAU), ("blur_sigma", _SIGMA)]
_KITTI_SGM = [("pi1", [0.25, 0.33, 0.44, 0.57, 0.76, 1.0, 1.32, 1.74, 2.3, 3.03, 4.0]),
              ("pi2", [8.0, 10.56, 13.93, 18.38, 24.25, 32.0, 42.22, 55.72, 73.52, 97.01, 128.0])] + _SGM_TAIL + \
             [("blur_t", [1, 2, 3, 4, 5, 6, 7])]
_KITTI_CBCA = [("L1", [0, 1, 2, 3, 4, 5, 6]), ("cbca_i1", [0, 2, 4, 6, 8]), ("cbca_i2", [0, 2, 4, 6, 8]), ("tau1", _TAU)]
_MB = [("pi1", [0.2, 0.3, 0.4, 0.6, 0.8, 1.0, 1.3, 1.7, 2.3, 3.0, 4.0]),
       ("pi2", [2.0, 2.6, 3.5, 4.6, 6.1, 8.0, 10.6, 13.9, 18.4, 24.3, 32.0])] + _SGM_TAIL + [("blur_t", [1, 2, 3, 4, 5])]

# (dataset, arch) -> [(parameter, values)], in the order a log line writes them: KITTI slow, KITTI ad and KITTI census (the
# cross-based aggregation's parameters, then the SGM and blur ones), KITTI fast (no aggregation), and Middlebury's one for every arch.
GRIDS = {}
for _d in ("kitti", "kitti2015"):
    GRIDS[(_d, "slow")] = _KITTI_CBCA + _KITTI_SGM
    GRIDS[(_d, "ad")] = _KITTI_CBCA + _KITTI_SGM
    GRIDS[(_d, "census")] = _KITTI_CBCA + _KITTI_SGM
    GRIDS[(_d, "fast")] = list(_KITTI_SGM)
for _a in ARCHS:
    GRIDS[("mb", _a)] = list(_MB)


def grid_of(dataset, arch, action="test_te"):
    if action != "test_te":
        raise SystemExit("hs: the %s search is not supported: only test_te is (of the reference's train_tr grid the depth is "
                         "trainable here, main.py -l1 1..5, but not the feature maps, fm 64 only; the da search is not built)" % action)
    return GRIDS[(dataset, arch)]


def valid(ps):
    """ps: {parameter: value}."""
    return ps["pi1"] <= ps["pi2"]


# ---- log lines ----------------------------------------------------------------------------------------------------------------
def format_line(score, dataset, arch, action, ps, net_fname=None):
    """hs.py:203-211: `score dataset arch action -name value ... [-net_fname NET]`; ps: [(name, value)] in the grid's order."""
    s = "%r %s %s %s %s" % (float(score), dataset, arch, action, " ".join("-%s %s" % p for p in ps))
    return s if net_fname is None else "%s -net_fname %s" % (s, net_fname)


def parse_line(line, dataset, arch, action, grid):
    """hs.py:162-178: (score, {name: value}) of a line of this dataset, arch and action whose parameters are the grid's, in its
    order (whatever follows them, hs.py's -use_cache or -net_fname NET, is ignored); None for every other line."""
    try:
        score, dataset_, arch_, action_, ps_str = line.strip().split(" ", 4)
        if (dataset_, arch_, action_) != (dataset, arch, action):
            return None
        score, tok = float(score), ps_str.split()
        ps = {}
        for i, (name, _) in enumerate(grid):
            if tok[2 * i] != "-" + name:
                return None
            ps[name] = float(tok[2 * i + 1])
        return score, ps
    except (ValueError, IndexError):
        return None


def read_results(dataset, arch, action, grid, directory=".", extra=()):
    """Every result of hs.sh.* in `directory` and of the files `extra`, in file-name order."""
    names = sorted(glob.glob(os.path.join(directory, "hs.sh.*")))
    names += [f for f in extra if f and os.path.exists(f) and os.path.abspath(f) not in [os.path.abspath(n) for n in names]]
    out = []
    for fname in names:
        with open(fname) as f:
            for line in f:
                r = parse_line(line, dataset, arch, action, grid)
                if r is not None:
                    out.append(r)
    return out


# ---- candidates -----------------------------------------------------------------------------------------------------------------
def nearest_index(val, values):
    """hs.py:177: the index of the grid value nearest to val; the lower index on a tie."""
    return min((abs(val - v), j) for j, v in enumerate(values))[1]


def snap(ps, grid):
    return [nearest_index(float(ps[name]), values) for name, values in grid]


def neighbour(method, x, grid, rng):
    """hs.py:180-195: the next candidate's indices from the best one's."""
    x = list(x)
    if method == "hillclimb_dim":
        i = rng.randrange(len(grid))
        x[i] = rng.randrange(len(grid[i][1]))
        return x
    dims = range(len(grid)) if method == "hillclimb_fast" else [rng.randint(0, len(grid) - 1)]
    for i in dims:
        ns = [x[i]]
        if x[i] - 1 >= 0:
            ns.append(x[i] - 1)
        if x[i] + 1 < len(grid[i][1]):
            ns.append(x[i] + 1)
        x[i] = rng.choice(ns)
    return x


def candidate(method, grid, rng, results, defaults):
    """One draw of hs.py:155-201, valid or not: the indices into the grid."""
    if method == "random":
        return [rng.randint(0, len(values) - 1) for _, values in grid]
    best = min(results, key=lambda r: r[0])[1] if results else defaults   # hs.py's min([]) would raise
    return neighbour(method, snap(best, grid), grid, rng)


def search(method, evalset, grid, n, rng, results, emit=None, **score_args):
    """Score n valid candidates (n = 0: until interrupted) on evalset -- anything with `prm`, the table of defaults, and
    `score(prm, **score_args)`.  results: [(score, {name: value})] found so far, appended to as the search goes.  emit(score, ps)
    is called per candidate with ps = [(name, value)].  Returns this run's [(score, {name: value})]."""
    if method not in METHODS:
        raise ValueError("search: method %r is not one of %s" % (method, " | ".join(METHODS)))
    mine = []
    while n == 0 or len(mine) < n:
        x = candidate(method, grid, rng, results, evalset.prm)
        ps = [(name, values[j]) for (name, values), j in zip(grid, x)]
        if not valid(dict(evalset.prm, **dict(ps))):
            continue
        score = evalset.score(dict(evalset.prm, **dict(ps)), **score_args)
        results.append((score, dict(ps)))
        mine.append((score, dict(ps)))
        if emit is not None:
            emit(score, ps)
    return mine


# ---- the command line -------------------------------------------------------------------------------------------------------------
def check_net(net_fname, dataset, arch, l1=None, l2=None):
    """([(w, b)], fc layers or None) of NET_FNAME for a learned arch; SystemExit where the file does not fit the arch.  l1: the
    -l1 of a fast net trained at another depth than the data set's; l2: the -l2 of a slow net, likewise."""
    from .main import FC_SHAPES, load_fc, load_net
    from .params import NET_SHAPES
    if arch not in ("fast", "slow"):
        return [], None
    default_l1, fm = NET_SHAPES[(dataset, arch)]
    l1 = default_l1 if l1 is None else l1
    try:
        layers = load_net(net_fname, dataset, arch, l1=l1)
        fc = load_fc(net_fname, dataset, l2=l2) if arch == "slow" else None
    except (KeyError, ValueError, OSError) as e:
        raise SystemExit("hs: %s does not fit %s %s: %s" % (net_fname, dataset, arch, e))
    got = [tuple(w.shape) for w, _ in layers]
    want = [(fm, 1 if i == 0 else fm, 3, 3) for i in range(l1)]
    if got != want:
        raise SystemExit("hs: %s does not fit %s %s: convolutions of %s, the arch has %s" % (net_fname, dataset, arch, got, want))
    if fc is not None:
        default_l2, nh2 = FC_SHAPES[dataset]
        l2 = default_l2 if l2 is None else l2
        dims = [2 * fm] + [nh2] * l2 + [1]
        want = [(dims[i + 1], dims[i]) for i in range(len(dims) - 1)]
        got = [tuple(w.shape) for w, _ in fc]
        if got != want:
            raise SystemExit("hs: %s does not fit %s slow: Linears of %s, the arch has %s" % (net_fname, dataset, got, want))
    return layers, fc


def parse(argv):
    ap = argparse.ArgumentParser(prog="hs", prefix_chars="-")
    ap.add_argument("method", choices=METHODS)
    ap.add_argument("dataset", choices=DATASETS)
    ap.add_argument("arch", choices=ARCHS)
    ap.add_argument("action", choices=("test_te", "train_tr", "da"))
    ap.add_argument("net_fname")
    ap.add_argument("-n", type=int, default=0, help="candidates to score (0: until interrupted)")
    ap.add_argument("-seed", type=int, default=42)
    ap.add_argument("-log", default="", help="file the result lines are appended to")
    ap.add_argument("-data_dir", default="")
    ap.add_argument("-disp_max", type=int, default=228, help="kitti / kitti2015 (mb takes each image's own from meta.bin)")
    ap.add_argument("-cache_gb", type=float, default=48.0, help="bound of the cached cost-stage outputs")
    ap.add_argument("-in_flight", type=int, default=2, help="streams the examples of a candidate are dealt over")
    ap.add_argument("-gpu", type=int, default=1, help="1-based, as main.py's")
    ap.add_argument("-no_reuse", action="store_true", help="run the whole pipeline for every candidate (no blur-only reuse)")
    ap.add_argument("-l1", type=int, default=None, help="arch fast: the convolutions of NET_FNAME, 1..5, where not the data set's")
    ap.add_argument("-l2", type=int, default=None, help="arch slow: the hidden Linears of NET_FNAME, 1..7, where not the data set's")
    ap.add_argument("-nh2", type=int, default=384, help="arch slow: units per hidden Linear; only 384 is supported")
    from .train_common import add_fc_mode_flag
    add_fc_mode_flag(ap)             # main.py's flag: arch slow's cost stage through mc_fc_stack (fp32) or mc_fc_split_stack (bf16x3)
    from .train_common import add_conv_mode_flag, check_conv_mode
    add_conv_mode_flag(ap)           # main.py's flag: the feature net's convolutions of the cost stage (mc_conv3x3 | mc_conv_split)
    opt = ap.parse_args(argv)
    check_conv_mode(opt, opt.arch, "hs")
    if opt.fc_mode != "fp32" and opt.arch != "slow":
        raise SystemExit("hs: -fc_mode %s for arch %s: only arch slow has an FC stack (main.py -fc_mode)" % (opt.fc_mode, opt.arch))
    if opt.l1 is not None and (opt.arch != "fast" or not 1 <= opt.l1 <= 5):
        raise SystemExit("hs: -l1 %d for arch %s: -l1 1..5 names the depth of a fast net (main.py -l1); the other archs keep "
                         "their data set's" % (opt.l1, opt.arch))
    if opt.l2 is not None and (opt.arch != "slow" or not 1 <= opt.l2 <= 7):
        raise SystemExit("hs: -l2 %d for arch %s: -l2 1..7 names the hidden Linears of a slow net (main.py -l2); the other archs have "
                         "no FC stack" % (opt.l2, opt.arch))
    if opt.nh2 != 384:
        raise SystemExit("hs: -nh2 %d is not supported: only -nh2 384 is (mc_fc_stack and mc_fc_split_stack are 384 wide)" % opt.nh2)
    if opt.action != "test_te":
        grid_of(opt.dataset, opt.arch, opt.action)   # refuses
    if opt.n < 0 or opt.in_flight < 1 or opt.cache_gb < 0:
        raise SystemExit("hs: -n %d, -in_flight %d, -cache_gb %g: none may be negative, -in_flight is at least 1" % (opt.n, opt.in_flight, opt.cache_gb))
    opt.a, opt.at, opt.rect, opt.color = "test_te", 0, "imperfect", "gray"     # what the loaders read besides (mb: data.mb.imperfect_gray)
    return opt


def main(argv=None):
    opt = parse(list(sys.argv[1:] if argv is None else argv))
    grid = grid_of(opt.dataset, opt.arch, opt.action)
    layers, fc_layers = check_net(opt.net_fname, opt.dataset, opt.arch, opt.l1, opt.l2)
    import torch
    from .evalset import EvalSet
    dev = torch.device("cuda", opt.gpu - 1)
    torch.cuda.set_device(dev)
    es = EvalSet(opt.dataset, opt.arch, opt, layers, fc_layers, dev, int(opt.cache_gb * (1 << 30)), reuse=not opt.no_reuse)
    results = read_results(opt.dataset, opt.arch, opt.action, grid, ".", (opt.log,))
    log = open(opt.log, "a") if opt.log else None

    def emit(score, ps):
        line = format_line(score, opt.dataset, opt.arch, opt.action, ps, opt.net_fname)
        print(line)
        sys.stdout.flush()
        if log is not None:
            log.write(line + "\n")
            log.flush()
    try:
        search(opt.method, es, grid, opt.n, random.Random(opt.seed), results, emit, in_flight=opt.in_flight)
    except KeyboardInterrupt:
        pass
    finally:
        if log is not None:
            log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
