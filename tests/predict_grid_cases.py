"""The case tables of tests/test_gpu_predict_grid.py (GPU: mc_predict against the CPU oracle at every value the parameter search
draws, hs.GRIDS) and tests/test_predict_grid_host.py (CPU: the oracle alone over the same tables, so that no GPU comparison is
vacuous).  A plain module, imported as it is.

A family names a (dataset, arch) for `hs.grid_of` and `params.TABLES`, a shape, an input pair and a cost stage.  The shapes are the
smallest at which the kernels behind the grid's axes still have image-border rows, part tiles and several arm lengths; family B has
D % 4 != 0 and W % 32 != 0, family E is test_gpu_planned_routes.py's real-scene shape.

`counts`: per axis, how many DISTINCT disparity maps the oracle gives over the axis' values with the rest of the table at its
defaults (test_predict_grid_host.py reproduces every figure).  Fewer than the axis has values where the inputs make values
indistinguishable: `cross` gives arm 1 for L1 = 0, 1 and 2 alike, a large pi2 stops mattering, ..."""
import random

import numpy as np

from util import features, natural_pair, raw_volumes, smooth_pair

CBCA_AXES = ("L1", "cbca_i1", "cbca_i2", "tau1")

FAMILIES = {
    "A": dict(dataset="kitti", arch="slow", H=26, W=84, D=20, pair="natural", stage="raw", axes=None,
              counts=dict(L1=5, cbca_i1=5, cbca_i2=5, tau1=9, pi1=11, pi2=4, sgm_q1=5, sgm_q2=6, alpha1=8, tau_so=9, blur_sigma=10, blur_t=7)),
    "B": dict(dataset="kitti", arch="fast", H=21, W=70, D=30, pair="smooth", stage="feat", axes=None,
              counts=dict(pi1=11, pi2=8, sgm_q1=5, sgm_q2=6, alpha1=8, tau_so=10, blur_sigma=10, blur_t=7)),
    "C": dict(dataset="mb", arch="slow", H=28, W=80, D=20, pair="natural", stage="raw", axes=None,
              counts=dict(pi1=11, pi2=10, sgm_q1=5, sgm_q2=6, alpha1=8, tau_so=9, blur_sigma=10, blur_t=5)),
    "D": dict(dataset="kitti", arch="ad", H=26, W=84, D=20, pair="natural", stage="raw", axes=None,
              counts=dict(L1=5, cbca_i1=5, cbca_i2=5, tau1=9, pi1=11, pi2=6, sgm_q1=5, sgm_q2=6, alpha1=8, tau_so=9, blur_sigma=10, blur_t=7)),
    "E": dict(dataset="kitti", arch="slow", H=60, W=300, D=16, pair="natural4", stage="raw", axes=CBCA_AXES,
              counts=dict(L1=5, cbca_i1=5, cbca_i2=5, tau1=9)),
}
# mb outside `-a predict` runs the left volume only (EvalSet sets left_only = 1): family C runs both ways
LEFT_ONLY = {"A": (0,), "B": (0,), "C": (0, 1), "D": (0,), "E": (0,)}
COMPARED = {0: ("volL", "volR", "dispL0", "dispR0", "disp"), 1: ("volL", "dispL0", "disp")}
WALK_N = 40
GENERIC_BLUR_SIGMAS = (1.0, 1.29, 2.15, 3.59, 10.0)    # kernel sizes 7, 9, 15, 23, 61: mean2d's run-time-size kernel


def grid(fam):
    """[(axis, values)] of the family, in hs.GRIDS' order."""
    from mc_cnn_amd import hs
    f = FAMILIES[fam]
    g = hs.grid_of(f["dataset"], f["arch"])
    return [(k, v) for k, v in g if f["axes"] is None or k in f["axes"]]


def base(fam):
    """The family's default table (a copy)."""
    from mc_cnn_amd.params import TABLES
    f = FAMILIES[fam]
    return dict(TABLES[(f["dataset"], f["arch"])])


def axes():
    """[(family, axis)] of every family."""
    return [(fam, k) for fam in FAMILIES for k, _ in grid(fam)]


_inputs = {}


def inputs(fam):
    """(x0, x1, the cost stage as oracle.stereo_predict's keywords), made once per family and never written to."""
    if fam not in _inputs:
        f = FAMILIES[fam]
        H, W, D = f["H"], f["W"], f["D"]
        if f["pair"] == "natural":
            x0, x1 = natural_pair(H, W, 8, seed=H + W, sigma=8.0)
        elif f["pair"] == "natural4":
            x0, x1 = natural_pair(H, W, 8, seed=4, sigma=8.0)
        else:
            x0, x1 = smooth_pair(H, W, 12, seed=77)
        if f["stage"] == "feat":
            ft = features(16, H, W, seed=5)
            stage = dict(featL=ft[0], featR=ft[1])
        else:
            vl, vr = raw_volumes(D, H, W, seed=7)
            stage = dict(rawL=vl, rawR=vr)
        for a in (x0, x1) + tuple(stage.values()):
            a.setflags(write=False)
        _inputs[fam] = (x0, x1, stage)
    return _inputs[fam]


def want(oracle, fam, prm):
    """oracle.stereo_predict of the family's inputs under the table prm."""
    x0, x1, stage = inputs(fam)
    with np.errstate(all="ignore"):
        return oracle.stereo_predict(prm, x0, x1, FAMILIES[fam]["D"], **stage)


def axis_cases(fam, axis):
    """One table per value of the axis, the rest at the defaults -- tau1 with L1 = 5, so that the axis is live (with the ad and
    census defaults L1 is 3 or 0 and every arm is 1 whatever tau1 is).  Only what hs.valid rejects (pi1 > pi2) is left out."""
    from mc_cnn_amd import hs
    b = base(fam)
    if axis == "tau1":
        b["L1"] = 5
    out = [dict(b, **{axis: v}) for v in dict(grid(fam))[axis]]
    return [p for p in out if hs.valid(p)]


def corner_cases(fam):
    """[(label, table)]: every axis at its lowest, every axis at its highest (pi1 at its lowest, so that the candidate is valid),
    and where the family has the aggregation's axes: the iteration counts' corners, and L1 around the tile kernel's arm classes
    (cap 4 | 5) crossed with tau1's ends."""
    b, g = base(fam), grid(fam)
    out = [("lowest", dict(b, **{k: v[0] for k, v in g})),
           ("highest", dict(b, **{k: (v[0] if k == "pi1" else v[-1]) for k, v in g}))]
    if "L1" in dict(g):
        out += [("i1=%d,i2=%d" % c, dict(b, cbca_i1=c[0], cbca_i2=c[1])) for c in ((0, 8), (8, 0), (0, 0), (8, 8))]
        out += [("L1=%d,tau1=%g" % (l, t), dict(b, L1=l, tau1=t)) for l in (0, 4, 5, 6) for t in (0.01, 1.0)]
    return out


def walk(fam, n=WALK_N):
    """The first n valid candidates of the family's random search seeded with 1, in the order drawn: [table]."""
    return walk_of(grid(fam), base(fam), n)


def walk_of(g, b, n):
    """... of the grid g over the default table b."""
    from mc_cnn_amd import hs
    rng, out = random.Random(1), []
    while len(out) < n:
        x = hs.candidate("random", g, rng, [], b)
        p = dict(b, **{name: values[j] for (name, values), j in zip(g, x)})
        if hs.valid(p):
            out.append(p)
    return out


def label(fam, prm):
    """The grid's axes of a table, for messages."""
    return "%s %s" % (fam, " ".join("%s=%g" % (k, prm[k]) for k, _ in grid(fam)))
