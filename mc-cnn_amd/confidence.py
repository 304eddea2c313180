"""Confidence measures from the maps the pipeline returns, and their score against ground truth: the sparsification curve and its area.

Torch only; everything runs on the device its inputs are on.

`measures` names what can be thresholded on: three margins of the cost curve (`mc_cost_margins`: `want_margins` of
`stereo_predict_fused`, or the `c1` / `c2` / `c2l` keys of `stereo_predict(return_all=True)`), the sub-pixel stage's curvature, the LR
check's class and the LR check's distance.  `sparsification` ranks the ground-truth pixels by a measure and counts the bad ones among the
most confident k / n of them, beside the same counts for the ranking by the error itself, which no measure can beat; `area` is the mean
of the rates (the area under the curve: lower is better, the oracle ranking's is the floor).  `keep_mask` turns a measure into a
dial: the most confident fraction of an image.

Ties are broken by the flat pixel index, ascending (stable sorts), so every count is reproducible with `np.argsort(kind="stable")`.
"""
import math

import torch

NAMES = ("msm", "mmn", "mlm", "cur", "cls", "lrc")   # every measure `measures` knows, in the order the command lines print them


def _map(t):
    return t.reshape(t.shape[-2:])


def measures(res, D, view="left"):
    """{name: (H,W) float32}, higher = more confident, from the dict `res` of stereo_predict_fused / stereo_predict(return_all=True):

      msm  -c1                    the matching cost itself
      mmn  c2 - c1                the margin to the runner-up
      mlm  c2l - c1               the margin to the runner-up among the curve's local minima
      cur  res["curvature"]       (left view only)
      cls  1 where outlier == 0, else 0
      lrc  -|d - d'(x')| for d = this view's arg-min map at (y,x), x' = x - d (left) or x + d (right), d' the other view's
           arg-min map; -(float)D where x' leaves the image

    Where c2 is +INF (a pixel with one candidate, e.g. column 0 of the left view) mmn = mlm = 0; otherwise mlm may be +INF (a unimodal
    curve).  view "right" reads c1_right / c2_right / c2l_right, outlier_right and swaps the roles of dispL0 / dispR0.  A name whose
    inputs are missing from res is left out; a NaN measure is replaced by -INF."""
    if view not in ("left", "right"):
        raise ValueError("measures: view %r is not one of left | right" % (view,))
    suffix = "" if view == "left" else "_right"
    out = {}
    if all(k + suffix in res for k in ("c1", "c2", "c2l")):
        c1, c2, c2l = (_map(res[k + suffix]).to(torch.float32) for k in ("c1", "c2", "c2l"))
        single = c2 == float("inf")
        zero = torch.zeros_like(c1)
        out["msm"] = -c1
        out["mmn"] = torch.where(single, zero, c2 - c1)
        out["mlm"] = torch.where(single, zero, c2l - c1)
    if view == "left" and "curvature" in res:
        out["cur"] = _map(res["curvature"]).to(torch.float32)
    if "outlier" + suffix in res:
        out["cls"] = (_map(res["outlier" + suffix]) == 0).to(torch.float32)
    if "dispL0" in res and "dispR0" in res:
        own, other = (res["dispL0"], res["dispR0"]) if view == "left" else (res["dispR0"], res["dispL0"])
        own, other = _map(own).to(torch.float32), _map(other).to(torch.float32)
        H, W = own.shape
        x = torch.arange(W, device=own.device).reshape(1, W).expand(H, W)
        d = own.to(torch.int64)
        xp = x - d if view == "left" else x + d
        inside = (xp >= 0) & (xp < W)
        seen = other.gather(1, xp.clamp(0, W - 1))
        out["lrc"] = torch.where(inside, -(own - seen).abs(), torch.full_like(own, -float(D)))
    for k, v in out.items():
        out[k] = torch.where(torch.isnan(v), torch.full_like(v, -float("inf")), v)
    return {k: out[k] for k in NAMES if k in out}


def _descending(conf):
    """the flat indices of conf by value descending, ties by index ascending; a NaN ranks with -INF"""
    key = -torch.where(torch.isnan(conf), torch.full_like(conf, -float("inf")), conf)
    return torch.sort(key, stable=True).indices


def sparsification(conf, pred, actual, err_at, n=100):
    """The sparsification curve of the confidence map `conf` for the disparity map `pred` against the ground truth `actual` (0 = no
    ground truth), all (H,W): over the N ground-truth pixels ordered by conf descending (ties: flat pixel index ascending), bad[k-1] is
    the number of pixels with |actual - pred| > err_at among the first m[k-1] = ceil(k N / n), k = 1..n.
    Returns (bad, bad_oracle, m), int64 tensors of n values; bad_oracle is the same for the ranking by |actual - pred| ascending."""
    if n < 1:
        raise ValueError("sparsification: n must be at least 1")
    conf, pred, actual = (t.reshape(-1) for t in (conf, pred, actual))
    at = torch.nonzero(actual != 0).reshape(-1)
    N = at.numel()
    if N == 0:
        raise ValueError("sparsification: no pixel with ground truth")
    err = (actual[at].to(torch.float32) - pred[at].to(torch.float32)).abs()
    wrong = (err > err_at).to(torch.int64)
    k = torch.arange(1, n + 1, dtype=torch.int64, device=conf.device)
    m = (k * N + (n - 1)) // n
    bad = torch.cumsum(wrong[_descending(conf[at].to(torch.float32))], 0)[m - 1]
    bad_oracle = torch.cumsum(wrong[torch.sort(err, stable=True).indices], 0)[m - 1]
    return bad, bad_oracle, m


def area(bad, m):
    """the mean of bad[k] / m[k] in float64: the area under a sparsification curve"""
    return float((bad.to(torch.float64) / m.to(torch.float64)).mean().item())


def keep_mask(conf, fraction):
    """(H,W) bool: the first ceil(fraction * H * W) pixels of conf in descending order, ties by flat pixel index ascending"""
    if not 0 < fraction <= 1:
        raise ValueError("keep_mask: fraction %r is outside (0, 1]" % (fraction,))
    flat = conf.reshape(-1)
    n = flat.numel()
    count = min(n, int(math.ceil(fraction * n)))
    mask = torch.zeros(n, dtype=torch.bool, device=conf.device)
    mask[_descending(flat.to(torch.float32))[:count]] = True
    return mask.reshape(conf.shape)

