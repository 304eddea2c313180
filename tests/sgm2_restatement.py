"""adcensus.sgm2 restated in torch tensor operations: the kernels sgm2<0..3> (adcensus.cu:535-618) in their launch order (adcensus.cu:639-693),
for disparity ranges the C oracle does not take (oracle_sgm2 stops at 512).  One scan STEP -- one launch of the reference -- is one tensor
operation over (lines x D), so the restatement runs on whichever device holds the tensors; the steps themselves stay a host loop, as the
reference's launches are.

Every add and subtract is an operation of its own, in the kernel's order: (input + cost) - min, then output += val, directions right, left,
down, up.  Minima are torch.fmin (the kernel's min() is fminf: a NaN operand loses).  The three penalty pairs and P1 / alpha1 are float32
divisions as written at adcensus.cu:595-613.

One point is restated rather than copied: the kernel's minimum over d is a `<`-tree over 512 shared floats (adcensus.cu:579-584).  Under
sgm2's contract -- a pixel's NaNs form a tail in d and d = 0 is finite -- that tree returns the minimum of the numbers; here it is
amin over d with NaN read as +inf.  tests/test_sgm_wide_host.py holds the two against each other bit for bit at every D the oracle takes.
The line state `tmp` is kept per line, as the oracle keeps it (the reference's own index aliases for H > W)."""
import numpy as np
import torch


def penalties(pi1, pi2, alpha1, q1, q2):
    """rows: class 0 both < tau_so, 1 mixed, 2 both > tau_so; columns P1, P2, P1 / alpha1 -- float32 arithmetic, adcensus.cu:595-613"""
    f = np.float32
    pi1, pi2, alpha1, q1, q2 = f(pi1), f(pi2), f(alpha1), f(q1), f(q2)
    P1 = [pi1, pi1 / q1, pi1 / (q1 * q2)]
    P2 = [pi2, pi2 / q1, pi2 / (q1 * q2)]
    return np.array([[P1[k], P2[k], P1[k] / alpha1] for k in range(3)], np.float32)


def _cls(v, tau):
    """0: v < tau, 2: v > tau, 1: neither (equal, or NaN)"""
    return torch.where(v < tau, 0, torch.where(v > tau, 2, 1))


def sgm2(x0, x1, vol, out, pi1, pi2, tau_so, alpha1, q1, q2, direction):
    """x0, x1: (H,W); vol, out: (H,W,D) float32 tensors on one device.  Adds the four directional costs to `out`, in place; returns it."""
    H, W, D = vol.shape
    dev = vol.device
    tau = float(np.float32(tau_so))
    pen = torch.from_numpy(penalties(pi1, pi2, alpha1, q1, q2)).to(dev)
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    d_idx = torch.arange(D, device=dev)
    for r, (dx, dy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        # COLOR_DIFF(img, p, p - dy * W - dx) at every pixel that has that neighbour (the others: border steps for x0, D2 = 10 for x1)
        def edge(img, fill):
            e = torch.full((H, W), fill, dtype=torch.float32, device=dev)
            ys = slice(max(dy, 0), H + min(dy, 0))
            xs = slice(max(dx, 0), W + min(dx, 0))
            yn = slice(max(dy, 0) - dy, H + min(dy, 0) - dy)
            xn = slice(max(dx, 0) - dx, W + min(dx, 0) - dx)
            e[ys, xs] = (img[ys, xs] - img[yn, xn]).abs()
            return e
        c1 = _cls(edge(x0, 10.0), tau)                                   # class of D1 per reference pixel
        e2 = torch.full((H, W + 2 * D), 10.0, dtype=torch.float32, device=dev)   # D2 = 10 where xx or xx - dx is outside, adcensus.cu:590-591
        e2[:, D:D + W] = edge(x1, 10.0)
        c2 = _cls(e2, tau)
        horizontal = dy == 0
        nsteps = W if horizontal else H
        nlines = H if horizontal else W
        # column of c2 that holds the partner pixel xx = x + d * direction of (line or step x, d)
        part = (D + direction * d_idx)[None, :] + (0 if horizontal else torch.arange(W, device=dev)[:, None])
        prev = None
        for step in range(nsteps):
            pos = step if dx + dy > 0 else nsteps - 1 - step
            C = vol[:, pos, :] if horizontal else vol[pos, :, :]         # (lines, D)
            O = out[:, pos, :] if horizontal else out[pos, :, :]
            if step == 0:                                                # adcensus.cu:567-572
                val = C.clone()
            else:
                if horizontal:
                    a = c1[:, pos]                                       # (lines,)
                    b = c2[:, pos + part[0]]                             # (lines, D)
                else:
                    a = c1[pos, :]
                    b = c2[pos][part]
                a = a[:, None].expand(nlines, D)
                k = torch.where((a == 0) & (b == 0), 0, torch.where((a == 2) & (b == 2), 2, 1))   # adcensus.cu:596-605
                P1, P2, P1a = pen[k, 0], pen[k, 1], pen[k, 2]
                m = torch.where(torch.isnan(prev), inf, prev).amin(dim=1, keepdim=True)           # output_min[0]
                cost = torch.fmin(prev, m + P2)                                                    # adcensus.cu:607
                cost[:, 1:] = torch.fmin(cost[:, 1:], prev[:, :-1] + (P1a if r == 2 else P1)[:, 1:])    # d - 1 >= 0, :608-610
                cost[:, :-1] = torch.fmin(cost[:, :-1], prev[:, 1:] + (P1a if r == 3 else P1)[:, :-1])  # d + 1 < D, :611-613
                val = (C + cost) - m                                     # adcensus.cu:615
            O += val                                                     # adcensus.cu:616
            prev = val
    return out


# ---- the cases the tests of the restatement and of mc_sgm2 share ----
# pi1, pi2, tau_so, alpha1, q1, q2: alpha1 != 1 (the down and up sweeps' P1 / alpha1), q1 * q2 not a power of two
PRM = (2.3, 42.3, None, 1.25, 3.0, 2.0)


def quantised_case(H, W, D, direction, seed):
    """x0, x1, an (H,W,D) volume and tau_so: images in eighths, so that the |differences| that pick the penalties lie below, above and ON
    tau_so = 1/8 (all three classes), and a volume in sixteenths, 1/16 .. 1 (ties in every minimum, no zero), with the direction's NaN
    triangle -- left volume d > x, right volume x + d >= W"""
    from util import raw_volumes
    rng = np.random.default_rng(seed)
    x0, x1 = rng.integers(0, 4, (2, H, W)) / 8
    vl, vr = raw_volumes(D, H, W, seed=seed + 1)
    vol = vl if direction == -1 else vr
    vol = (np.floor(vol * 16) + 1) / 16
    return x0.astype(np.float32), x1.astype(np.float32), np.ascontiguousarray(vol.transpose(1, 2, 0)).astype(np.float32), 0.125


# ---- what the GPU tests of these ranges share ----
def assert_same_bits_dev(got, want, name):
    """bit-exact equality on the device, NaN == NaN, NaN masks identical"""
    got, want = got.reshape(-1), want.reshape(-1)
    assert got.shape == want.shape, name
    ng, nw = torch.isnan(got), torch.isnan(want)
    bad = (ng != nw) | (~ng & (got.view(torch.int32) != want.view(torch.int32)))
    n = int(bad.sum().item())
    if n:
        idx = torch.nonzero(bad)[:5, 0]
        raise AssertionError("%s: %d of %d elements differ; first idx=%s got=%s want=%s" % (
            name, n, got.numel(), idx.tolist(), got[idx].tolist(), want[idx].tolist()))


def device_pair(H, W, seed):
    """a textured pair made on the device (no multi-GB host arrays): smoothed noise, the right image the left shifted by 9 pixels"""
    import torch.nn.functional as F
    g = torch.Generator(device="cuda").manual_seed(seed)
    x0 = F.avg_pool2d(torch.rand((1, 1, H, W + 16), device="cuda", generator=g), 3, 1, 1)
    x1 = torch.roll(x0, -9, dims=3) + 0.02 * torch.rand(x0.shape, device="cuda", generator=g)
    return torch.cat([x0, x1])[:, :, :, :W].contiguous()


def device_raw_volumes(D, H, W, seed):
    """uniform [0, 1) (1,D,H,W) volumes made on the device, with the NaN triangles (left d > x, right x + d >= W)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    d = torch.arange(D, device="cuda")[:, None, None]
    x = torch.arange(W, device="cuda")[None, None, :]
    vl = torch.rand((1, D, H, W), device="cuda", generator=g).masked_fill_((d > x)[None], float("nan"))
    vr = torch.rand((1, D, H, W), device="cuda", generator=g).masked_fill_((x + d >= W)[None], float("nan"))
    return vl, vr


def device_features(C, H, W, seed):
    """N(0, 1) features L2-normalised over C, made on the device; the right view is the left shifted by 9 pixels plus noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    f0 = torch.randn((1, C, H, W), device="cuda", generator=g)
    f1 = torch.roll(f0, -9, dims=3) + 0.3 * torch.randn(f0.shape, device="cuda", generator=g)
    f = torch.cat([f0, f1])
    return (f / torch.sqrt((f.double() ** 2).sum(1, keepdim=True) + 1e-5).float()).contiguous()
