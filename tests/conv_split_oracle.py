"""The arithmetic of mc_conv_split (include/mc_conv_split.h) restated in numpy: a 3x3 convolution, stride 1, zero padding 1, with every
product taken as three bf16 products of hi + lo parts.  Sums are accumulated in float64 and rounded to fp32 once, where the header says
"in fp32" (the kernel's summation order is the matrix cores'); every other rounding point is the header's.

    split(v): hi = bf16(v), round to nearest even; lo = bf16(v - float(hi))
    out[n,co,y,x] = act( sum_{ci,ky,kx} (Whi Xhi + Whi Xlo + Wlo Xhi) + b[co] ),  X at (y + ky - 1, x + kx - 1), zero outside the image
"""
import numpy as np

f32, f64 = np.float32, np.float64

# (N, Cin, Cout, H, W, relu) of tests/test_gpu_conv_split.py::test_conv_split; tests/test_conv_split_host.py holds the bars at each
CASES = [
    (2, 64, 64, 33, 65, True), (2, 64, 64, 20, 31, False), (2, 112, 112, 18, 45, True),
    (1, 16, 128, 8, 40, False),        # one k-step
    (1, 48, 96, 5, 33, True),
    (1, 64, 64, 1, 5, True),           # one row, less than a strip
    (3, 16, 64, 61, 33, False),        # tiles that cross images and short last tiles
    (1, 64, 33, 9, 40, False),         # Cout % 8 != 0
    (3, 32, 100, 13, 70, True),        # last group partly filled
    (1, 160, 40, 9, 70, True),         # more channel chunks than any net has
    (1, 64, 64, 300, 100, True),       # every block busy, several tiles per block
    (1, 112, 112, 130, 70, True),
    (2, 32, 32, 19, 37, True), (1, 16, 7, 5, 33, False),      # Cout <= 32: the kernel's one-tile instance
]


def bf16(v):
    """v (float32, finite) rounded to bfloat16, to nearest even, as float32"""
    u = np.ascontiguousarray(v, dtype=f32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(f32).reshape(np.shape(v))


def split(v):
    v = np.asarray(v, dtype=f32)
    hi = bf16(v)
    return hi, bf16((v - hi).astype(f32))


def inputs(N, Cin, Cout, H, W):
    """the inputs of tests/test_gpu_conv.py::test_conv3x3_vs_torch: standard-normal x, weights and bias uniform in +-1/sqrt(9 Cin)"""
    rng = np.random.default_rng(Cin * 1000 + Cout)
    x = rng.standard_normal((N, Cin, H, W)).astype(f32)
    bound = 1.0 / np.sqrt(Cin * 9)
    w = rng.uniform(-bound, bound, (Cout, Cin, 3, 3)).astype(f32)
    b = rng.uniform(-bound, bound, (Cout,)).astype(f32)
    return x, w, b


def conv64(x, w):
    """sum_{ci,ky,kx} w[co,ci,ky,kx] x[n,ci,y+ky-1,x+kx-1] in float64, zero padding 1: (N,Cin,H,W), (Cout,Cin,3,3) -> (N,Cout,H,W)"""
    x, w = np.asarray(x, f64), np.asarray(w, f64)
    N, Cin, H, W = x.shape
    xp = np.zeros((N, Cin, H + 2, W + 2), f64)
    xp[:, :, 1:-1, 1:-1] = x
    out = np.zeros((N, w.shape[0], H, W), f64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W], optimize=True)
    return out


def conv_f64(x, w, b, relu):
    """the float64 convolution the operator's 1e-4 bar is against (tests/test_gpu_conv.py)"""
    z = conv64(x, w) + np.asarray(b, f64)[None, :, None, None]
    return np.maximum(z, 0.0) if relu else z


def conv_split(x, w, b, relu, drop=None):
    """mc_conv_split's arithmetic -> (N,Cout,H,W) fp32.  drop: "hi.lo" (Whi Xlo) or "lo.hi" (Wlo Xhi) leaves that cross term out, "both"
    both (one bf16 pass): what a faulty kernel would compute -- the tests measure how far that moves the result."""
    xhi, xlo = split(x)
    whi, wlo = split(w)
    z = conv64(xhi, whi)
    if drop not in ("hi.lo", "both"):
        z += conv64(xlo, whi)
    if drop not in ("lo.hi", "both"):
        z += conv64(xhi, wlo)
    out = (z.astype(f32) + np.asarray(b, f32)[None, :, None, None]).astype(f32)
    return np.maximum(out, f32(0)) if relu else out


def exact_data(N, Cin, Cout, H, W, seed=0):
    """Inputs on which every partial sum of mc_conv_split is exact in fp32 in any order (exact_data_is_exact checks it).
    x = s (1 + b 2^-9), s = +-1, b in {1, 2, 3}: hi = s or s (1 + 2^-7), lo = +-2^-9 or s 2^-8, neither zero; about half of the interior
    pixels are zero instead (that keeps the sums small) and every border pixel is non-zero (so padding that is not zero shows).
    w = s (1 + b 2^-9) 2^-6, b odd in 1..61: hi a multiple of 2^-13, lo = +-2^-15; 62 values, any 62 consecutive (co, ci, tap) all
    different.  Every product of two parts is a multiple of 2^-22."""
    rng = np.random.default_rng(seed)
    s = rng.choice([-1.0, 1.0], (N, Cin, H, W))
    x = s * (1.0 + rng.integers(1, 4, (N, Cin, H, W)) * 2.0 ** -9)
    keep = rng.random((N, Cin, H, W)) < 0.5
    keep[:, :, [0, -1], :] = True
    keep[:, :, :, [0, -1]] = True
    x = np.where(keep, x, 0.0).astype(f32)
    idx = np.arange(Cout * Cin * 9).reshape(Cout, Cin, 3, 3)
    v = (idx * 37 + idx // 62) % 62
    w = (np.where(v % 2 == 0, 1.0, -1.0) * (1.0 + (2 * (v // 2) + 1) * 2.0 ** -9) * 2.0 ** -6).astype(f32)
    b = (rng.integers(-8, 9, Cout) * 2.0 ** -4).astype(f32)
    return x, w, b


def exact_data_is_exact(x, w):
    """True if every partial sum of the three split products, in any order, is an fp32 number: all parts non-zero where the value is,
    every product a multiple of 2^-22, and the sum of the products' magnitudes below 2^24 * 2^-22."""
    xhi, xlo = split(x)
    whi, wlo = split(w)
    nz = x != 0
    if not (np.all(xhi[nz] != 0) and np.all(xlo[nz] != 0) and np.all(whi != 0) and np.all(wlo != 0)):
        return False
    if not (np.array_equal(xhi.astype(f64) + xlo, x.astype(f64)) and np.array_equal(whi.astype(f64) + wlo, w.astype(f64))):
        return False
    grain = 2.0 ** -22
    for part, bits in ((xhi, 7), (xlo, 9), (whi, 13), (wlo, 15)):     # hi x hi, hi x lo, lo x hi: multiples of 2^-20, 2^-22, 2^-22
        if np.any(np.round(part.astype(f64) * 2 ** bits) != part.astype(f64) * 2 ** bits):
            return False
    bound = conv64(np.abs(xhi) + np.abs(xlo), np.abs(whi) + np.abs(wlo)).max()
    return bool(bound < 2 ** 24 * grain)
