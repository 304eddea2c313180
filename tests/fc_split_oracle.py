"""The arithmetic of mc_fc_split_stack (include/mc_fc_split.h) restated in numpy: the accurate net's FC stack with every hidden-layer
product taken as three bf16 products of hi + lo parts.  Sums are accumulated in float64 and rounded to fp32 once, where the header
says "in fp32" (the kernel's summation order is the matrix cores'); every other rounding point is the header's.

    split(v): hi = bf16(v), round to nearest even; lo = bf16(v - float(hi))
    layer 1:  PL = W1[:, :C] L(x), PR = W1[:, C:] R(x) (fp32); h = max((PL[x] + PR[x-d]) + b1, 0)
    hidden:   z[n] = sum_k (Whi[n,k] hhi[k] + Whi[n,k] hlo[k] + Wlo[n,k] hhi[k]); h' = max(z + b, 0)
    output:   s = sum_k w[k] (float(hhi[k]) + float(hlo[k])), + b, 1 / (1 + exp(-s)): the kernel keeps activations only as (hhi, hlo),
              so the output layer reads the split of the last h, not its fp32 value
    results:  volL[d,y,x] and volR[d,y,x-d] for x >= d, NaN everywhere else
"""
import numpy as np

f32, f64 = np.float32, np.float64


def bf16(v):
    """v (float32, finite) rounded to bfloat16, to nearest even, as float32"""
    u = np.ascontiguousarray(v, dtype=f32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(f32).reshape(np.shape(v))


def split(v):
    v = np.asarray(v, dtype=f32)
    hi = bf16(v)
    return hi, bf16((v - hi).astype(f32))


def hidden_layer(h, w, b, drop=None):
    """h: (voxels, 384) fp32; w: (384, 384) (out, in); -> (voxels, 384) fp32.  drop: "hi.lo" or "lo.hi" leaves that cross term out (what a
    faulty kernel would compute: the tests measure how far that moves the result)."""
    hhi, hlo = split(h)
    whi, wlo = split(w)
    z = hhi.astype(f64) @ whi.astype(f64).T
    if drop != "hi.lo":
        z += hlo.astype(f64) @ whi.astype(f64).T     # Whi . hlo
    if drop != "lo.hi":
        z += hhi.astype(f64) @ wlo.astype(f64).T     # Wlo . hhi
    return np.maximum((z.astype(f32) + np.asarray(b, f32)).astype(f32), f32(0))


def output_layer(h, w, b):
    hhi, hlo = split(h)
    hs = (hhi + hlo).astype(f32)
    s = (hs.astype(f64) @ np.asarray(w, f32).reshape(-1).astype(f64)).astype(f32)
    s = (s + f32(np.asarray(b).reshape(-1)[0])).astype(f32)
    return (1.0 / (1.0 + np.exp(-s.astype(f64)))).astype(f32)


def fc_split_stack(featL, featR, D, layers, drop=None):
    """featL, featR: (C,H,W) fp32; layers: [(w (out,in), b (out))], the first with 2C inputs, the last with one output
    -> (volL, volR), each (D,H,W) fp32 with NaN where x < d (volL) / x >= W - d (volR)"""
    featL, featR = np.asarray(featL, f32), np.asarray(featR, f32)
    C, H, W = featL.shape
    w1, b1 = np.asarray(layers[0][0], f32), np.asarray(layers[0][1], f32)
    PL = np.einsum("nc,chw->hwn", w1[:, :C].astype(f64), featL.astype(f64)).astype(f32)
    PR = np.einsum("nc,chw->hwn", w1[:, C:].astype(f64), featR.astype(f64)).astype(f32)
    volL = np.full((D, H, W), np.nan, f32)
    volR = np.full((D, H, W), np.nan, f32)
    for d in range(min(D, W)):
        n = W - d
        h = np.maximum(((PL[:, d:] + PR[:, :n]).astype(f32) + b1).astype(f32), f32(0)).reshape(H * n, -1)
        for w, b in layers[1:-1]:
            h = hidden_layer(h, w, b, drop)
        r = output_layer(h, *layers[-1]).reshape(H, n)
        volL[d, :, d:] = r
        volR[d, :, :n] = r
    return volL, volR
