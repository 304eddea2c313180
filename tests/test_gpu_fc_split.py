"""-m gpu: mc_fc_split_stack (libmcfcsplit.so, `-fc_mode bf16x3`): the accurate net's FC stack with every hidden-layer product taken as three
bf16 products, against the restatement of its arithmetic (tests/fc_split_oracle.py) and against the exact-product evaluation
(oracle.fc_stack).  Bars: NaN masks identical to the oracle's; within 1e-5 of the restatement on the sigmoid outputs (summation order
moves them by <= 1e-6, the smallest single missing term by 5e-5: tests/test_fc_split_host.py); within 1e-4 of the exact products, the
operator's bar (tests/test_gpu_fc.py)."""
import os

import numpy as np
import pytest

import fc_split_oracle as fo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VOXELS = 96      # MC_FC_SPLIT_VOXELS: voxels of one (y, d) per workgroup


def make_layers(C, n_hidden, seed, hidden_gain=1.0):
    """tests/test_gpu_fc.py's layers; hidden_gain 6 gives the hidden layers +-sqrt(6 / fan_in), under which six of them keep their spread"""
    rng = np.random.default_rng(seed)
    dims = [2 * C] + [384] * (n_hidden + 1) + [1]
    layers = []
    for i in range(len(dims) - 1):
        bound = (1.0 if i < len(dims) - 2 else 6.0) / np.sqrt(dims[i])
        if 0 < i < len(dims) - 2:
            bound = np.sqrt(hidden_gain) / np.sqrt(dims[i])
        layers.append((rng.uniform(-bound, bound, (dims[i + 1], dims[i])).astype(np.float32),
                       rng.uniform(-bound, bound, (dims[i + 1],)).astype(np.float32)))
    return layers


def device_layers(layers):
    return [(torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()) for w, b in layers]


CASES = [
    (8, 5, 50, 10, 3, 1.0), (16, 3, 100, 7, 2, 1.0), (112, 2, 40, 48, 3, 1.0), (4, 9, 97, 5, 1, 1.0),     # test_gpu_fc.py::test_fc_stack's (H = 9 among them)
    (5, 2, 60, 3, 0, 1.0),                  # no hidden layer, an odd C
    (7, 1, 70, 2, 6, 6.0),                  # six hidden layers (n_layers 8, the most), an odd C; measured 7.5e-6 from the restatement, the
                                            # accumulation's share over six layers that keep their scale (a missing term moves it by 2.1e-3)
    (4, 2, 6, 9, 1, 1.0),                   # D > W: disparities without a voxel
    (6, 2, VOXELS - 1, 3, 1, 1.0), (6, 2, VOXELS, 3, 1, 1.0), (6, 2, VOXELS + 1, 3, 1, 1.0), (6, 2, VOXELS + 2, 3, 1, 1.0),
    # ^ rows of 95, 96, 97 (d = 0) and, offset by the disparity, 94 .. 98 - d voxels: one below, at and one above a workgroup's 96
    (3, 9, 2 * VOXELS + 9, 12, 2, 1.0),     # three workgroups per row, two image rows on one XCD (H = 9)
]


@pytest.mark.parametrize("C,H,W,D,n_hidden,gain", CASES)
def test_fc_split_stack(mc, oracle, C, H, W, D, n_hidden, gain):
    from util import features
    from mc_cnn_amd.fc import fc_cost_volumes
    f = np.maximum(features(C, H, W, seed=C + W), 0) * 3.0
    layers = make_layers(C, n_hidden, seed=W, hidden_gain=gain)
    exact = oracle.fc_stack(f[0], f[1], D, layers)
    restated = fo.fc_split_stack(f[0], f[1], D, layers)
    vl, vr = fc_cost_volumes(torch.from_numpy(f).cuda(), device_layers(layers), D, mode="bf16x3")
    torch.cuda.synchronize()
    for got, want, rest, name in ((vl, exact[0], restated[0], "left"), (vr, exact[1], restated[1], "right")):
        g = got.cpu().numpy()[0]
        assert np.array_equal(np.isnan(g), np.isnan(want)), "%s: NaN mask differs" % name
        ok = ~np.isnan(want)
        e_rest, e_exact = np.abs(g[ok] - rest[ok]).max(), np.abs(g[ok] - want[ok]).max()
        print("%s: |kernel - restatement| %.3g, |kernel - exact| %.3g, std %.3g" % (name, e_rest, e_exact, want[ok].std()))
        assert e_rest <= 1e-5, "%s: max |kernel - restatement| = %g" % (name, e_rest)
        assert e_exact <= 1e-4, "%s: max |kernel - exact products| = %g" % (name, e_exact)
        assert want[ok].std() > 1e-3, want[ok].std()  # the comparison is not vacuous (outputs are not saturated)


def exact_case(seed=0):
    """Data on which every partial sum of the kernel is exact in fp32, so the lane maps show in the last bit:
      features in {0, 1, 2}, W1 in {0, 1} / 1024, b1[k] = I[k] + Jb[k] / 1024 with I in 4..7, Jb in 1..3
        -> h[k] = I[k] + J[k] / 1024, J = Jb + (features' part) in 1..11 < 16: hhi = I, hlo = J / 1024, both non-zero;
      hidden W[n,k] = s (P + Q / 1024), s = +-1, P in 1..2, Q in 1..3 -> Whi = s P, Wlo = s Q / 1024, both non-zero;
      z[n] = sum_k s (P I + (P J + Q I) / 1024): multiples of 2^-10 below 2^13 in any order, 23 bits; the dropped term is Q J / 2^20;
      b[n] puts z + b at 2 + (the voxel's part) / 1024, inside (0, 4): 12 bits below the point, so split(h') is exact as well."""
    rng = np.random.default_rng(seed)
    C, H, W, D = 2, 2, VOXELS + 5, 3
    f = rng.integers(0, 3, (2, C, H, W)).astype(np.float32)
    w1 = rng.integers(0, 2, (384, 2 * C)).astype(np.float32) / 1024
    I, Jb = rng.integers(4, 8, 384), rng.integers(1, 4, 384)
    b1 = (I + Jb / 1024).astype(np.float32)
    s, P, Q = rng.choice([-1, 1], (384, 384)), rng.integers(1, 3, (384, 384)), rng.integers(1, 4, (384, 384))
    wh = (s * (P + Q / 1024)).astype(np.float32)
    z0 = (s * P) @ I * 1024 + (s * P) @ Jb + (s * Q) @ I          # z * 1024 with the features at zero: integers
    bh = ((2048 - z0) / 1024).astype(np.float32)
    assert np.all(np.abs(z0) < 2 ** 23) and np.array_equal(bh.astype(np.float64) * 1024, 2048 - z0)
    # the expected logit per voxel and n, in integers: 2048 + sum_k s P (J - Jb), over 1024
    logit = np.full((384, D, H, W), np.nan)
    for d in range(D):
        jf = np.einsum("kc,chw->khw", np.rint(w1[:, :C] * 1024), f[0][:, :, d:]) + np.einsum("kc,chw->khw", np.rint(w1[:, C:] * 1024), f[1][:, :, :W - d])
        assert jf.max() + Jb.max() < 16
        logit[:, d, :, d:] = (2048 + np.einsum("nk,khw->nhw", s * P, jf)) / 1024
    assert np.nanmin(logit) > 0 and np.nanmax(logit) < 4
    return f, w1, b1, wh, bh, logit, D


def test_exact_data_lane_maps(mc):
    """One hidden layer, the output weights one-hot at n: the output is sigmoid(h'[n]) and h'[n] is known exactly.  The logit recovered
    from the output is held to one ulp of the sigmoid; a product at a wrong (n, k, voxel) moves it by 2^-10 or more, hundreds of ulps."""
    from mc_cnn_amd.fc import fc_cost_volumes
    f, w1, b1, wh, bh, logit, D = exact_case()
    ft = torch.from_numpy(f).cuda()
    head = device_layers([(w1, b1), (wh, bh)])
    worst = 0.0
    for n in list(range(0, 384, 7)) + [383]:           # every 32-row tile, wave, register group and lane half among them
        wl = np.zeros((1, 384), np.float32)
        wl[0, n] = 1.0
        vl, vr = fc_cost_volumes(ft, head + device_layers([(wl, np.zeros(1, np.float32))]), D, mode="bf16x3")
        out = vl.cpu().numpy()[0].astype(np.float64)
        ok = ~np.isnan(logit[n])
        assert np.array_equal(np.isnan(out), ~ok)
        o = out[ok]
        # the expected output is the exact logit's sigmoid rounded to fp32; both logits are recovered the same way, and one ulp of the
        # sigmoid (a step to the neighbouring fp32 value, what expf and the division may cost) is ulp / (o (1 - o)) of the logit
        want = (1.0 / (1.0 + np.exp(-logit[n][ok]))).astype(np.float32).astype(np.float64)
        got, ref = np.log(o / (1 - o)), np.log(want / (1 - want))
        ulp = np.spacing(want.astype(np.float32)).astype(np.float64) / (want * (1 - want))
        assert np.abs(ref - logit[n][ok]).max() < 2.0 ** -20                 # the rounding of the output, far below a granule 2^-10 of the data
        worst = max(worst, float((np.abs(got - ref) / ulp).max()))
        assert np.all(np.abs(got - ref) <= ulp * (1 + 1e-6)), "n %d: logit off by %g ulp of the sigmoid" % (n, (np.abs(got - ref) / ulp).max())
        r = vr.cpu().numpy()[0]
        for d in range(D):
            assert np.array_equal(r[d, :, :r.shape[2] - d], vl.cpu().numpy()[0][d, :, d:])
    print("worst logit error: %.3g ulp of the sigmoid" % worst)


def test_two_calls_on_two_streams_give_identical_results(mc):
    from util import features
    from mc_cnn_amd.fc import fc_cost_volumes
    C, H, W, D, n_hidden = 8, 9, 2 * VOXELS + 20, 12, 2
    ft = torch.from_numpy(np.maximum(features(C, H, W, seed=1), 0) * 3.0).cuda()
    dl = device_layers(make_layers(C, n_hidden, seed=2))
    alone = fc_cost_volumes(ft, dl, D, mode="bf16x3")
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = []
    for st in streams:                      # each call takes its own workspace; the two are in flight together
        with torch.cuda.stream(st):
            out.append(fc_cost_volumes(ft, dl, D, mode="bf16x3"))
    torch.cuda.synchronize()
    from util import same_bits
    for vl, vr in out:
        assert same_bits(vl.cpu().numpy(), alone[0].cpu().numpy()) and same_bits(vr.cpu().numpy(), alone[1].cpu().numpy())
    assert float(alone[0][~torch.isnan(alone[0])].std()) > 1e-3


def test_main_predict_arch_slow_bf16x3(mc, oracle, tmp_path, monkeypatch):
    """`main.py kitti slow -a predict -fc_mode bf16x3` at the set-up of test_gpu_fc.py::test_main_predict_arch_slow: the raw volumes
    within 1e-4 of the oracle, the .bin files bit-equal to the oracle pipeline run on those raw volumes; `-fc_mode fp32` writes what
    no flag writes, byte for byte."""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    from mc_cnn_amd import main as mcmain
    from util import diff_report, same_bits
    H, W, D = 24, 80, 12
    rng = np.random.default_rng(5)
    base = gaussian_filter(rng.random((H, W + 6)), 2.0)
    base = ((base - base.min()) / np.ptp(base) * 255).astype(np.uint8)
    Image.fromarray(base[:, 6:]).save(tmp_path / "L.png")
    Image.fromarray(base[:, :W]).save(tmp_path / "R.png")
    argv = ["kitti", "slow", "-a", "predict", "-net_fname", "random:3", "-left", str(tmp_path / "L.png"), "-right", str(tmp_path / "R.png"),
            "-disp_max", str(D)]
    files = {}
    for name, extra in (("none", []), ("fp32", ["-fc_mode", "fp32"]), ("bf16x3", ["-fc_mode", "bf16x3"])):
        os.makedirs(tmp_path / name)
        monkeypatch.chdir(tmp_path / name)
        assert mcmain.main(argv + extra) == 0
        files[name] = {k: open(k + ".bin", "rb").read() for k in ("left", "right", "disp")}
    assert files["fp32"] == files["none"]
    assert files["bf16x3"]["left"] != files["none"]["left"]               # the flag reached the FC stack
    disp, left, right = mc.read_bin("disp.bin", (1, 1, H, W)), mc.read_bin("left.bin", (1, D, H, W)), mc.read_bin("right.bin", (1, D, H, W))
    x0 = mcmain.normalize(mcmain.load_image(str(tmp_path / "L.png")))
    x1 = mcmain.normalize(mcmain.load_image(str(tmp_path / "R.png")))
    xb = torch.from_numpy(np.stack([x0, x1])).cuda()
    layers = mcmain.load_net("random:3", "kitti", "slow")
    fcl = mcmain.load_fc("random:3", "kitti")
    feat = mcmain.features_slow(xb, layers)
    vl, vr = mcmain.raw_volumes_slow(feat, fcl, D, len(layers), fc_mode="bf16x3")
    wl, wr = oracle.fc_stack(feat[0].cpu().numpy(), feat[1].cpu().numpy(), D, fcl)
    for got, want, direction in ((vl, wl, -1), (vr, wr, 1)):
        want = oracle.fix_border(want, len(layers), direction)
        ok = ~np.isnan(want)
        assert np.array_equal(np.isnan(got.cpu().numpy()[0]), np.isnan(want))
        assert np.abs(got.cpu().numpy()[0][ok] - want[ok]).max() <= 1e-4
    prm = dict(mc.TABLES[("kitti", "slow")])
    prm["border_n"] = len(layers)
    want = oracle.stereo_predict(prm, x0[0], x1[0], D, rawL=vl.cpu().numpy()[0], rawR=vr.cpu().numpy()[0])
    assert same_bits(left, want["volL"]), diff_report(left, want["volL"], "left.bin")
    assert same_bits(right, want["volR"]), diff_report(right, want["volR"], "right.bin")
    assert same_bits(disp, want["disp"]), diff_report(disp, want["disp"], "disp.bin")
