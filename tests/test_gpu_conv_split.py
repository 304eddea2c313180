"""-m gpu: mc_conv_split (libmcconvsplit.so, `-conv_mode bf16x3`): the feature nets' 3x3 convolution with every product taken as three bf16
products, against the restatement of its arithmetic (tests/conv_split_oracle.py) and against a float64 convolution.  Bars: within
1e-5 * max(1, scale) of the restatement (the fp32 summation order moves an output by <= 9.4e-7, the smallest single missing cross term by
1.5e-3: tests/test_conv_split_host.py holds both at every shape used here); within 1e-4 * max(1, scale) of float64, the operator's bar
(tests/test_gpu_conv.py)."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import conv_split_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def gpu_conv(mc, x, w, b, relu, mode="bf16x3"):
    from mc_cnn_amd import adcensus
    out = adcensus.conv3x3(dev(x), dev(w), dev(b), relu, mode=mode)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("N,Cin,Cout,H,W,relu", co.CASES)
def test_conv_split(mc, N, Cin, Cout, H, W, relu):
    x, w, b = co.inputs(N, Cin, Cout, H, W)
    exact = co.conv_f64(x, w, b, relu)
    restated = co.conv_split(x, w, b, relu)
    got = gpu_conv(mc, x, w, b, relu)
    scale = float(np.abs(exact).max())
    err_r, err_e = float(np.abs(got - restated).max()), float(np.abs(got - exact).max())
    print("%s: scale %.3g, vs restatement %.3g, vs float64 %.3g" % ((N, Cin, Cout, H, W, relu), scale, err_r, err_e))
    assert got.shape == exact.shape and np.isfinite(got).all()
    assert err_r <= 1e-5 * max(1.0, scale), "vs the restatement: max |diff| = %g (scale %g)" % (err_r, scale)
    assert err_e <= 1e-4 * max(1.0, scale), "vs float64: max |diff| = %g (scale %g)" % (err_e, scale)


@pytest.mark.parametrize("N,Cin,Cout,H,W", [(2, 32, 40, 21, 37), (1, 16, 70, 17, 33)])
def test_exact_data_lane_maps(mc, N, Cin, Cout, H, W):
    """Data on which every partial sum is exact in fp32 in any order: the output equals the restatement bit for bit.  A swapped or
    missing cross term, a wrong tap or channel index, or padding that is not zero each change bits."""
    from util import diff_report, same_bits
    x, w, b = co.exact_data(N, Cin, Cout, H, W)
    assert co.exact_data_is_exact(x, w)
    assert np.all(x[:, :, [0, -1], :] != 0) and np.all(x[:, :, :, [0, -1]] != 0)
    for relu in (False, True):
        want = co.conv_split(x, w, b, relu)
        got = gpu_conv(mc, x, w, b, relu)
        assert same_bits(got, want), diff_report(got, want, "exact data, relu %s" % relu)
    want = co.conv_split(x, w, b, False)
    for drop in ("hi.lo", "lo.hi"):
        assert not same_bits(co.conv_split(x, w, b, False, drop=drop), want)     # the data sees either term


@pytest.mark.parametrize("Cin,Cout", [(1, 64), (3, 7)])
def test_ineligible_layers_take_the_fp32_kernel(mc, Cin, Cout):
    from util import same_bits
    x, w, b = co.inputs(2, Cin, Cout, 24, 50)
    a = gpu_conv(mc, x, w, b, True, mode="bf16x3")
    f = gpu_conv(mc, x, w, b, True, mode="fp32")
    assert same_bits(a, f) and np.abs(f).max() > 0.1
    from mc_cnn_amd import adcensus
    with pytest.raises(ValueError, match="fp32 | bf16x3"):
        adcensus.conv3x3(dev(x), dev(w), dev(b), True, mode="bf16")


def test_streams_and_threads_do_not_disturb_each_other(mc):
    """Two calls on two streams, then four threads on four streams, each with its own layer: bit-identical to one call alone."""
    from mc_cnn_amd import adcensus
    from util import same_bits
    shapes = [(2, 64, 64, 40, 70), (1, 112, 112, 30, 45), (2, 32, 100, 33, 40), (1, 16, 24, 50, 65)]
    data = [tuple(dev(a) for a in co.inputs(*s)) for s in shapes]
    alone = [adcensus.conv3x3(x, w, b, True, mode="bf16x3") for x, w, b in data]
    torch.cuda.synchronize()
    alone = [a.cpu().numpy() for a in alone]
    assert all(np.abs(a).max() > 0.1 for a in alone)
    streams = [torch.cuda.Stream() for _ in shapes]
    outs = [None] * len(shapes)
    for i in range(2):
        with torch.cuda.stream(streams[i]):
            for _ in range(3):
                outs[i] = adcensus.conv3x3(*data[i], True, mode="bf16x3")
    torch.cuda.synchronize()
    for i in range(2):
        assert same_bits(outs[i].cpu().numpy(), alone[i])
    outs = [None] * len(shapes)
    errors = []

    def work(i):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[i]):
                for _ in range(3):
                    outs[i] = adcensus.conv3x3(*data[i], True, mode="bf16x3")
            streams[i].synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(shapes))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(len(shapes)):
        assert same_bits(outs[i].cpu().numpy(), alone[i])


@pytest.mark.parametrize("arch", ["fast", "slow"])
def test_feature_nets(mc, arch):
    """features_fast / features_slow under bf16x3 on 2 x 1 x 24 x 50 with random:3: within 1e-4 of the fp32 features, not bit-equal to
    them (the mode was taken), unit-norm for arch fast as the fp32 features are."""
    from mc_cnn_amd import main as mcmain
    layers = mcmain.load_net("random:3", "kitti", arch)
    xb = dev(np.random.default_rng(0).standard_normal((2, 1, 24, 50)))
    f = mcmain.features_fast if arch == "fast" else mcmain.features_slow
    a, b = f(xb, layers, "bf16x3"), f(xb, layers, "fp32")
    c = f(xb, layers)
    torch.cuda.synchronize()
    a, b, c = a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy()
    assert np.array_equal(b, c)                       # the default is fp32
    err = float(np.abs(a - b).max())
    print("arch %s: max |bf16x3 - fp32| = %.3g, scale %.3g" % (arch, err, np.abs(b).max()))
    assert a.shape == b.shape and err <= 1e-4 and not np.array_equal(a, b)
    if arch == "fast":
        # Normalize2 divides by sqrt(sum x^2 + 1e-5) (adcensus.cu:1284-1308), so a pixel's norm is sqrt(s / (s + 1e-5)): below 1 by
        # 5e-6 / s, the same under both modes up to the rounding of 64 fp32 values (64 * 2^-24 = 4e-6) -- the modes' s differ by 1e-4
        # relative at most, which moves 5e-6 / s by 5e-10 / s
        na, nb = (np.sqrt((v.astype(np.float64) ** 2).sum(1)) for v in (a, b))
        print("norms: bf16x3 %.6f .. %.6f, fp32 %.6f .. %.6f, max |difference| %.3g" % (na.min(), na.max(), nb.min(), nb.max(), np.abs(na - nb).max()))
        assert na.max() <= 1.0 + 4e-6 and na.min() >= 0.999 and np.abs(na - nb).max() <= 8e-6


def test_main_predict_arch_fast_bf16x3(mc, oracle, tmp_path, monkeypatch):
    """`main.py kitti fast -a predict -conv_mode bf16x3` at the set-up of test_gpu_parity.py::test_main_predict_writes_the_reference_files:
    the .bin files bit-equal to the oracle pipeline run on the bf16x3 features; `-conv_mode fp32` writes what no flag writes, byte for
    byte."""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    from mc_cnn_amd import main as mcmain
    from util import diff_report, same_bits
    H, W, D = 40, 96, 24
    rng = np.random.default_rng(3)
    base = gaussian_filter(rng.random((H, W + 8)), 2.0)
    base = ((base - base.min()) / np.ptp(base) * 255).astype(np.uint8)
    Image.fromarray(base[:, 8:]).save(tmp_path / "L.png")
    Image.fromarray(base[:, :W]).save(tmp_path / "R.png")
    argv = ["kitti", "fast", "-a", "predict", "-net_fname", "random:7", "-left", str(tmp_path / "L.png"), "-right", str(tmp_path / "R.png"),
            "-disp_max", str(D)]
    files = {}
    for name, extra in (("none", []), ("fp32", ["-conv_mode", "fp32"]), ("bf16x3", ["-conv_mode", "bf16x3"])):
        os.makedirs(tmp_path / name)
        monkeypatch.chdir(tmp_path / name)
        assert mcmain.main(argv + extra) == 0
        files[name] = {k: open(k + ".bin", "rb").read() for k in ("left", "right", "disp")}
    assert files["fp32"] == files["none"]
    assert files["bf16x3"]["left"] != files["none"]["left"]              # the flag reached the convolutions
    disp, left, right = mc.read_bin("disp.bin", (1, 1, H, W)), mc.read_bin("left.bin", (1, D, H, W)), mc.read_bin("right.bin", (1, D, H, W))
    x0 = mcmain.normalize(mcmain.load_image(str(tmp_path / "L.png")))
    x1 = mcmain.normalize(mcmain.load_image(str(tmp_path / "R.png")))
    layers = mcmain.load_net("random:7", "kitti", "fast")
    feat = mcmain.features_fast(dev(np.stack([x0, x1])), layers, "bf16x3").cpu().numpy()
    prm = dict(mc.TABLES[("kitti", "fast")])
    prm["border_n"] = len(layers)
    want = oracle.stereo_predict(prm, x0[0], x1[0], D, featL=feat[0], featR=feat[1])
    assert same_bits(left, want["volL"]), diff_report(left, want["volL"], "left.bin")
    assert same_bits(right, want["volR"]), diff_report(right, want["volR"], "right.bin")
    assert same_bits(disp, want["disp"]), diff_report(disp, want["disp"], "disp.bin")


def test_main_predict_arch_slow_both_modes(mc, oracle, tmp_path, monkeypatch):
    """`main.py kitti slow -a predict -conv_mode bf16x3 -fc_mode bf16x3` runs; its raw volumes (features and FC stack both split) are
    within 1e-4 of the oracle's FC stack on the fp32 features."""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    from mc_cnn_amd import main as mcmain
    H, W, D = 24, 80, 12
    rng = np.random.default_rng(5)
    base = gaussian_filter(rng.random((H, W + 6)), 2.0)
    base = ((base - base.min()) / np.ptp(base) * 255).astype(np.uint8)
    Image.fromarray(base[:, 6:]).save(tmp_path / "L.png")
    Image.fromarray(base[:, :W]).save(tmp_path / "R.png")
    monkeypatch.chdir(tmp_path)
    assert mcmain.main(["kitti", "slow", "-a", "predict", "-net_fname", "random:3", "-left", "L.png", "-right", "R.png", "-disp_max", str(D),
                        "-conv_mode", "bf16x3", "-fc_mode", "bf16x3"]) == 0
    assert (tmp_path / "disp.bin").stat().st_size == 4 * H * W and (tmp_path / "left.bin").stat().st_size == 4 * D * H * W
    x0 = mcmain.normalize(mcmain.load_image("L.png"))
    x1 = mcmain.normalize(mcmain.load_image("R.png"))
    xb = dev(np.stack([x0, x1]))
    layers = mcmain.load_net("random:3", "kitti", "slow")
    fcl = mcmain.load_fc("random:3", "kitti")
    vl, vr = mcmain.raw_volumes_slow(mcmain.features_slow(xb, layers, "bf16x3"), fcl, D, len(layers), fc_mode="bf16x3")
    feat = mcmain.features_slow(xb, layers).cpu().numpy()
    wl, wr = oracle.fc_stack(feat[0], feat[1], D, fcl)
    for got, want, direction in ((vl, wl, -1), (vr, wr, 1)):
        want = oracle.fix_border(want, len(layers), direction)
        ok = ~np.isnan(want)
        g = got.cpu().numpy()[0]
        assert np.array_equal(np.isnan(g), np.isnan(want))
        err = float(np.abs(g[ok] - want[ok]).max())
        print("raw volumes, both modes bf16x3, vs the oracle: %.3g" % err)
        assert err <= 1e-4


def test_evalset_score_equals_main_py_under_bf16x3(tmp_path, monkeypatch, capsys):
    """EvalSet with conv_mode bf16x3 scores what `main.py kitti fast -a test_te -conv_mode bf16x3` prints last, on the tests' synthetic
    KITTI set."""
    from train_fixtures import write_synthetic_kitti
    from mc_cnn_amd import hs
    from mc_cnn_amd import main as mcmain
    from mc_cnn_amd.evalset import EvalSet
    write_synthetic_kitti(str(tmp_path / "data.kitti"))
    monkeypatch.chdir(tmp_path)
    opt = hs.parse(["random", "kitti", "fast", "test_te", "random:3", "-disp_max", "32", "-conv_mode", "bf16x3"])
    assert opt.conv_mode == "bf16x3"
    layers, fc = hs.check_net("random:3", "kitti", "fast")
    es = EvalSet("kitti", "fast", opt, layers, fc, torch.device("cuda", 0), 1 << 30)
    assert es.conv_mode == "bf16x3"
    got = es.score(dict(es.prm))
    capsys.readouterr()
    assert mcmain.main(["kitti", "fast", "-a", "test_te", "-net_fname", "random:3", "-disp_max", "32", "-conv_mode", "bf16x3"]) == 0
    want = float(capsys.readouterr().out.strip().splitlines()[-1])
    print("test_te under bf16x3: EvalSet %r, main.py %r" % (got, want))
    assert got == want
