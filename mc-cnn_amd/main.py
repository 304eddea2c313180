"""`main.lua -a predict` / `-a time` on MI355X: the host side of the reference's predict path in Python.

    python -m mc_cnn_amd.main kitti fast -a predict -net_fname NET -left L.png -right R.png -disp_max 70

mirrors `./main.lua kitti fast -a predict ...` (main.lua:10-32 flags, 1084-1105 action): loads the two images, converts
RGB to luma, normalises each to zero mean / unit (unbiased) std on the host, uploads (2,1,H,W), runs the feature net
(arch fast: l1 x [3x3 conv, pad 1, ReLU] with no ReLU after the last conv, then Normalize2 -- main.lua:727-746; the
convolutions are `mc_conv3x3`, a hand-written fp32-MFMA implicit GEMM of libmcadcensus.so, like everything after them), then the post-CNN
pipeline in one `mc_predict` call, and writes `left.bin`, `right.bin` (1,D,H,W) and `disp.bin` (1,1,H,W), raw float32,
with the reference's messages.  `-a time` is main.lua:1140-1167 (min of N runs on an uninitialised batch).  `-a predict -extras` also
writes `outlier.bin`, `cost.bin` and `curvature.bin` (1,1,H,W) next to `disp.bin`: the LR check's class of every pixel (0 match, 1 occlusion,
2 mismatch) and the two confidence measures of the sub-pixel stage (`mc_predict_ex`; no counterpart in main.lua).  `-a predict -right_view`
also writes `disp_right.bin` (1,1,H,W), the RIGHT view's finished disparity map -- the post-processing on the x-mirrored arg-min maps and
right volume, mirrored back (`mc_predict_views`) -- and, with `-extras`, its classes as `outlier_right.bin`.  `-a predict -margins` also
writes `c1.bin`, `c2.bin` and `c2l.bin` (1,1,H,W), the margins of every pixel's cost curve in the final left volume (`mc_cost_margins`: its
minimum, the runner-up and the runner-up among its local minima), and with `-right_view` `c1_right.bin`, `c2_right.bin` and `c2l_right.bin`
from the final right volume.

Architectures: fast, slow (feature net + `mc_fc_stack`, main.lua:958-983; `-fc_mode bf16x3` takes the FC stack's products as three
bf16 products each, `mc_fc_split_stack` of libmcfcsplit.so, wherever arch slow predicts; the default `-fc_mode fp32` is `mc_fc_stack`;
`-conv_mode bf16x3` does the same for the 16n -> Cout convolutions of either feature net, `mc_conv_split` of libmcconvsplit.so, default
`-conv_mode fp32` = `mc_conv3x3`), ad and census (no net: `mc_ad` / `mc_census_ws`
volumes from the image pair, main.lua:932-942).

-net_fname: the reference's Torch7 `net_*.t7` (main.lua:892-902; read by `t7.py`), an `.npz` with arrays
w1,b1,...,w<l1>,b<l1> (w_i: (fm, in, 3, 3); arch slow also fw1,fb1,...), or `random:<seed>` for a seeded random net
(`-a train_tr` trains one: see below).  Hyper-parameter flags (-L1 -tau1 -cbca_i1 -cbca_i2 -pi1 -pi2 -sgm_i
-sgm_q1 -sgm_q2 -alpha1 -tau_so -blur_sigma -blur_t) default to main.lua's per-(dataset, arch) tables.

Arch fast takes main.lua's net flags: -l1 (3x3 convolutions, 1..5; default NET_SHAPES: 4 on kitti / kitti2015, 5 on mb), -fm
(64 only) and -ks (3 only).  -l1 sizes a `random:` or `.npz` net (a `.t7` carries its own depth) and, where it is not the
default, sends -a train_tr | train_all through train_depth.py (libmctraindepth.so: the same step at any depth, on either image
store); `route` is where that is decided.  -L1 is another flag, the cross arm length.  The three flags are refused on slow, ad
and census.

Arch slow takes main.lua's FC flags: -l2 (hidden Linears, 1..7; default FC_SHAPES: 4 on kitti / kitti2015, 3 on mb) and -nh2 (384
only: mc_fc_stack and mc_fc_split_stack are 384 wide).  -l2 sizes a `random:` or `.npz` net wherever the command line predicts (a
`.t7` carries its own depth) and, where it is not the default, sends -a train_tr | train_all through train_slow_depth.py
(libmctrainslowdepth.so: the accurate net's step with l2 given at run time, on either image store); `route` decides that too.  The
two flags are refused on fast, ad and census; -l1 / -fm / -ks stay refused on slow.

`-a train_tr | train_all` (kitti | kitti2015; main.lua:602-890) train the net on the GPU from `-data_dir` (arch fast:
train.py, libmctrain.so; arch slow: train_slow.py, libmctrainslow.so, with train_slow.parse's flags) and save
net/net_<args>.t7; train_tr then runs test_te.  `training_module` is the one routing table of the four trainable nets, whose
shared host side is train_common.py.  `-a test_te | test_all`
(main.lua:1121-1138, 1172-1293) predict the dataset's test (all) pairs with -net_fname and print `runtime err` per pair and
the mean error.  Training flags keep main.lua's names and defaults; -epochs and -max_steps shorten a run.  `-at 1` trains
and tests on data.kitti and data.kitti2015 together (main.lua:403-426).  `python -m mc_cnn_amd.preprocess_kitti` writes
both sets from the KITTI archives (preprocess_kitti.lua).  `mb fast -a train_tr | train_all | test_te` train and test
Middlebury's five-layer fast net (train_mb.py, libmctrainmb.so, with train_mb.parse's flags) and
`mb slow -a train_tr | train_all | test_te` its accurate net (train_mb_slow.py, libmctrainmbslow.so, with
train_mb_slow.parse's flags) from preprocess_mb.py's `data.mb.<rect>_<color>`; -a test_all on mb and -a submit are out of
scope.
"""
import sys
import time

import numpy as np

from .binio import write_bin
from .params import NET_SHAPES, TABLES
from .train_common import (add_conv_mode_flag, add_fc_flags, add_fc_mode_flag, add_net_flags, check_conv_mode, check_fc_flags, check_fc_mode,
                           check_net_flags, new_parser, pipeline_prm, refuse_fc_flags, refuse_net_flags)


def rgb2y(img):
    """image.rgb2y: Y = 0.299 R + 0.587 G + 0.114 B on a (3,H,W) float tensor."""
    return (0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2])[None]


def load_image(path):
    """image.load(path, nil, 'byte'):float() -> (C,H,W) float32 in 0..255."""
    from PIL import Image
    a = np.asarray(Image.open(path))
    if a.ndim == 2:
        a = a[None]
    else:
        a = np.transpose(a[:, :, :3], (2, 0, 1))
    return a.astype(np.float32)


def normalize(x):
    """x:add(-x:mean()):div(x:std()) -- torch's unbiased std, accumulations in double (main.lua:1095-1096)."""
    # in the reference's order: the mean is subtracted in float32 first, then the std of THAT tensor divides it
    y = (x - np.float32(x.astype(np.float64).mean())).astype(np.float32)
    return (y / np.float32(y.astype(np.float64).std(ddof=1))).astype(np.float32)


def parse(argv):
    if len(argv) < 2 or argv[0] not in ("kitti", "kitti2015", "mb") or argv[1] not in ("fast", "slow", "ad", "census"):
        raise SystemExit("usage: main.py {kitti|kitti2015|mb} {fast|slow|ad|census} -a {predict|time|train_tr|train_all|test_te|"
                         "test_all} [flags]  (main.lua:10-13)")
    dataset, arch = argv[0], argv[1]
    refuse_net_flags(argv, "main.py")
    refuse_fc_flags(argv, "main.py")
    t = TABLES[(dataset, arch)]
    ap = new_parser(dataset, arch, t, FAST_TRAIN_DEFAULTS)
    if arch == "fast":
        add_net_flags(ap, dataset, arch)
    if arch == "slow":
        add_fc_flags(ap, dataset)
    ap.add_argument("-a", default="predict", choices=["predict", "time"] + list(TRAIN_ACTIONS) + ["submit"])
    ap.add_argument("-left", default="")
    ap.add_argument("-right", default="")
    ap.add_argument("-disp_max", type=int, default=228 if dataset != "mb" else 200)
    ap.add_argument("-tiny", action="store_true")
    ap.add_argument("-extras", action="store_true", help="-a predict: also write outlier.bin, cost.bin and curvature.bin (mc_predict_ex)")
    ap.add_argument("-right_view", action="store_true",
                    help="-a predict: also write disp_right.bin, the right view's finished disparity map (mc_predict_views); with -extras also outlier_right.bin")
    ap.add_argument("-margins", action="store_true",
                    help="-a predict: also write c1.bin, c2.bin and c2l.bin, the margins of the final left volume's cost curves (mc_cost_margins); "
                         "with -right_view also c1_right.bin, c2_right.bin and c2l_right.bin")
    add_fc_mode_flag(ap)
    add_conv_mode_flag(ap)
    ap.add_argument("-data_dir", default="", help="default data.kitti / data.kitti2015 (main.lua:427-445)")
    if dataset in ("kitti", "kitti2015"):
        ap.add_argument("-at", type=int, default=0, choices=(0, 1),
                        help="1: train on KITTI 2012 and 2015 together (main.lua:72,208,236, 403-426)")
    opt = ap.parse_args(argv[2:])
    if arch == "fast":
        check_net_flags(opt, "main.py")
    if arch == "slow":
        check_fc_flags(opt, "main.py")
    check_fc_mode(opt, arch, "main.py")
    check_conv_mode(opt, arch, "main.py")
    if opt.a not in ("predict", "time") and (opt.a not in TRAIN_ACTIONS or dataset not in ("kitti", "kitti2015") or arch != "fast"):
        raise SystemExit("main.py: -a %s is not supported for %s %s; training and testing cover -a %s for "
                         "{kitti|kitti2015} fast only (arch slow trains through train_slow.parse, which main() routes "
                         "{kitti|kitti2015} slow to, mb fast -a train_tr | train_all | test_te through train_mb.parse, mb slow "
                         "-a train_tr | train_all | test_te through train_mb_slow.parse; -a test_all on mb and -a submit are "
                         "out of scope)"
                         % (opt.a, dataset, arch, " | ".join(TRAIN_ACTIONS)))
    if opt.extras and opt.a != "predict":
        raise SystemExit("main.py: -extras writes outlier.bin, cost.bin and curvature.bin next to disp.bin and goes with -a predict only")
    if opt.right_view and opt.a != "predict":
        raise SystemExit("main.py: -right_view writes disp_right.bin next to disp.bin and goes with -a predict only")
    if opt.margins and opt.a != "predict":
        raise SystemExit("main.py: -margins writes c1.bin, c2.bin and c2l.bin next to disp.bin and goes with -a predict only")
    if getattr(opt, "at", 0) == 1 and opt.data_dir:
        raise SystemExit("main.py: -at 1 reads data.kitti and data.kitti2015 together (main.lua:403-426) and takes no -data_dir")
    return dataset, arch, opt, pipeline_prm(t, opt)


TRAIN_ACTIONS = ("train_tr", "train_all", "test_te", "test_all")

FAST_TRAIN_DEFAULTS = dict(m=0.2, pow=1, lr=0.002, bs=128, mom=0.9, true1=1, false1=4, false2=10)   # main.lua:207-220, 236-248

FC_SHAPES = {"kitti": (4, 384), "kitti2015": (4, 384), "mb": (3, 384)}  # (l2, nh2), main.lua:76-77, 123-124


_t7_cache = {}   # the latest parsed .t7: arch slow reads its two nets from one file, and an ASCII net of 870 449 floats parses in seconds


def reference_nets(net_fname, arch):
    """t7.load_reference_net, parsed once per (file, size, mtime)."""
    import os
    from . import t7
    st = os.stat(net_fname)
    key = (os.path.abspath(net_fname), arch, st.st_size, st.st_mtime_ns)
    if key not in _t7_cache:
        _t7_cache.clear()
        _t7_cache[key] = t7.load_reference_net(net_fname, arch)
    return _t7_cache[key]


def load_net(net_fname, dataset, arch, n_input_plane=1, l1=None):
    """[(w, b)] of the feature net: from the reference's `.t7` (torch.save(..., 'ascii'), main.lua:587-600), an .npz, or
    seeded random (`random:<seed>`).  l1: the -l1 of a fast net where it is not the data set's (a `.t7` carries its own)."""
    default_l1, fm = NET_SHAPES[(dataset, arch)]
    l1 = default_l1 if l1 is None else l1
    if net_fname.endswith(".t7"):
        layers = reference_nets(net_fname, arch)[0]
        if not layers:
            raise ValueError("%s: no SpatialConvolution modules found" % net_fname)
        return layers
    if net_fname.startswith("random:"):
        rng = np.random.default_rng(int(net_fname.split(":")[1]))
        layers = []
        for i in range(l1):
            cin = n_input_plane if i == 0 else fm
            bound = 1.0 / np.sqrt(cin * 9)  # nn.SpatialConvolution:reset() range
            layers.append((rng.uniform(-bound, bound, (fm, cin, 3, 3)).astype(np.float32),
                           rng.uniform(-bound, bound, (fm,)).astype(np.float32)))
        return layers
    z = np.load(net_fname)
    return [(z["w%d" % (i + 1)].astype(np.float32), z["b%d" % (i + 1)].astype(np.float32)) for i in range(l1)]


def load_fc(net_fname, dataset, l2=None):
    """[(w (out,in), b (out))] of net_te2 (arch slow, main.lua:688-695): from the reference's `.t7`, an .npz (fw1,fb1,...)
    or seeded random.  l2: the -l2 of a net with another number of hidden Linears than the data set's (a `.t7` carries its own);
    a random net's layers are drawn in order, so its first ones are the same at every depth."""
    l1, fm = NET_SHAPES[(dataset, "slow")]
    if net_fname.endswith(".t7"):
        fc = reference_nets(net_fname, "slow")[1]
        if not fc:
            raise ValueError("%s: no SpatialConvolution1_fw modules found" % net_fname)
        return fc
    default_l2, nh2 = FC_SHAPES[dataset]
    l2 = default_l2 if l2 is None else l2
    dims = [2 * fm] + [nh2] * l2 + [1]
    if net_fname.startswith("random:"):
        rng = np.random.default_rng(int(net_fname.split(":")[1]) + 1)
        out = []
        for i in range(len(dims) - 1):
            bound = (1.0 if i < len(dims) - 2 else 6.0) / np.sqrt(dims[i])
            out.append((rng.uniform(-bound, bound, (dims[i + 1], dims[i])).astype(np.float32),
                        rng.uniform(-bound, bound, (dims[i + 1],)).astype(np.float32)))
        return out
    z = np.load(net_fname)
    return [(z["fw%d" % (i + 1)].astype(np.float32), z["fb%d" % (i + 1)].astype(np.float32)) for i in range(len(dims) - 1)]


def device_layers(layers, device):
    """[(w, b)] as float32 tensors on `device`: upload a net once, not once per call."""
    import torch
    return [tuple(t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).to(device) for t in wb)
            for wb in layers]


def features_slow(x_batch, layers, conv_mode="fp32"):
    """forward_free(net_te, x_batch) for arch slow (main.lua:681-686): l1 x [3x3 conv, pad 1, ReLU].  conv_mode: adcensus.conv3x3's
    mode, "fp32" (mc_conv3x3) or "bf16x3" (mc_conv_split for every layer it takes: all but the first)."""
    from . import adcensus
    h = x_batch.contiguous()
    for w, b in device_layers(layers, h.device):
        h = adcensus.conv3x3(h, w, b, relu=True, mode=conv_mode)
    return h


def raw_volumes_slow(feat, fc_layers, disp_max, border_n, fc_mode="fp32"):
    """main.lua:958-983: the FC stack for every (pixel, disparity) -> NaN-filled volumes, then fix_border.  fc_mode: fc.fc_cost_volumes'
    mode, "fp32" (mc_fc_stack) or "bf16x3" (mc_fc_split_stack)."""
    import torch
    from . import adcensus
    from .fc import fc_cost_volumes
    dl = [(torch.from_numpy(w).to(feat.device), torch.from_numpy(b).to(feat.device)) for w, b in fc_layers]
    vl, vr = fc_cost_volumes(feat, dl, disp_max, mode=fc_mode)
    adcensus.fix_border(vl, border_n, -1)
    adcensus.fix_border(vr, border_n, 1)
    return vl, vr


def features_fast(x_batch, layers, conv_mode="fp32"):
    """forward_free(net_te, x_batch) for arch fast (main.lua:945): convs (pad 1) + ReLU between, then Normalize2.  conv_mode: as
    features_slow's."""
    import torch
    from . import adcensus
    h = x_batch.contiguous()
    layers = device_layers(layers, h.device)
    for i, (w, b) in enumerate(layers):
        h = adcensus.conv3x3(h, w, b, relu=i < len(layers) - 1, mode=conv_mode)
    norm = torch.empty((h.shape[0], 1) + tuple(h.shape[2:]), dtype=torch.float32, device=h.device)
    out = torch.empty_like(h)
    adcensus.Normalize_forward(h, norm, out)   # Normalize2.lua:8-13 -> adcensus.cu:1310-1333
    return out


def training_module(argv):
    """The module whose `parse` takes argv, with its `train` and `evaluate`: train_slow for {kitti|kitti2015} slow, train_mb for
    mb fast and train_mb_slow for mb slow, each with `-a` one of its ACTIONS.  None for every other command line: `parse`
    above takes or refuses those ({kitti|kitti2015} fast trains through train.py)."""
    if len(argv) < 2 or "-a" not in argv[2:-1]:
        return None
    from . import train_mb, train_mb_slow, train_slow
    routes = {("kitti", "slow"): train_slow, ("kitti2015", "slow"): train_slow, ("mb", "fast"): train_mb, ("mb", "slow"): train_mb_slow}
    mod = routes.get((argv[0], argv[1]))
    return mod if mod is not None and argv[argv.index("-a", 2) + 1] in mod.ACTIONS else None


def route(argv):
    """(mod, trainer, dataset, arch, opt, prm) of a command line: mod is `training_module(argv)`, whose `parse` gave the rest
    (None: `parse` above did); trainer is the module whose `train` runs -a train_tr | train_all: train_depth for arch fast with
    a -l1 other than the data set's (libmctraindepth.so), train_slow_depth for arch slow with a -l2 other than the data set's
    (libmctrainslowdepth.so), otherwise mod, or train where mod is None.  The default depth, written or not, keeps the older
    libraries."""
    mod = training_module(argv)
    dataset, arch, opt, prm = parse(argv) if mod is None else mod.parse(argv)
    trainer = mod
    if arch == "fast" and opt.a in TRAIN_ACTIONS:
        if opt.l1 != NET_SHAPES[(dataset, arch)][0]:
            from . import train_depth as trainer
        elif mod is None:
            from . import train as trainer
    if arch == "slow" and opt.a in ("train_tr", "train_all") and opt.l2 != FC_SHAPES[dataset][0]:
        from . import train_slow_depth as trainer
    return mod, trainer, dataset, arch, opt, prm


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    mod, trainer, dataset, arch, opt, prm = route(argv)
    import torch
    from .predict import Workspace, stereo_predict_fused
    if arch not in ("fast", "slow", "ad", "census"):
        raise SystemExit("main.py: unknown architecture %r (main.lua:11: fast | slow | ad | census)" % arch)
    dev = torch.device("cuda", opt.gpu - 1)
    torch.cuda.set_device(dev)
    learned = arch in ("fast", "slow")
    l1 = getattr(opt, "l1", None)         # arch fast: the depth of a random: or .npz net
    layers = device_layers(load_net(opt.net_fname, dataset, arch, l1=l1), dev) if learned else []   # resident: uploaded once
    fc_layers = load_fc(opt.net_fname, dataset, l2=getattr(opt, "l2", None)) if arch == "slow" else None   # -l2: as -l1 above
    prm["border_n"] = len(layers)  # (1 + l1*(3-1) - 1) / 2, main.lua:382-391,923
    conv_mode = getattr(opt, "conv_mode", "fp32")   # the feature net's convolutions wherever this command line predicts

    def run(x_batch, D, workspace=None, want_volumes=False, extras=False, right_view=False, margins=False):
        more = dict(want_outlier=True, want_confidence=True) if extras else {}   # -extras: mc_predict_ex's three maps
        if right_view:                                                          # -right_view: mc_predict_views' two
            more["want_right"] = True
        if margins:                                                             # -margins: mc_cost_margins' three, per view
            more["want_margins"] = True
        if not learned:  # main.lua:932-942: hand-crafted costs straight from the image pair, no border fix
            from . import adcensus
            cost = adcensus.ad if arch == "ad" else adcensus.census
            H, W = x_batch.shape[2:]
            volL = torch.empty((1, D, H, W), dtype=torch.float32, device=x_batch.device)
            volR = torch.empty_like(volL)
            adcensus.fill_nan(volL)
            adcensus.fill_nan(volR)
            cost(x_batch[0:1], x_batch[1:2], volL, -1)
            cost(x_batch[1:2], x_batch[0:1], volR, 1)
            return stereo_predict_fused(x_batch, prm, D, raw=(volL, volR), workspace=workspace, want_volumes=want_volumes, **more)
        if arch == "fast":
            return stereo_predict_fused(x_batch, prm, D, feat=features_fast(x_batch, layers, conv_mode), workspace=workspace,
                                        want_volumes=want_volumes, **more)
        raw = raw_volumes_slow(features_slow(x_batch, layers, conv_mode), fc_layers, D, prm["border_n"], fc_mode=getattr(opt, "fc_mode", "fp32"))
        return stereo_predict_fused(x_batch, prm, D, raw=raw, workspace=workspace, want_volumes=want_volumes, **more)
    if opt.a in TRAIN_ACTIONS:
        if mod is None:
            from . import train as mod
        if opt.a in ("train_tr", "train_all"):   # main.lua:602-890; each train() keeps its own leading arguments
            lead = () if trainer is mod and dataset == "mb" else (dataset, arch) if arch == "fast" else (dataset,)
            opt.net_fname = trainer.train(*lead, opt, argv[2:], dev)
            if opt.a == "train_all":            # main.lua:884-887 goes on to submit, which is out of scope
                return 0
            opt.a = "test_te"
            layers[:] = device_layers(load_net(opt.net_fname, dataset, arch), dev)
            if arch == "slow":
                fc_layers[:] = load_fc(opt.net_fname, dataset)
        if dataset == "mb":
            mod.evaluate(opt, prm, run, dev)         # main.lua:1124-1130, 1183-1238
        else:
            mod.evaluate(dataset, opt, run, dev)     # main.lua:1121-1138, 1172-1293
        return 0
    if opt.a == "time":  # main.lua:1140-1167
        if dataset == "mb":
            prm["left_only"] = 1  # outside `-a predict` dataset mb runs direction -1 only (mb_directions, main.lua:953-955)
        H, W, D = (240, 320, 32) if opt.tiny else ((350, 1242, 228) if dataset != "mb" else (1000, 1500, 200))
        x_batch = torch.empty((2, 1, H, W), dtype=torch.float32, device=dev).normal_()
        ws = Workspace(prm, D, H, W, dev)
        best = float("inf")
        for _ in range(30 if arch == "fast" else 3):  # main.lua:1152
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(x_batch, D, workspace=ws)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        print(best)
        return 0
    x0, x1 = load_image(opt.left), load_image(opt.right)
    if x0.shape[0] == 3:
        assert x1.shape[0] == 3
        x0, x1 = rgb2y(x0), rgb2y(x1)
    D = opt.disp_max
    x_batch = torch.from_numpy(np.stack([normalize(x0), normalize(x1)])).to(dev)  # (2,1,H,W)
    res = run(x_batch, D, want_volumes=True, extras=opt.extras, right_view=opt.right_view, margins=opt.margins)
    torch.cuda.synchronize()
    H, W = x_batch.shape[2:]
    for name, key in (("right", "volR"), ("left", "volL")):  # main.lua:954-955 writes right.bin first
        print("Writing %s.bin, %d x %d x %d x %d" % (name, 1, D, H, W))
        write_bin("%s.bin" % name, res[key].cpu().numpy())
    print("Writing disp.bin, %d x %d x %d x %d" % (1, 1, H, W))
    write_bin("disp.bin", res["disp"].cpu().numpy())
    if opt.extras:
        for name, key in (("outlier", "outlier"), ("cost", "cost"), ("curvature", "curvature")):
            print("Writing %s.bin, %d x %d x %d x %d" % (name, 1, 1, H, W))
            write_bin("%s.bin" % name, res[key].cpu().numpy())
    if opt.right_view:
        for name in ("disp_right",) + (("outlier_right",) if opt.extras else ()):
            print("Writing %s.bin, %d x %d x %d x %d" % (name, 1, 1, H, W))
            write_bin("%s.bin" % name, res[name].cpu().numpy())
    if opt.margins:
        for name in ("c1", "c2", "c2l") + (("c1_right", "c2_right", "c2l_right") if opt.right_view else ()):
            print("Writing %s.bin, %d x %d x %d x %d" % (name, 1, 1, H, W))
            write_bin("%s.bin" % name, res[name].cpu().numpy())
    return 0


if __name__ == "__main__":
    sys.exit(main())
