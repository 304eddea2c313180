"""A test set resident on the device, scored for one set of stereo-method parameters after another: what hs.py's `test_te`
search pays a fresh `main.lua` process (and, for arch slow, a disk cache of volumes, main.lua:959-982) per candidate for.

`EvalSet(dataset, arch, opt, layers, fc_layers, device, cache_bytes)` takes the examples and the ground truth of `-a test_te`
from the loaders `train.evaluate` / `train_mb.evaluate` read (same example lists, same err_at; `data=` hands it what they return
instead, as both `evaluate`s allow), uploads every pair and its
ground truth once, and computes each example's COST STAGE -- what does not depend on the parameters searched -- once:

  arch fast       the features after `main.features_fast`        2 * fm * H * W floats
  arch slow       the raw volumes after `main.raw_volumes_slow`   2 * D * H * W floats
  ad / census     the two volumes as `main.run` builds them       2 * D * H * W floats

`mc_predict` documents its inputs as not modified, so they serve every candidate.  cache_bytes (-cache_gb) bounds what is kept:
examples are cached in list order while they fit, the rest recompute their cost stage per candidate.

`score(prm, in_flight=K)` deals the examples round-robin over K streams, each with its own `predict.Workspace` and output map;
per example one `stereo_predict_fused` and one `mc_eval_error` (libmceval.so) into row i of an (n, 3) int32 tensor, on the same
stream, with no host synchronisation and no read-back until every example is queued; then one synchronise and one copy of the
counts.  The mean is `train.evaluate`'s arithmetic on the same integers -- sum(bad_i / valid_i) / n in Python floats, in list order
-- so a score equals, bit for bit, the last line `main.py ... -a test_te` prints for the same parameters.

Blur-only reuse: blur_sigma and blur_t act after the median (main.lua:1072-1079).  With `reuse` on, a candidate runs `mc_predict`
with sm_terminate = 'median' into a per-example map that is kept (n x H x W floats) together with the candidate's UPSTREAM parameter
tuple -- everything but the two blur parameters -- and the blur is `adcensus.mean2d` on `adcensus.gaussian` (mc_gaussian_host): the
launcher and the table `mc_predict` itself uses, hence the same bits.  A candidate whose upstream tuple equals the held one runs only
blur + error count.  `n_predict_calls` counts the `mc_predict` launches.
"""
import numpy as np

from . import _eval_lib as ev
from .params import TABLES

BLUR_KEYS = ("blur_sigma", "blur_t")


def eval_error(pred, pred_ld, actual, actual_ld, H, W, err_at, counts):
    """mc_eval_error on torch's current stream: pred / actual device float32 tensors (any shape, read as H rows of W floats with
    the given row strides), counts a device int32 tensor of 3 (added to)."""
    import torch
    ev.check(ev.load().mc_eval_error(pred.data_ptr(), int(pred_ld), actual.data_ptr(), int(actual_ld), int(H), int(W), float(err_at),
                                     counts.data_ptr(), torch.cuda.current_stream().cuda_stream), "mc_eval_error")


class _Lane:
    """What one stream owns: its workspaces (one per (D, H, W)) and output maps (one per (H, W))."""

    def __init__(self, stream):
        self.stream, self.ws, self.out = stream, {}, {}


class EvalSet:
    def __init__(self, dataset, arch, opt, layers, fc_layers, device, cache_bytes=48 << 30, reuse=True, data=None):
        import torch
        from .main import device_layers
        if (dataset, arch) not in TABLES:
            raise ValueError("EvalSet: no parameter table for %s %s" % (dataset, arch))
        self.dataset, self.arch, self.dev, self.reuse = dataset, arch, device, reuse
        self.learned = arch in ("fast", "slow")
        self.layers = device_layers(layers, device) if self.learned else []
        self.fc_layers = fc_layers if arch == "slow" else None
        self.fc_mode = getattr(opt, "fc_mode", "fp32")        # arch slow's cost stage: main.raw_volumes_slow's fc_mode
        self.conv_mode = getattr(opt, "conv_mode", "fp32")    # either net's cost stage: main.features_fast / features_slow's conv_mode
        if self.conv_mode != "fp32" and arch not in ("fast", "slow"):
            raise ValueError("EvalSet: conv_mode %s for arch %s: it has no net" % (self.conv_mode, arch))
        if self.fc_mode != "fp32" and arch != "slow":
            raise ValueError("EvalSet: fc_mode %s for arch %s: only arch slow has an FC stack" % (self.fc_mode, arch))
        self.border_n = len(self.layers)                      # main.lua:382-391, 923, as main.main sets it
        self.prm = dict(TABLES[(dataset, arch)], border_n=self.border_n)   # the defaults a search starts from
        if dataset == "mb":
            self.prm["left_only"] = 1                         # outside -a predict mb runs direction -1 only (main.lua:953-955)
        self.err_at = 1 if dataset == "mb" else 3
        self.examples = self._load_mb(opt, data) if dataset == "mb" else self._load_kitti(opt, data)
        self.n = len(self.examples)
        self.n_predict_calls = 0
        self._lanes, self._gauss = [], {}
        self._held, self._held_key = None, None
        # the cost stage, once: in list order while it fits cache_bytes
        self.n_cached, self.resident_bytes = 0, 0
        for e in self.examples:
            need = 4 * 2 * (self.layers[-1][0].shape[0] if arch == "fast" else e["D"]) * e["H"] * e["W"]
            if self.resident_bytes + need > cache_bytes:
                break
            e["stage"] = self._cost_stage(e)
            self.resident_bytes += need
            self.n_cached += 1
        torch.cuda.synchronize(device)
        print("evalset: %s %s, %d examples, cost stage of %d resident (%.3f GB of %.3f GB allowed)%s"
              % (dataset, arch, self.n, self.n_cached, self.resident_bytes / 1e9, cache_bytes / 1e9,
                 "" if self.n_cached == self.n else "; the other %d recompute theirs per candidate" % (self.n - self.n_cached)))

    # ---- the examples ----------------------------------------------------------------------------------------------------------
    def _example(self, x_pair, actual, D, H, W):
        import torch
        xb = torch.from_numpy(np.ascontiguousarray(x_pair, np.float32)).to(self.dev)
        gt = torch.from_numpy(np.ascontiguousarray(actual, np.float32)).to(self.dev)
        return dict(xb=xb, gt=gt, gt_ld=actual.shape[-1], D=int(D), H=int(H), W=int(W), stage=None)

    def _load_kitti(self, opt, data=None):
        """train.evaluate's examples: image i of test_examples cropped to its own width w; the ground truth stays 1242 wide on the
        device and is read w wide (mc_eval_error's actual_ld)."""
        from . import train
        if data is None:
            data = train.load_data(self.dataset, opt, ("x0", "x1", "metadata", "tr", "te", "dispnoc"))
        x0, x1, meta, dispnoc = data["x0"], data["x1"], np.asarray(data["metadata"]), data["dispnoc"]
        H, W = x0.shape[-2], x0.shape[-1]
        out = []
        for i in train.test_examples(opt, data):
            w = int(meta[i - 1, 1])
            pair = np.stack([x0[i - 1].reshape(1, H, W)[..., :w], x1[i - 1].reshape(1, H, W)[..., :w]])
            out.append(self._example(pair, np.asarray(dispnoc[i - 1], np.float32).reshape(H, W), opt.disp_max, H, w))
        return out

    def _load_mb(self, opt, data=None):
        """train_mb.evaluate's examples: (te[i], 2) for every te, then (5, 3) and (5, 4), each with its image's own disp_max."""
        from . import train_mb
        if data is None:
            data = train_mb.load_mb_data(train_mb.data_dir_of(opt), "test_te")
        out = []
        for i, right in train_mb.test_examples(data["te"]):
            if not 1 <= i <= len(data["X"]) or not data["X"][i - 1] or np.asarray(data["X"][i - 1][0]).ndim != 4:
                raise SystemExit("test_te: image %d has no test views (x_%d_1.bin is missing or empty)" % (i, i))
            x = np.asarray(data["X"][i - 1][0], np.float32)
            if right > x.shape[0]:
                raise SystemExit("test_te: image %d has %d test views, view %d is asked for" % (i, x.shape[0], right))
            if i not in data["dispnoc"]:
                raise SystemExit("test_te: image %d has no dispnoc%d.bin" % (i, i))
            D = int(data["meta"][i - 1, 2])
            if D <= 0:
                raise SystemExit("test_te: meta.bin gives image %d a disp_max of %d" % (i, D))
            H, W = x.shape[-2:]
            out.append(self._example(np.stack([x[0], x[right - 1]]).reshape(2, 1, H, W),
                                     np.asarray(data["dispnoc"][i], np.float32).reshape(H, W), D, H, W))
        return out

    # ---- the cost stage ----------------------------------------------------------------------------------------------------------
    def _cost_stage(self, e):
        """The keyword of stereo_predict_fused that carries the example's cost stage, computed as main.run does, on torch's
        current stream."""
        import torch
        from . import adcensus, main
        xb, D = e["xb"], e["D"]
        if self.arch == "fast":
            return dict(feat=main.features_fast(xb, self.layers, self.conv_mode))
        if self.arch == "slow":
            return dict(raw=main.raw_volumes_slow(main.features_slow(xb, self.layers, self.conv_mode), self.fc_layers, D, self.border_n, fc_mode=self.fc_mode))
        cost = adcensus.ad if self.arch == "ad" else adcensus.census   # main.lua:932-942
        volL = torch.empty((1, D, e["H"], e["W"]), dtype=torch.float32, device=self.dev)
        volR = torch.empty_like(volL)
        adcensus.fill_nan(volL)
        adcensus.fill_nan(volR)
        cost(xb[0:1], xb[1:2], volL, -1)
        cost(xb[1:2], xb[0:1], volR, 1)
        return dict(raw=(volL, volR))

    # ---- a candidate ---------------------------------------------------------------------------------------------------------------
    def _workspace(self, lane, p, e):
        """The lane's workspace for the example's shape: re-created only when this candidate needs more than is held (L1 and the
        CBCA iteration counts change the plan area)."""
        from .predict import Workspace, workspace_bytes
        key = (e["D"], e["H"], e["W"])
        ws = lane.ws.get(key)
        if ws is None or ws.nbytes < workspace_bytes(p, *key):
            lane.ws[key] = None                 # release the smaller one before taking the next
            ws = lane.ws[key] = Workspace(p, e["D"], e["H"], e["W"], self.dev)
        return ws

    def _gaussian(self, sigma):
        from . import adcensus
        k = self._gauss.get(sigma)
        if k is None:
            k = self._gauss[sigma] = adcensus.gaussian(sigma).to(self.dev)
        return k

    def score(self, prm, in_flight=2):
        """The mean test error of the parameter table prm (a dict as params.TABLES holds; border_n and, on mb, left_only are this
        set's own)."""
        import torch
        from . import adcensus
        from .params import make_params
        from .predict import stereo_predict_fused
        if in_flight < 1:
            raise ValueError("EvalSet.score: in_flight %d" % in_flight)
        prm = dict(prm, border_n=self.border_n)
        if self.dataset == "mb":
            prm["left_only"] = 1
        plain = not prm.get("sm_terminate") and not prm.get("sm_skip")
        reuse = self.reuse and plain            # a candidate with stage switches of its own takes the whole pipeline as it is
        upstream = tuple(sorted((k, v) for k, v in prm.items() if k not in BLUR_KEYS))
        p = make_params(dict(prm, sm_terminate="median") if reuse else prm)
        run_predict = not (reuse and self._held is not None and self._held_key == upstream)
        if reuse and self._held is None:
            self._held = [torch.empty((1, 1, e["H"], e["W"]), dtype=torch.float32, device=self.dev) for e in self.examples]
        if reuse and run_predict:
            self._held_key = None               # until every map of this candidate is queued
        gk = self._gaussian(prm["blur_sigma"]) if reuse else None
        while len(self._lanes) < in_flight:
            self._lanes.append(_Lane(torch.cuda.Stream(self.dev)))
        counts = torch.zeros((self.n, 3), dtype=torch.int32, device=self.dev)
        here = torch.cuda.current_stream(self.dev)
        for lane in self._lanes[:in_flight]:
            lane.stream.wait_stream(here)
        for i, e in enumerate(self.examples):
            lane = self._lanes[i % in_flight]
            H, W = e["H"], e["W"]
            with torch.cuda.stream(lane.stream):
                if reuse:
                    med = self._held[i]
                    if run_predict:
                        stage = e["stage"] if e["stage"] is not None else self._cost_stage(e)
                        stereo_predict_fused(e["xb"], p, e["D"], workspace=self._workspace(lane, p, e), out=med, **stage)
                        self.n_predict_calls += 1
                    pred = adcensus.mean2d(med, gk, prm["blur_t"])
                else:
                    pred = lane.out.get((H, W))
                    if pred is None:
                        pred = lane.out[(H, W)] = torch.empty((1, 1, H, W), dtype=torch.float32, device=self.dev)
                    stage = e["stage"] if e["stage"] is not None else self._cost_stage(e)
                    stereo_predict_fused(e["xb"], p, e["D"], workspace=self._workspace(lane, p, e), out=pred, **stage)
                    self.n_predict_calls += 1
                eval_error(pred, W, e["gt"], e["gt_ld"], H, W, self.err_at, counts[i])
                del pred
        if reuse and run_predict:
            self._held_key = upstream
        torch.cuda.synchronize(self.dev)        # the one synchronisation of a candidate
        c = counts.cpu().numpy()                 # ... and its one read-back
        if (c[:, 2] != 0).any():                 # main.lua's assert(not isnan(pred:sum()))
            i = int(np.nonzero(c[:, 2])[0][0])
            raise FloatingPointError("EvalSet.score: %d NaN pixels in the prediction of example %d" % (int(c[i, 2]), i))
        return sum(float(c[i, 1]) / float(c[i, 0]) for i in range(self.n)) / self.n
