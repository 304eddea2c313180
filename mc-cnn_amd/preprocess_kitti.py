"""`preprocess_kitti.lua` on the MI355X: the KITTI 2012 / 2015 archives -> the training sets of `-a train_tr`.

    cd DIR_WITH_data.kitti_AND_data.kitti2015
    python -m mc_cnn_amd.preprocess_kitti            # both sets, 2012 first, as the reference
    python -m mc_cnn_amd.preprocess_kitti 2015       # one set only

reads `data.kitti/unzip/{training,testing}/{image_0,image_1}/%06d_10.png` and `training/disp_noc/` (2012, 8-bit grey) and
`data.kitti2015/unzip/.../{image_2,image_3}/` and `training/disp_noc_0/` (2015, RGB converted with `rgb2y`), and writes
`x0 x1 dispnoc metadata tr te nnz_tr nnz_te` (`.bin` with `.dim` / `.type` sidecars, binio.tofile) into `data.kitti/`
and `data.kitti2015/`, line for line as preprocess_kitti.lua does:

- every image is cropped to its bottom 350 rows, normalised (mean, then the unbiased std: `main.normalize`, the same
  conversion as `-a predict`) and copied into x0 / x1 (n_tr + n_te, 1, 350, 1242) with zeros right of its width;
- metadata[k] = (height, width, id) as int32; dispnoc (n_tr, 1, 350, 1242) is the unfiltered readPNG16 ground truth,
  cropped the same way;
- `torch.manualSeed(42)` before each set, then `perm = torch.randperm(n_tr)`, te = perm[1..40], tr = perm[41..] (int64,
  1-based): restated here by `MT19937` and `randperm` (no torch7 to check against: unpinned);
- for i = 1..n_tr, a copy of dispnoc[i] is filtered (remove_nonvisible, remove_occluded, remove_white with x0[i]) and its
  pixels with d > 0.5 are appended as (i, row, col, d) to nnz_te if i is in te, else to nnz_tr (make_dataset2).

The filters and the pixel lists run on the GPU (libmctrain.so: mc_train_filter_gt, mc_train_nnz_count / _fill) behind one
function, `gpu_stages`; decoding, normalisation and writing stay on the host.  Unlike the reference, the eight files are
overwritten and nothing else is deleted, and a missing file, an image shorter than 350 rows or wider than 1242 columns, or
a ground-truth map whose size differs from its image stops the run with a message naming the file.
"""
import os
import sys
import time

import numpy as np

from .binio import read_png16, tofile
from .main import load_image, normalize, rgb2y

HEIGHT, WIDTH = 350, 1242          # preprocess_kitti.lua:31-32
N_VAL = 40                         # te = perm[1..40]
SEED = 42
SETS = {   # preprocess_kitti.lua:12-28
    2012: dict(n_tr=194, n_te=195, path="data.kitti", image_0="image_0", image_1="image_1", disp_noc="disp_noc", nchannel=1),
    2015: dict(n_tr=200, n_te=200, path="data.kitti2015", image_0="image_2", image_1="image_3", disp_noc="disp_noc_0",
               nchannel=3),
}
OUTPUTS = ("x0", "x1", "dispnoc", "metadata", "tr", "te", "nnz_tr", "nnz_te")

last_timing = {}   # year -> seconds of the latest run's stages: host "decode" / "normalize" / "write", GPU stages' keys


class MT19937:
    """torch7's generator (THRandom.c): MT19937, seeded by init_genrand as torch.manualSeed does."""
    N, M = 624, 397

    def __init__(self, seed=5489):
        mt = [seed & 0xffffffff]
        for j in range(1, self.N):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + j) & 0xffffffff)
        self.mt, self.i = mt, self.N

    def _twist(self):
        mt, n = self.mt, self.N
        for k in range(n):
            y = (mt[k] & 0x80000000) | (mt[(k + 1) % n] & 0x7fffffff)
            mt[k] = mt[(k + self.M) % n] ^ (y >> 1) ^ (0x9908b0df if y & 1 else 0)
        self.i = 0

    def genrand_int32(self):
        if self.i >= self.N:
            self._twist()
        y = self.mt[self.i]
        self.i += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        return y ^ (y >> 18)


def randperm(n, gen):
    """torch.randperm(n) of torch7 (THTensorMath.c): swap r[i] with r[i + random() % (n - i)] for i < n - 1, then + 1."""
    r = list(range(n))
    for i in range(n - 1):
        z = gen.genrand_int32() % (n - i)
        r[i], r[i + z] = r[i + z], r[i]
    return np.array(r, np.int64) + 1


def split(n_tr, n_val=N_VAL, seed=SEED):
    """torch.manualSeed(seed); perm = torch.randperm(n_tr):long(); te = perm[1..n_val], tr = perm[n_val+1..] (1-based)."""
    perm = randperm(n_tr, MT19937(seed))
    return perm[n_val:].copy(), perm[:n_val].copy()


def _fail(path, what):
    raise SystemExit("preprocess_kitti: %s: %s" % (path, what))


def _load(path, nchannel):
    """image.loadPNG(path, nchannel, 'byte'):float(), then rgb2y for the RGB set: (1, h, w) float32."""
    if not os.path.isfile(path):
        _fail(path, "no such file")
    img = load_image(path)
    if img.shape[0] != nchannel:
        _fail(path, "%d channels, the set's images are %s" % (img.shape[0], "8-bit grey" if nchannel == 1 else "RGB"))
    return rgb2y(img) if nchannel == 3 else img


def pixel_list(maps, ids):
    """make_dataset2 on the GPU for the device maps (k, H, W) with image ids (k,): (n, 4) float32 device rows."""
    import torch
    from . import _train_lib as tl
    lib = tl.load()
    k, H, W = maps.shape
    dev, st = maps.device, torch.cuda.current_stream(maps.device).cuda_stream
    maps = maps.contiguous()
    ids = torch.as_tensor(np.asarray(ids, np.int32)).to(dev)
    ws = torch.empty(lib.mc_train_nnz_workspace_bytes(k, H) // 8 + 1, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    tl.check(lib.mc_train_nnz_count(maps.data_ptr(), k, H, W, count.data_ptr(), ws.data_ptr(), ws.numel() * 8, st),
             "mc_train_nnz_count")
    n = int(count.item())
    out = torch.empty((n, 4), dtype=torch.float32, device=dev)
    tl.check(lib.mc_train_nnz_fill(maps.data_ptr(), ids.data_ptr(), k, H, W, out.data_ptr(), n, ws.data_ptr(), ws.numel() * 8, st),
             "mc_train_nnz_fill")
    return out


def filter_gt(disp, x0):
    """remove_nonvisible, remove_occluded, remove_white (preprocess_kitti.lua:99-101) in place on device maps (n, H, W)
    with their device images x0 (n, H, W)."""
    import torch
    from . import _train_lib as tl
    n, H, W = disp.shape
    assert disp.is_contiguous() and x0.is_contiguous() and tuple(x0.shape) == (n, H, W)
    tl.check(tl.load().mc_train_filter_gt(disp.data_ptr(), x0.data_ptr(), n, H, W, torch.cuda.current_stream(disp.device).cuda_stream),
             "mc_train_filter_gt")
    return disp


def gpu_stages(dispnoc, x0, te):
    """preprocess_kitti.lua:97-113 on the GPU: filter a copy of every dispnoc[i] with x0[i] and list its pixels into
    nnz_te (i in te) or nnz_tr.  dispnoc (n_tr, 1, H, W) and x0 (>= n_tr, 1, H, W) float32; te 1-based.  Returns
    (nnz_tr, nnz_te) float32 (n, 4) and the stages' device-event times in seconds."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    n, _, H, W = dispnoc.shape
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    disp = torch.from_numpy(np.ascontiguousarray(dispnoc, np.float32).reshape(n, H, W)).to(dev)
    x = torch.from_numpy(np.ascontiguousarray(x0[:n], np.float32).reshape(n, H, W)).to(dev)
    ev[1].record()
    filter_gt(disp, x)
    ev[2].record()
    is_te = np.isin(np.arange(1, n + 1), np.asarray(te))
    lists = []
    for sel in (~is_te, is_te):
        idx = np.nonzero(sel)[0]
        lists.append(pixel_list(disp[torch.from_numpy(idx).to(dev)], idx + 1).cpu().numpy())
    ev[3].record()
    ev[3].synchronize()
    times = {"gpu_upload": ev[0].elapsed_time(ev[1]) / 1e3, "gpu_filter": ev[1].elapsed_time(ev[2]) / 1e3,
             "gpu_lists": ev[2].elapsed_time(ev[3]) / 1e3}
    return lists[0], lists[1], times


def preprocess_set(year, n_tr, n_te, n_val=N_VAL, root=".", stages=None):
    """One set of preprocess_kitti.lua (its loop body, lines 9-134) under `root`; returns {name: array} as written.
    `stages(dispnoc, x0, te) -> (nnz_tr, nnz_te, times)` replaces `gpu_stages`."""
    s = SETS[year]
    if not 0 <= n_val <= n_tr:
        raise ValueError("preprocess_kitti: %d validation images out of %d" % (n_val, n_tr))
    path = os.path.join(root, s["path"])
    print("dataset %d" % year)
    n = n_tr + n_te
    x0 = np.zeros((n, 1, HEIGHT, WIDTH), np.float32)
    x1 = np.zeros_like(x0)
    dispnoc = np.zeros((n_tr, 1, HEIGHT, WIDTH), np.float32)
    metadata = np.zeros((n, 3), np.int32)
    examples = [("training", i) for i in range(1, n_tr + 1)] + [("testing", i) for i in range(1, n_te + 1)]
    t = {"decode": 0.0, "normalize": 0.0, "write": 0.0}
    for k, (d, cnt) in enumerate(examples):
        name = "%06d_10.png" % (cnt - 1)
        t0 = time.perf_counter()
        p0, p1 = (os.path.join(path, "unzip", d, s[im], name) for im in ("image_0", "image_1"))
        img_0, img_1 = _load(p0, s["nchannel"]), _load(p1, s["nchannel"])
        h, w = img_0.shape[1:]
        if h < HEIGHT or w > WIDTH:
            _fail(p0, "%d x %d: the set needs at least %d rows and at most %d columns" % (h, w, HEIGHT, WIDTH))
        if img_1.shape != img_0.shape:
            _fail(p1, "%d x %d, its left image %s is %d x %d" % (img_1.shape[1], img_1.shape[2], p0, h, w))
        gt = None
        if d == "training":
            pd = os.path.join(path, "unzip", "training", s["disp_noc"], name)
            if not os.path.isfile(pd):
                _fail(pd, "no such file")
            gt = read_png16(pd)
            if gt.shape != (h, w):
                _fail(pd, "ground truth of %d x %d, its image %s is %d x %d" % (gt.shape + (p0, h, w)))
        t1 = time.perf_counter()
        print(k + 1)
        x0[k, :, :, :w] = normalize(img_0[:, h - HEIGHT:])
        x1[k, :, :, :w] = normalize(img_1[:, h - HEIGHT:])
        if gt is not None:
            dispnoc[k, 0, :, :w] = gt[h - HEIGHT:]
        metadata[k] = (h, w, cnt - 1)
        t2 = time.perf_counter()
        t["decode"] += t1 - t0
        t["normalize"] += t2 - t1
    tr, te = split(n_tr, n_val)
    nnz_tr, nnz_te, t_gpu = (stages or gpu_stages)(dispnoc, x0, te)
    out = dict(x0=x0, x1=x1, dispnoc=dispnoc, metadata=metadata, tr=tr, te=te,
               nnz_tr=np.asarray(nnz_tr, np.float32).reshape(-1, 4), nnz_te=np.asarray(nnz_te, np.float32).reshape(-1, 4))
    t0 = time.perf_counter()
    os.makedirs(path, exist_ok=True)
    for key in OUTPUTS:
        tofile(os.path.join(path, key + ".bin"), out[key])
    t["write"] = time.perf_counter() - t0
    t.update(t_gpu)
    last_timing[year] = t
    return out


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if any(a not in ("2012", "2015") for a in argv):
        raise SystemExit("usage: python -m mc_cnn_amd.preprocess_kitti [2012] [2015]  (default: both, 2012 first; run from the "
                         "directory that holds data.kitti/unzip and data.kitti2015/unzip)")
    years = [y for y in (2012, 2015) if not argv or str(y) in argv]
    for y in years:
        preprocess_set(y, SETS[y]["n_tr"], SETS[y]["n_te"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
