"""CPU, no library: the order in which the four `train()` functions draw from their ONE `numpy.random.Generator(-seed)`.
The permutation comes first; then, chunk by chunk and epoch by epoch, the chunk's augmentation parameters (`draw_params`)
and, on Middlebury, the chunk's sources (`draw_sources`) after them.  A run for a given -seed is bitwise what it is because
of that order, so every array handed to the Trainer is compared with what this test draws itself in that order."""
import numpy as np
import pytest

from mc_cnn_amd import train, train_mb, train_mb_slow, train_slow

N_TR, N_TE = 21, 5      # bs 4 (2 pairs per step): `for t = 1, 21 - 2, 2` is a 10-step epoch
CHUNKS = ((0, 4), (4, 4), (8, 2))    # (first step, steps) of the chunks of an epoch with CHUNK_STEPS 4
INDEX = np.array([[0, 2, 2], [8, 1, 1], [10, 3, 3], [28, 2, 1], [32, 1, 2]], np.int64)   # (first plane, lights, exposures) of 5 images


def recorder(mb):
    class Recorder:
        """Stands in for a module's Trainer: keeps the permutation it is given and every prm (and src) passed to run()."""
        made = []

        def __init__(self, store0, store1, nnz, perm, *net_and_rest):
            self.perm, self.net, self.prm, self.src = np.array(perm), net_and_rest[:-2], [], []
            Recorder.made.append(self)

        def run(self, t0, *args):
            if mb:
                self.src.append(args[0].numpy().copy())
            self.prm.append(args[1 if mb else 0].numpy().copy())
            args[-1][:args[1 if mb else 0].shape[0]] = 0.5

        def layers(self):
            return self.net[0]

        def nets(self):
            return self.net
    return Recorder


def nnz_rows(rng, n, first, n_img):
    return np.stack([rng.integers(1, n_img + 1, n), rng.integers(0, 8, n), rng.integers(0, 10, n), first + np.arange(n)], 1).astype(np.float32)


@pytest.mark.parametrize("mod", [train, train_slow, train_mb, train_mb_slow], ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_one_generator_draws_the_permutation_then_each_chunks_parameters_then_its_sources(mod, monkeypatch, tmp_path):
    import torch
    from mc_cnn_amd import main as mcmain
    mb = mod in (train_mb, train_mb_slow)
    Recorder = recorder(mb)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(mod, "Trainer", Recorder)
    monkeypatch.setattr(mod, "CHUNK_STEPS", 4)
    rng = np.random.default_rng(0)
    data = dict(nnz_tr=nnz_rows(rng, N_TR, 100, 5 if mb else 2), nnz_te=nnz_rows(rng, N_TE, 200, 5 if mb else 2))
    argv = ["-a", "train_tr", "-bs", "4", "-seed", "5", "-epochs", "2"]
    dev = torch.device("cpu")
    if mb:
        data.update(planes=np.zeros(16, np.float32), table=np.zeros(36, train_mb.PLANE_DTYPE), index=INDEX)
        opt = mod.parse(["mb", "slow" if mod is train_mb_slow else "fast"] + argv)[2]
        mod.train(opt, argv, dev, data=data)
    else:
        x = rng.standard_normal((2, 1, 12, 16)).astype(np.float32)
        data.update(x0=x, x1=x[..., ::-1].copy())
        if mod is train:
            opt = mcmain.parse(["kitti", "fast"] + argv)[2]
            mod.train("kitti", "fast", opt, argv, dev, data=data)
        else:
            opt = mod.parse(["kitti", "slow"] + argv)[2]
            mod.train("kitti", opt, argv, dev, data=data)
    rec, = Recorder.made
    assert mod.last_run["epochs"] == 2 and mod.last_run["losses"].size == 20

    want = np.random.default_rng(5)
    perm = want.permutation(N_TR)
    np.testing.assert_array_equal(rec.perm, perm)
    assert len(rec.prm) == 2 * len(CHUNKS) and len(rec.src) == (2 * len(CHUNKS) if mb else 0)
    call = 0
    for epoch in range(2):
        for s0, k in CHUNKS:
            np.testing.assert_array_equal(rec.prm[call], train.draw_params(want, opt, k, 2), err_msg="prm of epoch %d, step %d" % (epoch, s0))
            if mb:
                ids = data["nnz_tr"][perm[2 * s0:2 * (s0 + k)], 0].astype(np.int64).reshape(k, 2)
                np.testing.assert_array_equal(rec.src[call], train_mb.draw_sources(want, opt, ids, INDEX),
                                              err_msg="src of epoch %d, step %d" % (epoch, s0))
            call += 1
