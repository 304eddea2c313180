"""CPU: the host loop of `train.train` (main.lua:657, 779-875) with `train.Trainer` replaced by a recorder that has no
library: which `(t0, n_steps)` chunks it enqueues per epoch, where each chunk's losses go, the permutation, the epoch-12
learning-rate drop, the `-max_steps` budget and `train_all`'s pixel list.  And Normalize2's backward formula
(adcensus.cu:1345-1355) restated in float64 numpy against autograd of the oracle's normalisation."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_oracle as to  # noqa: E402
from mc_cnn_amd import main as mcmain  # noqa: E402

N_TR, N_TE = 21, 5      # bs 4 (2 pairs per step): `for t = 1, 21 - 2, 2` is a 10-step epoch


class Recorder:
    """Stands in for train.Trainer: stores the constructor's arguments and every run() call; a step's loss is its
    index in the whole run, so that the order of last_run["losses"] can be read back."""
    made = []

    def __init__(self, x0, x1, nnz, perm, layers, n_pairs, device):
        self.nnz, self.perm, self.n_pairs, self.device = np.array(nnz), perm, n_pairs, device
        self._layers = layers
        self.calls = []
        self.steps_done = 0
        Recorder.made.append(self)

    def run(self, t0, prm, lr, mom, margin, pow_, losses):
        k = prm.shape[0]
        self.calls.append(dict(t0=t0, n_steps=k, prm_shape=tuple(prm.shape), lr=lr, mom=mom, margin=margin, pow=pow_,
                               offset=losses.storage_offset(), room=losses.shape[0], base=losses.untyped_storage().data_ptr(),
                               perm=self.perm, prm_device=prm.device))
        for s in range(k):
            losses[s] = float(self.steps_done)
            self.steps_done += 1

    def layers(self):
        return self._layers


def _data(rng):
    nnz = lambda n, first: np.stack([rng.integers(1, 3, n), rng.integers(0, 12, n), rng.integers(0, 16, n),
                                     first + np.arange(n)], 1).astype(np.float32)
    x = rng.standard_normal((2, 1, 12, 16)).astype(np.float32)
    return dict(x0=x, x1=x[..., ::-1].copy(), nnz_tr=nnz(N_TR, 100), nnz_te=nnz(N_TE, 200))


def _train(monkeypatch, tmp_path, extra, a="train_tr"):
    import torch
    from mc_cnn_amd import train
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(train, "Trainer", Recorder)
    monkeypatch.setattr(train, "CHUNK_STEPS", 4)
    Recorder.made = []
    argv = ["-a", a, "-bs", "4", "-seed", "5"] + extra
    _, _, opt, _ = mcmain.parse(["kitti", "fast"] + argv)
    data = _data(np.random.default_rng(0))
    fname = train.train("kitti", "fast", opt, argv, torch.device("cpu"), data=data)
    assert len(Recorder.made) == 1            # one Trainer for the whole run: state and permutation persist over epochs
    return Recorder.made[0], train.last_run, opt, data, fname


def _epochs(calls):
    """run() calls grouped into epochs: a call with t0 == 0 starts one."""
    out = []
    for c in calls:
        if c["t0"] == 0:
            out.append([])
        out[-1].append(c)
    return out


def test_chunks_losses_permutation_and_the_learning_rate_drop(monkeypatch, tmp_path):
    rec, run, opt, data, fname = _train(monkeypatch, tmp_path, ["-epochs", "13", "-lr", "0.004"])
    eps = _epochs(rec.calls)
    assert len(eps) == 13 and run["epochs"] == 13
    for e, calls in enumerate(eps, 1):
        # steps s0 = 0, 4, 8 of the epoch: rows t0 = s0 * n_pairs of the permutation, 4 + 4 + 2 steps
        assert [(c["t0"], c["n_steps"]) for c in calls] == [(0, 4), (8, 4), (16, 2)], e
        for c, s0 in zip(calls, (0, 4, 8)):
            assert c["offset"] == s0 and c["room"] == 10 - s0      # losses[s0:] of the epoch's 10-step buffer
            assert c["base"] == calls[0]["base"]
            assert c["prm_shape"] == (c["n_steps"], 2, 18) and c["prm_device"].type == "cpu"
            assert c["perm"] is rec.perm
            want_lr = 0.004 if e < 12 else 0.004 / 10
            assert c["lr"] == want_lr, (e, c["lr"])
            assert (c["mom"], c["margin"], c["pow"]) == (opt.mom, opt.m, opt.pow)
    assert opt.lr == 0.004 / 10                                  # saved with the net, as main.lua leaves opt.lr
    # the permutation: of the nnz_tr rows, int32, drawn once
    perm = np.asarray(rec.perm)
    assert perm.dtype == np.int32 and sorted(perm.tolist()) == list(range(N_TR))
    assert not np.array_equal(perm, np.arange(N_TR))
    assert rec.n_pairs == 2
    np.testing.assert_array_equal(rec.nnz, data["nnz_tr"])
    # every step's loss, in order
    np.testing.assert_array_equal(run["losses"], np.arange(130, dtype=np.float32))
    assert os.path.exists(fname) and run["net_fname"] == fname


def test_max_steps_stops_inside_the_third_epoch(monkeypatch, tmp_path):
    rec, run, opt, _, _ = _train(monkeypatch, tmp_path, ["-epochs", "13", "-max_steps", "23"])
    eps = _epochs(rec.calls)
    assert [[(c["t0"], c["n_steps"]) for c in calls] for calls in eps] == [[(0, 4), (8, 4), (16, 2)]] * 2 + [[(0, 3)]]
    assert eps[2][0]["offset"] == 0
    assert run["epochs"] == 3
    np.testing.assert_array_equal(run["losses"], np.arange(23, dtype=np.float32))
    assert all(c["lr"] == opt.lr for c in rec.calls)


def test_max_steps_on_an_epoch_boundary_starts_no_empty_epoch(monkeypatch, tmp_path):
    rec, run, _, _, _ = _train(monkeypatch, tmp_path, ["-epochs", "13", "-max_steps", "20"])
    assert sum(c["n_steps"] for c in rec.calls) == 20 and run["epochs"] == 2 and len(_epochs(rec.calls)) == 2


def test_train_all_lists_the_training_rows_then_the_test_rows(monkeypatch, tmp_path):
    rec, run, _, data, _ = _train(monkeypatch, tmp_path, ["-epochs", "1"], a="train_all")
    np.testing.assert_array_equal(rec.nnz, np.concatenate([data["nnz_tr"], data["nnz_te"]], 0))
    assert sorted(np.asarray(rec.perm).tolist()) == list(range(N_TR + N_TE))
    # 26 rows: `for t = 1, 26 - 2, 2` is 12 steps
    assert [(c["t0"], c["n_steps"]) for c in rec.calls] == [(0, 4), (8, 4), (16, 4)]
    assert run["losses"].size == 12


def test_fewer_rows_than_a_batch_is_refused(monkeypatch, tmp_path):
    import torch
    from mc_cnn_amd import train
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(train, "Trainer", Recorder)
    argv = ["-a", "train_tr", "-bs", "64"]
    _, _, opt, _ = mcmain.parse(["kitti", "fast"] + argv)
    with pytest.raises(SystemExit, match="fewer than a batch"):
        train.train("kitti", "fast", opt, argv, torch.device("cpu"), data=_data(np.random.default_rng(0)))


def normalize_backward(x, grad_out):
    """Normalize2's gradient at its input, in float64: with n = sum_c x_c^2 + 1e-5 over the channels,
    dx_c = (n - x_c^2) / n^1.5 * g_c - (sum_{k != c} x_k g_k) * x_c / n^1.5."""
    n = (x * x).sum(1, keepdims=True) + 1e-5
    dot = (x * grad_out).sum(1, keepdims=True)
    return (n - x * x) / n ** 1.5 * grad_out - (dot - x * grad_out) * x / n ** 1.5


@pytest.mark.parametrize("scale", [1.0, 1e-3, 30.0])
def test_normalize_backward_formula_is_autograds(scale):
    import torch
    rng = np.random.default_rng(3)
    x = rng.standard_normal((24, 64, 1, 1)) * scale
    x[3] = 0                                                    # the all-zero feature vector of a dead net
    g = rng.standard_normal(x.shape)
    xt = torch.tensor(x, requires_grad=True)
    hn, _, _ = to.tail_parts(xt, 0.2, 1)
    hn.backward(torch.tensor(g))
    want = xt.grad.numpy()
    got = normalize_backward(x, g)
    assert np.abs(got - want).max() <= 1e-12
    np.testing.assert_allclose(got[3], g[3] / np.sqrt(1e-5), rtol=1e-14, atol=0)   # at 0 the Jacobian is 1 / sqrt(eps)
