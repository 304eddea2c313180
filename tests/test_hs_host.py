"""CPU: the host side of the parameter search (mc_cnn_amd/hs.py): the grid table, the valid rule, log lines, snapping, each
method's neighbour rule on a toy grid with a stub scorer, seeding, the start from defaults, the refusals; and libmceval.so's
symbols and host refusals (include/mc_eval.h), which need no GPU because every argument check runs before the launch."""
import ctypes as C
import itertools
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import libraries as L  # noqa: E402
from mc_cnn_amd import _eval_lib as ev  # noqa: E402
from mc_cnn_amd import hs  # noqa: E402
from mc_cnn_amd.params import TABLES, McParams  # noqa: E402


# ---- grids ---------------------------------------------------------------------------------------------------------------------
def test_every_grid_name_is_an_mc_params_field_and_every_pair_has_a_grid():
    fields = {k for k, _ in McParams._fields_}
    for dataset, arch in itertools.product(hs.DATASETS, hs.ARCHS):
        grid = hs.grid_of(dataset, arch, "test_te")
        names = [k for k, _ in grid]
        assert len(set(names)) == len(names)
        assert set(names) <= fields and set(names) <= set(TABLES[(dataset, arch)])
        assert all(len(v) >= 2 and list(v) == sorted(v) for _, v in grid)
        has_cbca = dataset != "mb" and arch != "fast"
        assert ({"L1", "tau1", "cbca_i1", "cbca_i2"} <= set(names)) == has_cbca
        assert {"pi1", "pi2", "sgm_q1", "sgm_q2", "alpha1", "tau_so", "blur_sigma", "blur_t"} <= set(names)
    assert set(hs.GRIDS) == set(TABLES)
    assert dict(hs.grid_of("kitti", "fast"))["pi2"][-1] == 128.0 and dict(hs.grid_of("mb", "fast"))["pi2"][-1] == 32.0
    assert dict(hs.grid_of("kitti", "slow"))["blur_t"] == [1, 2, 3, 4, 5, 6, 7] and dict(hs.grid_of("mb", "slow"))["blur_t"] == [1, 2, 3, 4, 5]


def test_valid_rule():
    assert hs.valid(dict(pi1=1.0, pi2=8.0)) and hs.valid(dict(pi1=4.0, pi2=4.0)) and not hs.valid(dict(pi1=4.0, pi2=3.5))


# ---- log lines -------------------------------------------------------------------------------------------------------------------
def test_log_line_round_trip():
    grid = hs.grid_of("kitti", "fast")
    ps = [(name, values[(3 * i) % len(values)]) for i, (name, values) in enumerate(grid)]
    score = 0.1 + 0.2   # needs all 17 digits
    line = hs.format_line(score, "kitti", "fast", "test_te", ps, "net/net_x.t7")
    assert line.startswith("0.30000000000000004 kitti fast test_te -pi1 0.25 -pi2 18.38 -sgm_q1 ") and line.endswith(" -net_fname net/net_x.t7")
    got = hs.parse_line(line + "\n", "kitti", "fast", "test_te", grid)
    assert got == (score, {k: float(v) for k, v in ps})
    assert hs.parse_line(line, "kitti2015", "fast", "test_te", grid) is None     # another dataset's
    assert hs.parse_line(line, "kitti", "slow", "test_te", hs.grid_of("kitti", "slow")) is None
    assert hs.parse_line("Traceback (most recent call last):", "kitti", "fast", "test_te", grid) is None
    assert hs.parse_line("", "kitti", "fast", "test_te", grid) is None


def test_a_line_in_the_references_format_parses():
    # what the reference's print(new_score, dataset, arch, action, ps_str) writes for kitti slow, with its -use_cache
    line = ("0.02613 kitti slow test_te -L1 5 -cbca_i1 2 -cbca_i2 0 -tau1 0.13 -pi1 1.32 -pi2 24.25 -sgm_q1 3 -sgm_q2 2 -alpha1 2.0 "
            "-tau_so 0.08 -blur_sigma 5.99 -blur_t 6 -use_cache")
    score, ps = hs.parse_line(line, "kitti", "slow", "test_te", hs.grid_of("kitti", "slow"))
    assert score == 0.02613 and ps["L1"] == 5 and ps["pi2"] == 24.25 and ps["blur_t"] == 6 and len(ps) == 12
    t = TABLES[("kitti", "slow")]
    assert all(ps[k] == t[k] for k in ps)     # it is main.lua's own table
    assert hs.snap(ps, hs.grid_of("kitti", "slow")) == [5, 1, 0, 5, 6, 4, 0, 0, 4, 4, 7, 5]


def test_read_results_takes_hs_sh_files_and_the_log(tmp_path):
    grid = hs.grid_of("mb", "fast")
    ps = [(name, values[0]) for name, values in grid]
    (tmp_path / "hs.sh.o1").write_text(hs.format_line(0.5, "mb", "fast", "test_te", ps, "n") + "\nnoise\n"
                                       + hs.format_line(0.4, "mb", "slow", "test_te", ps, "n") + "\n")
    (tmp_path / "other.txt").write_text(hs.format_line(0.1, "mb", "fast", "test_te", ps, "n") + "\n")
    (tmp_path / "mine.log").write_text(hs.format_line(0.3, "mb", "fast", "test_te", ps, "n") + "\n")
    got = hs.read_results("mb", "fast", "test_te", grid, str(tmp_path), (str(tmp_path / "mine.log"), str(tmp_path / "absent.log"), ""))
    assert [s for s, _ in got] == [0.5, 0.3]
    # a log that is itself named hs.sh.* is read once
    got = hs.read_results("mb", "fast", "test_te", grid, str(tmp_path), (str(tmp_path / "hs.sh.o1"),))
    assert [s for s, _ in got] == [0.5]


# ---- candidates ------------------------------------------------------------------------------------------------------------------
def test_nearest_index_snapping():
    v = [0.25, 0.33, 0.44, 0.57]
    assert [hs.nearest_index(x, v) for x in (-1, 0.25, 0.28, 0.30, 0.43, 0.57, 99)] == [0, 0, 0, 1, 2, 3, 3]
    assert hs.nearest_index(2.5, [1, 2, 3, 4]) == 1       # a tie goes to the lower index, as min() of (distance, index) does
    # every default table snaps somewhere, and a grid point snaps to itself
    for key, grid in hs.GRIDS.items():
        x = hs.snap(TABLES[key], grid)
        assert all(0 <= j < len(values) for j, (_, values) in zip(x, grid))
        for name, values in grid:
            assert [hs.nearest_index(val, values) for val in values] == list(range(len(values)))


TOY = [("pi1", [1.0, 2.0, 3.0]), ("pi2", [2.0, 3.0, 4.0, 5.0]), ("blur_t", [1, 2])]


class Stub:
    """Stands in for EvalSet: the defaults and a deterministic score."""

    def __init__(self):
        self.prm = dict(TABLES[("kitti", "fast")], pi1=2.0, pi2=4.1, blur_t=2)
        self.seen = []

    def score(self, prm):
        self.seen.append(prm)
        return abs(prm["pi1"] - 3.0) + abs(prm["pi2"] - 3.0) + 0.1 * prm["blur_t"]


@pytest.mark.parametrize("method", ["hillclimb_slow", "hillclimb_fast", "hillclimb_dim"])
def test_neighbour_rule_exhaustively_on_a_toy_grid(method):
    sizes = [len(v) for _, v in TOY]
    for x in itertools.product(*[range(n) for n in sizes]):
        reached = set()
        for seed in range(60):
            y = hs.neighbour(method, x, TOY, random.Random(seed))
            assert all(0 <= b < n for b, n in zip(y, sizes))
            moved = [i for i in range(3) if y[i] != x[i]]
            if method == "hillclimb_slow":
                assert len(moved) <= 1 and all(abs(y[i] - x[i]) == 1 for i in moved)
            elif method == "hillclimb_fast":
                assert all(abs(y[i] - x[i]) <= 1 for i in range(3))
            else:
                assert len(moved) <= 1
            reached.add(tuple(y))
        # the draws do reach what the rule allows: the point itself and more than one other
        assert tuple(x) in reached and len(reached) >= 3
        if method == "hillclimb_fast":
            assert any(sum(a != b for a, b in zip(y, x)) >= 2 for y in reached)
        if method == "hillclimb_dim":
            assert any(abs(y[1] - x[1]) >= 2 for y in reached)     # a redraw is not bound to the neighbours


@pytest.mark.parametrize("method", hs.METHODS)
def test_same_seed_gives_the_same_candidates_and_only_valid_ones(method):
    runs = []
    for seed in (5, 5, 6):
        stub, results = Stub(), []
        mine = hs.search(method, stub, TOY, 12, random.Random(seed), results)
        assert len(mine) == 12 and results == mine and all(p["pi1"] <= p["pi2"] for p in stub.seen)
        assert all(set(ps) == {"pi1", "pi2", "blur_t"} for _, ps in mine)
        # parameters outside the grid keep the defaults
        assert all(p["sgm_q1"] == stub.prm["sgm_q1"] and p["alpha1"] == stub.prm["alpha1"] for p in stub.seen)
        runs.append([ps for _, ps in mine])
    assert runs[0] == runs[1] and runs[0] != runs[2]


def test_hillclimb_starts_from_the_defaults_and_then_from_the_best():
    stub = Stub()
    x0 = hs.snap(stub.prm, TOY)
    assert x0 == [1, 2, 1]             # pi2 = 4.1 is no grid value: snapped to 4.0
    results = []
    hs.search("hillclimb_slow", stub, TOY, 1, random.Random(0), results)
    first = hs.snap(results[0][1], TOY)
    assert sum(abs(a - b) for a, b in zip(first, x0)) <= 1
    # with results, the next candidate is a neighbour of the best of them, wherever the defaults are
    results = [(0.9, dict(pi1=1.0, pi2=2.0, blur_t=1)), (0.2, dict(pi1=3.0, pi2=5.0, blur_t=2)), (0.5, dict(pi1=2.0, pi2=2.0, blur_t=1))]
    for seed in range(20):
        r = list(results)
        hs.search("hillclimb_slow", stub, TOY, 1, random.Random(seed), r)
        assert sum(abs(a - b) for a, b in zip(hs.snap(r[-1][1], TOY), [2, 3, 1])) <= 1
    with pytest.raises(ValueError, match="method"):
        hs.search("anneal", stub, TOY, 1, random.Random(0), [])


def test_emit_gets_every_candidate_in_grid_order():
    lines = []
    mine = hs.search("random", Stub(), TOY, 4, random.Random(1), [], lambda s, ps: lines.append(hs.format_line(s, "kitti", "fast", "test_te", ps)))
    assert len(lines) == 4
    for line, (score, ps) in zip(lines, mine):
        assert re.fullmatch(r"\S+ kitti fast test_te -pi1 \S+ -pi2 \S+ -blur_t \S+", line)
        assert hs.parse_line(line, "kitti", "fast", "test_te", TOY) == (score, {k: float(v) for k, v in ps.items()})


# ---- refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv, word", [
    (["random", "kitti", "fast", "train_tr", "random:3"], "train_tr search is not supported"),
    (["hillclimb_dim", "mb", "slow", "da", "random:3"], "da search is not supported"),
    (["random", "kitti", "fast", "test_te", "random:3", "-in_flight", "0"], "-in_flight"),
])
def test_parse_refusals(argv, word):
    with pytest.raises(SystemExit) as e:
        hs.parse(argv)
    assert word in str(e.value)


@pytest.mark.parametrize("argv", [["anneal", "kitti", "fast", "test_te", "random:3"], ["random", "eth3d", "fast", "test_te", "random:3"],
                                  ["random", "kitti", "resnet", "test_te", "random:3"], ["random", "kitti", "fast", "submit", "random:3"],
                                  ["random", "kitti", "fast", "test_te"]])
def test_parse_refuses_unknown_words(argv, capsys):
    with pytest.raises(SystemExit):
        hs.parse(argv)
    capsys.readouterr()


def test_a_net_that_does_not_fit_the_arch_is_refused(tmp_path):
    from mc_cnn_amd import main
    layers = main.load_net("random:1", "kitti", "slow")       # fm 112
    f = str(tmp_path / "slow.npz")
    np.savez(f, **{"%s%d" % (k, i + 1): a for i, wb in enumerate(layers) for k, a in zip("wb", wb)})
    with pytest.raises(SystemExit, match="does not fit kitti fast"):
        hs.check_net(f, "kitti", "fast")
    with pytest.raises(SystemExit, match="does not fit kitti slow"):    # no Linears in the file
        hs.check_net(f, "kitti", "slow")
    with pytest.raises(SystemExit, match="does not fit mb fast"):       # four convolutions, mb has five
        hs.check_net(f, "mb", "fast")
    got, fc = hs.check_net("random:3", "kitti", "fast")
    assert len(got) == 4 and fc is None
    got, fc = hs.check_net("random:3", "mb", "slow")
    assert len(got) == 5 and len(fc) == 4
    assert hs.check_net("anything", "kitti", "census") == ([], None)


def test_parse_defaults():
    opt = hs.parse(["hillclimb_fast", "kitti2015", "census", "test_te", "none"])
    assert (opt.n, opt.seed, opt.log, opt.data_dir, opt.disp_max, opt.cache_gb, opt.in_flight, opt.gpu, opt.no_reuse) == \
        (0, 42, "", "", 228, 48.0, 2, 1, False)
    assert (opt.a, opt.at) == ("test_te", 0)


# ---- libmceval.so ----------------------------------------------------------------------------------------------------------------
def test_eval_lib_loads_without_a_gpu_and_exports_the_headers_symbols():
    """what only libmceval.so has; tests/test_libraries_host.py holds it to the contract of every library"""
    assert L.exported_abi(ev.LIB_PATH) == {"mc_eval_version", "mc_eval_last_error", "mc_eval_error"}
    assert ev.load().mc_eval_version() == ev.ABI_VERSION == 1
    assert L.built_kernels(ev.LIB_PATH) == {"eval_error_kernel"}
    assert L.print_libraries()["libmceval.so"] == ["eval.o", "error.o"]


def test_mc_eval_error_refusals_write_nothing():
    lib = ev.load()
    counts = np.array([7, 8, 9, 10], np.int32)       # host memory: a refused call must not touch it, let alone launch
    cp = counts.ctypes.data
    P = 4096                                         # a non-null pointer that is never dereferenced

    def call(pred=P, pred_ld=160, actual=P, actual_ld=170, H=48, W=160, counts=cp):
        return lib.mc_eval_error(pred, pred_ld, actual, actual_ld, H, W, 3.0, counts, None)

    bad = [("H 0", lambda: call(H=0), "dims"), ("W 0", lambda: call(W=0), "dims"), ("H negative", lambda: call(H=-3), "dims"),
           ("pred_ld below W", lambda: call(pred_ld=159), "stride"), ("actual_ld below W", lambda: call(actual_ld=100), "stride"),
           ("2^31 pixels", lambda: call(H=65536, W=32768, pred_ld=32768, actual_ld=32768), "2^31"),
           ("null pred", lambda: call(pred=None), "null"), ("null actual", lambda: call(actual=None), "null"),
           ("null counts", lambda: call(counts=None), "null")]
    for what, f, word in bad:
        rc = f()
        assert rc == ev.EINVAL, (what, rc)
        assert word in ev.last_error(), (what, ev.last_error())
        assert counts.tolist() == [7, 8, 9, 10], what
    with pytest.raises(ev.EvalError, match="stride"):
        ev.check(call(pred_ld=1), "mc_eval_error")
