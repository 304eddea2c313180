"""CPU: the oracle alone over the tables of tests/predict_grid_cases.py -- what tests/test_gpu_predict_grid.py compares mc_predict
with.  A GPU comparison over an axis says something only if the axis' values give different maps and none of them is NaN (EvalSet.score
raises on NaN: a table that produced it would test the wrong thing)."""
import math

import numpy as np
import pytest

import predict_grid_cases as pg


def distinct(maps):
    return len(set(np.ascontiguousarray(m, np.float32).tobytes() for m in maps))


def test_the_tables_cover_the_grids():
    from mc_cnn_amd import hs
    n = {fam: sum(len(pg.axis_cases(fam, k)) for k, _ in pg.grid(fam)) for fam in pg.FAMILIES}
    assert n == dict(A=95, B=68, C=66, D=95, E=27)                      # no candidate of a one-axis sweep has pi1 > pi2
    for fam, f in pg.FAMILIES.items():
        g = pg.grid(fam)
        assert set(f["counts"]) == set(k for k, _ in g)
        if f["axes"] is None:
            assert g == hs.grid_of(f["dataset"], f["arch"])              # every axis the search draws
        else:
            assert [k for k, _ in g] == list(f["axes"])
    assert len(pg.axes()) == 12 + 8 + 8 + 12 + 4
    fb = pg.FAMILIES["B"]
    assert fb["D"] % 4 != 0 and fb["W"] % 32 != 0


@pytest.mark.parametrize("fam,axis", pg.axes(), ids=lambda v: str(v))
def test_an_axis_moves_the_disparity_map(oracle, fam, axis):
    cases = pg.axis_cases(fam, axis)
    maps = [pg.want(oracle, fam, p)["disp"] for p in cases]
    for p, m in zip(cases, maps):
        assert not np.isnan(m).any(), "NaN in the oracle's disp: %s" % pg.label(fam, p)
    n = distinct(maps)
    print(fam, axis, "%d distinct maps of %d values" % (n, len(cases)))
    assert n >= 3 and n == pg.FAMILIES[fam]["counts"][axis]


@pytest.mark.parametrize("fam", list(pg.FAMILIES))
def test_the_corners_are_free_of_nan(oracle, fam):
    from mc_cnn_amd import hs
    for name, p in pg.corner_cases(fam):
        assert hs.valid(p), name
        assert not np.isnan(pg.want(oracle, fam, p)["disp"]).any(), "NaN in the oracle's disp: %s %s" % (fam, name)
    if "L1" in dict(pg.grid(fam)):
        assert len(pg.corner_cases(fam)) == 2 + 4 + 8


@pytest.mark.parametrize("fam", list(pg.FAMILIES))
def test_the_walk_is_valid_and_varied(oracle, fam):
    from mc_cnn_amd import hs
    w = pg.walk(fam)
    assert len(w) == pg.WALK_N == 40 and all(hs.valid(p) for p in w)
    assert pg.walk(fam) == w                                             # seeded: the GPU test walks the same list
    for p in w:
        assert all(p[k] in values for k, values in pg.grid(fam))
    maps = [pg.want(oracle, fam, p)["disp"] for p in w]
    assert not any(np.isnan(m).any() for m in maps)
    n = distinct(maps)
    print(fam, "%d distinct maps of %d candidates" % (n, len(w)))
    assert n >= 30


def test_which_blur_sigmas_take_the_run_time_size_kernel(oracle):
    """`mean2d` (csrc/post.hip) has compiled instances for the kernel sizes 13, 19, 29, 37 and 49; every other size goes to the
    run-time-size mean2d_kernel.  Whoever adds an instance: keep a case of the generic path in the grid tests."""
    from mc_cnn_amd import hs
    sigmas = dict(hs.grid_of("kitti", "slow"))["blur_sigma"]
    assert sigmas == dict(hs.grid_of("mb", "fast"))["blur_sigma"]
    generic = [s for s in sigmas if 2 * math.ceil(3 * s) + 1 not in (13, 19, 29, 37, 49)]
    assert tuple(generic) == pg.GENERIC_BLUR_SIGMAS == (1.0, 1.29, 2.15, 3.59, 10.0)
    assert [2 * math.ceil(3 * s) + 1 for s in generic] == [oracle.gaussian(s).shape[0] for s in generic] == [7, 9, 15, 23, 61]
