"""tests/exact_joint.py held to the reference's own vectors (tests/golden/mutual_information_vectors.json: the unit
tests of TG/analyzers/advanced/mutual_information.rs, restated as data with their file:line)."""
import json
import os

import pytest

import exact_joint as ej

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "mutual_information_vectors.json")) as f:
    GOLDEN = json.load(f)


def table(name):
    xs = [float(i) for i in range(100)]
    ys = [float((37 * i + 13) % 100) for i in range(100)] if name == "independent" else [float(2 * i) for i in range(100)]
    return xs, ys


def state_of(name):
    xs, ys = table(name)
    binning = ej.binning_of(xs, ys, GOLDEN[name]["bins"])
    cells, outside = ej.joint_counts(xs, ys, binning)
    assert outside == 0
    return cells, sum(cells.values())


def test_independent_vector():
    g = GOLDEN["independent"]
    cells, n = state_of("independent")
    value, _, used = ej.mutual_information(cells, n)
    assert n == g["rows"] and used == len(cells) == g["non_empty_cells"]
    assert float(value) < g["metric_below"]
    assert abs(float(value) - float(g["metric"])) < 1e-13
    xc, yc = ej.marginals(cells)
    assert [xc.get(i, 0) for i in range(6)] == g["x_marginals"]
    assert [yc.get(i, 0) for i in range(6)] == g["y_marginals"]


def test_dependent_vector():
    g = GOLDEN["dependent"]
    cells, n = state_of("dependent")
    value, _, used = ej.mutual_information(cells, n)
    assert n == g["rows"] and used == len(cells) == g["non_empty_cells"]
    assert float(value) > g["metric_above"]
    assert abs(float(value) - float(g["metric"])) < 1e-13


def _state(d):
    return dict(n=d["n"], bins=d["bins"], joint_counts={(x, y): c for x, y, c in d["joint_counts"]},
                x_counts=dict(d["x_counts"]), y_counts=dict(d["y_counts"]))


def test_merge_vector():
    g = GOLDEN["merge"]
    assert ej.merge_states([_state(s) for s in g["states"]]) == _state(g["merged"])
    other = _state(g["states"][1])
    other["bins"] = 10
    with pytest.raises(ValueError, match=g["different_bins_error"]):
        ej.merge_states([_state(g["states"][0]), other])


def test_maximum_lands_in_the_last_or_the_extra_bin():
    import random

    rng = random.Random(7)
    for _ in range(20000):
        lo = rng.uniform(-1e6, 1e6)
        hi = lo + rng.uniform(1e-6, 1e6)
        bins = rng.randint(2, 127)
        w = ej.bin_width(lo, hi, bins)
        assert int((hi - lo) / w) in (bins - 1, bins)


def test_non_finite_and_null_rows_are_left_out():
    xs = [1.0, None, float("nan"), 4.0, float("inf"), 2.0]
    ys = [1.0, 2.0, 3.0, None, 5.0, float("-inf")]
    r = ej.pair_range(xs, ys)
    assert (r["n"], r["non_finite"], r["x_min"], r["x_max"]) == (1, 3, 1.0, 1.0)
    cells, outside = ej.joint_counts(xs, ys, ej.binning_of(xs, ys, 4))
    assert cells == {(0, 0): 1} and outside == 0
    assert ej.binning_of([None], [1.0], 5) is None
    assert float(ej.mutual_information({}, 0)[0]) == 0.0


# ---- the numpy fast paths of the differential tester, against the plain walks -----------------------------------------
def test_numpy_range_and_counts_equal_the_walks():
    import numpy as np

    for n in (0, 1, 6, 4000):
        rng = np.random.default_rng(n)
        x = np.round(rng.standard_normal(n) * 10, 1)
        m = rng.random(n) < 0.1
        pool = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, 1e308])
        x[m] = pool[rng.integers(0, len(pool), int(m.sum()))]
        y = rng.integers(-2**62, 2**62, n)
        xv, yv = rng.random(n) >= 0.1, rng.random(n) >= 0.3
        xs = [v if ok else None for v, ok in zip(x.tolist(), xv.tolist())]
        ys = [v if ok else None for v, ok in zip(y.tolist(), yv.tolist())]
        yd = y.astype(np.float64)
        r = ej.pair_range(xs, ys)
        assert ej.pair_range_np(x, yd, xv & yv) == r
        for bins in (2, 5, 127):
            b = ej.binning_of(xs, ys, bins)
            assert ej.binning_of_range(r, bins) == b
            if b is None:
                continue
            moved = (b[0] + b[1] / 2, b[1], b[2] + b[3] / 2, b[3], bins)
            tiny = (b[0], 5e-324, b[2], b[3], bins)  # (a quotient that overflows: outside)
            for binning in (b, moved, tiny):
                assert ej.joint_counts_np(x, yd, xv & yv, binning) == ej.joint_counts(xs, ys, binning)
