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
