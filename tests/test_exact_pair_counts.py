"""tests/exact_pair_counts.py held to hand-worked cases and to the reference's own categorical table
(tests/golden/pair_counts_vectors.json): the walk, the order of the pairs, every counter's precedence, the range phase,
the analyzer's state form and the metric with its bound."""
import json
import math
import os

import exact_joint as ej
import exact_pair_counts as ex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_counts_vectors.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)["categorical_table"]


def test_a_hand_worked_walk():
    xs = ["a", "a", None, "b", "a", "", "b"]
    ys = ["u", "v", "u", None, "u", "u", "u"]
    w = ex.walk(xs, ys)
    assert w["counts"] == {(b"", b"u"): 1, (b"a", b"u"): 2, (b"a", b"v"): 1, (b"b", b"u"): 1}
    assert list(w["counts"]) == [(b"", b"u"), (b"a", b"u"), (b"a", b"v"), (b"b", b"u")]
    assert (w["seen"], w["both_non_null"], w["distinct"], w["counted"]) == (7, 5, 4, 5)
    assert (w["overflow_rows"], w["long_rows"], w["non_finite"], w["out_of_range"]) == (0, 0, 0, 0)


def test_pairs_are_not_concatenations():
    w = ex.walk(["ab", "a", "", "x"], ["c", "bc", "x", ""])
    assert w["counts"] == {(b"", b"x"): 1, (b"a", b"bc"): 1, (b"ab", b"c"): 1, (b"x", b""): 1}


def test_the_order_is_bytewise_with_a_prefix_first():
    w = ex.walk(["b", "ab", "a", "ÿ", "a"], ["z", "z", "zz", "z", "z"])
    assert list(w["counts"]) == [(b"a", b"z"), (b"a", b"zz"), (b"ab", b"z"), (b"b", b"z"), ("ÿ".encode(), b"z")]


def test_long_rows_take_precedence_then_non_finite_then_out_of_range():
    binning = (0.0, 1.0, 4)  # cells 0 .. 4 for values in [0, 5)
    xs = [0.5, 4.0, 4.99, 5.0, -0.1, float("nan"), float("inf"), float("nan"), 1.0, None]
    ys = ["k", "k", "k", "k", "k", "k", "k", "long!", "long!", "k"]
    w = ex.walk(xs, ys, x_side=binning, max_value_bytes=4)
    assert w["counts"] == {(0, b"k"): 1, (4, b"k"): 2}
    assert (w["both_non_null"], w["long_rows"], w["non_finite"], w["out_of_range"]) == (9, 2, 2, 2)
    assert ex.walk(ys, xs, y_side=binning, max_value_bytes=4)["counts"] == {(b"k", 0): 1, (b"k", 4): 2}


def test_bin_indices_are_exact_joints():
    xs = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    ys = ["s"] * 10
    binning = ex.binning_of(xs, ys, 3)
    assert binning == (1.0, 3.0, 3)
    cells, outside = ej.joint_counts(xs, [0.0] * 10, (1.0, 3.0, 0.0, 1.0, 3))
    assert outside == 0
    assert ex.walk(xs, ys, x_side=binning)["counts"] == {(i, b"s"): c for (i, _), c in sorted(cells.items())}
    assert ex.walk(xs, ys, x_side=binning)["counts"][(3, b"s")] == 1  # the row at the maximum lands in bin `bins`


def test_the_range_phase():
    nums = [3, None, -2.5, float("nan"), 7, float("-inf"), 9]
    strs = ["a", "b", "c", "d", "e", "f", None]
    assert ex.side_range(nums, strs) == dict(seen=7, both_non_null=5, n=3, non_finite=2, min=-2.5, max=7.0)
    assert ex.side_range([None, 1], ["a", None]) == dict(seen=2, both_non_null=0, n=0, non_finite=0, min=None, max=None)
    assert ex.binning_of([4, 4, 4], ["a", "b", "c"], 10) == (4.0, 1.0, 10)  # a constant column: width 1.0
    assert ex.binning_of([None], ["a"], 10) is None


def test_the_reference_categorical_table():
    g = golden()
    xs, ys = g["columns"]["category"], g["columns"]["value"]
    assert len(xs) == len(ys) == 100
    w = ex.walk(xs, ys)
    assert [[x.decode(), y.decode(), c] for (x, y), c in w["counts"].items()] == g["expect"]["pairs"]
    assert ex.analyzer_state(w["counts"], g["bins"]) == g["expect"]["state"]
    exact, bound = ex.metric_bound(w["counts"])
    assert exact == 0.0 and exact < g["expect"]["metric_below"]
    assert 0.0 < bound < 1e-14


def test_the_metric_of_a_dependent_table():
    counts = ex.walk(["a"] * 8 + ["b"] * 8, ["u"] * 8 + ["v"] * 8)["counts"]
    exact, bound = ex.metric_bound(counts)
    assert abs(exact - 1.0) < 1e-15 and bound < 1e-14  # two equiprobable, fully dependent values: one bit
    mixed = ex.walk([0, 0, 1, 1], ["u", "u", "v", "v"], x_side=(0.0, 0.5, 2))["counts"]
    assert mixed == {(0, b"u"): 2, (2, b"v"): 2}
    assert ex.analyzer_state(mixed, 2) == dict(n=4, joint_counts=[["0.0", "u", 2], ["2.0", "v", 2]],
                                               x_counts={"0.0": 2, "2.0": 2}, y_counts={"u": 2, "v": 2}, bins=2)
    assert math.isclose(ex.metric_bound(mixed)[0], 1.0)
