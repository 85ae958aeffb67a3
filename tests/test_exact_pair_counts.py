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


# ---- the numpy twins against the plain walks -----------------------------------------------------------------------------
def _columns(rng, n, vocab=12, null_rate=0.2, specials=True):
    """a string column as (list with None, (codes, words), mask) and a numeric one as (list with None, doubles, mask)"""
    import numpy as np

    words = [b"", b"a", b"ab", b"b", "ÿ".encode(), b"long word!", b"x" * 40][:vocab] + \
        [b"w%d" % k for k in range(max(0, vocab - 7))]
    codes = rng.integers(0, len(words), size=n)
    s_mask = rng.random(n) >= null_rate
    strs = [words[c] if m else None for c, m in zip(codes, s_mask)]
    nums = np.round(rng.standard_normal(n) * 4, 1)
    if specials and n:
        pool = np.array([np.nan, np.inf, -np.inf, -0.0, 40.0, -40.0, 5e-324])
        hit = rng.random(n) < 0.15
        nums[hit] = pool[rng.integers(0, len(pool), size=int(hit.sum()))]
    n_mask = rng.random(n) >= null_rate
    return (strs, (codes, words), s_mask), ([float(v) if m else None for v, m in zip(nums, n_mask)], nums, n_mask)


def test_the_numpy_twins_agree_with_the_walks():
    import numpy as np

    rng = np.random.default_rng(20260)
    for n, null_rate, max_bytes in ((0, 0.0, 256), (1, 0.0, 256), (300, 0.2, 256), (300, 0.2, 4), (300, 1.0, 4),
                                    (2000, 0.05, 1), (2000, 0.3, 9)):
        (s1, c1, m1), (nums, doubles, mn) = _columns(rng, n, null_rate=null_rate)
        (s2, c2, m2), _ = _columns(rng, n, vocab=3, null_rate=null_rate)
        # two string sides, the same column on both sides among them
        for (sa, ca, ma), (sb, cb, mb) in (((s1, c1, m1), (s2, c2, m2)), ((s1, c1, m1), (s1, c1, m1))):
            want = ex.walk(sa, sb, max_value_bytes=max_bytes)
            got = ex.walk_np(ca, cb, ma & mb, max_value_bytes=max_bytes)
            assert got == want and list(got["counts"]) == list(want["counts"]), (n, null_rate, max_bytes)
        # the range phase, and a numeric side on either side under the exact binning and a moved, narrower one
        r = ex.side_range(nums, s1)
        assert ex.side_range_np(doubles, mn & m1) == r
        for bins in (2, 10):
            exact = ex.binning_of(nums, s1, bins)
            assert ex.binning_of_range(r, bins) == exact
            for binning in ([exact, (exact[0] + exact[1] / 2, exact[1] / 3, bins)] if exact else [(0.0, 1.0, bins)]):
                want = ex.walk(nums, s1, x_side=binning, max_value_bytes=max_bytes)
                got = ex.walk_np(doubles, c1, mn & m1, x_side=binning, max_value_bytes=max_bytes)
                assert got == want and list(got["counts"]) == list(want["counts"]), (n, binning, max_bytes)
                want = ex.walk(s1, nums, y_side=binning, max_value_bytes=max_bytes)
                got = ex.walk_np(c1, doubles, mn & m1, y_side=binning, max_value_bytes=max_bytes)
                assert got == want and list(got["counts"]) == list(want["counts"]), (n, binning, max_bytes)
                if n == 2000 and max_bytes == 9 and binning is not exact:  # every class of rows is met
                    assert min(want[k] for k in ("counted", "long_rows", "non_finite", "out_of_range")) > 0, want


def test_the_twin_sees_what_the_walk_sees_in_a_hand_worked_table():
    import numpy as np

    binning = (0.0, 1.0, 4)
    xs = [0.5, 4.0, 4.99, 5.0, -0.1, float("nan"), float("inf"), float("nan"), 1.0, None]
    words = [b"k", b"long!"]
    codes = np.array([0, 0, 0, 0, 0, 0, 0, 1, 1, 0])
    doubles = np.array([0.0 if v is None else v for v in xs])
    both = np.array([v is not None for v in xs])
    w = ex.walk_np(doubles, (codes, words), both, x_side=binning, max_value_bytes=4)
    assert w["counts"] == {(0, b"k"): 1, (4, b"k"): 2}
    assert (w["both_non_null"], w["long_rows"], w["non_finite"], w["out_of_range"]) == (9, 2, 2, 2)
