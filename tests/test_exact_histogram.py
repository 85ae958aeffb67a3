"""tests/exact_histogram.py, the plain-Python reference of the histogram tests, pinned to the reference's own test table
and to degenerate edge tables (tests/golden/histogram_vectors.json; data only).  No library, no device."""
import json
import math
import os
import random
from fractions import Fraction

import pytest

import exact_histogram as eh

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "histogram_vectors.json")) as f:
    GOLDEN = json.load(f)


def test_the_reference_table():
    """analyzers/advanced/tests.rs: 1, 2, 2, 3, 3, 3, 4, 5, 10 and a NULL, 5 buckets"""
    g = GOLDEN["reference_table"]
    r = eh.value_range(g["values"])
    assert (r["total"], r["nulls"], r["non_finite"], r["n"]) == (10, 1, 0, g["total_count"])
    assert (r["min"], r["max"]) == (g["min"], g["max"])
    assert r["sum"] == Fraction(g["mean_numerator"]) and r["sum"] / r["n"] == Fraction(g["mean_numerator"], g["mean_denominator"])
    assert r["sum_squared"] == 1 + 4 + 4 + 9 + 9 + 9 + 16 + 25 + 100
    edges = eh.edges_of(r["min"], r["max"], g["num_buckets"])
    assert edges == g["edges"]
    assert eh.counts_of(g["values"], edges) == (g["counts"], g["else_rows"], 0)
    state = eh.histogram_state(g["values"], g["num_buckets"])
    assert len(state["buckets"]) == g["buckets"] and state["total_count"] == g["total_count"]
    assert [b["count"] for b in state["buckets"]] == g["counts"]
    assert state["buckets"][1] == {"lower_bound": 2.8, "upper_bound": 4.6, "count": 4}
    assert (state["sum"], state["sum_squared"]) == (33.0, 177.0)


@pytest.mark.parametrize("case", GOLDEN["degenerate"], ids=lambda c: c["name"])
def test_degenerate_edge_tables(case):
    edges = eh.edges_of(case["min"], case["max"], case["num_buckets"])
    assert len(edges) == case["num_buckets"] + 1
    if "edges" in case:
        assert edges == case["edges"]
    if case.get("last_edge_equals_max"):
        assert edges[-1] == case["max"]  # max + width * 0.001 rounded back to max
    assert eh.bucket_of(case["probe"], edges) == (case["bucket"], case["else"])
    assert eh.bucket_of(case["min"], edges) == (0, False) or case["num_buckets"] == 1000


def test_width_rule():
    assert eh.bucket_width(0.0, 10.0, 5) == 2.0
    assert eh.bucket_width(3.0, 3.0, 5) == 1.0       # no range
    assert eh.bucket_width(0.0, 10.0, 1) == 1.0      # one bucket: width 1.0, the last edge still covers the maximum
    assert eh.edges_of(0.0, 10.0, 1) == [0.0, 10.001]


def test_the_case_chain_is_walked_literally():
    edges = [0.0, 1.0, 2.0, 3.0]
    assert [eh.bucket_of(x, edges) for x in (0.0, 0.999, 1.0, 2.5)] == [(0, False), (0, False), (1, False), (2, False)]
    assert eh.bucket_of(3.0, edges) == (2, True) and eh.bucket_of(-1.0, edges) == (2, True) and eh.bucket_of(1e300, edges) == (2, True)
    # a last edge below the one before: the last bucket's own WHEN never holds
    assert eh.bucket_of(2.0, [0.0, 1.0, 2.0, 1.5]) == (2, True) and eh.bucket_of(1.7, [0.0, 1.0, 2.0, 1.5]) == (1, False)
    # equal interior edges: the empty buckets between them take nothing
    assert eh.bucket_of(1.0, [0.0, 1.0, 1.0, 1.0, 2.0]) == (3, False)


def test_non_finite_rows_and_nulls():
    values = [1.0, None, math.nan, math.inf, -math.inf, 2.0, None, 2**53 + 1]
    r = eh.value_range(values)
    assert (r["total"], r["nulls"], r["non_finite"], r["n"]) == (8, 2, 3, 3)
    assert r["max"] == float(2**53)  # CAST AS DOUBLE rounds to even
    assert eh.counts_of(values, [0.0, 1.5, 1e17]) == ([1, 2], 0, 3)
    assert eh.value_range([None, math.nan])["min"] is None and eh.histogram_state([None], 5)["buckets"] == []


def test_sums_are_exact_and_the_bounds_hold_for_plain_summation():
    rng = random.Random(1)
    values = [rng.gauss(0.0, 1.0) * 10.0 ** rng.randint(-5, 12) for _ in range(5000)] + [1e150, -1e150, 5e-324]
    r = eh.value_range(values)
    assert r["sum"] == sum(Fraction(v) for v in values) and r["sum_squared"] == sum(Fraction(v) ** 2 for v in values)
    assert r["abs_sum"] == sum(abs(Fraction(v)) for v in values)
    b_sum, b_sq = eh.sum_bounds(r)
    for order in (values, sorted(values), values[::-1]):
        s = q = 0.0
        for v in order:
            s += v
            q += v * v
        assert abs(Fraction(s) - r["sum"]) <= b_sum and abs(Fraction(q) - r["sum_squared"]) <= b_sq
    assert eh.sum_bounds(eh.value_range([]))[0] == 0


def test_both_walks_of_the_chain_agree():
    rng = random.Random(2)
    values = [rng.uniform(-5.0, 1005.0) for _ in range(3000)] + [None, math.nan, 0.0, 1000.0]
    for edges in (eh.edges_of(0.0, 1000.0, 1000), eh.edges_of(0.0, 1000.0, 7), [0.0] + [250.0] * 40 + [900.0, 100.0]):
        values += edges + [math.nextafter(e, -math.inf) for e in edges]
        rows = eh.doubles(values)
        counts = [0] * (len(edges) - 1)
        else_rows = 0
        for d in rows:
            if math.isfinite(d):
                b, e = eh.bucket_of(d, edges)
                counts[b] += 1
                else_rows += e
        assert eh.counts_of_columnwise(values, edges) == (counts, else_rows, 1)


# ---- the numpy fast paths of the differential tester, against the plain walks -----------------------------------------
def _special_column(rng, n, pool):
    import numpy as np

    v = np.round(rng.standard_normal(n) * 10, 1)
    m = rng.random(n) < 0.1
    v[m] = np.array(pool, np.float64)[rng.integers(0, len(pool), int(m.sum()))]
    valid = rng.random(n) >= 0.1
    return v, valid, [x if ok else None for x, ok in zip(v.tolist(), valid.tolist())]


@pytest.mark.parametrize("n", [0, 1, 7, 255, 256, 257, 5000])
@pytest.mark.parametrize("pool", [[0.0], [float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 5e-324, -5e-324, 1e308],
                                  [1e154, -1e154, 1.5e-162, 2.0 ** -537, 2.0 ** 1023]], ids=["plain", "specials", "limits"])
def test_numpy_range_and_counts_equal_the_walks(n, pool):
    """value_range_np (the exact sums in segments of int64) and counts_of_np (binary search) over specials, squares
    that overflow or underflow, repeated edges, and a last edge below the one before"""
    import numpy as np

    rng = np.random.default_rng(n)
    v, valid, xs = _special_column(rng, n, pool)
    r = eh.value_range(xs)
    assert eh.value_range_np(v, valid) == r
    if r["n"] == 0:
        return
    finite = v[np.isfinite(v)]
    sample = sorted(rng.choice(finite, 12).tolist())
    for edges in (eh.edges_of(r["min"], r["max"], 7), eh.edges_of(-3.0, 4.0, 1000), [0.0, 1.0], sample,
                  sample[:6] + sample[5:6] * 3 + sample[6:], sample[:-1] + [sample[3]]):
        assert eh.counts_of_np(v, valid, edges) == eh.counts_of(xs, edges) == eh.counts_of_columnwise(xs, edges)


def test_numpy_exact_sum_of_integers_beyond_2_53():
    import numpy as np

    v = np.random.default_rng(1).integers(-2**62, 2**62, 3000).astype(np.float64)
    assert eh.exact_sum_np(v) == sum(int(x) for x in v.tolist()) == eh.exact_sum(v.tolist())
    assert eh.exact_sum_np(v, 2) == sum(int(x) ** 2 for x in v.tolist()) == eh.exact_sum(v.tolist(), 2)


def test_sum_rules_and_infinite_squares():
    """1e308: its rounded square is infinite (sum_squared must be +inf), and two of them overflow a plain sum in some
    order (an infinity of the exact sum's sign, or within the bound); a NaN passes neither"""
    inf, nan = math.inf, math.nan
    r = eh.value_range([1e308, 1e308, -2.0, None, nan])
    assert r["infinite_squares"] == 2 and r["abs_sum_squared"] == 4 and r["sum_squared"] == 2 * Fraction(1e308) ** 2 + 4
    rule_sum, rule_sq = eh.sum_rules(r)
    assert (rule_sum, rule_sq) == (("either", 1.0), ("infinite", 1.0))
    bound_sum, bound_sq = eh.sum_bounds(r)
    assert eh.sum_failure(inf, r["sum"], bound_sum, rule_sum) is None
    assert eh.sum_failure(-inf, r["sum"], bound_sum, rule_sum) is not None
    assert eh.sum_failure(nan, r["sum"], bound_sum, rule_sum) is not None
    assert eh.sum_failure(1e308, r["sum"], bound_sum, rule_sum) is not None  # finite, and far outside the bound
    assert eh.sum_failure(inf, r["sum_squared"], bound_sq, rule_sq) is None
    assert eh.sum_failure(1e308, r["sum_squared"], bound_sq, rule_sq) is not None
    assert eh.sum_failure(nan, r["sum_squared"], bound_sq, rule_sq) is not None
    small = eh.value_range([1.5, -2.0, 4.0])
    assert eh.sum_rules(small) == (("bound", 1.0), ("bound", 1.0))
    assert eh.sum_failure(3.5, small["sum"], eh.sum_bounds(small)[0], ("bound", 1.0)) is None
    assert eh.sum_failure(inf, small["sum"], eh.sum_bounds(small)[0], ("bound", 1.0)) is not None
    negative = eh.value_range([-1e308, -1e308, 3.0])
    assert eh.sum_rules(negative)[0] == ("either", -1.0)
    # 2^1023 is where a partial sum may first pass DBL_MAX
    assert eh.sum_rules(eh.value_range([2.0 ** 1022, 2.0 ** 1021]))[0][0] == "bound"
    assert eh.sum_rules(eh.value_range([2.0 ** 1022, 2.0 ** 1022]))[0][0] == "either"
