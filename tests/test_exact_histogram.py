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
