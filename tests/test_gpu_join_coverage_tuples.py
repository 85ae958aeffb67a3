"""JoinCoverageConstraint on composite keys (on_multiple + composite_keys_on_device) end to end through
ValidationSuite.run(table, tables=..): status, metric and message are held EQUAL to the literal nested-loop joins of
tests/exact_key_probe_tuples.py, for every coverage type, distinct_only, passing and failing rates with the examples
number, on (Int64, Utf8)-keyed tables of a few hundred rows with duplicates, NULL components and strangers."""
import functools
import json

import numpy as np
import pyarrow as pa
import pytest

import exact_key_probe_tuples as ex
import term_amd.suite as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def tables():
    """orders(order_id Int64, code Utf8) and lines(oid Int32, tag LargeUtf8): 300 and 220 rows from 40 tuples; every
    tuple several times, a tenth of the components NULL, strangers on both sides"""
    rng = np.random.default_rng(2026)
    pool = [(k % 13, "c%d" % (k // 4)) for k in range(40)]

    def draw(n, lo, hi, strangers):
        rows = []
        for _ in range(n):
            a, b = pool[int(rng.integers(lo, hi))]
            if rng.random() < 0.1:
                a, b = strangers[int(rng.integers(0, len(strangers)))]
            rows.append((None if rng.random() < 0.05 else a, None if rng.random() < 0.05 else b))
        return rows

    left = draw(300, 0, 30, [(100, "x"), (101, "c1"), (1, "zz")])
    right = draw(220, 10, 40, [(200, "y"), (2, "c99")])
    orders = pa.table({"order_id": pa.array([r[0] for r in left], pa.int64()), "code": pa.array([r[1] for r in left], pa.string()),
                       "n": pa.array(range(len(left)), pa.int64())})
    lines = pa.table({"tag": pa.array([r[1] for r in right], pa.large_string()), "oid": pa.array([r[0] for r in right], pa.int32())})
    return left, right, {"orders": orders, "lines": lines}


def constraint(expected, coverage_type="left", distinct_only=False, max_examples=100):
    c = S.JoinCoverageConstraint("orders", "lines").on_multiple([("order_id", "oid"), ("code", "tag")])
    c = c.composite_keys_on_device(True).expect_match_rate(expected).coverage_type(coverage_type)
    return c.distinct_only(distinct_only).max_examples_reported(max_examples)


def run_constraint(c, tabs, as_json=False):
    cb = S.Check.builder("c").level(S.Level.ERROR).constraint(c)
    suite = S.ValidationSuite.builder("s").check(cb.build()).build()
    if as_json:
        suite = S.ValidationSuite(json.loads(json.dumps(suite.spec)))
    r = suite.run(None, tables=tabs)
    m = r.report.metrics
    assert m.total_checks == 1 and m.passed_checks + m.failed_checks == 1
    metric = m.custom_metrics.get("c.join_coverage")
    if m.passed_checks:
        assert r.is_success() and not r.report.issues
        return "success", metric, None
    assert len(r.report.issues) == 1 and r.report.issues[0].constraint_name == "join_coverage"
    message = r.report.issues[0].message
    return ("error" if message.startswith("Error evaluating constraint: ") else "failure"), metric, message


@pytest.mark.parametrize("expected", [0.05, 0.999], ids=["passes", "fails"])
@pytest.mark.parametrize("coverage_type", ["left", "right", "bidirectional"])
def test_the_coverage_types(coverage_type, expected):
    left, right, tabs = tables()
    want = ex.coverage_verdict("orders", "lines", left, right, expected, coverage_type)
    assert want[0] == ("success" if expected < 0.5 else "failure") and 0.1 < want[1] < 0.999
    assert run_constraint(constraint(expected, coverage_type), tabs) == want
    assert run_constraint(constraint(expected, coverage_type), tabs, as_json=True) == want
    if want[2]:
        assert "unmatched examples found)" in want[2]


def test_distinct_only_counts_the_first_left_key():
    left, right, tabs = tables()
    for expected in (0.5, 1.0, 1e9):  # (the rate can exceed 1: pairs over COUNT(DISTINCT order_id); the rate clamps at 1)
        want = ex.coverage_verdict("orders", "lines", left, right, min(expected, 1.0), "left", True)
        assert run_constraint(constraint(expected, "left", True), tabs) == want
    assert want[1] > 1.0
    # Bidirectional ignores it; with Right it is the constraint's error
    want = ex.coverage_verdict("orders", "lines", left, right, 0.999, "bidirectional")
    assert run_constraint(constraint(0.999, "bidirectional", True), tabs) == want
    status, _, message = run_constraint(constraint(0.5, "right", True), tabs)
    assert status == "error" and "distinct_only with RightCoverage" in message


def test_the_examples_number_at_its_limit_and_the_swapped_key_order():
    left, right, tabs = tables()
    for limit in (0, 1, 7, 100):
        want = ex.coverage_verdict("orders", "lines", left, right, 0.999, "left", False, limit)
        assert run_constraint(constraint(0.999, "left", False, limit), tabs) == want
    found = len(ex.nested_loop_left_join(left, right)[2])
    assert "(%d unmatched examples found)" % found in want[2] and found > 10
    assert any(not ex.all_valid(t) for t in ex.nested_loop_left_join(left, right)[2])  # (NULL-bearing tuples among them)
    # the pairs in the other order: the same join, a (Utf8, Int64) tuple
    c = S.JoinCoverageConstraint("orders", "lines").on_multiple([("code", "tag"), ("order_id", "oid")])
    c = c.composite_keys_on_device(True).expect_match_rate(0.999)
    assert run_constraint(c, tabs) == want
    # a table joined with itself on three keys: every all-valid row meets its duplicates
    c = S.JoinCoverageConstraint("orders", "orders").on_multiple([("order_id", "order_id"), ("code", "code"), ("order_id", "order_id")])
    three = [(a, b, a) for a, b in left]
    want = ex.coverage_verdict("orders", "orders", three, three, 1.0)
    assert run_constraint(c.composite_keys_on_device(True), tabs) == want and want[0] == "failure"


def test_without_the_opt_in_and_the_errors_of_a_pair():
    left, right, tabs = tables()
    c = S.JoinCoverageConstraint("orders", "lines").on_multiple([("order_id", "oid"), ("code", "tag")])
    status, _, message = run_constraint(c, tabs)
    assert status == "error" and "a join on 2 key pairs (orders.order_id, orders.code, ..) is not on the GPU path" in message
    mixed = S.JoinCoverageConstraint("orders", "lines").on_multiple([("order_id", "oid"), ("code", "oid")])
    status, _, message = run_constraint(mixed.composite_keys_on_device(True), tabs)
    assert status == "error" and "key pair 1" in message and "'orders.code' and 'lines.oid'" in message
    assert "a string and an integer column" in message
    floats = dict(tabs, lines=tabs["lines"].append_column("f", pa.array([1.0] * tabs["lines"].num_rows, pa.float64())))
    c = S.JoinCoverageConstraint("orders", "lines").on_multiple([("order_id", "oid"), ("n", "f")])
    status, _, message = run_constraint(c.composite_keys_on_device(True), floats)
    assert status == "error" and "'lines.f' is a Float64 column" in message and "not on the GPU path" in message
    nine = S.JoinCoverageConstraint("orders", "lines").on_multiple([("order_id", "oid")] * 9).composite_keys_on_device(True)
    status, _, message = run_constraint(nine, tabs)
    assert status == "error" and "9 key pairs" in message and "2 .. 8 pairs" in message
    missing = S.JoinCoverageConstraint("orders", "lines").on_multiple([("order_id", "oid"), ("code", "nope")])
    status, _, message = run_constraint(missing.composite_keys_on_device(True), tabs)
    assert status == "error" and "No field named lines.nope" in message
