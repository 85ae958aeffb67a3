"""tests/exact_join_coverage.py against itself: the plain walk and its numpy twin are held equal to each other, and both
to a literal nested-loop outer join on tables small enough for that, so that the formula
    matched = sum over rows of L of m_R(l),   total = matched + missing rows + NULL rows
is tested, not assumed; the route rule at its edges; the three coverage types, distinct_only, the examples count, the
verdict and the message on the golden vectors."""
import json
import os

import numpy as np
import pytest

import exact_join_coverage as ex
import exact_key_probe as kp

HERE = os.path.dirname(os.path.abspath(__file__))
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def table(rng, n, lo, hi, nulls):
    return rng.integers(lo, hi, n), (rng.random(n) >= nulls if nulls else None)


@pytest.mark.parametrize("seed", range(6))
def test_the_walks_agree_with_each_other_and_with_the_nested_loop_join(seed):
    rng = np.random.default_rng(seed)
    left, lm = table(rng, 60 + 20 * seed, -5, 25, 0.1 * (seed % 3))
    right, rm = table(rng, 40 + 10 * seed, 0, 30, 0.15 * (seed % 2))
    got = []
    for (near, nm), (far, fm) in (((left, lm), (right, rm)), ((right, rm), (left, lm))):
        records = ex.records_of(far, fm)
        s, p = ex.walk(near, nm, records)
        assert (s, p) == ex.walk_np(near, nm, records)
        total, matched, unmatched = ex.nested_loop_left_join(near, nm, far, fm)
        assert (p["join_rows"], p["pairs"]) == (total, matched)
        assert len(unmatched) == s["missing_keys"] + (1 if s["null_rows"] else 0)
        assert p["parent_rows"] == (len(far) if fm is None else int(fm.sum())) and p["max_count"] == max(c for _, c in records)
        assert s["seen"] == s["non_null"] + s["null_rows"] and s["non_null"] == s["matched"] + s["missing_rows"]
        got.append(p["pairs"])
    assert got[0] == got[1]  # P is the same number from either side


def test_all_counts_one_is_the_foreign_key_walk():
    rng = np.random.default_rng(7)
    child, cm = table(rng, 500, 0, 300, 0.1)
    keys = np.arange(0, 300, 3)
    s, p = ex.walk(child, cm, [(int(k), 1) for k in keys])
    plain = kp.walk(child, cm, keys, None)
    assert p["pairs"] == s["matched"] == plain["matched"] and s["entries"] == plain["entries"]
    assert (s["parent_keys"], s["parent_digest"]) == (plain["parent_keys"], plain["parent_digest"])


def test_duplicate_records_add_up_and_both_digests():
    records = [(5, 2), (7, 2**40), (5, 2**32 + 1), (-1, 3), (I64_MIN, 1)]
    child = [5, 7, -1, 9, 5, I64_MIN]
    s, p = ex.walk(child, [True, True, True, True, False, True], records)
    assert (s, p) == ex.walk_np(child, [True, True, True, True, False, True], records)
    assert p["pairs"] == (2 + 2**32 + 1) + 2**40 + 3 + 1 and p["max_count"] == 2**40
    assert p["parent_rows"] == 2 + 2**40 + 2**32 + 1 + 3 + 1 and s["parent_keys"] == 4
    assert p["join_rows"] == p["pairs"] + 1 + 1 and s["entries"] == {9: 1}
    # the count digest is a sum over the RECORDS, linear in the counts; the key digest a sum over the distinct keys
    merged = sorted(ex.multiplicities(records).items())
    assert ex.count_digest(records) == ex.count_digest(merged) == ex.count_digest_np([k for k, _ in merged], [c for _, c in merged])
    assert ex.count_digest(records) != ex.count_digest([(k, 1) for k, _ in merged])
    assert s["parent_digest"] == kp.digest([k for k, _ in merged]) != ex.count_digest([(k, 1) for k, _ in merged])
    assert ex.count_digest([(3, 2)]) == (2 * kp.mix64(3 ^ ex.COUNT_SALT)) & ex.M64


def test_the_route_rule():
    assert ex.route_of([]) == ex.ROUTE_EMPTY
    assert ex.route_of([42]) == ex.ROUTE_COUNT_ARRAY
    assert ex.route_of([0, 5, 9, 15]) == ex.ROUTE_COUNT_ARRAY     # range 16 == 4 * 4
    assert ex.route_of([0, 5, 9, 16]) == ex.ROUTE_COUNT_HASH      # range 17 == 4 * 4 + 1
    assert ex.route_of([0, 5, 9, 16, 16]) == ex.ROUTE_COUNT_ARRAY  # (the records count)
    assert ex.route_of([I64_MIN, I64_MAX]) == ex.ROUTE_COUNT_HASH  # the range wraps to 0
    assert ex.route_of([I64_MIN, I64_MAX - 1]) == ex.ROUTE_COUNT_HASH
    assert ex.route_of([-1, 0]) == ex.ROUTE_COUNT_ARRAY
    assert ex.route_of([1, 2, 3], n_records=0) == ex.ROUTE_EMPTY


def golden_cases():
    with open(os.path.join(HERE, "golden", "join_coverage_vectors.json")) as f:
        return json.load(f)["cases"]


def sides(case):
    return [([v or 0 for v in case[k]], [v is not None for v in case[k]]) for k in ("left", "right")]


@pytest.mark.parametrize("case", golden_cases(), ids=[c["name"] for c in golden_cases()])
def test_the_golden_vectors(case):
    (lv, lm), (rv, rm) = sides(case)
    status, metric, message = ex.coverage(case["left_table"], case["right_table"], lv, lm, rv, rm, case["coverage_type"],
                                          case["distinct_only"], case["expected"], case.get("max_examples", 100))
    assert (status, message) == (case["status"], case["message"])
    assert abs(metric - case["metric"]) <= 1e-12
    # the rate from the literal joins
    lt, lmatched, unmatched = ex.nested_loop_left_join(lv, lm, rv, rm)
    rt, rmatched, _ = ex.nested_loop_left_join(rv, rm, lv, lm)
    if case["coverage_type"] == ex.LEFT and case["distinct_only"]:
        lt = len(set(v for v, ok in zip(lv, lm) if ok))
    rates = {ex.LEFT: [lmatched / lt], ex.RIGHT: [rmatched / rt], ex.BIDIRECTIONAL: [lmatched / lt, rmatched / rt]}
    assert metric == min(rates[case["coverage_type"]])
    if message and "unmatched" in message:
        assert "(%d unmatched examples found)" % min(case.get("max_examples", 100), len(unmatched)) in message


def test_the_coverage_types_differ_and_the_errors():
    left, right = [1, 1, 2, 8, 0], [1, 2, 2, 2, 9, 0]
    lm = [True, True, True, True, False]
    rm = [True] * 5 + [False]
    rate = {k: ex.coverage("l", "r", left, lm, right, rm, k, False, 0.0)[1] for k in (ex.LEFT, ex.RIGHT, ex.BIDIRECTIONAL)}
    assert rate == {ex.LEFT: 5 / 7, ex.RIGHT: 5 / 7, ex.BIDIRECTIONAL: 5 / 7}  # P = 5 both ways; 2 unmatched rows each
    rate = ex.coverage("l", "r", left, lm, right + [9, 9], rm + [True, True], ex.RIGHT, False, 0.0)[1]
    assert rate == 5 / 9 and ex.coverage("l", "r", left, lm, right + [9, 9], rm + [True, True], ex.BIDIRECTIONAL)[1] == 5 / 9
    assert ex.coverage("l", "r", left, lm, right, rm, ex.LEFT, True, 0.0)[1] == 5 / 3  # COUNT(DISTINCT l) = 3
    assert ex.coverage("l", "r", left, lm, right, rm, ex.BIDIRECTIONAL, True, 0.0)[1] == 5 / 7  # ignored
    assert ex.coverage("l", "r", left, lm, right, rm, ex.RIGHT, True)[0] == "error"
    assert ex.coverage("l", "r", [], None, right, rm)[0] == "error"            # an empty side: no rows
    assert ex.coverage("l", "r", left, lm, [], None, ex.RIGHT)[0] == "error"
    assert ex.coverage("l", "r", left, lm, [], None, ex.LEFT, False, 0.0) == ("success", 0.0, None)
    assert ex.coverage("l", "r", [0], [False], right, rm, ex.LEFT, True)[0] == "error"  # no distinct key at all


def test_the_message_rounds_as_the_reference_formats():
    # 19999 / 20000 = 99.995 % reads 99.99 or 100.00 by the double's exact value, as {:.2} reads it
    left = list(range(20000))
    status, rate, message = ex.coverage("l", "r", left, None, left[:-1], None, ex.LEFT, False, 1.0, 0)
    assert status == "failure" and rate == 19999 / 20000
    from decimal import Decimal

    exact_text = str(Decimal(rate * 100.0).quantize(Decimal("0.01")))  # round-half-even on the exact binary value
    assert message == "Join coverage constraint failed: l -> r coverage is %s%% (expected: 100.00%%)" % exact_text
    assert ex.coverage("l", "r", left, None, left[:-1], None, ex.LEFT, False, 1.0, 5)[2].endswith("(1 unmatched examples found)")
    assert ex.coverage("l", "r", left, None, [], None, ex.LEFT, False, 1.0, 5, overflow=True)[2].endswith("(5 unmatched examples found)")
    assert ex.coverage("l", "r", [1, 2], None, [], None, ex.LEFT, False, 1.0, 5, overflow=True)[2].endswith("(at least 2 unmatched examples found)")
