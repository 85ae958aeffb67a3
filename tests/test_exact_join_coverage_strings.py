"""tests/exact_join_coverage_strings.py against itself and against tests/exact_join_coverage.py: the counted walk over
bytes is held equal to a literal nested-loop outer join on seeded small tables, so that
    matched = sum over rows of L of m_R(l),   total = matched + missing rows + NULL rows
is tested, not assumed; the verdicts are held equal to the integer reference's under an order-preserving renaming of
integer keys to strings; the byte bound, the identity and the rows multiset at their edges; the golden vectors."""
import json
import os

import numpy as np
import pytest

import exact_join_coverage as exi
import exact_join_coverage_strings as ex
import exact_key_probe as kp
import fp_reference as fpr

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = bytes(range(1, 17))


def name_of(k):
    """an order-preserving renaming of the integers -5 .. 994 to strings: a fixed width, an offset that keeps them >= 0"""
    return b"k%03d" % (int(k) + 5)


def table(rng, n, lo, hi, nulls):
    values = rng.integers(lo, hi, n)
    mask = rng.random(n) >= nulls if nulls else None
    return values, mask, [None if mask is not None and not mask[i] else name_of(v) for i, v in enumerate(values)]


@pytest.mark.parametrize("seed", range(6))
def test_the_walk_agrees_with_the_nested_loop_join_and_with_the_integer_walk(seed):
    rng = np.random.default_rng(seed)
    lv, lm, left = table(rng, 60 + 20 * seed, -5, 25, 0.1 * (seed % 3))
    rv, rm, right = table(rng, 40 + 10 * seed, 0, 30, 0.15 * (seed % 2))
    got = []
    for (near, nv, nm), (far, fv, fm) in (((left, lv, lm), (right, rv, rm)), ((right, rv, rm), (left, lv, lm))):
        records = ex.records_of(far)
        s, p = ex.walk(near, records)
        total, matched, unmatched = ex.nested_loop_left_join(near, far)
        assert (p["join_rows"], p["pairs"]) == (total, matched)
        assert len(unmatched) == s["missing_keys"] + (1 if s["null_rows"] else 0)
        assert set(s["entries"]) == unmatched - {None} and list(s["entries"]) == sorted(s["entries"])
        assert p["parent_rows"] == sum(v is not None for v in far)
        assert p["max_count"] == max(ex.multiplicities(records).values())
        assert s["seen"] == s["non_null"] + s["null_rows"] and s["non_null"] == s["matched"] + s["missing_rows"]
        assert s["missing_rows"] == s["counted"] + s["long_rows"] and s["long_rows"] == 0 and s["route"] == 6
        # the integer walk of the same tables before the renaming: every count, and the entries key by key in order
        si, pi = exi.walk(nv, nm, exi.records_of(fv, fm))
        for f in ("seen", "non_null", "null_rows", "matched", "missing_rows", "counted", "missing_keys", "parent_keys"):
            assert s[f] == si[f], f
        assert list(s["entries"].items()) == [(name_of(k), c) for k, c in si["entries"].items()]
        assert {f: p[f] for f in ("pairs", "join_rows", "parent_rows", "max_count")} == \
            {f: pi[f] for f in ("pairs", "join_rows", "parent_rows", "max_count")}
        got.append(p["pairs"])
    assert got[0] == got[1]  # P is the same number from either side


@pytest.mark.parametrize("seed", range(4))
def test_the_verdicts_are_the_integer_references_under_the_renaming(seed):
    rng = np.random.default_rng(100 + seed)
    lv, lm, left = table(rng, 80, -5, 20, 0.1 * (seed % 2))
    rv, rm, right = table(rng, 50, 0, 25, 0.1 * (seed // 2))
    for kind in (ex.LEFT, ex.RIGHT, ex.BIDIRECTIONAL):
        for distinct in (False, True):
            for expected in (0.0, 0.5, 1.0):
                for examples in (0, 3, 100):
                    assert ex.coverage("l", "r", left, right, kind, distinct, expected, examples) == \
                        exi.coverage("l", "r", lv, lm, rv, rm, kind, distinct, expected, examples)


def test_long_rows_are_missing_rows_whose_keys_are_not_kept():
    child = [b"abcde", b"ab", b"zz", None, b"abcdef", b"abcde"]
    s, p = ex.walk(child, [(b"ab", 2), (b"abcdef", 3), (b"ab", 1)], max_value_bytes=4)
    assert (s["matched"], s["long_rows"], s["counted"], s["missing_rows"]) == (2, 2, 1, 3)
    assert s["entries"] == {b"zz": 1} and s["parent_keys"] == 2
    assert p == {"pairs": 3 + 3, "join_rows": 6 + 3 + 1, "parent_rows": 6, "max_count": 3}
    # the examples read "at least" when a long row was left out and the count is below the cap, as with an overflow
    m = ex.coverage("l", "r", child, [b"ab"], max_value_bytes=4)[2]
    assert m.endswith("(at least 2 unmatched examples found)")
    assert ex.coverage("l", "r", child, [b"ab"], max_value_bytes=6)[2].endswith("(4 unmatched examples found)")
    assert ex.coverage("l", "r", child, [b"ab"], max_examples=2, max_value_bytes=4)[2].endswith("(2 unmatched examples found)")
    assert ex.walk([], [])[0]["route"] == 0 and ex.walk([b"a"], [])[1] == \
        {"pairs": 0, "join_rows": 1, "parent_rows": 0, "max_count": 0}


def test_the_identity_and_the_rows_multiset():
    records = [(b"a", 2), (b"", 2**40), (b"a", 2**32 + 1), (b"x" * 300, 3)]
    ident = ex.identity(KEY, records)
    fa, fb = fpr.fingerprint(KEY, b"a")
    assert ident["parent_keys"] == 3 and ident["parent_rows"] == 2 + 2**40 + 2**32 + 1 + 3 and ident["max_count"] == 2**40
    # the key digest does not see the counts; the count digest is linear in them
    merged = sorted(ex.multiplicities(records).items())
    assert ex.identity(KEY, merged) == ident
    ones = ex.identity(KEY, [(v, 1) for v, _ in merged])
    assert ones["parent_digest"] == ident["parent_digest"] and ones["parent_count_digest"] != ident["parent_count_digest"]
    assert ex.identity(KEY, [(b"a", 5)])["parent_count_digest"] == \
        (5 * kp.mix64(kp.mix64(fa ^ ex.COUNT_SALT) ^ fb)) & ex.M64
    assert ex.identity(KEY, [(b"a", 5)])["parent_digest"] == kp.mix64(kp.mix64(fa ^ kp.DIGEST_SALT) ^ fb)
    assert ex.identity(KEY, []) == {"parent_keys": 0, "parent_digest": 0, "parent_rows": 0, "parent_count_digest": 0,
                                    "max_count": 0}
    # two fingerprints that share hash_a are two keys
    twins = ex.identity_of_fingerprints([((7, 1), 2), ((7, 2), 5), ((7, 1), 1)])
    assert (twins["parent_keys"], twins["parent_rows"], twins["max_count"]) == (2, 8, 5)
    rows = ex.rows_multiset(KEY, [b"a", None, b"", b"a", "a"])
    assert rows == {fpr.fingerprint(KEY, b"a"): 3, fpr.fingerprint(KEY, b""): 1}
    # a set built from a side's rows has the side's multiplicities
    assert ex.identity(KEY, ex.records_of([b"a", None, b"", b"a"])) == \
        ex.identity_of_fingerprints(list(ex.rows_multiset(KEY, [b"a", None, b"", b"a"]).items()))


def golden():
    with open(os.path.join(HERE, "golden", "join_coverage_string_vectors.json")) as f:
        return json.load(f)


def integer_cases():
    with open(os.path.join(HERE, "golden", "join_coverage_vectors.json")) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


@pytest.mark.parametrize("case", golden()["cases"], ids=[c["name"] for c in golden()["cases"]])
def test_the_golden_vectors(case):
    status, metric, message = ex.coverage(case["left_table"], case["right_table"], case["left"], case["right"],
                                          case["coverage_type"], case["distinct_only"], case["expected"],
                                          case.get("max_examples", 100), case.get("max_value_bytes", 256))
    assert status == case["status"]
    if status == "error":
        assert metric is None and case["metric"] is None
        return
    assert message == case["message"] and abs(metric - case["metric"]) <= 1e-12
    # the rate from the literal joins
    lt, lmatched, unmatched = ex.nested_loop_left_join(case["left"], case["right"])
    rt, rmatched, _ = ex.nested_loop_left_join(case["right"], case["left"])
    if case["coverage_type"] == ex.LEFT and case["distinct_only"]:
        lt = len(set(v for v in case["left"] if v is not None))
    rates = {ex.LEFT: [lmatched / lt], ex.RIGHT: [rmatched / rt], ex.BIDIRECTIONAL: [lmatched / lt, rmatched / rt]}
    assert metric == min(rates[case["coverage_type"]])
    # a re-keyed case states what the integer file states
    if "rekeyed_from" in case:
        origin = integer_cases()[case["rekeyed_from"]]
        assert [None if v is None else "k%d" % v for v in origin["left"]] == case["left"]
        assert [None if v is None else "k%d" % v for v in origin["right"]] == case["right"]
        for f in ("status", "metric", "message", "expected", "coverage_type", "distinct_only", "left_table", "right_table"):
            assert case[f] == origin[f], f


def test_every_integer_case_is_rekeyed():
    assert [c.get("rekeyed_from") for c in golden()["cases"]][:len(integer_cases())] == list(integer_cases())
