"""tests/exact_key_probe_tuples.py against itself: the walk over tuples is held equal to a literal nested-loop outer join
on seeded small tables, so that
    pairs = sum over all-valid rows of L of m_R(l),   join_rows = pairs + missing rows + rows with a NULL component
is tested, not assumed; the numpy twin is held equal to the walk; the NULL rule, the component types and the identity at
their edges; the hand-derived vectors of tests/golden/join_coverage_tuple_vectors.json."""
import json
import os

import numpy as np
import pytest

import exact_key_probe as kp
import exact_key_probe_tuples as ex
import fp_reference as fpr

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = bytes(range(1, 17))
with open(os.path.join(HERE, "golden", "join_coverage_tuple_vectors.json")) as f:
    GOLDEN = json.load(f)


def table(rng, n, arity, keys, nulls):
    """rows of (int, bytes, int, ..) components drawn from `keys` values each"""
    rows = []
    for _ in range(n):
        row = [int(rng.integers(-2, keys)) if c % 2 == 0 else b"s%d" % rng.integers(0, keys) for c in range(arity)]
        for c in range(arity):
            if rng.random() < nulls:
                row[c] = None
        rows.append(tuple(row))
    return rows


def columns_of(rows, arity):
    return [(np.array([0 if r[c] is None else r[c] for r in rows], object), np.array([r[c] is not None for r in rows], bool))
            for c in range(arity)]


@pytest.mark.parametrize("arity", [2, 3, 8])
@pytest.mark.parametrize("seed", range(4))
def test_the_walk_agrees_with_the_nested_loop_join_and_with_its_numpy_twin(seed, arity):
    rng = np.random.default_rng(100 * arity + seed)
    keys = 4 if arity == 2 else 2
    left = table(rng, 60 + 20 * seed, arity, keys, 0.05 * (seed % 3))
    right = table(rng, 40 + 10 * seed, arity, keys, 0.1 * (seed % 2))
    pairs = []
    for near, far in ((left, right), (right, left)):
        records = ex.records_of(far)
        for counted in (False, True):
            s = ex.walk(near, records, KEY, counted)
            assert s == ex.walk_np(columns_of(near, arity), records, KEY, counted)
            assert s["seen"] == s["non_null"] + s["null_rows"] and s["non_null"] == s["matched"] + s["missing_rows"]
            assert s["missing_rows"] == s["counted"] and s["null_rows"] == s["null_counted"]
            assert s["entries"] == sorted(s["entries"]) and s["arity"] == arity
        total, matched, unmatched = ex.nested_loop_left_join(near, far)
        assert (s["join_rows"], s["pairs"]) == (total, matched)
        # SELECT DISTINCT l0, l1 .. WHERE R.r0 IS NULL: the missing tuples and the NULL-bearing ones, each a value
        assert len(unmatched) == s["missing_keys"] + s["null_keys"]
        assert sorted(ex.fingerprint(KEY, t) for t in unmatched) == [e[:2] for e in s["entries"]]
        assert s["parent_rows"] == sum(ex.all_valid(r) for r in far)
        pairs.append(s["pairs"])
    assert pairs[0] == pairs[1]  # the inner join's COUNT(*) is one number from either side


def test_the_null_rule():
    child = [(1, None), (1, 2), (None, None), (1, None)]
    records = [((1, None), 1), ((1, 2), 3), ((None, None), 1)]
    s = ex.walk(child, records, KEY, True)
    assert (s["matched"], s["pairs"], s["null_rows"], s["null_keys"], s["missing_keys"]) == (1, 3, 3, 2, 0)
    assert s["parent_keys"] == 3 and s["join_rows"] == 3 + 3
    assert ex.fingerprint(KEY, (1, None)) + (2, 1) in s["entries"]
    assert not ex.joins((1, None), (1, None)) and ex.joins((1, b"a"), (1, b"a")) and not ex.joins((1, b"1"), (1, 1))


def test_components_are_kept_apart_and_in_order():
    fps = [ex.fingerprint(KEY, t) for t in (("ab", "c"), ("a", "bc"), ("abc", ""), (1, 2), (2, 1), (1, "2"), (1, None),
                                            (None, 1), (1, 2, None), (-1, 2), ((1 << 64) - 1, 2))]
    assert len(set(fps[:-1])) == len(fps) - 1
    assert fps[-2] == fps[-1]  # an int64 -1 and its 64 bits are one component
    assert ex.fingerprint(KEY, (1, b"x")) == fpr.tuple_fingerprint(KEY, [1, b"x"])
    assert ex.fingerprint(KEY, ("x", 1)) != ex.fingerprint(bytes(16), ("x", 1))


def test_the_identity_and_the_records():
    records = [((1, "a"), 2), ((2, "b"), 1 << 40), ((1, "a"), 5), ((3, None), 1)]
    keys, digest, rows, cdigest, most = ex.set_identity(KEY, records, True)
    fps = {ex.fingerprint(KEY, t) for t, _ in records}
    assert keys == 3 == len(fps) and rows == 8 + (1 << 40) and most == 1 << 40
    assert digest == sum(kp.mix64(kp.mix64(a ^ kp.DIGEST_SALT) ^ b) for a, b in fps) & kp.M64
    one = {ex.fingerprint(KEY, (1, "a")): 7, ex.fingerprint(KEY, (2, "b")): 1 << 40, ex.fingerprint(KEY, (3, None)): 1}
    assert cdigest == sum(c * kp.mix64(kp.mix64(a ^ ex.COUNT_SALT) ^ b) for (a, b), c in one.items()) & kp.M64
    assert ex.set_identity(KEY, records, False) == (3, digest, 0, 0, 0)
    assert ex.set_identity(KEY, [], True) == (0, 0, 0, 0, 0)
    rows = [(1, "a"), (None, "a"), (1, "a"), (2, None)]
    assert ex.records_of(rows) == [((1, b"a"), 1), ((1, b"a"), 1)]
    assert ex.record_words(KEY, ex.records_of(rows)) == [ex.fingerprint(KEY, (1, "a")) + (1, 0)] * 2


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=lambda c: c["name"])
def test_golden_vectors(case):
    """hand-derived: the counts are stated in the file, not computed here"""
    left = [tuple(r) for r in case["left"]]
    right = [tuple(r) for r in case["right"]]
    near, far = (left, right) if case["side"] == "left" else (right, left)
    s = ex.walk(near, ex.records_of(far), KEY, True)
    for f, v in case["state"].items():
        assert s[f] == v, f
    total, matched, unmatched = ex.nested_loop_left_join(near, far)
    assert (total, matched, len(unmatched)) == (case["state"]["join_rows"], case["state"]["pairs"], case["examples"])
    assert abs((matched / total if total else 1.0) - case["rate"]) < 1e-12
