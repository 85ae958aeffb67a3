"""tests/exact_key_probe_strings.py against a twin written another way (numpy object arrays and Counter), and the
hand-written reference expectations of tests/golden/foreign_key_string_vectors.json against the exact walk."""
import collections
import json
import os

import numpy as np
import pytest

import exact_key_probe_strings as ex

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "foreign_key_string_vectors.json")) as f:
    GOLDEN = json.load(f)


def twin(child, parent, max_value_bytes=256):
    """the same state from numpy masks and a Counter"""
    child, parent = ex.as_bytes(child), ex.as_bytes(parent)
    c = np.array(child + [None], dtype=object)[:-1]
    null = np.array([v is None for v in c], bool)
    keys = frozenset(v for v in parent if v is not None)
    hit = np.array([v in keys for v in c], bool) & ~null
    too_long = np.array([v is not None and len(v) > max_value_bytes for v in c], bool) & ~hit
    counts = collections.Counter(v for v, skip in zip(c, null | hit | too_long) if not skip)
    entries = {k: counts[k] for k in sorted(counts)}
    return {"seen": len(c), "non_null": int((~null).sum()), "null_rows": int(null.sum()), "matched": int(hit.sum()),
            "missing_rows": int((~null & ~hit).sum()), "counted": sum(entries.values()), "overflow_rows": 0,
            "long_rows": int(too_long.sum()), "missing_keys": len(entries), "parent_keys": len(keys), "entries": entries}


def random_side(rng, n, alphabet, null_rate):
    lengths = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 300]
    out = []
    for _ in range(n):
        if rng.random() < null_rate:
            out.append(None)
        else:
            size = lengths[int(rng.integers(0, len(lengths)))]
            out.append(bytes(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size)))
    return out


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("max_value_bytes", [1, 16, 256])
def test_the_walk_and_its_twin_agree(seed, max_value_bytes):
    rng = np.random.default_rng(seed)
    child = random_side(rng, 400, b"ab", [0.0, 0.5, 1.0][seed % 3])
    parent = random_side(rng, 60, b"ab", 0.2)
    want = ex.walk(child, parent, max_value_bytes)
    del want["within_bound"]
    got = twin(child, parent, max_value_bytes)
    assert got == want and list(got["entries"]) == list(want["entries"])
    assert want["seen"] == want["non_null"] + want["null_rows"]
    assert want["non_null"] == want["matched"] + want["missing_rows"]
    assert want["missing_rows"] == want["counted"] + want["overflow_rows"] + want["long_rows"]


def as_codes(child):
    """(codes, words, mask) of a list of bytes / None: the words in order of first appearance"""
    words, at, codes = [], {}, []
    for v in ex.as_bytes(child):
        if v is not None and v not in at:
            at[v] = len(words)
            words.append(v)
        codes.append(0 if v is None else at[v])
    return np.array(codes, np.int64), words or [b"unused"], np.array([v is not None for v in child], bool)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("max_value_bytes", [1, 16, 256])
def test_the_walk_and_its_numpy_twin_agree_on_a_seeded_table_with_long_rows(seed, max_value_bytes):
    rng = np.random.default_rng(100 + seed)
    child = random_side(rng, 400, b"ab", [0.0, 0.5, 1.0][seed % 3])
    parent = random_side(rng, 60, b"ab", 0.2) + [v for v in child if v is not None][:5]
    want = ex.walk(child, parent, max_value_bytes)
    got = ex.walk_np(*as_codes(child), parent, max_value_bytes)
    assert got == want and list(got["entries"]) == list(want["entries"])
    assert seed % 3 == 2 or max_value_bytes == 256 or want["long_rows"] > 0
    # a word no row holds (or only NULL rows point at) is no entry
    codes, words, mask = as_codes(child)
    assert ex.walk_np(codes, words + [b"never"], mask, parent, max_value_bytes) == want


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_the_numpy_twin_on_the_golden_cases(case):
    got, want = ex.walk_np(*as_codes(case["child"]), case["parent"]), ex.walk(case["child"], case["parent"])
    assert got == want and list(got["entries"]) == list(want["entries"])


def test_the_parent_digest_is_over_distinct_fingerprints():
    import exact_key_probe as kp
    import fp_reference as fpr

    key = bytes(range(1, 17))
    assert ex.parent_digest(key, []) == ex.parent_digest(key, [None]) == 0
    fa, fb = fpr.fingerprint(key, b"a")
    assert ex.parent_digest(key, ["a", b"a", None]) == kp.mix64(kp.mix64(fa ^ kp.DIGEST_SALT) ^ fb)
    assert ex.parent_digest(key, ["a", "b"]) == (ex.parent_digest(key, ["a"]) + ex.parent_digest(key, ["b"])) & kp.M64
    assert ex.parent_digest(bytes(16), ["a"]) != ex.parent_digest(key, ["a"])


def test_the_order_is_bytewise_and_a_long_value_in_the_parent_is_matched():
    long_value = b"x" * 300
    s = ex.walk([b"b", b"\xc3\xa9", b"a", b"", b"ab", long_value, long_value + b"y", None], [long_value], 256)
    assert list(s["entries"]) == [b"", b"a", b"ab", b"b", b"\xc3\xa9"]
    assert (s["matched"], s["long_rows"], s["null_rows"], s["missing_rows"]) == (1, 1, 1, 6)
    # exactly max_value_bytes is kept, one byte more is a long row
    s = ex.walk([b"12345678", b"123456789"], [], 8)
    assert s["entries"] == {b"12345678": 1} and s["long_rows"] == 1


def test_the_verdict_says_at_least_when_rows_were_not_kept():
    s = ex.walk(["a", "bbbb"], [], 2)
    assert ex.verdict(s, "c.x", "p.y")[2] == ("Foreign key constraint violation: 2 values in 'c.x' do not exist in 'p.y' "
                                              "(total: 2, unique: at least 1). Examples: [a]")
    s["overflow_rows"], s["long_rows"] = 1, 0
    assert "unique: at least 1" in ex.verdict(s, "c.x", "p.y")[2]


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_the_golden_cases_are_what_the_exact_walk_gives(case):
    assert "cannot be run here" in GOLDEN["header"]
    state = ex.walk(case["child"], case["parent"])
    status, metric, message = ex.verdict(state, GOLDEN["child_column"], GOLDEN["parent_column"],
                                         allow_nulls=case["options"].get("allow_nulls", False),
                                         max_violations_reported=case["options"].get("max_violations_reported", 100))
    assert (status, metric, message) == (case["status"], case["metric"], case["message"])


def test_the_golden_cases_cover_what_they_should():
    names = {c["name"] for c in GOLDEN["cases"]}
    assert {"clean", "missing keys", "NULLs are violations", "NULLs allowed", "the empty string is a key",
            "more than five missing keys", "more missing keys than max_violations_reported", "an empty parent"} <= names
