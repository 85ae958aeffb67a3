"""tests/exact_value_rule.py held against itself and against the reference's own tests: the numpy twin equals the literal
walk on seeded tables with every special value in them, the hand-worked rows of include/tgx.h come out as stated, and
the vectors of tests/golden/datatype_vectors.json (datatype.rs:473-623, transcribed as data) go through the walk.  No
device, no library: tests/test_value_rule_host.py and tests/test_gpu_value_rule.py hold the library against this module."""
import json
import math
import os

import numpy as np
import pytest

import exact_value_rule as ev

NAN_POS, NAN_NEG = 0x7FF8000000000000, -0x0008000000000000
NAN_PAYLOAD, NAN_NEG_PAYLOAD = 0x7FF0000000000123, -0x0010000000000000 + 0x123
INT_SPECIALS = [ev.I64_MIN, ev.I64_MIN + 1, -2**53 - 1, -2**53, -2**31 - 1, -2**31, -1, 0, 1, 2**31 - 1, 2**31, 2**53,
                2**53 + 1, 2**53 + 2, ev.I64_MAX - 1, ev.I64_MAX]
FLOAT_SPECIALS = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, float("inf"), -float("inf"), NAN_POS, NAN_NEG,
                  NAN_PAYLOAD, NAN_NEG_PAYLOAD, 0.5, -0.5, 2.0, 2.5, -2147483648.9, -2147483649.0, 2147483647.5,
                  2147483648.0, 2147483647.0, -2147483648.0, 1e300, -1e300, 2.0 ** 53, 2.0 ** 63, -(2.0 ** 63)]
RULES = [ev.rule(ev.GE_ZERO), ev.rule(ev.GT_ZERO), ev.rule(ev.INTEGER), ev.rule(ev.BETWEEN, 0, -5, 5, -5.0, 5.0),
         ev.rule(ev.BETWEEN, 0, 5, -5, 5.0, -5.0), ev.rule(ev.BETWEEN, 0, 2**53, 2**53, 2.0 ** 53, 2.0 ** 53),
         ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, 2.0 ** 53, 2.0 ** 53),
         ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, -0.0, 0.0), ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, 0.0, 0.0),
         ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, -0.5, 2.0 ** 31 + 0.5),
         ev.rule(ev.BETWEEN, 0, ev.I64_MIN, ev.I64_MAX, -float("inf"), float("inf")),
         ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, ev.float_of(NAN_NEG), ev.float_of(NAN_POS))]


def f64(values):
    return np.array([v if isinstance(v, int) else ev.bits_of(v) for v in values], np.int64).view(np.float64)


def int_table(seed, n):
    rng = np.random.default_rng(seed)
    v = rng.integers(-10, 10, n, dtype=np.int64)
    far = rng.random(n) < 0.3
    v[far] = rng.integers(-2**62, 2**62, int(far.sum()), dtype=np.int64) >> rng.integers(0, 62, int(far.sum()))
    at = rng.choice(n, len(INT_SPECIALS), replace=False)
    v[at] = np.array(INT_SPECIALS, np.int64)
    return v, rng.random(n) >= 0.15


def float_table(seed, n):
    rng = np.random.default_rng(seed)
    v = np.round(rng.standard_normal(n) * 4, 1)
    whole = rng.random(n) < 0.4
    v[whole] = np.trunc(v[whole] * 1e9)
    at = rng.choice(n, len(FLOAT_SPECIALS), replace=False)
    v[at] = f64(FLOAT_SPECIALS)
    return v, rng.random(n) >= 0.15


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_twin_equals_the_walk(seed):
    n = 4000
    for v, m in (int_table(seed, n), float_table(seed, n)):
        is_float = v.dtype == np.float64
        rows = v.view(np.int64).tolist()
        for r in RULES:
            for mask in (None, m):
                walked = ev.counts(r, rows, None if mask is None else mask.tolist(), is_float)
                assert ev.counts_np(r, v, mask) == walked, (r, is_float)
                assert walked[0] == n and walked[2] + walked[3] <= walked[1] <= walked[0]


def test_total_order_keys():
    """-NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN, and key(+0.0) is 0"""
    ordered = [NAN_NEG, NAN_NEG_PAYLOAD, -float("inf"), -1e300, -2.5, -5e-324, -0.0, 0.0, 5e-324, 2.5, 1e300, float("inf"),
               NAN_PAYLOAD, NAN_POS]
    keys = [ev.key(v if isinstance(v, int) else ev.bits_of(v)) for v in ordered]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert ev.KEY_ZERO == 0 and ev.key(ev.bits_of(-0.0)) == -1
    assert all(ev.I64_MIN <= k <= ev.I64_MAX for k in keys)
    for b in (0, 1, -1, ev.I64_MIN, ev.I64_MAX, NAN_NEG):  # the formula of include/tgx.h on two's-complement words
        word = b & (2**64 - 1)
        formula = word ^ ((2**64 - 1 if word >> 63 else 0) & 0x7FFFFFFFFFFFFFFF)
        assert ev.key(b) == formula - (1 << 64 if formula >> 63 else 0)


def judged(mode, value, **kw):
    is_float = not isinstance(value, int) or kw.pop("pattern", False)
    v = value if isinstance(value, int) else ev.bits_of(value)
    return ev.judge(ev.rule(mode, **kw), v, is_float)


def test_the_rows_the_header_states():
    P = dict(pattern=True)
    # GE_ZERO / GT_ZERO on floats: -0.0 fails both, +0.0 passes GE only, +NaN passes both, -NaN fails both
    assert [judged(ev.GE_ZERO, x)[0] for x in (-0.0, 0.0)] == [False, True]
    assert [judged(ev.GT_ZERO, x)[0] for x in (-0.0, 0.0, 5e-324)] == [False, False, True]
    assert judged(ev.GE_ZERO, NAN_POS, **P)[0] and judged(ev.GT_ZERO, NAN_POS, **P)[0]
    assert not judged(ev.GE_ZERO, NAN_NEG, **P)[0] and not judged(ev.GT_ZERO, NAN_NEG, **P)[0]
    assert [judged(ev.GE_ZERO, v)[0] for v in (-1, 0, 1)] == [False, True, True]
    assert [judged(ev.GT_ZERO, v)[0] for v in (-1, 0, 1)] == [False, False, True]
    # INTEGER: 2.0 is valid, 2.5 is not, -0.0 is not; num-traits' range rule
    assert judged(ev.INTEGER, 2.0) == (True, False) and judged(ev.INTEGER, 2.5) == (False, False)
    assert judged(ev.INTEGER, -0.0) == (False, False) and judged(ev.INTEGER, 0.0) == (True, False)
    assert judged(ev.INTEGER, -2147483648.9) == (False, False) and judged(ev.INTEGER, -2147483649.0) == (False, True)
    assert judged(ev.INTEGER, 2147483647.5) == (False, False) and judged(ev.INTEGER, 2147483648.0) == (False, True)
    assert judged(ev.INTEGER, -2147483648.0) == (True, False) and judged(ev.INTEGER, 2147483647.0) == (True, False)
    for x in (float("inf"), -float("inf"), 1e300):
        assert judged(ev.INTEGER, x) == (False, True)
    assert judged(ev.INTEGER, NAN_POS, **P) == (False, True) and judged(ev.INTEGER, NAN_NEG_PAYLOAD, **P) == (False, True)
    assert [judged(ev.INTEGER, v) for v in (-2**31 - 1, -2**31, 2**31 - 1, 2**31)] == \
        [(False, True), (True, False), (True, False), (False, True)]
    # BETWEEN: int64 bounds compare as integers; double bounds see CAST(col AS DOUBLE), which rounds 2^53 + 1 to 2^53
    assert not judged(ev.BETWEEN, 2**53 + 1, lo_i=2**53, hi_i=2**53)[0]
    assert judged(ev.BETWEEN, 2**53 + 1, flags=ev.BOUNDS_AS_DOUBLE, lo_f=2.0 ** 53, hi_f=2.0 ** 53)[0]
    assert not judged(ev.BETWEEN, 2**53 + 2, flags=ev.BOUNDS_AS_DOUBLE, lo_f=2.0 ** 53, hi_f=2.0 ** 53)[0]
    assert not judged(ev.BETWEEN, 3, lo_i=5, hi_i=1)[0] and not judged(ev.BETWEEN, 3.0, lo_f=5.0, hi_f=1.0)[0]
    # lo_f = -0.0 against +0.0 data, and the other way round
    assert judged(ev.BETWEEN, 0.0, lo_f=-0.0, hi_f=1.0)[0] and not judged(ev.BETWEEN, -0.0, lo_f=0.0, hi_f=1.0)[0]
    assert judged(ev.BETWEEN, 0, flags=ev.BOUNDS_AS_DOUBLE, lo_f=-0.0, hi_f=0.0)[0]
    assert float(2**53 + 1) == 2.0 ** 53 and float(2**53 + 3) == 2.0 ** 53 + 4  # (float(int): nearest-even)


def test_null_rows_are_seen_and_never_considered():
    rows = [5, -5, 2**40, 5, -5, 2**40]
    valid = [True] * 3 + [False] * 3
    assert ev.counts(ev.rule(ev.GE_ZERO), rows, valid) == (6, 3, 2, 0)
    assert ev.counts(ev.rule(ev.INTEGER), rows, valid) == (6, 3, 2, 1)
    assert ev.counts(ev.rule(ev.INTEGER), rows, [False] * 6) == (6, 0, 0, 0)
    assert ev.counts(ev.rule(ev.GT_ZERO), [], None) == (0, 0, 0, 0)


def test_widening_keeps_what_the_rules_read():
    raw = np.array([0x7FC00000, 0xFFC00000, 0x80000000, 0, 0x3F000000, 0x40000000], np.uint32).view(np.float32)
    wide = ev.widen(raw, "float32")
    rows = wide.view(np.int64).tolist()
    assert [ev.judge(ev.rule(ev.GE_ZERO), v, True)[0] for v in rows] == [True, False, False, True, True, True]
    assert [ev.judge(ev.rule(ev.INTEGER), v, True) for v in rows[2:]] == [(False, False), (True, False), (False, False), (True, False)]
    u32 = np.array([0, 2**31 - 1, 2**31, 2**32 - 1], np.uint32)
    assert ev.counts_np(ev.rule(ev.INTEGER), ev.widen(u32, "uint32")) == (4, 4, 2, 2)
    assert ev.widen(np.array([-128, 127], np.int8), "int8").tolist() == [-128, 127]


def test_bound_classification_and_texts():
    assert ev.classify_bound(2.0 ** 53) == ("int", 2**53) and ev.classify_bound(-(2.0 ** 53)) == ("int", -2**53)
    assert ev.classify_bound(2.0 ** 53 + 2)[0] == "error" and ev.classify_bound(1e300)[0] == "error"
    assert ev.classify_bound(0.5) == ("float", 0.5) and ev.classify_bound(-0.0) == ("int", 0)
    assert ev.classify_bound(float("inf"))[0] == "error" and ev.classify_bound(float("nan"))[0] == "error"
    assert ev.range_params(0.0, 100.0) == ev.rule(ev.BETWEEN, 0, 0, 100, 0.0, 100.0)
    assert ev.range_params(1.0, 2.5) == ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, 1.0, 2.5)
    assert ev.range_params(0.0, float("inf")) is None
    assert ev.rust_f64(0.0) == "0" and ev.rust_f64(-0.0) == "-0" and ev.rust_f64(100.0) == "100"
    assert ev.rust_f64(0.5) == "0.5" and ev.rust_f64(1e-7) == "0.0000001" and ev.rust_f64(1e21) == "1" + "0" * 21
    assert ev.description("range", min=0.0, max=100.0) == "values between 0 and 100"
    assert ev.verdict(4, 4, "x") == ("Success", 1.0, None)
    assert ev.verdict(4, 3, "non-negative values") == ("Failure", 0.75, "75.0% of values satisfy non-negative values")
    status, metric, message = ev.verdict(0, 0, "non-negative values")
    assert status == "Failure" and math.isnan(metric) and message == "NaN% of values satisfy non-negative values"


def test_the_references_own_tests_through_the_walk():
    """datatype.rs:473-623.  The numeric cases go through `counts`; the NotEmpty case (a mode that stays off the device)
    through the same COUNT / SUM(CASE ..) shape with LENGTH(col) > 0 as its predicate"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datatype_vectors.json")) as f:
        golden = json.load(f)
    assert len(golden["cases"]) == 6
    seen_kinds = set()
    for case in golden["cases"]:
        col = case["table"][case["column"]]
        v = case["validation"]
        seen_kinds.add(v["kind"])
        values = col["values"]
        valid = [x is not None for x in values]
        if v["kind"] == "specific_type":
            status, metric = ("Success", 1.0) if col["type"] == v["type"] else ("Failure", 0.0)
        elif v["kind"] == "string_not_empty":
            considered = sum(valid)
            status, metric, _ = ev.verdict(considered, sum(1 for x in values if x), "non-empty strings")
        else:
            assert col["type"] == "Float64" and case["on_device"]
            r = ev.rule(ev.GE_ZERO) if v["kind"] == "non_negative" else ev.range_params(v["min"], v["max"])
            rows = [ev.bits_of(float(x)) if x is not None else 0 for x in values]
            seen, considered, ok, errors = ev.counts(r, rows, valid, True)
            assert seen == len(values) and errors == 0
            text = ev.description(v["kind"], **{k: v[k] for k in ("min", "max") if k in v})
            status, metric, _ = ev.verdict(considered, ok, text)
        assert status == case["status"], case["source"]
        if "metric" in case:
            assert metric == case["metric"]
        if "metric_below" in case:
            assert metric < case["metric_below"]
        if "metric_near" in case:
            assert abs(metric - case["metric_near"]) < case["metric_within"] and metric == 0.75
    assert seen_kinds == {"specific_type", "non_negative", "range", "string_not_empty"}
