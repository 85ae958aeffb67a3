"""tests/exact_temporal.py held against an independent origin: Python's datetime for the time of day, the weekday and
the TIMESTAMP literals.  No device, no library: tests/test_temporal_host.py and tests/test_gpu_temporal.py hold the
library against this module."""
import datetime as dt
import random

import pytest

import exact_temporal as et

EPOCH = dt.datetime(1970, 1, 1)


def instant(t, tps):
    """(datetime at the second at or before tick t, ticks into that second)"""
    whole, frac = divmod(t, tps)  # (floor: Python integers)
    return EPOCH + dt.timedelta(seconds=whole), frac


def instants(tps, seed):
    rng = random.Random(seed)
    day = 86400 * tps
    # datetime covers years 1 .. 9999; nanosecond ticks in an int64 cover 1677 .. 2262
    span = min(et.I64_MAX // tps, 200 * 365 * 86400)
    out = [rng.randrange(-span * tps, span * tps) for _ in range(4000)]
    for d in [rng.randrange(-span // 86400, span // 86400) for _ in range(300)] + [-1, 0, 1]:
        out += [d * day - 1, d * day, d * day + 1]
    return out


@pytest.mark.parametrize("unit", ["s", "ms", "us", "ns"])
def test_time_of_day_and_weekday_against_datetime(unit):
    tps = et.TICKS[unit]
    ts = instants(tps, 11 + tps)
    assert any(t < 0 for t in ts)
    for t in ts:
        when, frac = instant(t, tps)
        tod = (when.hour * 3600 + when.minute * 60 + when.second) * tps + frac
        assert et.time_of_day(t, tps) == tod, t
        assert et.day_of_week(t, tps) == when.isoweekday() % 7, t  # (isoweekday: Monday 1 .. Sunday 7; DOW: Sunday 0)


def test_cxx_style_remainders_would_differ():
    """what the floor forms are for: one second before the epoch is 23:59:59 on a Wednesday"""
    assert et.time_of_day(-1, 1) == 86399 and et.day_of_week(-1, 1) == 3
    assert et.time_of_day(-86400, 1) == 0 and et.day_of_week(-86400, 1) == 3
    assert et.day_of_week(0, 1) == 4


def test_literals_against_fromisoformat():
    rng = random.Random(5)
    for _ in range(3000):
        when = EPOCH + dt.timedelta(seconds=rng.randrange(-250 * 365 * 86400, 250 * 365 * 86400))
        digits = rng.randrange(0, 10)
        frac = "".join(rng.choice("0123456789") for _ in range(digits))
        for sep in (" ", "T"):
            text = when.strftime("%Y-%m-%d") + sep + when.strftime("%H:%M:%S") + ("." + frac if frac else "")
            parsed = dt.datetime.fromisoformat(when.strftime("%Y-%m-%d %H:%M:%S"))
            want = ((parsed - EPOCH) // dt.timedelta(seconds=1)) * 10**9 + int(frac.ljust(9, "0") or 0)
            assert et.literal_ns(text) == want, text
            assert et.literal_ns(text + "Z") == want
        date = when.strftime("%Y-%m-%d")
        assert et.literal_ns(date) == ((dt.datetime.fromisoformat(date) - EPOCH) // dt.timedelta(seconds=1)) * 10**9
    for bad in ("", "2024", "2024-13-01", "2024-02-30", "2023-02-29", "2024-01-01 24:00:00", "2024-01-01 10:00",
                "2024-01-01 10:00:00+01:00", "2024-01-01Z", "2024-01-01 10:00:00.", "2024-01-01 10:00:00.1234567890",
                "01/02/2024", " 2024-01-01"):
        assert et.literal_ns(bad) is None, bad
    assert et.literal_ns("2024-02-29") is not None and et.literal_ns("1900-02-29") is None


def test_range_bounds_round_inwards():
    assert et.range_bounds(1_000_000_000, 1_000_000_000, 1) == (1, 1)
    assert et.range_bounds(1_000_000_001, 1_999_999_999, 1) == (2, 1)   # nothing in between at second resolution
    assert et.range_bounds(999_999_999, 1_000_000_001, 1) == (1, 1)
    assert et.range_bounds(-1, -1, 1000) == (0, -1)
    assert et.range_bounds(-1_000_000, -1_000_000, 1000) == (-1, -1)
    assert et.range_bounds(5, 7, 10**9) == (5, 7)
    assert et.range_bounds(None, None, 1) == (et.I64_MIN, et.I64_MAX)


def test_null_truth_table():
    """the docstring's table, row by row: Thursday and Saturday, noon (inside 09:00-17:00) and 01:00 (outside)"""
    noon, night, saturday = 12 * 3600, 3600, 2 * 86400
    tod = {"ticks_per_second": 1, "tod_lo": 9 * 3600, "tod_hi": 17 * 3600}
    rows = [(noon, True), (night, True), (saturday + noon, True), (saturday + night, True), (noon, False),
            (saturday + noon, False)]
    ts, valid = [r[0] for r in rows], [r[1] for r in rows]
    assert et.counts(et.TIME_OF_DAY, dict(tod, flags=0), ts, None, valid) == (6, 4, 2)
    assert et.counts(et.TIME_OF_DAY, dict(tod, flags=et.KEEP_NULLS), ts, None, valid) == (6, 6, 4)
    assert et.counts(et.TIME_OF_DAY, dict(tod, flags=et.WEEKDAYS_ONLY), ts, None, valid) == (6, 2, 1)
    assert et.counts(et.TIME_OF_DAY, dict(tod, flags=et.WEEKDAYS_ONLY | et.KEEP_NULLS), ts, None, valid) == (6, 2, 1)
    assert et.counts(et.ORDER, {"delta": 0}, [0, 0, 0, 5], [1, 1, 1, 0], [True, False, True, True],
                     [True, True, False, True]) == (4, 2, 1)
    assert et.counts(et.ORDER, {"delta": 0, "flags": et.KEEP_NULLS}, [0, 0, 0, 5], [1, 1, 1, 0],
                     [True, False, True, True], [True, True, False, True]) == (4, 4, 3)
    assert et.counts(et.RANGE, {"lo": 0}, [], None) == (0, 0, 0)


def test_order_delta_keeps_the_inverted_comparison():
    """temporal_ordering.rs:352-368: allow_equal picks '>', the default picks '>='; a tolerance <= 0 is ignored"""
    assert et.order_delta(False, 0, 10**9) == 0 and et.order_delta(True, 0, 10**9) == 1
    assert et.order_delta(False, 60, 10**6) == 60 * 10**6 and et.order_delta(True, 60, 10**6) == 60 * 10**6 + 1
    assert et.order_delta(False, -5, 1) == 0 and et.order_delta(True, -5, 1) == 1


def test_verdict_formatting():
    assert et.verdict("before_after", 2, 0, "a", "b") == ("Success", 1.0, None)
    assert et.verdict("date_range", 0, 0, "t") == ("Success", 1.0, None)
    s, m, msg = et.verdict("before_after", 2, 1, "created_at", "processed_at")
    assert (s, m) == ("Failure", 0.5)
    assert msg == ("Temporal ordering violation: 1 records where 'created_at' is not before 'processed_at' "
                   "(50.00% compliance)")
    assert et.verdict("business_hours", 4, 4, "t")[2].endswith("(0.00% compliance)")
    assert et.verdict("date_range", 20000, 1, "t")[2].endswith("(100.00% compliance)")  # 99.995 % rounds up


def test_reference_unit_tests_as_data():
    """tests/golden/temporal_ordering_vectors.json: the reference's two evaluated tables through counts + verdict"""
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_ordering_vectors.json")) as f:
        golden = json.load(f)
    for case in golden["evaluated"]:
        before_col, after_col = case["builder"]["before_after"]
        before = [et.literal_ns(r[before_col]) for r in case["rows"]]
        after = [et.literal_ns(r[after_col]) for r in case["rows"]]
        delta = et.order_delta(False, 0, 10**9)
        seen, considered, violations = et.counts(et.ORDER, {"delta": delta}, before, after)
        status, metric, message = et.verdict("before_after", considered, violations, before_col, after_col)
        assert status == case["status"] and (message is not None) == case["message_is_some"], case["source"]
        assert seen == considered == 2


# ---- the numpy fast path of the differential tester, against the plain walk -------------------------------------------
def test_numpy_counts_equal_the_walk():
    import numpy as np

    for n in (0, 1, 9, 3000):
        rng = np.random.default_rng(n)
        for make in (lambda: rng.integers(-2**62, 2**62, n), lambda: rng.integers(-10**6, 10**6, n),
                     lambda: rng.integers(-2 * 10**18, 2 * 10**18, n)):
            b, a = make(), make()
            if n > 2:
                b[0], a[0], b[1], a[1] = et.I64_MIN, et.I64_MAX, et.I64_MAX, et.I64_MIN
            vb, va = rng.random(n) >= 0.2, rng.random(n) >= 0.2
            for delta in (0, 1, -1, 2**39 + 5, et.I64_MAX, et.I64_MIN):
                for flags in (0, et.KEEP_NULLS):
                    p = dict(delta=delta, flags=flags)
                    assert et.counts_np(et.ORDER, p, b, a, vb, va) == et.counts(et.ORDER, p, b.tolist(), a.tolist(), vb.tolist(), va.tolist())
            for tps in et.TICKS.values():
                for flags in (0, 1, 2, 3):
                    p = dict(ticks_per_second=tps, tod_lo=3 * tps, tod_hi=50_000 * tps, flags=flags)
                    assert et.counts_np(et.TIME_OF_DAY, p, b, None, vb) == et.counts(et.TIME_OF_DAY, p, b.tolist(), None, vb.tolist())
            for p in (dict(), dict(lo=-5, flags=1), dict(hi=10**5), dict(lo=-(2**61), hi=2**61, flags=1)):
                assert et.counts_np(et.RANGE, p, b, None, vb) == et.counts(et.RANGE, p, b.tolist(), None, vb.tolist())
            assert et.counts_np(et.RANGE, dict(lo=0), b) == et.counts(et.RANGE, dict(lo=0), b.tolist())
