"""A plain-Python reference for TGX_CHECK_TEMPORAL: Python integers only (no numpy, no library), so nothing can wrap.

The SQL the reference generates (TG/constraints/temporal_ordering.rs) is, for all three modes,

    SELECT COUNT(*) AS total_rows, SUM(CASE WHEN <predicate> THEN 0 ELSE 1 END) AS violations
    FROM t WHERE 1=1 [AND EXTRACT(DOW FROM t) BETWEEN 1 AND 5] [AND <col> IS NOT NULL ...]

and `counts` returns (seen, considered, violations) = (rows of the table, COUNT(*), SUM(..) -- 0 when no row is
considered, where the SQL SUM is NULL and the reference reads 0).

NULL rules, as a truth table.  `null` = the row has a NULL in a column the mode reads (either side in order mode);
`dow` = the row's weekday is Monday .. Friday (only asked under WEEKDAYS_ONLY; NULL for a NULL row, and a WHERE term
that is NULL drops the row).

    KEEP_NULLS  WEEKDAYS_ONLY  null  dow   considered  violation
    ----------  -------------  ----  ----  ----------  -------------------
    no          no             no    -     yes         predicate is false
    no          no             yes   -     no          -                     IS NOT NULL in WHERE: :370-374, :402-406, :439-443
    yes         no             no    -     yes         predicate is false
    yes         no             yes   -     yes         yes                   predicate is NULL -> ELSE 1: :379, :411, :448
    no          yes            no    yes   yes         predicate is false    weekday term in WHERE: :396-400, :413
    no          yes            no    no    no          -
    no          yes            yes   NULL  no          -
    yes         yes            no    yes   yes         predicate is false
    yes         yes            no    no    no          -
    yes         yes            yes   NULL  no          -                     EXTRACT(DOW FROM NULL) BETWEEN .. is NULL

Predicates (include/tgx.h), everything in the column's own ticks:
    ORDER        after - before >= delta
    TIME_OF_DAY  tod_lo <= floormod(t, 86400 * ticks_per_second) <= tod_hi
    RANGE        lo <= t <= hi
"""
import re

ORDER, TIME_OF_DAY, RANGE = 1, 2, 3
KEEP_NULLS, WEEKDAYS_ONLY = 1, 2
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TICKS = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}


def time_of_day(t, ticks_per_second):
    """ticks since the last midnight at or before t (Python's % is a floor modulus)"""
    return t % (86400 * ticks_per_second)


def day_of_week(t, ticks_per_second):
    """SQL's EXTRACT(DOW ..): 0 = Sunday .. 6 = Saturday; 1970-01-01 is a Thursday"""
    return (t // (86400 * ticks_per_second) + 4) % 7


def passes(mode, params, before, after):
    if mode == ORDER:
        return after - before >= params["delta"]
    if mode == TIME_OF_DAY:
        return params["tod_lo"] <= time_of_day(before, params["ticks_per_second"]) <= params["tod_hi"]
    if mode == RANGE:
        return params.get("lo", I64_MIN) <= before <= params.get("hi", I64_MAX)
    raise ValueError(mode)


def counts(mode, params, before, after=None, valid_b=None, valid_a=None):
    """before / after: sequences of Python ints (`after` only in order mode); valid_*: sequences of bools or None (no
    NULLs); params: dict with the mode's fields and "flags".  Returns (seen, considered, violations)."""
    flags = params.get("flags", 0)
    keep, weekdays = bool(flags & KEEP_NULLS), bool(flags & WEEKDAYS_ONLY)
    seen = considered = violations = 0
    for i, b in enumerate(before):
        seen += 1
        null = (valid_b is not None and not valid_b[i]) or (mode == ORDER and valid_a is not None and not valid_a[i])
        if weekdays:
            if null or not 1 <= day_of_week(int(b), params["ticks_per_second"]) <= 5:
                continue
        if null:
            if keep:
                considered += 1
                violations += 1
            continue
        considered += 1
        a = int(after[i]) if mode == ORDER else None
        if not passes(mode, params, int(b), a):
            violations += 1
    return seen, considered, violations


# ---- the host layer's parameter rules, restated --------------------------------------------------------------------
def order_delta(allow_equal, tolerance_seconds, ticks_per_second):
    """temporal_ordering.rs:352-368: allow_equal -> '>' (sic), else '>='; the tolerance only when > 0"""
    tol = tolerance_seconds * ticks_per_second if tolerance_seconds > 0 else 0
    return tol + 1 if allow_equal else tol


def hhmm_ticks(text, ticks_per_second):
    """'HH:MM' + ':00' as ticks into the day"""
    h, m = text.split(":")
    return (int(h) * 3600 + int(m) * 60) * ticks_per_second


_LITERAL = re.compile(r"^(\d{4})-(\d{2})-(\d{2})(?:[ T](\d{2}):(\d{2}):(\d{2})(?:\.(\d{1,9}))?)?(Z)?$")


def days_from_civil(y, m, d):
    """days since 1970-01-01 in the proleptic Gregorian calendar (integer arithmetic only)"""
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def literal_ns(text):
    """TIMESTAMP '<text>' as nanoseconds since the epoch (UTC), or None where the literal is not one of the accepted
    forms: YYYY-MM-DD, YYYY-MM-DD HH:MM:SS[.f{1,9}], the T form, each with no offset or with Z"""
    m = _LITERAL.match(text)
    if not m:
        return None
    y, mo, d = int(m.group(1)), int(m.group(2)), int(m.group(3))
    if m.group(4) is None and m.group(8):
        return None
    hh, mi, ss = (int(m.group(k)) if m.group(k) else 0 for k in (4, 5, 6))
    frac = int((m.group(7) or "").ljust(9, "0") or 0)
    leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
    mdays = [31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
    if not (1 <= mo <= 12 and 1 <= d <= mdays[mo - 1] and hh < 24 and mi < 60 and ss < 60):
        return None
    return (days_from_civil(y, mo, d) * 86400 + hh * 3600 + mi * 60 + ss) * 10**9 + frac


def range_bounds(min_ns, max_ns, ticks_per_second):
    """a nanosecond instant against a coarser column: lo = ceil(min / ns_per_tick), hi = floor(max / ns_per_tick)"""
    per = 10**9 // ticks_per_second
    lo = I64_MIN if min_ns is None else -((-min_ns) // per)
    hi = I64_MAX if max_ns is None else max_ns // per
    return lo, hi


# ---- the verdict (temporal_ordering.rs:521-602) -----------------------------------------------------------------------
MESSAGES = {
    "before_after": "Temporal ordering violation: {v} records where '{a}' is not before '{b}' ({p:.2f}% compliance)",
    "business_hours": "Business hours violation: {v} records with '{a}' outside business hours ({p:.2f}% compliance)",
    "date_range": "Date range violation: {v} records with '{a}' outside valid range ({p:.2f}% compliance)",
}


def verdict(kind, considered, violations, column, column2=None):
    """(status, metric, message)"""
    if violations == 0:
        return "Success", 1.0, None
    rate = (considered - violations) / considered if considered > 0 else 1.0
    return "Failure", rate, MESSAGES[kind].format(v=violations, a=column, b=column2, p=rate * 100.0)


# ---- the same over numpy arrays (the differential tester's tables: 400 000 rows a case) ---------------------------
def counts_np(mode, params, before, after=None, valid_b=None, valid_a=None):
    """counts over numpy int64 columns.  TIME_OF_DAY and RANGE stay in int64 (a floor modulus or floor division by a
    positive day length, and comparisons: nothing can wrap); ORDER subtracts as Python integers, in object arrays, since
    the difference of two Int64 values needs 65 bits.  tests/test_exact_temporal.py holds it to the walk above."""
    import numpy as np

    flags = params.get("flags", 0)
    keep, weekdays = bool(flags & KEEP_NULLS), bool(flags & WEEKDAYS_ONLY)
    t = np.asarray(before, np.int64)
    n = len(t)
    null = np.zeros(n, bool)
    if valid_b is not None:
        null |= ~np.asarray(valid_b, bool)
    if mode == ORDER and valid_a is not None:
        null |= ~np.asarray(valid_a, bool)
    if mode == ORDER:
        ok = (np.asarray(after, np.int64).astype(object) - t.astype(object)) >= params["delta"]
        ok = np.asarray(ok, bool) if n else np.zeros(0, bool)
    elif mode == TIME_OF_DAY:
        tod = np.mod(t, 86400 * params["ticks_per_second"])
        ok = (tod >= params["tod_lo"]) & (tod <= params["tod_hi"])
    elif mode == RANGE:
        ok = (t >= params.get("lo", I64_MIN)) & (t <= params.get("hi", I64_MAX))
    else:
        raise ValueError(mode)
    considered = ~null | keep
    if weekdays:
        dow = np.mod(np.floor_divide(t, 86400 * params["ticks_per_second"]) + 4, 7)
        considered = ~null & (dow >= 1) & (dow <= 5)
    violations = considered & (null | ~ok)
    return n, int(considered.sum()), int(violations.sum())
