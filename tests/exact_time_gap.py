"""A plain-Python reference for TGX_CHECK_TIME_GAP: per partition `sorted()`, Python integers only (no numpy, no
library), so nothing can wrap.

The SQL the reference generates for MaxTimeGap (TG/constraints/temporal_ordering.rs:454-481) is a window query,

    WITH gaps AS (SELECT ts - LAG(ts) OVER ([PARTITION BY g] ORDER BY ts) AS gap FROM t WHERE ts IS NOT NULL)
    SELECT COUNT(*), SUM(CASE WHEN gap > max_gap THEN 1 ELSE 0 END) FROM gaps WHERE gap IS NOT NULL

The rules (include/tgx.h), in the timestamp column's own ticks:

    - a row whose timestamp is NULL is seen and otherwise ignored;
    - without a group column the remaining rows form one partition; with one there is a partition per group value, and
      ALL rows whose group is NULL form one partition of their own (SQL's PARTITION BY);
    - within a partition the timestamps are put in non-decreasing order and every row but the first has the gap
      t_i - t_(i-1): an exact, non-negative integer of up to 2^64 - 1 (INT64_MAX - INT64_MIN); equal timestamps give 0;
    - gaps = non-NULL rows - non-empty partitions; violations = gaps with gap > max_gap (a gap EQUAL to max_gap is
      none; a negative max_gap makes every gap one); largest_gap = the maximum gap, 0 when there is none.

`counts` returns (seen, rows, gaps, violations, largest_gap), the fields of tgx_time_gap_counts.  It is the
definition.  `gaps_np` / `counts_np` are its numpy twin for the tables of the differential tester (tests/fuzz_plans.py:
400 000 rows, a task's gaps computed once and shared by its thresholds); tests/test_exact_time_gap.py holds the twin
equal to the plain walk.
"""
import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
TICKS = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}

_NULL_GROUP = object()  # the one partition of all rows whose group is NULL


def partitions(t, valid_t=None, g=None, valid_g=None):
    """{partition key: sorted list of its timestamps} over the rows whose timestamp is not NULL"""
    parts = {}
    for i, ts in enumerate(t):
        if valid_t is not None and not valid_t[i]:
            continue
        if g is None:
            key = None
        elif valid_g is not None and not valid_g[i]:
            key = _NULL_GROUP
        else:
            key = int(g[i])
        parts.setdefault(key, []).append(int(ts))
    return {k: sorted(v) for k, v in parts.items()}


def gaps_of(t, valid_t=None, g=None, valid_g=None):
    """every gap of the table, as Python integers (in no particular order)"""
    out = []
    for stamps in partitions(t, valid_t, g, valid_g).values():
        out.extend(b - a for a, b in zip(stamps, stamps[1:]))
    return out


def counts(max_gap, t, valid_t=None, g=None, valid_g=None):
    """t / g: sequences of Python ints (g: None without a group column); valid_*: sequences of bools or None (no NULLs).
    Returns (seen, rows, gaps, violations, largest_gap)."""
    seen = len(t)
    rows = sum(1 for i in range(seen) if valid_t is None or valid_t[i])
    gaps = gaps_of(t, valid_t, g, valid_g)
    violations = sum(1 for x in gaps if x > max_gap)
    return seen, rows, len(gaps), violations, max(gaps) if gaps else 0


# ---- the numpy twin ---------------------------------------------------------------------------------------------------
def gaps_np(t, valid_t=None, g=None, valid_g=None):
    """(seen, rows, every gap of the table as an ascending uint64 array).  One stable sort puts every partition's rows
    side by side in timestamp order (the NULL group last); a gap is the difference of the neighbours' Int64 bit
    patterns as unsigned 64-bit numbers: t_i >= t_(i-1), so it is the exact difference, up to 2^64 - 1."""
    t = np.asarray(t, np.int64)
    keep = np.ones(len(t), bool) if valid_t is None else np.asarray(valid_t, bool)
    stamps = t[keep]
    if g is None:
        null = np.zeros(len(stamps), bool)
        key = np.zeros(len(stamps), np.int64)
    else:
        null = np.zeros(len(stamps), bool) if valid_g is None else ~np.asarray(valid_g, bool)[keep]
        key = np.where(null, 0, np.asarray(g).astype(np.int64)[keep])  # (a NULL's slot holds anything)
    order = np.lexsort((stamps, key, null))  # stable; the last key is the primary one
    stamps, key, null = stamps[order], key[order], null[order]
    same = (null[1:] == null[:-1]) & (key[1:] == key[:-1])
    with np.errstate(over="ignore"):
        diff = stamps[1:].view(np.uint64) - stamps[:-1].view(np.uint64)
    return len(t), int(keep.sum()), np.sort(diff[same])


def counts_of_gaps(max_gap, seen, rows, gaps):
    """the five counters from gaps_np's answer: one task's gaps serve all its thresholds"""
    if max_gap < 0:
        violations = len(gaps)
    else:
        violations = len(gaps) - int(np.searchsorted(gaps, np.uint64(max_gap), side="right"))
    return seen, rows, len(gaps), violations, int(gaps[-1]) if len(gaps) else 0


def counts_np(max_gap, t, valid_t=None, g=None, valid_g=None):
    """`counts` for numpy columns (t: Int64; g: any integer type that widens to Int64; valid_*: bool arrays or None)"""
    return counts_of_gaps(max_gap, *gaps_np(t, valid_t, g, valid_g))


# ---- the host layer's rules, restated --------------------------------------------------------------------------------
def max_gap_ticks(max_gap_seconds, unit):
    """max_gap_seconds x ticks per second, or None where it does not fit an Int64 (the constraint's evaluation error)"""
    v = max_gap_seconds * TICKS[unit]
    return v if I64_MIN <= v <= I64_MAX else None


MESSAGE = "Time gap violation: {v} gaps exceed maximum allowed ({p:.2f}% compliance)"


def verdict(gaps, violations):
    """(status, metric, message), temporal_ordering.rs:551-601: no violations, or no gaps at all, is a Success with 1.0"""
    if violations == 0:
        return "Success", 1.0, None
    rate = (gaps - violations) / gaps if gaps > 0 else 1.0
    return "Failure", rate, MESSAGE.format(v=violations, p=rate * 100.0)
