"""Exact reference for the counted mode of TGX_CHECK_KEY_PROBE and the verdict JoinCoverageConstraint derives from it
(TG/constraints/join_coverage.rs:181-286, 327-421): a plain walk with Python dicts, a numpy twin of it, and a literal
nested-loop outer join to hold both against.  Nothing here looks at the library.

A table side is (values, mask): integer values and a bool array (True: the row is non-NULL; None: every row is).  For
L LEFT JOIN R ON L.l = R.r let m_R(k) be the number of rows of R that hold key k; a NULL never joins.  Then

    matched_left = SUM(CASE WHEN R.r IS NOT NULL ..) = sum over rows of L of m_R(l)            = pairs
    total_left   = COUNT(*) = sum over rows of L of max(1, m_R(l)) = pairs + missing_rows + null_rows = join_rows

A counted set is built from {key, count} records; records of one key add up.  The walk gives the plain walk's summary
(tests/exact_key_probe.py) with the counted routes, and

    pairs, join_rows, parent_rows (the counts' sum), parent_count_digest (the wrapping sum of count * mix64(key ^ salt')
    over the records), max_count (the largest multiplicity of a key)"""
import numpy as np

import exact_key_probe as kp

M64 = kp.M64
COUNT_SALT = 0xC2B2AE3D27D4EB4F
ROUTE_EMPTY, ROUTE_COUNT_ARRAY, ROUTE_COUNT_HASH = 0, 3, 4
LEFT, RIGHT, BIDIRECTIONAL = "left", "right", "bidirectional"


# ---- records ----------------------------------------------------------------------------------------------------------------
def records_of(values, mask=None):
    """one {key, count} record per distinct non-NULL value, ascending: what a DISTINCT export hands out"""
    m = {}
    for i, v in enumerate(values):
        if mask is None or mask[i]:
            m[int(v)] = m.get(int(v), 0) + 1
    return sorted(m.items())


def multiplicities(records):
    """key -> count of the set built from the records (duplicate records add up)"""
    m = {}
    for k, c in records:
        m[int(k)] = m.get(int(k), 0) + int(c)
    return m


def count_digest(records):
    return sum(int(c) * kp.mix64((int(k) & M64) ^ COUNT_SALT) for k, c in records) & M64


def count_digest_np(keys, counts):
    keys = np.asarray(keys, np.int64)
    counts = np.asarray(counts, np.uint64)
    with np.errstate(over="ignore"):
        return int((counts * kp.mix64_np(keys.view(np.uint64) ^ np.uint64(COUNT_SALT))).sum(dtype=np.uint64))


# ---- the route rule -------------------------------------------------------------------------------------------------------
def route_of(keys, n_records=None):
    """keys: the records' keys; empty: 0.  A count array over [min, max] when range = max - min + 1, in unsigned 64-bit
    arithmetic, is not 0 and <= 4 * n_records; else the counted hash table"""
    keys = [int(k) for k in keys]
    n = len(keys) if n_records is None else n_records
    if n == 0:
        return ROUTE_EMPTY
    rng = (max(keys) - min(keys) + 1) & M64
    return ROUTE_COUNT_ARRAY if rng != 0 and rng <= 4 * n else ROUTE_COUNT_HASH


# ---- the walk -------------------------------------------------------------------------------------------------------------
def walk(child, child_mask, records, max_missing_keys=10000):
    """(summary, pairs) of the child column against the counted set of `records` ((key, count) pairs)"""
    m = multiplicities(records)
    seen = non_null = matched = pairs = 0
    entries = {}
    for i, c in enumerate(child):
        seen += 1
        if child_mask is not None and not child_mask[i]:
            continue
        non_null += 1
        times = m.get(int(c), 0)
        if times:
            matched += 1
            pairs += times
        else:
            entries[int(c)] = entries.get(int(c), 0) + 1
    keys = [k for k, _ in records]
    s = kp.summary(seen, non_null, matched, entries, keys, max_missing_keys)
    s["route"] = route_of(keys)
    del s["within_bound"]
    p = {"pairs": pairs, "join_rows": pairs + s["missing_rows"] + s["null_rows"], "parent_rows": sum(m.values()),
         "parent_count_digest": count_digest(records), "max_count": max(m.values()) if m else 0}
    return s, p


def walk_np(child, child_mask, records, max_missing_keys=10000):
    """the numpy twin; the counts of the records must fit int64 sums (the hand-made 2^40 ones do)"""
    child = np.asarray(child).astype(np.int64)
    cm = np.ones(len(child), bool) if child_mask is None else np.asarray(child_mask, bool)
    rk = np.array([k for k, _ in records], np.int64)
    rc = np.array([c for _, c in records], np.uint64)
    uk, inv = np.unique(rk, return_inverse=True)
    mult = np.zeros(len(uk), np.uint64)
    np.add.at(mult, inv, rc)
    kept = child[cm]
    at = np.searchsorted(uk, kept)
    at_c = np.minimum(at, max(len(uk) - 1, 0))
    hit = (uk[at_c] == kept) if len(uk) else np.zeros(len(kept), bool)
    times = np.where(hit, mult[at_c], np.uint64(0)) if len(uk) else np.zeros(len(kept), np.uint64)
    pairs = int(times.astype(object).sum()) if len(times) else 0  # (Python ints: a count may be 2^40)
    uniq, n = np.unique(kept[~hit], return_counts=True)
    counted = int(n.sum())
    s = {"seen": len(child), "non_null": int(cm.sum()), "null_rows": int((~cm).sum()), "matched": int(hit.sum()),
         "missing_rows": counted, "counted": counted, "overflow_rows": 0, "missing_keys": len(uniq),
         "parent_keys": len(uk), "parent_digest": kp.digest_np(rk), "route": route_of(rk.tolist()),
         "entries": {int(u): int(c) for u, c in zip(uniq, n)}}
    p = {"pairs": pairs, "join_rows": pairs + counted + s["null_rows"], "parent_rows": int(rc.sum(dtype=object)),
         "parent_count_digest": count_digest_np(rk, rc), "max_count": int(mult.max()) if len(uk) else 0}
    return s, p


# ---- the literal join -------------------------------------------------------------------------------------------------------
def nested_loop_left_join(left, left_mask, right, right_mask):
    """(COUNT(*), SUM(CASE WHEN R.r IS NOT NULL THEN 1 ELSE 0 END), the distinct L.l of the rows WHERE R.r IS NULL with a
    NULL as None) of L LEFT JOIN R ON L.l = R.r, row pair by row pair"""
    total = matched = 0
    unmatched = set()
    for i, l in enumerate(left):
        l_null = left_mask is not None and not left_mask[i]
        joined = 0
        for j, r in enumerate(right):
            if not l_null and (right_mask is None or right_mask[j]) and int(l) == int(r):
                joined += 1
        if joined:
            total += joined
            matched += joined
        else:
            total += 1
            unmatched.add(None if l_null else int(l))
    return total, matched, unmatched


# ---- the verdict (join_coverage.rs:327-421) ---------------------------------------------------------------------------------
def direction(near, near_mask, far, far_mask):
    """(matched, total, summary) of `near` OUTER JOIN `far`, from near's side"""
    s, p = walk(near, near_mask, records_of(far, far_mask))
    return p["pairs"], p["join_rows"], s


def fmt2(x):
    return "%.2f" % x


def coverage(left_table, right_table, left, left_mask, right, right_mask, coverage_type=LEFT, distinct_only=False,
             expected=1.0, max_examples=100, overflow=False):
    """(status, metric, message) as the reference gives it.  Right: the sides swapped.  distinct_only: total is
    COUNT(DISTINCT L.l) over the left join's rows (Left only; Bidirectional ignores it; with Right it is this
    library's own error, as an empty join is).  The examples are always taken from the left side."""
    expected = min(1.0, max(0.0, expected))
    if coverage_type == RIGHT and distinct_only:
        return "error", None, "distinct_only"
    rates = []
    if coverage_type in (LEFT, BIDIRECTIONAL):
        matched, total, _ = direction(left, left_mask, right, right_mask)
        if coverage_type == LEFT and distinct_only:
            total = len(records_of(left, left_mask))
        rates.append((matched, total))
    if coverage_type in (RIGHT, BIDIRECTIONAL):
        matched, total, _ = direction(right, right_mask, left, left_mask)
        rates.append((matched, total))
    if any(total == 0 for _, total in rates):
        return "error", None, "no rows"
    rate = min(float(m) / float(t) for m, t in rates)
    if rate >= expected:
        return "success", rate, None
    arrow = {LEFT: "->", RIGHT: "<-", BIDIRECTIONAL: "<->"}[coverage_type]
    msg = "Join coverage constraint failed: %s %s %s coverage is %s%% (expected: %s%%)" % (
        left_table, arrow, right_table, fmt2(rate * 100.0), fmt2(expected * 100.0))
    _, _, s = direction(left, left_mask, right, right_mask)
    n = min(max_examples, s["missing_keys"] + (1 if s["null_rows"] > 0 else 0))
    if max_examples > 0 and n > 0:
        msg += " (%s%d unmatched examples found)" % ("at least " if overflow and n < max_examples else "", n)
    return "failure", rate, msg
