"""Exact reference for the counted mode of TGX_CHECK_KEY_PROBE on STRING keys (Plan.set_key_probe_strings_counted), for
the records a rows strings spec gathers (Plan.set_key_probe_rows_strings) and for the verdict JoinCoverageConstraint
derives from them on string columns (TG/constraints/join_coverage.rs:181-286, 327-421): a literal nested-loop outer join
and a plain walk over Python `bytes` with dicts.  Nothing here looks at the library, and no fingerprint decides a count:
the walk compares the values themselves, which is what the library's counts are exact over unless two values share all
128 bits of a keyed fingerprint.  (The exceptions are the set's identity and the gathered records, which are DEFINED
over fingerprints: they are restated here with tests/fp_reference.py.)

A table side is a list whose items are `bytes` (or str, taken as UTF-8) or None for a NULL row; a NULL never joins.  For
L LEFT JOIN R ON L.l = R.r let m_R(v) be the number of rows of R that hold v.  Then

    matched_left = SUM(CASE WHEN R.r IS NOT NULL ..) = sum over rows of L of m_R(l)                      = pairs
    total_left   = COUNT(*) = sum over rows of L of max(1, m_R(l)) = pairs + missing_rows + null_rows    = join_rows

A counted set is built from (value, count) records; records of one value add up.  The walk gives the strings walk's
summary (tests/exact_key_probe_strings.py: a missing row whose value is longer than max_value_bytes is a long row, which
is a missing row whose key is not kept) with route 6 (0: the empty set), and

    pairs, join_rows, parent_rows (the counts' sum), max_count (the largest multiplicity of a value)"""
import exact_key_probe as kp
import exact_key_probe_strings as ks

M64 = kp.M64
COUNT_SALT = 0xC2B2AE3D27D4EB4F
ROUTE_EMPTY, ROUTE_STRINGS_COUNTED = 0, 6
LEFT, RIGHT, BIDIRECTIONAL = "left", "right", "bidirectional"
as_bytes = ks.as_bytes


# ---- the literal join -------------------------------------------------------------------------------------------------------
def nested_loop_left_join(left, right):
    """(COUNT(*), SUM(CASE WHEN R.r IS NOT NULL THEN 1 ELSE 0 END), the distinct L.l of the rows WHERE R.r IS NULL with a
    NULL as None) of L LEFT JOIN R ON L.l = R.r, row pair by row pair"""
    total = matched = 0
    unmatched = set()
    left, right = as_bytes(left), as_bytes(right)
    for l in left:
        joined = 0
        for r in right:
            if l is not None and r is not None and l == r:
                joined += 1
        if joined:
            total += joined
            matched += joined
        else:
            total += 1
            unmatched.add(l)
    return total, matched, unmatched


# ---- records ----------------------------------------------------------------------------------------------------------------
def records_of(values):
    """one (value, 1) record per non-NULL row: what a rows strings spec gathers from a plain string layout"""
    return [(v, 1) for v in as_bytes(values) if v is not None]


def multiplicities(records):
    """value -> count of the set built from the records (duplicate records add up)"""
    m = {}
    for v, c in records:
        m[v] = m.get(v, 0) + int(c)
    return m


# ---- the counted walk -------------------------------------------------------------------------------------------------------
def walk(child, records, max_value_bytes=256, max_missing_keys=10000):
    """(summary, pairs) of the child column against the counted set of `records` ((value, count) pairs)"""
    m = multiplicities([(as_bytes([v])[0], c) for v, c in records])
    s = ks.walk(child, list(m), max_value_bytes, max_missing_keys)
    del s["within_bound"]
    s["route"] = ROUTE_STRINGS_COUNTED if m else ROUTE_EMPTY
    pairs = sum(m.get(v, 0) for v in as_bytes(child) if v is not None)
    p = {"pairs": pairs, "join_rows": pairs + s["missing_rows"] + s["null_rows"], "parent_rows": sum(m.values()),
         "max_count": max(m.values()) if m else 0}
    return s, p


# ---- what is defined over fingerprints ----------------------------------------------------------------------------------------
def digest_term(fa, fb, salt):
    return kp.mix64(kp.mix64(fa ^ salt) ^ fb)


def identity_of_fingerprints(records):
    """the identity of the set built from ((fa, fb), count) records: parent_keys, parent_digest -- the wrapping sum over
    the distinct fingerprints of mix64(mix64(fa ^ 0x9e37..) ^ fb) --, parent_rows, parent_count_digest -- the wrapping sum
    over the distinct fingerprints of count * mix64(mix64(fa ^ 0xc2b2..) ^ fb) -- and max_count"""
    m = {}
    for fp, c in records:
        m[fp] = m.get(fp, 0) + int(c)
    return {"parent_keys": len(m),
            "parent_digest": sum(digest_term(fa, fb, kp.DIGEST_SALT) for fa, fb in m) & M64,
            "parent_rows": sum(m.values()),
            "parent_count_digest": sum(c * digest_term(fa, fb, COUNT_SALT) for (fa, fb), c in m.items()) & M64,
            "max_count": max(m.values()) if m else 0}


def identity(key, records):
    """... of (value, count) records under the 16-byte fingerprint key `key`"""
    import fp_reference as fpr

    return identity_of_fingerprints([(fpr.fingerprint(key, as_bytes([v])[0]), c) for v, c in records])


def rows_multiset(key, values):
    """(fa, fb) -> the sum of the counts of its records, for the records a rows strings spec gathers from `values`: a
    record a non-NULL row for a plain layout, a record an entry and batch for a dictionary -- the sums are the same"""
    import fp_reference as fpr

    m = {}
    for v in as_bytes(values):
        if v is not None:
            fp = fpr.fingerprint(key, v)
            m[fp] = m.get(fp, 0) + 1
    return m


# ---- the verdict (join_coverage.rs:327-421) ---------------------------------------------------------------------------------
def direction(near, far, max_value_bytes=256):
    """(matched, total, summary) of `near` OUTER JOIN `far`, from near's side"""
    s, p = walk(near, records_of(far), max_value_bytes)
    return p["pairs"], p["join_rows"], s


def coverage(left_table, right_table, left, right, coverage_type=LEFT, distinct_only=False, expected=1.0,
             max_examples=100, max_value_bytes=256, overflow=False):
    """(status, metric, message) as the reference gives it.  Right: the sides swapped.  distinct_only: total is
    COUNT(DISTINCT L.l) over the left join's rows (Left only; Bidirectional ignores it; with Right it is this library's
    own error, as an empty join is).  The examples are always taken from the left side: its distinct values without a
    partner, a NULL counting once; a missing value longer than max_value_bytes is not kept, so the number then reads
    "at least" (when it is below max_examples)."""
    expected = min(1.0, max(0.0, expected))
    if coverage_type == RIGHT and distinct_only:
        return "error", None, "distinct_only"
    rates = []
    if coverage_type in (LEFT, BIDIRECTIONAL):
        matched, total, _ = direction(left, right)
        if coverage_type == LEFT and distinct_only:
            total = len(set(v for v in as_bytes(left) if v is not None))
        rates.append((matched, total))
    if coverage_type in (RIGHT, BIDIRECTIONAL):
        matched, total, _ = direction(right, left)
        rates.append((matched, total))
    if any(total == 0 for _, total in rates):
        return "error", None, "no rows"
    rate = min(float(m) / float(t) for m, t in rates)
    if rate >= expected:
        return "success", rate, None
    arrow = {LEFT: "->", RIGHT: "<-", BIDIRECTIONAL: "<->"}[coverage_type]
    msg = "Join coverage constraint failed: %s %s %s coverage is %.2f%% (expected: %.2f%%)" % (
        left_table, arrow, right_table, rate * 100.0, expected * 100.0)
    _, _, s = direction(left, right, max_value_bytes)
    n = min(max_examples, s["missing_keys"] + (1 if s["null_rows"] > 0 else 0))
    if max_examples > 0 and n > 0:
        partial = overflow or s["long_rows"] > 0
        msg += " (%s%d unmatched examples found)" % ("at least " if partial and n < max_examples else "", n)
    return "failure", rate, msg
