"""Exact reference for a TGX_CHECK_KEY_PROBE spec on TUPLE keys (Plan.set_key_probe_tuples, _tuples_counted,
_rows_tuples): a composite join key, the device side of the reference's JoinCoverageConstraint::on_multiple
(TG/constraints/join_coverage.rs:127-138, the join condition at :192-197).  A literal nested-loop outer join over Python
tuples decides every count; nothing here looks at the library.  Fingerprints come in only where the library's answer is
DEFINED over them -- the set's identity, the gathered records and the entries, which keep no bytes -- and are restated with
tests/fp_reference.py's tuple_fingerprint under a fixed key.

A table side is a list of rows; a row is a tuple whose components are None (NULL), an int (an integer column's value,
taken modulo 2^64: the sign- or zero-extended int64) or bytes / str (a string column's value, whatever its layout).

The SQL NULL rule: L.l0 = R.r0 AND L.l1 = R.r1 .. is never true where a component is NULL, so a row with a NULL
component matches nothing -- a parent tuple with a NULL in the same place included.  For L LEFT JOIN R with m_R(t) the
rows of R that hold the all-valid tuple t:

    pairs     = sum over all-valid rows of L of m_R(l)             SUM(CASE WHEN R.r0 IS NOT NULL ..)
    join_rows = pairs + missing_rows + null_rows                   COUNT(*)

`non_null` counts the rows whose every component is non-NULL and null_rows the others; the three identities of the
single-column probe hold over the all-valid rows.  The rows with a NULL component are counted per distinct tuple too (the
reference's examples query is SELECT DISTINCT l0, l1 .. WHERE R.r0 IS NULL, where such a tuple is a value of its own):
null_counted, null_keys, and entries (hash_a, hash_b, count, has_null) ascending by (hash_a, hash_b), both classes
together.

A set is built from (tuple, count) records; records of one tuple add up.  A record whose tuple holds a NULL can be
hand-made (a rows spec gathers none): it is a key of the set's identity and still matches nothing."""
import exact_key_probe as kp
import fp_reference as fpr

M64 = kp.M64
COUNT_SALT = 0xC2B2AE3D27D4EB4F
ROUTE_EMPTY, ROUTE_PLAIN, ROUTE_COUNTED = 0, 5, 6


def as_tuple(row):
    """components normalised: None, an int in [0, 2^64), or bytes"""
    return tuple(None if c is None else (c & M64) if isinstance(c, int) else (c.encode() if isinstance(c, str) else bytes(c))
                 for c in row)


def all_valid(row):
    return all(c is not None for c in row)


def joins(l, r):
    """L.l0 = R.r0 AND L.l1 = R.r1 ..: never with a NULL, never an integer with a string"""
    return len(l) == len(r) and all(a is not None and b is not None and type(a) is type(b) and a == b for a, b in zip(l, r))


def fingerprint(key, row):
    return fpr.tuple_fingerprint(key, list(as_tuple(row)))


# ---- the literal join -------------------------------------------------------------------------------------------------------
def nested_loop_left_join(left, right):
    """(COUNT(*), SUM(CASE WHEN R.r0 IS NOT NULL THEN 1 ELSE 0 END), the distinct rows of L WHERE R.r0 IS NULL) of
    L LEFT JOIN R ON every component pair, row pair by row pair"""
    total = matched = 0
    unmatched = set()
    left, right = [as_tuple(l) for l in left], [as_tuple(r) for r in right]
    for l in left:
        joined = sum(1 for r in right if joins(l, r))
        total += max(1, joined)
        matched += joined
        if not joined:
            unmatched.add(l)
    return total, matched, unmatched


# ---- records ----------------------------------------------------------------------------------------------------------------
def records_of(rows):
    """one (tuple, 1) record per all-valid row: what a rows tuples spec gathers"""
    return [(as_tuple(r), 1) for r in rows if all_valid(r)]


def record_words(key, records):
    """the 32-byte {hash_a, hash_b, count, 0} records as rows of four integers"""
    return [fingerprint(key, t) + (c, 0) for t, c in records]


def set_identity(key, records, counted):
    """(parent_keys, parent_digest, parent_rows, parent_count_digest, max_count): over the DISTINCT fingerprints of the
    records; the last three of a counted set only"""
    counts = {}
    for t, c in records:
        fp = fingerprint(key, t)
        counts[fp] = counts.get(fp, 0) + c
    digest = sum(kp.mix64(kp.mix64(fa ^ kp.DIGEST_SALT) ^ fb) for fa, fb in counts) & M64
    if not counted:
        return len(counts), digest, 0, 0, 0
    cdigest = sum(c * kp.mix64(kp.mix64(fa ^ COUNT_SALT) ^ fb) for (fa, fb), c in counts.items()) & M64
    return len(counts), digest, sum(counts.values()), cdigest, max(counts.values(), default=0)


# ---- the walk ---------------------------------------------------------------------------------------------------------------
def walk(child, records, key, counted=False):
    """the state of a tuples spec that has seen the rows of `child` under the set built from `records`
    ((tuple, count) pairs): the join is decided row pair by row pair, record by record"""
    child = [as_tuple(r) for r in child]
    records = [(as_tuple(t), c) for t, c in records]
    arity = len(child[0]) if child else (len(records[0][0]) if records else 0)
    seen = non_null = matched = pairs = 0
    missing, with_null = {}, {}
    for l in child:
        seen += 1
        if not all_valid(l):
            with_null[l] = with_null.get(l, 0) + 1
            continue
        non_null += 1
        times = sum(c for t, c in records if joins(l, t))  # (the nested loop: the records are the parent's rows)
        if times:
            matched += 1
            pairs += times
        else:
            missing[l] = missing.get(l, 0) + 1
    entries = sorted([fingerprint(key, t) + (n, 0) for t, n in missing.items()] +
                     [fingerprint(key, t) + (n, 1) for t, n in with_null.items()])
    parent_keys, digest, parent_rows, cdigest, max_count = set_identity(key, records, counted)
    counted_rows, null_counted = sum(missing.values()), sum(with_null.values())
    state = {"seen": seen, "non_null": non_null, "null_rows": seen - non_null, "matched": matched,
             "missing_rows": counted_rows, "counted": counted_rows, "overflow_rows": 0, "missing_keys": len(missing),
             "parent_keys": parent_keys, "parent_digest": digest,
             "route": 0 if not parent_keys else ROUTE_COUNTED if counted else ROUTE_PLAIN,
             "null_counted": null_counted, "null_overflow_rows": 0, "null_keys": len(with_null), "arity": arity,
             "entries": entries}
    if counted:
        state.update(pairs=pairs, join_rows=pairs + counted_rows + (seen - non_null), parent_rows=parent_rows,
                     parent_count_digest=cdigest, max_count=max_count)
    return state


def walk_np(child_columns, records, key, counted=False):
    """numpy twin of walk.  child_columns: one (values, mask) per component -- values an int64 / uint64 array, or an
    object array / list of bytes; mask a bool array, True where the row is non-NULL.  Rows are grouped with np.unique
    over per-component codes, the multiplicities come from one dict lookup per DISTINCT tuple"""
    import numpy as np

    n = len(child_columns[0][1]) if child_columns else 0
    arity = len(child_columns)
    codes, words = [], []
    for values, mask in child_columns:
        mask = np.asarray(mask, bool)
        vals = [None if not m else v for v, m in zip(list(values), mask)]
        norm = [as_tuple((v if v is None or not isinstance(v, np.integer) else int(v),))[0] for v in vals]
        distinct = sorted(set(x for x in norm if x is not None), key=lambda x: (isinstance(x, bytes), x))
        at = {x: i + 1 for i, x in enumerate(distinct)}
        codes.append(np.array([0 if x is None else at[x] for x in norm], np.int64))  # (0: NULL)
        words.append([None] + distinct)
    m = {}
    for t, c in records:
        t = as_tuple(t)
        m[t] = m.get(t, 0) + c
    if n:
        stacked = np.stack(codes, axis=1)
        groups, per_group = np.unique(stacked, axis=0, return_counts=True)
    else:
        groups, per_group = np.zeros((0, arity), np.int64), np.zeros(0, np.int64)
    valid = (groups != 0).all(axis=1) if len(groups) else np.zeros(0, bool)
    tuples = [tuple(words[c][g[c]] for c in range(arity)) for g in groups]
    times = np.array([m.get(t, 0) if v else 0 for t, v in zip(tuples, valid)], np.int64).reshape(-1)
    hit = valid & (times > 0)
    miss = valid & (times == 0)
    entries = sorted([fingerprint(key, tuples[g]) + (int(per_group[g]), 0) for g in np.flatnonzero(miss)] +
                     [fingerprint(key, tuples[g]) + (int(per_group[g]), 1) for g in np.flatnonzero(~valid)])
    non_null, matched = int(per_group[valid].sum()), int(per_group[hit].sum())
    counted_rows, null_counted = int(per_group[miss].sum()), int(per_group[~valid].sum())
    pairs = int(sum(int(per_group[g]) * int(times[g]) for g in np.flatnonzero(hit)))
    parent_keys, digest, parent_rows, cdigest, max_count = set_identity(key, [(t, c) for t, c in records], counted)
    state = {"seen": n, "non_null": non_null, "null_rows": n - non_null, "matched": matched,
             "missing_rows": counted_rows, "counted": counted_rows, "overflow_rows": 0, "missing_keys": int(miss.sum()),
             "parent_keys": parent_keys, "parent_digest": digest,
             "route": 0 if not parent_keys else ROUTE_COUNTED if counted else ROUTE_PLAIN,
             "null_counted": null_counted, "null_overflow_rows": 0, "null_keys": int((~valid).sum()) if len(groups) else 0,
             "arity": arity if n else (len(as_tuple(records[0][0])) if records else 0), "entries": entries}
    if counted:
        state.update(pairs=pairs, join_rows=pairs + counted_rows + (n - non_null), parent_rows=parent_rows,
                     parent_count_digest=cdigest, max_count=max_count)
    return state


# ---- JoinCoverageConstraint over composite keys (TG/constraints/join_coverage.rs:181-286, 289-324, 327-421) ---------------
LEFT, RIGHT, BIDIRECTIONAL = "left", "right", "bidirectional"
ARROWS = {LEFT: "->", RIGHT: "<-", BIDIRECTIONAL: "<->"}


def coverage_verdict(left_table, right_table, left, right, expected, coverage_type=LEFT, distinct_only=False,
                     max_examples=100):
    """(status, metric, message) from the literal joins.  rate = matched / total of L LEFT JOIN R (Right: the sides
    swapped; Bidirectional: the lesser of the two, distinct_only ignored); distinct_only with Left replaces the total by
    COUNT(DISTINCT l0), the first left key alone, under the same numerator.  The examples are always the left side's:
    the distinct rows of L without a partner, a tuple with a NULL component being a value of its own"""
    rates = []
    if coverage_type != RIGHT:
        total, matched, _ = nested_loop_left_join(left, right)
        if coverage_type == LEFT and distinct_only:
            total = len(set(as_tuple(l)[0] for l in left) - {None})
        rates.append(matched / total)
    if coverage_type != LEFT:
        total, matched, _ = nested_loop_left_join(right, left)
        rates.append(matched / total)
    rate = min(rates)
    if rate >= expected:
        return "success", rate, None
    message = "Join coverage constraint failed: %s %s %s coverage is %.2f%% (expected: %.2f%%)" % (
        left_table, ARROWS[coverage_type], right_table, rate * 100.0, expected * 100.0)
    found = min(max_examples, len(nested_loop_left_join(left, right)[2]))
    if found:
        message += " (%d unmatched examples found)" % found
    return "failure", rate, message
