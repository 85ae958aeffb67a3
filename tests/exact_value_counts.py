"""Exact reference for TGX_CHECK_VALUE_COUNTS and what HistogramConstraint / EntropyAnalyzer derive from it
(TG/constraints/histogram.rs:205-391, TG/analyzers/advanced/entropy.rs:95-163): a plain per-row walk, and a numpy twin of
it.  Nothing here looks at the library.

A column is a list of None (NULL), ints (an integer column: the value is the int64) or bytes (a string column: the
value is the bytes; the empty string is a value).  The walk gives what the library's state holds:

    seen, non_null, distinct, counted, overflow_rows (always 0 here: the walk has no table), long_rows, counts

with counted + overflow_rows + long_rows == non_null.  A string row longer than max_value_bytes is a long row and in
no entry.  The derived figures follow the reference: buckets ordered by count descending, then by the value's TEXT
ascending (the SQL orders CAST(col AS VARCHAR); Python compares str by code point, which is UTF-8 byte order);
ratio = count / (total - nulls); entropies and Gini with `decimal` at 60 digits."""
import decimal
import math

import numpy as np

CTX = decimal.Context(prec=60)
D = decimal.Decimal


# ---- the walk -----------------------------------------------------------------------------------------------------------
def walk(column, max_value_bytes=256):
    seen = non_null = long_rows = 0
    counts = {}
    for v in column:
        seen += 1
        if v is None:
            continue
        non_null += 1
        if isinstance(v, (bytes, bytearray)) and len(v) > max_value_bytes:
            long_rows += 1
            continue
        key = bytes(v) if isinstance(v, (bytes, bytearray)) else int(v)
        counts[key] = counts.get(key, 0) + 1
    return summary(seen, non_null, counts, long_rows)


def summary(seen, non_null, counts, long_rows=0, overflow_rows=0):
    counts = dict(sorted(counts.items()))  # ascending by value: int order, or bytewise
    return {"seen": seen, "non_null": non_null, "distinct": len(counts), "counted": sum(counts.values()),
            "overflow_rows": overflow_rows, "long_rows": long_rows, "counts": counts}


# ---- the numpy twin -------------------------------------------------------------------------------------------------------
def twin_ints(values, valid=None, max_value_bytes=256):
    """values: an integer array; valid: a bool array or None"""
    values = np.asarray(values)
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    kept = values[valid].astype(np.int64)
    uniq, n = np.unique(kept, return_counts=True)
    return summary(len(values), int(valid.sum()), {int(u): int(c) for u, c in zip(uniq, n)})


def twin_bytes(values, valid=None, max_value_bytes=256):
    """values: a list of bytes (whatever stands at a NULL row is not looked at); valid: a bool array or None"""
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    lengths = np.fromiter((len(v) if ok else 0 for v, ok in zip(values, valid)), np.int64, len(values))
    is_long = valid & (lengths > max_value_bytes)
    kept = np.array([v for v, ok, lg in zip(values, valid, is_long) if ok and not lg] + [b""], dtype=object)[:-1]
    uniq, n = np.unique(kept, return_counts=True) if len(kept) else ([], [])
    return summary(len(values), int(valid.sum()), {bytes(u): int(c) for u, c in zip(uniq, n)}, int(is_long.sum()))


# ---- what the constraint and the analyzer derive ----------------------------------------------------------------------------
def value_text(v):
    return v.decode("utf-8") if isinstance(v, (bytes, bytearray)) else str(int(v))


def buckets(state):
    """[(text, count, ratio)] in the SQL's order: count descending, then text ascending"""
    denominator = state["non_null"]  # total - nulls
    rows = sorted(((value_text(v), c) for v, c in state["counts"].items()), key=lambda tc: (-tc[1], tc[0]))
    return [(t, c, c / denominator) for t, c in rows]


def exact_entropy(counts, base=None):
    """-sum p ln p (nats), or in bits with base=2, over the counts' own total, at 60 digits"""
    counts = [c for c in counts if c > 0]
    total = sum(counts)
    if total == 0:
        return D(0)
    h = D(0)
    term = {}  # (p ln p per distinct count: a column of 65536 values has far fewer distinct counts)
    for c in counts:
        if c not in term:
            p = CTX.divide(D(c), D(total))
            term[c] = CTX.multiply(p, CTX.ln(p))
        h = CTX.subtract(h, term[c])
    return CTX.divide(h, CTX.ln(D(2))) if base == 2 else h


def exact_gini(counts):
    total = sum(counts)
    if total == 0:
        return D(0)
    s = D(0)
    for c in counts:
        p = CTX.divide(D(c), D(total))
        s = CTX.add(s, CTX.multiply(p, p))
    return CTX.subtract(D(1), s)


def float_entropy_nats(ratios):
    """Histogram::entropy as the reference evaluates it (histogram.rs:103-109)"""
    return sum(-r * math.log(r) for r in ratios if r > 0.0)


def float_entropy_bits(counts, total):
    """EntropyState::entropy (entropy.rs:97-114)"""
    if total == 0:
        return 0.0
    return sum(-(c / total) * math.log2(c / total) for c in counts if c / total > 0.0)


def float_gini(counts, total):
    """EntropyState::gini_impurity (entropy.rs:132-148)"""
    if total == 0:
        return 0.0
    return 1.0 - sum((c / total) * (c / total) for c in counts)


def tolerance(n_values, h):
    """what a float evaluation of an entropy (or Gini figure) h over n values may be off by: n + 4 roundings of terms of
    size <= h in the sum, and the quotient, logarithm and product of each term (2 units against 1)"""
    return 2.0 ** -52 * ((n_values + 4) * float(h) + 2)
