"""A plain-Python reference for TGX_CHECK_HISTOGRAM and HistogramAnalyzer (TG/analyzers/advanced/histogram.rs:184-330),
independent of the library and of the oracle: the edges by the reference's formula in Python floats (IEEE doubles, one
rounding per operation), the bucket of a value by walking the literal CASE chain, n / min / max, and the two sums as
exact rationals (tests/exact_moments.py has the pattern).

A column is a list of Python ints / floats with None for NULL.  Every value is CAST AS DOUBLE first (float(v): an
int beyond 2^53 rounds to nearest even, as the device's conversion does)."""
import math
from fractions import Fraction

U = Fraction(1, 2 ** 53)  # unit roundoff of a double


def bucket_width(mn, mx, buckets):
    """histogram.rs:253-258"""
    rng = mx - mn
    return rng / float(buckets) if rng > 0.0 and buckets > 1 else 1.0


def edges_of(mn, mx, buckets):
    """histogram.rs:262-275: lower_i = min + (i as f64 * width); the last upper edge = max + width * 0.001"""
    w = bucket_width(mn, mx, buckets)
    return [mn + (float(i) * w) for i in range(buckets)] + [mx + w * 0.001]


def bucket_of(x, edges):
    """the literal CASE: WHEN c >= lower_i AND c < upper_i THEN i + 1 ... ELSE num_buckets, 0-based here.
    Returns (bucket, came through ELSE)"""
    buckets = len(edges) - 1
    for i in range(buckets):
        if x >= edges[i] and x < edges[i + 1]:
            return i, False
    return buckets - 1, True


def doubles(values):
    """the non-NULL rows CAST AS DOUBLE"""
    return [float(v) for v in values if v is not None]


def exact_sum(ds, power=1):
    """the exact sum of d ** power (power 1 or 2) over finite doubles, as a Fraction: every double is M * 2^e with an
    integer M (math.frexp), and the terms are added as integers at the column's smallest exponent"""
    terms = []
    for d in ds:
        m, e = math.frexp(d)
        terms.append((int(m * 2.0 ** 53) ** power, (e - 53) * power))
    if not terms:
        return Fraction(0)
    e0 = min(e for _, e in terms)
    total = sum(m << (e - e0) for m, e in terms)
    return Fraction(total * 2 ** e0) if e0 >= 0 else Fraction(total, 2 ** -e0)


def value_range(values):
    """the range phase: total, nulls, non_finite, n, min, max (None when n == 0) and the exact sums over the n rows;
    `abs_sum`, `abs_sum_squared`: the sums of the magnitudes of the terms as the device adds them (x, and the ROUNDED
    square x * x), for the error bounds"""
    ds = doubles(values)
    finite = [d for d in ds if math.isfinite(d)]
    squares = [d * d for d in finite]  # rounded once, as SUM(c * c) multiplies before it adds
    return {"total": len(values), "nulls": len(values) - len(ds), "non_finite": len(ds) - len(finite), "n": len(finite),
            "min": min(finite) if finite else None, "max": max(finite) if finite else None,
            "sum": exact_sum(finite), "sum_squared": exact_sum(finite, 2),
            "abs_sum": exact_sum([abs(d) for d in finite]), "abs_sum_squared": exact_sum(squares)}


def sum_bounds(r):
    """|device - exact| for the two sums under ANY summation order of n doubles: gamma_n * sum|term| with
    gamma_n = n u / (1 - n u); for sum_squared the terms are the rounded squares, which are themselves within
    u * x^2 of the exact ones: one more u * sum x^2.  That model of a product holds above the underflow threshold
    only: a square that lands among the subnormals (or at 0) is off by up to half their spacing, 2^-1075, whatever
    x^2 is -- the standard model's additive term, once per row.  (Sums of doubles are exact there: no such term.)"""
    n = r["n"]
    gamma = n * U / (1 - n * U)
    return gamma * r["abs_sum"], gamma * r["abs_sum_squared"] + U * r["sum_squared"] + n * Fraction(1, 2 ** 1075)


def counts_of(values, edges):
    """the count phase: (counts per bucket, else_rows, non_finite).  Long columns walk the same chain one WHEN at a time
    over the whole column (counts_of_columnwise); tests/test_exact_histogram.py holds the two walks together."""
    if len(values) * len(edges) > 200_000:
        return counts_of_columnwise(values, edges)
    counts = [0] * (len(edges) - 1)
    else_rows = non_finite = 0
    for d in doubles(values):
        if not math.isfinite(d):
            non_finite += 1
            continue
        b, through_else = bucket_of(d, edges)
        counts[b] += 1
        else_rows += through_else
    return counts, else_rows, non_finite


def counts_of_columnwise(values, edges):
    """counts_of with the CASE chain evaluated WHEN by WHEN over the column: a row takes the first WHEN that holds"""
    import numpy as np

    d = np.array(doubles(values), dtype=np.float64)
    finite = np.isfinite(d)
    non_finite = int(len(d) - finite.sum())
    d = d[finite]
    buckets = len(edges) - 1
    bucket = np.full(len(d), -1, dtype=np.int64)
    for i in range(buckets):
        hit = (bucket < 0) & (d >= edges[i]) & (d < edges[i + 1])
        bucket[hit] = i
    through_else = bucket < 0
    bucket[through_else] = buckets - 1
    return np.bincount(bucket, minlength=buckets).tolist(), int(through_else.sum()), non_finite


def histogram_state(values, buckets):
    """HistogramState as compute_state_from_data builds it, with the sums as doubles of the exact sums (a device sum is
    held to sum_bounds, not to these)"""
    r = value_range(values)
    if r["n"] == 0:
        return {"buckets": [], "min_value": 0.0, "max_value": 0.0, "total_count": 0, "sum": 0.0, "sum_squared": 0.0}
    edges = edges_of(r["min"], r["max"], buckets)
    counts, _, _ = counts_of(values, edges)
    return {"buckets": [{"lower_bound": edges[i], "upper_bound": edges[i + 1], "count": counts[i]} for i in range(buckets)],
            "min_value": r["min"], "max_value": r["max"], "total_count": r["n"], "sum": float(r["sum"]),
            "sum_squared": float(r["sum_squared"])}
