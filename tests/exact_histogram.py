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
    square x * x), for the error bounds.  A rounded square may be infinite (1e308 * 1e308): `infinite_squares` counts
    those, and abs_sum_squared runs over the finite ones (exact_sum takes finite doubles only)"""
    ds = doubles(values)
    finite = [d for d in ds if math.isfinite(d)]
    squares = [d * d for d in finite]  # rounded once, as SUM(c * c) multiplies before it adds
    finite_squares = [q for q in squares if math.isfinite(q)]
    return {"total": len(values), "nulls": len(values) - len(ds), "non_finite": len(ds) - len(finite), "n": len(finite),
            "min": min(finite) if finite else None, "max": max(finite) if finite else None,
            "sum": exact_sum(finite), "sum_squared": exact_sum(finite, 2),
            "abs_sum": exact_sum([abs(d) for d in finite]), "abs_sum_squared": exact_sum(finite_squares),
            "infinite_squares": len(squares) - len(finite_squares)}


def sum_bounds(r):
    """|device - exact| for the two sums under ANY summation order of n doubles: gamma_n * sum|term| with
    gamma_n = n u / (1 - n u); for sum_squared the terms are the rounded squares, which are themselves within
    u * x^2 of the exact ones: one more u * sum x^2.  That model of a product holds above the underflow threshold
    only: a square that lands among the subnormals (or at 0) is off by up to half their spacing, 2^-1075, whatever
    x^2 is -- the standard model's additive term, once per row.  (Sums of doubles are exact there: no such term.)"""
    n = r["n"]
    gamma = n * U / (1 - n * U)
    return gamma * r["abs_sum"], gamma * r["abs_sum_squared"] + U * r["sum_squared"] + n * Fraction(1, 2 ** 1075)


OVERFLOW_FROM = Fraction(2) ** 1023


def sum_rules(r):
    """What each of the two sums may be, decided from the exact rationals alone: ((rule, sign) for sum, the same for
    sum_squared), rule one of

      "bound"     the device's double lies within sum_bounds of the exact sum;
      "infinite"  it IS the infinity of that sign;
      "either"    it is the infinity of that sign, or lies within sum_bounds.

    sum_bounds models every addition as fl(a + b) = (a + b)(1 + d), |d| <= u, which holds as long as no addition
    overflows.  Every partial sum of any association of the terms is, in exact arithmetic, at most A = sum |term| in
    magnitude, and as computed at most (1 + gamma_n) A.  With A < 2^1023 that stays below 2^1023 (1 + gamma_n) <
    DBL_MAX for every n a table can have: no association overflows, and the bound holds ("bound").  With A >= 2^1023
    some association may carry a partial sum past DBL_MAX (two rows of 1e308), and an infinity, once there, stays --
    batches, merges, blobs and ranks only add further finite terms or infinities.  An association that stays finite all
    the way is still covered by the bound, so both answers stand ("either"); the infinity has the exact sum's sign, the
    side on which the magnitude lies (and +inf for the squares, which are never negative).
    A rounded square that is itself infinite is a term of sum_squared: the other terms are >= 0 or +inf, and no order
    leads anywhere but +inf ("infinite").  A NaN would need infinities of both signs to meet: it passes no rule."""
    sign = -1.0 if r["sum"] < 0 else 1.0
    rule_sum = ("either", sign) if r["abs_sum"] >= OVERFLOW_FROM else ("bound", sign)
    if r["infinite_squares"]:
        rule_sq = ("infinite", 1.0)
    else:
        rule_sq = ("either", 1.0) if r["abs_sum_squared"] >= OVERFLOW_FROM else ("bound", 1.0)
    return rule_sum, rule_sq


def sum_failure(got, exact, bound, rule):
    """None when the device's double `got` satisfies `rule` (one of sum_rules'), else a line that says why not"""
    kind, sign = rule
    if math.isnan(got):
        return "NaN"
    if math.isinf(got):
        return None if kind != "bound" and got == sign * math.inf else "%r where the rule is %r" % (got, rule)
    if kind == "infinite":
        return "%r where only %r can come out" % (got, sign * math.inf)
    diff = abs(Fraction(got) - exact)
    return None if diff <= bound else "%.17g is %.3g from the exact sum, bound %.3g" % (got, float(diff), float(bound))


# ---- the same over numpy arrays (the differential tester's tables: 400 000 rows a case) ---------------------------
# `d`: the column CAST AS DOUBLE as a float64 array, `valid`: booleans.  tests/test_exact_histogram.py holds each of
# these to the plain walks.
def _segment_sums(terms, exps):
    """{exponent: exact integer sum} of int64 `terms` (|term| < 2^54) grouped by `exps`: in segments of 256 rows at the
    most, whose int64 sums cannot wrap, then in Python integers"""
    import numpy as np

    out = {}
    if len(terms) == 0:
        return out
    order = np.argsort(exps, kind="stable")
    t, e = terms[order], exps[order]
    starts = np.flatnonzero((np.arange(len(t)) % 256 == 0) | np.concatenate([[True], e[1:] != e[:-1]]))
    for s, k in zip(np.add.reduceat(t, starts).tolist(), e[starts].tolist()):
        out[k] = out.get(k, 0) + s
    return out


def exact_sum_np(d, power=1):
    """exact_sum over a float64 array of finite values"""
    import numpy as np

    d = np.asarray(d, np.float64)
    m, e = np.frexp(d)
    big = (m * 2.0 ** 53).astype(np.int64)  # exact: an integer below 2^53 in magnitude
    e = e.astype(np.int64) - 53
    if power == 1:
        parts = _segment_sums(big, e)
    else:  # M = a 2^27 + b, 0 <= b < 2^27, |a| <= 2^26: M^2 = a^2 2^54 + 2ab 2^27 + b^2, each below 2^54 in magnitude
        a, b = big >> 27, big & ((1 << 27) - 1)
        parts = {}
        for terms, shift in ((a * a, 54), (2 * a * b, 27), (b * b, 0)):
            for k, s in _segment_sums(terms, 2 * e + shift).items():
                parts[k] = parts.get(k, 0) + s
    if not parts:
        return Fraction(0)
    e0 = min(parts)
    total = sum(s << (k - e0) for k, s in parts.items())
    return Fraction(total * 2 ** e0) if e0 >= 0 else Fraction(total, 2 ** -e0)


def value_range_np(d, valid):
    """value_range of a column given as (doubles, validity)"""
    import numpy as np

    d = np.asarray(d, np.float64)[np.asarray(valid, bool)]
    finite = d[np.isfinite(d)]
    with np.errstate(over="ignore", under="ignore"):
        squares = finite * finite
    finite_squares = squares[np.isfinite(squares)]
    return {"total": len(valid), "nulls": len(valid) - len(d), "non_finite": len(d) - len(finite), "n": len(finite),
            "min": float(finite.min()) if len(finite) else None, "max": float(finite.max()) if len(finite) else None,
            "sum": exact_sum_np(finite), "sum_squared": exact_sum_np(finite, 2),
            "abs_sum": exact_sum_np(np.abs(finite)), "abs_sum_squared": exact_sum_np(finite_squares),
            "infinite_squares": len(squares) - len(finite_squares)}


def counts_of_np(d, valid, edges):
    """counts_of by binary search.  edges[0 .. buckets-1] are non-decreasing (the rule of tgx_plan_set_histogram_edges),
    so with j the LAST i < buckets whose edges[i] <= x: a WHEN before j fails on x < edges[i+1] <= edges[j]; WHEN j
    holds for j < buckets-1 (edges[j+1] > x by the choice of j) and, for j = buckets-1, iff x < edges[buckets]; no j, or
    that last comparison failing, is ELSE"""
    import numpy as np

    d = np.asarray(d, np.float64)[np.asarray(valid, bool)]
    finite = np.isfinite(d)
    non_finite = int(len(d) - finite.sum())
    d = d[finite]
    buckets = len(edges) - 1
    lower = np.array(edges[:buckets], np.float64)
    assert (lower[1:] >= lower[:-1]).all()
    j = np.searchsorted(lower, d, side="right") - 1
    through_else = (j < 0) | ((j == buckets - 1) & ~(d < edges[buckets]))
    j[through_else] = buckets - 1
    return np.bincount(j, minlength=buckets).tolist(), int(through_else.sum()), non_finite


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
