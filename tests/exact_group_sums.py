"""Sums per group, exactly: SELECT g, COUNT(*) AS rows, COUNT(col) AS non_null, SUM(col) AS sum FROM t GROUP BY g as a plain
dictionary walk over Python lists, the NULL key a group as in SQL -- what TGX_CHECK_GROUP_SUMS answers for one value column
and one group column -- and on top of it the reference's CrossTableSumConstraint
(TG/constraints/cross_table_sum.rs:185-284, :572-630): the full outer join of the two sides' groups and the verdict.

Integer sums are DataFusion's: 64-bit, wrapping, so they are kept modulo 2^64 and read as signed.  Float sums have no one
value -- the device adds in whatever order -- so a float group keeps two exact references instead: math.fsum of its values
(the correctly rounded sum) and the sum of their magnitudes, from which float_bound() gives what ANY order or tree of
IEEE additions may differ from the exact sum by."""
import math

M64 = (1 << 64) - 1


def wrap(x):
    """an integer modulo 2^64, read as Int64"""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def group_by(values, groups):
    """{key: [rows, the non-NULL values]}; the key is None for a NULL; insertion order = first occurrence"""
    out = {}
    for v, g in zip(values, groups):
        c = out.setdefault(g, [0, []])
        c[0] += 1
        if v is not None:
            c[1].append(v)
    return out


def int_class(rows, vals):
    return (rows, len(vals), wrap(sum(vals)))


def float_class(rows, vals):
    """(rows, non_null, fsum, sum of magnitudes); a NaN or opposite infinities make fsum NaN, as IEEE addition does"""
    try:
        exact = math.fsum(vals)
    except (ValueError, OverflowError):  # (inf - inf; an intermediate overflow cannot happen at the tests' magnitudes)
        exact = math.nan
    return (rows, len(vals), exact, math.fsum(abs(v) for v in vals) if vals else 0.0)


def walk(values, groups, max_value_bytes=256, is_float=False):
    """what TGX_CHECK_GROUP_SUMS answers when nothing overflows: seen, groups, is_float, the four classes and `entries`,
    key -> class, ascending by key.  A class is (rows, non_null, sum) for integer values and (rows, non_null, fsum,
    sum of magnitudes) for floats.  A key is an int or bytes; bytes longer than max_value_bytes are long rows"""
    cls = float_class if is_float else int_class
    nothing = cls(0, [])
    s = dict(seen=len(values), is_float=bool(is_float) and len(values) > 0, null_group=nothing, overflow=nothing)
    entries, longs = {}, [0, []]
    for key, (rows, vals) in group_by(values, groups).items():
        if key is None:
            s["null_group"] = cls(rows, vals)
        elif isinstance(key, bytes) and len(key) > max_value_bytes:
            longs[0] += rows
            longs[1] += vals
        else:
            entries[key] = cls(rows, vals)
    s["long_rows"] = cls(*longs)
    # (ascending by key: integers numerically, bytes bytewise with a prefix first)
    s["entries"] = {k: entries[k] for k in sorted(entries)}
    s["groups"] = len(entries)
    if is_float:
        s["counted"] = (sum(e[0] for e in entries.values()), sum(e[1] for e in entries.values()))
    else:
        s["counted"] = (sum(e[0] for e in entries.values()), sum(e[1] for e in entries.values()),
                        wrap(sum(e[2] for e in entries.values())))
    return s


def float_bound(non_null, exact, magnitudes):
    """how far a double sum of m values, added in ANY order or tree, may lie from math.fsum of them: the m - 1 additions
    each round once, so the computed sum differs from the true sum S by at most gamma_{m-1} * sum|x| (Higham, Accuracy
    and Stability of Numerical Algorithms, section 4.2), and fsum from S by at most 2^-53 * |fsum|"""
    u = 2.0 ** -53
    k = max(non_null - 1, 0)
    return k * u / (1 - k * u) * magnitudes + u * abs(exact)


# ---- the constraint -------------------------------------------------------------------------------------------------------
def parse_qualified(name):
    """cross_table_sum.rs:158-175: exactly one dot"""
    parts = name.split(".")
    if len(parts) != 2:
        raise ValueError("Column must be qualified (table.column): '%s'" % name)
    return parts[0], parts[1]


def side_sums(values, groups=None, is_float=False):
    """one side: {key: COALESCE(SUM(col), 0.0) as a double}; an integer sum is cast AFTER the wrapping Int64 sum
    (:251-262; the reader downcasts to Float64Array, :536-570).  groups None: the ungrouped form, a single float"""
    def total(vals):
        if not vals:
            return 0.0
        return float_class(0, vals)[2] if is_float else float(wrap(sum(vals)))
    if groups is None:
        return total([v for v in values if v is not None])
    return {k: total(vals) for k, (_rows, vals) in group_by(values, groups).items()}


def fixed4(x):
    """Rust's {:.4}"""
    if x != x:
        return "NaN"
    if x in (math.inf, -math.inf):
        return "inf" if x > 0 else "-inf"
    return "%.4f" % x


def rust_f64(x):
    """Rust's {} for an f64: the shortest digits that round-trip, never an exponent, no trailing .0"""
    if x != x:
        return "NaN"
    if x in (math.inf, -math.inf):
        return "inf" if x > 0 else "-inf"
    from decimal import Decimal
    text = format(Decimal(repr(x)), "f")  # (repr: the shortest digits; beyond them Rust prints zeros, as this does)
    return text[:-2] if text.endswith(".0") else text


def cross_table_sum(left, right, tolerance=0.0, group_by_columns=(), left_name="orders.total", right_name="payments.amount",
                    max_violations_reported=100):
    """the reference's result row and verdict.  left / right: side_sums() of each table -- dicts for the grouped form,
    floats for the ungrouped one.  The full outer join is on l.g = r.g, so a key on one side only is a group against 0.0
    and NULL keys never join: each side's NULL group is a group of its own against 0.0.  The totals add the groups in
    ascending key order, the NULL groups last (the left one first).  NaN > tolerance is false, as in SQL; a NaN
    difference makes max_difference NaN.  Both tables empty, grouped: COUNT(*) = 0 and NULL aggregates whose slots
    read 0 through .value(0): success with metric 0.0"""
    tolerance = abs(tolerance)
    if isinstance(left, dict):
        keys = sorted(set(k for k in left if k is not None) | set(k for k in right if k is not None))
        rows = [(left.get(k, 0.0), right.get(k, 0.0)) for k in keys]
        if None in left:
            rows.append((left[None], 0.0))
        if None in right:
            rows.append((0.0, right[None]))
    else:
        rows = [(left, right)]
    out = dict(total_groups=len(rows), violating_groups=0, total_left_sum=0.0, total_right_sum=0.0, max_difference=0.0)
    for l, r in rows:
        diff = abs(l - r)
        out["violating_groups"] += diff > tolerance
        out["total_left_sum"] += l
        out["total_right_sum"] += r
        if diff != diff or (out["max_difference"] == out["max_difference"] and diff > out["max_difference"]):
            out["max_difference"] = diff
    out["metric"] = out["max_difference"]
    if out["violating_groups"] == 0:
        return dict(out, status="success", message=None)
    tol = " (tolerance: %s)" % fixed4(tolerance) if tolerance > 0.0 else " (exact match required)"
    grouping = "groups by [%s]" % ", ".join(group_by_columns) if group_by_columns else "overall totals"
    head = "Cross-table sum mismatch: %d/%d %s failed validation%s" % (out["violating_groups"], out["total_groups"],
                                                                         grouping, tol)
    if not group_by_columns and max_violations_reported > 0:  # (:409-413: examples for the ungrouped form only)
        l, r = rows[0]
        message = "%s. Examples: [Group 'ALL': %s = %s, %s = %s (diff: %s)]" % (head, left_name, fixed4(l), right_name,
                                                                                   fixed4(r), fixed4(abs(l - r)))
    else:
        message = "%s, total sums: %s vs %s (max diff: %s)" % (head, rust_f64(out["total_left_sum"]),
                                                               rust_f64(out["total_right_sum"]), fixed4(out["max_difference"]))
    return dict(out, status="failure", message=message)
