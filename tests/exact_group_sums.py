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
    except (ValueError, OverflowError):  # (inf - inf, or partial sums beyond DBL_MAX: float_rule decides such a group)
        exact = math.nan
    return (rows, len(vals), exact, magnitudes_of(vals))


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


def magnitudes_of(vals):
    """math.fsum of the magnitudes; inf where an infinity is among them or the exact sum lies beyond DBL_MAX (fsum raises
    OverflowError there), NaN with a NaN"""
    try:
        return math.fsum(abs(v) for v in vals) if len(vals) else 0.0
    except OverflowError:
        return math.inf


def float_rule(vals):
    """how a float group's sum is decided, in the manner of exact_histogram.sum_rules.  ("bound", None): finite values
    whose magnitudes add up to a finite number -- no order of additions overflows, float_bound holds.  Otherwise, by IEEE
    addition in any order or tree:
      - a NaN among the values gives NaN: ("is", nan);
      - infinities of both signs give NaN: ("is", nan);
      - infinities of ONE sign give that infinity, provided the finite values cannot overflow on their own (their
        magnitudes add up to a finite number; an overflow to the other infinity would meet this one as NaN):
        ("is", +-inf);
      - finite values whose magnitudes add up beyond DBL_MAX (with or without an infinity beside them) overflow in some
        orders and not in others: ("unpinned", None).  The group's rows and non_null stay pinned.
    vals: the group's non-NULL values"""
    pos = neg = False
    for v in vals:
        if v != v:
            return ("is", math.nan)
        pos |= v == math.inf
        neg |= v == -math.inf
    if pos and neg:
        return ("is", math.nan)
    if not math.isfinite(magnitudes_of([v for v in vals if math.isfinite(v)])):
        return ("unpinned", None)
    if pos or neg:
        return ("is", math.inf if pos else -math.inf)
    return ("bound", None)


def float_failure(got, rule, non_null, exact, magnitudes):
    """None, or why `got` is not a double sum of the group; rule: float_rule's answer ("bound" without looking when the
    magnitudes are finite)"""
    how, value = rule
    if how == "unpinned":
        return None
    if how == "is":
        same = (got != got) if value != value else got == value
        return None if same else "the overflow rule gives %r, got %r" % (value, got)
    bound = float_bound(non_null, exact, magnitudes)
    if got == got and abs(got - exact) <= bound:
        return None
    return "%r is %r from fsum %r, the bound is %r" % (got, abs(got - exact), exact, bound)


# ---- the numpy twin (the differential tester's tables: 400 000 rows a case) ----------------------------------------------
def _float_class_np(rows, vals):
    """float_class over a float64 slice"""
    if len(vals) == 1:
        v = float(vals[0])
        return (rows, 1, v, abs(v))
    return float_class(rows, vals.tolist())


def walk_np(values, valid, keys, key_valid=None, words=None, max_value_bytes=256, rules=False):
    """walk() over arrays: `values` an int64 or float64 array (the value column, widened), `valid` its non-NULL mask,
    `keys` an int64 array -- the group column's values, or with `words` (a list of distinct bytes) the index of each
    row's word -- and `key_valid` the group column's mask (None: no NULL keys).  Sorts the rows by key once and sums
    each group's slice: integers wrapping in uint64, floats with math.fsum as the walk does.
    rules=True adds, for float values, what a comparison beyond the entries needs: s["all"] and s["counted_class"], the
    float_class of every non-NULL value and of the entries' values together, and s["rules"], float_rule's answer for
    every entry (by key) and class (by name: null_group, long_rows, counted_class, all) whose magnitudes are not finite"""
    import numpy as np

    values, valid, keys = np.asarray(values), np.asarray(valid, bool), np.asarray(keys, np.int64)
    is_float = values.dtype == np.float64
    if not is_float and values.dtype != np.int64:
        raise TypeError("widen first: %s" % values.dtype)
    n = len(values)
    key_valid = np.ones(n, bool) if key_valid is None else np.asarray(key_valid, bool)

    def cls(rows_mask):
        v = values[rows_mask & valid]
        if is_float:
            return float_class(int(rows_mask.sum()), v.tolist())
        return (int(rows_mask.sum()), len(v), wrap(int(v.view(np.uint64).sum(dtype=np.uint64))))

    nothing = float_class(0, []) if is_float else int_class(0, [])
    s = dict(seen=n, is_float=bool(is_float) and n > 0, null_group=cls(~key_valid) if n else nothing, overflow=nothing)
    by_rule = {}

    def judged(name, c, vals):
        if rules and is_float and not math.isfinite(c[3]):
            by_rule[name] = float_rule(vals.tolist())
        return c
    if words is not None:
        order_of = np.argsort(np.array([bytes(w) for w in words] + [b""], dtype=object)[:-1], kind="stable") \
            if len(words) else np.zeros(0, np.int64)
        rank = np.empty(len(words), np.int64)
        rank[order_of] = np.arange(len(words))
        is_long = np.array([len(w) > max_value_bytes for w in words], bool)
        long_rows = key_valid & is_long[np.where(key_valid, keys, 0)] if len(words) else np.zeros(n, bool)
        sort_keys = rank[np.where(key_valid, keys, 0)] if len(words) else keys
    else:
        long_rows, sort_keys = np.zeros(n, bool), keys
    s["long_rows"] = cls(long_rows) if n else nothing
    live = key_valid & ~long_rows
    rows = np.flatnonzero(live)
    rows = rows[np.argsort(sort_keys[rows], kind="stable")]
    k_sorted = sort_keys[rows]
    starts = np.flatnonzero(np.concatenate([[True], k_sorted[1:] != k_sorted[:-1]])) if len(rows) else np.zeros(0, np.int64)
    ends = np.concatenate([starts[1:], [len(rows)]]).astype(np.int64)
    v_ok = valid[rows]
    non_null = np.add.reduceat(v_ok.astype(np.int64), starts) if len(starts) else np.zeros(0, np.int64)
    entries = {}
    if is_float:
        v_sorted = values[rows]
        for a, b, nn, key in zip(starts.tolist(), ends.tolist(), non_null.tolist(), keys[rows[starts]].tolist()):
            vals = v_sorted[a:b][v_ok[a:b]] if nn != b - a else v_sorted[a:b]
            key = bytes(words[key]) if words is not None else key
            entries[key] = judged(key, _float_class_np(b - a, vals), vals) if nn else (b - a, 0, 0.0, 0.0)
        s["counted"] = (sum(e[0] for e in entries.values()), sum(e[1] for e in entries.values()))
    else:
        masked = np.where(v_ok, values[rows], 0).view(np.uint64)
        sums = np.add.reduceat(masked, starts) if len(starts) else np.zeros(0, np.uint64)
        for a, b, nn, t, key in zip(starts.tolist(), ends.tolist(), non_null.tolist(), sums.tolist(),
                                    keys[rows[starts]].tolist()):
            entries[bytes(words[key]) if words is not None else key] = (b - a, nn, wrap(t))
        s["counted"] = (sum(e[0] for e in entries.values()), sum(e[1] for e in entries.values()),
                        wrap(sum(e[2] for e in entries.values())))
    if rules and is_float:
        for name, rows_mask in (("null_group", ~key_valid), ("long_rows", long_rows), ("counted_class", live),
                                ("all", np.ones(n, bool))):
            judged(name, s[name] if name in s else s.setdefault(name, cls(rows_mask)), values[rows_mask & valid])
        s["rules"] = by_rule
    s["entries"] = entries  # (ascending by key already: the rows were sorted by it)
    s["groups"] = len(entries)
    return s


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
