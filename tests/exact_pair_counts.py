"""The exact reference for TGX_CHECK_PAIR_COUNTS and the categorical branches of MutualInformationAnalyzer
(TG/analyzers/advanced/mutual_information.rs:249-293, 378-407): plain Python over lists with None, independent of the
library and of the oracle.

  SELECT cell(x), cell(y), COUNT(*) FROM t WHERE x IS NOT NULL AND y IS NOT NULL GROUP BY 1, 2

A side is a VALUE side (strings: the cell is the value's bytes) or a BINNED side (numbers with a binning (origin, width,
bins): the cell is FLOOR((CAST(v AS DOUBLE) - origin) / width), through tests/exact_joint.py's index walk).  A row with
both sides non-NULL is, in this order of precedence, a long row (a string longer than max_value_bytes on either side), a
non-finite row (a NaN or an infinity on a binned side), a row out of range (an index outside [0, bins]) or counted in its
pair.  The reference has no bounds, so overflow_rows is 0 here; a test that provokes overflow checks the invariant."""
import math

import mpmath

import exact_joint as ej


def as_cell(v):
    """a list element as a VALUE side sees it"""
    return None if v is None else (v.encode() if isinstance(v, str) else bytes(v))


def bin_of(v, binning):
    """("bin", i) | ("non_finite",) | ("outside",) for one non-NULL number, by exact_joint's walk of one row"""
    origin, width, bins = binning
    rows, non_finite = ej.live_rows([v], [0.0])
    if non_finite:
        return ("non_finite",)
    cells, outside = ej.joint_counts([v], [0.0], (origin, width, 0.0, 1.0, bins))
    if outside:
        return ("outside",)
    ((i, _),) = cells.keys()
    return ("bin", i)


def walk(xs, ys, x_side=None, y_side=None, max_value_bytes=256):
    """the eight counters and the pairs, ascending by (x cell, y cell): {seen, both_non_null, distinct, counted,
    overflow_rows, long_rows, non_finite, out_of_range, counts {(cx, cy): count}}.  x_side / y_side: None for a VALUE
    side, (origin, width, bins) for a BINNED one."""
    assert len(xs) == len(ys)
    out = dict(seen=len(xs), both_non_null=0, distinct=0, counted=0, overflow_rows=0, long_rows=0, non_finite=0,
               out_of_range=0)
    counts = {}
    for x, y in zip(xs, ys):
        if x is None or y is None:
            continue
        out["both_non_null"] += 1
        cells, kinds = [], []
        for v, side in ((x, x_side), (y, y_side)):
            if side is None:
                b = as_cell(v)
                kinds.append("long" if len(b) > max_value_bytes else "ok")
                cells.append(b)
            else:
                r = bin_of(v, side)
                kinds.append("ok" if r[0] == "bin" else r[0])
                cells.append(r[1] if r[0] == "bin" else None)
        if "long" in kinds:
            out["long_rows"] += 1
        elif "non_finite" in kinds:
            out["non_finite"] += 1
        elif "outside" in kinds:
            out["out_of_range"] += 1
        else:
            key = (cells[0], cells[1])
            counts[key] = counts.get(key, 0) + 1
    out["counts"] = dict(sorted(counts.items()))  # bytes compare bytewise (a prefix first), bins as integers
    out["distinct"] = len(counts)
    out["counted"] = sum(counts.values())
    assert out["counted"] + out["long_rows"] + out["non_finite"] + out["out_of_range"] == out["both_non_null"]
    return out


def side_range(nums, others):
    """the range phase: the numeric side over the rows with both sides non-NULL -> {seen, both_non_null, n, non_finite,
    min, max} (min / max None without rows)"""
    both = [float(v) for v, o in zip(nums, others) if v is not None and o is not None]
    finite = [v for v in both if math.isfinite(v)]
    return dict(seen=len(nums), both_non_null=len(both), n=len(finite), non_finite=len(both) - len(finite),
                min=min(finite) if finite else None, max=max(finite) if finite else None)


def binning_of(nums, others, bins):
    """(origin, width, bins) as mutual_information.rs:219-233 derives them from the range phase; None without rows"""
    r = side_range(nums, others)
    if r["n"] == 0:
        return None
    return (r["min"], ej.bin_width(r["min"], r["max"], bins), bins)


def marginals(counts):
    return ej.marginals(counts)


def label(cell):
    """a cell as the analyzer's state names it: the string itself, or the bin as CAST(FLOOR(..) AS VARCHAR) prints a
    double ("0.0", "1.0", ..)"""
    return "%d.0" % cell if isinstance(cell, int) else cell.decode("utf-8")


def analyzer_state(counts, bins):
    """MutualInformationState's serde form from the pairs, entries in the pairs' order"""
    xc, yc = marginals(counts)
    return dict(n=sum(counts.values()), joint_counts=[[label(x), label(y), c] for (x, y), c in counts.items()],
                x_counts={label(k): c for k, c in xc.items()}, y_counts={label(k): c for k, c in yc.items()}, bins=bins)


def mutual_information(counts):
    """the metric at 50 digits over the pairs: (value, sum of the terms' magnitudes, non-empty cells), as mpf"""
    return ej.mutual_information(counts, sum(counts.values()))


def metric_bound(counts):
    """|computed - exact| for sum p_xy ln(p_xy / (p_x p_y)) / LN_2 in doubles, from the cells themselves: per term two
    divisions by n for the marginals and one for p_xy, a product, a division, ln (within 1 ulp), a product -- 7
    roundings, each at most 2^-53 relative on a term (the roundings inside ln's argument move the term by the same
    relative amount times p_xy <= |term| only when |ln| >= 1, so they are charged against max(|term|, p_xy)); the
    running sum rounds once per term on a partial sum no larger than the sum of magnitudes; LN_2 and the last division
    one each.  Returns (exact value as a float, the bound)."""
    n = sum(counts.values())
    if n == 0:
        return 0.0, 0.0
    exact, magnitude, used = mutual_information(counts)
    xc, yc = marginals(counts)
    charged = mpmath.mpf(0)
    for (i, j), c in counts.items():
        p = mpmath.mpf(c) / n
        charged += max(abs(p * mpmath.log(p / (mpmath.mpf(xc[i]) / n * mpmath.mpf(yc[j]) / n))), p)
    u = 2.0 ** -53
    return float(exact), float((7 * charged + used * magnitude + 2 * magnitude) * u / mpmath.log(2)) + 2 * u * abs(float(exact))
