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


# ---- the same over numpy arrays (the differential tester's tables: 400 000 rows a case) ---------------------------------
# A VALUE side is (codes, words): an int64 array of indices into a list of DISTINCT bytes; a BINNED side is the column
# CAST AS DOUBLE as a float64 array.  tests/test_exact_pair_counts.py holds each of these to its walk.
def side_range_np(nums, both_valid):
    """side_range: nums the numeric side CAST AS DOUBLE, both_valid the rows with both sides non-NULL"""
    import numpy as np

    both = np.asarray(nums, np.float64)[np.asarray(both_valid, bool)]
    finite = both[np.isfinite(both)]
    return dict(seen=len(nums), both_non_null=len(both), n=len(finite), non_finite=len(both) - len(finite),
                min=float(finite.min()) if len(finite) else None, max=float(finite.max()) if len(finite) else None)


def binning_of_range(r, bins):
    """binning_of from a side_range"""
    if r["n"] == 0:
        return None
    return (r["min"], ej.bin_width(r["min"], r["max"], bins), bins)


def _bins_np(v, binning):
    """per row of a BINNED side: (bin index as int64, non-finite value, index outside [0, bins]), by the arithmetic of
    exact_joint.joint_counts_np: float64 subtract, divide and floor"""
    import numpy as np

    origin, width, bins = binning
    non_finite = ~np.isfinite(v)
    with np.errstate(over="ignore", invalid="ignore"):
        f = (np.where(non_finite, origin, v) - origin) / width
        inside = np.isfinite(f)
        i = np.floor(np.where(inside, f, -1.0))
    outside = ~inside | (i < 0) | (i > bins)
    return np.where(outside, 0, i).astype(np.int64), non_finite, outside


def _cells_np(words, max_value_bytes):
    """per word of a VALUE side: (its rank in bytewise order, longer than max_value_bytes)"""
    import numpy as np

    order = np.argsort(np.array([bytes(w) for w in words] + [b""], dtype=object)[:-1], kind="stable")
    rank = np.empty(len(words), np.int64)
    rank[order] = np.arange(len(words))
    return rank, order, np.array([len(w) > max_value_bytes for w in words] + [False], bool)[:-1]


def walk_np(x, y, both_valid, x_side=None, y_side=None, max_value_bytes=256):
    """walk() over arrays: x / y are (codes, words) for a VALUE side (x_side / y_side None) or a float64 array for a
    BINNED one; both_valid: the rows with both sides non-NULL"""
    import numpy as np

    both = np.asarray(both_valid, bool)
    n = len(both)
    is_long, non_finite, outside = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    ranks, cell_of = [], []
    for col, side in ((x, x_side), (y, y_side)):
        if side is None:
            codes, words = np.where(both, np.asarray(col[0], np.int64), 0), col[1]
            if len(words) == 0:  # (no word: no non-NULL row)
                ranks.append(np.zeros(n, np.int64))
                cell_of.append(lambda r: b"")
                continue
            rank, order, long_word = _cells_np(words, max_value_bytes)
            is_long |= both & long_word[codes]
            ranks.append(rank[codes])
            cell_of.append(lambda r, words=words, order=order: bytes(words[order[r]]))
        else:
            i, nf, out = _bins_np(np.asarray(col, np.float64), side)
            non_finite |= nf
            outside |= out
            ranks.append(i)
            cell_of.append(lambda r: r)
    non_finite &= both & ~is_long
    outside &= both & ~is_long & ~non_finite
    counted = both & ~is_long & ~non_finite & ~outside
    out = dict(seen=n, both_non_null=int(both.sum()), distinct=0, counted=int(counted.sum()), overflow_rows=0,
               long_rows=int(is_long.sum()), non_finite=int(non_finite.sum()), out_of_range=int(outside.sum()))
    rx, ry = ranks[0][counted], ranks[1][counted]
    span = int(ry.max()) + 1 if len(ry) else 1
    flat, c = np.unique(rx * span + ry, return_counts=True)
    out["counts"] = {(cell_of[0](k // span), cell_of[1](k % span)): cnt for k, cnt in zip(flat.tolist(), c.tolist())}
    out["distinct"] = len(flat)
    return out


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
