"""The exact reference for the joint bin counts behind MutualInformationAnalyzer (numeric x numeric branch of
TG/analyzers/advanced/mutual_information.rs:143-248, 378-407): plain Python floats and integer counts, written from
the reference's SQL and independent of the library and of the oracle.

  1. over rows where both sides are non-NULL (and, the rule of include/tgx.h, finite), values as doubles:
     x_min, x_max, y_min, y_max;
  2. width = range / bins if range > 0 else 1.0 per side;
  3. per such row i = floor((x - x_min) / x_width), j likewise; COUNT(*) GROUP BY i, j;
  4. metric = sum p_xy ln(p_xy / (p_x p_y)) / ln 2, here with mpmath at 50 digits over the same cells.

Python's float arithmetic IS IEEE double arithmetic (subtract, correctly rounded divide), math.floor is exact, and
float(int) rounds an Int64 to nearest-even as CAST(.. AS DOUBLE) does."""
import math

import mpmath


def as_double(v):
    return None if v is None else float(v)


def live_rows(xs, ys):
    """(pairs of doubles with both sides non-NULL and finite, count of non-NULL pairs with a NaN / infinity)"""
    rows, non_finite = [], 0
    for x, y in zip(xs, ys):
        if x is None or y is None:
            continue
        a, b = float(x), float(y)
        if math.isfinite(a) and math.isfinite(b):
            rows.append((a, b))
        else:
            non_finite += 1
    return rows, non_finite


def pair_range(xs, ys):
    rows, non_finite = live_rows(xs, ys)
    out = dict(n=len(rows), non_finite=non_finite, x_min=None, x_max=None, y_min=None, y_max=None)
    if rows:
        out.update(x_min=min(r[0] for r in rows), x_max=max(r[0] for r in rows),
                   y_min=min(r[1] for r in rows), y_max=max(r[1] for r in rows))
    return out


def bin_width(lo, hi, bins):
    rng = hi - lo
    return rng / bins if rng > 0.0 else 1.0


def binning_of(xs, ys, bins):
    """(x_origin, x_width, y_origin, y_width, bins) as mutual_information.rs:219-233 derives them; None without rows"""
    bins = max(bins, 2)
    r = pair_range(xs, ys)
    if r["n"] == 0:
        return None
    return (r["x_min"], bin_width(r["x_min"], r["x_max"], bins), r["y_min"], bin_width(r["y_min"], r["y_max"], bins), bins)


def joint_counts(xs, ys, binning):
    """{(i, j): count} over the live rows, and the rows whose index fell outside [0, bins]"""
    x0, xw, y0, yw, bins = binning
    cells, outside = {}, 0
    rows, _ = live_rows(xs, ys)
    for a, b in rows:
        fi, fj = (a - x0) / xw, (b - y0) / yw
        if not (math.isfinite(fi) and math.isfinite(fj)):
            outside += 1
            continue
        i, j = math.floor(fi), math.floor(fj)
        if 0 <= i <= bins and 0 <= j <= bins:
            cells[(i, j)] = cells.get((i, j), 0) + 1
        else:
            outside += 1
    return cells, outside


def dense(cells, bins):
    """row-major (bins + 1)^2 list, the layout of tgx_joint_counts"""
    side = bins + 1
    out = [0] * (side * side)
    for (i, j), c in cells.items():
        out[i * side + j] = c
    return out


def marginals(cells):
    xc, yc = {}, {}
    for (i, j), c in cells.items():
        xc[i] = xc.get(i, 0) + c
        yc[j] = yc.get(j, 0) + c
    return xc, yc


def mutual_information(cells, n, x_counts=None, y_counts=None):
    """the metric at 50 digits: (value as mpf, sum of the terms' magnitudes as mpf, number of non-empty cells)"""
    if n == 0:
        return mpmath.mpf(0), mpmath.mpf(0), 0
    if x_counts is None:
        x_counts, y_counts = marginals(cells)
    with mpmath.workdps(50):
        total, mag, used = mpmath.mpf(0), mpmath.mpf(0), 0
        for (i, j), c in cells.items():
            cx, cy = x_counts.get(i, 0), y_counts.get(j, 0)
            if c > 0 and cx > 0 and cy > 0:
                p_xy, p_x, p_y = mpmath.mpf(c) / n, mpmath.mpf(cx) / n, mpmath.mpf(cy) / n
                term = p_xy * mpmath.log(p_xy / (p_x * p_y))
                total += term
                mag += abs(term)
                used += 1
        return total / mpmath.log(2), mag / mpmath.log(2), used


def merge_states(states):
    """MutualInformationState::merge (:31-75) on dicts {n, bins, joint_counts {(x, y): c}, x_counts, y_counts}"""
    if not states:
        raise ValueError("Cannot merge empty states")
    bins = states[0]["bins"]
    out = dict(n=0, bins=bins, joint_counts={}, x_counts={}, y_counts={})
    for s in states:
        if s["bins"] != bins:
            raise ValueError("Cannot merge states with different bin counts")
        out["n"] += s["n"]
        for name in ("joint_counts", "x_counts", "y_counts"):
            for k, c in s[name].items():
                out[name][k] = out[name].get(k, 0) + c
    return out


# ---- the same over numpy arrays (the differential tester's tables: 400 000 rows a case) ---------------------------
# x, y: the two columns CAST AS DOUBLE as float64 arrays; valid: rows with both sides non-NULL.  numpy's float64
# subtract, divide and floor are the IEEE operations the walks above do one row at a time; tests/test_exact_joint.py
# holds each of these to its walk.
def live_rows_np(x, y, valid):
    import numpy as np

    x, y = np.asarray(x, np.float64)[valid], np.asarray(y, np.float64)[valid]
    live = np.isfinite(x) & np.isfinite(y)
    return x[live], y[live], int(len(x) - live.sum())


def pair_range_np(x, y, valid):
    a, b, non_finite = live_rows_np(x, y, valid)
    out = dict(n=len(a), non_finite=non_finite, x_min=None, x_max=None, y_min=None, y_max=None)
    if len(a):
        out.update(x_min=float(a.min()), x_max=float(a.max()), y_min=float(b.min()), y_max=float(b.max()))
    return out


def binning_of_range(r, bins):
    """binning_of from a pair_range"""
    bins = max(bins, 2)
    if r["n"] == 0:
        return None
    return (r["x_min"], bin_width(r["x_min"], r["x_max"], bins), r["y_min"], bin_width(r["y_min"], r["y_max"], bins), bins)


def joint_counts_np(x, y, valid, binning):
    import numpy as np

    x0, xw, y0, yw, bins = binning
    a, b, _ = live_rows_np(x, y, valid)
    with np.errstate(over="ignore", invalid="ignore"):
        fi, fj = (a - x0) / xw, (b - y0) / yw
        inside = np.isfinite(fi) & np.isfinite(fj)
        i, j = np.floor(fi[inside]), np.floor(fj[inside])
    ok = (i >= 0) & (i <= bins) & (j >= 0) & (j <= bins)
    flat = i[ok].astype(np.int64) * (bins + 1) + j[ok].astype(np.int64)
    cells = {(int(k) // (bins + 1), int(k) % (bins + 1)): int(c) for k, c in zip(*np.unique(flat, return_counts=True))}
    return cells, int(len(a) - ok.sum())
