"""Exact ranks of numeric columns: the yardstick the -m gpu KLL tests compare the sketches with.

What the sketch sees of a column follows KllSketch::update (kll_sketch.rs:195-229): the non-NULL values, Int64 CAST AS
DOUBLE (rounded to nearest, ties to even: distinct integers beyond 2^53 become ties), every NaN bit pattern dropped,
+-inf and +-0 kept.  `kept` is that multiset, sorted.  From it follow the exact rank interval of a value, the rank error
of an answer and the exact order statistic; `rule_quantile` applies the library's query rule (kll_host.h,
KllHost::quantile) to the items and weights a sketch exports, and `check_sketch` holds a sketch to all of it."""
import math

import numpy as np

LEVEL_CAP = 1024      # kKllLevelCap (kll_host.h): items a level may hold after compaction
EXACT_BELOW = 1024    # fewer values than this are never compacted, on the device or on the host
RANK_CAP = 0.01       # the rank error the 512-item runs keep in practice, whatever k


def valid_mask(n, validity=None, offset=0):
    """bool[n]: Arrow's LSB-first validity bits offset .. offset + n (all valid without a bitmap)"""
    if validity is None:
        return np.ones(n, dtype=bool)
    bits = np.unpackbits(np.asarray(validity, dtype=np.uint8), bitorder="little")
    return bits[offset: offset + n].astype(bool)


def kept(values, validity=None, n=None, offset=0):
    """the values the sketch must see, sorted, as float64: rows offset .. offset + n that are valid and not NaN"""
    vals = np.asarray(values)
    n = len(vals) - offset if n is None else n
    v = vals[offset: offset + n][valid_mask(n, validity, offset)]
    if v.dtype.kind in "iu":
        f = v.astype(np.int64).astype(np.float64)  # CAST AS DOUBLE: round to nearest even (tests/test_exact_quantiles.py)
    else:
        f = v.astype(np.float64)
    return np.sort(f[~np.isnan(f)])


def rank_interval(srt, q):
    """[#kept < q, #kept <= q]"""
    return int(np.searchsorted(srt, q, side="left")), int(np.searchsorted(srt, q, side="right"))


def rank_error(srt, q, phi):
    """distance from phi * n to the rank interval of q, over n"""
    n = len(srt)
    lo, hi = rank_interval(srt, q)
    target = phi * n
    if lo <= target <= hi:
        return 0.0
    return min(abs(lo - target), abs(hi - target)) / n


def exact_quantile(srt, phi):
    """the order statistic the query rule picks from unweighted data: min, max, or srt[ceil(phi * n) - 1]"""
    n = len(srt)
    if phi == 0.0:
        return srt[0]
    if phi == 1.0:
        return srt[-1]
    return srt[max(1, math.ceil(phi * float(n))) - 1]


def phi_grid(n):
    """0, 1e-300, 1/n, 0.001 .. 0.999, 1 - 2^-53, 1"""
    grid = [0.0, 1e-300]
    if n:
        grid.append(1.0 / n)
    grid += [i / 1000 for i in range(1, 1000)]
    grid += [1.0 - 2.0 ** -53, 1.0]
    return grid


class Levels:
    """the items a sketch exports, in the order the library queries them: level 0 first, each level as stored"""

    def __init__(self, levels, min_v, max_v):
        self.levels = [np.asarray(lv, dtype=np.float64) for lv in levels]
        self.min_v, self.max_v = min_v, max_v
        items = np.concatenate(self.levels) if self.levels else np.zeros(0)
        weights = np.concatenate([np.full(len(lv), 1 << l, dtype=np.int64) for l, lv in enumerate(self.levels)]) \
            if self.levels else np.zeros(0, dtype=np.int64)
        order = np.argsort(items, kind="stable")  # std::stable_sort by `<`: -0 and +0 keep their level order
        self.items = items[order]
        self.cum = np.cumsum(weights[order])
        self.total = int(self.cum[-1]) if len(self.cum) else 0

    @property
    def weight(self):
        return sum(len(lv) << l for l, lv in enumerate(self.levels))


def rule_quantile(levels, phi):
    """KllHost::quantile on exported levels: phi = 0 -> min, phi = 1 -> max, otherwise the first item (stable order by
    value) whose cumulative weight, as a double, reaches ceil(phi * total weight)"""
    if phi == 0.0:
        return levels.min_v
    if phi == 1.0:
        return levels.max_v
    target = float(math.ceil(phi * float(levels.total)))
    i = int(np.searchsorted(levels.cum.astype(np.float64), target, side="left"))
    return levels.items[i] if i < len(levels.items) else levels.max_v


def export(st, spec_index):
    s = st.kll_summary(spec_index)
    return s, Levels([st.kll_level_items(spec_index, l) for l in range(s["num_levels"])], s["min"], s["max"])


def check_sketch(st, spec_index, srt, k, exact=None, result=None):
    """Holds the sketch of KLL spec `spec_index` of state `st` to the exact data `srt` (kept(...)).  Returns the worst
    rank error over the phi grid.  exact: every quantile is the exact order statistic (default: fewer than 1024
    values).  result: the spec's tgx_result, if the caller has one."""
    import term_amd as T

    n = len(srt)
    exact = n < EXACT_BELOW if exact is None else exact
    s, lv = export(st, spec_index)
    where = "spec %d (n=%d, k=%d)" % (spec_index, n, k)
    # 1. weight
    assert s["n"] == n, "weight: summary n %d != %d values, %s" % (s["n"], n, where)
    if result is not None:
        assert result.kll_n == n, "weight: kll_n %d != %d values, %s" % (result.kll_n, n, where)
    assert lv.weight == n, "weight: sum |level l| 2^l = %d != %d values, %s" % (lv.weight, n, where)
    # 4. level sizes
    sizes = [len(x) for x in lv.levels]
    assert max(sizes, default=0) <= LEVEL_CAP, "level cap: sizes %s, %s" % (sizes, where)
    assert s["num_retained"] == sum(sizes), "num_retained %d != %d, %s" % (s["num_retained"], sum(sizes), where)
    if n == 0:
        return 0.0
    # 2. MIN / MAX by value (which zero comes out of -0 and +0 is not pinned: both compare equal)
    assert s["min"] == srt[0] and s["max"] == srt[-1], "min/max: %r %r != %r %r, %s" % (
        s["min"], s["max"], srt[0], srt[-1], where)
    # 3. membership: every retained item is a value of the column (no NaN, no NULL row's value, nothing made up)
    items = lv.items
    pos = np.minimum(np.searchsorted(srt, items), n - 1)
    bad = items[srt[pos] != items]
    assert len(bad) == 0, "membership: %d retained items are not values of the column, e.g. %r, %s" % (
        len(bad), [float(x).hex() for x in bad[:4]], where)
    # 5. rule consistency, 6. rank error, 7. exactness
    bound = min(T.lib().tgx_kll_relative_error_bound(k), RANK_CAP)
    worst, worst_phi = 0.0, None
    for phi in phi_grid(n):
        got = st.kll_quantile(spec_index, phi)
        want = rule_quantile(lv, phi)
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), \
            "rule: quantile(%r) = %r, the rule on the exported levels gives %r, %s" % (phi, got, want, where)
        e = rank_error(srt, got, phi)
        if e > worst:
            worst, worst_phi = e, phi
        if exact:
            assert got == exact_quantile(srt, phi), "exact: quantile(%r) = %r != order statistic %r, %s" % (
                phi, got, exact_quantile(srt, phi), where)
    assert worst <= bound, "rank error %.5f at phi=%r above the bound %.5f, %s" % (worst, worst_phi, bound, where)
    return worst
