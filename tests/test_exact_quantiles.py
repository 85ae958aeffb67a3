"""The exact rank reference of tests/exact_quantiles.py, pinned on the CPU: the order statistic against NumPy and a
brute-force count, the query rule against an expansion of the items by weight, and what the sketch keeps of a column
(NULL rows, every NaN payload, Int64 CAST AS DOUBLE near 2^63)."""
import math
import struct

import numpy as np
import pytest

import exact_quantiles as Q


def brute_quantile(values, phi):
    """the smallest v with #{x <= v} >= phi * n (phi in (0, 1)): counted, not indexed"""
    n = len(values)
    for v in sorted(set(values.tolist())):
        if np.count_nonzero(values <= v) >= phi * n:
            return v
    raise AssertionError("unreachable")


@pytest.mark.parametrize("data", ["random", "ties", "one", "two", "signed_zeros", "infinities"])
def test_exact_quantile_is_the_inverted_cdf(data):
    rng = np.random.default_rng(7)
    x = {"random": lambda: rng.standard_normal(777),
         "ties": lambda: rng.integers(0, 5, 500).astype(np.float64),
         "one": lambda: np.array([3.5]),
         "two": lambda: np.array([2.0, -1.0]),
         "signed_zeros": lambda: np.array([0.0, -0.0, 1.0, -1.0, 0.0]),
         "infinities": lambda: np.array([np.inf, -np.inf, 1.0, 2.0, np.inf])}[data]()
    srt = np.sort(x)
    for phi in [1e-9, 0.001, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.9, 0.999, 1 - 1e-9]:
        got = Q.exact_quantile(srt, phi)
        assert got == np.quantile(x, phi, method="inverted_cdf"), (phi, got)
        assert got == brute_quantile(x, phi), (phi, got)
    assert Q.exact_quantile(srt, 0.0) == srt[0] and Q.exact_quantile(srt, 1.0) == srt[-1]
    for phi in Q.phi_grid(len(x)):  # the rank interval of the exact answer holds phi * n
        assert Q.rank_error(srt, Q.exact_quantile(srt, phi), phi) <= 1.0 / len(x)


def test_rank_interval_and_error():
    srt = np.array([1.0, 2.0, 2.0, 2.0, 5.0])
    assert Q.rank_interval(srt, 2.0) == (1, 4)
    assert Q.rank_interval(srt, 3.0) == (4, 4)
    assert Q.rank_interval(srt, 0.0) == (0, 0)
    assert Q.rank_error(srt, 2.0, 0.5) == 0.0              # 2.5 in [1, 4]
    assert Q.rank_error(srt, 5.0, 0.5) == (4 - 2.5) / 5    # [4, 5]
    assert Q.rank_error(srt, 1.0, 0.9) == (4.5 - 1) / 5    # [0, 1]


def expand(levels):
    out = []
    for l, lv in enumerate(levels):
        for v in lv:
            out += [v] * (1 << l)
    return np.sort(np.array(out))


@pytest.mark.parametrize("seed", range(6))
def test_rule_quantile_is_the_weighted_order_statistic(seed):
    """the rule (first item whose cumulative weight reaches ceil(phi W)) on a weighted sketch = the exact order
    statistic of the items expanded by their weights"""
    rng = np.random.default_rng(seed)
    levels = [rng.integers(0, 40, int(rng.integers(0, 30))).astype(np.float64) for _ in range(int(rng.integers(1, 6)))]
    levels[-1] = np.append(levels[-1], 17.0)
    lv = Q.Levels(levels, -100.0, 100.0)
    flat = expand(levels)
    assert lv.weight == lv.total == len(flat)
    for phi in Q.phi_grid(len(flat))[1:-1]:
        assert Q.rule_quantile(lv, phi) == Q.exact_quantile(flat, phi), phi
    assert Q.rule_quantile(lv, 0.0) == -100.0 and Q.rule_quantile(lv, 1.0) == 100.0  # MIN / MAX, not the items


def test_rule_quantile_by_hand_and_stable_across_levels():
    lv = Q.Levels([[5.0, 1.0], [3.0], [2.0]], 0.5, 9.0)  # weights 1, 1, 2, 4: total 8
    # sorted: 1 (w1, cum 1), 2 (w4, cum 5), 3 (w2, cum 7), 5 (w1, cum 8)
    for phi, want in ((0.1, 1.0), (0.125, 1.0), (0.126, 2.0), (0.625, 2.0), (0.626, 3.0), (0.875, 3.0), (0.9, 5.0)):
        assert Q.rule_quantile(lv, phi) == want, phi
    # equal values keep their level order: -0 (level 0) before +0 (level 1), as std::stable_sort with `<`
    z = Q.Levels([[-0.0], [0.0]], -0.0, 0.0)
    assert math.copysign(1, Q.rule_quantile(z, 0.2)) == -1.0
    z = Q.Levels([[0.0], [-0.0]], -0.0, 0.0)
    assert math.copysign(1, Q.rule_quantile(z, 0.2)) == 1.0


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_kept_drops_nulls_and_every_nan_keeps_inf_and_zeros():
    x = np.array([f64(0x7FF8000000000000), f64(0xFFF8000000000000), f64(0x7FF0000000000001),  # qNaN, -qNaN, sNaN
                  f64(0x7FF4000000000BEE), f64(0xFFF0000000000001), np.inf, -np.inf, 0.0, -0.0, 5e-324, 1.0, 99.0])
    mask = np.ones(len(x), bool)
    mask[-1] = False  # a NULL row's value
    validity = np.packbits(mask, bitorder="little")
    k = Q.kept(x, validity)
    assert len(k) == 6 and k[0] == -np.inf and k[-1] == np.inf and 99.0 not in k
    assert sorted(np.signbit(k[1:3]).tolist()) == [False, True]
    # an Arrow offset: rows 3 .. 3 + 8 of the buffer
    k = Q.kept(x, validity, n=8, offset=3)
    assert len(k) == 6 and not np.isnan(k).any()


def test_int64_cast_near_the_ends_rounds_as_the_cast():
    """Int64 CAST AS DOUBLE rounds to nearest, ties to even; Python's int -> float does that exactly, and the helper
    (NumPy's astype) must agree on the values where it matters: INT64_MIN / MAX, 2^53 + 1, halfway cases"""
    edge = [-2 ** 63, -2 ** 63 + 1, -2 ** 63 + 512, -2 ** 63 + 513, 2 ** 63 - 1, 2 ** 63 - 512, 2 ** 63 - 513,
            2 ** 63 - 1024, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, -(2 ** 53) - 1, 2 ** 54 + 2, 2 ** 54 + 6,
            1_700_000_000_123_456_789, 1_700_000_000_123_456_833, 0, -1]
    rng = np.random.default_rng(3)
    rand = rng.integers(-2 ** 63, 2 ** 63 - 1, 2000, dtype=np.int64, endpoint=True).tolist()
    vals = np.array(edge + rand, dtype=np.int64)
    k = Q.kept(vals)
    assert k.tolist() == sorted(float(int(v)) for v in vals.tolist())
    assert float(2 ** 63 - 1) == 2.0 ** 63 and float(2 ** 53 + 1) == 2.0 ** 53  # they do collapse
    # distinct integers become ties
    assert len(np.unique(k)) < len(np.unique(vals))
