"""The exact moment reference (tests/exact_moments.py) pinned on the CPU: it equals a plain Fraction evaluation on small
inputs, its sums equal math.fsum, and on well-conditioned pairs it agrees with the extended-precision two-pass of
test_gpu_correlation.exact_corr."""
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import exact_moments as X
import oracle_binding as orc


def _fraction_moments(vals):
    q = [Fraction(float(v)) for v in vals]
    n = len(q)
    mean = sum(q, Fraction(0)) / n
    m2 = sum(((v - mean) ** 2 for v in q), Fraction(0))
    return sum(q, Fraction(0)), mean, m2


def _small_cases():
    rng = np.random.default_rng(1)
    yield rng.standard_normal(50)
    yield 1e9 + rng.standard_normal(37)
    yield rng.standard_normal(64) * np.exp(rng.uniform(-40, 40, size=64))  # exponents far apart
    yield np.array([1.5e305] * 5)
    yield np.array([-0.0, 0.0, 5e-324, -5e-324, 1.0])
    yield rng.integers(-2 ** 62, 2 ** 62, size=40, dtype=np.int64)
    yield rng.integers(-2 ** 31, 2 ** 31, size=40).astype(np.int32)
    yield rng.integers(0, 2 ** 32, size=40).astype(np.uint32)
    yield (1e4 + rng.standard_normal(40)).astype(np.float32)


@pytest.mark.parametrize("case", range(9))
def test_moments_equal_a_fraction_evaluation(case):
    vals = list(_small_cases())[case]
    got = X.moments(vals)
    f64 = vals.astype(np.int64).astype(np.float64) if vals.dtype.kind in "iu" else vals.astype(np.float64)
    s, mean, m2 = _fraction_moments(f64)
    assert got.n == len(vals) and got.has_variance
    assert got.m2 == m2
    assert got.var_samp == float(m2 / (len(vals) - 1))
    if vals.dtype.kind in "iu":
        assert got.sum == sum(int(v) for v in vals)  # SUM(Int64): the exact integer, not the doubles' sum
    else:
        assert got.sum == s
        assert got.mean == float(mean)
    # the square root, rounded once: within half an ulp of the true one
    sd = got.stddev_samp
    var = m2 / (len(vals) - 1)
    assert abs(Fraction(sd) ** 2 - var) <= abs(Fraction(sd) * 2 * Fraction(math.ulp(sd))) / 2 + Fraction(1, 10 ** 300)


def test_validity_offset_and_non_finite():
    vals = np.array([1.0, 2.0, np.nan, 4.0, 7.0, np.inf])
    mask = np.array([True, False, False, True, True, True])
    v = orc.pack_validity(mask)
    got = X.moments(vals, v, n=4, offset=1)  # rows 1..4: 2 (NULL), NaN (NULL), 4, 7
    assert (got.total, got.n, got.sum, got.var_samp) == (4, 2, 11, 4.5)
    inf = X.moments(vals, v)
    assert inf.n == 4 and inf.sum_f == math.inf and math.isnan(inf.var_samp) and inf.has_variance
    nan = X.moments(vals)
    assert math.isnan(nan.sum_f) and math.isnan(nan.var_samp)
    assert X.moments(np.full(4096, 1.5e305)).sum_f == math.inf and X.moments(np.full(4096, 1.5e305)).var_samp == 0.0
    one = X.moments(np.array([3.0]))
    assert one.n == 1 and not one.has_variance and math.isnan(one.var_samp)
    none = X.moments(np.array([3.0]), orc.pack_validity(np.array([False])))
    assert none.n == 0 and not none.has_value


@pytest.mark.parametrize("seed", range(4))
def test_sums_equal_fsum(seed):
    rng = np.random.default_rng(seed)
    big = rng.standard_normal(20_000) * np.exp(rng.uniform(-30, 30, size=20_000))
    cancel = np.concatenate([big, -big[:-7], rng.standard_normal(7)])  # sum(|x|) / |sum(x)| around 1e13
    for vals in (big, cancel, 1.7e9 + rng.standard_normal(10_000)):
        got = X.moments(vals)
        assert got.sum_f == math.fsum(vals)
        assert X.moments(vals[:2000]).sum_sq == sum((Fraction(v) ** 2 for v in vals[:2000]), Fraction(0))
    ys = rng.standard_normal(5000)
    xs = 1e6 + rng.standard_normal(5000)
    c = X.comoments(xs, ys)
    assert float(c.sum_x) == math.fsum(xs) and float(c.sum_y) == math.fsum(ys)
    assert float(c.sum_xy) == float(sum(Fraction(a) * Fraction(b) for a, b in zip(xs, ys)))


def test_comoments_equal_a_fraction_evaluation():
    rng = np.random.default_rng(4)
    n = 300
    x = 1e9 + rng.standard_normal(n)
    y = rng.integers(-10 ** 12, 10 ** 12, size=n, dtype=np.int64)
    xm, ym = rng.random(n) > 0.2, rng.random(n) > 0.3
    got = X.comoments(x, y, orc.pack_validity(xm), orc.pack_validity(ym))
    both = xm & ym
    qx = [Fraction(float(v)) for v in x[both]]
    qy = [Fraction(float(v)) for v in y[both]]  # Int64 CAST AS DOUBLE
    k = len(qx)
    mx, my = sum(qx) / k, sum(qy) / k
    cxy = sum((a - mx) * (b - my) for a, b in zip(qx, qy))
    m2x = sum((a - mx) ** 2 for a in qx)
    m2y = sum((b - my) ** 2 for b in qy)
    assert (got.n, got.c_xy, got.m2_x, got.m2_y) == (k, cxy, m2x, m2y)
    assert got.sum_xy == sum(a * b for a, b in zip(qx, qy))
    assert got.covar_samp == float(cxy / (k - 1))
    assert abs(got.corr - float(cxy) / math.sqrt(float(m2x) * float(m2y))) <= 1e-15
    const = X.comoments(np.full(10, 1.7e9), x[:10])
    assert const.corr == 0.0 and const.m2_x == 0


def test_agrees_with_the_extended_two_pass_when_well_conditioned():
    from test_gpu_correlation import exact_corr

    rng = np.random.default_rng(9)
    n = 200_000
    x = rng.standard_normal(n) * 10
    y = 0.4 * x + rng.standard_normal(n)
    xv, yv = orc.pack_validity(rng.random(n) > 0.05), orc.pack_validity(rng.random(n) > 0.1)
    corr, cov = exact_corr(x, y, xv, yv)
    got = X.comoments(x, y, xv, yv)
    assert abs(got.corr - corr) <= 1e-15 * abs(corr)
    assert abs(got.covar_samp - cov) <= 1e-15 * abs(cov)
    m = X.moments(x, xv)
    xs = x[X.valid_mask(n, xv)].astype(np.longdouble)
    var = float(((xs - xs.mean()) ** 2).sum() / (len(xs) - 1))
    assert abs(m.var_samp - var) <= 1e-15 * var


def test_three_million_rows():
    """the size the GPU tests feed (a few seconds; reported, not asserted: a loaded machine must not fail it)"""
    rng = np.random.default_rng(0)
    x = 1_700_000_000_000 + rng.integers(0, 10 ** 8, size=3_000_000, dtype=np.int64)
    y = 1e9 + rng.standard_normal(3_000_000)
    t = time.perf_counter()
    m, c = X.moments(x), X.comoments(x, y)
    print("exact moments of 3 M rows and pairs: %.2f s" % (time.perf_counter() - t))
    assert m.n == c.n == 3_000_000 and m.sum == int(x.astype(object).sum())
