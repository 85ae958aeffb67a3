"""Exact moments of numeric columns: the yardstick the -m gpu moment tests compare the kernels with.

Every finite double is m * 2^e with an integer m of at most 53 bits (np.frexp).  Brought to the column's smallest
exponent, the values are Python integers, and n, SUM(x), SUM(x^2), M2 = SUM(x^2) - SUM(x)^2 / n and, for pairs,
SUM(x y) and C_xy = SUM(x y) - SUM(x) SUM(y) / n are exact integers or fractions.  Results are rounded to double once, at
the end; square roots are taken in `decimal` at 60 digits first.

What a value is follows the kernels and DataFusion: Int64 / Int32 / UInt32 columns are summed as exact integers
(SUM(Int64)), while their VARIANCE, CORR and COVAR_SAMP are those of the values CAST AS DOUBLE; Float32 is widened to
Float64 exactly.  A NaN or an infinity among the valid values gives the IEEE result (a NaN variance; SUM inf or NaN)."""
import decimal
import math
from fractions import Fraction

import numpy as np

_DEC = decimal.Context(prec=60)


def valid_mask(n, validity=None, offset=0):
    """bool[n]: Arrow's LSB-first validity bits offset .. offset + n (all valid without a bitmap)"""
    if validity is None:
        return np.ones(n, dtype=bool)
    bits = np.unpackbits(np.asarray(validity, dtype=np.uint8), bitorder="little")
    return bits[offset: offset + n].astype(bool)


def _values(values, validity, n, offset):
    vals = np.asarray(values)
    n = len(vals) - offset if n is None else n
    return vals[offset: offset + n], valid_mask(n, validity, offset)


def _as_f64(v):
    """what the kernels fold for the moments: every value cast to double (Float32 / integers widened exactly first)"""
    if v.dtype.kind in "iu":
        return v.astype(np.int64).astype(np.float64)
    return v.astype(np.float64)


def dyadic(x):
    """(X, e0) with x[i] == X[i] * 2**e0 exactly: X an object array of Python ints.  x: finite float64."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if len(x) == 0:
        return np.zeros(0, dtype=object), 0
    m, e = np.frexp(x)
    mant = (m * 2.0 ** 53).astype(np.int64)  # exact: |m| in [0.5, 1) has 53 significant bits
    exp = e.astype(np.int64) - 53
    nz = mant != 0
    e0 = int(exp[nz].min()) if nz.any() else 0
    shift = np.where(nz, exp - e0, 0)
    return mant.astype(object) << shift.astype(object), e0


def _scaled(num, e):
    """Fraction(num * 2**e)"""
    return Fraction(num * 2 ** e) if e >= 0 else Fraction(num, 2 ** -e)


def to_float(q):
    """a Fraction rounded to double once; beyond DBL_MAX it is the infinity IEEE arithmetic ends at"""
    try:
        return float(q)
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def _dec(q):
    return _DEC.divide(decimal.Decimal(q.numerator), decimal.Decimal(q.denominator))


def _sqrt(q):
    """correctly rounded to 60 digits first, then to double"""
    return float(_DEC.sqrt(_dec(q)))


class Moments:
    """NUMERIC_STATS of one column, exactly.  sum / sum_sq / m2 are Fractions (sum: of the values as SUM sees them);
    mean, var_samp, stddev_samp are doubles rounded once from the exact values."""

    def __init__(self, n, total, integer, s, finite, sum_ieee, s1=None, s2=None, e0=0):
        self.total, self.n, self.integer = total, n, integer
        self.has_value = n > 0
        self.has_variance = n >= 2
        self.finite = finite
        self.sum = s
        if not finite:
            self.sum_f = sum_ieee
            self.mean = sum_ieee / n if n else math.nan
            self.sum_sq = self.m2 = None
            self.var_samp = self.stddev_samp = math.nan
            return
        self.sum_f = to_float(s)
        self.mean = float(s / n) if n else math.nan
        # SUM and SUM^2 of the doubles: the variance of an integer column is that of its values cast to double
        self.sum_sq = _scaled(s2, 2 * e0)
        self.m2 = _scaled(n * s2 - s1 * s1, 2 * e0) / n if n else Fraction(0)
        if n >= 2:
            var = self.m2 / (n - 1)
            self.var_samp = float(var)
            self.stddev_samp = _sqrt(var)
        else:
            self.var_samp = self.stddev_samp = math.nan

    @property
    def sum_i_wrapping(self):
        """SUM(Int64) as the kernels report it: the exact sum wrapped to 64 bits"""
        v = int(self.sum) & (2 ** 64 - 1)
        return v - 2 ** 64 if v >= 2 ** 63 else v


def moments(values, validity=None, n=None, offset=0):
    v, m = _values(values, validity, n, offset)
    total = len(v)
    v = v[m]
    cnt = len(v)
    integer = v.dtype.kind in "iu"
    f = _as_f64(v)
    finite = bool(np.isfinite(f).all())
    if not finite:
        with np.errstate(invalid="ignore", over="ignore"):
            sum_ieee = float(np.sum(f[~np.isfinite(f)]))  # inf, -inf or NaN: what any order of summation gives
        return Moments(cnt, total, integer, None, False, sum_ieee)
    X, e0 = dyadic(f)
    s1 = int(X.sum()) if cnt else 0
    s2 = int((X * X).sum()) if cnt else 0
    s = Fraction(int(v.astype(np.int64).astype(object).sum()) if cnt else 0) if integer else _scaled(s1, e0)
    return Moments(cnt, total, integer, s, True, None, s1, s2, e0)


class CoMoments:
    """COMOMENTS of a pair over the rows where both values are valid, every value CAST AS DOUBLE: the raw sums as
    Fractions (sum_x, sum_y, sum_x2, sum_y2, sum_xy), the centred ones (m2_x, m2_y, c_xy) and CORR / COVAR_SAMP as
    doubles rounded once."""


def comoments(x, y, xv=None, yv=None, n=None, xoff=0, yoff=0):
    n = len(x) - xoff if n is None else n
    xs, xm = _values(x, xv, n, xoff)
    ys, ym = _values(y, yv, n, yoff)
    both = xm & ym
    fx, fy = _as_f64(xs[both]), _as_f64(ys[both])
    out = CoMoments()
    out.total, out.n = n, int(both.sum())
    out.finite = bool(np.isfinite(fx).all() and np.isfinite(fy).all())
    if not out.finite:
        raise ValueError("comoments: non-finite values (the exact reference covers finite pairs)")
    X, ex = dyadic(fx)
    Y, ey = dyadic(fy)
    k = out.n
    sx, sy = (int(X.sum()), int(Y.sum())) if k else (0, 0)
    sxx, syy, sxy = (int((X * X).sum()), int((Y * Y).sum()), int((X * Y).sum())) if k else (0, 0, 0)
    out.sum_x, out.sum_y = _scaled(sx, ex), _scaled(sy, ey)
    out.sum_x2, out.sum_y2, out.sum_xy = _scaled(sxx, 2 * ex), _scaled(syy, 2 * ey), _scaled(sxy, ex + ey)
    # n * centred sums, as integers of the common scales
    a, b, c = k * sxx - sx * sx, k * syy - sy * sy, k * sxy - sx * sy
    if k == 0:
        out.m2_x = out.m2_y = out.c_xy = Fraction(0)
        out.corr = out.covar_samp = math.nan
        return out
    out.m2_x, out.m2_y, out.c_xy = _scaled(a, 2 * ex) / k, _scaled(b, 2 * ey) / k, _scaled(c, ex + ey) / k
    out.mean_x, out.mean_y = float(out.sum_x / k), float(out.sum_y / k)
    # CORR = c / sqrt(a b): the scales cancel.  DataFusion returns 0 when a deviation is 0.
    if a == 0 or b == 0:
        out.corr = 0.0
    else:
        out.corr = float(_DEC.divide(decimal.Decimal(c), _DEC.sqrt(_DEC.multiply(decimal.Decimal(a), decimal.Decimal(b)))))
    out.covar_samp = float(out.c_xy / (k - 1)) if k >= 2 else math.nan
    return out
