"""An independent reference for SPEARMAN: the rank sums of SQL RANK() over CAST(x AS DOUBLE), in exact integers.

What is ranked (TG/analyzers/advanced/correlation.rs:334-350): the rows where BOTH sides are non-NULL; each side CAST
AS DOUBLE -- an Int64 rounds to nearest, ties to even (Python's float(int)), so distinct integers beyond 2^53 can tie;
a Float64 keeps its bits, every NaN payload of either sign a value of its own; a Float32 widens exactly, and its NaNs
come out quiet (the CAST of a signalling NaN is the quiet NaN of the same payload, kernels/spearman.hip).  The order is
IEEE 754 totalOrder (Rust's f64::total_cmp): -NaN (larger payload first) < -inf < ... < -0 < +0 < ... < +inf < +NaN.
RANK() is the min-rank: 1 + the number of values strictly below.

From the ranks: n and the five sums (x, y, x^2, y^2, xy) as exact Python ints and wrapped mod 2^64 (DataFusion's UInt64
SUM); the doubles a tgx_result holds (float(int): one rounding, to nearest even); rho as a Fraction; the coefficient
the library computes from five doubles, step for step, and the error that computation may have."""
import decimal
import math
import struct
from fractions import Fraction

import numpy as np

import exact_widening as W

SIGN = 1 << 63
MAG = SIGN - 1
F64_QUIET = 1 << 51


# ---- keys, one value at a time (Python ints) ------------------------------------------------------------------------
def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def cast_int64_bits(v):
    """CAST(v AS DOUBLE) of an Int64, as bits: round to nearest, ties to even"""
    return f64_bits(float(int(v)))


def total_order_key(bits):
    """an integer that orders Float64 patterns as IEEE totalOrder: the magnitude on the positive side, -(magnitude + 1)
    on the negative side (so -0 sits just below +0 and a larger negative NaN payload sorts first)"""
    bits &= (1 << 64) - 1
    mag = bits & MAG
    return -mag - 1 if bits & SIGN else mag


def min_ranks_brute(keys):
    """RANK() by counting, O(n^2)"""
    return [1 + sum(1 for k in keys if k < q) for q in keys]


# ---- keys, vectorised -----------------------------------------------------------------------------------------------
def cast_bits(values, kind=None):
    """uint64 patterns of CAST(values AS DOUBLE).  kind: "i64", "f64", "f32" (raw Float32 patterns or float32 values),
    taken from the dtype when None"""
    v = np.asarray(values)
    if kind is None:
        kind = {"i": "i64", "f": "f64" if v.dtype.itemsize == 8 else "f32", "u": "f64"}[v.dtype.kind]
    if kind == "i64":
        ints = v.astype(np.int64)
        # float(int) rounds to nearest even; numpy's int64 -> float64 conversion is pinned against it in
        # tests/test_exact_ranks.py, the values where rounding matters are checked there one by one
        return ints.astype(np.float64).view(np.uint64)
    if kind == "f64":
        return np.ascontiguousarray(v).view(np.uint64) if v.dtype != np.uint64 else v
    if kind == "f32":
        return W.cast_f32_bits(v.view(np.uint32) if v.dtype == np.float32 else v.astype(np.uint32))
    raise ValueError(kind)


def keys_np(b64):
    """total_order_key of uint64 patterns as int64 (both formulas fit: -(2^63 - 1) - 1 .. 2^63 - 1)"""
    u = np.asarray(b64, np.uint64)
    mag = (u & np.uint64(MAG)).astype(np.int64)
    return np.where((u >> np.uint64(63)) != 0, -mag - 1, mag)


def min_ranks(keys):
    """RANK() by sorting: 1 + #{keys < k}"""
    k = np.asarray(keys, np.int64)
    return np.searchsorted(np.sort(k, kind="stable"), k, side="left").astype(np.int64) + 1


def pair_mask(n, xv=None, yv=None, xoff=0, yoff=0):
    return W.M.valid_mask(n, xv, xoff) & W.M.valid_mask(n, yv, yoff)


class RankSums:
    """n and the five sums of RANK(x), RANK(y) over the valid pairs, exact"""

    def __init__(self, rx, ry):
        rx, ry = np.asarray(rx, np.int64), np.asarray(ry, np.int64)
        self.n = len(rx)
        self.rx, self.ry = rx, ry
        self.exact = (_sum(rx), _sum(ry), _dot(rx, rx), _dot(ry, ry), _dot(rx, ry))

    @property
    def wrapped(self):
        return tuple(s % (1 << 64) for s in self.exact)

    def doubles(self, exact_sums=False):
        """the five doubles a tgx_result must hold: float() of the wrapped sums (default) or of the exact ones"""
        return tuple(float(s) for s in (self.exact if exact_sums else self.wrapped))

    def rho(self):
        return rho_fraction(self.n, *self.exact)


def _sum(r):
    return int(np.sum(r, dtype=np.int64))  # (ranks < 2^32, fewer than 2^31 of them: no overflow)


def _dot(a, b):
    """sum a_i b_i exactly: each product < 2^64 is split into 32-bit halves summed separately"""
    p = a.astype(np.uint64) * b.astype(np.uint64)
    lo = np.sum(p & np.uint64(MASK32_U), dtype=np.uint64)
    hi = np.sum(p >> np.uint64(32), dtype=np.uint64)
    return (int(hi) << 32) + int(lo)


MASK32_U = 0xFFFFFFFF


def rank_sums(xbits, ybits, mask=None):
    """RankSums of two columns given as CAST patterns (cast_bits), rows kept where mask is set"""
    xb, yb = np.asarray(xbits, np.uint64), np.asarray(ybits, np.uint64)
    if mask is not None:
        xb, yb = xb[mask], yb[mask]
    return RankSums(min_ranks(keys_np(xb)), min_ranks(keys_np(yb)))


def spearman(x, y, xv=None, yv=None, n=None, xoff=0, yoff=0, xkind=None, ykind=None):
    """RankSums of rows offset .. offset + n of two columns with Arrow validity bitmaps"""
    n = len(x) - xoff if n is None else n
    m = pair_mask(n, xv, yv, xoff, yoff)
    xb = cast_bits(np.asarray(x)[xoff: xoff + n], xkind)
    yb = cast_bits(np.asarray(y)[yoff: yoff + n], ykind)
    return rank_sums(xb, yb, m)


# ---- the coefficient ------------------------------------------------------------------------------------------------
def rho_fraction(n, sx, sy, sxx, syy, sxy, digits=60):
    """rho = (n Sxy - Sx Sy) / sqrt((n Sxx - Sx^2)(n Syy - Sy^2)) from exact sums: the numerator and the square of the
    denominator are exact integers, the square root is taken at `digits` digits; 0 where the denominator is 0 (a
    constant column), as the library answers"""
    num = n * sxy - sx * sy
    den2 = (n * sxx - sx * sx) * (n * syy - sy * sy)
    if den2 == 0:
        return Fraction(0)
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        den = decimal.Decimal(den2).sqrt()
    return Fraction(num) / Fraction(den)


def rho_double(n, sx, sy, sx2, sy2, sxy):
    """the library's coefficient from the five doubles (host/analyzers.cpp, CorrelationAnalyzer::metric_from_state),
    step for step in IEEE doubles; NaN below two pairs"""
    if n < 2:
        return math.nan
    n = float(n)
    num = n * sxy - sx * sy
    den = math.sqrt((n * sx2 - sx * sx) * (n * sy2 - sy * sy))
    return 0.0 if den == 0.0 else num / den


U = 2.0 ** -53


def rho_error_bound(n, sx, sy, sx2, sy2, sxy):
    """how far rho_double of these five doubles may lie from the rho of the exact sums they round: first-order error
    analysis of the rounding of each input (one unit in the last place at most) and of each operation, doubled.  A rho
    near 0 over many pairs is a small difference of two large products: the bound scales with the products, not with
    rho."""
    n = float(n)
    a, b = n * sx2 - sx * sx, n * sy2 - sy * sy
    if a <= 0.0 or b <= 0.0:
        return 0.0
    e_num = 3 * U * (abs(n * sxy) + abs(sx * sy)) + U * abs(n * sxy - sx * sy)
    e_a = 3 * U * (abs(n * sx2) + sx * sx)
    e_b = 3 * U * (abs(n * sy2) + sy * sy)
    den = math.sqrt(a * b)
    rho = abs(n * sxy - sx * sy) / den
    rel_den = 0.5 * (e_a / a + e_b / b) + 3 * U
    return 2.0 * (e_num / den + rho * rel_den + U * rho) + 1e-300
