"""An independent reference for APPROX_DISTINCT: the HyperLogLog registers and the cardinality estimate, written from
the rule in DESIGN.md / kernels/device_types.h and Ertl's paper, not from the oracle.

- hash_int / registers_int: the hash and the register update in Python ints (slow; a cross-check for a few values).
- hash_np / ranks_np / registers: the same in numpy uint32 arithmetic, fast enough for 10^7 values.
  A value is its 64-bit pattern (Int64 as two's complement, Float64 as its bits, Int32 sign-extended, Float32 widened
  bit-preservingly: exact_widening); lo / hi are its two 32-bit halves.
      a = lo ^ rotl32(hi * 0x9E3779B1, 15), then Murmur3's 32-bit finaliser
      b = (hi ^ rotl32(a, 16)) * 0x27D4EB2F
      register = a mod 2^14, rank = clz32(b) + 1 (1 .. 32), and 33 when b == 0
  A register holds the largest rank of the values that map to it, 0 when none does.  NULL rows are skipped.
- estimate_exact: Ertl (2017), "New cardinality estimation algorithms for HyperLogLog sketches", algorithm 6 with
  m = 2^14 and q = 32 (ranks 0 .. q + 1), sigma and tau summed in `decimal` at 60 digits, rounded to the nearest
  integer.
- estimate_double: the same steps in IEEE doubles, in the library's order of operations (tgx_api.cpp, hll_estimate),
  rounded half away from zero as llround.  The library must equal it exactly; it must lie within 1 of estimate_exact.
- rel_bound(n): the relative error an estimate of n distinct values is held to (see there)."""
import decimal
import math

import numpy as np

P = 14
M = 1 << P
Q = 32           # the rank comes from a 32-bit word: ranks 1 .. 32, and q + 1 = 33 for b == 0
MAX_RANK = Q + 1
MASK32 = 0xFFFFFFFF


# ---- the hash, in Python ints ---------------------------------------------------------------------------------------
def _rotl_int(x, r):
    return ((x << r) | (x >> (32 - r))) & MASK32


def hash_int(bits):
    """(a, b) of one 64-bit pattern (a Python int, taken mod 2^64)"""
    bits &= (1 << 64) - 1
    lo, hi = bits & MASK32, bits >> 32
    a = lo ^ _rotl_int((hi * 0x9E3779B1) & MASK32, 15)
    a ^= a >> 16
    a = (a * 0x85EBCA6B) & MASK32
    a ^= a >> 13
    a = (a * 0xC2B2AE35) & MASK32
    a ^= a >> 16
    b = ((hi ^ _rotl_int(a, 16)) * 0x27D4EB2F) & MASK32
    return a, b


def rank_int(b):
    """clz32(b) + 1; 33 for b == 0"""
    return 32 - b.bit_length() + 1


def registers_int(values):
    """registers of an iterable of 64-bit patterns (Python ints; None is a NULL)"""
    regs = [0] * M
    for v in values:
        if v is None:
            continue
        a, b = hash_int(v)
        i = a & (M - 1)
        regs[i] = max(regs[i], rank_int(b))
    return np.array(regs, dtype=np.uint8)


# ---- the hash, vectorised -------------------------------------------------------------------------------------------
def _rotl_np(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def hash_np(b64):
    """(a, b) as uint32 arrays of uint64 patterns (any 8-byte dtype is read as its bits)"""
    u = np.ascontiguousarray(b64)
    if u.dtype != np.uint64:
        u = u.view(np.uint64)
    lo = (u & np.uint64(MASK32)).astype(np.uint32)
    hi = (u >> np.uint64(32)).astype(np.uint32)
    with np.errstate(over="ignore"):  # (uint32 products wrap mod 2^32, as the C multiplies)
        a = lo ^ _rotl_np(hi * np.uint32(0x9E3779B1), 15)
        a ^= a >> np.uint32(16)
        a *= np.uint32(0x85EBCA6B)
        a ^= a >> np.uint32(13)
        a *= np.uint32(0xC2B2AE35)
        a ^= a >> np.uint32(16)
        b = (hi ^ _rotl_np(a, 16)) * np.uint32(0x27D4EB2F)
    return a, b


def ranks_np(b):
    """clz32(b) + 1 of a uint32 array, 33 where b == 0: 33 - bit_length(b), the bit length found by shifts"""
    x = np.asarray(b, np.uint32).copy()
    bl = np.zeros(x.shape, np.uint8)
    for s in (16, 8, 4, 2, 1):
        hi = (x >> np.uint32(s)) != 0
        bl[hi] += np.uint8(s)
        x[hi] >>= np.uint32(s)
    bl[x != 0] += np.uint8(1)
    return np.uint8(MAX_RANK) - bl


def valid_rows(n, validity=None, offset=0):
    if validity is None:
        return np.ones(n, dtype=bool)
    bits = np.unpackbits(np.asarray(validity, dtype=np.uint8), bitorder="little")
    return bits[offset: offset + n].astype(bool)


def index_and_rank(b64):
    a, b = hash_np(b64)
    return (a & np.uint32(M - 1)).astype(np.int64), ranks_np(b)


def registers(b64, validity=None, n=None, offset=0):
    """uint8[2^14] registers of rows offset .. offset + n of uint64 patterns; NULL rows skipped"""
    u = np.ascontiguousarray(b64)
    if u.dtype != np.uint64:
        u = u.view(np.uint64)
    n = len(u) - offset if n is None else n
    v = u[offset: offset + n][valid_rows(n, validity, offset)]
    idx, rank = index_and_rank(v)
    seen = np.bincount(idx * 64 + rank.astype(np.int64), minlength=M * 64).reshape(M, 64) > 0
    top = 63 - np.argmax(seen[:, ::-1], axis=1)  # the largest rank seen per register
    return np.where(seen.any(axis=1), top, 0).astype(np.uint8)


def merge(*regs):
    return np.maximum.reduce([np.asarray(r, np.uint8) for r in regs])


def histogram(regs):
    """C_k: the number of registers of rank k, k = 0 .. q + 1"""
    return np.bincount(np.asarray(regs, np.int64), minlength=MAX_RANK + 1)[: MAX_RANK + 1]


# ---- the estimator --------------------------------------------------------------------------------------------------
DIGITS = 60


def sigma_decimal(x):
    """sigma(x) = x + sum_{k >= 1} x^(2^k) 2^(k - 1); infinite at x = 1"""
    x = decimal.Decimal(x)
    if x == 1:
        return decimal.Decimal("Infinity")
    total, power, w = x, x, decimal.Decimal(1)
    eps = decimal.Decimal(10) ** -(DIGITS + 5)
    while True:
        power = power * power
        term = power * w
        if term < eps:
            return total
        total += term
        w += w


def tau_decimal(x):
    """tau(x) = (1 - x - sum_{k >= 1} (1 - x^(2^-k))^2 2^-k) / 3; 0 at x = 0 and x = 1"""
    x = decimal.Decimal(x)
    if x == 0 or x == 1:
        return decimal.Decimal(0)
    total, root, w = 1 - x, x, decimal.Decimal(1)
    eps = decimal.Decimal(10) ** -(DIGITS + 5)
    while True:
        root = root.sqrt()
        w /= 2
        term = (1 - root) * (1 - root) * w
        if term < eps:
            return total / 3
        total -= term


def estimate_exact_value(regs):
    """Ertl's algorithm 6 at 60 digits, unrounded (a Decimal); 0 for empty registers"""
    c = histogram(regs)
    with decimal.localcontext() as ctx:
        ctx.prec = DIGITS
        m = decimal.Decimal(M)
        z = m * tau_decimal((m - int(c[Q + 1])) / m)
        for k in range(Q, 0, -1):
            z = (z + int(c[k])) / 2
        z += m * sigma_decimal(int(c[0]) / m)
        if z.is_infinite():
            return decimal.Decimal(0)
        return m * m / (2 * decimal.Decimal(2).ln() * z)


def estimate_exact(regs):
    e = estimate_exact_value(regs)
    return int(e.to_integral_value(rounding=decimal.ROUND_HALF_UP))


def sigma_double(x):
    """hll_sigma's steps in doubles"""
    if x == 1.0:
        return math.inf
    y, z = 1.0, x
    while True:
        x *= x
        z0 = z
        z += x * y
        y += y
        if z0 == z:
            return z


def tau_double(x):
    """hll_tau's steps in doubles"""
    if x == 0.0 or x == 1.0:
        return 0.0
    y, z = 1.0, 1.0 - x
    while True:
        x = math.sqrt(x)
        z0 = z
        y *= 0.5
        z -= (1.0 - x) * (1.0 - x) * y
        if z0 == z:
            return z / 3.0


def llround(e):
    f = math.floor(e)
    return int(f) + (1 if e - f >= 0.5 else 0)


def estimate_double(regs):
    """the estimate in IEEE doubles, in the library's order of operations"""
    c = histogram(regs)
    m = float(M)
    z = m * tau_double((m - float(c[Q + 1])) / m)
    for k in range(Q, 0, -1):
        z = 0.5 * (z + float(c[k]))
    z += m * sigma_double(float(c[0]) / m)
    with np.errstate(divide="ignore"):
        e = 0.5 / math.log(2.0) * m * m / z if z != 0.0 else math.inf
    return llround(e) if math.isfinite(e) else 0


# ---- accuracy -------------------------------------------------------------------------------------------------------
RSE = 1.04 / math.sqrt(M)  # the large-range relative standard error of HyperLogLog, 1.04 / 128


def rel_bound(n):
    """Four standard errors, plus one count for the rounding to an integer.  The standard error is the smaller of
    HyperLogLog's 1.04 / sqrt(m) and that of linear counting, sqrt(m (e^t - t - 1)) / n with t = n / m (Whang et al.
    1990): Ertl's estimator behaves like linear counting while most registers are empty, and below about t = 2 that
    is the smaller error -- 0.55 % for small n, where 1.04 / 128 would let a two-value column come out as one."""
    if n <= 0:
        return 0.0
    t = n / M
    lc = math.sqrt(M * math.expm1(t) - M * t) / n if t < 50 else math.inf
    return 4.0 * min(RSE, lc) + 1.0 / n


def _inv_xorshift(y, s):
    x = y
    for _ in range(32 // s + 1):
        x = y ^ (x >> s)
    return x


def value_with_b_zero(hi):
    """the 64-bit pattern with high half `hi` whose b is 0 (rank 33): b = (hi ^ rotl(a, 16)) * odd is 0 exactly when
    a = rotr(hi, 16), and the finaliser that makes a from lo is a bijection -- inverted here"""
    x = _rotl_int(hi, 16)  # (rotr by 16 = rotl by 16)
    x = _inv_xorshift(x, 16)
    x = (x * pow(0xC2B2AE35, -1, 1 << 32)) & MASK32
    x = _inv_xorshift(x, 13)
    x = (x * pow(0x85EBCA6B, -1, 1 << 32)) & MASK32
    x = _inv_xorshift(x, 16)
    lo = x ^ _rotl_int((hi * 0x9E3779B1) & MASK32, 15)
    return (hi << 32) | lo
