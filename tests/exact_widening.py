"""Exact references for the columns that are not 8 bytes wide (include/tgx.h: TGX_INT32 / TGX_FLOAT32 and the narrow
integers, TGX_BOOL), computed from the ORIGINAL-width values with integer arithmetic only.

The kernels widen with hardware conversions; a reference that widened with numpy's `astype` would share their faults
(a float-to-double conversion quiets a signalling NaN, and may flush a subnormal).  Here nothing is converted by a
floating-point unit:

- widen_f32_bits: the Float64 bit pattern a Float32 pattern stands for, bit-preserving and injective.  Normal numbers
  are rebiased, subnormals normalised by integer shifts, +-0 / +-inf map to themselves, and a NaN keeps its sign, its
  payload (shifted up by 29) and its quiet bit as it was.  This is the key DISTINCT, multiplicity and APPROX_DISTINCT
  see, and the order MIN / MAX take.
- cast_f32_bits: what CAST(x AS DOUBLE) gives: the same map with the quiet bit of every NaN set.  Spearman's RANK()
  orders the CAST values (kernels/spearman.hip).
- widen_int: Int8 / Int16 / Int32 sign-extended, UInt8 / UInt16 / UInt32 zero-extended, Boolean bits read from any
  bit offset; each from the raw bytes.

The expected answers per check kind follow at the end; moments and KLL go through exact_moments / exact_quantiles."""
import numpy as np

import exact_moments as M
import exact_quantiles as Q

F32_SIGN, F32_EXP, F32_MANT, F32_QUIET = 0x80000000, 0x7F800000, 0x007FFFFF, 0x00400000
F64_EXP, F64_QUIET = 0x7FF0000000000000, 0x0008000000000000


def _u32(bits):
    bits = np.asarray(bits)
    if bits.dtype == np.float32 or bits.dtype == np.int32:
        bits = bits.view(np.uint32)
    return bits.astype(np.uint64)  # (an integer widening: uint32 -> uint64 is exact)


def _bit_length(m):
    """floor(log2 m) + 1 of positive integers below 2^24, by shifts (0 for 0)"""
    out = np.zeros(m.shape, np.uint64)
    x = m.copy()
    for s in (16, 8, 4, 2, 1):
        hi = (x >> np.uint64(s)) != 0
        out[hi] += np.uint64(s)
        x[hi] >>= np.uint64(s)
    out[x != 0] += np.uint64(1)
    return out


def widen_f32_bits(bits):
    """uint32 Float32 patterns -> uint64 Float64 patterns, bit-preserving (NaN payloads and quiet bits kept)"""
    u = _u32(bits)
    sign = (u >> np.uint64(31)) << np.uint64(63)
    e = (u >> np.uint64(23)) & np.uint64(0xFF)
    m = u & np.uint64(F32_MANT)
    out = sign.copy()  # +-0
    normal = (e != 0) & (e != 0xFF)
    out[normal] |= ((e[normal] + np.uint64(1023 - 127)) << np.uint64(52)) | (m[normal] << np.uint64(29))
    special = e == 0xFF  # inf (m = 0) and NaN: the payload moves up, the quiet bit (f32 bit 22) becomes bit 51
    out[special] |= np.uint64(F64_EXP) | (m[special] << np.uint64(29))
    sub = (e == 0) & (m != 0)  # m * 2^-149 = 2^p * (1 + f), p = bitlen(m) - 1 - 149
    if sub.any():
        ms = m[sub]
        p = _bit_length(ms) - np.uint64(1)  # 0 .. 22: the leading one's position
        frac = (ms - (np.uint64(1) << p)) << (np.uint64(52) - p)
        out[sub] |= ((p + np.uint64(1023 - 149)) << np.uint64(52)) | frac
    return out


def cast_f32_bits(bits):
    """CAST(x AS DOUBLE) of Float32 patterns: widen_f32_bits with every NaN made quiet"""
    u = _u32(bits)
    out = widen_f32_bits(u)
    nan = (u & np.uint64(0x7FFFFFFF)) > np.uint64(F32_EXP)
    out[nan] |= np.uint64(F64_QUIET)
    return out


INT_WIDTH = {"int8": (1, True), "int16": (2, True), "int32": (4, True),
             "uint8": (1, False), "uint16": (2, False), "uint32": (4, False)}


def widen_int(values, type_name, n=None, bit_offset=0):
    """the Int64 values a narrow integer column stands for, from its raw bytes (numpy int64).  type_name "bool":
    `values` is the bit-packed buffer, row i is bit bit_offset + i (n rows)."""
    if type_name == "bool":
        buf = np.frombuffer(np.ascontiguousarray(values).tobytes(), np.uint8).astype(np.int64)
        i = np.arange(n, dtype=np.int64) + bit_offset
        return (buf[i >> 3] >> (i & 7)) & 1
    width, signed = INT_WIDTH[type_name]
    raw = np.frombuffer(np.ascontiguousarray(values).tobytes(), np.uint8).reshape(-1, width).astype(np.int64)
    u = np.zeros(raw.shape[0], np.int64)
    for b in range(width):  # little-endian bytes
        u |= raw[:, b] << (8 * b)
    if signed:
        u -= (u >> (8 * width - 1)) << (8 * width)
    return u


def is_nan_bits(b64):
    return (np.asarray(b64, np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(F64_EXP)


def total_key(b64):
    """the signed total order of Float64 patterns (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)"""
    s = np.asarray(b64, np.uint64).view(np.int64)
    return np.where(s < 0, s ^ np.int64(0x7FFFFFFFFFFFFFFF), s)


def _mask(n, validity, offset):
    return M.valid_mask(n, validity, offset)


def count(n, validity=None, offset=0):
    return n, int(_mask(n, validity, offset).sum())


def minmax_bits(b64, validity=None, n=None, offset=0):
    """MIN / MAX of Float64 patterns under the total order, as patterns (None, None when no value is valid)"""
    n = len(b64) - offset if n is None else n
    v = np.asarray(b64, np.uint64)[offset:offset + n][_mask(n, validity, offset)]
    if len(v) == 0:
        return None, None
    k = total_key(v)
    return int(v[np.argmin(k)]), int(v[np.argmax(k)])


def int_stats(wide, validity=None, n=None, offset=0):
    """(non_null, min, max, exact sum) of Int64 values"""
    n = len(wide) - offset if n is None else n
    v = np.asarray(wide, np.int64)[offset:offset + n][_mask(n, validity, offset)]
    if len(v) == 0:
        return 0, None, None, 0
    return len(v), int(v.min()), int(v.max()), int(v.astype(object).sum())


def float_moments(b64, validity=None, n=None, offset=0):
    """exact_moments.moments of the widened column (Float64 patterns)"""
    return M.moments(np.asarray(b64, np.uint64).view(np.float64), validity, n, offset)


def distinct(raw, validity=None, n=None, offset=0):
    """(non_null, distinct, groups_once) by the ORIGINAL bits (any integer dtype; floats as their bit patterns)"""
    raw = np.asarray(raw)
    if raw.dtype.kind == "f":
        raw = raw.view({4: np.uint32, 8: np.uint64}[raw.dtype.itemsize])
    n = len(raw) - offset if n is None else n
    v = raw[offset:offset + n][_mask(n, validity, offset)]
    if len(v) == 0:
        return 0, 0, 0
    _, cnt = np.unique(v, return_counts=True)
    return len(v), len(cnt), int((cnt == 1).sum())


def hll_registers(b64, validity=None, n=None, offset=0):
    """the HyperLogLog registers of the injective widening (the oracle's hash of the 8-byte keys)"""
    import oracle_binding as orc

    b = np.ascontiguousarray(np.asarray(b64, np.uint64)).view(np.int64)
    return orc.hll_registers(b, validity, n=len(b) - offset if n is None else n, offset=offset)


def kll_kept(b64, validity=None, n=None, offset=0):
    """the sorted values a KLL sketch of the widened column holds to (NaN dropped)"""
    return Q.kept(np.asarray(b64, np.uint64).view(np.float64), validity, n, offset)


def rank_sums(kx, ky):
    """Spearman's state from sort keys (total_key of the CAST patterns, or Int64 values) of the valid pairs:
    min-rank RANK() of each side, the sums in UInt64 arithmetic that wraps, as the doubles the result reports"""
    kx, ky = np.asarray(kx, np.int64), np.asarray(ky, np.int64)
    rx = np.searchsorted(np.sort(kx), kx, side="left").astype(np.uint64) + np.uint64(1)
    ry = np.searchsorted(np.sort(ky), ky, side="left").astype(np.uint64) + np.uint64(1)
    with np.errstate(over="ignore"):  # (uint64 sums wrap modulo 2^64, as the reference's UInt64 SUM)
        sums = [np.sum(a * b, dtype=np.uint64) for a, b in ((rx, np.uint64(1)), (ry, np.uint64(1)), (rx, rx), (ry, ry), (rx, ry))]
    return (len(kx),) + tuple(float(int(s)) for s in sums)
