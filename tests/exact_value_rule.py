"""A plain-Python reference for TGX_CHECK_VALUE_RULE: the numeric predicates of the reference's DataTypeConstraint
(TG/constraints/datatype.rs:144-160), each evaluated by

    SELECT COUNT(*) AS total, SUM(CASE WHEN <predicate> THEN 1 ELSE 0 END) AS valid FROM t WHERE col IS NOT NULL

`counts` is a literal per-row walk: integer values are Python ints, floats are their 64-bit patterns (Python ints again,
so a NaN keeps its sign and payload) compared through IEEE totalOrder keys, and CAST(col AS DOUBLE) is float(int), which
rounds to nearest-even.  `counts_np` is the numpy twin for large tables; tests/test_exact_value_rule.py holds the two
against each other.  Both return (seen, considered, valid, cast_errors).

The rules (include/tgx.h states them as the contract).  A row's value is an int64 when the column's Arrow type is an
integer type and a double when it is Float32 / Float64; a NULL row is seen and never considered.  arrow-ord orders floats
by totalOrder, for `=` as well:  -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN.

    GE_ZERO   integer: v >= 0             float: key(x) >= key(+0.0)
    GT_ZERO   integer: v > 0              float: key(x) >  key(+0.0)
    BETWEEN   integer, no flag: lo_i <= v <= hi_i
              BOUNDS_AS_DOUBLE or a float column: key(lo_f) <= key((double)v) <= key(hi_f)
    INTEGER   col = CAST(col AS INT), INT = Int32.  A cast error: an integer outside [-2^31, 2^31 - 1]; a float that is
              NaN or +-inf, or whose truncation toward zero lies outside that range.  A row that casts is valid iff
              key(x) == key((double)(int32)trunc(x)) (integers: always).  A cast error is considered and not valid.
"""
import math
import struct

import numpy as np

import exact_widening as W

GE_ZERO, GT_ZERO, BETWEEN, INTEGER = 1, 2, 3, 4
BOUNDS_AS_DOUBLE = 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
_LOW63 = (1 << 63) - 1


def bits_of(x):
    """the 64-bit pattern of a Python float, as a signed int"""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def float_of(bits):
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def key(bits):
    """the totalOrder key of a pattern: k ^ ((k >> 63) & 0x7fff..ff) on signed 64-bit k"""
    return bits ^ _LOW63 if bits < 0 else bits


KEY_ZERO = key(bits_of(0.0))  # 0


def rule(mode, flags=0, lo_i=0, hi_i=0, lo_f=0.0, hi_f=0.0):
    return {"mode": mode, "flags": flags, "lo_i": lo_i, "hi_i": hi_i, "lo_f": lo_f, "hi_f": hi_f}


def _bound_key(x):
    """a double bound, given as a float or (for NaN payloads) as its pattern wrapped in a 1-tuple"""
    return key(x[0] if isinstance(x, tuple) else bits_of(x))


def judge(r, v, is_float):
    """one non-NULL row: (valid, cast_error).  v: a Python int, the value of an integer column or the pattern of a
    float one"""
    mode = r["mode"]
    if mode in (GE_ZERO, GT_ZERO):
        k, zero = (key(v), KEY_ZERO) if is_float else (v, 0)
        return (k >= zero if mode == GE_ZERO else k > zero), False
    if mode == BETWEEN:
        if is_float or (r["flags"] & BOUNDS_AS_DOUBLE):
            k = key(v) if is_float else key(bits_of(float(v)))
            return _bound_key(r["lo_f"]) <= k <= _bound_key(r["hi_f"]), False
        return r["lo_i"] <= v <= r["hi_i"], False
    if mode == INTEGER:
        if not is_float:
            fits = I32_MIN <= v <= I32_MAX
            return fits, not fits
        x = float_of(v)
        if math.isnan(x) or math.isinf(x):
            return False, True
        t = math.trunc(x)
        if not I32_MIN <= t <= I32_MAX:
            return False, True
        return key(v) == key(bits_of(float(t))), False
    raise ValueError(mode)


def counts(r, values, valid=None, is_float=False):
    """values: a sequence of Python ints (float columns: patterns); valid: a sequence of bools or None (no NULLs)"""
    seen = considered = ok = errors = 0
    for i, v in enumerate(values):
        seen += 1
        if valid is not None and not valid[i]:
            continue
        considered += 1
        passes, cast_error = judge(r, int(v), is_float)
        ok += bool(passes)
        errors += bool(cast_error)
    return seen, considered, ok, errors


# ---- the numpy twin ---------------------------------------------------------------------------------------------------
def _np_key(bits):
    return W.total_key(np.asarray(bits).view(np.uint64))


def _i64_to_f64_bits(v):
    """CAST(Int64 AS DOUBLE): numpy's astype rounds to nearest-even, as the C conversion does"""
    return v.astype(np.float64).view(np.int64)


def counts_np(r, values, mask=None):
    """values: an np.int64 array (integer column) or an np.float64 array (float column; patterns are kept); mask: bools
    or None"""
    values = np.asarray(values)
    is_float = values.dtype == np.float64
    if not is_float and values.dtype != np.int64:
        raise TypeError("widen first: %s" % values.dtype)
    n = len(values)
    live = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    bits = values.view(np.int64)
    mode = r["mode"]
    errors = np.zeros(n, bool)
    if mode in (GE_ZERO, GT_ZERO):
        k = _np_key(bits) if is_float else bits
        ok = k >= 0 if mode == GE_ZERO else k > 0
    elif mode == BETWEEN:
        if is_float or (r["flags"] & BOUNDS_AS_DOUBLE):
            k = _np_key(bits if is_float else _i64_to_f64_bits(bits))
            ok = (k >= _bound_key(r["lo_f"])) & (k <= _bound_key(r["hi_f"]))
        else:
            lo, hi = r["lo_i"], r["hi_i"]
            ok = (bits >= lo) & (bits <= hi) if lo <= hi else np.zeros(n, bool)
    elif mode == INTEGER:
        if is_float:
            x = bits.view(np.float64)
            with np.errstate(invalid="ignore"):
                fits = (x > -2147483649.0) & (x < 2147483648.0)  # (a NaN fails both)
                t = np.trunc(np.where(fits, x, 0.0))
            errors = ~fits
            ok = fits & (t.astype(np.int64).astype(np.float64).view(np.int64) == bits)
        else:
            errors = (bits < I32_MIN) | (bits > I32_MAX)
            ok = ~errors
    else:
        raise ValueError(mode)
    return n, int(live.sum()), int((ok & live).sum()), int((errors & live).sum())


def widen(raw, type_name):
    """a narrow column's raw values -> what the rules see: int64 values, or float64 with a Float32's NaN sign and payload
    kept (exact_widening)"""
    if type_name == "float32":
        return W.widen_f32_bits(np.asarray(raw, np.float32).view(np.uint32)).view(np.float64)
    if type_name in W.INT_WIDTH:
        return W.widen_int(raw, type_name)
    raise ValueError(type_name)


# ---- the constraint's verdict (datatype.rs:424-438) -------------------------------------------------------------------
def rust_f64(x):
    """Rust's `{}` for f64: shortest round-trip digits, no exponent"""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    if x == int(x) and abs(x) < 1e16:
        return ("-" if math.copysign(1.0, x) < 0 else "") + str(abs(int(x)))
    s = repr(x)
    if "e" in s or "E" in s:
        from decimal import Decimal

        s = format(Decimal(s), "f")
    return s


def description(validation, **kw):
    if validation == "non_negative":
        return "non-negative values"
    if validation == "positive":
        return "positive values"
    if validation == "integer":
        return "integer values"
    if validation == "range":
        return "values between %s and %s" % (rust_f64(kw["min"]), rust_f64(kw["max"]))
    raise ValueError(validation)


def verdict(considered, valid, text):
    """(status, metric, message) as ValidationSuite reports them: a Success carries no message"""
    rate = valid / considered if considered else float("nan")
    if rate >= 1.0:
        return "Success", rate, None
    pct = "NaN" if math.isnan(rate) else "%.1f" % (rate * 100.0)
    return "Failure", rate, "%s%% of values satisfy %s" % (pct, text)


def classify_bound(b):
    """how DataFusion reads the bound the reference prints with `{}`: ("int", i), ("float", x), or ("error", why)"""
    if math.isnan(b) or math.isinf(b):
        return "error", "not a SQL literal"
    if b == math.floor(b):
        if abs(b) <= 2.0 ** 53:
            return "int", int(b)
        return "error", "an integral bound beyond 2^53"
    return "float", b


def range_params(lo, hi):
    """Range {min, max} -> the rule, or None where the constraint errs"""
    a, b = classify_bound(lo), classify_bound(hi)
    if "error" in (a[0], b[0]):
        return None
    if "float" in (a[0], b[0]):
        return rule(BETWEEN, BOUNDS_AS_DOUBLE, 0, 0, float(a[1]), float(b[1]))
    return rule(BETWEEN, 0, a[1], b[1], float(a[1]), float(b[1]))
