"""The widening reference of tests/exact_widening.py pinned on the CPU: against numpy's conversion wherever that one is
exact (every non-NaN pattern), against struct's round trips, against a brute force on every pattern of the exponent
edges, and injective on every NaN and subnormal pattern."""
import math
import struct

import numpy as np
import pytest

import exact_widening as W

ALL_NAN_F32 = np.concatenate([np.arange(0x7F800001, 0x80000000, dtype=np.uint64),
                              np.arange(0xFF800001, 0x100000000, dtype=np.uint64)]).astype(np.uint32)
ALL_SUB_F32 = np.concatenate([np.arange(1, 0x800000, dtype=np.uint64),
                              np.arange(0x80000001, 0x80800000, dtype=np.uint64)]).astype(np.uint32)


def brute(u):
    """one pattern at a time, from the definition: (-1)^s 2^(e-150) (2^23 + m), or 2^-149 m, in exact integers"""
    s, e, m = u >> 31, (u >> 23) & 0xFF, u & 0x7FFFFF
    if e == 0xFF:
        return (s << 63) | (0x7FF << 52) | (m << 29)
    if e == 0 and m == 0:
        return s << 63
    sig, exp = (m, -149) if e == 0 else ((1 << 23) | m, e - 150)
    while sig < (1 << 52):  # normalise: 53 significant bits
        sig <<= 1
        exp -= 1
    return (s << 63) | ((exp + 52 + 1023) << 52) | (sig - (1 << 52))


def test_agrees_with_numpy_on_every_non_nan_pattern_of_a_sample():
    rng = np.random.default_rng(0)
    u = rng.integers(0, 2 ** 32, size=2_000_000, dtype=np.uint64).astype(np.uint32)
    u = np.concatenate([u, ALL_SUB_F32[::97], np.array([0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF,
                                                        0x00800000, 0x80800000, 0x007FFFFF, 0x00000001], np.uint32)])
    u = u[(u & 0x7FFFFFFF) <= 0x7F800000]
    want = u.view(np.float32).astype(np.float64).view(np.uint64)
    assert np.array_equal(W.widen_f32_bits(u), want)
    assert np.array_equal(W.cast_f32_bits(u), want)


def test_struct_round_trips():
    rng = np.random.default_rng(1)
    for u in [int(x) for x in rng.integers(0, 2 ** 32, size=20_000, dtype=np.uint64)] + [1, 0x807FFFFF, 0x7F7FFFFF]:
        f = struct.unpack("<f", struct.pack("<I", u))[0]
        w = int(W.widen_f32_bits(np.array([u], np.uint32))[0])
        d = struct.unpack("<d", struct.pack("<Q", w))[0]
        if math.isnan(f):
            assert math.isnan(d) and (w >> 63) == (u >> 31)
            continue
        assert d == f and math.copysign(1, d) == math.copysign(1, f)
        assert struct.unpack("<I", struct.pack("<f", d))[0] == u  # narrowing back is exact and gives the pattern


@pytest.mark.parametrize("hi", [0x0000, 0x0080, 0x7F80, 0x7F00, 0x8000, 0x8080, 0xFF80, 0xFF00, 0x7FC0, 0xFFC0])
def test_brute_force_on_all_2_16_patterns_of_the_exponent_edges(hi):
    """the top 16 bits fixed (sign, exponent 0 / 1 / 254 / 255, the quiet bit), the low 16 all taken"""
    for mid in (0, 0x3F, 0x7F):
        u = ((hi | mid) << 16) + np.arange(0, 2 ** 16, dtype=np.uint64)
        got = W.widen_f32_bits(u.astype(np.uint32))
        assert [int(x) for x in got] == [brute(int(x)) for x in u]
        nan = (u & 0x7FFFFFFF) > 0x7F800000
        want_cast = np.where(nan, got | np.uint64(W.F64_QUIET), got)
        assert np.array_equal(W.cast_f32_bits(u.astype(np.uint32)), want_cast)


def test_nan_map_keeps_sign_payload_and_quiet_bit_and_is_injective():
    w = W.widen_f32_bits(ALL_NAN_F32)
    assert len(np.unique(w)) == len(ALL_NAN_F32) == 2 * (2 ** 23 - 1)
    assert W.is_nan_bits(w).all()
    u = ALL_NAN_F32.astype(np.uint64)
    assert np.array_equal(w >> np.uint64(63), u >> np.uint64(31))
    assert np.array_equal((w >> np.uint64(51)) & np.uint64(1), (u >> np.uint64(22)) & np.uint64(1))
    assert np.array_equal(w & np.uint64((1 << 29) - 1), np.zeros_like(w))
    # the hardware conversion does not keep them apart: the reason this reference exists
    with np.errstate(invalid="ignore"):
        hw = ALL_NAN_F32.view(np.float32).astype(np.float64).view(np.uint64)
    assert len(np.unique(hw)) < len(ALL_NAN_F32)
    c = W.cast_f32_bits(ALL_NAN_F32)
    assert len(np.unique(c)) == 2 ** 23  # sNaN p meets qNaN p: 2 signs x 2^22 low payload bits
    assert ((c & np.uint64(W.F64_QUIET)) != 0).all()


def test_subnormals_are_exact_and_injective():
    w = W.widen_f32_bits(ALL_SUB_F32)
    assert len(np.unique(w)) == len(ALL_SUB_F32)
    d = w.view(np.float64)
    m = (ALL_SUB_F32 & 0x7FFFFF).astype(np.float64)
    sign = np.where(ALL_SUB_F32 >> 31, -1.0, 1.0)
    assert np.array_equal(d, sign * np.ldexp(m, -149))  # m 2^-149 is a normal double: ldexp is exact
    # the order of the patterns is the order of the values
    pos = W.widen_f32_bits(np.arange(0, 0x00800001, dtype=np.uint32)).view(np.float64)
    assert (np.diff(pos) > 0).all()


def test_total_key_and_minmax_order_every_class():
    u = np.array([0xFFFFFFFF, 0xFF800001, 0xFF800000, 0xFF7FFFFF, 0x80000001, 0x80000000, 0, 1, 0x7F7FFFFF, 0x7F800000,
                  0x7F800001, 0x7FC00000, 0x7FFFFFFF], np.uint32)
    k = W.total_key(W.widen_f32_bits(u))
    assert (np.diff(k) > 0).all()
    lo, hi = W.minmax_bits(W.widen_f32_bits(u[::-1]))
    assert (lo, hi) == (0xFFFFFFFFE0000000, 0x7FFFFFFFE0000000)


@pytest.mark.parametrize("name,dtype", [("int8", np.int8), ("int16", np.int16), ("int32", np.int32),
                                        ("uint8", np.uint8), ("uint16", np.uint16), ("uint32", np.uint32)])
def test_widen_int_over_the_whole_domain_or_its_edges(name, dtype):
    info = np.iinfo(dtype)
    if info.bits <= 16:
        v = np.arange(int(info.min), int(info.max) + 1, dtype=np.int64)
    else:
        v = np.array([info.min, info.min + 1, -1 if info.min else 0, 0, 1, 2 ** 31 - 1, info.max - 1, info.max], np.int64)
        v = v[(v >= info.min) & (v <= info.max)]
        if not info.min:
            v = np.concatenate([v, [2 ** 31, 2 ** 31 + 1]])
    got = W.widen_int(v.astype(dtype), name)
    assert [int(x) for x in got] == [int(x) for x in v]


@pytest.mark.parametrize("bit_offset", range(8))
def test_boolean_bits_at_every_offset(bit_offset):
    rng = np.random.default_rng(bit_offset)
    bools = rng.random(203) < 0.4
    buf = np.packbits(np.concatenate([np.zeros(bit_offset, bool), bools]), bitorder="little")
    assert np.array_equal(W.widen_int(buf, "bool", n=len(bools), bit_offset=bit_offset), bools.astype(np.int64))


def test_answers_per_check_kind():
    u = np.array([0x7F800001, 0x7FC00001, 0x7FC00001, 0x00000001, 0x80000000, 0, 0x3F800000], np.uint32)
    valid = np.packbits(np.array([1, 1, 1, 1, 1, 1, 0], bool), bitorder="little")
    # by the original bits: the two NaNs and the two zeros are four keys, the repeated qNaN is not once
    assert W.distinct(u.view(np.float32), valid) == (6, 5, 4)
    assert W.count(7, valid) == (7, 6)
    b = W.widen_f32_bits(u)
    lo, hi = W.minmax_bits(b, valid)
    assert (lo, hi) == (0x8000000000000000, 0x7FF8000020000000)
    assert [float(x) for x in W.kll_kept(b, valid)] == [-0.0, 0.0, 2.0 ** -149]
    assert W.int_stats(np.array([2 ** 62, 2 ** 62, -5], np.int64)) == (3, -5, 2 ** 62, 2 ** 63 - 5)
    # RANK(): ties take the lowest rank; the CAST NaNs of the same payload tie
    kx = W.total_key(W.cast_f32_bits(np.array([0x7F800001, 0x7FC00001, 0x3F800000], np.uint32)))
    ky = np.array([3, 2, 1], np.int64)
    assert W.rank_sums(kx, ky) == (3, 5.0, 6.0, 9.0, 14.0, 2 * 3 + 2 * 2 + 1 * 1.0)
