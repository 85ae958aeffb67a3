"""The HyperLogLog reference of tests/exact_hll.py, pinned on the CPU: the vectorised hash against the Python-int one,
registers and estimates against the oracle, the double estimator against the 60-digit one, and the hash's rank and
register distributions over 2^22 values of structured families against what HyperLogLog assumes."""
import math
import struct

import numpy as np
import pytest

import exact_hll as H
import exact_widening as W
import oracle_binding as orc


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


SPECIAL_BITS = [0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000,
                0x7FF0000000000001, 0x7FF4000000000BEE, 0xFFFFFFFFFFFFFFFF, 1, 0x000FFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF,
                0xFFFFFFFF, 1 << 32, (1 << 63) - 1, 0x3FF0000000000000, 0xBFF0000000000000]


def families(n):
    """uint64 patterns of the structured families the hash must spread"""
    i = np.arange(n, dtype=np.int64)
    return {
        "consecutive_int64": i.view(np.uint64),
        "epoch_millis": (np.int64(1_700_000_000_000) + i).view(np.uint64),
        "int32": W.widen_int((i - n // 2).astype(np.int32), "int32").view(np.uint64),
        "float32": W.widen_f32_bits(np.arange(n, dtype=np.float32) * np.float32(0.25)),
        "shifted_32": (i << 32).view(np.uint64),
    }


def test_vectorised_hash_equals_the_python_int_hash():
    rng = np.random.default_rng(1)
    vals = SPECIAL_BITS + rng.integers(0, 2**64, 3000, dtype=np.uint64, endpoint=False).tolist() + list(range(500)) + \
        [k << 32 for k in range(500)] + [(1 << 64) - 1 - k for k in range(100)]
    u = np.array(vals, dtype=np.uint64)
    a, b = H.hash_np(u)
    want = [H.hash_int(v) for v in vals]
    assert a.tolist() == [w[0] for w in want] and b.tolist() == [w[1] for w in want]
    r = H.ranks_np(b)
    assert r.tolist() == [H.rank_int(w[1]) for w in want]
    # the rank rule by hand: clz + 1, 33 for zero
    assert H.ranks_np(np.array([0, 1, 2, 3, 0x80000000, 0xFFFFFFFF, 0x00010000], np.uint32)).tolist() == \
        [33, 32, 31, 31, 1, 1, 16]
    assert [H.rank_int(b) for b in (0, 1, 0x80000000)] == [33, 32, 1]


def test_a_value_whose_b_is_zero_has_rank_33():
    """b == 0 (rank q + 1 = 33) happens once in 2^32 values: made on purpose by inverting the finaliser"""
    for hi in (0x12345678, 0, 0xFFFFFFFF):
        bits = H.value_with_b_zero(hi)
        a, b = H.hash_int(bits)
        assert b == 0 and bits >> 32 == hi and H.rank_int(b) == 33
        regs = H.registers(np.array([bits], np.uint64))
        assert regs[a & (H.M - 1)] == 33 and int(regs.sum()) == 33
        assert np.array_equal(regs, orc.hll_registers(np.array([bits], np.uint64).view(np.int64)))
        assert H.estimate_double(regs) == H.estimate_exact(regs) == orc.hll_estimate(regs) == 1


@pytest.mark.parametrize("data", ["random", "small_ints", "specials", "float_normal", "nulls_offset"])
def test_registers_equal_the_python_ints_and_the_oracle(data):
    rng = np.random.default_rng(hash(data) % 1000)
    n = 20_000
    validity, offset = None, 0
    if data == "random":
        u = rng.integers(0, 2**64, n, dtype=np.uint64, endpoint=False)
    elif data == "small_ints":
        u = rng.integers(-300, 300, n).astype(np.int64).view(np.uint64)
    elif data == "specials":
        u = np.array(SPECIAL_BITS * 50 + [0x7FF8000000000000 | k for k in range(1000)] +
                     [0xFFF0000000000000 | k for k in range(1, 1000)], dtype=np.uint64)
    elif data == "float_normal":
        u = np.round(rng.standard_normal(n), 2).view(np.uint64)
    else:
        u = rng.integers(0, 5000, n).astype(np.int64).view(np.uint64)
        mask = rng.random(n) >= 0.4
        validity = orc.pack_validity(mask)
        offset = 13
    m = len(u) - offset
    regs = H.registers(u, validity, n=m, offset=offset)
    keep = H.valid_rows(m, validity, offset)
    py = H.registers_int([int(v) if k else None for v, k in zip(u[offset:].tolist(), keep)])
    assert np.array_equal(regs, py)
    assert np.array_equal(regs, orc.hll_registers(u.view(np.int64), validity, n=m, offset=offset))
    assert H.estimate_double(regs) == orc.hll_estimate(regs)
    assert abs(H.estimate_double(regs) - H.estimate_exact(regs)) <= 1


def simulated_registers(rng, n):
    """registers as n ideal random values would leave them: uniform register, rank geometric with P(k) = 2^-k"""
    idx = rng.integers(0, H.M, n)
    b = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    regs = np.zeros(H.M, np.uint8)
    np.maximum.at(regs, idx, H.ranks_np(b))
    return regs


def crafted_registers():
    rng = np.random.default_rng(11)
    out = {"empty": np.zeros(H.M, np.uint8), "all_33": np.full(H.M, 33, np.uint8),
           "all_32": np.full(H.M, 32, np.uint8), "all_1": np.ones(H.M, np.uint8)}
    one = np.zeros(H.M, np.uint8)
    one[5] = 1
    out["one_register"] = one
    half = np.zeros(H.M, np.uint8)
    half[::2] = 2
    out["half_empty"] = half
    last_empty = np.full(H.M, 7, np.uint8)
    last_empty[-1] = 0
    out["one_empty"] = last_empty
    top = np.full(H.M, 20, np.uint8)
    top[:100] = 33
    out["some_33"] = top
    out["random_ranks"] = rng.integers(0, 34, H.M).astype(np.uint8)
    for n in (1, 2, 3, 100, 5000, 11000, 16384, 30000, 40000, 60000, 81920, 200_000, 10**6, 10**7, 10**9, 10**11):
        out["sim_%d" % n] = simulated_registers(rng, min(n, 3 * 10**7)) if n <= 10**7 else \
            np.clip(np.round(np.log2(n / H.M) + rng.standard_normal(H.M) * 1.2), 0, 33).astype(np.uint8)
    return out


CRAFTED = crafted_registers()


@pytest.mark.parametrize("name", list(CRAFTED))
def test_estimate_double_equals_the_oracle_and_the_60_digit_estimate(name):
    regs = CRAFTED[name]
    d = H.estimate_double(regs)
    assert d == orc.hll_estimate(regs), (name, d, orc.hll_estimate(regs))
    if name == "all_33":  # z = 0 in both: no finite estimate (0 by the library's rule); all ranks beyond q
        assert d == 0
        return
    e = H.estimate_exact(regs)
    assert abs(d - e) <= 1, (name, d, e, H.estimate_exact_value(regs))
    if name == "empty":
        assert d == e == 0
    if name == "one_register":
        assert d == e == 1
    if name.startswith("sim_") and int(name[4:]) <= 10**7:
        n = int(name[4:])
        assert abs(e - n) <= H.rel_bound(n) * n, (name, e)


def test_sigma_and_tau_in_doubles_against_decimal():
    import decimal

    xs = [0.0, 1e-300, 1e-9, 1.0 / H.M, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1 - 1.0 / H.M, 1 - 1e-9]
    xs += [k / H.M for k in range(1, H.M, 97)]
    for x in xs:
        with decimal.localcontext() as ctx:
            ctx.prec = H.DIGITS
            s, t = H.sigma_decimal(x), H.tau_decimal(x)
        sd, td = H.sigma_double(x), H.tau_double(x)
        # (x^(2^k) by k squarings: the rounding of x grows 2^k-fold, and the terms matter up to 2^k ~ 1 / (1 - x))
        assert abs(sd - float(s)) <= 16 * 2**-53 / (1 - x) * float(s) + 1e-320, (x, sd, s)
        assert abs(td - float(t)) <= 1e-14 * float(t) + 1e-300, (x, td, t)
    assert H.sigma_double(1.0) == math.inf and H.sigma_decimal(1).is_infinite()
    assert H.tau_double(0.0) == H.tau_double(1.0) == 0.0
    # the series by hand: sigma(1/2) = 1/2 + 1/4 + 2/16 + 4/256 + ...; tau(x) -> (1 - x) / 3 - ... < (1 - x) / 3
    assert abs(H.sigma_double(0.5) - (0.5 + 0.25 + 0.125 + 4 / 256 + 8 / 65536 + 16 / 2**32)) < 1e-15
    assert 0 < H.tau_double(0.5) < 0.5 / 3


def chi_square(observed, expected):
    return float((((observed - expected) ** 2) / expected).sum())


@pytest.mark.parametrize("family", ["consecutive_int64", "epoch_millis", "int32", "float32", "shifted_32"])
def test_rank_and_register_distributions_of_structured_families(family):
    """2^22 distinct values: rank k with probability 2^-k (the tail from rank 18 on pooled), registers uniform"""
    from scipy.stats import chi2

    n = 1 << 22
    u = families(n)[family]
    assert len(np.unique(u)) == n
    idx, rank = H.index_and_rank(u)
    counts = np.bincount(rank.astype(np.int64), minlength=H.MAX_RANK + 1)
    assert counts[0] == 0 and counts.sum() == n
    kmax = 17
    obs = np.append(counts[1: kmax + 1], counts[kmax + 1:].sum()).astype(np.float64)
    exp = np.array([n * 2.0 ** -k for k in range(1, kmax + 1)] + [n * 2.0 ** -kmax])
    stat = chi_square(obs, exp)
    assert stat < chi2.isf(1e-6, len(obs) - 1), (family, stat, obs[:8], exp[:8])
    per_reg = np.bincount(idx, minlength=H.M).astype(np.float64)
    stat = chi_square(per_reg, np.full(H.M, n / H.M))
    assert stat < chi2.isf(1e-6, H.M - 1), (family, stat)
    # and the estimate of the family is within the bound
    regs = H.registers(u)
    e = H.estimate_double(regs)
    assert abs(e - n) <= H.rel_bound(n) * n, (family, e)


def test_rel_bound():
    assert H.rel_bound(0) == 0.0
    assert H.rel_bound(1) >= 1.0 and H.rel_bound(2) >= 0.5  # a count is always allowed its rounding
    big = H.rel_bound(10**7)
    assert abs(big - 4 * 1.04 / 128) < 1e-6
    # linear counting's smaller error while most registers are empty, HyperLogLog's beyond
    assert H.rel_bound(3000) < big and H.rel_bound(16384) < big
    assert all(H.rel_bound(n) <= big + 1.0 / n for n in (10, 100, 10**4, 10**5, 10**6))
