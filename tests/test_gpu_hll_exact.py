"""-m gpu: APPROX_DISTINCT against the independent reference of tests/exact_hll.py, on every route the lane takes.

Each result is held to three things: the device's registers equal exact_hll.registers of the widened values byte for
byte (where the blob shows them), the estimate equals exact_hll.estimate_double of those registers (which lies within 1
of the 60-digit estimate), and the estimate lies within exact_hll.rel_bound of the true count.

Routes (update.cpp): the lane alone (skip_stats) or next to NUMERIC_STATS / KLL; launch_scan_hll folds the workgroups'
register rows with 1, 4 or 32 slices by blocks_per_col (< 8, 8 .. 63, >= 64; one column of 8192 B aligned rows takes
B workgroups); ragged Arrow offsets, HOST batches, coalesced 8192-row streams, finalize half-way, reset, merges, blobs
and threaded ranks.  Where the lane does not apply the exact key set answers with the exact count."""
import numpy as np
import pytest

import exact_hll as H
import exact_widening as W
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import numeric_column
from test_gpu_numeric32 import col32

pytestmark = pytest.mark.gpu

NAN_BITS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FF4DEADBEEF0000, 0xFFF0000000000ABC]
KINDS = ["consecutive", "epoch_ms", "int32", "float32", "shift32", "float64_specials", "b_zero"]


def values(kind, n, rng):
    """n rows of a column of the family (its values distinct but for float64_specials' zeros and NaN payloads)"""
    i = np.arange(n, dtype=np.int64)
    if kind == "consecutive":
        return i + int(rng.integers(-10 ** 12, 10 ** 12))
    if kind == "epoch_ms":
        return np.int64(1_700_000_000_000) + i * int(rng.integers(1, 1000))
    if kind == "int32":
        return (i - n // 2 + int(rng.integers(-1000, 1000))).astype(np.int32)
    if kind == "float32":  # (exact up to 2^24 rows: halves below 2^23)
        return i.astype(np.float32) * np.float32(0.5) - np.float32(1000.0)
    if kind == "shift32":
        return (i + int(rng.integers(0, 1000))) << 32
    if kind == "float64_specials":
        x = rng.standard_normal(n) * 1e6
        bits = x.view(np.uint64)
        at = rng.random(n) < 0.02
        bits[at] = np.array(NAN_BITS + [0, 1 << 63, 0x7FF0000000000000, 0xFFF0000000000000, 1], np.uint64)[
            rng.integers(0, len(NAN_BITS) + 5, int(at.sum()))]
        return x
    if kind == "b_zero":  # consecutive values, the first three replaced by values whose b is 0 (rank q + 1 = 33)
        return np.concatenate([zero_b(min(n, 3), 7), i[3:] + 1000])
    raise ValueError(kind)


def zero_b(count, seed):
    """`count` Int64 values of rank 33 in as many registers (their register is bits 16 .. 29 of the high half, which
    starts from 2^31: none of them is a small integer)"""
    hi = [(1 << 31) | (((seed * 977 + 7919 * k) & (H.M - 1)) << 16) | k for k in range(count)]
    return np.array([H.value_with_b_zero(h) for h in hi], dtype=np.uint64).view(np.int64)


def bits_of(vals):
    """the 64-bit patterns the registers are made of"""
    if vals.dtype == np.int32:
        return W.widen_int(vals, "int32").view(np.uint64)
    if vals.dtype == np.float32:
        return W.widen_f32_bits(vals)
    return np.ascontiguousarray(vals).view(np.uint64)


def column(vals, validity, device=True, offset=0, length=None):
    if vals.dtype in (np.int32, np.float32):
        return col32(vals, validity, device, offset=offset, length=length)
    return numeric_column(vals, validity, device, offset=offset, length=length)


def registers_of(state):
    """the last HyperLogLog task's registers: the tail of the state blob (term_amd/wire.py)"""
    return np.frombuffer(state.serialize()[-H.M:], dtype=np.uint8)


def true_count(bits, validity=None, n=None, offset=0):
    n = len(bits) - offset if n is None else n
    return len(np.unique(bits[offset: offset + n][H.valid_rows(n, validity, offset)]))


def check(r, vals, validity=None, n=None, offset=0, regs=None, accuracy=True, counts=True):
    """r: the APPROX_DISTINCT result of rows offset .. offset + n; regs: the device's registers, if known; accuracy:
    hold the estimate to rel_bound of the true count; counts: check total / non_null.  Returns the signed relative
    error of the estimate."""
    bits = bits_of(vals)
    n = len(bits) - offset if n is None else n
    want = H.registers(bits, validity, n=n, offset=offset)
    if regs is not None:
        diff = np.nonzero(regs != want)[0]
        assert len(diff) == 0, "registers differ at %d places, e.g. %s: %s != %s" % (
            len(diff), diff[:4].tolist(), regs[diff[:4]].tolist(), want[diff[:4]].tolist())
    d = H.estimate_double(want)
    assert r.distinct == d, (r.distinct, d)
    assert abs(d - H.estimate_exact(want)) <= 1
    if counts:
        assert (r.total, r.non_null) == (n, int(H.valid_rows(n, validity, offset).sum()))
    true = true_count(bits, validity, n, offset)
    if not accuracy:
        return 0.0
    assert abs(r.distinct - true) <= H.rel_bound(true) * true, (r.distinct, true, H.rel_bound(true))
    return (r.distinct - true) / true if true else 0.0


def run(specs, batches):
    T.init()
    st = T.State(T.Plan(specs))
    for cols in batches:
        st.update(cols)
    return st.finalize(), st


# ---- the estimator itself: registers of any shape through a blob ----------------------------------------------------
def test_estimate_of_crafted_registers_equals_the_reference():
    """every histogram of tests/test_exact_hll.py's CRAFTED set (empty, one register, all 32, all 33, simulated n from
    1 to 10^11) put into a state blob: the library's estimate is estimate_double's"""
    from test_exact_hll import CRAFTED

    T.init()
    plan = T.Plan([spec(T.APPROX_DISTINCT, 0)])
    st = T.State(plan)
    st.update([numeric_column(np.arange(100, dtype=np.int64), None, True)])
    blob = st.serialize()
    head = blob[:-H.M]
    assert np.array_equal(np.frombuffer(blob[-H.M:], np.uint8), H.registers(np.arange(100, dtype=np.int64)))
    for name, regs in CRAFTED.items():
        back = T.State.deserialize(plan, head + regs.tobytes())
        got = back.finalize()[0].distinct
        assert got == H.estimate_double(regs), (name, got, H.estimate_double(regs))


# ---- cardinalities x families ---------------------------------------------------------------------------------------
SWEEP = [0, 1, 2, 3, 100, 5000, 11_000, 16_384, 30_000, 40_960, 5 * 16_384, 200_000, 10 ** 6]


@pytest.mark.parametrize("n", SWEEP)
@pytest.mark.parametrize("kind", KINDS)
def test_cardinality_sweep(kind, n):
    rng = np.random.default_rng([KINDS.index(kind), n])
    vals = values(kind, n, rng)
    # the lane alone (column 0), and the same values next to NUMERIC_STATS (column 1)
    res, st = run([spec(T.APPROX_DISTINCT, 0), spec(T.APPROX_DISTINCT, 1), spec(T.NUMERIC_STATS, 1)],
                  [[column(vals, None), column(vals, None)]])
    check(res[0], vals)
    check(res[1], vals, regs=registers_of(st) if n else None)


@pytest.mark.parametrize("kind", ["consecutive", "float64_specials", "int32"])
def test_ten_million(kind):
    n = 10 ** 7
    vals = values(kind, n, np.random.default_rng(7))
    validity = orc.pack_validity(np.random.default_rng(8).random(n) >= 0.01)
    res, st = run([spec(T.APPROX_DISTINCT, 0)], [[column(vals, validity)]])
    check(res[0], vals, validity, regs=registers_of(st))


def test_mean_signed_error_stays_near_zero():
    """48 disjoint sets of 100 000 .. 400 000 distinct values: each estimate within the bound, their mean signed
    relative error within four standard errors of the mean"""
    rng = np.random.default_rng(99)
    errs = []
    T.init()
    plan = T.Plan([spec(T.APPROX_DISTINCT, 0)])
    for k in range(48):
        kind = KINDS[k % 6]
        n = int(rng.integers(100_000, 400_000))
        vals = values(kind, n, rng)
        # (sets of one family kept apart from each other: 48 independent estimates)
        vals = {"consecutive": lambda: vals + k * (1 << 40), "epoch_ms": lambda: vals + k * (1 << 40),
                "int32": lambda: vals + np.int32(k * 1_000_000), "float32": lambda: vals * np.float32(1 + k / 7),
                "shift32": lambda: vals + (k << 20), "float64_specials": lambda: vals}[kind]()
        st = T.State(plan)
        st.update([column(vals, None)])
        errs.append(check(st.finalize()[0], vals))
    mean = float(np.mean(errs))
    assert abs(mean) <= 4 * H.RSE / np.sqrt(len(errs)), (mean, errs)


# ---- validity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["all_null", "sparse", "first_half", "one_valid"])
@pytest.mark.parametrize("kind", ["consecutive", "float32", "float64_specials"])
def test_validity(kind, layout):
    n = 300_001
    rng = np.random.default_rng([KINDS.index(kind), len(layout)])
    vals = values(kind, n, rng)
    r = np.arange(n)
    mask = {"all_null": np.zeros(n, bool), "sparse": rng.random(n) < 0.003, "first_half": r >= n // 2,
            "one_valid": r == n - 1}[layout]
    validity = orc.pack_validity(mask)
    res, st = run([spec(T.APPROX_DISTINCT, 0), spec(T.COUNT, 0)], [[column(vals, validity)]])
    check(res[0], vals, validity, regs=registers_of(st) if mask.any() else None)
    if layout == "all_null":
        assert res[0].distinct == 0
    if layout == "one_valid":
        assert res[0].distinct == 1


# ---- workgroups per column: the reduce's slices -----------------------------------------------------------------------
@pytest.mark.parametrize("blocks", [1, 7, 8, 63, 64, 367])
@pytest.mark.parametrize("offset", [0, 3])
def test_blocks_per_column(blocks, offset):
    """8192 B aligned rows are B workgroups of the lane (scan_blocks_for: 16 tiles of 512 rows each), folded with 1
    slice below 8, 4 up to 63, 32 from 64 on; an odd Arrow offset takes the ragged per-lane path instead"""
    n = 8192 * blocks
    rng = np.random.default_rng(blocks)
    vals = rng.permutation(n + offset).astype(np.int64) * 5 + 11
    res, st = run([spec(T.APPROX_DISTINCT, 0)], [[numeric_column(vals, None, True, offset=offset, length=n)]])
    check(res[0], vals, None, n=n, offset=offset, regs=registers_of(st))
    # the same with the last workgroup's rows alone holding rank-33 values: those registers' maximum sits in the
    # last row of the reduce's last slice (the estimate is not held to the true count: 64 ranks of 33 are no sample)
    both = np.concatenate([vals[: n + offset - 64], zero_b(64, blocks)])
    res, st = run([spec(T.APPROX_DISTINCT, 0)], [[numeric_column(both, None, True, offset=offset, length=n)]])
    regs = registers_of(st)
    check(res[0], both, None, n=n, offset=offset, regs=regs, accuracy=False)
    assert (regs == 33).sum() >= 60


# ---- next to other checks ----------------------------------------------------------------------------------------------
def test_next_to_numeric_stats_and_kll():
    n = 2_000_003
    rng = np.random.default_rng(5)
    vals = values("float64_specials", n, rng)
    validity = orc.pack_validity(rng.random(n) >= 0.1)
    res, st = run([spec(T.KLL, 0, kll_k=200), spec(T.NUMERIC_STATS, 0), spec(T.APPROX_DISTINCT, 0)],
                  [[column(vals, validity, offset=0, length=n // 2)],
                   [column(vals, validity, offset=n // 2, length=n - n // 2)]])
    check(res[2], vals, validity, regs=registers_of(st))
    o = orc.stats(vals, validity)
    assert res[1].non_null == o.non_null and orc.nan_equal(res[1].min_f, o.min_f) and orc.nan_equal(res[1].max_f, o.max_f)
    import exact_quantiles as Q

    Q.check_sketch(st, 0, Q.kept(vals, validity), 200, result=res[0])


def test_exact_key_set_route_gives_the_exact_count():
    import pyarrow as pa

    rng = np.random.default_rng(3)
    n = 300_000
    vals = values("float64_specials", n, rng)
    vals[n // 2:] = vals[: n - n // 2]  # duplicates
    true = true_count(bits_of(vals))
    for specs in ([spec(T.APPROX_DISTINCT, 0), spec(T.DISTINCT, 0)],
                  [spec(T.APPROX_DISTINCT, 0), spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE)]):
        res, _ = run(specs, [[numeric_column(vals, None, True)]])
        assert res[0].distinct == true and res[0].non_null == n
    words = ["v%d" % (i % 12345) for i in range(100_000)] + [None] * 7
    res, _ = run([spec(T.APPROX_DISTINCT, 0)], [[T.Column.from_arrow(pa.array(words, type=pa.string()))]])
    assert (res[0].distinct, res[0].non_null) == (12345, 100_000)


# ---- batches, streams and the life of a state ---------------------------------------------------------------------------
def test_ragged_batches_and_host_buffers():
    n = 1_500_000
    rng = np.random.default_rng(11)
    vals = values("epoch_ms", n, rng)
    validity = orc.pack_validity(rng.random(n) >= 0.05)
    cuts = [0, 1, 8, 1031, 1031 + 4097, 70_000, 70_001, 600_000, 1_100_003, n]
    T.init()
    plan = T.Plan([spec(T.APPROX_DISTINCT, 0), spec(T.COUNT, 0)])
    st = T.State(plan)
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        st.update([column(vals, validity, device=k % 2 == 0, offset=a, length=b - a)])
    check(st.finalize()[0], vals, validity, regs=registers_of(st))


@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("device", [True, False])
def test_streams_of_8192_rows(device, coalesce):
    try:
        T.init(flags=0 if coalesce else T.OPT_NO_COALESCE)
        for kind in ("int32", "float32", "consecutive"):
            n = 300_007
            rng = np.random.default_rng([device, coalesce, KINDS.index(kind)])
            vals = values(kind, n, rng)
            validity = orc.pack_validity(rng.random(n) >= 0.02)
            st = T.State(T.Plan([spec(T.APPROX_DISTINCT, 0)]))
            for a in range(0, n, 8192):
                st.update([column(vals, validity, device, offset=a, length=min(n, a + 8192) - a)])
            check(st.finalize()[0], vals, validity, regs=registers_of(st))
    finally:
        T.init()


def test_finalize_half_way_then_more_then_reset():
    n = 1_000_000
    rng = np.random.default_rng(21)
    vals = values("shift32", n, rng)
    T.init()
    st = T.State(T.Plan([spec(T.APPROX_DISTINCT, 0)]))
    st.update([column(vals, None, offset=0, length=n // 3)])
    check(st.finalize()[0], vals[: n // 3], regs=registers_of(st))
    st.update([column(vals, None, offset=n // 3, length=n - n // 3)])
    st.sync()
    check(st.finalize()[0], vals, regs=registers_of(st))
    st.reset()
    assert st.finalize()[0].distinct == 0
    st.update([column(vals[:5000], None)])
    check(st.finalize()[0], vals[:5000], regs=registers_of(st))


def test_merges_in_two_orders_with_an_empty_state_and_a_blob():
    n = 900_000
    rng = np.random.default_rng(31)
    vals = values("float64_specials", n, rng)
    validity = orc.pack_validity(rng.random(n) >= 0.1)
    T.init()
    plan = T.Plan([spec(T.APPROX_DISTINCT, 0), spec(T.COUNT, 0)])
    cuts = [0, n // 9, n // 2, n // 2, n]  # (one part empty)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = T.State(plan)
        if b > a:
            s.update([column(vals, validity, offset=a, length=b - a)])
        parts.append(s)
    parts.append(T.State(plan))  # never updated
    for order in ([0, 1, 2, 3, 4], [4, 3, 2, 0, 1]):
        m = T.State(plan)
        m.merge([parts[i] for i in order])
        check(m.finalize()[0], vals, validity, regs=registers_of(m))
        back = T.State.deserialize(plan, m.serialize())
        assert np.array_equal(registers_of(back), registers_of(m))
        check(back.finalize()[0], vals, validity)


@pytest.mark.parametrize("world", [2, 5])
def test_threaded_ranks(world):
    from test_gpu_distributed_sim import _run_ranks

    n = 1_200_000
    rng = np.random.default_rng(51 + world)
    vals = values("epoch_ms", n, rng)
    mask = rng.random(n) >= 0.05
    validity = orc.pack_validity(mask)
    cuts = [n * r // world for r in range(world + 1)]
    T.init()
    plan = T.Plan([spec(T.APPROX_DISTINCT, 0), spec(T.NUMERIC_STATS, 0)])

    def shards_of(rank):
        a, b = cuts[rank], cuts[rank + 1]
        return [numeric_column(vals[a:b], orc.pack_validity(mask[a:b]), True)]

    for res, st in _run_ranks(world, plan, shards_of):  # every rank ends with the whole table's answer
        check(res[0], vals, validity, counts=False)
        assert res[0].non_null == int(mask.sum())
