"""-m gpu: TGX_CHECK_VALUE_RULE, the numeric row predicates behind DataTypeConstraint (TG/constraints/datatype.rs:144-160,
383-439).  The reference is tests/exact_value_rule.py -- the literal per-row walk for the small tables, its numpy twin
(held to the walk by tests/test_exact_value_rule.py) for the large ones; neither the library nor the oracle -- and EVERY
count (seen, considered, valid, cast_errors) is compared for equality; there are no tolerances."""
import ctypes
import json
import os
import threading

import numpy as np
import pytest

import exact_value_rule as ev
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, to_device

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = ev.I64_MIN, ev.I64_MAX
NAN_POS, NAN_NEG = 0x7FF8000000000000, -0x0008000000000000            # quiet NaNs of both signs, as int64 patterns
NAN_PAYLOAD, NAN_NEG_PAYLOAD = 0x7FF0000000000123, -0x0010000000000000 + 0x123  # signalling, with a payload
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datatype_vectors.json")


def f64(patterns_or_floats):
    """a float64 array from floats and / or int patterns (a pattern keeps a NaN's sign and payload)"""
    bits = [p if isinstance(p, int) else ev.bits_of(p) for p in patterns_or_floats]
    return np.array(bits, np.int64).view(np.float64)


def column(vals, mask=None, mem=T.MEM_DEVICE, offset=0):
    """an Int64 / Float64 column whose Arrow offset is `offset`: `offset` rows of other data (and set validity bits) lead
    the buffers, the view starts behind them"""
    vals = np.ascontiguousarray(vals)
    is_float = vals.dtype == np.float64
    lead = np.full(offset, 0x5A5A5A5A5A5A5A5A, np.int64)
    vals = np.concatenate([lead.view(np.float64) if is_float else lead, vals])
    validity = None
    if mask is not None:
        validity = pad_validity(orc.pack_validity(np.concatenate([np.ones(offset, bool), mask])))
    if mem == T.MEM_DEVICE:
        vals, validity = to_device(vals), to_device(validity)
    return T.Column(T.FLOAT64 if is_float else T.INT64, len(vals), values=vals, validity=validity,
                    mem=mem).sliced(offset, len(vals) - offset)


def batches_of(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def plan_of(rules, extra=(), columns=None):
    """rules: exact_value_rule.rule dicts; rule i reads column columns[i] (default: column 0)"""
    columns = columns or [0] * len(rules)
    plan = T.Plan([spec(T.VALUE_RULE, c) for c in columns] + list(extra))
    for i, r in enumerate(rules):
        plan.set_value_rule(i, r["mode"], r["flags"], r["lo_i"], r["hi_i"], r["lo_f"], r["hi_f"])
    return plan


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def walk(rules, vals, mask):
    """the literal walk"""
    is_float = vals.dtype == np.float64
    return [ev.counts(r, vals.view(np.int64).tolist(), None if mask is None else mask.tolist(), is_float) for r in rules]


def twin(rules, vals, mask):
    return [ev.counts_np(r, vals, mask) for r in rules]


def check(rules, vals, mask=None, offset=0, mem=T.MEM_DEVICE, cuts=None, want=None):
    T.init()
    want = walk(rules, vals, mask) if want is None else want
    plan = plan_of(rules)
    st = feed(plan, batches_of([column(vals, mask, mem, offset)], len(vals), cuts))
    got = [st.value_rule_counts(i) for i in range(len(rules))]
    assert got == want
    for r, (seen, considered, valid, errors) in zip(st.finalize(), want):
        assert (r.total, r.non_null, r.matches, r.distinct) == (seen, considered, valid, errors)
    return st, plan, want


INT_RULES = [ev.rule(ev.GE_ZERO), ev.rule(ev.GT_ZERO), ev.rule(ev.BETWEEN, 0, -1000, 1000),
             ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, -0.5, 2.0 ** 33 + 0.5), ev.rule(ev.INTEGER)]
FLOAT_RULES = [ev.rule(ev.GE_ZERO), ev.rule(ev.GT_ZERO), ev.rule(ev.BETWEEN, 0, 0, 0, -1.5, 1.5),
               ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, -0.0, 1e10), ev.rule(ev.INTEGER)]

INT_EDGES = [I64_MIN, -1, 0, 1, I64_MAX, 2**31, -2**31, 2**31 - 1, -2**31 - 1, 2**53, 2**53 + 1, -2**53, -2**53 - 1,
             2**53 + 2, 1000, -1000, 1001]
FLOAT_EDGES = [0.0, -0.0, 5e-324, -5e-324, float("inf"), -float("inf"), NAN_POS, NAN_NEG, NAN_PAYLOAD,
               NAN_NEG_PAYLOAD, 0.5, -0.5, 2.0, 2.5, -2147483648.9, -2147483649.0, 2147483647.5,
               2147483648.0, 1e300, -1e300, 2147483647.0, -2147483648.0, 1.5, -1.5, 1e10]


def int_table(rng, n, null=0.1):
    v = rng.integers(-3000, 3000, n, dtype=np.int64)
    far = rng.random(n) < 0.2
    v[far] = rng.integers(-2**40, 2**40, int(far.sum()), dtype=np.int64)
    k = min(n, len(INT_EDGES))
    v[:k] = np.array(INT_EDGES[:k], np.int64)
    return v, (None if null is None else rng.random(n) >= null)


def float_table(rng, n, null=0.1):
    v = np.round(rng.standard_normal(n) * 3.0, 1)
    whole = rng.random(n) < 0.4
    v[whole] = np.trunc(v[whole] * 1e3)
    far = rng.random(n) < 0.1
    v[far] *= 1e9
    k = min(n, len(FLOAT_EDGES))
    v[:k] = f64(FLOAT_EDGES[:k])
    return v, (None if null is None else rng.random(n) >= null)


def tiled(values):
    """every value at every lane position: a list of odd length repeated 64 times"""
    values = list(values)
    if len(values) % 2 == 0:
        values.append(values[0])
    return values * 64


# ---- sizes, offsets, validity -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    check(INT_RULES, *int_table(rng, n))
    check(FLOAT_RULES, *float_table(rng, n))


def test_more_than_one_sweep_of_the_launch():
    """Two column groups in the plan: each gets max(32, 4 * CUs / 2) = 512 workgroups of 512 lanes on the 256-CU part, and
    a lane takes 4 row PAIRS per sweep on the 16-byte path: one sweep is 4 * 512 * 512 * 2 = 2 097 152 rows.
    2 097 152 + 5 rows start a second sweep there (and a fifth one on the one-row-per-load path, which the odd offset
    takes)."""
    n = 4 * 512 * 512 * 2 + 5
    rng = np.random.default_rng(1)
    iv, im = int_table(rng, n, 0.5)
    fv, _ = float_table(rng, n, None)
    rules = [INT_RULES[0], INT_RULES[4], FLOAT_RULES[1], FLOAT_RULES[4]]
    want = twin(rules[:2], iv, im) + twin(rules[2:], fv, None)
    T.init()
    for offsets in ((0, 0), (1, 0)):
        cols = [column(iv, im, T.MEM_DEVICE, offsets[0]), column(fv, None, T.MEM_DEVICE, offsets[1])]
        st = feed(plan_of(rules, columns=[0, 0, 1, 1]), [cols])
        assert [st.value_rule_counts(i) for i in range(4)] == want


@pytest.mark.parametrize("offset", [0, 1, 7, 8, 9])
def test_arrow_offsets(offset):
    rng = np.random.default_rng(100 + offset)
    n = 8192 + 77
    check(INT_RULES, *int_table(rng, n), offset=offset)
    check(FLOAT_RULES, *float_table(rng, n), offset=offset)


@pytest.mark.parametrize("nulls", ["absent", "present", "all_null", "none_null"])
def test_validity_absent_present_all_null(nulls):
    rng = np.random.default_rng(5)
    n = 20_001
    frac = {"absent": None, "present": 0.3, "all_null": 1.1, "none_null": 0.0}[nulls]
    for rules, table in ((INT_RULES, int_table), (FLOAT_RULES, float_table)):
        v, m = table(rng, n, frac)
        _, _, want = check(rules, v, m)
        if nulls == "all_null":
            assert want == [(n, 0, 0, 0)] * len(rules)


def test_null_truth_table():
    """a NULL row is seen and never considered, whatever stands in its slot: a value that passes, one that fails, one
    that cannot be cast"""
    iv = np.array([5, -5, 2**40, 5, -5, 2**40], np.int64)
    mask = np.array([True] * 3 + [False] * 3)
    _, _, want = check(INT_RULES, iv, mask)
    assert want == [(6, 3, 2, 0), (6, 3, 2, 0), (6, 3, 2, 0), (6, 3, 1, 0), (6, 3, 2, 1)]
    fv = f64([2.0, -2.5, NAN_POS, 2.0, -2.5, NAN_POS])
    _, _, want = check(FLOAT_RULES, fv, mask)
    assert want == [(6, 3, 2, 0), (6, 3, 2, 0), (6, 3, 0, 0), (6, 3, 1, 0), (6, 3, 1, 1)]


# ---- the values where a rule can go wrong -----------------------------------------------------------------------------
def test_int64_edges_at_every_lane():
    """the ends of Int64 and of Int32, and 2^53 / 2^53 + 1 under double bounds, where CAST AS DOUBLE rounds"""
    v = np.array(tiled(INT_EDGES), np.int64)
    rules = INT_RULES + [
        ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, 2.0 ** 53, 2.0 ** 53),       # 2^53 + 1 rounds INTO the range
        ev.rule(ev.BETWEEN, 0, 2**53, 2**53),                                         # ... and is outside as an int64
        ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, -(2.0 ** 63), 2.0 ** 63)]     # INT64_MAX rounds to 2^63
    _, _, want = check(rules, v)
    per = 64  # (rows per value of the list)
    assert want[5][2] == 2 * per and want[6][2] == per and want[7][2] == len(v)
    assert want[4][3] == sum(1 for x in v.tolist() if not ev.I32_MIN <= x <= ev.I32_MAX) > 0
    mask = np.arange(len(v)) % 5 != 0
    check(rules, v, mask, offset=1)


def test_float64_edges_at_every_lane():
    """signed zeros, denormals, infinities, NaNs of both signs and with a payload, halves, the Int32 cast boundary"""
    v = f64(tiled(FLOAT_EDGES))
    _, _, want = check(FLOAT_RULES, v)
    one = walk(FLOAT_RULES, f64(FLOAT_EDGES), None)
    # by hand, on one copy of the list: what passes GE_ZERO is +0.0, the positive values and the positive NaNs
    ge = [x for x in FLOAT_EDGES if (x >= 0 if isinstance(x, int) else (x > 0 or ev.bits_of(x) == 0))]
    assert one[0][2] == len(ge) and one[1][2] == len(ge) - 1
    # INTEGER: four NaNs, +-inf, +-1e300, 1e10, -2147483649.0 and 2147483648.0 do not cast; 2.0, +0.0 and the two ends of
    # Int32 are whole
    assert one[4][3] == 4 + 2 + 2 + 1 + 2 and one[4][2] == 4
    mask = np.arange(len(v)) % 3 != 1
    check(FLOAT_RULES, v, mask, offset=9)


def test_between_bounds():
    iv = np.array(tiled(INT_EDGES), np.int64)
    rules = [ev.rule(ev.BETWEEN, 0, 7, 7), ev.rule(ev.BETWEEN, 0, 1000, 1000), ev.rule(ev.BETWEEN, 0, 1000, -1000),
             ev.rule(ev.BETWEEN, 0, I64_MIN, I64_MAX), ev.rule(ev.BETWEEN, 0, I64_MAX, I64_MAX),
             ev.rule(ev.BETWEEN, 0, I64_MIN, I64_MIN), ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, 1.5, -1.5),
             ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, -0.0, 0.0)]
    _, _, want = check(rules, iv)
    assert want[0][2] == 0 and want[2][2] == 0 and want[6][2] == 0 and want[3][2] == len(iv)
    assert want[1][2] == want[4][2] == want[5][2] == want[7][2] > 0  # (each value of the list stands in it once)
    fv = f64(tiled(FLOAT_EDGES))
    inf = float("inf")
    rules = [ev.rule(ev.BETWEEN, 0, 0, 0, 0.5, 0.5), ev.rule(ev.BETWEEN, 0, 0, 0, 1.5, -1.5),
             ev.rule(ev.BETWEEN, 0, 0, 0, -inf, inf), ev.rule(ev.BETWEEN, 0, 0, 0, ev.float_of(NAN_NEG), ev.float_of(NAN_POS)),
             ev.rule(ev.BETWEEN, 0, 0, 0, -0.0, -0.0), ev.rule(ev.BETWEEN, 0, 0, 0, -0.0, 0.0),
             ev.rule(ev.BETWEEN, 0, 0, 0, 0.0, 0.0), ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, -1.5, 1.5)]
    _, _, want = check(rules, fv)
    zeros = {z: sum(1 for x in tiled(FLOAT_EDGES) if not isinstance(x, int) and ev.bits_of(x) == ev.bits_of(z))
             for z in (0.0, -0.0)}
    # lo_f = -0.0 against +0.0 data: [-0.0, -0.0] holds -0.0 alone, [-0.0, +0.0] both zeros, [+0.0, +0.0] +0.0 alone
    assert (want[4][2], want[5][2], want[6][2]) == (zeros[-0.0], zeros[-0.0] + zeros[0.0], zeros[0.0])
    assert want[1][2] == 0 and want[0][2] == 64 and zeros[0.0] >= 64 and zeros[-0.0] == 64


def test_nine_rules_on_one_column_take_two_groups():
    """every spec's answer equals that spec alone in a plan of its own"""
    rng = np.random.default_rng(9)
    n = 50_001
    for table, base in ((int_table, INT_RULES), (float_table, FLOAT_RULES)):
        v, m = table(rng, n)
        rules = base + [ev.rule(ev.BETWEEN, 0, -7, 7, -7.0, 7.0), ev.rule(ev.BETWEEN, ev.BOUNDS_AS_DOUBLE, 0, 0, 0.25, 99.5),
                        ev.rule(ev.INTEGER), ev.rule(ev.GE_ZERO)]
        assert len(rules) == 9
        T.init()
        col = column(v, m)
        st = feed(plan_of(rules), [[col]])
        together = [st.value_rule_counts(i) for i in range(9)]
        assert together == twin(rules, v, m)
        for i, r in enumerate(rules):
            alone = feed(plan_of([r]), [[col]])
            assert alone.value_rule_counts(0) == together[i]


NARROW = [("int8", T.INT8, np.int8), ("uint8", T.UINT8, np.uint8), ("int16", T.INT16, np.int16),
          ("uint16", T.UINT16, np.uint16), ("int32", T.INT32, np.int32), ("uint32", T.UINT32, np.uint32),
          ("date32", T.INT32, np.int32), ("float32", T.FLOAT32, np.float32)]


@pytest.mark.parametrize("name,type_id,dtype", NARROW, ids=[t[0] for t in NARROW])
@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
def test_narrow_and_4_byte_columns(name, type_id, dtype, mem):
    rng = np.random.default_rng(len(name))
    n = 10_007
    if name == "float32":
        raw = np.round(rng.standard_normal(n) * 3.0, 1).astype(np.float32)
        raw[rng.random(n) < 0.4] = np.float32(7.0)
        specials = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800123, 0x80000000, 0, 0x7F800000, 0xFF800000,
                             0x00000001, 0x80000001, 0x4F000000, 0xCF000000, 0xCF000001], np.uint32)  # (+-2^31, the next below)
        raw[:len(specials)] = specials.view(np.float32)
        rules = FLOAT_RULES
    else:
        info = np.iinfo(dtype)
        raw = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        raw[:4] = [info.min, info.max, 0, 1]
        rules = INT_RULES
    mask = rng.random(n) >= 0.1
    wide = ev.widen(raw, "int32" if name == "date32" else name)
    want = walk(rules, wide, mask)
    if name == "uint32":  # values above 2^31 - 1 are cast errors in INTEGER mode
        assert want[4][3] == int(((raw > 2**31 - 1) & mask).sum()) > 0
    if name == "float32":  # the NaNs' signs survive widening: +NaN passes GE_ZERO, -NaN does not
        assert ev.judge(rules[0], int(wide.view(np.int64)[0]), True)[0] and not ev.judge(rules[0], int(wide.view(np.int64)[1]), True)[0]
    T.init()
    validity = pad_validity(orc.pack_validity(mask))
    vals = np.concatenate([raw, np.zeros(16, dtype)])
    if mem == T.MEM_DEVICE:
        vals, validity = to_device(vals), to_device(validity)
    ctor = {T.INT32: T.Column.int32, T.FLOAT32: T.Column.float32}.get(type_id)
    col = ctor(vals, validity, length=n) if ctor else T.Column.narrow(type_id, vals, validity, length=n)
    if mem == T.MEM_HOST:
        col = T.Column(type_id, n, values=vals, validity=validity, mem=T.MEM_HOST)
    for cuts in (None, 4096):
        st = feed(plan_of(rules), batches_of([col], n, cuts))
        assert [st.value_rule_counts(i) for i in range(len(rules))] == want


# ---- batching, fusion, the state's algebra ----------------------------------------------------------------------------
BATCH_N = 300_000


@pytest.fixture(scope="module")
def big_table():
    rng = np.random.default_rng(7)
    iv, im = int_table(rng, BATCH_N)
    fv, fm = float_table(rng, BATCH_N, 0.07)
    rules = INT_RULES + FLOAT_RULES
    columns = [0] * len(INT_RULES) + [1] * len(FLOAT_RULES)
    return iv, im, fv, fm, rules, columns, twin(INT_RULES, iv, im) + twin(FLOAT_RULES, fv, fm)


def got_of(st, n):
    return [st.value_rule_counts(i) for i in range(n)]


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192),
                                      (T.MEM_HOST_RETAINED, 8192), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_HOST, [3, 8195, 8196, 200_001])])
def test_batching_independence(big_table, mem, cuts):
    iv, im, fv, fm, rules, columns, want = big_table
    T.init()
    cols = [column(iv, im, mem), column(fv, fm, mem)]
    st = feed(plan_of(rules, columns=columns), batches_of(cols, BATCH_N, cuts))
    assert got_of(st, len(rules)) == want


def test_no_coalesce(big_table):
    iv, im, fv, fm, rules, columns, want = big_table
    T.init(flags=T.OPT_NO_COALESCE)
    try:
        cols = [column(iv, im, T.MEM_HOST), column(fv, fm, T.MEM_HOST)]
        st = feed(plan_of(rules, columns=columns), batches_of(cols, BATCH_N, 8192))
        assert got_of(st, len(rules)) == want
    finally:
        T.init(flags=0)


def test_fusion_leaves_the_other_kinds_bit_for_bit(big_table):
    """NUMERIC_STATS, DISTINCT, TEMPORAL and HISTOGRAM on the same columns answer the same, byte for byte, with and
    without the VALUE_RULE specs beside them"""
    iv, im, fv, fm, rules, columns, want = big_table
    T.init()
    cols = [column(iv, im), column(fv, fm)]
    others = [spec(T.COUNT, 0), spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE), spec(T.NUMERIC_STATS, 1),
              spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.DISTINCT, 1), spec(T.TEMPORAL, 0),
              spec(T.HISTOGRAM, 0), spec(T.HISTOGRAM, 1)]
    edges = [-3000.0, -1000.0, 0.0, 1000.0, 3000.0]

    def finish(plan, at):
        plan.set_temporal(at + 5, T.TEMPORAL_RANGE, lo=-1000, hi=1000)
        plan.set_histogram_edges(at + 6, edges)  # (the float column's histogram stays in its range phase)
        st = feed(plan, [cols])
        res = st.finalize()
        return st, res, (st.temporal_counts(at + 5), st.histogram_counts(at + 6), st.histogram_range(at + 7))

    _, alone, alone_side = finish(T.Plan(others), 0)
    st, res, side = finish(plan_of(rules, extra=others, columns=columns), len(rules))
    assert got_of(st, len(rules)) == want
    for got, ref in zip(res[len(rules):], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))
    assert repr(side) == repr(alone_side)  # (repr of a float round-trips its bits)


def test_state_algebra(big_table):
    iv, im, fv, fm, rules, columns, want = big_table
    T.init()
    cols = [column(iv, im), column(fv, fm)]
    parts = batches_of(cols, BATCH_N, [100_000, 200_001])
    plan = plan_of(rules, columns=columns)
    n = len(rules)
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    assert got_of(states[0], n) == want
    # serialize -> deserialize -> merge
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    assert got_of(back, n) == want and back.serialize() == blob
    twice = feed(plan, [cols])
    twice.merge([back])
    assert got_of(twice, n) == [tuple(2 * v for v in w) for w in want]
    # a blob counted under other bounds is refused
    changed = [dict(r) for r in rules]
    changed[2]["hi_i"] += 1
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plan_of(changed, columns=columns), blob)
    zero = [dict(r) for r in rules]
    zero[8]["lo_f"] = 0.0  # (was -0.0: another bound under totalOrder)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plan_of(zero, columns=columns), blob)
    # reset; a read half-way, feed more, read again
    st = states[0]
    st.reset()
    assert got_of(st, n) == [(0, 0, 0, 0)] * n
    st.update(parts[0])
    first = twin(INT_RULES, iv[:100_000], im[:100_000]) + twin(FLOAT_RULES, fv[:100_000], fm[:100_000])
    assert got_of(st, n) == first
    assert [(r.total, r.non_null, r.matches, r.distinct) for r in st.finalize()] == first
    st.update(parts[1])
    st.update(parts[2])
    assert [(r.total, r.non_null, r.matches, r.distinct) for r in st.finalize()] == want


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(big_table, world, device_buffers):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    iv, im, fv, fm, rules, columns, want = big_table
    T.init()
    whole = [column(iv, im), column(fv, fm)]
    plan = plan_of(rules, extra=[spec(T.COUNT, 0)], columns=columns)
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(BATCH_N, world, rank)
            st = T.State(plan)
            comm = thread_comm(group, rank, device_buffers=device_buffers)
            for _ in range(2):
                res = sharded_suite_step(plan, st, [c.sliced(lo, hi - lo) for c in whole], comm)
            results[rank] = (res, got_of(st, len(rules)))
        except Exception:  # noqa: BLE001
            import traceback

            errors.append((rank, traceback.format_exc()))
            group.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=150)
    assert not errors, errors
    assert not any(t.is_alive() for t in threads), "a rank is stuck"
    for res, got in results:
        assert got == want
        assert res[len(rules)].total == BATCH_N


def test_other_column_types_are_unsupported_and_the_state_stays_usable():
    T.init()
    n = 1000
    good = column(np.arange(n, dtype=np.int64) - 10, None, T.MEM_HOST)
    u64 = T.Column.narrow(T.UINT64, np.arange(n, dtype=np.uint64))
    boolean = T.Column.boolean(np.zeros(n // 8 + 8, np.uint8), n)
    offs, data, _ = orc.utf8_from_list(["a%d" % i for i in range(n)])
    text = T.Column.utf8(offs, np.concatenate([data, np.zeros(64, np.uint8)]))
    st = T.State(plan_of([ev.rule(ev.GE_ZERO)]))
    for bad in (u64, boolean, text):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED"):
            st.update([bad])
    st.update([good])
    assert st.value_rule_counts(0) == (n, n, n - 10, 0)


def test_a_spec_without_parameters_fails_state_create():
    T.init()
    plan = T.Plan([spec(T.VALUE_RULE, 0), spec(T.VALUE_RULE, 0)])
    plan.set_value_rule(0, ev.GE_ZERO)
    with pytest.raises(T.TgxError, match="tgx_plan_set_value_rule"):
        T.State(plan)
    plan.set_value_rule(1, ev.INTEGER)
    st = T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):  # fixed once a state exists
        plan.set_value_rule(1, ev.GT_ZERO)
    for bad in (dict(mode=0), dict(mode=5), dict(mode=ev.GE_ZERO, flags=ev.BOUNDS_AS_DOUBLE), dict(mode=ev.BETWEEN, flags=2)):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.Plan([spec(T.VALUE_RULE, 0)]).set_value_rule(0, **bad)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.Plan([spec(T.VALUE_RULE, 0, column2=1)])
    del st


# ---- end to end: ValidationSuite.run --------------------------------------------------------------------------------
def run_suite(table, constraints, column_types=None):
    """every constraint in a check of its own; returns [(status, metric, message)] in order"""
    import term_amd.suite as S

    T.init()
    sb = S.ValidationSuite.builder("datatype")
    for col, typ in (column_types or {}).items():
        sb.column_type(col, typ)
    for i, c in enumerate(constraints):
        sb.check(S.Check.builder("c%d" % i).level(S.Level.ERROR).constraint(c).build())
    res = sb.build().run(table)
    issues = {i.check_name: i for i in res.report.issues}
    out = []
    for i in range(len(constraints)):
        if "c%d" % i in issues:
            out.append(("Failure", issues["c%d" % i].metric, issues["c%d" % i].message))
        else:
            out.append(("Success", res.report.metrics.custom_metrics["c%d.datatype" % i], None))
    return out


def constraint_of(case):
    import term_amd.suite as S

    v = case["validation"]
    if v["kind"] == "specific_type":
        return S.DataTypeConstraint.specific_type(case["column"], v["type"])
    if v["kind"] == "non_negative":
        return S.DataTypeConstraint.non_negative(case["column"])
    if v["kind"] == "range":
        return S.DataTypeConstraint(case["column"], S.DataTypeValidation.Numeric(S.NumericValidation.Range(v["min"], v["max"])))
    if v["kind"] == "string_not_empty":
        return S.DataTypeConstraint(case["column"], S.DataTypeValidation.String(S.StringTypeValidation.NotEmpty))
    raise ValueError(v["kind"])


def test_suite_on_the_reference_tables():
    """the reference's own tests (datatype.rs:473-623), through ValidationSuite"""
    import pyarrow as pa

    with open(GOLDEN) as f:
        golden = json.load(f)
    for case in golden["cases"]:
        types = {"Float64": pa.float64(), "Int64": pa.int64(), "Utf8": pa.string()}
        table = pa.table({name: pa.array(col["values"], types[col["type"]]) for name, col in case["table"].items()})
        (got,) = run_suite(table, [constraint_of(case)])
        if case["on_device"] or case["validation"]["kind"] == "specific_type":
            assert got[0] == case["status"], case["source"]
            if "metric" in case:
                assert got[1] == case["metric"]
            if "metric_below" in case:
                assert got[1] < case["metric_below"]
        else:  # stays off the device: the constraint's own error
            assert got[0] == "Failure" and "not on the GPU path" in got[2]


def test_suite_on_numeric_tables():
    """a Float64 / Int64 / Int32 table: statuses, metrics and messages from exact_value_rule"""
    import pyarrow as pa
    import term_amd.suite as S

    rng = np.random.default_rng(44)
    n = 20_003
    fv, fm = float_table(rng, n)
    iv, im = int_table(rng, n)
    sv = rng.integers(0, 1000, n, dtype=np.int32)
    def arr(v, m, t):
        return pa.array(v, t, mask=None if m is None else ~m)
    table = pa.table({"f": arr(fv, fm, pa.float64()), "i": arr(iv, im, pa.int64()), "s": arr(sv, None, pa.int32()),
                      "clean": pa.array(np.abs(np.trunc(rng.standard_normal(n) * 10)) + 1.0, pa.float64())})
    wide = {"f": (fv, fm), "i": (iv, im), "s": (sv.astype(np.int64), None), "clean": (table["clean"].to_numpy(), None)}
    N, D, V = S.NumericValidation, S.DataTypeConstraint, S.DataTypeValidation
    cases = []
    for col in ("f", "i", "s", "clean"):
        cases += [(D.non_negative(col), col, ev.rule(ev.GE_ZERO), ev.description("non_negative")),
                  (D(col, V.Numeric(N.Positive)), col, ev.rule(ev.GT_ZERO), ev.description("positive"))]
        for lo, hi in ((-1000.0, 1000.0), (0.5, 2.0 ** 33 + 0.5), (-0.0, 1e6)):
            cases.append((D(col, V.Numeric(N.Range(lo, hi))), col, ev.range_params(lo, hi), ev.description("range", min=lo, max=hi)))
    cases.append((D("s", V.Numeric(N.Integer)), "s", ev.rule(ev.INTEGER), ev.description("integer")))
    cases.append((D("clean", V.Numeric(N.Integer)), "clean", ev.rule(ev.INTEGER), ev.description("integer")))
    got = run_suite(table, [c for c, _, _, _ in cases])
    for g, (_, col, r, text) in zip(got, cases):
        _, considered, valid, errors = ev.counts_np(r, *wide[col])
        assert errors == 0 and g == ev.verdict(considered, valid, text)
    assert got[-1] == ("Success", 1.0, None) and got[-2] == ("Success", 1.0, None)
    assert {g[0] for g in got} == {"Success", "Failure"}
    # INTEGER where rows do not fit Int32: the constraint's error, with the count
    (err,) = run_suite(table, [D("i", V.Numeric(N.Integer))])
    _, _, _, errors = ev.counts_np(ev.rule(ev.INTEGER), iv, im)
    assert err[0] == "Failure" and ("%d rows do not fit Int32" % errors) in err[2] and errors > 0
    # no non-NULL row: 0 / 0
    empty = pa.table({"f": pa.array([None, None], pa.float64())})
    (nan,) = run_suite(empty, [D.non_negative("f")])
    assert nan[0] == "Failure" and nan[2].startswith("NaN% of values satisfy non-negative values")
    assert nan[1] is None or nan[1] != nan[1]


def test_suite_mixes_device_rules_with_what_stays_off_the_device():
    """Finite and a String validation are their own errors; the rules beside them still get their verdicts"""
    import pyarrow as pa
    import term_amd.suite as S

    table = pa.table({"x": pa.array([1.0, 2.0, 0.0, -3.0]), "name": pa.array(["a", "", "c", "d"])})
    N, D, V = S.NumericValidation, S.DataTypeConstraint, S.DataTypeValidation
    got = run_suite(table, [D.non_negative("x"), D("x", V.Numeric(N.Finite)),
                            D("name", V.String(S.StringTypeValidation.NotEmpty)), D("x", V.Numeric(N.Range(-5.0, 5.0))),
                            D.specific_type("x", "Float64"), D.specific_type("x", "Int64"), D.type_consistency("x", 0.9),
                            D.type_consistency("x", 0.99)])
    assert got[0] == ("Failure", 0.75, "75.0% of values satisfy non-negative values")
    assert got[3] == ("Success", 1.0, None)
    prefix = "Error evaluating constraint: Constraint evaluation failed for 'datatype': "
    assert got[1][2].startswith(prefix) and "ISFINITE" in got[1][2] and "not on the GPU path" in got[1][2]
    assert got[2][2].startswith(prefix) and "not on the GPU path" in got[2][2]
    assert got[4] == ("Success", 1.0, None)
    assert got[5] == ("Failure", 0.0, "Column 'x' has type Float64, expected Int64")
    assert got[6] == ("Success", 0.95, None)
    assert got[7] == ("Failure", 0.95, "Type consistency 95.0% below threshold 99.0%")
