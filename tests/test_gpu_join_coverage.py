"""The counted mode of TGX_CHECK_KEY_PROBE on the device, held against tests/exact_join_coverage.py: every counter, every
missing key, both digests, parent_rows, max_count, the route, pairs and join_rows are compared for equality with the
exact walk -- for every shape of counted set (empty, one key, the count array, the counted hash table, their threshold,
the marker key and both extremes), 64-bit counts, duplicate records, the refusals of a set, the guard against a wrapping
sum, every batching and every way a state travels -- and JoinCoverageConstraint end to end through ValidationSuite.run."""
import json
import os

import numpy as np
import pyarrow as pa
import pytest

import exact_join_coverage as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2**63, 2**63 - 1
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- columns, records and states ------------------------------------------------------------------------------------------
def padded(buf):
    if buf is None:
        return None
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return to_device(np.concatenate([raw, np.zeros(64, np.uint8)]))


def column(arr, mem=T.MEM_DEVICE):
    col = T.Column.from_arrow(arr)
    if mem == T.MEM_DEVICE:
        values, validity = col._keep[:2]
        return T.Column(col.c.type, col.c.length, values=padded(values), validity=padded(validity), offset=col.c.offset,
                        mem=T.MEM_DEVICE)
    col.c.mem = mem
    return col


def ints(values, type=pa.int64(), mask=None):
    return pa.array(values, type=type, mask=None if mask is None else ~np.asarray(mask))


def split(arr):
    mask = None if arr.null_count == 0 else np.asarray(arr.is_valid())
    return np.asarray(arr.fill_null(0)).astype(np.int64), mask


def cut(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def device_records(records):
    """(key, count) pairs as 16-byte records in device memory"""
    if not records:
        return None
    recs = np.zeros((len(records), 2), np.uint64)
    recs[:, 0] = np.array([k for k, _ in records], np.int64).view(np.uint64)
    recs[:, 1] = np.array([c for _, c in records], np.uint64)
    return to_device(recs.reshape(-1))


def set_parent(st, records, i=0):
    d = device_records(records)
    st.key_probe_set_parent(i, d.data_ptr() if d is not None else None, len(records))


def counted_plan(n=1, bound=10000, plain=0, extra=()):
    """n counted specs, then `plain` plain ones, all on column 0"""
    plan = T.Plan([spec(T.KEY_PROBE, 0) for _ in range(n + plain)] + list(extra))
    for k in range(n):
        plan.set_key_probe_counted(k, bound)
    for k in range(n, n + plain):
        plan.set_key_probe(k, bound)
    return plan


def read(st, i=0):
    summary, entries = st.key_probe(i)
    got = dict(summary, entries=entries)
    assert got["seen"] == got["non_null"] + got["null_rows"]
    assert got["non_null"] == got["matched"] + got["missing_rows"]
    assert got["missing_rows"] == got["counted"] + got["overflow_rows"]
    pairs = st.key_probe_pairs(i)
    assert pairs["join_rows"] == pairs["pairs"] + got["missing_rows"] + got["null_rows"]
    assert pairs["pairs"] >= got["matched"]
    return got, pairs


def exact(child, records, bound=10000):
    values, mask = split(child)
    return ex.walk_np(values, mask, records, bound)


def check(child, records, mem=T.MEM_DEVICE, cuts=None, route=None):
    T.init()
    st = T.State(counted_plan())
    set_parent(st, records)
    for b in cut([column(child, mem)], len(child), cuts):
        st.update(b)
    want = exact(child, records)
    got = read(st)
    assert got == want and list(got[0]["entries"]) == list(want[0]["entries"])
    if route is not None:
        assert got[0]["route"] == route
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.matches, r.distinct) == (want[0]["seen"], want[0]["non_null"], want[0]["matched"],
                                                           want[0]["missing_keys"])
    return st, want


def mixed_counts(keys, seed):
    rng = np.random.default_rng(seed)
    return [(int(k), int(c)) for k, c in zip(keys, rng.integers(1, 6, len(keys)))]


DENSE = np.arange(-500, 500)  # 1000 dense keys, the marker (-1) among them: route 3
SPREAD = np.concatenate([(np.arange(1000, dtype=np.int64) - 500) * 18_446_744_073_709_551 + 7,
                         [I64_MIN, I64_MAX, -1]])  # about 1000 keys over int64, the extremes and the marker: route 4


def child_for(keys, n, nulls, seed):
    """n rows drawn from the keys and from as many values that are not keys"""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.asarray(keys, np.int64), np.asarray(keys, np.int64)[: max(1, len(keys) // 2)] + 3])
    v = pool[rng.integers(0, len(pool), n)]
    return ints(v, mask=rng.random(n) >= nulls)


# ---- rows and sets ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65, 1025, 16_385])
@pytest.mark.parametrize("nulls", [0.0, 0.05, 1.0])
def test_child_lengths_on_both_routes(n, nulls):
    _, want = check(child_for(DENSE, n, nulls, n), mixed_counts(DENSE, 1), route=ex.ROUTE_COUNT_ARRAY)
    assert nulls == 1.0 or n < 60 or want[1]["pairs"] > want[0]["matched"] > 0
    _, want = check(child_for(SPREAD, n, nulls, n + 1), mixed_counts(SPREAD, 2), route=ex.ROUTE_COUNT_HASH)
    assert nulls == 1.0 or n < 60 or want[1]["pairs"] > want[0]["matched"] > 0


def test_an_empty_set_and_a_set_of_one_key():
    child = ints([3, 4, None, 3, -1, 3] * 50)
    _, want = check(child, [], route=ex.ROUTE_EMPTY)
    assert want[1] == {"pairs": 0, "join_rows": 300, "parent_rows": 0, "parent_count_digest": 0, "max_count": 0}
    _, want = check(child, [(3, 7)], route=ex.ROUTE_COUNT_ARRAY)
    assert want[1]["pairs"] == 7 * 150 and want[1]["join_rows"] == 7 * 150 + 150
    _, want = check(child, [(-1, 2)], route=ex.ROUTE_COUNT_ARRAY)  # the marker key alone
    assert want[1]["pairs"] == 100


def test_all_counts_one_pairs_are_the_matched_rows():
    for keys, route in ((DENSE, ex.ROUTE_COUNT_ARRAY), (SPREAD, ex.ROUTE_COUNT_HASH)):
        _, want = check(child_for(keys, 5000, 0.05, 3), [(int(k), 1) for k in keys], route=route)
        assert want[1]["pairs"] == want[0]["matched"] > 0 and want[1]["max_count"] == 1


def test_the_threshold_between_the_count_array_and_the_hash_table():
    child = ints(np.arange(-5, 40))
    at = [(0, 2), (5, 1), (9, 3), (15, 1)]       # range 16 == 4 * 4
    beyond = [(0, 2), (5, 1), (9, 3), (16, 1)]   # range 17
    check(child, at, route=ex.ROUTE_COUNT_ARRAY)
    check(child, beyond, route=ex.ROUTE_COUNT_HASH)
    check(child, beyond + [(16, 4)], route=ex.ROUTE_COUNT_ARRAY)  # (the records count, not the distinct keys)


def test_both_extremes_wrap_the_range_and_the_marker_has_its_own_count():
    records = [(I64_MIN, 3), (I64_MAX, 2), (-1, 5)]
    child = ints([I64_MIN, I64_MAX, 0, -1, I64_MIN + 1, I64_MAX - 1, None, -1] * 30)
    _, want = check(child, records, route=ex.ROUTE_COUNT_HASH)
    assert want[1]["pairs"] == 30 * (3 + 2 + 5 + 5) and sorted(want[0]["entries"]) == [I64_MIN + 1, 0, I64_MAX - 1]
    _, want = check(child, records[:2], route=ex.ROUTE_COUNT_HASH)  # the marker in the child only: missing, exact
    assert want[0]["entries"][-1] == 60


def test_64_bit_counts_and_duplicate_records():
    big = [(10, 2**32 + 1), (11, 2**40), (12, 1), (10**15, 2**40 + 3)]
    child = ints([10, 11, 12, 10, 13, None, 10**15] * 9)
    _, want = check(child, big, route=ex.ROUTE_COUNT_HASH)
    assert want[1]["pairs"] == 9 * (2 * (2**32 + 1) + 2**40 + 1 + 2**40 + 3) and want[1]["max_count"] == 2**40 + 3
    _, want = check(child, big[:3], route=ex.ROUTE_COUNT_ARRAY)
    assert want[1]["parent_rows"] == 2**32 + 1 + 2**40 + 1
    # duplicate records of one key add up, as a merge of two exports would; max_count is the largest sum
    dup = [(10, 2), (11, 5), (10, 2**33), (12, 1), (10, 4), (-1, 1), (-1, 6)]
    for records, route in ((dup, ex.ROUTE_COUNT_ARRAY), (dup + [(10**15, 1)], ex.ROUTE_COUNT_HASH)):
        _, want = check(ints([10, 11, -1, 12, 14] * 20), records, route=route)
        assert want[1]["max_count"] == 2**33 + 6 and want[0]["parent_keys"] == len(set(k for k, _ in records))
        assert want[1]["pairs"] == 20 * (2**33 + 6 + 5 + 7 + 1)


def test_a_zero_count_and_a_total_of_2_63_are_refused_and_the_state_stays_usable():
    T.init()
    st = T.State(counted_plan())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*count of 0"):
        set_parent(st, [(1, 1), (2, 0), (3, 1)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*needs its parent set"):  # (it kept no set)
        st.update([column(ints([1, 2, 3]))])
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*2\\^63"):
        set_parent(st, [(1, 2**62), (2, 2**62)])
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*2\\^63"):
        set_parent(st, [(k, 2**63 // 4096 + 1) for k in range(4096)])
    records = [(1, 2**62), (2, 2**62 - 1)]  # 2^63 - 1: allowed
    set_parent(st, records)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*count of 0"):  # the set it had goes as well
        set_parent(st, [(7, 0)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*needs its parent set"):
        st.update([column(ints([1, 2, 3]))])
    set_parent(st, records)
    child = ints([1, 2, 3])
    st.update([column(child)])
    assert read(st) == exact(child, records) and read(st)[1]["parent_rows"] == 2**63 - 1


def test_the_guard_refuses_the_batch_that_could_wrap_the_pairs():
    T.init()
    st = T.State(counted_plan(extra=[spec(T.COUNT, 0)]))
    records = [(1, 2**62), (2, 1)]
    set_parent(st, records)
    fresh = read(st)
    assert fresh[0]["seen"] == 0 and fresh[1]["max_count"] == 2**62
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*2\\^64 - 1"):  # 5 * 2^62 > 2^64 - 1, whatever the rows hold
        st.update([column(ints([2, 2, 2, 2, 2]))])
    assert read(st) == fresh and st.finalize()[1].total == 0  # nothing was noted or run
    three = ints([1, 2, 1])
    st.update([column(three)])  # the next acceptable batch is counted
    before = read(st)
    assert before == exact(three, records) and before[1]["pairs"] == 2**63 + 1 and st.finalize()[1].total == 3
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*2\\^64 - 1"):  # the bound stands at 3 * 2^62: one more row is too many
        st.update([column(ints([9]))])
    assert read(st) == before
    st.reset()
    st.update([column(ints([9, 1, None]))])
    assert read(st) == exact(ints([9, 1, None]), records)


def test_a_counted_and_a_plain_spec_in_one_plan_agree():
    T.init()
    records = mixed_counts(SPREAD, 4) + mixed_counts(SPREAD[:50], 5)
    child = child_for(SPREAD, 30_000, 0.05, 6)
    for recs in (records, mixed_counts(DENSE, 7)):
        st = T.State(counted_plan(1, plain=1))
        set_parent(st, recs, 0)
        set_parent(st, recs, 1)
        st.update([column(child)])
        (counted, pairs), (plain, entries) = read(st, 0), st.key_probe(1)
        plain = dict(plain, entries=entries)
        assert counted["route"] in (3, 4) and plain["route"] == counted["route"] - 2
        assert {k: v for k, v in counted.items() if k != "route"} == {k: v for k, v in plain.items() if k != "route"}
        assert (counted, pairs) == exact(child, recs)
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not counted"):
            st.key_probe_pairs(1)


def test_plan_calls():
    T.init()
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 0), spec(T.COUNT, 0)])
    plan.set_key_probe_counted(0, 100)
    plan.set_key_probe_counted(0, 200)  # (the same call again: the parameters may still change)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*counted"):
        plan.set_key_probe(0, 100)
    plan.set_key_probe(1, 100)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*plain"):
        plan.set_key_probe_counted(1, 100)
    with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*reserved must be 0 \(7\)"):
        plan.set_key_probe_counted(0, 100, reserved=7)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*max_missing_keys must be"):
        plan.set_key_probe_counted(0, 0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        plan.set_key_probe_counted(2, 100)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*counted"):
        plan.set_key_probe_rows(0)
    rows = T.Plan([spec(T.KEY_PROBE, 0)])
    rows.set_key_probe_rows(0)
    rows.set_key_probe_rows(0)
    for call in (rows.set_key_probe, rows.set_key_probe_counted):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*gather rows"):
            call(0, 100)


# ---- P from both sides ----------------------------------------------------------------------------------------------------------
def gathered(arr, cuts=None, mem=T.MEM_DEVICE):
    """(state, pointer, n) of a rows spec fed `arr`: its non-NULL keys as {key, 1} records"""
    plan = T.Plan([spec(T.KEY_PROBE, 0)])
    plan.set_key_probe_rows(0)
    st = T.State(plan)
    for b in cut([column(arr, mem)], len(arr), cuts):
        st.update(b)
    return (st,) + st.key_probe_rows(0)


def host_records(ptr, n):
    import torch

    if n == 0:
        return np.zeros((0, 2), np.uint64)

    class P:
        __cuda_array_interface__ = {"shape": (n * 16,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    return torch.as_tensor(P(), device="cuda").clone().cpu().numpy().view(np.uint64).reshape(n, 2)


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 20_001]), (T.MEM_HOST, 8192)])
def test_a_rows_spec_gathers_every_non_null_key_once(mem, cuts):
    rng = np.random.default_rng(20)
    T.init()
    n = 50_000
    arr = ints(rng.integers(-300, 300, n), pa.int32() if mem == T.MEM_HOST else pa.int64(), mask=rng.random(n) >= 0.1)
    values, mask = split(arr)
    st, ptr, count = gathered(arr, cuts, mem)
    recs = host_records(ptr, count)
    assert count == int(mask.sum()) and (recs[:, 1] == 1).all()
    assert sorted(recs[:, 0].view(np.int64).tolist()) == sorted(values[mask].tolist())
    summary, entries = st.key_probe(0)
    assert (summary["seen"], summary["non_null"], summary["null_rows"], entries) == (n, count, n - count, {})
    r = st.finalize()[0]
    assert (r.total, r.non_null) == (n, count)
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*gathers rows"):
        st.serialize()
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*gathers rows"):
        T.State(st.plan).merge([st])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*takes no parent set"):
        set_parent(st, [(1, 1)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not counted"):
        st.key_probe_pairs(0)
    st.reset()
    assert st.key_probe_rows(0) == (None, 0)
    st.update([column(ints([5, None, 5]))])
    ptr, count = st.key_probe_rows(0)
    assert host_records(ptr, count).tolist() == [[5, 1], [5, 1]]
    nothing = gathered(ints([None, None]))
    assert nothing[1:] == (None, 0)
    plain = T.State(counted_plan())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*does not gather rows"):
        plain.key_probe_rows(0)


def test_pairs_from_both_sides_and_the_nested_loop_join():
    """L against R's gathered rows and R against L's give the same pairs; both join_rows are the literal joins' rows"""
    rng = np.random.default_rng(8)
    T.init()
    left = ints(rng.integers(-20, 40, 700), mask=rng.random(700) >= 0.1)
    right = ints(rng.integers(0, 60, 500), pa.int32(), mask=rng.random(500) >= 0.1)  # an Int32 side, negative keys on the other
    (lv, lm), (rv, rm) = split(left), split(right)
    got = []
    for near, far in ((left, right), (right, left)):
        pst, ptr, count = gathered(far)
        st = T.State(counted_plan())
        st.key_probe_set_parent(0, ptr, count)
        st.update([column(near)])
        summary, pairs = read(st)
        fv, fm = split(far)
        assert (summary, pairs) == exact(near, [(int(v), 1) for v in fv[fm]])
        got.append(pairs)
    assert got[0]["pairs"] == got[1]["pairs"] > 0
    assert (got[0]["join_rows"], got[0]["pairs"]) == ex.nested_loop_left_join(lv, lm, rv, rm)[:2]
    assert (got[1]["join_rows"], got[1]["pairs"]) == ex.nested_loop_left_join(rv, rm, lv, lm)[:2]
    assert got[0]["parent_rows"] == int(rm.sum()) and got[1]["parent_rows"] == int(lm.sum())


@pytest.mark.parametrize("type,lo,hi", [(pa.int8(), -128, 127), (pa.uint16(), 0, 600), (pa.int32(), -2**31, -2**31 + 600)],
                         ids=["int8", "uint16", "int32"])
def test_narrow_children_against_an_int64_set(type, lo, hi):
    rng = np.random.default_rng(9)
    values = rng.integers(lo, hi + 1, 4000)
    mask = rng.random(4000) >= 0.2
    records = mixed_counts(np.arange(lo, hi + 1, 3), 10)
    T.init()
    for mem in (T.MEM_DEVICE, T.MEM_HOST):
        st = T.State(counted_plan())
        set_parent(st, records)
        st.update([column(ints(values, type, mask), mem)])
        assert read(st) == ex.walk_np(values, mask, records)


# ---- batching and the ways a state travels ------------------------------------------------------------------------------------
N_BIG = 200_000


@pytest.fixture(scope="module")
def big():
    """one child column against a count-array and a counted-hash set"""
    rng = np.random.default_rng(13)
    base = rng.zipf(1.3, N_BIG) % 5000 - 100
    mask = rng.random(N_BIG) >= 0.05
    child0, child = ints(base, mask=mask), ints(base * 3, mask=mask)
    sets = [mixed_counts(np.arange(-50, 4000), 14),
            mixed_counts(np.concatenate([np.arange(-100, 2000) * 6, [I64_MAX - 5, -1]]), 15)]
    want = [exact(child0, sets[0]), exact(child, sets[1])]
    assert [w[0]["route"] for w in want] == [ex.ROUTE_COUNT_ARRAY, ex.ROUTE_COUNT_HASH]
    assert all(w[0]["missing_keys"] > 100 and w[1]["pairs"] > w[0]["matched"] for w in want)
    return [child0, child], sets, want


def big_plan():
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 1)])
    plan.set_key_probe_counted(0)
    plan.set_key_probe_counted(1)
    return plan


def big_state(plan, sets):
    st = T.State(plan)
    for i, records in enumerate(sets):
        set_parent(st, records, i)
    return st


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192)])
def test_batching_independence(big, mem, cuts):
    children, sets, want = big
    T.init()
    st = big_state(big_plan(), sets)
    for b in cut([column(c, mem) for c in children], N_BIG, cuts):
        st.update(b)
    assert [read(st, i) for i in range(2)] == want


def test_state_algebra(big):
    children, sets, want = big
    T.init()
    cols = [column(c) for c in children]
    parts = cut(cols, N_BIG, [70_000, 150_001])
    plan = big_plan()
    st = big_state(plan, sets)
    for p in parts:
        st.update(p)
    assert [read(st, i) for i in range(2)] == want
    # reset keeps the set
    st.reset()
    empty, pairs = read(st)
    assert (empty["seen"], empty["entries"], empty["route"], pairs["pairs"]) == (0, {}, ex.ROUTE_COUNT_ARRAY, 0)
    assert {k: pairs[k] for k in ("parent_rows", "parent_count_digest", "max_count")} == \
        {k: want[0][1][k] for k in ("parent_rows", "parent_count_digest", "max_count")}
    st.update(cols)
    assert [read(st, i) for i in range(2)] == want
    # a merge of three states
    states = []
    for p in parts:
        s = big_state(plan, sets)
        s.update(p)
        states.append(s)
    states[0].merge(states[1:])
    assert [read(states[0], i) for i in range(2)] == want
    # a blob round trip; equal states give equal bytes
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    held = [(dict(w[0], route=0), w[1]) for w in want]  # (a deserialized state holds no set)
    assert [read(back, i) for i in range(2)] == held and back.serialize() == blob == st.serialize()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
        back.update(cols)
    # the same keys with other counts are another set
    other_counts = [(k, c + 1) for k, c in sets[0]]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*another parent set"):
        set_parent(back, other_counts, 0)
    for i in range(2):
        set_parent(back, sets[i], i)
    back.update(cols)
    doubled, pairs = read(back, 1)
    assert pairs["pairs"] == 2 * want[1][1]["pairs"] and doubled["matched"] == 2 * want[1][0]["matched"]
    assert doubled["route"] == ex.ROUTE_COUNT_HASH
    other = big_state(plan, [other_counts, sets[1]])
    other.update(parts[0])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different parent sets"):
        st.merge([other])
    assert [read(st, i) for i in range(2)] == want


def test_plain_and_counted_do_not_unite(big):
    children, sets, _ = big
    T.init()
    cols = [column(c) for c in children]
    plain_plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 1)])
    plain_plan.set_key_probe(0)
    plain_plan.set_key_probe(1)
    plain = big_state(plain_plan, sets)
    plain.update(cols)
    counted = big_state(big_plan(), sets)
    counted.update(cols)
    before = [read(counted, i) for i in range(2)]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(big_plan(), plain.serialize())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plain_plan, counted.serialize())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        counted.merge([plain])
    assert [read(counted, i) for i in range(2)] == before


def test_counted_tasks_of_one_route_share_a_launch(big):
    children, sets, want = big
    T.init()
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 1), spec(T.KEY_PROBE, 0)])
    for k in range(3):
        plan.set_key_probe_counted(k)
    st = big_state(plan, sets + [sets[0][:100]])
    st.profile_enable(True)
    st.update([column(c) for c in children])
    st.finalize()
    assert st.profile_get("key_probe")["launches"] == 2  # (two routes: one launch each)
    assert [read(st, i) for i in range(2)] == want and read(st, 2) == exact(children[0], sets[0][:100])


# ---- end to end: JoinCoverageConstraint through ValidationSuite.run(.., tables=..) ----------------------------------------------
def run_constraint(constraint, tables, builder=None):
    cb = S.Check.builder("c").level(S.Level.ERROR)
    cb = builder(cb) if builder else cb.constraint(constraint)
    r = S.ValidationSuite.builder("s").check(cb.build()).build().run(None, tables=tables)
    m = r.report.metrics
    assert m.total_checks == 1 and m.passed_checks + m.failed_checks == 1
    metric = m.custom_metrics.get("c.join_coverage")
    if m.passed_checks:
        assert r.is_success() and not r.report.issues
        return "success", metric, None
    assert len(r.report.issues) == 1 and r.report.issues[0].constraint_name == "join_coverage"
    message = r.report.issues[0].message
    return ("error" if message.startswith("Error evaluating constraint: ") else "failure"), metric, message


def golden_cases():
    with open(os.path.join(HERE, "golden", "join_coverage_vectors.json")) as f:
        return json.load(f)["cases"]


def sides(case):
    out = []
    for key in ("left", "right"):
        out.append(([v or 0 for v in case[key]], [v is not None for v in case[key]]))
    return out


def constraint_of(case):
    c = S.JoinCoverageConstraint(case["left_table"], case["right_table"]).on(case["left_column"], case["right_column"])
    c = c.expect_match_rate(case["expected"]).coverage_type(case["coverage_type"]).distinct_only(case["distinct_only"])
    return c.max_examples_reported(case.get("max_examples", 100))


@pytest.mark.parametrize("case", golden_cases(), ids=[c["name"] for c in golden_cases()])
def test_the_golden_tables_through_the_suite(case):
    T.init()
    tables = {case["left_table"]: pa.table({"id": pa.array(range(len(case["left"])), pa.int64()),
                                            case["left_column"]: pa.array(case["left"], pa.int64())}),
              case["right_table"]: pa.table({case["right_column"]: pa.array(case["right"], pa.int64()),
                                             "name": pa.array(["n"] * len(case["right"]), pa.string())})}
    status, metric, message = run_constraint(constraint_of(case), tables)
    (lv, lm), (rv, rm) = sides(case)
    want = ex.coverage(case["left_table"], case["right_table"], lv, lm, rv, rm, case["coverage_type"],
                       case["distinct_only"], case["expected"], case.get("max_examples", 100))
    assert (status, metric, message) == want
    assert status == case["status"] and (metric is None) == (case["metric"] is None)
    assert metric is None or abs(metric - case["metric"]) <= 1e-12
    assert case.get("message") is None or message == case["message"]
    # the same constraint from its JSON form
    again = S.JoinCoverageConstraint.from_spec(json.loads(json.dumps(constraint_of(case).spec)))
    assert run_constraint(again, tables) == (status, metric, message)


def test_the_big_tables_through_the_suite(big):
    children, sets, want = big
    T.init()
    rng = np.random.default_rng(16)
    right_rows = np.repeat(np.array([k for k, _ in sets[1]], np.int64), [c for _, c in sets[1]])
    right = ints(rng.permutation(right_rows), mask=rng.random(len(right_rows)) >= 0.02)
    left = children[1]
    (lv, lm), (rv, rm) = split(left), split(right)
    tables = {"orders": pa.table({"customer_id": left, "small": left.cast(pa.int32()),
                                  "f": pa.array(np.arange(N_BIG, dtype=np.float64))}),
              "customers": pa.table({"id": right, "name": pa.array(["n"] * len(right), pa.string())})}
    for kind in (ex.LEFT, ex.RIGHT, ex.BIDIRECTIONAL):
        for expected in (0.0, 1.0):
            c = S.JoinCoverageConstraint("orders", "customers").on("customer_id", "id").coverage_type(kind)
            got = run_constraint(c.expect_match_rate(expected), tables)
            assert got == ex.coverage("orders", "customers", lv, lm, rv, rm, kind, False, expected)
    c = S.JoinCoverageConstraint("orders", "customers").on("small", "id").distinct_only(True).max_examples_reported(7)
    got = run_constraint(c.expect_match_rate(1.0), tables)
    assert got == ex.coverage("orders", "customers", lv, lm, rv, rm, ex.LEFT, True, 1.0, 7) and got[1] > 1.0
    got = run_constraint(None, tables, builder=lambda cb: cb.join_coverage("orders", "customers"))
    assert got[0] == "error" and "No join keys specified. Use .on() or .on_multiple() to set join keys" in got[2]
    c = S.JoinCoverageConstraint("orders", "customers").on("f", "id")
    got = run_constraint(c, tables)
    assert got[0] == "error" and "Float64" in got[2] and "orders.f" in got[2]
    c = S.JoinCoverageConstraint("orders", "customers").on("customer_id", "id").max_missing_keys(16).max_examples_reported(10**6)
    got = run_constraint(c, tables)
    assert got[0] == "failure" and "(at least " in got[2]
