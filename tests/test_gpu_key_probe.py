"""TGX_CHECK_KEY_PROBE on the device, held against tests/exact_key_probe.py: every counter, every missing key with its
rows, parent_keys, parent_digest and the route are compared for equality with the exact walk, and the three identities
are checked on every read -- for every shape of parent set (empty, one key, dense, the bitmap / hash threshold, a
wrapping range, colliding keys, duplicates, the marker key on either side), every class of missing keys, NULLs, Arrow
offsets, narrow types, every batching and every way a state travels (reset, merge, blob, tgx_allreduce), and end to end
through ForeignKeyConstraint."""
import ctypes
import json
import os
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_key_probe as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2**63, 2**63 - 1
SHARE = 1024 * 16  # rows a workgroup takes before a second one is launched
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- columns and states -------------------------------------------------------------------------------------------------
def padded(buf):
    if buf is None:
        return None
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return to_device(np.concatenate([raw, np.zeros(64, np.uint8)]))


def on_device(col):
    values, validity = col._keep[:2]
    return T.Column(col.c.type, col.c.length, values=padded(values), validity=padded(validity), offset=col.c.offset,
                    mem=T.MEM_DEVICE)


def column(arr, mem=T.MEM_DEVICE):
    col = arr if isinstance(arr, T.Column) else T.Column.from_arrow(arr)
    if mem == T.MEM_DEVICE:
        return on_device(col)
    col.c.mem = mem
    return col


def ints(values, type=pa.int64(), mask=None):
    return pa.array(values, type=type, mask=None if mask is None else ~np.asarray(mask))


def split(arr):
    """(int64 values with 0 at NULL rows, bool mask or None) of a pyarrow integer array"""
    mask = None if arr.null_count == 0 else np.asarray(arr.is_valid())
    return np.asarray(arr.fill_null(0)).astype(np.int64), mask


def cut(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def records(keys):
    """{key, count} records of the given keys (an int64 array, duplicates allowed) in device memory"""
    keys = np.asarray(keys, np.int64)
    recs = np.ones((len(keys), 2), np.uint64)
    recs[:, 0] = keys.view(np.uint64)
    return to_device(recs.reshape(-1)) if len(keys) else None


def set_parent(st, keys, i=0):
    d = records(keys)
    st.key_probe_set_parent(i, d.data_ptr() if d is not None else None, len(keys))


def plan_of(bounds=(10000,), columns=None, extra=()):
    plan = T.Plan([spec(T.KEY_PROBE, columns[k] if columns else 0) for k in range(len(bounds))] + list(extra))
    for k, b in enumerate(bounds):
        plan.set_key_probe(k, b)
    return plan


def state_of(plan, parents):
    st = T.State(plan)
    for i, keys in enumerate(parents):
        set_parent(st, keys, i)
    return st


def read(st, i=0):
    summary, entries = st.key_probe(i)
    got = dict(summary, entries=entries)
    assert got["seen"] == got["non_null"] + got["null_rows"]
    assert got["non_null"] == got["matched"] + got["missing_rows"]
    assert got["missing_rows"] == got["counted"] + got["overflow_rows"]
    assert got["counted"] == sum(entries.values()) and got["missing_keys"] == len(entries)
    return got


def exact(child, parent, bound=10000):
    values, mask = split(child)
    want = ex.walk_np(values, mask, parent, None, bound)
    del want["within_bound"]
    return want


def check(child, parent, bound=10000, mem=T.MEM_DEVICE, cuts=None, route=None, want=None):
    T.init()
    plan = plan_of((bound,))
    st = state_of(plan, [parent])
    for b in cut([column(child, mem)], len(child), cuts):
        st.update(b)
    want = want or exact(child, parent, bound)
    got = read(st)
    assert got == want and list(got["entries"]) == list(want["entries"])  # (the order too: ascending)
    if route is not None:
        assert got["route"] == route
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.matches, r.distinct) == (want["seen"], want["non_null"], want["matched"], want["missing_keys"])
    return st, plan, want


# ---- rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, SHARE - 1, SHARE, SHARE + 1])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    child = ints(rng.integers(-30, 60, n), mask=rng.random(n) >= 0.1)
    check(child, np.arange(0, 40), route=ex.ROUTE_BITMAP)
    check(child, np.arange(0, 40) * 1_000_003, route=ex.ROUTE_HASH)


# ---- parent sets ------------------------------------------------------------------------------------------------------------
def test_an_empty_set_and_a_set_of_one_key():
    rng = np.random.default_rng(1)
    child = ints(rng.integers(0, 5, 3000), mask=rng.random(3000) >= 0.2)
    _, _, want = check(child, np.zeros(0, np.int64), route=ex.ROUTE_EMPTY)
    assert want["matched"] == 0 and want["parent_keys"] == 0 and want["parent_digest"] == 0
    _, _, want = check(child, np.array([3]), route=ex.ROUTE_BITMAP)
    assert want["matched"] > 0 and want["missing_keys"] == 4


def test_a_dense_range_at_its_edges_and_at_a_word_boundary():
    lo, hi = -1000, 2000  # bit 31 / 32 of the first word: keys -969 and -968
    parent = np.arange(lo, hi + 1)
    edge = [lo - 1, lo, hi, hi + 1, lo + 31, lo + 32, lo + 63, lo + 64, I64_MIN, I64_MAX]
    _, _, want = check(ints(edge * 40), parent, route=ex.ROUTE_BITMAP)
    assert sorted(want["entries"]) == [I64_MIN, lo - 1, hi + 1, I64_MAX]
    holes = parent[(parent - lo) % 32 != 31]  # the last bit of every word is clear, its neighbours are set
    _, _, want = check(ints(np.arange(lo - 40, hi + 40)), holes, route=ex.ROUTE_BITMAP)
    assert lo + 31 in want["entries"] and lo + 30 not in want["entries"] and lo + 32 not in want["entries"]


def test_the_threshold_between_the_bitmap_and_the_hash_table():
    child = ints(np.arange(-5, 520))
    at = np.array([0, 100, 300, 511])  # range 512 == 128 * 4
    beyond = np.array([0, 100, 300, 512])
    check(child, at, route=ex.ROUTE_BITMAP)
    check(child, beyond, route=ex.ROUTE_HASH)
    # (the records count, not the distinct keys: a duplicate widens what the bitmap may span)
    check(child, np.array([0, 100, 300, 512, 512]), route=ex.ROUTE_BITMAP)


def test_both_extremes_wrap_the_range():
    parent = np.array([I64_MIN, I64_MAX])
    assert ex.route_of(parent) == ex.ROUTE_HASH
    child = ints([I64_MIN, I64_MAX, 0, -1, I64_MIN + 1, I64_MAX - 1, None] * 30)
    _, _, want = check(child, parent, route=ex.ROUTE_HASH)
    assert sorted(want["entries"]) == [I64_MIN + 1, -1, 0, I64_MAX - 1]
    check(child, np.array([I64_MIN, I64_MAX, -1, 0]), route=ex.ROUTE_HASH)


def test_keys_that_share_one_home_slot_wrap_past_the_tables_end():
    n = 8
    slots = ex.hash_slots(n)  # 16
    cand = np.arange(1, 4000, dtype=np.int64) * 1_000_000_007
    home = ex.mix64_np(cand.view(np.uint64)) & np.uint64(slots - 1)
    same = cand[home == np.uint64(slots - 1)]  # all start at the last slot: the chain goes on at slot 0
    assert len(same) >= 2 * n
    parent, others = same[:n], same[n:2 * n]
    child = ints(np.concatenate([parent, others, parent[::-1], others[:3]]))
    _, _, want = check(child, parent, route=ex.ROUTE_HASH)
    assert want["matched"] == 2 * n and sorted(want["entries"]) == sorted(others.tolist())


def test_duplicate_records():
    rng = np.random.default_rng(2)
    child = ints(rng.integers(0, 3000, 5000))
    for keys in (np.arange(0, 2000, 7), np.arange(0, 2000, 7) * 1_000_003):
        dup = np.concatenate([keys, keys[::3], keys])
        _, _, want = check(child, rng.permutation(dup))
        assert want["parent_keys"] == len(keys) and want["parent_digest"] == ex.digest(keys.tolist())


@pytest.mark.parametrize("dense", [True, False])
def test_the_marker_key_on_either_side(dense):
    base = np.arange(-3, 40) if dense else np.arange(-3, 40) * 1_000_003
    route = ex.ROUTE_BITMAP if dense else ex.ROUTE_HASH
    without = base[base != -1]
    with_marker = np.concatenate([without, [-1]])
    marker_child = ints([-1, 5, -1, None, -2, -1, 77777] * 50)
    plain_child = ints([5, None, -2, 77777, 0] * 50)
    _, _, want = check(plain_child, with_marker, route=route)           # in the parent only
    assert -1 not in want["entries"]
    _, _, want = check(marker_child, without, route=route)             # in the child only: missing, and exact
    assert want["entries"][-1] == 150
    _, _, want = check(marker_child, with_marker, route=route)          # in both
    assert -1 not in want["entries"] and want["matched"] >= 150
    _, _, want = check(ints([-1] * 300), np.zeros(0, np.int64))          # missing from an empty set
    assert want["entries"] == {-1: 300}


# ---- missing keys -----------------------------------------------------------------------------------------------------------
def test_no_key_missing_and_one_key_on_every_row():
    rng = np.random.default_rng(3)
    n = 20_000
    _, _, want = check(ints(rng.integers(0, 500, n)), np.arange(500))
    assert want["missing_rows"] == 0 and want["entries"] == {}
    _, _, want = check(ints(np.full(n, 42)), np.arange(100, 200))
    assert want["entries"] == {42: n}
    check(ints(np.full(n, 42), mask=np.arange(n) % 3 != 0), np.arange(100, 200) * 1_000_003)


def test_64_distinct_missing_keys_in_a_wave():
    n = 20_000
    _, _, want = check(ints(np.arange(n) % 64 * 1_000_003 + 7), np.arange(64) * 1_000_003)
    assert want["missing_keys"] == 64 and want["matched"] == 0


def test_more_missing_keys_than_a_workgroups_lds_table_holds():
    """30 000 missing keys in 8 workgroups' shares of 15 000 rows: a share holds some 11 000 of them, more than the 8192
    LDS slots take, so rows go to the global table directly"""
    rng = np.random.default_rng(4)
    v = rng.integers(0, 30_000, 120_000) * 1_000_003 - 5
    _, _, want = check(ints(v), np.arange(0, 30_000, 2) * 1_000_003 - 5, bound=40_000)
    assert want["missing_keys"] > 8192 and want["matched"] > 0


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_max_missing_keys_and_one_above(extra):
    n = 1000 + extra
    v = np.random.default_rng(5).permutation(n) * 7 - 3000
    _, _, want = check(ints(np.concatenate([v, [1, 2, 1]])), np.array([1, 2]), bound=1000)
    assert want["missing_keys"] == n and want["overflow_rows"] == 0  # one above: reported, the caller compares


def test_more_missing_keys_than_the_global_table_has_slots():
    rng = np.random.default_rng(6)
    v = rng.integers(0, 200, 30_000)
    T.init()
    st = state_of(plan_of((16,)), [np.arange(0, 200, 2)])  # 32 slots for 100 missing keys
    st.update([column(ints(v))])
    got, true = read(st), ex.walk_np(v, None, np.arange(0, 200, 2), None)
    assert got["overflow_rows"] > 0 and got["missing_keys"] <= 32
    assert (got["seen"], got["non_null"], got["matched"], got["missing_rows"]) == (30_000, 30_000, true["matched"], true["missing_rows"])
    assert all(0 < c <= true["entries"][k] for k, c in got["entries"].items())  # only keys of the table, none counted too often


# ---- NULLs and layout -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", [0.0, 0.3, 1.0])
def test_null_rates(nulls):
    rng = np.random.default_rng(7)
    n = 30_000
    for parent in (np.arange(0, 900, 2), np.arange(0, 900, 2) * 1_000_003):
        scale = 1 if parent[1] == 2 else 1_000_003
        check(ints(rng.integers(0, 1000, n) * scale, mask=rng.random(n) >= nulls), parent)


def test_a_column_without_a_validity_buffer():
    rng = np.random.default_rng(8)
    child = ints(rng.integers(0, 1000, 10_000))
    assert child.buffers()[0] is None
    _, _, want = check(child, np.arange(0, 900, 3))
    assert want["null_rows"] == 0


@pytest.mark.parametrize("offset", [1, 7, 8, 63, 64, 65])
def test_arrow_offsets(offset):
    rng = np.random.default_rng(9 + offset)
    n = 5000
    whole = ints(rng.integers(0, 1000, n + offset), mask=rng.random(n + offset) >= 0.3)
    child = whole.slice(offset)
    assert child.offset == offset
    check(child, np.arange(0, 900, 3))
    check(child, np.arange(0, 900, 3) * 1_000_003 + 1, mem=T.MEM_HOST)


# ---- column types -----------------------------------------------------------------------------------------------------------
NARROW = [(pa.int8(), -128, 127), (pa.int16(), -300, 300), (pa.uint8(), 0, 255), (pa.uint16(), 0, 600),
          (pa.uint32(), 2**32 - 300, 2**32 - 1), (pa.int32(), -2**31, -2**31 + 600), (pa.date32(), -300, 300)]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST])
@pytest.mark.parametrize("type,lo,hi", NARROW, ids=[str(t[0]) for t in NARROW])
def test_narrow_child_types(type, lo, hi, mem):
    rng = np.random.default_rng(10)
    n = 4000
    values = rng.integers(lo, hi + 1, n)
    mask = rng.random(n) >= 0.2
    arr = pa.array(values, pa.int32(), mask=~mask).cast(type) if type == pa.date32() else ints(values, type, mask)
    parent = np.arange(lo, hi + 1, 3)  # the sign- or zero-extended values
    want = ex.walk_np(values, mask, parent, None)
    del want["within_bound"]
    check(arr, parent, mem=mem, want=want)


def test_an_int32_parent_joins_an_int64_child():
    """the parent's set comes from a DISTINCT spec over an Int32 column, negative keys among them: DISTINCT keeps the
    sign-extended int64 value, so the join is SQL's coercion"""
    rng = np.random.default_rng(11)
    T.init()
    p_values = rng.integers(-500, 500, 3000)
    p_mask = rng.random(3000) >= 0.1
    pplan = T.Plan([spec(T.DISTINCT, 0)])
    pst = T.State(pplan)
    pst.update([column(ints(p_values, pa.int32(), p_mask))])
    ptr, counts = pst.distinct_export(0, 1)
    child = ints(rng.integers(-700, 700, 20_000), mask=rng.random(20_000) >= 0.1)
    values, mask = split(child)
    want = ex.walk_np(values, mask, p_values, p_mask, n_records=counts[0])
    del want["within_bound"]
    assert counts[0] == want["parent_keys"] and want["matched"] > 0 and min(want["entries"]) < -500
    st = T.State(plan_of())
    st.key_probe_set_parent(0, ptr, counts[0])
    st.update([column(child)])
    assert read(st) == want


def test_two_specs_on_one_column_with_different_parent_sets():
    rng = np.random.default_rng(12)
    child = ints(rng.integers(0, 1000, 50_000) * 1_000_003, mask=rng.random(50_000) >= 0.1)
    parents = [np.arange(0, 1000, 2) * 1_000_003, np.arange(0, 1000), np.zeros(0, np.int64)]  # hash, bitmap, empty
    T.init()
    st = state_of(plan_of((10000, 10000, 10000), columns=[0, 0, 0]), parents)
    st.update([column(child)])
    for i, p in enumerate(parents):
        assert read(st, i) == exact(child, p)
    assert [read(st, i)["route"] for i in range(3)] == [ex.ROUTE_HASH, ex.ROUTE_BITMAP, ex.ROUTE_EMPTY]


def test_every_mode_in_one_plan_with_a_route_that_spans_two_launches():
    """nine plain specs on the bitmap route (a launch takes eight tasks: the ninth rides a second launch alone), a plain
    one on the hash route, a counted one, one that gathers rows and one on string keys, in one plan over an Int64 and a
    Utf8 column of 65 rows (a wave and a row), each probing spec with five keys of its own"""
    import torch

    import exact_join_coverage as exj
    import exact_key_probe_strings as exs
    import fp_reference as fpr

    rng = np.random.default_rng(15)
    n, key = 65, bytes(range(1, 17))
    child = ints(rng.integers(-3, 40, n), mask=rng.random(n) >= 0.15)
    words = ["k%d" % v for v in rng.integers(0, 12, n)]
    strings = [None if rng.random() < 0.15 else w for w in words]
    assert 0 < child.null_count < n and 0 < strings.count(None) < n
    bitmaps = [np.arange(5) + 3 * j for j in range(9)]
    spread = np.array([0, 7, 1_000_003, 2_000_006, 30])
    counted = [(2, 3), (5, 1), (7, 2), (11, 4), (36, 1)]
    parent_words = ["k1", "k4", "k5", "k9", "zz"]
    assert all(ex.route_of(p) == ex.ROUTE_BITMAP for p in bitmaps) and ex.route_of(spread) == ex.ROUTE_HASH

    T.init()
    plan = T.Plan([spec(T.KEY_PROBE, 0) for _ in range(12)] + [spec(T.KEY_PROBE, 1)])
    plan.set_fingerprint_key(key)
    for i in range(10):
        plan.set_key_probe(i, 100)
    plan.set_key_probe_counted(10, 100)
    plan.set_key_probe_rows(11)
    plan.set_key_probe_strings(12, 100, 256)
    st = T.State(plan)
    st.profile_enable(True)
    for i, keys in enumerate(bitmaps + [spread]):
        set_parent(st, keys, i)
    recs = to_device(np.array(counted, np.int64).view(np.uint64).reshape(-1))
    st.key_probe_set_parent(10, recs.data_ptr(), len(counted))
    fps = [fpr.fingerprint(key, w.encode()) for w in parent_words]
    frecs = to_device(np.array([(fa, fb, 1, 0) for fa, fb in fps], np.uint64).reshape(-1))
    st.key_probe_set_parent(12, frecs.data_ptr(), len(fps))
    scol = T.Column.from_arrow(pa.array(strings, pa.string()))
    validity, offsets, data = scol._keep[1:4]
    st.update([column(child), T.Column(scol.c.type, n, validity=padded(validity), offsets=padded(offsets),
                                       data=padded(data), mem=T.MEM_DEVICE)])

    for i, keys in enumerate(bitmaps + [spread]):
        assert read(st, i) == exact(child, keys, 100), i
    values, mask = split(child)
    want, want_pairs = exj.walk_np(values, mask, counted, 100)
    assert read(st, 10) == want and st.key_probe_pairs(10) == want_pairs
    assert want["route"] == exj.ROUTE_COUNT_HASH and want_pairs["pairs"] > want["matched"] > 0

    ptr, count = st.key_probe_rows(11)
    assert count == n - child.null_count

    class Records:
        __cuda_array_interface__ = {"shape": (count * 16,), "typestr": "|u1", "data": (ptr, False), "version": 2}

    gathered = torch.as_tensor(Records(), device="cuda").clone().cpu().numpy().view(np.int64).reshape(count, 2)
    assert sorted(gathered[:, 0].tolist()) == sorted(values[mask].tolist()) and set(gathered[:, 1].tolist()) == {1}

    want = exs.walk(strings, parent_words, 256, 100)
    del want["within_bound"]
    digest = sum(ex.mix64(ex.mix64(fa ^ ex.DIGEST_SALT) ^ fb) for fa, fb in set(fps)) & ex.M64
    want.update(max_value_bytes=256, parent_digest=digest, route=5)
    summary, entries = st.key_probe_strings(12)
    assert dict(summary, entries=entries) == want and list(entries) == list(want["entries"])
    assert want["matched"] > 0 and want["missing_keys"] > 0
    # the bitmap route's nine tasks in two launches, then one launch each for the hash route, the counted route and the strings
    assert st.profile_get("key_probe")["launches"] == 5 and st.profile_get("key_probe_rows")["launches"] == 1


# ---- batching and the ways a state travels ------------------------------------------------------------------------------------
N_BIG = 200_000


@pytest.fixture(scope="module")
def big():
    """one child column against a hash-route and a bitmap-route parent"""
    rng = np.random.default_rng(13)
    child = ints((rng.zipf(1.3, N_BIG) % 5000 - 100) * 3, mask=rng.random(N_BIG) >= 0.05)
    parents = [np.arange(-50, 4000) * 3, np.concatenate([np.arange(-100, 2000) * 6, [I64_MAX - 5]])]
    want = [exact(child, p) for p in parents]
    assert [w["route"] for w in want] == [ex.ROUTE_BITMAP, ex.ROUTE_HASH] and all(w["missing_keys"] > 100 for w in want)
    return child, parents, want


def big_plan(extra=()):
    return plan_of((10000, 10000), columns=[0, 0], extra=extra)


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192), (T.MEM_HOST, [3, 8195, 8196, 150_001])])
def test_batching_independence(big, mem, cuts):
    child, parents, want = big
    T.init()
    st = state_of(big_plan(), parents)
    for b in cut([column(child, mem)], N_BIG, cuts):
        st.update(b)
    assert [read(st, i) for i in range(2)] == want


def test_state_algebra(big):
    child, parents, want = big
    T.init()
    col = column(child)
    parts = cut([col], N_BIG, [70_000, 150_001])
    plan = big_plan()
    st = state_of(plan, parents)
    st.update(parts[0])
    assert read(st) == exact(child.slice(0, 70_000), parents[0])  # read half-way, then on
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*before the state's first batch"):
        set_parent(st, parents[0])
    st.update(parts[1])
    st.update(parts[2])
    assert [read(st, i) for i in range(2)] == want
    # reset keeps the parent set
    st.reset()
    empty = read(st)
    assert (empty["seen"], empty["entries"], empty["route"]) == (0, {}, ex.ROUTE_BITMAP)
    assert (empty["parent_keys"], empty["parent_digest"]) == (want[0]["parent_keys"], want[0]["parent_digest"])
    st.update([col])
    assert [read(st, i) for i in range(2)] == want
    # merge of three states
    states = []
    for p in parts:
        s = state_of(plan, parents)
        s.update(p)
        states.append(s)
    states[0].merge(states[1:])
    assert [read(states[0], i) for i in range(2)] == want
    # a blob round trip; equal states give equal bytes
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    held = [dict(w, route=0) for w in want]  # (a deserialized state holds no set)
    assert [read(back, i) for i in range(2)] == held and back.serialize() == blob == st.serialize()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
        back.update([col])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*another parent set"):
        set_parent(back, parents[0][:-1], 0)
    for i in range(2):
        set_parent(back, parents[i], i)
    back.update([col])
    doubled = read(back, 1)
    assert doubled["entries"] == {k: 2 * c for k, c in want[1]["entries"].items()} and doubled["matched"] == 2 * want[1]["matched"]
    assert doubled["route"] == ex.ROUTE_HASH
    # states of different parent sets do not merge
    other = state_of(plan, [parents[0][1:], parents[1]])
    other.update(parts[0])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different parent sets"):
        st.merge([other])
    assert [read(st, i) for i in range(2)] == want
    tight = plan_of((10000, 9999), columns=[0, 0])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(tight, blob)


def test_a_state_without_a_parent_set_refuses_batches():
    T.init()
    st = T.State(plan_of((100, 100), columns=[0, 0]))
    set_parent(st, np.arange(5), 0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*needs its parent set"):
        st.update([column(ints([1, 2, 3]))])
    set_parent(st, np.arange(2), 1)
    st.update([column(ints([1, 2, 3]))])
    assert read(st, 1)["entries"] == {2: 1, 3: 1} and read(st, 0)["entries"] == {}


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(big, world, device_buffers):
    """every rank a thread with its own state, parent sets and row shard, tgx_allreduce over the thread-barrier
    transport; every rank ends with the table's counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    child, parents, want = big
    T.init()
    whole = [column(child)]
    plan = big_plan(extra=[spec(T.COUNT, 0)])
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(N_BIG, world, rank)
            st = state_of(plan, parents)
            comm = thread_comm(group, rank, device_buffers=device_buffers)
            for _ in range(2):
                res = sharded_suite_step(plan, st, [c.sliced(lo, hi - lo) for c in whole], comm)
            results[rank] = (res, [read(st, i) for i in range(2)])
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
        assert res[2].total == N_BIG and res[0].non_null == res[2].non_null


# ---- isolation ------------------------------------------------------------------------------------------------------------------
def test_the_kind_leaves_the_other_kinds_bit_for_bit(big):
    child, parents, want = big
    T.init()
    rng = np.random.default_rng(14)
    cols = [column(child), column(pa.array(rng.standard_normal(N_BIG)))]
    others = [spec(T.COUNT, 0), spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.NUMERIC_STATS, 0),
              spec(T.NUMERIC_STATS, 1, flags=T.FLAG_VARIANCE), spec(T.COMOMENTS, 0, column2=1), spec(T.VALUE_COUNTS, 0)]
    alone_plan = T.Plan(others)
    alone_plan.set_value_counts(5)
    alone = T.State(alone_plan)
    alone.update(cols)
    ref = alone.finalize()
    plan = big_plan(extra=others)
    plan.set_value_counts(7)
    st = state_of(plan, parents)
    st.update(cols)
    res = st.finalize()
    assert [read(st, i) for i in range(2)] == want
    assert st.value_counts(7) == alone.value_counts(5)
    for got, r in zip(res[2:], ref):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r))


def test_a_plan_without_the_kind_profiles_no_such_kernel(big):
    child, parents, _ = big
    T.init()
    col = column(child)
    launches = []
    for plan, sets in ((T.Plan([spec(T.COUNT, 0), spec(T.NUMERIC_STATS, 0)]), []),
                       (plan_of((10000,), extra=[spec(T.COUNT, 0)]), parents[:1]),
                       (big_plan(), parents)):
        st = T.State(plan)
        st.profile_enable(True)
        for i, p in enumerate(sets):
            set_parent(st, p, i)
        st.update([col])
        st.finalize()
        launches.append((st.profile_get("key_probe")["launches"], st.profile_get("key_probe_build")["launches"]))
    assert launches == [(0, 0), (1, 1), (2, 2)]  # (two routes: one launch each)


def test_other_column_types_are_unsupported_and_the_state_stays_usable():
    """the refused batches go to the very state that is read afterwards"""
    T.init()
    n = 1000
    st = state_of(plan_of(), [np.arange(0, 10, 2)])
    refused = [(pa.array(np.arange(n, dtype=np.float64)), "Float64"), (pa.array(np.arange(n, dtype=np.float32)), "Float32"),
               (pa.array(np.arange(n, dtype=np.uint64)), "UInt64"), (pa.array(np.arange(n) % 2 == 0), "Boolean")]
    for arr, name in refused:
        for mem in (T.MEM_HOST, T.MEM_DEVICE):
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*KEY_PROBE.*" + name):
                st.update([column(arr, mem)])
    strings = [pa.array(["a", "b"] * 500, pa.string()), pa.array(["a", "b"] * 500, pa.large_string()),
               pa.array(["a", "b"] * 500, pa.string_view()), pa.array(["a", "b"] * 500, pa.string()).dictionary_encode()]
    for arr in strings:
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*KEY_PROBE.*strings"):
            st.update([T.Column.from_arrow(arr)])
    assert read(st)["seen"] == 0
    st.update([column(ints(np.arange(n) % 10))])
    got = read(st)
    assert got["seen"] == n and got["entries"] == {k: 100 for k in (1, 3, 5, 7, 9)} and got["matched"] == 500


# ---- end to end: ForeignKeyConstraint through ValidationSuite.run(.., tables=..) ----------------------------------------------
def run_constraint(constraint, tables, builder=False):
    """(status of the constraint, its metric, its message) of a one-constraint suite"""
    cb = S.Check.builder("c").level(S.Level.ERROR)
    cb = cb.foreign_key(constraint.child_column(), constraint.parent_column()) if builder else cb.constraint(constraint)
    r = S.ValidationSuite.builder("s").check(cb.build()).build().run(None, tables=tables)
    m = r.report.metrics
    assert m.total_checks == 1 and m.passed_checks + m.failed_checks == 1
    metric = m.custom_metrics.get("c.foreign_key")
    if m.passed_checks:
        assert r.is_success() and not r.report.issues
        return "success", metric, None
    assert len(r.report.issues) == 1 and r.report.issues[0].constraint_name == "foreign_key"
    message = r.report.issues[0].message
    return ("error" if message.startswith("Error evaluating constraint: ") else "failure"), metric, message


def golden_cases():
    with open(os.path.join(HERE, "golden", "foreign_key_vectors.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", golden_cases(), ids=[c["name"] for c in golden_cases()])
def test_the_golden_tables_through_the_suite(case):
    T.init()
    (ct, cc), (pt, pc) = case["child_column"].split("."), case["parent_column"].split(".")
    tables = {ct: pa.table({"id": pa.array(range(len(case["child"])), pa.int64()), cc: pa.array(case["child"], pa.int64())}),
              pt: pa.table({pc: pa.array(case["parent"], pa.int64()), "name": pa.array(["n"] * len(case["parent"]), pa.string())})}
    c = S.ForeignKeyConstraint(case["child_column"], case["parent_column"]).allow_nulls(case["allow_nulls"])
    status, metric, message = run_constraint(c, tables)
    child = [None if v is None else 1 for v in case["child"]]
    state = ex.walk([v or 0 for v in case["child"]], child, [v or 0 for v in case["parent"]],
                    [v is not None for v in case["parent"]])
    assert (status, metric, message) == ex.verdict(state, case["child_column"], case["parent_column"], case["allow_nulls"])
    assert (status, metric) == (case["status"], case["metric"])
    assert all(part in message for part in case["message_parts"])
    if not case["allow_nulls"]:
        assert run_constraint(c, tables, builder=True) == (status, metric, message)


def test_the_big_table_through_the_suite(big):
    child, parents, want = big
    T.init()
    tables = {"orders": pa.table({"customer_id": child, "small": child.cast(pa.int32()),
                                  "f": pa.array(np.arange(N_BIG, dtype=np.float64))}),
              "customers": pa.table({"id": pa.array(parents[0], pa.int64()),
                                     "name": pa.array(["n"] * len(parents[0]), pa.string())}),
              "accounts": pa.table({"id": pa.array(parents[1], pa.int64())})}
    for allow in (False, True):
        c = S.ForeignKeyConstraint("orders.customer_id", "customers.id").allow_nulls(allow)
        assert run_constraint(c, tables) == ex.verdict(want[0], "orders.customer_id", "customers.id", allow)
    c = S.ForeignKeyConstraint("orders.customer_id", "accounts.id")  # the hash route
    assert run_constraint(c, tables) == ex.verdict(want[1], "orders.customer_id", "accounts.id")
    got = run_constraint(S.ForeignKeyConstraint("orders.small", "customers.id").max_violations_reported(3), tables)
    assert got == ex.verdict(want[0], "orders.small", "customers.id", max_violations_reported=3)
    got = run_constraint(S.ForeignKeyConstraint("orders.customer_id", "customers.id").max_violations_reported(0), tables)
    assert got == ex.verdict(want[0], "orders.customer_id", "customers.id", max_violations_reported=0) and "Examples" not in got[2]
    # a bound the missing keys overrun: the verdict and the metric stand, unique reads "at least"
    status, metric, message = run_constraint(S.ForeignKeyConstraint("orders.customer_id", "customers.id").max_missing_keys(16), tables)
    total = want[0]["missing_rows"] + want[0]["null_rows"]
    assert (status, metric) == ("failure", float(total)) and "unique: at least " in message and "Examples: [" in message
    # what is not on the GPU path, and what the reference's planner refuses
    for name, word in (("orders.f", "Float64"), ("customers.name", "Utf8")):
        pair = (name, "customers.id") if name.startswith("orders") else ("orders.customer_id", name)
        status, _, message = run_constraint(S.ForeignKeyConstraint(*pair), tables)
        assert status == "error" and word in message and "not on the GPU path" in message
    status, _, message = run_constraint(S.ForeignKeyConstraint("orders.customer_id", "nowhere.id"), tables)
    assert status == "error" and "Foreign key validation query failed: Error during planning: table 'datafusion.public.nowhere' not found" in message
    status, _, message = run_constraint(S.ForeignKeyConstraint("orders.customer_id", "customers.nothing"), tables)
    assert status == "error" and "Foreign key validation query failed: Schema error: No field named nothing." in message
    status, _, message = run_constraint(S.ForeignKeyConstraint("customer_id", "customers.id"), tables)
    assert status == "error" and "Foreign key column must be qualified (table.column): 'customer_id'" in message
