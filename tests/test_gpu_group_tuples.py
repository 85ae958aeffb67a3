"""GROUP BY several columns on the device -- TGX_CHECK_GROUP_COUNTS / TGX_CHECK_GROUP_SUMS specs with a column list -- held
against tests/exact_group_tuples.py: every entry (its encoded key, its counters), the entries' order and all ten
counters (or the four classes) equal the exact walk, and the identities are checked each time against a plain COUNT (and
SUM) of the value column.  Bounds are chosen so that the reference alone has no overflow (max_groups >= the distinct
tuples), except in the overflow tests."""
import ctypes
import math
import struct
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_group_sums as exs
import exact_group_tuples as ext
import term_amd as T
import test_gpu_group_sums as gs
from _lib_spec import spec
from test_gpu_group_counts import as_exact, column, cut, dictionary, feed, flags, identities, ints, on_device, padded, read

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2**63, 2**63 - 1
E = ext.encode


# ---- plans and references -------------------------------------------------------------------------------------------------
def counts_plan(arity, n_values, bounds=(10000, 256), extra=()):
    """columns 0 .. arity-1 are the group columns, the next n_values the value columns: a spec each, then a COUNT each"""
    cols = list(range(arity))
    plan = T.Plan([spec(T.GROUP_COUNTS, arity + m, columns=cols) for m in range(n_values)] +
                  [spec(T.COUNT, arity + m) for m in range(n_values)] + list(extra))
    for m in range(n_values):
        plan.set_group_counts(m, *bounds)
    return plan


def cells_of(arr):
    """an arrow array as the exact walk's cells: None, int or bytes (a dictionary array reads as its values)"""
    if pa.types.is_date32(arr.type):
        arr = arr.cast(pa.int32())
    return as_exact(arr.to_pylist())


def exact_counts(value, groups, max_value_bytes=256):
    return ext.walk([None if v is None else 1 for v in value.to_pylist()], [cells_of(g) for g in groups], max_value_bytes)


def check(values, groups, max_groups=10000, max_value_bytes=256, mem=T.MEM_DEVICE, cuts=None, want=None):
    """`values`: the value columns (arrow arrays) of one walk over the tuple of `groups` (arrow arrays)"""
    T.init()
    n, k = len(groups[0]), len(groups)
    plan = counts_plan(k, len(values), (max_groups, max_value_bytes))
    cols = [column(g, mem) for g in groups] + [column(v, mem) for v in values]
    st = feed(plan, cut(cols, n, cuts))
    res = st.finalize()
    wants = []
    for m, v in enumerate(values):
        w = want[m] if want is not None else exact_counts(v, groups, max_value_bytes)
        got = read(st, m)
        assert got == w and list(got["entries"]) == list(w["entries"])  # (the order too: ascending by encoded key)
        assert (got["null_group_rows"], got["null_group_non_null"]) == (0, 0)
        count = res[len(values) + m]
        assert count.total == n
        identities(got, count.non_null)
        r = res[m]
        assert (r.total, r.non_null, r.distinct, r.matches) == (n, count.non_null, w["groups"], w["counted"])
        wants.append(w)
    return st, plan, wants


def int_groups(rng, n, arity, nulls=0.2, keys=5):
    return [ints(rng.integers(-keys, keys, n) * (1 if c % 2 else 2**60 + 7), mask=rng.random(n) >= nulls) for c in range(arity)]


def mixed_groups(rng, n, arity, nulls=0.2):
    """integers, Utf8, a dictionary, LargeUtf8, Utf8View, Int32, ... in turn"""
    makers = [lambda: ints(rng.integers(-3, 3, n), mask=rng.random(n) >= nulls),
              lambda: pa.array([None if rng.random() < nulls else "s%d" % k for k in rng.integers(0, 4, n)], pa.string()),
              lambda: dictionary(rng.integers(0, 4, n), ["a", None, "", "a"], mask=rng.random(n) >= nulls),
              lambda: pa.array([None if rng.random() < nulls else "L" * k for k in rng.integers(0, 3, n)], pa.large_string()),
              lambda: pa.array([None if rng.random() < nulls else "view-%015d" % k if k % 2 else "v%d" % k
                                for k in rng.integers(0, 4, n)], pa.string_view()),
              lambda: ints(rng.integers(-2, 2, n), type=pa.int32(), mask=rng.random(n) >= nulls)]
    return [makers[c % len(makers)]() for c in range(arity)]


# ---- GROUP_COUNTS: rows, arities, NULLs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1023, 1024, 1025])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    check([flags(rng, n)], int_groups(rng, n, 2))
    check([flags(rng, n)], mixed_groups(rng, n, 2))


@pytest.mark.parametrize("arity", [2, 3, 8])
@pytest.mark.parametrize("numeric", [True, False], ids=["integers", "mixed"])
def test_arities(arity, numeric):
    rng = np.random.default_rng(arity)
    n = 3000
    groups = int_groups(rng, n, arity, keys=2) if numeric else mixed_groups(rng, n, arity)
    _, _, want = check([flags(rng, n), flags(rng, n, 0.0)], groups)
    assert want[0]["groups"] >= 25  # (arity 2 over four values and NULL a column)


@pytest.mark.parametrize("rate", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("position", [0, 1, 2])
def test_a_null_in_every_position(position, rate):
    rng = np.random.default_rng(int(position * 10 + rate * 100))
    n = 3000
    groups = mixed_groups(rng, n, 3, nulls=0.0)
    src = groups[position]
    mask = rng.random(n) >= rate
    groups[position] = pa.array([v if ok else None for v, ok in zip(src.to_pylist(), mask)], type=src.type) \
        if not pa.types.is_dictionary(src.type) else dictionary(src.indices.to_numpy(), ["a", "b", "", "c"], mask=mask)
    _, _, want = check([flags(rng, n, 0.5)], groups)
    with_null = sum(t for k, (t, _) in want[0]["entries"].items() if ext.decode(k)[position] is None)
    assert with_null == int((~mask).sum())


def test_null_and_the_empty_string_are_three_groups():
    a = pa.array([None, "", None, None, ""], pa.string())
    b = pa.array(["a", "a", None, "a", "a"], pa.string())
    _, _, want = check([ints([1, None, 3, 4, 5])], [a, b])
    assert want[0]["entries"] == {E((None, None)): (1, 1), E((None, b"a")): (2, 2), E((b"", b"a")): (2, 1)}


def test_a_constant_tuple_and_64_distinct_tuples_in_a_wave():
    rng = np.random.default_rng(1)
    n = 20_000
    check([flags(rng, n), flags(rng, n, 0.0)], [ints(np.full(n, 42)), ints(np.full(n, -1))])
    check([flags(rng, n)], [ints(np.full(n, 42), mask=np.arange(n) % 3 != 0), pa.array(["k"] * n, pa.string())])
    check([flags(rng, n)], [ints(np.arange(n) % 8), ints(np.arange(n) // 8 % 8 * 1_000_003)])


def test_more_tuples_than_a_workgroups_lds_table_holds():
    """3000 distinct tuples in 20 000 rows: more than the 1024 LDS slots, so rows go to the global table directly"""
    rng = np.random.default_rng(3)
    n = 20_000
    a, b = rng.integers(0, 60, n), rng.integers(0, 50, n) * 1_000_003 - 5
    ma = rng.random(n) >= 0.02
    valid = rng.random(n) >= 0.4
    want = ext.walk_np(valid, [a, b], [ma, None])
    assert want["groups"] > 2 * 1024
    check([ints(np.arange(n), mask=valid)], [ints(a, mask=ma), ints(b)], want=[want])
    s = pa.array(["t%d" % k for k in b], pa.string())
    check([ints(np.arange(n), mask=valid)], [ints(a, mask=ma), s])


@pytest.mark.parametrize("extra", [0, 1])
def test_all_rows_distinct_at_max_groups_and_one_above(extra):
    rng = np.random.default_rng(4)
    n = 1000 + extra
    p = rng.permutation(n)
    _, _, want = check([flags(rng, n)], [ints(p % 37), ints(p // 37 * 7 - 3000)], max_groups=1000)
    assert want[0]["groups"] == n and want[0]["overflow_rows"] == 0  # one above: reported, the caller compares


def test_more_tuples_than_the_global_table_has_slots():
    rng = np.random.default_rng(5)
    n = 30_000
    a, b, valid = rng.integers(0, 70, n), rng.integers(0, 70, n), rng.random(n) >= 0.5
    T.init()
    plan = counts_plan(2, 1, (4, 256))  # 8 slots
    st = feed(plan, [[column(ints(a)), column(ints(b)), column(ints(np.arange(n), mask=valid))]])
    got, true = read(st), ext.walk_np(valid, [a, b])
    assert got["overflow_rows"] > 0 and 0 < got["overflow_non_null"] < got["overflow_rows"] and got["groups"] <= 8
    identities(got, int(valid.sum()))
    assert st.finalize()[1].non_null == int(valid.sum())
    # only keys of the table are held, and none is counted too often
    assert all(0 < t <= true["entries"][k][0] and nn <= true["entries"][k][1] for k, (t, nn) in got["entries"].items())


@pytest.mark.parametrize("numeric", [True, False], ids=["integers", "mixed"])
def test_an_encoded_length_of_exactly_max_value_bytes_and_one_above(numeric):
    rng = np.random.default_rng(6)
    n = 2000
    if numeric:  # (int, int) is 18 bytes, (int, NULL) 10
        groups = [ints(rng.integers(0, 5, n)), ints(rng.integers(0, 5, n), mask=rng.random(n) >= 0.3)]
        at, short = 18, 10
    else:  # (int, string of k bytes) is 12 + k
        groups = [ints(rng.integers(0, 3, n)), pa.array(["x" * k for k in rng.integers(19, 23, n)], pa.string())]
        at, short = 12 + 21, 12 + 19
    v = flags(rng, n, 0.5)
    _, _, want = check([v], groups, max_value_bytes=at)
    assert (want[0]["long_rows"] == 0) == numeric and max(map(len, want[0]["entries"])) == at
    _, _, above = check([v], groups, max_value_bytes=at - 1)
    assert above[0]["long_rows"] > above[0]["long_non_null"] > 0 and max(map(len, above[0]["entries"])) < at
    assert min(map(len, above[0]["entries"])) == short


# ---- component types ----------------------------------------------------------------------------------------------------------
NARROW = [(pa.int8(), [-128, -1, 0, 127, 5]), (pa.int16(), [-32768, -1, 32767, 5]), (pa.int32(), [-2**31, -1, 2**31 - 1, 5]),
          (pa.uint8(), [0, 255, 128, 5]), (pa.uint16(), [0, 65535, 32768, 5]), (pa.uint32(), [0, 2**31, 2**32 - 1, 5]),
          (pa.date32(), [-1, 0, 19000, 5])]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("type,values", NARROW, ids=[str(t) for t, _ in NARROW])
def test_narrow_types_are_widened(type, values, mem):
    rng = np.random.default_rng(7)
    n = 700
    picks = [None if rng.random() < 0.1 else values[i] for i in rng.integers(0, len(values), n)]
    arr = pa.array(picks, type=pa.int32() if type == pa.date32() else type)
    arr = arr.cast(type) if type == pa.date32() else arr
    wide = ints(rng.integers(4, 7, n))
    _, _, want = check([flags(rng, n)], [arr, wide], mem=mem)
    assert E((5, 5)) in want[0]["entries"]  # a narrow 5 and a wide 5 have the same bytes


STRING_TYPES = [pa.string(), pa.large_string(), pa.string_view()]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("type", STRING_TYPES, ids=str)
def test_string_layouts(type, mem):
    rng = np.random.default_rng(8)
    n = 4000
    words = ["x" * k for k in (0, 1, 12, 13, 16, 17, 33)] + ["Zoë", "a\x00b"]
    s = pa.array([None if rng.random() < 0.1 else words[i] for i in rng.integers(0, len(words), n)], type=type)
    g = ints(rng.integers(0, 3, n), mask=rng.random(n) >= 0.1)
    check([flags(rng, n, 0.5)], [s, g], mem=mem)
    check([flags(rng, n + 3, 0.5).slice(0, n - 3)], [g.slice(3), s.slice(3)], max_value_bytes=40, mem=mem)


def test_a_view_column_with_two_data_buffers():
    rng = np.random.default_rng(9)
    words = ["x" * k for k in (0, 5, 12, 13, 20, 31)]
    vals = [words[i] for i in rng.integers(0, len(words), 2000)]
    bufs, views = [bytearray(), bytearray()], bytearray()
    for k, s in enumerate(vals):
        b = s.encode()
        if len(b) <= 12:
            views += struct.pack("<i12s", len(b), b)
        else:
            which = k % 2
            views += struct.pack("<i4sii", len(b), b[:4], which, len(bufs[which]))
            bufs[which] += b
    T.init()
    col = T.Column.utf8_view(padded(np.frombuffer(bytes(views), np.uint8)),
                             [padded(np.frombuffer(bytes(b), np.uint8)) for b in bufs])
    g = ints(rng.integers(0, 3, len(vals)))
    v = flags(rng, len(vals))
    st = feed(counts_plan(2, 1), [[column(g), col.sliced(0, len(vals)), column(v)]])
    assert read(st) == ext.walk(v.to_pylist(), [cells_of(g), as_exact(vals)])


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
def test_a_dictionary_with_null_unused_and_repeated_entries(mem):
    rng = np.random.default_rng(10)
    n = 4000
    entries = ["a", None, "b", "a", "unused", "", "b"]  # 0 and 3, 2 and 6 repeat a value; 1 is NULL
    d = dictionary(rng.choice([0, 1, 2, 3, 5, 6], n), entries, mask=rng.random(n) >= 0.1)
    _, _, want = check([flags(rng, n, 0.5)], [d, ints(rng.integers(0, 2, n))], mem=mem)
    firsts = {ext.decode(k)[0] for k in want[0]["entries"]}
    assert firsts == {None, b"a", b"b", b""}


def test_an_index_outside_the_dictionary_is_a_null_component():
    rng = np.random.default_rng(11)
    n = 1000
    idx = rng.integers(-1, 4, n).astype(np.int32)  # -1 and 3 lie outside a dictionary of three entries
    v = flags(rng, n)
    g = ints(rng.integers(0, 2, n))
    T.init()
    d = on_device(T.Column.dict32_utf8(idx, T.Column.from_arrow(pa.array(["p", "q", "r"], pa.string()))))
    st = feed(counts_plan(2, 1), [[column(g), d, column(v)]])
    keys = [None if i in (-1, 3) else [b"p", b"q", b"r"][i] for i in idx]
    got = read(st)
    assert got == ext.walk(v.to_pylist(), [cells_of(g), keys])
    assert sum(t for k, (t, _) in got["entries"].items() if ext.decode(k)[1] is None) == int(((idx == -1) | (idx == 3)).sum())
    identities(got, n - v.null_count)


OFFSETS = [0, 1, 9, 63, 64]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("off", OFFSETS)
def test_every_component_and_value_column_has_its_own_arrow_offset(off, mem):
    rng = np.random.default_rng(off)
    n, room = 3000, 70
    a = ints(rng.integers(0, 5, n + room), mask=rng.random(n + room) >= 0.3).slice(off, n)
    b = pa.array(["k%d" % k if k else None for k in rng.integers(0, 5, n + room)], pa.string()).slice((off + 7) % 65, n)
    c = dictionary(rng.integers(0, 3, n + room), ["u", "v", None], mask=rng.random(n + room) >= 0.2).slice((off + 13) % 65, n)
    v1 = flags(rng, n + room, 0.5).slice((off + 9) % 65, n)
    v2 = flags(rng, n + room, 0.2).slice((off + 31) % 65, n)
    check([v1, v2], [a, b, c], mem=mem)


# ---- walks ----------------------------------------------------------------------------------------------------------------------
def launches_of(plan, cols, name="group_counts_tuples"):
    st = T.State(plan)
    st.profile_enable(True)
    st.update(cols)
    st.finalize()
    return st, st.profile_get(name)["launches"]


@pytest.mark.parametrize("n_values,walks", [(1, 1), (8, 1), (9, 2)])
def test_value_columns_share_one_walk_of_the_list(n_values, walks):
    rng = np.random.default_rng(20 + n_values)
    n = 20_000
    groups = [ints(rng.integers(0, 30, n) * 77, mask=rng.random(n) >= 0.1), ints(rng.integers(0, 10, n))]
    values = [flags(rng, n + 70, m / 8).slice(m * 7 + 1, n) for m in range(n_values)]  # every member its own offset
    T.init()
    cols = [column(g) for g in groups] + [column(v) for v in values]
    st, launches = launches_of(counts_plan(2, n_values), cols)
    assert launches == walks  # one launch a walk, not one a spec
    res = st.finalize()
    for m, v in enumerate(values):
        got = read(st, m)
        assert got == exact_counts(v, groups)
        identities(got, res[n_values + m].non_null)


def test_lists_in_another_order_or_with_other_bounds_walk_apart_and_the_value_column_may_be_a_group_column():
    rng = np.random.default_rng(22)
    n = 5000
    a, b = ints(rng.integers(0, 9, n), mask=rng.random(n) >= 0.2), ints(rng.integers(0, 4, n), mask=rng.random(n) >= 0.2)
    T.init()
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, columns=[0, 1]), spec(T.GROUP_COUNTS, 1, columns=[0, 1]),
                   spec(T.GROUP_COUNTS, 0, columns=[1, 0]), spec(T.GROUP_COUNTS, 0, columns=[0, 1]),
                   spec(T.GROUP_COUNTS, 0, column2=1), spec(T.COUNT, 0), spec(T.COUNT, 1)])
    for i in range(5):
        plan.set_group_counts(i, 10000, 256 if i != 3 else 255)
    st, launches = launches_of(plan, [column(a), column(b)])
    assert launches == 3 and st.profile_get("group_counts")["launches"] == 1
    res = st.finalize()
    assert read(st, 0) == read(st, 3) == exact_counts(a, [a, b])
    assert read(st, 1) == exact_counts(b, [a, b]) and read(st, 2) == exact_counts(a, [b, a])
    got = read(st, 0)  # the value column is the first group column: a group's non-NULL count is 0 or its rows
    assert all(nn == (0 if ext.decode(k)[0] is None else t) for k, (t, nn) in got["entries"].items())
    identities(got, res[5].non_null)
    identities(read(st, 1), res[6].non_null)


# ---- batching and the ways a state travels ------------------------------------------------------------------------------------
N_BIG = 200_000


@pytest.fixture(scope="module")
def big():
    """an (Int64, Int32) list, a (Utf8, Dictionary, Int32) list, two value columns"""
    rng = np.random.default_rng(30)
    i0 = ints(rng.zipf(1.3, N_BIG) % 300 - 100, mask=rng.random(N_BIG) >= 0.05)
    i1 = ints(rng.integers(-3, 3, N_BIG), type=pa.int32(), mask=rng.random(N_BIG) >= 0.05)
    s0 = pa.array(["c%d" % k if k % 7 else None for k in rng.integers(0, 40, N_BIG)], pa.string())
    d0 = dictionary(rng.integers(0, 10, N_BIG), ["d%d" % (k % 8) for k in range(10)], mask=rng.random(N_BIG) >= 0.02)
    va, vb = gs.amounts(rng, N_BIG, 0.3), flags(rng, N_BIG, 0.9)
    arrs = [i0, i1, s0, d0, va, vb]
    lists = ([i0, i1], [s0, d0, i1])
    counts = [exact_counts(v, g) for g in lists for v in (va, vb)]
    sums = [ext.walk_sums(va.to_pylist(), [cells_of(c) for c in g]) for g in lists]
    return arrs, counts, sums


LISTS = ([0, 1], [2, 3, 1])


def big_plan(extra=()):
    plan = T.Plan([spec(T.GROUP_COUNTS, v, columns=g) for g in LISTS for v in (4, 5)] +
                  [spec(T.GROUP_SUMS, 4, columns=g) for g in LISTS] + list(extra))
    for i in range(4):
        plan.set_group_counts(i)
    for i in (4, 5):
        plan.set_group_sums(i)
    return plan


def read_all(st):
    return [read(st, i) for i in range(4)], [gs.read(st, i) for i in (4, 5)]


def same_as(st, counts, sums):
    got_counts, got_sums = read_all(st)
    assert got_counts == counts
    assert got_sums == sums
    for got, want in zip(got_counts + got_sums, counts + sums):
        assert list(got["entries"]) == list(want["entries"])


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192), (T.MEM_HOST, [3, 8195, 8196, 100_001])])
def test_batching_independence(big, mem, cuts):
    arrs, counts, sums = big
    T.init()
    st = feed(big_plan(), cut([column(a, mem) for a in arrs], N_BIG, cuts))
    same_as(st, counts, sums)


def test_state_algebra(big):
    arrs, counts, sums = big
    T.init()
    cols = [column(a) for a in arrs]
    parts = cut(cols, N_BIG, [70_000, 140_001])
    plan = big_plan()
    # read half-way, then on
    st = feed(plan, parts[:1])
    head = [a.slice(0, 70_000) for a in arrs]
    assert read(st, 0) == exact_counts(head[4], head[:2])
    st.update(parts[1])
    st.update(parts[2])
    same_as(st, counts, sums)
    # reset and refill
    st.reset()
    assert read(st)["seen"] == 0 and read(st)["entries"] == {} and gs.read(st, 4)["entries"] == {}
    st.update(cols)
    same_as(st, counts, sums)
    # merge of three states
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    same_as(states[0], counts, sums)
    # a blob round trip into a fresh state; equal states give equal bytes
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    same_as(back, counts, sums)
    assert back.serialize() == blob == st.serialize()
    back.merge([st])
    assert read(back, 2)["entries"] == {k: (2 * t, 2 * n) for k, (t, n) in counts[2]["entries"].items()}
    other = T.Plan([spec(T.GROUP_COUNTS, v, columns=g) for g in ([0, 1], [2, 3]) for v in (4, 5)] +
                   [spec(T.GROUP_SUMS, 4, columns=g) for g in LISTS])
    for i in range(4):
        other.set_group_counts(i)
    for i in (4, 5):
        other.set_group_sums(i)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*the blob groups by 3 columns, the plan's task by 2"):
        T.State.deserialize(other, blob)


def test_an_int32_state_and_an_int64_state_of_the_same_values_merge_to_one_entry_a_key():
    rng = np.random.default_rng(31)
    n = 3000
    a, b = rng.integers(-4, 4, n), rng.integers(-2**31, -2**31 + 3, n)
    mask = rng.random(n) >= 0.2
    v = flags(rng, n)
    T.init()
    plan = counts_plan(2, 1)
    narrow = feed(plan, [[column(ints(a, type=pa.int8(), mask=mask)), column(ints(b, type=pa.int32())), column(v)]])
    wide = feed(plan, [[column(ints(a, mask=mask)), column(ints(b)), column(v)]])
    want = exact_counts(v, [ints(a, mask=mask), ints(b)])
    assert read(narrow) == read(wide) == want
    narrow.merge([wide])
    assert read(narrow)["entries"] == {k: (2 * t, 2 * nn) for k, (t, nn) in want["entries"].items()}


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(big, world, device_buffers):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's entries"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    arrs, counts, sums = big
    T.init()
    whole = [column(a) for a in arrs]
    plan = big_plan(extra=[spec(T.COUNT, 4)])
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(N_BIG, world, rank)
            st = T.State(plan)
            comm = thread_comm(group, rank, device_buffers=device_buffers)
            for _ in range(2):
                res = sharded_suite_step(plan, st, [c.sliced(lo, hi - lo) for c in whole], comm)
            results[rank] = (res, read_all(st))
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
    for res, (got_counts, got_sums) in results:
        assert got_counts == counts and got_sums == sums
        assert res[6].total == N_BIG and res[0].non_null == res[6].non_null


# ---- isolation ------------------------------------------------------------------------------------------------------------------
def test_refused_group_types_leave_the_state_usable():
    T.init()
    n = 1000
    plan = T.Plan([spec(T.GROUP_COUNTS, 2, columns=[0, 1]), spec(T.GROUP_SUMS, 2, columns=[0, 1]), spec(T.COUNT, 2)])
    plan.set_group_counts(0)
    plan.set_group_sums(1)
    st = T.State(plan)
    v = ints(np.arange(n), mask=np.arange(n) % 4 != 0)
    g = ints(np.arange(n) % 10)
    bad = [(pa.array(np.arange(n, dtype=np.float64)), "Float64"), (pa.array(np.arange(n, dtype=np.float32)), "Float32"),
           (pa.array(np.arange(n, dtype=np.uint64)), "UInt64"), (pa.array(np.arange(n) % 2 == 0), "Boolean")]
    for mem in (T.MEM_HOST, T.MEM_DEVICE):
        for arr, name in bad:
            for cols in ([arr, g], [g, arr]):  # in either position
                with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*GROUP_(COUNTS|SUMS) groups by.*" + name):
                    st.update([column(cols[0], mem), column(cols[1], mem), column(v, mem)])
        nested = T.Column.validity_only(pa.array([[1]] * n, pa.list_(pa.int64())))
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*validity-only"):
            st.update([column(g, mem), column(nested, mem), column(v, mem)])
    assert read(st)["seen"] == 0 and gs.read(st, 1)["seen"] == 0
    st.update([column(g), column(g), column(v)])
    assert read(st) == exact_counts(v, [g, g]) and gs.read(st, 1) == ext.walk_sums(v.to_pylist(), [cells_of(g)] * 2)
    identities(read(st), 750)


def test_a_plan_without_tuple_tasks_profiles_no_tuples_kernel(big):
    arrs, _, _ = big
    T.init()
    cols = [column(arrs[0]), column(arrs[1]), column(arrs[4])]
    single = T.Plan([spec(T.GROUP_COUNTS, 2, column2=0), spec(T.GROUP_SUMS, 2, column2=1), spec(T.COUNT, 0)])
    single.set_group_counts(0)
    single.set_group_sums(1)
    st = T.State(single)
    st.profile_enable(True)
    st.update(cols)
    st.finalize()
    launches = {name: st.profile_get(name)["launches"] for name in
                ("group_counts", "group_counts_tuples", "group_sums", "group_sums_tuples")}
    assert launches == {"group_counts": 1, "group_counts_tuples": 0, "group_sums": 1, "group_sums_tuples": 0}
    tuples = T.Plan([spec(T.GROUP_COUNTS, 2, columns=[0, 1]), spec(T.GROUP_SUMS, 2, columns=[0, 1])])
    tuples.set_group_counts(0)
    tuples.set_group_sums(1)
    st = T.State(tuples)
    st.profile_enable(True)
    st.update(cols)
    st.finalize()
    launches = {name: st.profile_get(name)["launches"] for name in
                ("group_counts", "group_counts_tuples", "group_sums", "group_sums_tuples")}
    assert launches == {"group_counts": 0, "group_counts_tuples": 1, "group_sums": 0, "group_sums_tuples": 1}


def test_the_tuple_specs_leave_the_other_kinds_bit_for_bit(big):
    arrs, counts, sums = big
    T.init()
    cols = [column(a) for a in arrs]
    others = [spec(T.COUNT, 0), spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.DISTINCT, 0, columns=[0, 4]),
              spec(T.COUNT, 2), spec(T.DISTINCT, 2), spec(T.REGEX_MATCH, 2, pattern=r"^c1\d*$"), spec(T.DISTINCT, 3),
              spec(T.COUNT, 4), spec(T.NUMERIC_STATS, 4), spec(T.GROUP_COUNTS, 4, column2=0), spec(T.GROUP_SUMS, 4, column2=2)]

    def with_bounds(plan, at):
        plan.set_group_counts(at)
        plan.set_group_sums(at + 1)
        return plan
    alone_st = feed(with_bounds(T.Plan(others), 9), [cols])
    alone = alone_st.finalize()
    st = feed(with_bounds(big_plan(extra=others), 15), [cols])
    res = st.finalize()
    same_as(st, counts, sums)
    for got, ref in zip(res[6:], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))
    assert st.group_counts(15) == alone_st.group_counts(9) and st.group_sums(16) == alone_st.group_sums(10)


# ---- GROUP_SUMS -------------------------------------------------------------------------------------------------------------------
def sums_plan(arity, bounds=(10000, 256)):
    """columns 0 .. arity-1 the group columns, column `arity` the value column: the spec, a COUNT, the plain SUM"""
    plan = T.Plan([spec(T.GROUP_SUMS, arity, columns=list(range(arity))), spec(T.COUNT, arity), spec(T.NUMERIC_STATS, arity)])
    plan.set_group_sums(0, *bounds)
    return plan


def check_sums(values, groups, is_float=False, exactly=True, max_groups=10000, max_value_bytes=256, mem=T.MEM_DEVICE,
               cuts=None, want=None):
    T.init()
    n, k = len(values), len(groups)
    plan = sums_plan(k, (max_groups, max_value_bytes))
    st = feed(plan, cut([column(g, mem) for g in groups] + [column(values, mem)], n, cuts))
    res = st.finalize()
    if want is None:
        want = ext.walk_sums(values.to_pylist(), [cells_of(g) for g in groups], max_value_bytes, is_float)
    got = gs.read(st)
    assert res[1].total == n and got["null_group"][:2] == (0, 0)
    r = res[0]
    assert (r.total, r.non_null, r.distinct, r.matches, r.has_value) == (n, res[1].non_null, want["groups"],
                                                                       want["counted"][0], int(res[1].non_null > 0))
    if is_float:
        gs.compare_float(got, want, exactly)
        gs.identities(got, res[1].non_null)
        assert r.sum_i == 0
    else:
        assert got == want and list(got["entries"]) == list(want["entries"])
        gs.identities(got, res[1].non_null, res[2].sum_i)
        assert (r.sum_i, r.sum_f) == (res[2].sum_i, float(res[2].sum_i))
    return st, plan, want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1023, 1024, 1025])
def test_sums_row_counts(n):
    rng = np.random.default_rng(100 + n)
    check_sums(gs.amounts(rng, n), int_groups(rng, n, 2))
    check_sums(gs.floats(rng.integers(-50, 50, n), mask=rng.random(n) >= 0.3), mixed_groups(rng, n, 2), is_float=True)


@pytest.mark.parametrize("arity", [2, 8])
@pytest.mark.parametrize("numeric", [True, False], ids=["integers", "mixed"])
def test_sums_arities_with_integer_sums_that_wrap(arity, numeric):
    rng = np.random.default_rng(110 + arity)
    n = 3000
    groups = int_groups(rng, n, arity, keys=2) if numeric else mixed_groups(rng, n, arity)
    v = ints(rng.choice(np.array([I64_MAX, I64_MIN, -1, 1, 2**62], np.int64), n), mask=rng.random(n) >= 0.3)
    _, _, want = check_sums(v, groups)
    assert any(abs(e[2]) > 2**62 for e in want["entries"].values())


def test_sums_more_tuples_than_the_lds_table_and_the_global_table():
    rng = np.random.default_rng(120)
    n = 20_000
    a, b = rng.integers(0, 60, n), rng.integers(0, 50, n) * 1_000_003 - 5
    valid = rng.random(n) >= 0.4
    vals = rng.integers(-1000, 1000, n)
    want = ext.walk_sums_np(vals, valid, [a, b])
    assert want["groups"] > 2 * 1024
    check_sums(ints(vals, mask=valid), [ints(a), ints(b)], want=want)
    T.init()
    st = feed(sums_plan(2, (4, 256)), [[column(ints(a)), column(ints(b)), column(ints(vals, mask=valid))]])  # 8 slots
    got = gs.read(st)
    assert got["overflow"][0] > got["overflow"][1] > 0 and got["groups"] <= 8
    gs.identities(got, int(valid.sum()), exs.wrap(int(vals[valid].sum())))
    assert all(e[0] <= want["entries"][k][0] for k, e in got["entries"].items())


def test_sums_long_rows_and_every_row_distinct_one_above_max_groups():
    rng = np.random.default_rng(121)
    n = 1001
    p = rng.permutation(n)
    _, _, want = check_sums(gs.amounts(rng, n), [ints(p % 37), ints(p // 37)], max_groups=1000)
    assert want["groups"] == n
    groups = [ints(rng.integers(0, 3, n)), pa.array(["x" * k for k in rng.integers(19, 23, n)], pa.string())]
    _, _, want = check_sums(gs.amounts(rng, n), groups, max_value_bytes=12 + 20)
    assert want["long_rows"][0] > want["long_rows"][1] > 0 and want["long_rows"][2] != 0


def test_float_sums_of_small_integers_are_exact_and_general_ones_lie_within_the_any_order_bound():
    rng = np.random.default_rng(122)
    n = 20_000
    groups = [ints(rng.integers(0, 5, n), mask=rng.random(n) >= 0.1), pa.array(["g%d" % k for k in rng.integers(0, 4, n)])]
    check_sums(gs.floats(rng.integers(-1000, 1000, n), mask=rng.random(n) >= 0.3), groups, is_float=True)
    check_sums(gs.floats(rng.standard_normal(n) * 1e6, mask=rng.random(n) >= 0.3), groups, is_float=True, exactly=False)


def test_nan_and_infinities_propagate():
    g0 = ints([1, 1, 2, 2, 3, 3, 4, 4, None, None])
    g1 = ints([7, 7, 7, 7, None, None, 7, 7, None, None])
    v = gs.floats([math.nan, 1.0, math.inf, 5.0, math.inf, -math.inf, -math.inf, -2.0, 1.5, 0.0],
                  mask=np.arange(10) < 9)
    st, _, want = check_sums(v, [g0, g1], is_float=True)
    e = gs.read(st)["entries"]
    assert e[E((1, 7))][2] != e[E((1, 7))][2] and e[E((2, 7))][2] == math.inf and e[E((3, None))][2] != e[E((3, None))][2]
    assert e[E((4, 7))][2] == -math.inf and e[E((None, None))] == (2, 1, 1.5)


def test_sums_the_value_column_is_one_of_the_group_columns_and_narrow_values():
    rng = np.random.default_rng(123)
    n = 3000
    a = ints(rng.integers(-5, 5, n), type=pa.int16(), mask=rng.random(n) >= 0.2)
    b = ints(rng.integers(0, 3, n))
    T.init()
    plan = T.Plan([spec(T.GROUP_SUMS, 0, columns=[0, 1]), spec(T.COUNT, 0)])
    plan.set_group_sums(0)
    for mem in (T.MEM_DEVICE, T.MEM_HOST):
        st = feed(plan, [[column(a, mem), column(b, mem)]])
        got = gs.read(st)
        assert got == ext.walk_sums(a.to_pylist(), [cells_of(a), cells_of(b)])
        assert all(e[2] == (0 if ext.decode(k)[0] is None else ext.decode(k)[0] * e[0]) for k, e in got["entries"].items())


# ---- end to end: the analyzer through AnalysisRunner, the constraint through ValidationSuite.run(.., tables=..) ----------------
import json  # noqa: E402
import os  # noqa: E402

import exact_group_counts as exc  # noqa: E402
import term_amd.suite as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARROW = {"int64": pa.int64(), "int32": pa.int32(), "float64": pa.float64(), "string": pa.string()}


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def metric_values(ctx, key):
    m = ctx.get_metric(key)
    assert m["type"] == "Map"
    return {k: v["value"] for k, v in m["value"].items()}


def exact_metric(values, groups, by, **kw):
    valid = [None if v is None else 1 for v in values.to_pylist()]
    return exc.metric_map(exc.grouped_state(exc.group_by(valid, *[cells_of(g) for g in groups]), list(by), **kw))


def composite(by, **kw):
    return S.GroupingConfig(list(by), composite_groups_on_device=True, **kw)


def test_the_reference_table_through_the_runner():
    g = golden("grouped_completeness_tuple_vectors.json")
    T.init()
    t = g["table"]
    table = pa.table({"region": pa.array(t["region"], pa.string()), "product": pa.array(t["product"], pa.string()),
                      "sales": pa.array(t["sales"], pa.int32())})
    runner = S.AnalysisRunner()
    runner.add(S.CompletenessAnalyzer("sales").with_grouping(composite(g["group_by"])))
    runner.add(S.CompletenessAnalyzer("sales").with_grouping(S.GroupingConfig(g["group_by"])))  # without the opt-in
    runner.add(S.CompletenessAnalyzer("sales").with_grouping(S.GroupingConfig(["region"])))
    ctx = runner.run(table)
    got = metric_values(ctx, g["metric_key"])
    assert {k: v for k, v in got.items() if k != "__metadata__"} == g["metrics"]
    assert got["US_A"] == 1.0 and got["EU_A"] == 0.5 and len(ctx.states[g["metric_key"]]["groups"]) == 4
    state = ctx.states[g["metric_key"]]
    assert state["groups"] == [{k: e[k] for k in ("key", "total_count", "non_null_count")} for e in g["groups"]]
    assert state["overall"] == g["overall"] and state["metadata"] == g["metadata"] and state["null_group"] is None
    assert metric_values(ctx, "completeness.sales_grouped_by_region")["EU"] == 2 / 3
    assert [e["analyzer_name"] for e in ctx.errors()] == ["completeness"]
    assert "groups by exactly one column on the GPU path (2 given)" in ctx.errors()[0]["error"]


def test_a_big_table_through_the_runner(big):
    arrs, counts, _ = big
    T.init()
    table = pa.table({"i0": arrs[0], "i1": arrs[1], "s0": arrs[2], "d0": arrs[3], "va": arrs[4], "vb": arrs[5],
                      "f": pa.array(np.arange(N_BIG, dtype=np.float64))})
    loose = dict(strict_reference_types=False)
    runner = S.AnalysisRunner()
    runner.add(S.CompletenessAnalyzer("va").with_grouping(composite(["i0", "i1"], **loose)))
    runner.add(S.CompletenessAnalyzer("vb").with_grouping(composite(["d0", "i1"], max_groups=40, **loose)))  # 128 slots hold the 63
    runner.add(S.CompletenessAnalyzer("va").with_grouping(composite(["s0", "i0"])))            # strict: i0 is Int64
    runner.add(S.CompletenessAnalyzer("va").with_grouping(composite(["s0", "f"], **loose)))    # floats: the device refuses
    runner.add(S.CompletenessAnalyzer("vb").with_grouping(composite(["i0", "i1"], max_groups=16, **loose)))  # overflows
    ctx = runner.run(table)
    got = metric_values(ctx, "completeness.va_grouped_by_i0_i1")
    assert got == exact_metric(arrs[4], arrs[:2], ["i0", "i1"])
    state = ctx.states["completeness.va_grouped_by_i0_i1"]
    assert len(state["groups"]) == counts[0]["groups"] and state["null_group"] is None
    cut = exc.grouped_state(exc.group_by([None if v is None else 1 for v in arrs[5].to_pylist()],
                                         *[cells_of(arrs[c]) for c in (3, 1)]), ["d0", "i1"], max_groups=40)
    state = ctx.states["completeness.vb_grouped_by_d0_i1"]
    assert state["metadata"] == cut["metadata"] and cut["metadata"]["total_groups"] == 41
    assert (state["overall"]["total_count"], state["overall"]["non_null_count"]) == cut["overall"]
    assert metric_values(ctx, "completeness.vb_grouped_by_d0_i1") == exc.metric_map(cut)
    errors = [e["error"] for e in ctx.errors()]
    assert len(errors) == 3
    assert "group column 'i0' is Int64" in errors[0] and "GROUP_COUNTS groups by integer and string columns" in errors[1]
    assert "columns [i0, i1] have more groups" in errors[2] and " 0 overflow rows" not in errors[2]


def arrow_table(side):
    return pa.table({name: pa.array(values, ARROW[kind]) for name, (kind, values) in side["columns"].items()})


@pytest.mark.parametrize("case", golden("cross_table_sum_tuple_vectors.json")["cases"], ids=lambda c: c["name"])
def test_the_golden_tables_through_the_suite(case):
    T.init()
    left, right = case["left"], case["right"]
    c = S.CrossTableSumConstraint("%s.%s" % (left["table"], left["column"]), "%s.%s" % (right["table"], right["column"])) \
        .group_by(case["group_by"]).tolerance(case["tolerance"]).composite_groups_on_device()
    got = gs.run_constraint(c, {left["table"]: arrow_table(left), right["table"]: arrow_table(right)})
    want = case["expect"]
    assert got == (want["status"], want["max_difference"], want["message"])
    plain = S.CrossTableSumConstraint("%s.%s" % (left["table"], left["column"]), "%s.%s" % (right["table"], right["column"])) \
        .group_by(case["group_by"])
    status, _, message = gs.run_constraint(plain, {left["table"]: arrow_table(left), right["table"]: arrow_table(right)})
    assert "GROUP BY over 2 columns is not on the GPU path" in message


def test_two_big_tables_through_the_suite():
    """200 000 rows a side, grouped by (Int64, Utf8): integer sums, so the verdict is exact"""
    rng = np.random.default_rng(40)
    n = 200_000

    def side(seed_shift):
        a = rng.integers(0, 300, n)
        b = rng.integers(0, 20, n)
        v = rng.integers(-1000, 1000, n)
        return (pa.table({"a": ints(a, mask=rng.random(n) >= 0.01), "b": pa.array(["k%d" % k if k else None for k in b], pa.string()),
                          "v": ints(v, mask=rng.random(n) >= 0.2)}))
    orders, payments = side(0), side(1)
    T.init()
    c = S.CrossTableSumConstraint("orders.v", "payments.v").group_by(["a", "b"]).composite_groups_on_device()
    status, metric, message = gs.run_constraint(c, {"orders": orders, "payments": payments})

    def sums(t):
        keys = list(zip(cells_of(t["a"].combine_chunks()), cells_of(t["b"].combine_chunks())))
        return exs.side_sums(t["v"].to_pylist(), keys, False)
    left, right = sums(orders), sums(payments)
    joinable = sorted(set(k for k in list(left) + list(right) if None not in k), key=E)
    rows = [(left.get(k, 0.0), right.get(k, 0.0)) for k in joinable]
    rows += [(left[k], 0.0) for k in sorted(left, key=E) if None in k] + [(0.0, right[k]) for k in sorted(right, key=E) if None in k]
    violating = sum(abs(l - r) > 0 for l, r in rows)
    tl = tr = 0.0
    for l, r in rows:
        tl += l
        tr += r
    worst = max(abs(l - r) for l, r in rows)
    assert status == "failure" and metric == worst
    assert message == ("Cross-table sum mismatch: %d/%d groups by [a, b] failed validation (exact match required), total sums: "
                       "%s vs %s (max diff: %s)" % (violating, len(rows), exs.rust_f64(tl), exs.rust_f64(tr), exs.fixed4(worst)))
    same = S.CrossTableSumConstraint("orders.v", "orders.v").group_by(["a", "b"]).composite_groups_on_device()
    status, metric, message = gs.run_constraint(same, {"orders": orders})
    # a table against itself: every key without a NULL joins with no difference; each key with one is two groups
    nulls = [abs(left[k]) for k in left if None in k]
    assert (status == "success") == (max(nulls) == 0) and metric == max(nulls)


# ---- GROUP_SUMS: the value column's own offset and the long class, case by case as for GROUP_COUNTS ---------------------------
@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("off", OFFSETS)
def test_sums_every_component_and_the_value_column_has_its_own_arrow_offset(off, mem):
    rng = np.random.default_rng(200 + off)
    n, room = 3000, 70
    a = ints(rng.integers(0, 5, n + room), mask=rng.random(n + room) >= 0.3).slice(off, n)
    b = pa.array(["k%d" % k if k else None for k in rng.integers(0, 5, n + room)], pa.string()).slice((off + 7) % 65, n)
    c = dictionary(rng.integers(0, 3, n + room), ["u", "v", None], mask=rng.random(n + room) >= 0.2).slice((off + 13) % 65, n)
    vi = gs.amounts(rng, n + room, 0.4).slice((off + 9) % 65, n)
    vf = gs.floats(rng.integers(-50, 50, n + room), mask=rng.random(n + room) >= 0.4).slice((off + 31) % 65, n)
    check_sums(vi, [a, b, c], mem=mem)
    check_sums(vf, [a, b, c], is_float=True, mem=mem)
    check_sums(vi, [a, ints(rng.integers(0, 4, n + room), mask=rng.random(n + room) >= 0.1).slice((off + 5) % 65, n)], mem=mem)


@pytest.mark.parametrize("rate", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("position", [0, 1, 2])
def test_sums_a_null_in_every_position(position, rate):
    rng = np.random.default_rng(int(300 + position * 10 + rate * 100))
    n = 3000
    groups = mixed_groups(rng, n, 3, nulls=0.0)
    src = groups[position]
    mask = rng.random(n) >= rate
    groups[position] = pa.array([v if ok else None for v, ok in zip(src.to_pylist(), mask)], type=src.type) \
        if not pa.types.is_dictionary(src.type) else dictionary(src.indices.to_numpy(), ["a", "b", "", "c"], mask=mask)
    _, _, want = check_sums(gs.amounts(rng, n, 0.5), groups)
    assert sum(e[0] for k, e in want["entries"].items() if ext.decode(k)[position] is None) == int((~mask).sum())


def test_sums_an_index_outside_the_dictionary_is_a_null_component():
    rng = np.random.default_rng(310)
    n = 1000
    idx = rng.integers(-1, 4, n).astype(np.int32)  # -1 and 3 lie outside a dictionary of three entries
    v = gs.amounts(rng, n)
    g = ints(rng.integers(0, 2, n))
    T.init()
    d = on_device(T.Column.dict32_utf8(idx, T.Column.from_arrow(pa.array(["p", "q", "r"], pa.string()))))
    st = feed(sums_plan(2), [[column(g), d, column(v)]])
    keys = [None if i in (-1, 3) else [b"p", b"q", b"r"][i] for i in idx]
    got = gs.read(st)
    assert got == ext.walk_sums(v.to_pylist(), [cells_of(g), keys])
    assert sum(e[0] for k, e in got["entries"].items() if ext.decode(k)[1] is None) == int(((idx == -1) | (idx == 3)).sum())
    gs.identities(got, n - v.null_count, exs.wrap(sum(x for x in v.to_pylist() if x is not None)))


@pytest.mark.parametrize("numeric", [True, False], ids=["integers", "mixed"])
def test_sums_an_encoded_length_of_exactly_max_value_bytes_and_one_above(numeric):
    rng = np.random.default_rng(320)
    n = 2000
    if numeric:  # (int, int) is 18 bytes, (int, NULL) 10
        groups = [ints(rng.integers(0, 5, n)), ints(rng.integers(0, 5, n), mask=rng.random(n) >= 0.3)]
        at, short = 18, 10
    else:  # (int, string of k bytes) is 12 + k
        groups = [ints(rng.integers(0, 3, n)), pa.array(["x" * k for k in rng.integers(19, 23, n)], pa.string())]
        at, short = 12 + 21, 12 + 19
    for v, is_float in ((gs.amounts(rng, n, 0.5), False), (gs.floats(rng.integers(-9, 9, n), mask=rng.random(n) >= 0.5), True)):
        _, _, want = check_sums(v, groups, is_float=is_float, max_value_bytes=at)
        assert (want["long_rows"][0] == 0) == numeric and max(map(len, want["entries"])) == at
        _, _, above = check_sums(v, groups, is_float=is_float, max_value_bytes=at - 1)
        assert above["long_rows"][0] > above["long_rows"][1] > 0 and max(map(len, above["entries"])) < at
        assert min(map(len, above["entries"])) == short
