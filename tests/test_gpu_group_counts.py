"""TGX_CHECK_GROUP_COUNTS on the device, held against tests/exact_group_counts.py: the whole key -> (total, non_null)
map and all ten counters are compared for equality with the exact per-row walk, and both identities are checked each
time -- the second against a plain COUNT of the value column -- on every route (integers through the workgroups' LDS
tables and their spill path, Utf8 / LargeUtf8 / Utf8View, dictionaries), for value columns whose validity has its own
Arrow offset, for walks shared by several value columns, every memory kind and batching, and every way a state travels
(read half-way, reset, merge, blob, tgx_allreduce)."""
import ctypes
import struct
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_group_counts as ex
import term_amd as T
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2**63, 2**63 - 1
SHARE = 1024 * 16  # rows a workgroup of the integer kernel takes before a second one is launched


# ---- columns ------------------------------------------------------------------------------------------------------------
def padded(buf):
    """a device copy with 64 spare bytes behind it (string kernels read whole 8-byte words)"""
    if buf is None:
        return None
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return to_device(np.concatenate([raw, np.zeros(64, np.uint8)]))


def on_device(col):
    values, validity, offsets, data, dictionary, variadic = col._keep[:6]
    return T.Column(col.c.type, col.c.length, values=padded(values), validity=padded(validity), offsets=padded(offsets),
                    data=padded(data), offset=col.c.offset, mem=T.MEM_DEVICE,
                    dictionary=None if dictionary is None else on_device(dictionary),
                    variadic=None if variadic is None else [padded(b) for b in variadic])


def column(arr, mem=T.MEM_DEVICE):
    col = arr if isinstance(arr, T.Column) else T.Column.from_arrow(arr)
    if mem == T.MEM_DEVICE:
        return on_device(col)
    col.c.mem = mem
    return col


def as_exact(values):
    return [None if v is None else (v.encode() if isinstance(v, str) else (bytes(v) if isinstance(v, bytes) else int(v)))
            for v in values]


def cut(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def ints(values, type=pa.int64(), mask=None):
    return pa.array(values, type=type, mask=None if mask is None else ~np.asarray(mask))


def flags(rng, n, nulls=0.3):
    """a value column of which only the validity matters"""
    return ints(np.arange(n), mask=rng.random(n) >= nulls)


def plan_of(n_values, bounds=None, extra=()):
    """column 0 is the group column, columns 1 .. n_values the value columns; one spec each, then a COUNT each"""
    plan = T.Plan([spec(T.GROUP_COUNTS, 1 + m, column2=0) for m in range(n_values)] +
                  [spec(T.COUNT, 1 + m) for m in range(n_values)] + list(extra))
    for m in range(n_values):
        plan.set_group_counts(m, *(bounds[m] if bounds else (10000, 256)))
    return plan


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def read(st, i=0):
    summary, entries = st.group_counts(i)
    return dict(summary, entries=entries)


def identities(got, count):
    """every row is in exactly one class, and so is every non-NULL value; `count`: COUNT(value column)"""
    assert got["counted"] + got["null_group_rows"] + got["overflow_rows"] + got["long_rows"] == got["seen"]
    assert got["counted_non_null"] + got["null_group_non_null"] + got["overflow_non_null"] + got["long_non_null"] == count
    assert got["counted"] == sum(t for t, _ in got["entries"].values())
    assert got["counted_non_null"] == sum(n for _, n in got["entries"].values())
    assert got["groups"] == len(got["entries"])


def exact(value_arr, group_arr, max_value_bytes=256):
    valid = [None if v is None else 1 for v in (value_arr.to_pylist() if not isinstance(value_arr, list) else value_arr)]
    return ex.walk(valid, as_exact(group_arr.to_pylist()), max_value_bytes)


def check(values, groups, max_groups=10000, max_value_bytes=256, mem=T.MEM_DEVICE, cuts=None, want=None, group_col=None,
          value_cols=None):
    """`values`: the value columns (pyarrow arrays) of one walk over `groups`"""
    T.init()
    n = len(groups)
    plan = plan_of(len(values), [(max_groups, max_value_bytes)] * len(values))
    cols = [group_col or column(groups, mem)] + (value_cols or [column(v, mem) for v in values])
    st = feed(plan, cut(cols, n, cuts))
    res = st.finalize()
    wants = []
    for m, v in enumerate(values):
        w = want[m] if want is not None else exact(v, groups, max_value_bytes)
        got = read(st, m)
        assert got == w and list(got["entries"]) == list(w["entries"])  # (the order too: ascending by key)
        count = res[len(values) + m]
        assert count.total == n
        identities(got, count.non_null)
        r = res[m]
        assert (r.total, r.non_null, r.distinct, r.matches) == (n, count.non_null, w["groups"], w["counted"])
        wants.append(w)
    return st, plan, wants


# ---- integer keys ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, SHARE - 1, SHARE, SHARE + 1])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    check([flags(rng, n)], ints(rng.integers(-20, 20, n), mask=rng.random(n) >= 0.1))


def test_a_constant_key_and_64_distinct_keys_in_a_wave():
    rng = np.random.default_rng(1)
    n = 20_000
    check([flags(rng, n), flags(rng, n, 0.0)], ints(np.full(n, 42)))
    check([flags(rng, n)], ints(np.full(n, 42), mask=np.arange(n) % 3 != 0))
    check([flags(rng, n)], ints(np.arange(n) % 64 * 1_000_003))


def test_the_marker_value_and_the_extremes():
    rng = np.random.default_rng(2)
    v = [-1, -1, I64_MIN, I64_MAX, 0, -1, I64_MAX, -2, 1, None, -1] * 50
    _, _, want = check([flags(rng, len(v), 0.5)], ints(v))
    assert -1 in want[0]["entries"] and 0 < want[0]["entries"][-1][1] < want[0]["entries"][-1][0]
    check([flags(rng, 300)], ints([-1] * 300))
    check([flags(rng, 300), flags(rng, 300, 1.0)], ints([None, -1, None] * 100))


def test_more_keys_than_a_workgroups_lds_table_holds():
    """20 000 keys over 200 000 rows: a workgroup's share of 16 384 rows holds some 11 000 keys, more than any LDS
    table takes (8192 slots with one member, 2048 with eight), so rows go to the global table directly"""
    rng = np.random.default_rng(3)
    n = 200_000
    keys = rng.integers(0, 20_000, n) * 1_000_003 - 5
    valid = rng.random(n) >= 0.4
    want = ex.walk_np(valid, keys)
    assert want["groups"] > 2 * 8192
    check([ints(np.arange(n), mask=valid)], ints(keys), max_groups=30_000, want=[want])
    valids = [rng.random(n) >= p for p in (0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0)]
    check([ints(np.arange(n), mask=v) for v in valids], ints(keys), max_groups=30_000,
          want=[ex.walk_np(v, keys) for v in valids])


@pytest.mark.parametrize("extra", [0, 1])
def test_all_rows_distinct_at_max_groups_and_one_above(extra):
    rng = np.random.default_rng(4)
    n = 1000 + extra
    _, _, want = check([flags(rng, n)], ints(rng.permutation(n) * 7 - 3000), max_groups=1000)
    assert want[0]["groups"] == n and want[0]["overflow_rows"] == 0  # one above: reported, the caller compares


def test_more_keys_than_the_global_table_has_slots():
    rng = np.random.default_rng(5)
    n = 30_000
    keys, valid = rng.integers(0, 5000, n), rng.random(n) >= 0.5
    T.init()
    plan = plan_of(1, [(4, 256)])  # 8 slots
    st = feed(plan, [[column(ints(keys)), column(ints(np.arange(n), mask=valid))]])
    got, true = read(st), ex.walk_np(valid, keys)
    assert got["overflow_rows"] > 0 and 0 < got["overflow_non_null"] < got["overflow_rows"] and got["groups"] <= 8
    identities(got, int(valid.sum()))
    assert st.finalize()[1].non_null == int(valid.sum())
    assert all(0 < t <= true["entries"][k][0] and nn <= true["entries"][k][1] for k, (t, nn) in got["entries"].items())


NARROW = [(pa.int8(), [-128, -1, 0, 127, -1]), (pa.int16(), [-32768, -1, 32767, 5]), (pa.int32(), [-2**31, -1, 2**31 - 1, 7]),
          (pa.uint8(), [0, 255, 128]), (pa.uint16(), [0, 65535, 32768]), (pa.uint32(), [0, 2**31, 2**32 - 1, 2**31 + 1]),
          (pa.date32(), [-1, 0, 19000])]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("type,values", NARROW, ids=[str(t) for t, _ in NARROW])
def test_narrow_group_types_are_widened(type, values, mem):
    rng = np.random.default_rng(6)
    picks = [values[i] for i in rng.integers(0, len(values), 700)]
    arr = pa.array([None if rng.random() < 0.1 else p for p in picks], type=pa.int32() if type == pa.date32() else type)
    v = flags(rng, 700)
    want = [exact(v, arr)]
    check([v], arr.cast(type) if type == pa.date32() else arr, mem=mem, want=want)


# ---- Arrow offsets and NULL rates ---------------------------------------------------------------------------------------------
OFFSETS = [0, 1, 8, 9, 63, 64]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("goff", OFFSETS)
def test_the_two_columns_have_independent_arrow_offsets(goff, mem):
    rng = np.random.default_rng(goff)
    n, room = 3000, 64
    for voff in [o for o in OFFSETS if o != goff]:
        g = ints(rng.integers(0, 9, n + room), mask=rng.random(n + room) >= 0.3).slice(goff, n)
        v = flags(rng, n + room, 0.5).slice(voff, n)
        check([v], g, mem=mem)
    s = pa.array(["k%d" % k if k else None for k in rng.integers(0, 9, n + room)], pa.string()).slice(goff, n)
    check([flags(rng, n + room, 0.5).slice((goff + 9) % 65, n)], s, mem=mem)


@pytest.mark.parametrize("group_nulls", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("value_nulls", [0.0, 0.5, 1.0])
def test_null_rates(value_nulls, group_nulls):
    rng = np.random.default_rng(int(value_nulls * 10 + group_nulls * 100))
    n = 3000
    g = ints(rng.integers(0, 9, n), mask=rng.random(n) >= group_nulls)
    _, _, want = check([flags(rng, n, value_nulls).slice(0)], g)
    assert want[0]["null_group_rows"] == g.null_count


def test_a_value_column_without_a_validity_buffer():
    rng = np.random.default_rng(7)
    n = 5000
    v = ints(np.arange(n))
    assert T.Column.from_arrow(v).c.validity is None
    g = ints(rng.integers(0, 9, n), mask=rng.random(n) >= 0.2)
    _, _, want = check([v, flags(rng, n)], g)
    assert all(t == nn for t, nn in want[0]["entries"].values()) and want[0]["null_group_non_null"] == g.null_count


# ---- value column types ---------------------------------------------------------------------------------------------------
def test_value_columns_of_every_type():
    rng = np.random.default_rng(8)
    n = 4000
    mask = rng.random(n) >= 0.3
    g = ints(rng.integers(0, 9, n), mask=rng.random(n) >= 0.1)
    plain = [ints(np.arange(n), mask=mask), pa.array(np.arange(n, dtype=np.float64), mask=~mask),
             pa.array(["s%d" % i for i in range(n)], pa.string(), mask=~mask), pa.array(np.arange(n) % 2 == 0, mask=~mask),
             pa.array(np.arange(n, dtype=np.int32), mask=~mask)]
    want = [exact(ints(np.arange(n), mask=mask), g)] * (len(plain) + 1)
    for mem in (T.MEM_DEVICE, T.MEM_HOST):
        nested = pa.array([None if not ok else [i, i] for i, ok in enumerate(mask)], pa.list_(pa.int64()))
        cols = [column(a, mem) for a in plain] + [column(T.Column.validity_only(nested), mem)]
        check(plain + [nested], g, mem=mem, want=want, value_cols=cols)


def test_the_value_column_is_the_group_column():
    rng = np.random.default_rng(9)
    n = 4000
    g = ints(rng.integers(0, 9, n), mask=rng.random(n) >= 0.2)
    T.init()
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, column2=0), spec(T.COUNT, 0)])
    plan.set_group_counts(0)
    st = feed(plan, [[column(g)]])
    got = read(st)
    assert got == exact(g, g) and all(t == nn for t, nn in got["entries"].values())
    assert (got["null_group_rows"], got["null_group_non_null"]) == (g.null_count, 0)
    identities(got, st.finalize()[1].non_null)


# ---- shared walks -----------------------------------------------------------------------------------------------------------
def launches_of(plan, cols):
    st = T.State(plan)
    st.profile_enable(True)
    st.update(cols)
    st.finalize()
    return st, st.profile_get("group_counts")["launches"]


@pytest.mark.parametrize("n_values,walks", [(8, 1), (9, 2)])
def test_value_columns_share_one_walk_of_the_group_column(n_values, walks):
    rng = np.random.default_rng(10 + n_values)
    n = 20_000
    g = ints(rng.integers(0, 300, n) * 77, mask=rng.random(n) >= 0.1)
    values = [flags(rng, n + 70, m / 8).slice(m * 7 + 1, n) for m in range(n_values)]  # every member its own offset
    T.init()
    cols = [column(g)] + [column(v) for v in values]
    st, launches = launches_of(plan_of(n_values), cols)
    assert launches == walks  # one launch a walk, not one a spec
    res = st.finalize()
    for m, v in enumerate(values):
        got = read(st, m)
        assert got == exact(v, g)
        identities(got, res[n_values + m].non_null)


def test_the_same_value_column_twice_and_two_specs_with_different_bounds():
    rng = np.random.default_rng(12)
    n = 20_000
    g = pa.array(["key-%d" % k for k in rng.integers(0, 200, n)], pa.string())
    v = flags(rng, n)
    T.init()
    plan = T.Plan([spec(T.GROUP_COUNTS, 1, column2=0), spec(T.GROUP_COUNTS, 1, column2=0), spec(T.GROUP_COUNTS, 1, column2=0)])
    plan.set_group_counts(0)
    plan.set_group_counts(1)
    plan.set_group_counts(2, 64, 5)
    st, launches = launches_of(plan, [column(g), column(v)])
    assert launches == 2
    want = exact(v, g)
    assert read(st, 0) == read(st, 1) == want
    tight = read(st, 2)
    assert (tight["long_rows"], tight["long_non_null"]) == (exact(v, g, 5)["long_rows"], exact(v, g, 5)["long_non_null"])
    assert tight["long_rows"] > 0
    identities(tight, n - v.null_count)


# ---- string keys ------------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 12, 13, 15, 16, 17, 32, 33, 40, 41]
WORDS = ["x" * k for k in LENGTHS] + ["y" * k for k in LENGTHS[1:]] + ["Zoë", "a\x00b", "user@example.com"]


def words(rng, n, null=0.1):
    return [None if rng.random() < null else WORDS[i] for i in rng.integers(0, len(WORDS), n)]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("type", [pa.string(), pa.large_string(), pa.string_view()], ids=str)
def test_string_layouts_and_lengths(type, mem):
    """the empty string is a key apart from NULL; 40 is max_value_bytes, 41 a long row; a Utf8View holds values of up
    to 12 bytes inline"""
    rng = np.random.default_rng(13)
    g = pa.array(words(rng, 5000), type=type)
    _, _, want = check([flags(rng, 5000, 0.5), flags(rng, 5000, 0.0)], g, max_value_bytes=40, mem=mem)
    w = want[0]
    assert w["long_rows"] > w["long_non_null"] > 0 and b"" in w["entries"] and b"x" * 40 in w["entries"]
    assert w["null_group_rows"] > 0
    check([flags(rng, 5003, 0.5).slice(0, 4997)], g.slice(3), max_value_bytes=40, mem=mem)


def test_a_view_column_with_two_data_buffers():
    rng = np.random.default_rng(14)
    vals = words(rng, 2000, null=0.0)
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
    v = flags(rng, len(vals))
    plan = plan_of(1, [(100, 40)])
    st = feed(plan, [[col.sliced(0, len(vals)), column(v)]])
    assert read(st) == ex.walk(v.to_pylist(), as_exact(vals), 40)


# ---- dictionaries -------------------------------------------------------------------------------------------------------------
def dictionary(indices, entries, mask=None):
    return pa.DictionaryArray.from_arrays(pa.array(indices, pa.int32(), mask=None if mask is None else ~np.asarray(mask)),
                                          pa.array(entries, pa.string()))


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
def test_a_dictionary_with_unused_null_and_repeated_entries(mem):
    rng = np.random.default_rng(15)
    entries = ["a", None, "b", "a", "unused", "", "x" * 41, "b"]  # 0 and 3, 2 and 7 repeat a value; 1 is NULL; 6 is long
    idx = rng.choice([0, 1, 2, 3, 5, 6, 7], 4000)
    g = dictionary(idx, entries, mask=rng.random(4000) >= 0.1)
    _, _, want = check([flags(rng, 4000, 0.5), flags(rng, 4009).slice(9)], g, max_value_bytes=40, mem=mem)
    assert set(want[0]["entries"]) == {b"a", b"b", b""} and want[0]["long_rows"] > 0
    assert want[0]["null_group_rows"] > g.indices.null_count  # (the rows of the NULL entry are NULL-key rows too)


def test_an_index_outside_the_dictionary_is_a_null_key_row():
    rng = np.random.default_rng(16)
    n = 1000
    idx = rng.integers(-1, 4, n).astype(np.int32)  # -1 and 3 lie outside a dictionary of three entries
    v = flags(rng, n)
    entries = T.Column.from_arrow(pa.array(["p", "q", "r"], pa.string()))
    T.init()
    g = on_device(T.Column.dict32_utf8(idx, entries))
    st = feed(plan_of(1), [[g, column(v)]])
    keys = [None if i in (-1, 3) else [b"p", b"q", b"r"][i] for i in idx]
    got = read(st)
    assert got == ex.walk(v.to_pylist(), keys) and got["null_group_rows"] == int(((idx == -1) | (idx == 3)).sum())
    identities(got, n - v.null_count)


def test_batches_with_different_dictionaries_unite_by_value():
    T.init()
    a = dictionary([0, 1, 1, 2], ["red", "green", "blue"])
    b = dictionary([0, 0, 1, 2, 2], ["blue", "yellow", "red"])
    va, vb = ints([1, None, 3, 4]), ints([None, 2, 3, None, 5])
    st = feed(plan_of(1), [[column(a), column(va)], [column(b), column(vb)]])
    assert read(st)["entries"] == {b"blue": (3, 2), b"green": (2, 1), b"red": (3, 2), b"yellow": (1, 1)}
    identities(read(st), 6)


def test_a_dictionary_above_the_lds_cell_limit():
    """16 384 LDS cells hold (1 + members) counters an entry: 9000 entries with one member and 2000 with eight go
    through global cells, 1000 with one member through LDS"""
    rng = np.random.default_rng(17)
    n = 50_000
    for n_entries, members in ((9000, 1), (2000, 8), (1000, 1)):
        entries = ["k%05d" % i for i in range(n_entries)]
        g = dictionary(rng.integers(0, n_entries, n), entries, mask=rng.random(n) >= 0.05)
        check([flags(rng, n, m / 8) for m in range(members)], g, max_groups=30_000)


# ---- batching and the ways a state travels ---------------------------------------------------------------------------------
N_BIG = 300_000


@pytest.fixture(scope="module")
def big():
    """three group columns (integers, strings, a dictionary), each with two value columns"""
    rng = np.random.default_rng(18)
    iv = ints(rng.zipf(1.3, N_BIG) % 5000 - 100, mask=rng.random(N_BIG) >= 0.05)
    sv = pa.array(["c%d" % k if k % 7 else None for k in rng.integers(0, 300, N_BIG)], pa.string())
    dv = dictionary(rng.integers(0, 50, N_BIG), ["d%d" % (k % 40) for k in range(50)], mask=rng.random(N_BIG) >= 0.02)
    va, vb = flags(rng, N_BIG, 0.3), flags(rng, N_BIG, 0.9)
    arrs = [iv, sv, dv, va, vb]
    return arrs, [exact(v, g) for g in (iv, sv, dv) for v in (va, vb)]


def big_plan(extra=()):
    plan = T.Plan([spec(T.GROUP_COUNTS, v, column2=g) for g in (0, 1, 2) for v in (3, 4)] + list(extra))
    for i in range(6):
        plan.set_group_counts(i)
    return plan


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192), (T.MEM_HOST_RETAINED, 8192),
                                      (T.MEM_HOST, [3, 8195, 8196, 200_001])])
def test_batching_independence(big, mem, cuts):
    arrs, want = big
    T.init()
    st = feed(big_plan(), cut([column(a, mem) for a in arrs], N_BIG, cuts))
    assert [read(st, i) for i in range(6)] == want


def test_state_algebra(big):
    arrs, want = big
    T.init()
    cols = [column(a) for a in arrs]
    parts = cut(cols, N_BIG, [100_000, 200_001])
    plan = big_plan()
    # read half-way, then on
    st = feed(plan, parts[:1])
    head = [a.slice(0, 100_000) for a in arrs]
    assert [read(st, i) for i in range(6)] == [exact(v, g) for g in head[:3] for v in head[3:]]
    st.update(parts[1])
    st.update(parts[2])
    assert [read(st, i) for i in range(6)] == want
    # reset and refill
    st.reset()
    assert read(st)["seen"] == 0 and read(st)["entries"] == {} and read(st)["null_group_rows"] == 0
    st.update(cols)
    assert [read(st, i) for i in range(6)] == want
    # merge of three states
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    assert [read(states[0], i) for i in range(6)] == want
    # a blob round trip into a fresh state; equal states give equal bytes
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    assert [read(back, i) for i in range(6)] == want and back.serialize() == blob == st.serialize()
    back.merge([st])
    assert read(back, 2)["entries"] == {k: (2 * t, 2 * n) for k, (t, n) in want[2]["entries"].items()}
    assert read(back, 2)["null_group_non_null"] == 2 * want[2]["null_group_non_null"]
    other = T.Plan([spec(T.GROUP_COUNTS, v, column2=g) for g in (0, 1, 2) for v in (3, 4)])
    for i in range(6):
        other.set_group_counts(i, 10000, 255)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(other, blob)


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(big, world, device_buffers):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    arrs, want = big
    T.init()
    whole = [column(a) for a in arrs]
    plan = big_plan(extra=[spec(T.COUNT, 3)])
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
            results[rank] = (res, [read(st, i) for i in range(6)])
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
        assert res[6].total == N_BIG and res[0].non_null == res[6].non_null


# ---- isolation ------------------------------------------------------------------------------------------------------------------
def test_the_kind_leaves_the_other_kinds_bit_for_bit(big):
    arrs, want = big
    T.init()
    cols = [column(a) for a in arrs]
    others = [spec(T.COUNT, 0), spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.COUNT, 1), spec(T.DISTINCT, 1),
              spec(T.REGEX_MATCH, 1, pattern=r"^c1\d*$"), spec(T.DISTINCT, 2), spec(T.COUNT, 3), spec(T.NUMERIC_STATS, 4)]
    alone = feed(T.Plan(others), [cols]).finalize()
    st = feed(big_plan(extra=others), [cols])
    res = st.finalize()
    assert [read(st, i) for i in range(6)] == want
    for got, ref in zip(res[6:], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))


def test_a_plan_without_the_kind_profiles_no_such_kernel(big):
    arrs, _ = big
    T.init()
    cols = [column(arrs[0]), column(arrs[3])]
    launches = []
    plans = [T.Plan([spec(T.COUNT, 0), spec(T.COUNT, 1)]), T.Plan([spec(T.GROUP_COUNTS, 1, column2=0), spec(T.COUNT, 0)])]
    plans[1].set_group_counts(0)
    for plan in plans:
        launches.append(launches_of(plan, cols)[1])
    assert launches == [0, 1]


def test_other_group_types_are_unsupported_and_the_state_stays_usable():
    """the refused batches go to the very state that is read afterwards"""
    T.init()
    n = 1000
    st = T.State(plan_of(1))
    v = ints(np.arange(n), mask=np.arange(n) % 4 != 0)
    refused = [(pa.array(np.arange(n, dtype=np.float64)), "Float64"), (pa.array(np.arange(n, dtype=np.float32)), "Float32"),
               (pa.array(np.arange(n, dtype=np.uint64)), "UInt64"), (pa.array(np.arange(n) % 2 == 0), "Boolean")]
    for arr, name in refused:
        for mem in (T.MEM_HOST, T.MEM_DEVICE):
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*GROUP_COUNTS.*" + name):
                st.update([column(arr, mem), column(v, mem)])
    for mem in (T.MEM_HOST, T.MEM_DEVICE):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*GROUP_COUNTS.*validity-only"):
            st.update([column(T.Column.validity_only(pa.array([[1]] * n, pa.list_(pa.int64()))), mem), column(v, mem)])
    assert read(st)["seen"] == 0
    st.update([column(ints(np.arange(n) % 10)), column(v)])
    got = read(st)
    assert got["seen"] == n and {k: t for k, (t, _) in got["entries"].items()} == {k: 100 for k in range(10)}
    identities(got, 750)


# ---- end to end: CompletenessAnalyzer(c).with_grouping(..) through AnalysisRunner ---------------------------------------------
def exact_metric(values, group, by, **kw):
    """the metric map of `values` grouped by the pyarrow column `group`, by the exact module"""
    valid = [None if v is None else 1 for v in values.to_pylist()]
    return ex.metric_map(ex.grouped_state(ex.group_by(valid, as_exact(group.to_pylist())), [by], **kw))


def metric_values(ctx, key):
    m = ctx.get_metric(key)
    assert m["type"] == "Map"
    return {k: v["value"] for k, v in m["value"].items()}


def test_the_reference_table_through_the_runner():
    import json
    import os

    import term_amd.suite as S

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grouped_completeness_vectors.json")) as f:
        golden = json.load(f)
    T.init()
    t = golden["table"]
    table = pa.table({"region": pa.array(t["region"], pa.string()), "product": pa.array(t["product"], pa.string()),
                      "sales": pa.array(t["sales"], pa.int32())})
    runner = S.AnalysisRunner()
    for by in ("region", "product"):
        runner.add(S.CompletenessAnalyzer("sales").with_grouping(S.GroupingConfig([by])))
    runner.add(S.CompletenessAnalyzer("sales")).add(S.CompletenessAnalyzer("sales").with_grouping(S.GroupingConfig(["region", "product"])))
    ctx = runner.run(table)
    for by in ("region", "product"):
        key = "completeness.sales_grouped_by_" + by
        want = {g["key"][0]: g["non_null_count"] / g["total_count"] for g in golden["by_" + by]["groups"]}
        got = metric_values(ctx, key)
        assert {k: got[k] for k in want} == want and got["__overall__"] == 5 / 6
        assert got == exact_metric(table["sales"].combine_chunks(), table[by].combine_chunks(), by)
        assert [(g["key"], g["total_count"], g["non_null_count"]) for g in ctx.states[key]["groups"]] == \
            [(g["key"], g["total_count"], g["non_null_count"]) for g in golden["by_" + by]["groups"]]
        assert ctx.states[key]["overall"] == {"total_count": 6, "non_null_count": 5}
    assert ctx.get_metric("completeness.sales")["value"] == 5 / 6
    assert [e["analyzer_name"] for e in ctx.errors()] == ["completeness"]  # two group columns: the analyzer's error
    assert "exactly one column" in ctx.errors()[0]["error"]


def test_a_big_table_through_the_runner(big):
    import term_amd.suite as S

    arrs, want = big
    T.init()
    table = pa.table({"n": arrs[0], "s": arrs[1], "va": arrs[3], "vb": arrs[4],
                      "f": pa.array(np.arange(N_BIG, dtype=np.float64))})
    loose = dict(strict_reference_types=False)
    runner = S.AnalysisRunner()
    runner.add(S.CompletenessAnalyzer("va").with_grouping(S.GroupingConfig(["s"])))
    runner.add(S.CompletenessAnalyzer("vb").with_grouping(S.GroupingConfig(["s"], max_groups=200)))  # a table of 512 slots holds the 258
    runner.add(S.CompletenessAnalyzer("va").with_grouping(S.GroupingConfig(["n"], **loose)))
    runner.add(S.CompletenessAnalyzer("va").with_grouping(S.GroupingConfig(["n"])))            # strict: Int64 is refused
    runner.add(S.CompletenessAnalyzer("va").with_grouping(S.GroupingConfig(["f"], **loose)))   # floats: the device refuses
    runner.add(S.CompletenessAnalyzer("vb").with_grouping(S.GroupingConfig(["n"], max_groups=16, **loose)))  # overflows
    runner.add(S.CompletenessAnalyzer("va"))
    ctx = runner.run(table)
    assert metric_values(ctx, "completeness.va_grouped_by_s") == exact_metric(arrs[3], arrs[1], "s")
    got = metric_values(ctx, "completeness.va_grouped_by_n")
    assert got == exact_metric(arrs[3], arrs[0], "n") and len(got) == want[0]["groups"] + 3  # + NULL, overall, metadata
    cut = ex.grouped_state(ex.group_by([None if v is None else 1 for v in arrs[4].to_pylist()], as_exact(arrs[1].to_pylist())),
                           ["s"], max_groups=200)
    state = ctx.states["completeness.vb_grouped_by_s"]
    assert state["metadata"] == cut["metadata"] and cut["metadata"]["truncated"] and cut["metadata"]["total_groups"] == 201
    assert (state["overall"]["total_count"], state["overall"]["non_null_count"]) == cut["overall"]
    kept = {tuple(g["key"]): (g["total_count"], g["non_null_count"]) for g in state["groups"]}
    if state["null_group"]:
        kept[("",)] = (state["null_group"]["total_count"], state["null_group"]["non_null_count"])
    assert kept == cut["groups"]
    assert ctx.get_metric("completeness.va")["value"] == (N_BIG - arrs[3].null_count) / N_BIG
    errors = [e["error"] for e in ctx.errors()]
    assert [e["analyzer_name"] for e in ctx.errors()] == ["completeness"] * 3
    assert "group column 'n' is Int64" in errors[0] and "GROUP_COUNTS groups by integer and string columns" in errors[1]
    assert "overflow rows" in errors[2] and " 0 overflow rows" not in errors[2]
