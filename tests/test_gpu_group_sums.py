"""TGX_CHECK_GROUP_SUMS on the device, held against tests/exact_group_sums.py.  Integer sums, every counter and the
entries are compared for EQUALITY with the exact per-row walk (sums modulo 2^64), and the three identities are checked each
time.  Float sums are checked two ways: data of small integers held as doubles, whose every partial sum is exact in any
order, for equality; general data group by group against math.fsum within the bound of any summation order
(exact_group_sums.float_bound).  Every route (integers through the workgroups' LDS tables and their spill path, Utf8 /
LargeUtf8 / Utf8View, dictionaries), every memory kind and batching, and every way a state travels (read half-way, reset,
merge, blob, tgx_allreduce)."""
import ctypes
import math
import struct
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_group_sums as ex
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


def floats(values, mask=None, type=pa.float64()):
    return pa.array(np.asarray(values, np.float64), type=type, mask=None if mask is None else ~np.asarray(mask))


def amounts(rng, n, nulls=0.3, lo=-1000, hi=1000):
    """an Int64 value column"""
    return ints(rng.integers(lo, hi, n), mask=rng.random(n) >= nulls)


def plan_of(bounds=(10000, 256), extra=()):
    """column 0 is the group column, column 1 the value column: the spec, a COUNT and the plain SUM of the value column"""
    plan = T.Plan([spec(T.GROUP_SUMS, 1, column2=0), spec(T.COUNT, 1), spec(T.NUMERIC_STATS, 1)] + list(extra))
    plan.set_group_sums(0, *bounds)
    return plan


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def read(st, i=0):
    summary, entries = st.group_sums(i)
    return dict(summary, entries=entries)


CLASSES = ("counted", "null_group", "overflow", "long_rows")


def identities(got, count, total=None):
    """every row is in exactly one class, and so are every non-NULL value and (integers, modulo 2^64) the sum;
    `count`: COUNT(value column), `total`: its SUM"""
    assert sum(got[c][0] for c in CLASSES) == got["seen"]
    assert sum(got[c][1] for c in CLASSES) == count
    assert got["counted"][0] == sum(e[0] for e in got["entries"].values())
    assert got["counted"][1] == sum(e[1] for e in got["entries"].values())
    assert got["groups"] == len(got["entries"])
    if not got["is_float"]:
        assert got["counted"][2] == ex.wrap(sum(e[2] for e in got["entries"].values()))
        if total is not None:
            assert ex.wrap(sum(got[c][2] for c in CLASSES)) == total


def exact(value_arr, group_arr, max_value_bytes=256, is_float=False):
    return ex.walk(value_arr.to_pylist(), as_exact(group_arr.to_pylist()), max_value_bytes, is_float)


def same_float(got, want, exactly):
    """one class: (rows, non_null, sum) against (rows, non_null, fsum, sum of magnitudes)"""
    assert got[:2] == want[:2], (got, want)
    if want[2] != want[2]:
        assert got[2] != got[2], (got, want)
    elif exactly or math.isinf(want[2]):
        assert got[2] == want[2], (got, want)
    else:
        assert abs(got[2] - want[2]) <= ex.float_bound(want[1], want[2], want[3]), (got, want)


def compare_float(got, want, exactly):
    assert (got["seen"], got["groups"], got["is_float"]) == (want["seen"], want["groups"], want["is_float"])
    assert list(got["entries"]) == list(want["entries"])  # (the order too: ascending by key)
    for k, w in want["entries"].items():  # every group
        same_float(got["entries"][k], w, exactly)
    for c in CLASSES[1:]:
        same_float(got[c], want[c], exactly)
    assert got["counted"][:2] == want["counted"]
    total = 0.0
    for e in got["entries"].values():  # the host adds the entries in ascending key order
        total += e[2]
    assert got["counted"][2] == total or (total != total and got["counted"][2] != got["counted"][2])


def check(values, groups, is_float=False, exactly=True, max_groups=10000, max_value_bytes=256, mem=T.MEM_DEVICE, cuts=None,
          want=None, group_col=None, value_col=None):
    T.init()
    n = len(groups)
    plan = plan_of((max_groups, max_value_bytes))
    cols = [group_col or column(groups, mem), value_col or column(values, mem)]
    st = feed(plan, cut(cols, n, cuts))
    res = st.finalize()
    want = want if want is not None else exact(values, groups, max_value_bytes, is_float)
    got = read(st)
    assert res[1].total == n
    r = res[0]
    assert (r.total, r.non_null, r.distinct, r.matches, r.has_value) == (n, res[1].non_null, want["groups"],
                                                                       want["counted"][0], int(res[1].non_null > 0))
    if is_float:
        compare_float(got, want, exactly)
        identities(got, res[1].non_null)
        assert r.sum_i == 0
    else:
        assert got == want and list(got["entries"]) == list(want["entries"])  # (the order too: ascending by key)
        identities(got, res[1].non_null, res[2].sum_i)
        assert (r.sum_i, r.sum_f) == (res[2].sum_i, float(res[2].sum_i))  # the plain SUM(col) of the scan
    return st, plan, want


# ---- integer keys, integer sums ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, SHARE - 1, SHARE, SHARE + 1])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    check(amounts(rng, n), ints(rng.integers(-20, 20, n), mask=rng.random(n) >= 0.1))


def test_key_patterns_within_a_wave():
    rng = np.random.default_rng(1)
    n = 20_000
    check(amounts(rng, n), ints(np.full(n, 42)))                                  # the whole wave is one reduction
    check(amounts(rng, n, 0.0), ints(np.full(n, 42), mask=np.arange(n) % 3 != 0))
    check(amounts(rng, n), ints(np.arange(n) % 64 * 1_000_003))                     # 64 distinct keys in a wave
    check(amounts(rng, n), ints(np.arange(n) % 2 * 7))                              # two keys alternating
    check(amounts(rng, n), ints(np.repeat(np.arange(n // 50), 50)))                 # runs that straddle waves


def test_the_marker_value_and_the_extremes():
    rng = np.random.default_rng(2)
    k = [-1, -1, I64_MIN, I64_MAX, 0, -1, I64_MAX, -2, 1, None, -1] * 50
    _, _, want = check(amounts(rng, len(k), 0.5), ints(k))
    assert -1 in want["entries"] and 0 < want["entries"][-1][1] < want["entries"][-1][0]
    check(amounts(rng, 300), ints([-1] * 300))
    check(amounts(rng, 300, 1.0), ints([None, -1, None] * 100))


def test_integer_sums_wrap():
    rng = np.random.default_rng(3)
    n = 10_000
    big = rng.choice(np.array([I64_MAX, I64_MAX - 1, I64_MIN, I64_MIN + 1, 2**62, -2**62, 1, -1], dtype=np.int64), n)
    v, g = ints(big, mask=rng.random(n) >= 0.1), ints(rng.integers(0, 5, n), mask=rng.random(n) >= 0.1)
    check(v, g)
    true = [sum(vals) for _rows, vals in ex.group_by(v.to_pylist(), g.to_pylist()).values()]
    assert all(abs(t) >= 2**63 for t in true)  # (the true sums lie outside Int64: every group's sum has wrapped)
    check(ints(np.full(n, I64_MAX)), ints(np.full(n, 3)))   # one reduction a wave, every partial sum wraps
    check(ints(np.full(n, I64_MIN)), ints(np.arange(n) % 2))


def test_more_keys_than_a_workgroups_lds_table_holds():
    """20 000 keys over 200 000 rows: a workgroup's share of 16 384 rows holds some 11 000 keys, more than the 4096 LDS
    slots, so rows go to the global table directly"""
    rng = np.random.default_rng(4)
    n = 200_000
    keys = rng.integers(0, 20_000, n) * 1_000_003 - 5
    _, _, want = check(amounts(rng, n, 0.4, -2**40, 2**40), ints(keys), max_groups=30_000)
    assert want["groups"] > 4 * 4096


@pytest.mark.parametrize("extra", [0, 1])
def test_all_rows_distinct_at_max_groups_and_one_above(extra):
    rng = np.random.default_rng(5)
    n = 1000 + extra
    _, _, want = check(amounts(rng, n), ints(rng.permutation(n) * 7 - 3000), max_groups=1000)
    assert want["groups"] == n and want["overflow"][0] == 0  # one above: reported, the caller compares


def test_more_keys_than_the_global_table_has_slots():
    rng = np.random.default_rng(6)
    n = 30_000
    keys = rng.integers(0, 5000, n)
    v = ints(rng.choice(np.array([I64_MAX, 2**62, -5, 17], dtype=np.int64), n), mask=rng.random(n) >= 0.5)
    T.init()
    plan = plan_of((4, 256))  # 8 slots
    st = feed(plan, [[column(ints(keys)), column(v)]])
    got, true = read(st), exact(v, ints(keys))
    assert got["overflow"][0] > 0 and 0 < got["overflow"][1] < got["overflow"][0] and got["groups"] <= 8
    res = st.finalize()
    identities(got, n - v.null_count, res[2].sum_i)  # the third identity stays exact
    assert res[2].sum_i == ex.wrap(sum(x for x in v.to_pylist() if x is not None)) == res[0].sum_i
    assert all(0 < e[0] <= true["entries"][k][0] and e[1] <= true["entries"][k][1] for k, e in got["entries"].items())


NARROW = [(pa.int8(), [-128, -1, 0, 127, -1]), (pa.int16(), [-32768, -1, 32767, 5]), (pa.int32(), [-2**31, -1, 2**31 - 1, 7]),
          (pa.uint8(), [0, 255, 128]), (pa.uint16(), [0, 65535, 32768]), (pa.uint32(), [0, 2**31, 2**32 - 1, 2**31 + 1]),
          (pa.date32(), [-1, 0, 19000])]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("type,values", NARROW, ids=[str(t) for t, _ in NARROW])
def test_narrow_key_and_value_types_are_widened(type, values, mem):
    rng = np.random.default_rng(7)
    storage = pa.int32() if type == pa.date32() else type

    def narrow():
        picks = [values[i] for i in rng.integers(0, len(values), 700)]
        arr = pa.array([None if rng.random() < 0.1 else p for p in picks], type=storage)
        return arr, (arr.cast(type) if type == pa.date32() else arr)
    keys, key_col = narrow()
    vals, val_col = narrow()
    wide = amounts(rng, 700)
    check(wide, key_col, mem=mem, want=exact(wide, keys))               # a narrow key column
    g = ints(rng.integers(0, 7, 700), mask=rng.random(700) >= 0.1)
    check(val_col, g, mem=mem, want=exact(vals, g))                     # a narrow value column
    check(val_col, key_col, mem=mem, want=exact(vals, keys))            # both


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
def test_float32_values_are_widened(mem):
    rng = np.random.default_rng(8)
    n = 3000
    vals = floats(rng.integers(-500, 500, n), mask=rng.random(n) >= 0.2, type=pa.float32())
    g = ints(rng.integers(0, 9, n), mask=rng.random(n) >= 0.1)
    check(vals, g, is_float=True, mem=mem)  # small integers: exact in any order
    frac = pa.array(rng.standard_normal(n).astype(np.float32), mask=rng.random(n) < 0.2)
    check(frac, g, is_float=True, exactly=False, mem=mem)


# ---- Arrow offsets and NULL rates ---------------------------------------------------------------------------------------------
OFFSETS = [0, 1, 8, 9, 63, 64]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("goff", OFFSETS)
def test_the_two_columns_have_independent_arrow_offsets(goff, mem):
    rng = np.random.default_rng(goff)
    n, room = 3000, 64
    for voff in [o for o in OFFSETS if o != goff]:
        g = ints(rng.integers(0, 9, n + room), mask=rng.random(n + room) >= 0.3).slice(goff, n)
        check(amounts(rng, n + room, 0.5).slice(voff, n), g, mem=mem)
    s = pa.array(["k%d" % k if k else None for k in rng.integers(0, 9, n + room)], pa.string()).slice(goff, n)
    check(amounts(rng, n + room, 0.5).slice((goff + 9) % 65, n), s, mem=mem)
    d = dictionary(rng.integers(0, 5, n + room), ["a", "b", None, "d", "e"], mask=rng.random(n + room) >= 0.1).slice(goff, n)
    check(amounts(rng, n + room, 0.5).slice((goff + 9) % 65, n), d, mem=mem)


@pytest.mark.parametrize("group_nulls", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("value_nulls", [0.0, 0.5, 1.0])
def test_null_rates(value_nulls, group_nulls):
    rng = np.random.default_rng(int(value_nulls * 10 + group_nulls * 100))
    n = 3000
    g = ints(rng.integers(0, 9, n), mask=rng.random(n) >= group_nulls)
    _, _, want = check(amounts(rng, n, value_nulls).slice(0), g)
    assert want["null_group"][0] == g.null_count
    check(floats(rng.integers(-9, 9, n), mask=rng.random(n) >= value_nulls), g, is_float=True)


def test_a_value_column_without_a_validity_buffer():
    rng = np.random.default_rng(9)
    n = 5000
    v = ints(rng.integers(-100, 100, n))
    assert T.Column.from_arrow(v).c.validity is None
    g = ints(rng.integers(0, 9, n), mask=rng.random(n) >= 0.2)
    _, _, want = check(v, g)
    assert all(e[0] == e[1] for e in want["entries"].values()) and want["null_group"][1] == g.null_count
    s = pa.array(["k%d" % k for k in rng.integers(0, 9, n)], pa.string())
    check(v, s)


def test_the_value_column_is_the_group_column():
    rng = np.random.default_rng(10)
    n = 4000
    g = ints(rng.integers(-4, 9, n), mask=rng.random(n) >= 0.2)
    T.init()
    plan = T.Plan([spec(T.GROUP_SUMS, 0, column2=0), spec(T.COUNT, 0), spec(T.NUMERIC_STATS, 0)])
    plan.set_group_sums(0)
    st = feed(plan, [[column(g)]])
    got = read(st)
    assert got == exact(g, g) and all(e == (e[0], e[0], ex.wrap(k * e[0])) for k, e in got["entries"].items())
    assert got["null_group"] == (g.null_count, 0, 0)
    res = st.finalize()
    identities(got, res[1].non_null, res[2].sum_i)


# ---- float sums -------------------------------------------------------------------------------------------------------------
def test_float_sums_of_small_integers_are_exact_in_any_order():
    """|x| < 2^20 and fewer than 2^20 rows a group: every partial sum is an integer below 2^53"""
    rng = np.random.default_rng(11)
    n = 100_000
    v = floats(rng.integers(-2**20, 2**20, n), mask=rng.random(n) >= 0.2)
    check(v, ints(rng.integers(0, 40, n), mask=rng.random(n) >= 0.05), is_float=True)
    check(v, ints(np.full(n, 7)), is_float=True)
    check(v, ints(rng.integers(0, 20_000, n)), is_float=True, max_groups=30_000)  # past the LDS table
    check(v, pa.array(["k%d" % k for k in rng.integers(0, 300, n)], pa.string()), is_float=True)
    check(v, dictionary(rng.integers(0, 50, n), ["d%d" % k for k in range(50)]), is_float=True)
    check(v, dictionary(rng.integers(0, 5000, n), ["d%d" % k for k in range(5000)]), is_float=True)


@pytest.mark.parametrize("scale", [1.0, 1e-300, 1e280])
def test_general_float_sums_lie_within_the_bound_of_any_order(scale):
    """m * max|x| < 1e300: no order of additions overflows"""
    rng = np.random.default_rng(12)
    n = 60_000
    x = rng.standard_normal(n) * np.exp(rng.uniform(-20, 20, n)) * scale
    assert n * np.abs(x).max() < 1e300
    v = floats(x, mask=rng.random(n) >= 0.2)
    check(v, ints(rng.integers(0, 40, n), mask=rng.random(n) >= 0.05), is_float=True, exactly=False)
    check(v, ints(np.full(n, -3)), is_float=True, exactly=False)
    check(v, pa.array(["k%d" % k for k in rng.integers(0, 300, n)], pa.string()), is_float=True, exactly=False)
    check(v, dictionary(rng.integers(0, 50, n), ["d%d" % k for k in range(50)]), is_float=True, exactly=False)
    check(v, ints(rng.integers(0, 40, n)), is_float=True, exactly=False, cuts=8192, mem=T.MEM_HOST)


def test_nan_and_infinities_propagate_by_ieee_rules():
    inf, nan = math.inf, math.nan
    keys = [1, 1, 1, 2, 2, 3, 3, 3, 4, 4, None, None] * 40
    vals = [1.0, nan, 2.0, inf, inf, inf, -inf, 5.0, 1.5, None, -inf, 2.0] * 40
    for g in (ints(keys), pa.array([None if k is None else "k%d" % k for k in keys], pa.string())):
        st, _, want = check(pa.array(vals, pa.float64()), g, is_float=True)
        e = list(read(st)["entries"].values())
        assert e[0][2] != e[0][2] and e[1][2] == inf and e[2][2] != e[2][2] and e[3][2] == 60.0
        assert read(st)["null_group"] == (80, 80, -inf)
        r = st.finalize()[0]
        assert r.sum_f != r.sum_f and r.has_value == 1


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
    _, _, w = check(amounts(rng, 5000, 0.5), g, max_value_bytes=40, mem=mem)
    assert w["long_rows"][0] > w["long_rows"][1] > 0 and b"" in w["entries"] and b"x" * 40 in w["entries"]
    assert w["null_group"][0] > 0
    check(amounts(rng, 5003, 0.5).slice(0, 4997), g.slice(3), max_value_bytes=40, mem=mem)
    check(floats(rng.integers(-99, 99, 5000), mask=rng.random(5000) >= 0.3), g, is_float=True, max_value_bytes=40, mem=mem)


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
    v = amounts(rng, len(vals))
    st = feed(plan_of((100, 40)), [[col.sliced(0, len(vals)), column(v)]])
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
    _, _, want = check(amounts(rng, 4009, 0.5).slice(9), g, max_value_bytes=40, mem=mem)
    assert set(want["entries"]) == {b"a", b"b", b""} and want["long_rows"][0] > 0
    assert want["null_group"][0] > g.indices.null_count  # (the rows of the NULL entry are NULL-key rows too)


def test_an_index_outside_the_dictionary_is_a_null_key_row():
    rng = np.random.default_rng(16)
    n = 1000
    idx = rng.integers(-1, 4, n).astype(np.int32)  # -1 and 3 lie outside a dictionary of three entries
    v = amounts(rng, n)
    entries = T.Column.from_arrow(pa.array(["p", "q", "r"], pa.string()))
    T.init()
    g = on_device(T.Column.dict32_utf8(idx, entries))
    st = feed(plan_of(), [[g, column(v)]])
    keys = [None if i in (-1, 3) else [b"p", b"q", b"r"][i] for i in idx]
    got = read(st)
    assert got == ex.walk(v.to_pylist(), keys) and got["null_group"][0] == int(((idx == -1) | (idx == 3)).sum())
    identities(got, n - v.null_count)


def test_batches_with_different_dictionaries_unite_by_value():
    T.init()
    a = dictionary([0, 1, 1, 2], ["red", "green", "blue"])
    b = dictionary([0, 0, 1, 2, 2], ["blue", "yellow", "red"])
    va, vb = ints([1, None, 3, 4]), ints([None, 20, 30, None, 50])
    st = feed(plan_of(), [[column(a), column(va)], [column(b), column(vb)]])
    assert read(st)["entries"] == {b"blue": (3, 2, 24), b"green": (2, 1, 3), b"red": (3, 2, 51), b"yellow": (1, 1, 30)}
    identities(read(st), 6)


def test_a_dictionary_above_the_lds_cell_limit():
    """4096 entries keep their cells in LDS: 4097 and 9000 entries go through global cells, 4096 and 1000 through LDS"""
    rng = np.random.default_rng(17)
    n = 50_000
    for n_entries in (9000, 4097, 4096, 1000):
        entries = ["k%05d" % i for i in range(n_entries)]
        g = dictionary(rng.integers(0, n_entries, n), entries, mask=rng.random(n) >= 0.05)
        check(amounts(rng, n, 0.3, -2**50, 2**50), g, max_groups=30_000)


# ---- batching and the ways a state travels ---------------------------------------------------------------------------------
N_BIG = 300_000


@pytest.fixture(scope="module")
def big():
    """three group columns (integers, strings, a dictionary), an Int64 and a Float64 value column (small integers: exact)"""
    rng = np.random.default_rng(18)
    iv = ints(rng.zipf(1.3, N_BIG) % 5000 - 100, mask=rng.random(N_BIG) >= 0.05)
    sv = pa.array(["c%d" % k if k % 7 else None for k in rng.integers(0, 300, N_BIG)], pa.string())
    dv = dictionary(rng.integers(0, 50, N_BIG), ["d%d" % (k % 40) for k in range(50)], mask=rng.random(N_BIG) >= 0.02)
    va = ints(rng.integers(-2**61, 2**61, N_BIG), mask=rng.random(N_BIG) >= 0.3)  # (the sums wrap)
    vb = floats(rng.integers(-2**16, 2**16, N_BIG), mask=rng.random(N_BIG) >= 0.6)
    arrs = [iv, sv, dv, va, vb]
    return arrs, [exact(v, g, is_float=f) for g in (iv, sv, dv) for v, f in ((va, False), (vb, True))]


def big_plan(extra=()):
    plan = T.Plan([spec(T.GROUP_SUMS, v, column2=g) for g in (0, 1, 2) for v in (3, 4)] + list(extra))
    for i in range(6):
        plan.set_group_sums(i)
    return plan


def same_as(st, want):
    for i, w in enumerate(want):
        got = read(st, i)
        if i % 2:
            compare_float(got, w, True)
        else:
            assert got == w and list(got["entries"]) == list(w["entries"])


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192), (T.MEM_HOST_RETAINED, 8192),
                                      (T.MEM_HOST, [3, 8195, 8196, 200_001])])
def test_batching_independence(big, mem, cuts):
    arrs, want = big
    T.init()
    st = feed(big_plan(), cut([column(a, mem) for a in arrs], N_BIG, cuts))
    same_as(st, want)


def test_state_algebra(big):
    arrs, want = big
    T.init()
    cols = [column(a) for a in arrs]
    parts = cut(cols, N_BIG, [100_000, 200_001])
    plan = big_plan()
    # read half-way, then on
    st = feed(plan, parts[:1])
    head = [a.slice(0, 100_000) for a in arrs]
    same_as(st, [exact(v, g, is_float=f) for g in head[:3] for v, f in ((head[3], False), (head[4], True))])
    st.update(parts[1])
    st.update(parts[2])
    same_as(st, want)
    # reset and refill
    st.reset()
    assert read(st)["seen"] == 0 and read(st)["entries"] == {} and read(st)["null_group"] == (0, 0, 0)
    assert read(st, 1)["is_float"] is False  # (no rows: no kind of sum)
    st.update(cols)
    same_as(st, want)
    # merge of three states
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    same_as(states[0], want)
    # a blob round trip into a fresh state; equal states give equal bytes (the float sums here are exact in any order)
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    same_as(back, want)
    assert back.serialize() == blob == st.serialize()
    back.merge([st])
    assert read(back, 2)["entries"] == {k: (2 * e[0], 2 * e[1], ex.wrap(2 * e[2])) for k, e in want[2]["entries"].items()}
    assert read(back, 2)["null_group"][:2] == tuple(2 * c for c in want[2]["null_group"][:2])
    assert read(back, 3)["entries"] == {k: (2 * e[0], 2 * e[1], 2 * e[2]) for k, e in want[3]["entries"].items()}
    other = T.Plan([spec(T.GROUP_SUMS, v, column2=g) for g in (0, 1, 2) for v in (3, 4)])
    for i in range(6):
        other.set_group_sums(i, 10000, 255)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(other, blob)


def test_integer_and_float_states_of_one_spec_do_not_merge():
    rng = np.random.default_rng(19)
    n = 2000
    g = ints(rng.integers(0, 9, n))
    T.init()
    plan = plan_of()
    a = feed(plan, [[column(g), column(amounts(rng, n))]])
    b = feed(plan, [[column(g), column(floats(rng.integers(0, 9, n)))]])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS task 0.*different value column types"):
        a.merge([b])
    s = feed(plan, [[column(pa.array(["k%d" % k for k in rng.integers(0, 9, n)], pa.string())), column(amounts(rng, n))]])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS task 0.*different group column types"):
        a.merge([s])
    assert read(a)["seen"] == n  # (the refused merges left the state as it was)


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(big, world, device_buffers):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's sums"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    arrs, want = big
    T.init()
    whole = [column(a) for a in arrs]
    plan = big_plan(extra=[spec(T.COUNT, 3), spec(T.NUMERIC_STATS, 3)])
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
            same_as(st, want)
            results[rank] = res
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
    for res in results:
        assert res[6].total == N_BIG and res[0].non_null == res[6].non_null and res[0].sum_i == res[7].sum_i


# ---- isolation ------------------------------------------------------------------------------------------------------------------
def launches_of(plan, cols):
    st = T.State(plan)
    st.profile_enable(True)
    st.update(cols)
    st.finalize()
    return st, st.profile_get("group_sums")["launches"]


def test_the_kind_leaves_the_other_kinds_bit_for_bit(big):
    arrs, want = big
    T.init()
    cols = [column(a) for a in arrs]
    others = [spec(T.COUNT, 0), spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.COUNT, 1), spec(T.DISTINCT, 1),
              spec(T.REGEX_MATCH, 1, pattern=r"^c1\d*$"), spec(T.DISTINCT, 2), spec(T.COUNT, 3), spec(T.NUMERIC_STATS, 3),
              spec(T.GROUP_COUNTS, 3, column2=0)]

    def with_bounds(plan, at):
        plan.set_group_counts(at)
        return plan
    alone = feed(with_bounds(T.Plan(others), 8), [cols]).finalize()
    st = feed(with_bounds(big_plan(extra=others), 14), [cols])
    res = st.finalize()
    same_as(st, want)
    for got, ref in zip(res[6:], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))
    assert st.group_counts(14)[1] == {k: e[:2] for k, e in want[0]["entries"].items()}


def test_a_plan_without_the_kind_profiles_no_such_kernel(big):
    arrs, _ = big
    T.init()
    cols = [column(arrs[0]), column(arrs[3])]
    launches = []
    plans = [T.Plan([spec(T.COUNT, 0), spec(T.COUNT, 1)]), T.Plan([spec(T.GROUP_COUNTS, 1, column2=0), spec(T.COUNT, 0)]),
             T.Plan([spec(T.GROUP_SUMS, 1, column2=0), spec(T.GROUP_SUMS, 1, column2=0)])]
    plans[1].set_group_counts(0)
    plans[2].set_group_sums(0)
    plans[2].set_group_sums(1)
    for plan in plans:
        launches.append(launches_of(plan, cols)[1])
    assert launches == [0, 0, 2]  # (two specs on one group column each walk it)


def test_refused_types_are_unsupported_and_the_state_stays_usable():
    """the refused batches go to the very state that is read afterwards"""
    T.init()
    n = 1000
    plan = T.Plan([spec(T.GROUP_SUMS, 1, column2=0), spec(T.COUNT, 1)])  # (a plain SUM refuses some of the types itself)
    plan.set_group_sums(0)
    st = T.State(plan)
    v = ints(np.arange(n), mask=np.arange(n) % 4 != 0)
    g = ints(np.arange(n) % 10)
    bad_groups = [(pa.array(np.arange(n, dtype=np.float64)), "Float64"), (pa.array(np.arange(n, dtype=np.float32)), "Float32"),
                  (pa.array(np.arange(n, dtype=np.uint64)), "UInt64"), (pa.array(np.arange(n) % 2 == 0), "Boolean")]
    bad_values = [(pa.array(np.arange(n, dtype=np.uint64)), "UInt64"), (pa.array(np.arange(n) % 2 == 0), "Boolean"),
                  (pa.array(["s%d" % i for i in range(n)], pa.string()), "this type")]
    for mem in (T.MEM_HOST, T.MEM_DEVICE):
        for arr, name in bad_groups:
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*GROUP_SUMS groups by.*" + name):
                st.update([column(arr, mem), column(v, mem)])
        for arr, name in bad_values:
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*GROUP_SUMS sums.*" + name):
                st.update([column(g, mem), column(arr, mem)])
        nested = T.Column.validity_only(pa.array([[1]] * n, pa.list_(pa.int64())))
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*GROUP_SUMS.*validity-only"):
            st.update([column(nested, mem), column(v, mem)])
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*GROUP_SUMS.*validity-only"):
            st.update([column(g, mem), column(nested, mem)])
    assert read(st)["seen"] == 0
    st.update([column(g), column(v)])
    got = read(st)
    assert got["seen"] == n and {k: e[0] for k, e in got["entries"].items()} == {k: 100 for k in range(10)}
    assert got == exact(v, g)
    identities(got, 750)


# ---- end to end: CrossTableSumConstraint through ValidationSuite.run(.., tables=..) ----------------------------------------------
import term_amd.suite as S  # noqa: E402
from test_exact_group_sums import golden_cases, golden_side  # noqa: E402

ARROW = {"int64": pa.int64(), "int32": pa.int32(), "float64": pa.float64(), "string": pa.string()}


def run_constraint(constraint, tables, table=None):
    """(status of the constraint, its metric, its message) of a one-constraint suite"""
    suite = S.ValidationSuite.builder("s").check(S.Check.builder("c").level(S.Level.ERROR).constraint(constraint).build())
    r = suite.build().run(table, tables=tables)
    m = r.report.metrics
    assert m.total_checks == 1 and m.passed_checks + m.failed_checks == 1
    metric = m.custom_metrics.get("c.cross_table_sum")
    if m.passed_checks:
        assert r.is_success() and not r.report.issues
        return "success", metric, None
    assert r.is_failure() and len(r.report.issues) == 1 and r.report.issues[0].constraint_name == "cross_table_sum"
    message = r.report.issues[0].message
    return ("error" if message.startswith("Error evaluating constraint: ") else "failure"), metric, message


def same_verdict(got, want):
    assert got == (want["status"], want["metric"], want["message"])


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_the_golden_vectors_through_the_suite(case):
    T.init()
    tables = {}
    for side in (case["left"], case["right"]):
        tables[side["table"]] = pa.table({name: pa.array(values, ARROW[kind]) for name, (kind, values) in side["columns"].items()})
    c = S.CrossTableSumConstraint("%s.%s" % (case["left"]["table"], case["left"]["column"]),
                                  "%s.%s" % (case["right"]["table"], case["right"]["column"]))
    c.group_by(case["group_by"]).tolerance(case["tolerance"]).max_violations_reported(case.get("max_violations_reported", 100))
    want = case["expect"]
    same_verdict(run_constraint(c, tables), dict(want, metric=want["max_difference"]))


@pytest.fixture(scope="module")
def two_tables():
    """orders and payments of a few hundred thousand rows: integer amounts per customer (some customers on one side only,
    NULL customers on both, NULL amounts), payments split into instalments; every fiftieth customer is short-paid"""
    rng = np.random.default_rng(20)
    n_orders, customers = 300_000, 20_000
    cust = rng.integers(0, customers, n_orders)
    total = rng.integers(1, 10**12, n_orders)
    o_cust = ints(cust, mask=rng.random(n_orders) >= 0.01)
    o_total = ints(total, mask=rng.random(n_orders) >= 0.02)
    # payments: every order's total in two instalments, for the customers that pay; customers >= 19 900 never pay
    pays = (cust < 19_900) & np.asarray(o_total.is_valid()) & np.asarray(o_cust.is_valid())
    first = total[pays] // 3
    short = np.where(cust[pays] % 50 == 0, 1, 0)  # a unit short on the second instalment
    p_cust = np.concatenate([cust[pays], cust[pays], rng.integers(30_000, 30_100, 500)])
    p_amount = np.concatenate([first, total[pays] - first - short, rng.integers(1, 100, 500)])
    order = rng.permutation(len(p_cust))
    p_mask = rng.random(len(p_cust)) >= 0.001
    orders = pa.table({"customer_id": o_cust, "total": o_total, "region": pa.array(["r%d" % (c % 97) for c in cust], pa.string())})
    payments = pa.table({"customer_id": ints(p_cust[order], mask=p_mask[order]), "amount": ints(p_amount[order]),
                         "region": pa.array(["r%d" % (c % 97) for c in p_cust[order]], pa.string())})
    return {"orders": orders, "payments": payments}


def exact_verdict(tables, group, is_float=False, left="total", right="amount", **kw):
    sides = []
    for name, col in (("orders", left), ("payments", right)):
        t = tables[name]
        groups = None if group is None else as_exact(t[group].to_pylist())
        sides.append(ex.side_sums(t[col].to_pylist(), groups, is_float))
    return ex.cross_table_sum(sides[0], sides[1], group_by_columns=[group] if group else [], left_name="orders." + left,
                              right_name="payments." + right, **kw)


@pytest.mark.parametrize("group", ["customer_id", "region"])
def test_two_tables_with_integer_values(two_tables, group):
    T.init()
    c = S.CrossTableSumConstraint("orders.total", "payments.amount").group_by([group])
    want = exact_verdict(two_tables, group)
    assert want["status"] == "failure" and want["violating_groups"] > 0 and want["total_groups"] > 90
    # the message carries total_groups, violating_groups and both totals (shortest digits: the doubles themselves), the
    # metric is max_difference
    same_verdict(run_constraint(c, two_tables), want)
    loose = exact_verdict(two_tables, group, tolerance=1e16)
    assert loose["status"] == "success"
    same_verdict(run_constraint(c.tolerance(1e16), two_tables), loose)


def test_the_suites_own_table_rides_its_fused_plan_beside_the_constraint(two_tables):
    T.init()
    check = S.Check.builder("c").level(S.Level.ERROR).has_size(S.Assertion.Equals(300_000)) \
        .cross_table_sum("orders.total", "payments.amount").build()
    r = S.ValidationSuite.builder("s").table_name("orders").check(check).build() \
        .run(two_tables["orders"], tables={"payments": two_tables["payments"]})
    want = exact_verdict(two_tables, None)
    assert r.report.metrics.passed_checks == 1 and [i.message for i in r.report.issues] == [want["message"]]
    assert r.report.metrics.custom_metrics["c.cross_table_sum"] == want["metric"]
    # without `tables` nothing changes for a suite of one table
    alone = S.ValidationSuite.builder("s").table_name("orders").check(
        S.Check.builder("c").has_size(S.Assertion.Equals(300_000)).build()).build()
    assert alone.run(two_tables["orders"]).report.metrics.passed_checks == 1
    assert alone.run(two_tables["orders"], tables={}).report.metrics.passed_checks == 1


def test_the_ungrouped_form(two_tables):
    T.init()
    c = S.CrossTableSumConstraint("orders.total", "payments.amount")
    want = exact_verdict(two_tables, None)
    assert want["status"] == "failure" and "Group 'ALL'" in want["message"]
    same_verdict(run_constraint(c, two_tables), want)
    same_verdict(run_constraint(c.max_violations_reported(0), two_tables), exact_verdict(two_tables, None, max_violations_reported=0))
    same = S.CrossTableSumConstraint("orders.total", "orders.total")  # a table against itself
    assert run_constraint(same, two_tables) == ("success", 0.0, None)


def test_float_values_with_a_tolerance_far_from_every_difference():
    """every group's difference is 0 (the same values in another order) or at least 1000; the tolerance is 1: no summation
    order moves a group across it (the values are below 1e6, 2000 a group: an error below 1e-6)"""
    rng = np.random.default_rng(21)
    n = 200_000
    g = rng.integers(0, 100, n)
    x = rng.random(n) * 1e6
    perm = rng.permutation(n)
    y = x[perm].copy()
    gy = g[perm]
    bad = np.flatnonzero(gy % 10 == 3)[::50]
    y[bad] += 1000.0
    tables = {"orders": pa.table({"g": ints(g), "total": floats(x)}), "payments": pa.table({"g": ints(gy), "amount": floats(y)})}
    T.init()
    want = exact_verdict(tables, "g", is_float=True, tolerance=1.0)
    assert (want["status"], want["total_groups"], want["violating_groups"]) == ("failure", 100, 10)
    status, metric, message = run_constraint(S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(["g"]).tolerance(1.0),
                                             tables)
    assert status == "failure" and message.startswith("Cross-table sum mismatch: 10/100 groups by [g] failed validation "
                                                      "(tolerance: 1.0000), total sums: ")
    assert abs(metric - want["max_difference"]) < 1e-3
    y[bad] -= 1000.0
    tables["payments"] = pa.table({"g": ints(gy), "amount": floats(y)})
    status, metric, message = run_constraint(S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(["g"]).tolerance(1.0),
                                             tables)
    assert (status, message) == ("success", None) and 0.0 <= metric < 1e-3


def test_overflow_is_an_error_that_names_the_bound(two_tables):
    T.init()
    c = S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(["customer_id"]).max_groups(1000)
    status, metric, message = run_constraint(c, two_tables)
    assert status == "error" and metric is None
    assert "'cross_table_sum': the left side has more groups than the bound max_groups = 1000" in message
    assert " 0 overflow rows" not in message
    long_keys = {"orders": pa.table({"g": pa.array(["x" * 257, "a"], pa.string()), "total": ints([1, 2])}),
                 "payments": pa.table({"g": pa.array(["a"], pa.string()), "amount": ints([2])})}
    status, _, message = run_constraint(S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(["g"]), long_keys)
    assert status == "error" and "1 rows with a longer key" in message


def test_key_kinds_and_refused_types_are_the_constraints_errors():
    T.init()
    mixed = {"orders": pa.table({"g": ints([1, 2]), "total": ints([1, 2])}),
             "payments": pa.table({"g": pa.array(["1", "2"], pa.string()), "amount": ints([1, 2])})}
    status, _, message = run_constraint(S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(["g"]), mixed)
    assert status == "error" and "must both be integer or both be string columns" in message
    floats_as_keys = {"orders": pa.table({"g": floats([1.0, 2.0]), "total": ints([1, 2])}),
                      "payments": pa.table({"g": floats([1.0]), "amount": ints([1])})}
    status, _, message = run_constraint(S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(["g"]),
                                        floats_as_keys)
    assert status == "error" and "Cross-table sum validation query failed: TGX_UNSUPPORTED" in message
    assert "GROUP_SUMS groups by integer and string columns, not Float64" in message
