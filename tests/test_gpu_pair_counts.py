"""TGX_CHECK_PAIR_COUNTS on the device, held against tests/exact_pair_counts.py: the whole (x cell, y cell) -> count map
and all eight counters are compared for equality with the exact per-row walk -- at the wave and workgroup edges, on every
string layout on either side, through the workgroups' LDS tables and their direct-to-global path, in both phases of a
mixed pair, and on every way a state travels (ragged cuts, HOST batches, merge, blob)."""
import numpy as np
import pyarrow as pa
import pytest

import exact_joint as ej
import exact_pair_counts as ex
import fp_reference as F
import term_amd as T
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

KEY = bytes(range(0x30, 0x40))
LDS_SLOTS = 1024      # pairs one workgroup's LDS table holds
SHARE = 256 * 16      # rows a workgroup takes before a second one is launched


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
    col = T.Column.from_arrow(arr)
    if mem == T.MEM_DEVICE:
        return on_device(col)
    col.c.mem = mem
    return col


def cut(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def plan_of(x=None, y=None, max_pairs=10000, max_value_bytes=256, columns=(0, 1), extra=(), key=None):
    plan = T.Plan([spec(T.PAIR_COUNTS, columns[0], column2=columns[1])] + list(extra), fingerprint_key=key)
    plan.set_pair_counts(0, x=x, y=y, max_pairs=max_pairs, max_value_bytes=max_value_bytes)
    return plan


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def read(st, i=0):
    summary, counts = st.pair_counts(i)
    return dict(summary, counts=counts)


def same(got, want):
    """every counter, every entry and the order of the entries"""
    assert got == want and list(got["counts"]) == list(want["counts"])


def check(xa, ya, x=None, y=None, max_pairs=10000, max_value_bytes=256, mem=T.MEM_DEVICE, cuts=None, want=None):
    T.init()
    if want is None:
        want = ex.walk(xa.to_pylist(), ya.to_pylist(), x, y, max_value_bytes)
    plan = plan_of(x, y, max_pairs, max_value_bytes)
    st = feed(plan, cut([column(xa, mem), column(ya, mem)], len(xa), cuts))
    same(read(st), want)
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.distinct, r.matches) == (want["seen"], want["both_non_null"], want["distinct"], want["counted"])
    return st, plan, want


def strs(values, type=pa.string()):
    return pa.array(values, type=type)


def pick(rng, words, n, null=0.1):
    return [None if rng.random() < null else words[i] for i in rng.integers(0, len(words), n)]


# ---- row counts, validity, offsets --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    check(strs(pick(rng, ["a", "b", "", "cc"], n)), strs(pick(rng, ["u", "v", "a"], n)))


def test_one_side_all_null_and_no_validity_buffer():
    rng = np.random.default_rng(1)
    n = 300
    some = strs(pick(rng, ["a", "b"], n))
    nothing = pa.array([None] * n, pa.string())
    _, _, want = check(some, nothing)
    assert want["both_non_null"] == 0 and want["counts"] == {}
    check(nothing, some)
    plain = strs(pick(rng, ["a", "b", "c"], n, null=0.0))
    assert plain.null_count == 0 and plain.buffers()[0] is None
    _, _, want = check(plain, strs(pick(rng, ["u", "v"], n, null=0.0)))
    assert want["both_non_null"] == n


@pytest.mark.parametrize("xoff,yoff", [(3, 0), (0, 5), (9, 8), (1, 1)])
def test_sliced_columns(xoff, yoff):
    rng = np.random.default_rng(xoff * 10 + yoff)
    n = 700
    xa = strs(pick(rng, ["a", "bb", "", "c"], n + xoff)).slice(xoff)
    ya = strs(pick(rng, ["u", "v", "ww"], n + yoff)).slice(yoff)
    check(xa, ya)
    check(xa, ya, mem=T.MEM_HOST)


# ---- keys -------------------------------------------------------------------------------------------------------------------
def test_pairs_are_not_concatenations_of_their_bytes():
    xa = strs(["ab", "a", "", "x", "ab", ""] * 50)
    ya = strs(["c", "bc", "x", "", "c", ""] * 50)
    _, _, want = check(xa, ya)
    assert want["counts"] == {(b"", b""): 50, (b"", b"x"): 50, (b"a", b"bc"): 50, (b"ab", b"c"): 100, (b"x", b""): 50}


def test_the_same_column_on_both_sides():
    rng = np.random.default_rng(2)
    vals = pick(rng, ["a", "b", "", "long enough to leave the view"], 500)
    T.init()
    plan = plan_of(columns=(0, 0))
    st = feed(plan, [[column(strs(vals))]])
    want = ex.walk(vals, vals)
    same(read(st), want)
    assert all(x == y for x, y in want["counts"])


@pytest.mark.parametrize("type", [pa.string(), pa.string_view()], ids=str)
def test_values_of_exactly_max_value_bytes_and_one_more(type):
    """either side and both; the longer values give long rows; lengths 15 / 16 / 17 / 32 / 33 straddle the fingerprint's
    blocks"""
    rng = np.random.default_rng(3)
    words = ["", "x", "x" * 15, "x" * 16, "x" * 17, "x" * 32, "x" * 33, "y" * 40, "z" * 41]
    n = 2000
    xs, ys = pick(rng, words, n), pick(rng, words, n)
    _, _, want = check(strs(xs, type), strs(ys), max_value_bytes=40)
    assert want["long_rows"] == sum(1 for a, b in zip(xs, ys) if a is not None and b is not None and 41 in (len(a), len(b)))
    assert (b"y" * 40, b"y" * 40) in want["counts"] and want["long_rows"] > 0
    assert any(a == "z" * 41 and b == "z" * 41 for a, b in zip(xs, ys))


# ---- wave combining -------------------------------------------------------------------------------------------------------
def test_wave_combining():
    n = 64 * 40
    i = np.arange(n)
    const = ["k"] * n
    check(strs(const), strs(const))                                            # a constant pair: one insert per wave
    check(strs(["a" if k % 2 else "b" for k in i]), strs(const))             # two pairs alternating
    check(strs(["v%d" % (k % 6) for k in i]), strs(const))                   # six pairs in every wave: beyond the four rounds
    _, _, want = check(strs(["once" if k % 64 == 17 else "k" for k in i]), strs(const))  # a pair that occurs once per wave
    assert want["counts"][(b"once", b"k")] == 40


# ---- table edges ------------------------------------------------------------------------------------------------------------
def test_more_pairs_than_a_workgroups_lds_table_holds():
    """3000 distinct pairs in 20 000 rows: five workgroups of 4096 rows, each with more than twice the pairs its 1024 LDS
    slots hold, so leaders go to the global table directly; nothing overflows"""
    rng = np.random.default_rng(4)
    k = rng.integers(0, 3000, 20_000)
    assert 20_000 // SHARE + 1 == 5
    _, _, want = check(strs(["x%d" % (v % 60) for v in k]), strs(["y%d" % (v // 60) for v in k]))
    assert want["distinct"] > 2 * LDS_SLOTS and want["overflow_rows"] == 0


def test_more_pairs_than_the_global_table_has_slots():
    rng = np.random.default_rng(5)
    k = rng.integers(0, 40, 6000)
    xs, ys = ["x%d" % (v % 8) for v in k], ["y%d" % (v // 8) for v in k]
    T.init()
    st = feed(plan_of(max_pairs=4), [[column(strs(xs)), column(strs(ys))]])  # 8 slots
    got, true = read(st), ex.walk(xs, ys)
    assert true["distinct"] == 40 and got["overflow_rows"] > 0 and 0 < got["distinct"] <= 8
    assert got["counted"] + got["overflow_rows"] + got["long_rows"] + got["non_finite"] + got["out_of_range"] == \
        got["both_non_null"] == 6000
    assert got["counted"] == sum(got["counts"].values())
    assert all(c == true["counts"][p] for p, c in got["counts"].items())  # every entry that is held: its exact count


def test_the_largest_table_is_accepted():
    rng = np.random.default_rng(6)
    check(strs(pick(rng, ["a", "b"], 500)), strs(pick(rng, ["u", "v"], 500)), max_pairs=65536)


# ---- layouts ----------------------------------------------------------------------------------------------------------------
WORDS = ["", "a", "twelve bytes", "thirteen byte", "a value that lies outside the view", "Zoë", "a\x00b"]


def dictionary(indices, entries, mask=None):
    return pa.DictionaryArray.from_arrays(pa.array(indices, pa.int32(), mask=None if mask is None else ~np.asarray(mask)),
                                          pa.array(entries, pa.string()))


def layouts(rng, n):
    vals = pick(rng, WORDS, n)
    entries = ["a", None, "b", "a", "unused", "", "twelve bytes", "b"]  # 0 and 3, 2 and 7 repeat a value; 1 is NULL
    idx = rng.choice([0, 1, 2, 3, 5, 6, 7], n)
    return [strs(vals), strs(vals, pa.large_string()), strs(vals, pa.string_view()),
            dictionary(idx, entries, mask=rng.random(n) >= 0.1)]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("layout", range(4), ids=["utf8", "large_utf8", "utf8_view", "dictionary"])
def test_every_layout_on_either_side(layout, mem):
    rng = np.random.default_rng(7 + layout)
    n = 1500
    side = layouts(rng, n)[layout]
    other = strs(pick(rng, ["u", "v", "", "a value that lies outside the view"], n))
    _, _, want = check(side, other, mem=mem)
    assert want["distinct"] > 4
    check(other, side, mem=mem)
    check(side.slice(5), other.slice(5), mem=mem)


def test_a_dictionary_index_outside_the_dictionary_is_a_null_row():
    T.init()
    entries = pa.array(["a", None, "b", "a"], pa.string())
    idx = [0, 1, 2, 3, 4, -1, 2, 1000, 0, None]
    arr = pa.DictionaryArray.from_arrays(pa.array(idx, pa.int32()), entries, safe=False)
    ys = ["u"] * len(idx)
    values = ["a", None, "b", "a", None, None, "b", None, "a", None]  # what the rows hold: NULL entry, outside, NULL row
    for cols, want in (([column(arr), column(strs(ys))], ex.walk(values, ys)),
                       ([column(strs(ys)), column(arr)], ex.walk(ys, values))):
        st = feed(plan_of(), [cols])
        same(read(st), want)
        assert want["both_non_null"] == 5


def test_batches_with_different_dictionaries_unite_by_value():
    T.init()
    a = dictionary([0, 1, 1, 2], ["red", "green", "blue"])
    b = dictionary([0, 0, 1, 2, 2], ["blue", "yellow", "red"])
    ya, yb = strs(["s", "s", "t", "s"]), strs(["s", "t", "s", "s", "s"])
    st = feed(plan_of(), [[column(a), column(ya)], [column(b), column(yb)]])
    same(read(st), ex.walk(a.to_pylist() + b.to_pylist(), ya.to_pylist() + yb.to_pylist()))
    assert read(st)["counts"][(b"red", b"s")] == 3


# ---- mixed pairs: a numeric side in two phases ------------------------------------------------------------------------------
def mixed(num, cat, num_is_x, bins, mem=T.MEM_DEVICE, count_num=None, count_cat=None):
    """both phases as the analyzer runs them: the range of the numeric side, the binning from it, the count; returns
    (range, binning, counts read)"""
    T.init()
    nums, cats = num.to_pylist(), cat.to_pylist()
    cols = [column(num, mem), column(cat, mem)] if num_is_x else [column(cat, mem), column(num, mem)]
    first = plan_of(x="range" if num_is_x else None, y=None if num_is_x else "range")
    st = feed(first, [cols])
    rng = st.pair_range(0)
    want = ex.side_range(nums, cats)
    assert {k: rng[k] for k in ("seen", "both_non_null", "n", "non_finite")} == {k: want[k] for k in ("seen", "both_non_null", "n", "non_finite")}
    if want["n"] == 0:
        assert rng["min"] != rng["min"] and rng["max"] != rng["max"]
        return rng, None, None
    assert (rng["min"], rng["max"]) == (want["min"], want["max"])
    assert read(st)["counts"] == {} and read(st)["both_non_null"] == want["both_non_null"]
    binning = (rng["min"], ej.bin_width(rng["min"], rng["max"], bins), bins)
    assert binning == ex.binning_of(nums, cats, bins)
    if count_num is not None:  # the count pass over another table
        num, cat = count_num, count_cat
        nums, cats = num.to_pylist(), cat.to_pylist()
        cols = [column(num, mem), column(cat, mem)] if num_is_x else [column(cat, mem), column(num, mem)]
    second = plan_of(x=binning if num_is_x else None, y=None if num_is_x else binning)
    st = feed(second, [cols])
    got = read(st)
    same(got, ex.walk(nums, cats, binning, None) if num_is_x else ex.walk(cats, nums, None, binning))
    return rng, binning, got


NUMERIC = [(pa.int64(), lambda rng, n: rng.integers(-1000, 1000, n)), (pa.float64(), lambda rng, n: rng.normal(0, 50, n)),
           (pa.int16(), lambda rng, n: rng.integers(-300, 300, n)), (pa.float32(), lambda rng, n: rng.normal(0, 5, n).astype(np.float32))]


@pytest.mark.parametrize("num_is_x", [True, False], ids=["numeric_x", "numeric_y"])
@pytest.mark.parametrize("type,draw", NUMERIC, ids=[str(t) for t, _ in NUMERIC])
def test_a_numeric_side_in_both_phases(type, draw, num_is_x):
    rng = np.random.default_rng(11)
    n = 3000
    num = pa.array(draw(rng, n), type=type, mask=rng.random(n) < 0.1)
    cat = strs(pick(rng, ["a", "b", "", "c"], n))
    _, binning, got = mixed(num, cat, num_is_x, 10)
    side = 0 if num_is_x else 1
    assert max(p[side] for p in got["counts"]) == 10  # the row at the maximum lands in bin `bins`
    assert got["out_of_range"] == 0 and got["non_finite"] == 0
    mixed(num.slice(7), cat.slice(7), num_is_x, 10, mem=T.MEM_HOST)


def test_a_constant_column_gives_width_one():
    num = pa.array([4] * 200, pa.int64())
    _, binning, got = mixed(num, strs(["a", "b"] * 100), True, 10)
    assert binning == (4.0, 1.0, 10) and got["counts"] == {(0, b"a"): 100, (0, b"b"): 100}


def test_non_finite_rows_and_an_all_null_numeric_side():
    rng = np.random.default_rng(12)
    n = 1000
    v = rng.normal(0, 1, n)
    v[::7] = np.nan
    v[3::50] = np.inf
    v[4::60] = -np.inf
    num = pa.array(v, pa.float64(), mask=rng.random(n) < 0.1)
    r, _, got = mixed(num, strs(pick(rng, ["a", "b"], n)), False, 5)
    assert r["non_finite"] > 100 and got["non_finite"] == r["non_finite"] and got["both_non_null"] == r["both_non_null"]
    mixed(pa.array([None] * 100, pa.float64()), strs(["a"] * 100), True, 5)


def test_a_count_pass_over_a_table_that_grew():
    rng = np.random.default_rng(13)
    n = 1000
    cat = strs(pick(rng, ["a", "b"], n, null=0.0))
    first = pa.array(rng.integers(0, 100, n), pa.int64())
    grown = pa.array(np.concatenate([rng.integers(0, 100, n - 20), rng.integers(500, 900, 10), rng.integers(-90, -1, 10)]), pa.int64())
    _, _, got = mixed(first, cat, True, 10, count_num=grown, count_cat=cat)
    assert got["out_of_range"] == 20


# ---- routes: one table five ways --------------------------------------------------------------------------------------------
N_ROUTES = 5000


@pytest.fixture(scope="module")
def table():
    rng = np.random.default_rng(14)
    entries = ["d%d" % (k % 30) for k in range(40)]
    xa = dictionary(rng.integers(0, 40, N_ROUTES), entries, mask=rng.random(N_ROUTES) >= 0.05)
    ya = strs(["c%d" % k if k % 11 else None for k in rng.integers(0, 50, N_ROUTES)], pa.string_view())
    za = pa.array(rng.normal(10, 3, N_ROUTES), pa.float64(), mask=rng.random(N_ROUTES) < 0.05)
    zb = ex.binning_of(za.to_pylist(), ya.to_pylist(), 10)
    want = [ex.walk(xa.to_pylist(), ya.to_pylist()), ex.walk(za.to_pylist(), ya.to_pylist(), zb, None)]
    return [xa, ya, za], zb, want


def routes_plan(zb, extra=()):
    plan = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1), spec(T.PAIR_COUNTS, 2, column2=1)] + list(extra), fingerprint_key=KEY)
    plan.set_pair_counts(0)
    plan.set_pair_counts(1, x=zb)
    return plan


def test_five_routes_give_identical_entries(table):
    arrs, zb, want = table
    T.init()
    plan = routes_plan(zb)
    dev = [column(a) for a in arrs]
    host = [column(a, T.MEM_HOST) for a in arrs]
    one = feed(plan, [dev])
    ragged = feed(plan, cut(dev, N_ROUTES, [1, 64, 65, 257, 4097]))
    hosted = feed(plan, cut(host, N_ROUTES, 1024))
    halves = [feed(plan, [p]) for p in cut(dev, N_ROUTES, [2001])]
    halves[0].merge(halves[1:])
    blob = one.serialize()
    back = T.State.deserialize(plan, blob)
    for st in (one, ragged, hosted, halves[0], back):
        for i in range(2):
            same(read(st, i), want[i])
        assert st.serialize() == blob  # equal states, equal bytes
    back.merge([one])
    assert read(back, 0)["counts"] == {p: 2 * c for p, c in want[0]["counts"].items()}
    one.reset()
    assert read(one, 0)["seen"] == 0 and read(one, 0)["counts"] == {} and read(one, 1)["counts"] == {}
    one.update(dev)
    same(read(one, 1), want[1])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(routes_plan((zb[0], zb[1], 11)), blob)


def test_the_kind_leaves_the_other_kinds_bit_for_bit(table):
    import ctypes

    arrs, zb, want = table
    T.init()
    cols = [column(a) for a in arrs]
    others = [spec(T.COUNT, 0), spec(T.DISTINCT, 1), spec(T.NUMERIC_STATS, 2), spec(T.DISTINCT, 0, columns=[0, 1])]
    alone = feed(T.Plan(others, fingerprint_key=KEY), [cols]).finalize()
    st = feed(routes_plan(zb, extra=others), [cols])
    res = st.finalize()
    same(read(st, 0), want[0])
    for got, ref in zip(res[2:], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))
    assert res[5].distinct >= want[0]["distinct"]  # (the tuple DISTINCT counts NULL components as values too)


def test_profile_kernel_names(table):
    arrs, zb, _ = table
    T.init()
    cols = [column(a) for a in arrs]
    ranged = T.Plan([spec(T.PAIR_COUNTS, 2, column2=1)])
    ranged.set_pair_counts(0, x="range")
    seen = []
    for plan in (T.Plan([spec(T.COUNT, 0)]), routes_plan(zb), ranged):
        st = T.State(plan)
        st.profile_enable(True)
        st.update(cols)
        st.finalize()
        seen.append((st.profile_get("pair_counts")["launches"], st.profile_get("pair_range")["launches"]))
    assert seen == [(0, 0), (2, 0), (0, 1)]


# ---- fingerprint collisions ---------------------------------------------------------------------------------------------------
def test_colliding_pairs_unite_by_their_bytes_across_states():
    """two distinct x values with one fingerprint under the plan's key, beside one y: the two pairs have one pair key.
    Each state holds one of them; the merge, which unites by bytes, holds both"""
    rng = np.random.default_rng(15)
    a, b = F.colliding_pair(KEY, rng)
    assert F.tuple_fingerprint(KEY, [a, b"y"]) == F.tuple_fingerprint(KEY, [b, b"y"])
    assert F.tuple_fingerprint(KEY, [b"ab", b"c"]) != F.tuple_fingerprint(KEY, [b"a", b"bc"])
    T.init()
    plan = plan_of(key=KEY)
    ys = strs(["y"] * 3)
    sa = feed(plan, [[column(pa.array([a] * 3, pa.binary())), column(ys)]])
    sb = feed(plan, [[column(pa.array([b] * 3, pa.binary())), column(ys)]])
    assert read(sa)["counts"] == {(a, b"y"): 3} and read(sb)["counts"] == {(b, b"y"): 3}
    sa.merge([sb])
    assert read(sa)["counts"] == dict(sorted({(a, b"y"): 3, (b, b"y"): 3}.items())) and read(sa)["distinct"] == 2


# ---- types ----------------------------------------------------------------------------------------------------------------------
def test_other_column_types_are_unsupported_and_the_state_stays_usable():
    T.init()
    n = 500
    good = strs(["a", "b"] * (n // 2))
    st = T.State(plan_of())
    binned = T.State(plan_of(x=(0.0, 1.0, 10)))
    for arr in (pa.array(np.arange(n, dtype=np.uint64)), pa.array(np.arange(n) % 2 == 0), pa.array(np.arange(n, dtype=np.int64))):
        for mem in (T.MEM_HOST, T.MEM_DEVICE):
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*PAIR_COUNTS"):
                st.update([column(arr, mem), column(good, mem)])
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*PAIR_COUNTS"):
                st.update([column(good, mem), column(arr, mem)])
    for arr in (pa.array(np.arange(n, dtype=np.uint64)), pa.array(np.arange(n) % 2 == 0), good):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*PAIR_COUNTS"):
            binned.update([column(arr), column(good)])
    assert read(st)["seen"] == 0 and read(binned)["seen"] == 0
    st.update([column(good), column(good)])
    assert read(st)["counts"] == {(b"a", b"a"): n // 2, (b"b", b"b"): n // 2}
    binned.update([column(pa.array(np.arange(n) % 10, pa.int32())), column(good)])
    assert read(binned)["counted"] == n and read(binned)["distinct"] == 10


# ---- MutualInformationAnalyzer through AnalysisRunner.run -----------------------------------------------------------------------
def golden():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_counts_vectors.json")) as f:
        return json.load(f)["categorical_table"]


def check_metric(ctx, key, counts):
    exact, bound = ex.metric_bound(counts)
    got = ctx.get_metric(key)["value"]
    print("%s: %r against %r within %r" % (key, got, exact, bound))
    assert abs(got - exact) <= bound
    return got


def test_the_reference_categorical_table_through_the_runner():
    import term_amd.suite as S

    T.init()
    g = golden()
    table = pa.table({"category": strs(g["columns"]["category"]), "value": strs(g["columns"]["value"])})
    ctx = S.AnalysisRunner().add(S.MutualInformationAnalyzer("category", "value", g["bins"], max_pairs=100)).run(table)
    assert not ctx.errors()
    key = "mutual_information_category_value"
    assert ctx.states[key] == g["expect"]["state"]
    counts = ex.walk(g["columns"]["category"], g["columns"]["value"])["counts"]
    assert check_metric(ctx, key, counts) < g["expect"]["metric_below"]
    # without the opt-in the analyzer is what it was: the library's refusal is its error
    plain = S.AnalysisRunner().add(S.MutualInformationAnalyzer("category", "value", g["bins"])).run(table)
    assert [e["analyzer_name"] for e in plain.errors()] == ["mutual_information"] and "TGX_UNSUPPORTED" in plain.errors()[0]["error"]


@pytest.fixture(scope="module")
def wide():
    rng = np.random.default_rng(16)
    n = 20_000
    k = rng.integers(0, 12, n)
    s = strs([None if v % 13 == 0 else "s%d" % (v % 5) for v in rng.integers(0, 100, n)])
    lg = strs(["cat-%d" % (v // 2) for v in k], pa.large_string())
    d = dictionary(k % 7, ["d%d" % i for i in range(7)], mask=rng.random(n) >= 0.03)
    a = pa.array(k * 1.5 + rng.normal(0, 1, n), pa.float64(), mask=rng.random(n) < 0.02)
    b = pa.array(rng.integers(0, 50, n), pa.int64())
    return pa.table({"s": s, "lg": lg, "d": d, "a": a, "b": b})


def test_three_layouts_beside_other_analyzers(wide):
    import term_amd.suite as S

    T.init()
    pairs = [("s", "lg"), ("d", "s"), ("lg", "d")]
    runner = S.AnalysisRunner().add(S.SizeAnalyzer()).add(S.MutualInformationAnalyzer("a", "b", 8))
    for x, y in pairs:
        runner.add(S.MutualInformationAnalyzer(x, y, 10, max_pairs=1000))
    ctx = runner.run(wide)
    assert not ctx.errors()
    alone = S.AnalysisRunner().add(S.SizeAnalyzer()).add(S.MutualInformationAnalyzer("a", "b", 8)).run(wide)
    for key in ("size", "mutual_information_a_b"):
        assert ctx.get_metric(key) == alone.get_metric(key) and ctx.states[key] == alone.states[key]
    for x, y in pairs:
        counts = ex.walk(wide[x].to_pylist(), wide[y].to_pylist())["counts"]
        key = "mutual_information_%s_%s" % (x, y)
        assert ctx.states[key] == ex.analyzer_state(counts, 10)
        assert list(map(tuple, ctx.states[key]["joint_counts"])) == [(a.decode(), b.decode(), c) for (a, b), c in counts.items()]
        check_metric(ctx, key, counts)


@pytest.mark.parametrize("x,y", [("a", "s"), ("d", "b")])
def test_a_mixed_pair_through_both_passes(wide, x, y):
    import term_amd.suite as S

    T.init()
    ctx = S.AnalysisRunner().add(S.MutualInformationAnalyzer(x, y, 6, max_pairs=500)).add(S.MutualInformationAnalyzer("a", "b", 8)).run(wide)
    assert not ctx.errors()
    xs, ys = wide[x].to_pylist(), wide[y].to_pylist()
    num_is_x = x in ("a", "b")
    binning = ex.binning_of(xs, ys, 6) if num_is_x else ex.binning_of(ys, xs, 6)
    counts = (ex.walk(xs, ys, binning, None) if num_is_x else ex.walk(xs, ys, None, binning))["counts"]
    key = "mutual_information_%s_%s" % (x, y)
    assert ctx.states[key] == ex.analyzer_state(counts, 6)
    check_metric(ctx, key, counts)
    assert "mutual_information_a_b" in ctx.metrics


def test_the_analyzers_own_errors_leave_the_others_answering(wide):
    import term_amd.suite as S

    T.init()
    n = wide.num_rows
    table = wide.append_column("long", strs(["x" * (9 if i == 77 else 3) for i in range(n)]))
    table = table.append_column("numberish", strs(["k%d" % (i % 4) if i != 5 else " 1e5 " for i in range(n)]))
    table = table.append_column("bin", pa.array([b"ab"] * n, pa.binary()))
    runner = S.AnalysisRunner().add(S.SizeAnalyzer())
    runner.add(S.MutualInformationAnalyzer("s", "lg", 10, max_pairs=10))                    # 30 pairs
    runner.add(S.MutualInformationAnalyzer("long", "s", 10, max_pairs=100, max_value_bytes=8))
    runner.add(S.MutualInformationAnalyzer("s", "numberish", 10, max_pairs=100))
    runner.add(S.MutualInformationAnalyzer("bin", "s", 10, max_pairs=100))
    runner.add(S.MutualInformationAnalyzer("d", "s", 10, max_pairs=100))
    ctx = runner.run(table)
    errors = [e["error"] for e in ctx.errors()]
    assert [e["analyzer_name"] for e in ctx.errors()] == ["mutual_information"] * 4
    assert "30 distinct pairs (max_pairs 10)" in errors[0] or "(max_pairs 10)" in errors[0] and "overflow rows" in errors[0]
    assert "1 rows with a value longer than 8 bytes" in errors[1]
    assert "a value of numberish may parse as a number: the reference would bin this column (not on the GPU path)" in errors[2]
    assert "column 'bin' is declared Binary" in errors[3]
    assert ctx.get_metric("size")["value"] == n
    counts = ex.walk(wide["d"].to_pylist(), wide["s"].to_pylist())["counts"]
    assert ctx.states["mutual_information_d_s"] == ex.analyzer_state(counts, 10)


def test_threaded_ranks(table):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's pairs"""
    import threading

    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    arrs, zb, want = table
    T.init()
    world = 2
    whole = [column(a) for a in arrs]
    plan = routes_plan(zb, extra=[spec(T.COUNT, 0)])
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(N_ROUTES, world, rank)
            st = T.State(plan)
            comm = thread_comm(group, rank, device_buffers=True)
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
        for i in range(2):
            same(got[i], want[i])
        assert res[2].total == N_ROUTES
