"""A TGX_CHECK_KEY_PROBE spec on TUPLE keys (a column list; Plan.set_key_probe_tuples, _tuples_counted, _rows_tuples) on
the device, held against tests/exact_key_probe_tuples.py: every counter, the identity fields, `route` and the full entry
list (hash_a, hash_b, count, has_null) are compared for EQUALITY with the nested-loop reference under a set fingerprint
key, and the identities are checked on every read.  Every case but the one named overflow case has bounds above its
distinct keys, so the reference alone decides all of it."""
import functools

import numpy as np
import pyarrow as pa
import pytest

import exact_key_probe_tuples as ex
import fp_reference as fpr
import term_amd as T
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

KEY = bytes(range(1, 17))
M64 = (1 << 64) - 1
I64, I32, U8 = pa.int64(), pa.int32(), pa.uint8()
UTF8, LARGE, VIEW, DICT = pa.string(), pa.large_string(), pa.string_view(), "dictionary"


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


def array(values, typ):
    """one component's column: ints under an integer type, bytes / str under a string layout"""
    if typ in (I64, I32, U8):
        return pa.array(values, typ)
    values = [None if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in values]
    if typ == DICT:
        entries = sorted(set(v for v in values if v is not None))
        at = {v: i for i, v in enumerate(entries)}
        idx = pa.array([None if v is None else at[v] for v in values], pa.int32())
        return pa.DictionaryArray.from_arrays(idx, pa.array(entries, pa.binary()).cast(pa.string(), safe=False))
    return pa.array(values, {UTF8: pa.binary(), LARGE: pa.large_binary(), VIEW: pa.binary_view()}[typ])


def column(arr, mem=T.MEM_DEVICE):
    col = T.Column.from_arrow(arr)
    if mem == T.MEM_DEVICE:
        return on_device(col)
    col.c.mem = mem
    return col


def filler(typ):
    return 0 if typ in (I64, I32, U8) else b"pad"


def columns_of(rows, types, mem=T.MEM_DEVICE, offsets=None):
    """the table's columns; offsets[c]: component c is a slice that starts at that Arrow offset"""
    offsets = offsets or [0] * len(types)
    cols = []
    for c, typ in enumerate(types):
        arr = array([filler(typ)] * offsets[c] + [r[c] for r in rows], typ)
        cols.append(column(arr, mem).sliced(offsets[c], len(rows)))
    return cols


def batches_of(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[col.sliced(lo, hi - lo) for col in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


# ---- plans, sets, reads ---------------------------------------------------------------------------------------------------
def plan_of(arity, mode="plain", bound=10000, key=KEY):
    plan = T.Plan([spec(T.KEY_PROBE, 0, columns=list(range(arity)))])
    plan.set_fingerprint_key(key)
    if mode == "rows":
        plan.set_key_probe_rows_tuples(0)
    elif mode == "counted":
        plan.set_key_probe_tuples_counted(0, bound)
    else:
        plan.set_key_probe_tuples(0, bound)
    return plan


def set_records(st, records, key=KEY):
    """hand-made 32-byte records of (tuple, count) pairs"""
    words = ex.record_words(key, records)
    d = to_device(np.array(words, np.uint64).reshape(-1)) if words else None
    st.key_probe_set_parent(0, d.data_ptr() if d is not None else None, len(words))


def set_gathered(st, rows, types, key=KEY):
    """the parent's rows walked under a rows tuples spec of a plan with the same key; what it gathered goes in"""
    parent = T.State(plan_of(len(types), "rows", key=key))
    if rows:
        parent.update(columns_of(rows, types))
    ptr, n = parent.key_probe_rows(0)
    assert n == sum(ex.all_valid(r) for r in rows)
    st.key_probe_set_parent(0, ptr, n)
    return parent


def read(st, counted=False):
    summary, entries = st.key_probe_tuples(0)
    got = dict(summary, entries=entries)
    assert got["seen"] == got["non_null"] + got["null_rows"]
    assert got["non_null"] == got["matched"] + got["missing_rows"]
    assert got["missing_rows"] == got["counted"] + got["overflow_rows"]
    assert got["null_rows"] == got["null_counted"] + got["null_overflow_rows"]
    assert got["counted"] == sum(e[2] for e in entries if not e[3]) and got["missing_keys"] == sum(1 for e in entries if not e[3])
    assert got["null_counted"] == sum(e[2] for e in entries if e[3]) and got["null_keys"] == sum(1 for e in entries if e[3])
    assert entries == sorted(entries)
    if counted:
        pairs = st.key_probe_pairs(0)
        assert pairs["join_rows"] == pairs["pairs"] + got["missing_rows"] + got["null_rows"]
        got.update(pairs)
    return got


def check(child, types, records, counted=False, mem=T.MEM_DEVICE, cuts=None, offsets=None, parent_types=None,
          gathered=None, want=None):
    """child: rows; records: (tuple, count) pairs of the set, given hand-made -- or `gathered`: the parent's rows, walked
    by a rows tuples spec (then records is what that gathers)"""
    T.init()
    arity = len(types)
    st = T.State(plan_of(arity, "counted" if counted else "plain"))
    if gathered is not None:
        records = ex.records_of(gathered)
        keep = set_gathered(st, gathered, parent_types or types)
    else:
        set_records(st, records)
    if child:
        cols = columns_of(child, types, mem, offsets)
        for b in batches_of(cols, len(child), cuts):
            st.update(b)
    want = dict(want if want is not None else ex.walk(child, records, KEY, counted))
    want["arity"] = arity  # (the plan's, rows or none)
    got = read(st, counted)
    assert got == want
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.matches, r.distinct) == (want["seen"], want["non_null"], want["matched"], want["missing_keys"])
    return st, want


# ---- the rules of a row, on five-row tables ---------------------------------------------------------------------------------
@pytest.mark.parametrize("counted", [False, True], ids=["plain", "counted"])
def test_a_null_component_matches_nothing_even_a_parent_tuple_with_a_null_in_the_same_place(counted):
    child = [(1, None), (1, 2), (None, None), (1, None), (3, 4)]
    records = [((1, None), 1), ((1, 2), 1), ((None, None), 1)]  # (hand-made: the NULL-bearing tuples fingerprint alike)
    st, want = check(child, [I64, I64], records, counted)
    assert want["matched"] == 1 and want["null_rows"] == 3 and want["null_keys"] == 2 and want["missing_keys"] == 1
    assert want["parent_keys"] == 3
    fp = ex.fingerprint(KEY, (1, None))
    assert fp + (2, 1) in want["entries"] and ex.fingerprint(KEY, (3, 4)) + (1, 0) in want["entries"]
    # the same parent as rows: its NULL-bearing tuples are gathered nowhere
    st, want = check(child, [I64, I64], None, counted, gathered=[(1, None), (1, 2), (None, None)])
    assert want["parent_keys"] == 1 and want["matched"] == 1


@pytest.mark.parametrize("layout", [UTF8, LARGE, VIEW, DICT], ids=str)
def test_where_one_string_ends_and_the_order_of_the_components_matter(layout):
    child = [("ab", "c"), ("a", "bc"), ("abc", ""), ("", "abc"), ("ab", "c")]
    st, want = check(child, [layout, layout], [(("a", "bc"), 1)])
    assert want["matched"] == 1 and want["missing_keys"] == 3 and want["counted"] == 4
    child = [(1, 2), (2, 1), (1, 1), (2, 2), (1, 2)]
    st, want = check(child, [I64, I64], [((2, 1), 1)])
    assert want["matched"] == 1 and want["missing_keys"] == 3
    # an integer and the string of its digits, its bytes, nothing: different components
    st, want = check([(1, "1"), (1, b"\x01"), (1, "")], [I64, layout], [((1, "1"), 1)])
    assert want["matched"] == 1 and want["missing_keys"] == 2


def test_duplicate_parent_records_add_up_to_pairs():
    child = [(1, "a"), (1, "a"), (2, "b"), (3, "c"), (None, "a")]
    records = [((1, "a"), 1), ((1, "a"), 1), ((2, "b"), 5), ((1, "a"), 3), ((9, "z"), 1 << 40)]
    st, want = check(child, [I64, UTF8], records, counted=True)
    assert want["pairs"] == 2 * 5 + 5 and want["join_rows"] == 15 + 1 + 1 and want["max_count"] == 1 << 40
    assert want["parent_rows"] == 10 + (1 << 40) and want["parent_keys"] == 3 and want["route"] == 6
    # as rows
    parent = [(1, "a"), (1, "a"), (2, "b"), (1, "a"), (None, "q"), (2, None)]
    st, want = check(child, [I64, UTF8], None, counted=True, gathered=parent)
    assert want["pairs"] == 2 * 3 + 1 and want["parent_rows"] == 4


# ---- arities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("numeric", [True, False], ids=["numeric", "mixed"])
@pytest.mark.parametrize("arity", [2, 3, 8])
def test_arities(arity, numeric):
    rng = np.random.default_rng(arity)
    types = [I64 if numeric or c % 2 == 0 else (UTF8, VIEW, DICT, LARGE)[(c // 2) % 4] for c in range(arity)]

    def draw(n):
        rows = []
        for _ in range(n):
            base = int(rng.integers(0, 12))
            row = [base + c if types[c] == I64 else b"s%d-%d" % (base, c) for c in range(arity)]
            if rng.random() < 0.2:  # a tuple that differs in its LAST component only
                row[-1] = (row[-1] + 100) if types[-1] == I64 else row[-1] + b"!"
            if rng.random() < 0.15:
                row[int(rng.integers(0, arity))] = None
            rows.append(tuple(row))
        return rows

    child, parent = draw(300), draw(40)
    for counted in (False, True):
        st, want = check(child, types, None, counted, gathered=parent)
        assert want["matched"] > 0 and want["missing_keys"] > 0 and want["null_keys"] > 0


def test_nine_columns_a_null_list_and_a_list_on_another_kind_are_refused_at_plan_creation():
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*KEY_PROBE over 9 columns"):
        T.Plan([spec(T.KEY_PROBE, 0, columns=list(range(9)))])
    s = spec(T.KEY_PROBE, 0)
    s.n_columns = 2  # (and no list)
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*KEY_PROBE over 2 columns"):
        T.Plan([s])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*only DISTINCT takes a column list"):
        T.Plan([spec(T.VALUE_COUNTS, 0, columns=[0, 1])])


# ---- component types ------------------------------------------------------------------------------------------------------------
def test_a_narrow_child_joins_a_wide_parent():
    child = [(-5, 200), (7, 255), (-5, 0), (None, 3), (2_000_000_000, 200)]
    parent = [(-5, 200), (2_000_000_000, 200), (7, 0)]
    st, want = check(child, [I32, U8], None, gathered=parent, parent_types=[I64, I64])
    assert want["matched"] == 2 and want["missing_keys"] == 2 and want["null_keys"] == 1
    # the sign extension is the key: Int32 -5 is int64 -5, not 2^32 - 5
    st, want = check([(-5, 1)], [I32, U8], [(((1 << 32) - 5, 1), 1)])
    assert want["matched"] == 0
    st, want = check([(-5, 1)], [I32, U8], [((-5 & M64, 1), 1)])
    assert want["matched"] == 1


@pytest.mark.parametrize("parent_layout", [UTF8, DICT], ids=str)
@pytest.mark.parametrize("layout", [UTF8, LARGE, VIEW, DICT], ids=str)
def test_any_string_layout_joins_any_other_with_values_at_a_views_inline_edge(layout, parent_layout):
    v12, v13, w12, w13 = b"x" * 12, b"x" * 13, b"y" * 12, b"y" * 13
    child = [(1, v12), (1, v13), (2, w12), (2, w13), (1, None), (1, b""), (3, b"x" * 40)]
    parent = [(1, v12), (2, w13), (1, b""), (3, b"x" * 40), (1, v12)]
    for counted in (False, True):
        st, want = check(child, [I64, layout], None, counted, gathered=parent, parent_types=[I64, parent_layout])
        assert want["matched"] == 4 and want["missing_keys"] == 2 and want["null_keys"] == 1


def test_a_dictionary_with_a_null_entry_and_an_index_outside_it():
    T.init()
    entries = pa.array([b"x", None, b"y"], pa.binary()).cast(pa.string(), safe=False)
    idx = pa.array([0, 1, 2, 7, None, 0, -1, 2], pa.int32())
    strings = pa.DictionaryArray.from_arrays(idx, entries, safe=False)
    ints = pa.array([1, 1, 1, 1, 1, 2, 2, None], pa.int64())
    child = [(1, b"x"), (1, None), (1, b"y"), (1, None), (1, None), (2, b"x"), (2, None), (None, b"y")]
    records = [((1, b"x"), 1), ((2, b"x"), 2)]
    for mode in ("plain", "counted"):
        st = T.State(plan_of(2, mode))
        set_records(st, records)
        st.update([column(ints), column(strings)])
        got, want = read(st, mode == "counted"), ex.walk(child, records, KEY, mode == "counted")
        assert got == want and want["null_rows"] == 5 and want["null_keys"] == 3 and want["matched"] == 2
    # the gather emits a record for the all-valid rows only
    st = T.State(plan_of(2, "rows"))
    st.update([column(ints), column(strings)])
    recs = st.key_probe_rows_records(0, 32)
    assert sorted(map(tuple, np.asarray(recs).reshape(-1, 4).tolist())) == \
        sorted(ex.record_words(KEY, ex.records_of(child)))


@pytest.mark.parametrize("offsets", [(1, 3), (7, 13), (63, 2), (9, 65)], ids=str)
def test_sliced_columns_whose_arrow_offsets_differ_between_the_components(offsets):
    rng = np.random.default_rng(sum(offsets))
    child = [(None if rng.random() < 0.2 else int(rng.integers(0, 9)), None if rng.random() < 0.2 else b"v%d" % rng.integers(0, 9))
             for _ in range(300)]
    parent = [(k, b"v%d" % ((k * 3) % 9)) for k in range(9)] + [(1, b"v1")]
    for types in ([I64, UTF8], [I32, VIEW], [I64, I64]):
        rows = child if types[1] != I64 else [(a, None if b is None else int(b[1:])) for a, b in child]
        prows = parent if types[1] != I64 else [(a, int(b[1:])) for a, b in parent]
        check(rows, types, None, True, offsets=list(offsets), gathered=prows)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    child = [(int(rng.integers(0, 6)), None if rng.random() < 0.25 else b"w%d" % rng.integers(0, 6)) for _ in range(n)]
    parent = [(k, b"w%d" % k) for k in range(6)] + [(0, b"w1"), (0, b"w1")]
    check(child, [I64, UTF8], None, True, gathered=parent)
    check([(a, None if b is None else int(b[1:])) for a, b in child], [I64, I64], None, False,
          gathered=[(a, int(b[1:])) for a, b in parent])


# ---- 70 000 rows, every batching, both memory spaces ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big():
    """70 000 rows of (Int64, Utf8) from 400 tuples, a fifth of them strangers, 5 % NULLs a component; the parent holds
    300 of the tuples, some twice.  The reference is the numpy twin, computed once"""
    rng = np.random.default_rng(70_000)
    pool = [(int(k % 37) - 5, b"name-%d" % (k // 3)) for k in range(400)]
    picks = rng.integers(0, len(pool), 70_000)
    a_null, b_null = rng.random(70_000) < 0.05, rng.random(70_000) < 0.05
    child = [(None if a_null[i] else pool[p][0], None if b_null[i] else pool[p][1]) for i, p in enumerate(picks)]
    parent = pool[:300] + pool[:50] + [(None, b"name-1"), (4, None)]
    records = ex.records_of(parent)
    cols = [(np.array([0 if r[c] is None else r[c] for r in child], object), np.array([r[c] is not None for r in child]))
            for c in range(2)]
    want = {counted: ex.walk_np(cols, records, KEY, counted) for counted in (False, True)}
    return child, parent, want


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("cuts", [None, 8192, (1, 64, 8191, 8192, 40_000, 69_999)], ids=["one", "8192", "ragged"])
def test_70000_rows_in_every_batching_give_one_answer(cuts, mem):
    child, parent, want = big()
    for counted in (False, True):
        st, w = check(child, [I64, UTF8], None, counted, mem=mem, cuts=cuts, gathered=parent, want=want[counted])
        assert w["matched"] > 40_000 and w["missing_keys"] > 50 and w["null_keys"] > 100


# ---- the set's sources ------------------------------------------------------------------------------------------------------------
def test_the_empty_set_an_empty_child_and_an_all_null_child():
    child = [(1, "a"), (2, "b"), (1, "a"), (None, "a")]
    for counted in (False, True):
        st, want = check(child, [I64, UTF8], [], counted)
        assert want["route"] == 0 and want["parent_keys"] == 0 and want["matched"] == 0 and want["missing_keys"] == 2
        st, want = check(child, [I64, UTF8], None, counted, gathered=[])
        assert want["route"] == 0
        st, want = check([], [I64, UTF8], [((1, "a"), 2)], counted)
        assert want["seen"] == 0 and want["route"] == (6 if counted else 5) and want["entries"] == []
        st, want = check([(None, None), (None, "a"), (1, None), (None, None)], [I64, UTF8], [((1, "a"), 2)], counted)
        assert want["non_null"] == 0 and want["null_rows"] == 4 and want["null_keys"] == 3


def test_hand_made_records_with_multiplicities_up_to_2_to_the_40_and_their_refusals():
    child = [(k % 5, b"t%d" % (k % 3)) for k in range(200)]
    records = [((k, b"t%d" % k), (1 << (10 * k)) + k) for k in range(3)] + [((0, b"t0"), 1 << 40)]
    st, want = check(child, [I64, UTF8], records, counted=True)
    assert want["max_count"] == (1 << 40) + 1 and want["pairs"] > 1 << 40
    T.init()
    good = ex.record_words(KEY, records)
    for bad, message in (((M64, 5, 1, 0), "TGX_INVALID_ARGUMENT.*free-slot marker"),
                         ((5, M64, 1, 0), "TGX_INVALID_ARGUMENT.*free-slot marker"),
                         ((5, 6, 0, 0), "TGX_INVALID_ARGUMENT.*count of 0"),
                         ((5, 6, 1 << 63, 0), "TGX_UNSUPPORTED.*2\\^63")):
        st = T.State(plan_of(2, "counted"))
        d = to_device(np.array(good + [bad], np.uint64).reshape(-1))
        with pytest.raises(T.TgxError, match=message):
            st.key_probe_set_parent(0, d.data_ptr(), len(good) + 1)
        assert read(st, True)["route"] == 0
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
            st.update(columns_of(child, [I64, UTF8]))


def test_a_tuple_distinct_export_is_a_set_of_the_plain_probe():
    T.init()
    parent = [(1, b"a"), (2, b"b"), (1, b"a"), (3, None), (None, None), (4, b"d" * 20)]
    child = [(1, b"a"), (4, b"d" * 20), (3, None), (5, b"e"), (None, None), (2, b"b"), (2, b"bb")]
    dplan = T.Plan([spec(T.DISTINCT, 0, columns=[0, 1])])
    dplan.set_fingerprint_key(KEY)
    dst = T.State(dplan)
    dst.update(columns_of(parent, [I64, UTF8]))
    assert dst.distinct_record_bytes(0) == 32
    ptr, counts = dst.distinct_export(0, 1)
    st = T.State(plan_of(2))
    st.key_probe_set_parent(0, ptr, counts[0])
    st.update(columns_of(child, [I32, VIEW]))
    # (DISTINCT keeps a NULL-bearing tuple as a value of its own: it is a key of the set, and matches nothing)
    want = ex.walk(child, [(t, 1) for t in set(ex.as_tuple(r) for r in parent)], KEY)
    assert read(st) == want and want["parent_keys"] == 5 and want["matched"] == 3 and want["null_keys"] == 2


# ---- how a state travels ----------------------------------------------------------------------------------------------------------
def halves():
    rng = np.random.default_rng(5)
    child = [(None if rng.random() < 0.1 else int(rng.integers(0, 30)), None if rng.random() < 0.1 else b"h%d" % rng.integers(0, 4))
             for _ in range(2000)]
    parent = [(k, b"h%d" % (k % 4)) for k in range(0, 30, 2)] * 2
    return child, parent


@pytest.mark.parametrize("counted", [False, True], ids=["plain", "counted"])
def test_reset_keeps_the_set(counted):
    child, parent = halves()
    st, want = check(child, [I64, UTF8], None, counted, gathered=parent)
    st.reset()
    empty = read(st, counted)
    assert empty["seen"] == 0 and empty["entries"] == [] and empty["null_counted"] == 0
    assert (empty["route"], empty["parent_keys"], empty["parent_digest"]) == (want["route"], want["parent_keys"], want["parent_digest"])
    st.update(columns_of(child, [I64, UTF8]))
    assert read(st, counted) == want


@pytest.mark.parametrize("counted", [False, True], ids=["plain", "counted"])
def test_a_blob_taken_mid_table_and_a_merge_of_two_halves(counted):
    T.init()
    child, parent = halves()
    mode = "counted" if counted else "plain"
    plan = plan_of(2, mode)
    want = ex.walk(child, ex.records_of(parent), KEY, counted)
    cols = columns_of(child, [I64, UTF8])
    first, second = [c.sliced(0, 900) for c in cols], [c.sliced(900, 1100) for c in cols]
    a = T.State(plan)
    keep = set_gathered(a, parent, [I64, UTF8])
    a.update(first)
    blob = a.serialize()
    assert fpr is not None and T.blob_fingerprint_key(blob) == KEY  # (a keyed blob)
    b = T.State.deserialize(plan, blob)
    half = read(b, counted)
    assert half["seen"] == 900 and half["route"] == 0 and half["parent_digest"] == want["parent_digest"]  # (no set came back)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*needs its parent set"):
        b.update(second)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*another parent set"):
        set_records(b, [((1, b"h1"), 1)])
    keep2 = set_gathered(b, parent, [I64, UTF8])
    b.update(second)
    assert read(b, counted) == want
    # two half-table states merged equal one state
    c, d = T.State(plan), T.State(plan)
    k3, k4 = set_gathered(c, parent, [I64, UTF8]), set_gathered(d, parent, [I64, UTF8])
    c.update(first)
    d.update(second)
    c.merge([d])
    assert read(c, counted) == want
    # a blob under a plan of another mode, or of another arity, is refused; so is a merge under another set
    other = plan_of(2, "plain" if counted else "counted")
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(other, blob)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plan_of(3, mode), blob)
    e = T.State(plan)
    set_records(e, [((1, b"h1"), 1)])
    e.update(first)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different parent sets"):
        c.merge([e])


def test_states_of_another_arity_mode_or_kind_of_key_do_not_merge():
    """a state belongs to its plan: tgx_merge takes the states of ONE plan, so a live state of a plan of another arity,
    of the other mode, or of a strings or an integer spec is refused, whichever way round"""
    T.init()
    child, parent = halves()
    cols = columns_of(child[:100], [I64, UTF8])
    states = {}
    for name, plan in (("plain2", plan_of(2, "plain")), ("counted2", plan_of(2, "counted")), ("plain3", plan_of(3, "plain"))):
        st = T.State(plan)
        set_records(st, [((1, b"h1"), 1)] if name != "plain3" else [((1, b"h1", 1), 1)])
        st.update(cols if name != "plain3" else cols + [cols[0]])
        states[name] = st
    splan = T.Plan([spec(T.KEY_PROBE, 1)])
    splan.set_fingerprint_key(KEY)
    splan.set_key_probe_strings(0, 100, 64)
    states["strings"] = T.State(splan)
    states["strings"].key_probe_set_parent(0, None, 0)
    states["strings"].update(cols)
    iplan = T.Plan([spec(T.KEY_PROBE, 0)])
    iplan.set_key_probe(0, 100)
    states["integers"] = T.State(iplan)
    states["integers"].key_probe_set_parent(0, None, 0)
    states["integers"].update(cols)
    before = read(states["plain2"])
    for other in ("counted2", "plain3", "strings", "integers"):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*does not belong to plan"):
            states["plain2"].merge([states[other]])
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*does not belong to plan"):
            states[other].merge([states["plain2"]])
    assert read(states["plain2"]) == before
    # their blobs do not cross either: the strings and the integer spec's under the tuples plan, and the reverse
    for other in ("strings", "integers", "counted2", "plain3"):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan_of(2, "plain"), states[other].serialize())
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(states[other].plan, states["plain2"].serialize())


def test_a_rows_state_does_not_merge_or_serialize():
    T.init()
    plan = plan_of(2, "rows")
    a, b = T.State(plan), T.State(plan)
    a.update(columns_of([(1, "a")], [I64, UTF8]))
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*gathers rows does not serialize"):
        a.serialize()
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*gathers rows does not merge"):
        b.merge([a])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*takes no parent set"):
        a.key_probe_set_parent(0, None, 0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_a_float_component_is_unsupported_and_the_next_batch_still_runs():
    T.init()
    st = T.State(plan_of(2))
    set_records(st, [((1, 2), 1)])
    ints = column(pa.array([1, 3], pa.int64()))
    for bad in (pa.array([2.0, 4.0], pa.float64()), pa.array([2.0, 4.0], pa.float32()), pa.array([2, 4], pa.uint64()),
                pa.array([True, False])):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*tuple keys takes integer and string columns"):
            st.update([ints, column(bad)])
        assert read(st)["seen"] == 0
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*validity-only"):
        st.update([ints, T.Column.validity_only(pa.array([2, 4], pa.int64()))])
    st.update([ints, column(pa.array([2, 4], pa.int64()))])
    got = read(st)
    assert (got["seen"], got["matched"], got["missing_keys"]) == (2, 1, 1)


def test_a_second_plan_call_a_tuples_call_without_a_list_and_the_calls_of_other_kinds():
    T.init()
    for first in ("set_key_probe_tuples", "set_key_probe_tuples_counted", "set_key_probe_rows_tuples"):
        for second in ("set_key_probe_tuples", "set_key_probe_tuples_counted", "set_key_probe_rows_tuples"):
            plan = T.Plan([spec(T.KEY_PROBE, 0, columns=[0, 1])])
            getattr(plan, first)(0)
            if first != second:
                with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*has been set"):
                    getattr(plan, second)(0)
    plan = T.Plan([spec(T.KEY_PROBE, 0, columns=[0, 1]), spec(T.KEY_PROBE, 0)])
    for call in ("set_key_probe", "set_key_probe_counted", "set_key_probe_rows", "set_key_probe_strings",
                 "set_key_probe_strings_counted", "set_key_probe_rows_strings"):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*has a column list"):
            getattr(plan, call)(0)
    for call in ("set_key_probe_tuples", "set_key_probe_tuples_counted", "set_key_probe_rows_tuples"):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*needs a spec with a column list"):
            getattr(plan, call)(1)
    plan.set_key_probe_tuples(0)
    plan.set_key_probe(1)
    st = T.State(plan)
    lib, err = T.lib(), T._lib._Error()
    n = T._lib.C.c_uint64(0)
    C = T._lib.C
    # the reads of the other kinds of spec on a tuples spec, and the tuples' reads on an integer spec
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_key_probe_entries_tuples"):
        st.key_probe(0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*does not probe string keys"):
        st.key_probe_strings(0)
    assert lib.tgx_key_probe_entries_bytes(plan.h, st.h, 0, None, 0, C.byref(n), None, 0, C.byref(n), C.byref(err)) == 1
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*does not read tuple keys"):
        st.key_probe_tuples(1)
    assert lib.tgx_key_probe_entries_tuples(plan.h, st.h, 1, None, 0, C.byref(n), C.byref(err)) == 1


# ---- the one case whose bounds are below its keys ------------------------------------------------------------------------------
def test_overflow_three_missing_and_three_null_bearing_tuples_under_a_bound_of_one():
    """max_missing_keys 1: a table of 4 slots for 6 distinct tuples.  Which tuples find a slot is the device's business:
    the identities hold, and the entries are a subset of the true ones with counts no larger"""
    T.init()
    child = [(10, 1), (20, 2), (30, 3), (None, 1), (2, None), (None, None)] * 50 + [(7, 7)] * 9
    records = [((7, 7), 1)]
    true = ex.walk(child, records, KEY)
    plan = plan_of(2, "plain", bound=1)
    st = T.State(plan)
    set_records(st, records)
    st.update(columns_of(child, [I64, I64]))
    got = read(st)  # (the identities)
    for f in ("seen", "non_null", "null_rows", "matched", "missing_rows", "parent_keys", "parent_digest", "route"):
        assert got[f] == true[f], f
    assert got["overflow_rows"] + got["null_overflow_rows"] >= 2 * 50  # (at most 4 of the 6 tuples have a slot)
    by_key = {e[:2]: e for e in true["entries"]}
    for e in got["entries"]:
        assert e[:2] in by_key and e[3] == by_key[e[:2]][3] and 0 < e[2] <= by_key[e[:2]][2]
