"""Join coverage on STRING keys on the device: a counted strings spec (Plan.set_key_probe_strings_counted, route 6) and a
rows strings spec (Plan.set_key_probe_rows_strings), held against tests/exact_join_coverage_strings.py.  Every counter,
`pairs`, `join_rows`, the set's identity, `max_count`, the route and every missing key with its rows and its place are
compared for EQUALITY with the exact walk over bytes, and the identities are checked on every read -- for every string
layout and value length, Arrow offsets and NULL rates, every shape of set (gathered by a rows strings spec and from
hand-made records: tests/fp_reference.py), dictionaries, every batching and every way a state travels, and end to end
through JoinCoverageConstraint on string columns.  No input holds two values of one 128-bit fingerprint, so there is no
tolerance anywhere."""
import functools
import json
import os
import struct
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_join_coverage_strings as ex
import fp_reference as fpr
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

KEY = bytes(range(1, 17))
M64 = (1 << 64) - 1
HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [0, 1, 7, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 300]  # the fingerprint's block edges; 12 | 13: a view's inline edge
LAYOUTS = [pa.string(), pa.large_string(), pa.string_view(), "dictionary"]
with open(os.path.join(HERE, "golden", "join_coverage_string_vectors.json")) as f:
    GOLDEN = json.load(f)["cases"]


@pytest.fixture(autouse=True)
def the_two_entry_points():
    """every test here is about the two new modes: without them in the library none has anything to say"""
    for name in ("tgx_plan_set_key_probe_strings_counted", "tgx_plan_set_key_probe_rows_strings"):
        assert hasattr(T.lib(), name), name


@functools.lru_cache(maxsize=None)
def fp(value, key=KEY):
    return fpr.fingerprint(key, value)


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


def array(values, layout=pa.string()):
    """values: bytes / str / None.  (Binary arrays have the string layouts: values need not be UTF-8)"""
    values = ex.as_bytes(values)
    if layout == "dictionary":
        entries = sorted(set(v for v in values if v is not None))
        at = {v: i for i, v in enumerate(entries)}
        idx = pa.array([None if v is None else at[v] for v in values], pa.int32())
        return pa.DictionaryArray.from_arrays(idx, pa.array(entries, pa.binary()).cast(pa.string(), safe=False))
    binary = {pa.string(): pa.binary(), pa.large_string(): pa.large_binary(), pa.string_view(): pa.binary_view()}[layout]
    return pa.array(values, binary)


def batches(values, layout=pa.string(), mem=T.MEM_DEVICE, cuts=None, offset=0):
    """the column of `values` as a list of batches: whole, cut every `cuts` rows, or cut at the rows `cuts` lists; with
    `offset` rows of padding in front that the view slices off"""
    n = len(values)
    col = column(array([b"pad"] * offset + list(values), layout), mem).sliced(offset, n)
    if cuts is None:
        return [[col]] if n else []
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[col.sliced(lo, hi - lo)] for lo, hi in zip(bounds[:-1], bounds[1:])]


def values_of(rng, n, n_distinct, null_rate=0.0, lengths=(1, 2, 3, 5, 8, 12, 13)):
    pool = [bytes(rng.integers(97, 123, lengths[i % len(lengths)], dtype=np.uint8)) + b"%d" % i for i in range(n_distinct)]
    picks = rng.integers(0, n_distinct, n)
    nulls = rng.random(n) < null_rate
    return [None if nulls[i] else pool[picks[i]] for i in range(n)], pool


# ---- sets -------------------------------------------------------------------------------------------------------------------
def device_records(recs):
    """32-byte {hash_a, hash_b, count, 0} records of ((fa, fb), count) pairs in device memory"""
    out = np.zeros((len(recs), 4), np.uint64)
    for i, ((fa, fb), c) in enumerate(recs):
        out[i] = (fa, fb, c, 0)
    return to_device(out.reshape(-1)) if len(recs) else None


def set_fingerprints(st, recs, i=0):
    d = device_records(recs)
    st.key_probe_set_parent(i, d.data_ptr() if d is not None else None, len(recs))


def set_hand_made(st, records, i=0, key=KEY):
    """records: (value, count) pairs"""
    set_fingerprints(st, [(fp(ex.as_bytes([v])[0], key), c) for v, c in records], i)


def rows_plan(key=KEY, n=1):
    plan = T.Plan([spec(T.KEY_PROBE, 0) for _ in range(n)])
    if key is not None:
        plan.set_fingerprint_key(key)
    for k in range(n):
        plan.set_key_probe_rows_strings(k)
    return plan


def set_gathered(st, values, i=0, key=KEY, layout=pa.string(), cuts=None):
    """the far side's column walked under a rows strings spec of a second plan with the same key; its records go in"""
    far = T.State(rows_plan(key))
    for b in batches(values, layout, cuts=cuts):
        far.update(b)
    ptr, n = far.key_probe_rows(0)
    st.key_probe_set_parent(i, ptr, n)


def plan_of(bounds=((10000, 256),), extra=(), key=KEY):
    plan = T.Plan([spec(T.KEY_PROBE, 0) for _ in bounds] + list(extra))
    plan.set_fingerprint_key(key)
    for k, (keys, size) in enumerate(bounds):
        plan.set_key_probe_strings_counted(k, keys, size)
    return plan


def read(st, i=0):
    summary, entries = st.key_probe_strings(i)
    pairs = st.key_probe_pairs(i)
    got = dict(summary, entries=entries, **pairs)
    assert got["seen"] == got["non_null"] + got["null_rows"]
    assert got["non_null"] == got["matched"] + got["missing_rows"]
    assert got["missing_rows"] == got["counted"] + got["overflow_rows"] + got["long_rows"]
    assert got["counted"] == sum(entries.values()) and got["missing_keys"] == len(entries)
    assert got["join_rows"] == got["pairs"] + got["missing_rows"] + got["null_rows"]
    assert got["matched"] <= got["pairs"] <= got["matched"] * max(got["max_count"], 1)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_key_probe_entries_bytes"):
        st.key_probe(i)
    return got


def exact(child, records, max_value_bytes=256, key=KEY):
    """records: (value, count) pairs"""
    s, p = ex.walk(child, records, max_value_bytes)
    ident = ex.identity(key, records) if key == KEY else ex.identity_of_fingerprints(
        [(fpr.fingerprint(key, ex.as_bytes([v])[0]), c) for v, c in records])
    assert (ident["parent_keys"], ident["parent_rows"], ident["max_count"]) == (s["parent_keys"], p["parent_rows"], p["max_count"])
    return dict(s, max_value_bytes=max_value_bytes, **p, parent_digest=ident["parent_digest"],
                parent_count_digest=ident["parent_count_digest"])


def check(child, far, layout=pa.string(), max_value_bytes=256, bound=10000, mem=T.MEM_DEVICE, cuts=None, offset=0,
          gathered=True, far_layout=pa.string()):
    """child: bytes / str / None; far: the far side's rows (gathered by a rows strings spec) or, hand-made, (value,
    count) records"""
    T.init()
    plan = plan_of(((bound, max_value_bytes),))
    st = T.State(plan)
    if gathered:
        set_gathered(st, far, layout=far_layout)
        records = ex.records_of(far)
    else:
        set_hand_made(st, far)
        records = list(far)
    for b in batches(child, layout, mem, cuts, offset):
        st.update(b)
    want = exact(child, records, max_value_bytes)
    got = read(st)
    assert got == want and list(got["entries"]) == list(want["entries"])  # (the order too: ascending bytewise)
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.matches, r.distinct) == (want["seen"], want["non_null"], want["matched"], want["missing_keys"])
    assert read(st) == want
    return st, plan, want


# ---- lengths and layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gathered", [True, False], ids=["gathered", "hand-made"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_lengths_at_the_fingerprints_block_edges(layout, gathered):
    """every length among the matched values (each with a multiplicity of its own) and among the missing ones; 300
    bytes: matched when the far side holds it, a long row when it does not"""
    hit = [b"h" * n for n in LENGTHS]
    miss = [b"m" * n for n in LENGTHS if n]
    child = (hit + miss + [None]) * 3
    far = [v for i, v in enumerate(hit) for _ in range(i % 4 + 1)] + [None, None]
    st, _, want = check(child, far if gathered else [(v, i % 4 + 1) for i, v in enumerate(hit)], layout, gathered=gathered,
                        far_layout=layout)
    assert want["matched"] == 3 * len(hit) and want["long_rows"] == 3 and b"m" * 33 in want["entries"]
    assert want["pairs"] == 3 * sum(i % 4 + 1 for i in range(len(hit))) and want["max_count"] == 4 and want["route"] == 6
    # values whose bytes all differ: the order of the bytes within a block and of the blocks
    rng = np.random.default_rng(21)
    hit = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in LENGTHS if n]
    swapped = [v[8:16] + v[:8] + v[16:] for v in hit if len(v) >= 16] + [v[::-1] for v in hit if len(v) > 1]
    child = hit + swapped + [None] + hit
    st, _, want = check(child, hit + hit[:3] if gathered else [(v, 2) for v in hit], layout, gathered=gathered)
    assert want["matched"] == 2 * len(hit) and want["long_rows"] == 2
    # the empty string missing, and a far side that holds nothing but it
    check([b"", b"a", b"", None], [b"a"] if gathered else [(b"a", 1)], layout, gathered=gathered)
    check([b"", b"a", b"", None], [b"", b""] if gathered else [(b"", 2)], layout, gathered=gathered)


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_the_byte_bound(layout):
    child = [b"x" * 40, b"x" * 41, b"y" * 40, b"y" * 41, b"z" * 300, b"x" * 41]
    st, _, want = check(child, [b"y" * 41, b"z" * 300, b"z" * 300], layout, max_value_bytes=40)
    assert want["entries"] == {b"x" * 40: 1, b"y" * 40: 1} and want["long_rows"] == 2 and want["pairs"] == 3
    assert want["join_rows"] == 3 + 4
    check([b"ab", b"a", b""], [], layout, max_value_bytes=1)


# ---- offsets, validity, row counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
@pytest.mark.parametrize("offset", [1, 63])
def test_sliced_arrays(layout, offset):
    rng = np.random.default_rng(offset)
    child, pool = values_of(rng, 700, 40, 0.3)
    far = [None if i % 10 == 0 else pool[k] for i, k in enumerate(rng.integers(0, 20, 300))]
    check(child, far, layout, offset=offset)


@pytest.mark.parametrize("null_rate", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_row_counts_and_null_rates(n, null_rate):
    """0 % NULLs: a column without a validity buffer"""
    rng = np.random.default_rng(n)
    child, pool = values_of(rng, n, 50, null_rate)
    far = [pool[i] for i in rng.integers(0, 30, 90)] + [None]
    check(child, far)


@functools.lru_cache(maxsize=None)
def big():
    """70 000 rows with 30 000 distinct values, of which the far side holds 2 000 with multiplicities 1 .. 7: more
    distinct missing keys than a workgroup's LDS table of 1024 slots holds"""
    rng = np.random.default_rng(70)
    pool = [b"v%05d-%s" % (i, b"x" * (i % 9)) for i in range(30_000)]
    picks = rng.integers(0, len(pool), 70_000)
    nulls = rng.random(70_000) < 0.05
    child = [None if nulls[i] else pool[picks[i]] for i in range(70_000)]
    records = [(pool[i], int(i % 7 + 1)) for i in range(0, 30_000, 15)]
    return child, records, exact(child, records)


def test_70_000_rows_and_more_missing_keys_than_the_lds_table_holds():
    child, records, want = big()
    T.init()
    st = T.State(plan_of(((65536, 256),)))
    set_hand_made(st, records)
    for b in batches(child):
        st.update(b)
    got = read(st)
    assert want["missing_keys"] > 20_000 and want["overflow_rows"] == 0
    assert got == want and list(got["entries"]) == list(want["entries"])


def test_70_000_rows_against_a_table_of_16_missing_keys():
    """the overflow counter: the global table has 32 slots; the counters and pairs stay exact, every entry held is a true
    missing key with no more than its rows"""
    child, records, want = big()
    T.init()
    st = T.State(plan_of(((16, 256),)))
    set_hand_made(st, records)
    for b in batches(child):
        st.update(b)
    got = read(st)
    assert got["overflow_rows"] > 0 and got["missing_keys"] <= 32
    for f in ("seen", "non_null", "null_rows", "matched", "missing_rows", "pairs", "join_rows", "parent_keys", "parent_digest",
              "parent_rows", "parent_count_digest", "max_count", "route", "long_rows"):
        assert got[f] == want[f], f
    assert all(0 < c <= want["entries"][k] for k, c in got["entries"].items())


# ---- the set ----------------------------------------------------------------------------------------------------------------------
def test_the_empty_set_one_record_a_power_of_two_and_records_that_add_up():
    rng = np.random.default_rng(1)
    child, pool = values_of(rng, 3000, 20, 0.2)
    for gathered in (True, False):
        st, _, want = check(child, [], gathered=gathered)
        assert want["route"] == 0 and want["pairs"] == 0 and want["parent_keys"] == 0 and want["max_count"] == 0
    st, _, want = check(child, [(pool[3], 1)], gathered=False)
    assert want["route"] == 6 and want["parent_keys"] == 1 and want["pairs"] == want["matched"] > 0
    # exactly 32 records (64 slots), of 20 values: records of one value add up; one count is 2^40
    records = [(pool[i % 20], i + 1) for i in range(31)] + [(pool[7], 2**40)]
    st, _, want = check(child, records, gathered=False)
    assert want["parent_keys"] == 20 and want["max_count"] == 2**40 + 8 + 28 and want["pairs"] > 2**40
    assert want["parent_rows"] == sum(range(1, 32)) + 2**40


def test_two_fingerprints_that_share_hash_a_keep_their_own_counts():
    """hand-made records: the fingerprint of a child value with count 3 and a twin that is equal in hash_a and differs in
    hash_b with count 5 (the fingerprint of no value here), in both orders; eight records whose hash_a & mask is the
    table's last slot, so the chain wraps"""
    T.init()
    child = [b"v%d" % i for i in range(20)]
    fa, fb = fp(child[0])
    for twins in ([((fa, fb), 3), ((fa, fb ^ 1), 5)], [((fa, fb ^ 1), 5), ((fa, fb), 3)]):
        crowd = [(((a & ~15) | 15, b ^ 4), 7) for a, b in (fp(v) for v in child[8:14])]
        recs = twins + crowd  # 8 records: 16 slots
        st = T.State(plan_of())
        set_fingerprints(st, recs)
        st.update([column(array(child))])
        got = read(st)
        ident = ex.identity_of_fingerprints(recs)
        assert ident["parent_keys"] == 8 and ident["max_count"] == 7
        assert {f: got[f] for f in ident} == ident and got["route"] == 6
        assert (got["matched"], got["pairs"], got["missing_keys"]) == (1, 3, 19)


def test_refused_sets_leave_the_state_without_one():
    T.init()
    st = T.State(plan_of())
    good = [(fp(b"a"), 2), (fp(b"b"), 1)]
    set_fingerprints(st, good)
    refusals = [([((M64, 5), 1)], "TGX_INVALID_ARGUMENT.*spec 0.*1 records.*free-slot marker"),
                ([((5, M64), 1)], "TGX_INVALID_ARGUMENT.*spec 0.*1 records.*free-slot marker"),
                ([(fp(b"c"), 0)], "TGX_INVALID_ARGUMENT.*spec 0.*1 records.*count of 0"),
                ([(fp(b"c"), 2**62), (fp(b"a"), 2**62 - 3)], "TGX_UNSUPPORTED.*spec 0.*sum to 2\\^63 or more")]
    for bad, text in refusals:
        with pytest.raises(T.TgxError, match=text):
            set_fingerprints(st, good + bad)
        assert read(st)["route"] == 0
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
            st.update([column(array([b"a"]))])
        set_fingerprints(st, good)
    st.update([column(array([b"a", b"c", b"a"]))])
    got = read(st)
    assert (got["matched"], got["pairs"], got["entries"], got["route"]) == (2, 4, {b"c": 1}, 6)
    # one below the bound is taken
    st = T.State(plan_of())
    set_fingerprints(st, [(fp(b"c"), 2**62), (fp(b"a"), 2**62 - 1)])
    assert read(st)["parent_rows"] == 2**63 - 1 and read(st)["max_count"] == 2**62


def test_a_batch_that_could_carry_pairs_past_the_word_is_refused():
    T.init()
    st = T.State(plan_of())
    set_fingerprints(st, [(fp(b"a"), 2**62)])
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*spec 0.*4 rows.*past 2\\^64 - 1"):
        st.update([column(array([b"a", b"b", b"a", None]))])
    assert read(st)["seen"] == 0
    st.update([column(array([b"a", b"b", None]))])  # 3 * 2^62 fits
    got = read(st)
    assert (got["pairs"], got["join_rows"], got["entries"]) == (2**62, 2**62 + 2, {b"b": 1})
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*past 2\\^64 - 1"):
        st.update([column(array([b"a"]))])
    assert read(st)["pairs"] == 2**62


# ---- the gather -----------------------------------------------------------------------------------------------------------------
def gathered_multiset(st, i=0):
    recs = st.key_probe_rows_records(i, 32)
    assert not recs[:, 3].any() and (recs[:, 2] > 0).all()
    m = {}
    for fa, fb, c, _ in recs.tolist():
        m[(fa, fb)] = m.get((fa, fb), 0) + c
    return m, recs


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_the_gathered_records_are_the_columns_fingerprints(layout):
    """three equal-sized batches: the first sizes the buffer, the second and the third each make it grow (room for at
    least twice the records there were), and the records of the batches before stay"""
    T.init()
    rng = np.random.default_rng(41)
    values, _ = values_of(rng, 3 * 2500, 300, 0.3, lengths=LENGTHS[:-1])
    values[5], values[2600], values[7000] = b"L" * 300, b"", b"L" * 300
    st = T.State(rows_plan())
    seen = 0
    for b in batches(values, layout, cuts=2500, offset=3):
        st.update(b)
        seen += 2500
        m, recs = gathered_multiset(st)
        assert m == ex.rows_multiset(KEY, values[:seen])
        if layout != "dictionary":
            assert len(recs) == sum(v is not None for v in values[:seen]) and (recs[:, 2] == 1).all()
    non_null = sum(v is not None for v in values)
    r = st.finalize()[0]
    assert (r.total, r.non_null) == (len(values), non_null)
    if layout == "dictionary":
        # a record per entry that rows of the batch refer to, with their number: per batch
        per_batch = sum(len(set(v for v in values[lo:lo + 2500] if v is not None)) for lo in range(0, 7500, 2500))
        assert len(recs) == per_batch and int(recs[:, 2].sum()) == non_null
    # such a state keeps its records to itself, takes no set, and reset empties it
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*gathers rows does not merge"):
        T.State(st.plan).merge([st])
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*gathers rows does not serialize"):
        st.serialize()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*gathers rows takes no parent set"):
        set_fingerprints(st, [(fp(b"a"), 1)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not counted"):
        st.key_probe_pairs(0)
    st.reset()
    assert st.key_probe_rows(0) == (None, 0)
    st.update(batches(values[:100], layout)[0])
    assert gathered_multiset(st)[0] == ex.rows_multiset(KEY, values[:100])


SETTERS = {"plain": lambda p: p.set_key_probe(0, 10), "counted": lambda p: p.set_key_probe_counted(0, 10),
           "rows": lambda p: p.set_key_probe_rows(0), "strings": lambda p: p.set_key_probe_strings(0, 10, 16),
           "strings_counted": lambda p: p.set_key_probe_strings_counted(0, 10, 16),
           "rows_strings": lambda p: p.set_key_probe_rows_strings(0)}


@pytest.mark.parametrize("mode", list(SETTERS))
def test_the_column_types_of_each_mode(mode):
    """the string layouts are taken by the three string modes and refused by the three integer ones; integers the other
    way round; floats, UInt64 and Boolean by none.  A refused batch leaves the state as it was"""
    T.init()
    n = 100
    strings = ["a", "b", None, "a"] * 25
    columns = {"Int64": pa.array(np.arange(n, dtype=np.int64)), "Int32": pa.array(np.arange(n, dtype=np.int32)),
               "Float64": pa.array(np.arange(n, dtype=np.float64)), "Float32": pa.array(np.arange(n, dtype=np.float32)),
               "UInt64": pa.array(np.arange(n, dtype=np.uint64)), "Boolean": pa.array(np.arange(n) % 2 == 0),
               "Utf8": pa.array(strings), "LargeUtf8": pa.array(strings, pa.large_string()),
               "Utf8View": pa.array(strings, pa.string_view()), "Dictionary": pa.array(strings).dictionary_encode()}
    string_mode = "strings" in mode
    for name, arr in columns.items():
        plan = T.Plan([spec(T.KEY_PROBE, 0)])
        SETTERS[mode](plan)
        st = T.State(plan)
        if "rows" not in mode:
            st.key_probe_set_parent(0, None, 0)
        is_string, is_int = name in ("Utf8", "LargeUtf8", "Utf8View", "Dictionary"), name in ("Int64", "Int32")
        for mem in (T.MEM_HOST, T.MEM_DEVICE):
            if (string_mode and is_string) or (not string_mode and is_int):
                st.update([column(arr, mem)])
                continue
            word = "takes string columns, not " if string_mode else "takes integer columns, not "
            word += "strings" if is_string else "integers" if is_int else name
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*KEY_PROBE " + ("on string keys " if string_mode else "") + word):
                st.update([column(arr, mem)])
        r = st.finalize()[0]
        taken = (string_mode and is_string) or (not string_mode and is_int)
        assert (r.total, r.non_null) == ((2 * n, 2 * (75 if is_string else n)) if taken else (0, 0))
        if mode == "rows_strings" and taken:
            own = plan.fingerprint_key()  # (the key the plan drew)
            assert gathered_multiset(st)[0] == {fpr.fingerprint(own, b"a"): 100, fpr.fingerprint(own, b"b"): 50}


# ---- dictionaries -----------------------------------------------------------------------------------------------------------------
def dictionary(indices, entries, mask=None):
    return pa.DictionaryArray.from_arrays(pa.array(indices, pa.int32(), mask=None if mask is None else ~np.asarray(mask)),
                                          pa.array(entries, pa.string()))


def test_dictionary_columns_probed_and_gathered():
    """repeated values among the entries, a NULL entry, an entry no row refers to, different dictionaries across
    batches, an empty dictionary"""
    T.init()
    rng = np.random.default_rng(6)
    entries = ["a", "b", "a", None, "unused", "c", "b"]
    idx = rng.integers(0, 7, 5000)
    idx[idx == 4] = 0
    mask = rng.random(5000) >= 0.1
    first = dictionary(idx, entries, mask)
    second = dictionary(rng.integers(0, 3, 3000), ["c", "zz", "a"])
    empty = dictionary([None, None, None], [])
    logical = first.to_pylist() + second.to_pylist() + [None] * 3
    records = [(b"a", 3), (b"zz", 2), (b"never", 9)]
    for mem in (T.MEM_DEVICE, T.MEM_HOST):
        st = T.State(plan_of())
        set_hand_made(st, records)
        far = T.State(rows_plan())
        for arr in (first, second, empty):
            st.update([column(arr, mem)])
            far.update([column(arr, mem)])
        want = exact(logical, records)
        assert read(st) == want and b"unused" not in want["entries"]
        m, recs = gathered_multiset(far)
        assert m == ex.rows_multiset(KEY, logical) and fp(b"unused") not in m
        # per batch: the distinct VALUES among the entries referred to are fewer than the entries (a and b stand twice)
        assert len(recs) == 5 + 3 and int(recs[:, 2].sum()) == want["non_null"]
        assert far.finalize()[0].non_null == want["non_null"]


def test_dictionary_indices_outside_the_dictionary_are_null_rows():
    T.init()
    idx = np.array([0, 1, 5, -1, 2, 2**31 - 1, 1], np.int32)
    entries = on_device(T.Column.from_arrow(pa.array(["a", "b", "c"])))
    col = T.Column(T.DICT32_UTF8, len(idx), values=padded(idx), mem=T.MEM_DEVICE, dictionary=entries)
    st = T.State(plan_of())
    set_hand_made(st, [(b"a", 4)])
    far = T.State(rows_plan())
    st.update([col])
    far.update([col])
    got = read(st)
    assert (got["seen"], got["null_rows"], got["matched"], got["pairs"], got["entries"]) == (7, 3, 1, 4, {b"b": 2, b"c": 1})
    assert gathered_multiset(far)[0] == {fp(b"a"): 1, fp(b"b"): 2, fp(b"c"): 1}
    r = far.finalize()[0]
    assert (r.total, r.non_null) == (7, 4)


# ---- batching and feeding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST, T.MEM_HOST_RETAINED], ids=["device", "host", "host-retained"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_batching_independence(layout, mem):
    rng = np.random.default_rng(7)
    child, pool = values_of(rng, 20_000, 300, 0.05)
    far = [pool[i] for i in rng.integers(0, 100, 400)]
    T.init()
    want = exact(child, ex.records_of(far))
    for cuts in (None, [1, 64, 65, 5000, 5001, 19_999], 8192):
        st = T.State(plan_of())
        set_gathered(st, far, layout=layout, cuts=[1, 64, 65, 399] if isinstance(cuts, list) else 128 if cuts else None)
        for b in batches(child, layout, mem, cuts):
            st.update(b)
        got = read(st)
        assert got == want and list(got["entries"]) == list(want["entries"])


# ---- the state algebra ----------------------------------------------------------------------------------------------------------------
def test_reset_half_way_reads_blobs_and_merges():
    T.init()
    rng = np.random.default_rng(9)
    child, pool = values_of(rng, 30_000, 200, 0.1)
    child[7] = b"L" * 40
    records = [(pool[i], i % 5 + 1) for i in range(120)]
    plan = plan_of(((10000, 32),))
    want = exact(child, records, 32)
    parts = [child[:10_000], child[10_000:20_000], child[20_000:]]
    st = T.State(plan)
    set_hand_made(st, records)
    st.update([column(array(parts[0]))])
    assert read(st) == exact(parts[0], records, 32)  # read half-way, then on
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*before the state's first batch"):
        set_hand_made(st, records)
    for p in parts[1:]:
        st.update([column(array(p))])
    assert read(st) == want
    st.reset()  # keeps the set
    empty = read(st)
    assert (empty["seen"], empty["pairs"], empty["entries"], empty["route"]) == (0, 0, {}, 6)
    assert all(empty[f] == want[f] for f in ("parent_keys", "parent_digest", "parent_rows", "parent_count_digest", "max_count"))
    st.update([column(array(child))])
    assert read(st) == want
    states = []
    for p in parts:
        s = T.State(plan)
        set_hand_made(s, records)
        s.update([column(array(p))])
        states.append(s)
    states[0].merge(states[1:])
    assert read(states[0]) == want
    blob = states[0].serialize()
    assert blob == st.serialize()  # equal states, equal bytes
    back = T.State.deserialize(plan, blob)
    assert read(back) == dict(want, route=0) and back.serialize() == blob  # (a deserialized state holds no set)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
        back.update([column(array(child))])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*another parent set"):
        set_hand_made(back, records[:-1])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*another parent set"):
        set_hand_made(back, records[:-1] + [(records[-1][0], records[-1][1] + 1)])  # the same keys, another count
    set_hand_made(back, records)
    back.update([column(array(child))])
    doubled = read(back)
    assert doubled["entries"] == {k: 2 * c for k, c in want["entries"].items()} and doubled["long_rows"] == 2
    assert doubled["pairs"] == 2 * want["pairs"]
    # a blob written mid-table, read back without the set: it refuses the next batch and goes on once the set is given
    mid = T.State.deserialize(plan, states[1].serialize())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
        mid.update([column(array(parts[0]))])
    set_hand_made(mid, records)
    mid.update([column(array(parts[0]))])
    mid.update([column(array(parts[2]))])
    assert read(mid) == want
    # differing identities do not merge: other keys, and the same keys with another count
    for others in (records[1:], [(records[0][0], records[0][1] + 1)] + records[1:]):
        other = T.State(plan)
        set_hand_made(other, others)
        other.update([column(array(parts[0]))])
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different parent sets"):
            st.merge([other])
    assert read(st) == want
    # the blob carries the plan's key and its own mode word: a plan with another key, with another max_value_bytes, and a
    # plain strings plan refuse it
    assert struct.unpack_from("<I", blob, 36)[0] == 1 and blob[40:56] == KEY  # (the head's { u32 keyed, u8 key[16] })
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fingerprint key"):
        T.State.deserialize(plan_of(((10000, 32),), key=bytes(16)), blob)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(plan_of(((10000, 33),)), blob)
    plain = T.Plan([spec(T.KEY_PROBE, 0)])
    plain.set_fingerprint_key(KEY)
    plain.set_key_probe_strings(0, 10000, 32)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other mode \\(plain / counted\\)"):
        T.State.deserialize(plain, blob)


def test_threaded_ranks_share_a_fingerprint_key():
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    T.init()
    rng = np.random.default_rng(10)
    n, world = 40_000, 2
    child, pool = values_of(rng, n, 300, 0.1)
    records = [(pool[i], i % 3 + 1) for i in range(200)]
    want = exact(child, records)
    whole = [column(array(child))]
    plan = plan_of(extra=[spec(T.COUNT, 0)])
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(n, world, rank)
            st = T.State(plan)
            set_hand_made(st, records)
            comm = thread_comm(group, rank, device_buffers=True)
            res = sharded_suite_step(plan, st, [c.sliced(lo, hi - lo) for c in whole], comm)
            results[rank] = (res, read(st))
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
        assert got == want and res[1].total == n


def test_a_counted_strings_spec_and_a_rows_strings_spec_on_one_column():
    """the pair the bidirectional walk uses: one plan, one walk of the column"""
    T.init()
    rng = np.random.default_rng(12)
    child, pool = values_of(rng, 9000, 150, 0.1)
    records = [(pool[i], 2) for i in range(70)]
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 0), spec(T.DISTINCT, 0, flags=T.FLAG_EXACT_KEYS)])
    plan.set_fingerprint_key(KEY)
    plan.set_key_probe_strings_counted(0, 10000, 256)
    plan.set_key_probe_rows_strings(1)
    st = T.State(plan)
    set_hand_made(st, records)
    for b in batches(child, cuts=4000):
        st.update(b)
    assert read(st) == exact(child, records)
    assert gathered_multiset(st, 1)[0] == ex.rows_multiset(KEY, child)
    assert st.finalize()[2].distinct == len(set(v for v in child if v is not None))


# ---- end to end: JoinCoverageConstraint through ValidationSuite.run(.., tables=..) ------------------------------------------------------
def run_constraint(constraint, tables, as_json=False):
    cb = S.Check.builder("c").level(S.Level.ERROR).constraint(constraint)
    suite = S.ValidationSuite.builder("s").check(cb.build()).build()
    if as_json:
        suite = S.ValidationSuite(json.loads(json.dumps(suite.spec)))
    r = suite.run(None, tables=tables)
    m = r.report.metrics
    assert m.total_checks == 1 and m.passed_checks + m.failed_checks == 1
    metric = m.custom_metrics.get("c.join_coverage")
    if m.passed_checks:
        assert r.is_success() and not r.report.issues
        return "success", metric, None
    assert len(r.report.issues) == 1 and r.report.issues[0].constraint_name == "join_coverage"
    message = r.report.issues[0].message
    return ("error" if message.startswith("Error evaluating constraint: ") else "failure"), metric, message


def table_of(name, values, layout):
    if layout == "dictionary":
        col = pa.array(values, pa.string()).dictionary_encode().cast(pa.dictionary(pa.int32(), pa.string()))
    else:
        col = pa.array(values, layout)
    return pa.table({"n": pa.array(range(len(values)), pa.int64()), name: col})


def constraint_of(case):
    c = S.JoinCoverageConstraint(case["left_table"], case["right_table"]).on(case["left_column"], case["right_column"])
    c = c.expect_match_rate(case["expected"]).coverage_type(case["coverage_type"]).distinct_only(case["distinct_only"])
    if "max_value_bytes" in case:
        c.max_value_bytes(case["max_value_bytes"])
    return c.max_examples_reported(case.get("max_examples", 100))


def low_level_counts(case):
    """the counts tgx_host_join_coverage_json takes, from the low-level calls: each side gathered by a rows strings spec
    of a plan with the copied key, the other side probed under a counted strings spec"""
    out = {}
    sides = {"left": (case["left"], case["right"]), "right": (case["right"], case["left"])}
    for name, (near, far) in sides.items():
        st = T.State(plan_of(((10000, case.get("max_value_bytes", 256)),)))
        set_gathered(st, far)
        for b in batches(near):
            st.update(b)
        got = read(st)
        out[name] = {"pairs": got["pairs"], "join_rows": got["join_rows"]}
        if name == "left":
            out["examples"] = {f: got[f] for f in ("missing_keys", "null_rows", "overflow_rows", "long_rows")}
            out["left_distinct"] = len(set(v for v in near if v is not None))
    return out


@pytest.mark.parametrize("layouts", [(pa.string(), pa.string()), (pa.large_string(), pa.string_view()),
                                     ("dictionary", pa.string()), (pa.string_view(), "dictionary")], ids=str)
@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_the_golden_tables_through_the_suite(case, layouts):
    T.init()
    tables = {case["left_table"]: table_of(case["left_column"], case["left"], layouts[0]),
              case["right_table"]: table_of(case["right_column"], case["right"], layouts[1])}
    c = constraint_of(case)
    status, metric, message = run_constraint(c, tables)
    want = ex.coverage(case["left_table"], case["right_table"], case["left"], case["right"], case["coverage_type"],
                       case["distinct_only"], case["expected"], case.get("max_examples", 100),
                       case.get("max_value_bytes", 256))
    assert status == want[0] == case["status"]
    if status == "error":
        assert metric is None and case["message"] in message
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + case["message"]):
            c.verdict_from_counts(low_level_counts(case))
        return
    assert (metric, message) == want[1:] and message == case["message"] and abs(metric - case["metric"]) <= 1e-12
    # the same constraint from its JSON forms, and the verdict of tgx_host_join_coverage_json on the low-level counts
    assert run_constraint(S.JoinCoverageConstraint.from_spec(json.loads(json.dumps(c.spec))), tables) == (status, metric, message)
    assert run_constraint(c, tables, as_json=True) == (status, metric, message)
    if layouts == (pa.string(), pa.string()):
        v = c.verdict_from_counts(low_level_counts(case))
        assert (v["status"], v["metric"], v["message"]) == (status, metric, message)


def test_the_coverage_types_through_the_suite():
    T.init()
    rng = np.random.default_rng(16)
    left, pool = values_of(rng, 20_000, 400, 0.05, lengths=(1, 30))
    right = [pool[i] for i in rng.integers(100, 500, 6000) if i < 400] + [None] * 50 + [b"only-right-%d" % i for i in range(30)]
    text = lambda values: [None if v is None else v.decode() for v in values]  # noqa: E731
    tables = {"orders": table_of("code", text(left), pa.string()).append_column("id", pa.array(range(len(left)), pa.int64()))
              .append_column("raw", pa.array([b"x"] * len(left), pa.binary())),
              "customers": table_of("code", text(right), pa.large_string())}
    for kind in (ex.LEFT, ex.RIGHT, ex.BIDIRECTIONAL):
        for expected in (0.0, 1.0):
            c = S.JoinCoverageConstraint("orders", "customers").on("code", "code").coverage_type(kind)
            assert run_constraint(c.expect_match_rate(expected), tables) == \
                ex.coverage("orders", "customers", left, right, kind, False, expected)
    c = S.JoinCoverageConstraint("orders", "customers").on("code", "code").distinct_only(True).max_examples_reported(7)
    got = run_constraint(c.expect_match_rate(1.0), tables)
    assert got == ex.coverage("orders", "customers", left, right, ex.LEFT, True, 1.0, 7) and got[1] > 1.0
    c = S.JoinCoverageConstraint("orders", "customers").on("code", "code").distinct_only(True).coverage_type(ex.RIGHT)
    assert run_constraint(c, tables)[0] == "error"
    # the bounds that are overrun: the rate stands, the examples read "at least"
    want = ex.coverage("orders", "customers", left, right, ex.LEFT, False, 1.0, 10**6)
    c = S.JoinCoverageConstraint("orders", "customers").on("code", "code").max_examples_reported(10**6)
    got = run_constraint(c.max_missing_keys(16), tables)
    assert got[:2] == want[:2] and "(at least " in got[2]
    c = S.JoinCoverageConstraint("orders", "customers").on("code", "code").max_examples_reported(10**6).max_value_bytes(8)
    assert run_constraint(c, tables) == ex.coverage("orders", "customers", left, right, ex.LEFT, False, 1.0, 10**6, 8)
    assert "(at least " in run_constraint(c, tables)[2]
    for right_kind in (ex.RIGHT, ex.BIDIRECTIONAL):
        c = S.JoinCoverageConstraint("orders", "customers").on("code", "code").coverage_type(right_kind).max_value_bytes(8)
        assert run_constraint(c, tables) == ex.coverage("orders", "customers", left, right, right_kind, False, 1.0, 100, 8)
    # a pair of an integer and a string column, a Binary column and an option out of range are the constraint's errors
    for pair, words in ((("id", "code"), ("an integer and a string", "orders.id")), (("code", "n"), ("a string and an integer", "customers.n")),
                        (("raw", "code"), ("Binary", "orders.raw"))):
        status, _, message = run_constraint(S.JoinCoverageConstraint("orders", "customers").on(*pair), tables)
        assert status == "error" and all(w in message for w in words) and "not on the GPU path" in message
    status, _, message = run_constraint(S.JoinCoverageConstraint("orders", "customers").on("code", "code").max_value_bytes(257), tables)
    assert status == "error" and "max_value_bytes must be 1 .. 256 (257)" in message


def test_a_far_side_gathered_under_another_key_matches_nothing():
    """the library cannot verify the key: a set made under a key that was NOT copied simply matches nothing"""
    T.init()
    child = [b"a", b"b", None, b"a"]
    st = T.State(plan_of())
    set_gathered(st, [b"a", b"b", b"a"], key=None)  # (the second plan keeps the key it drew)
    st.update([column(array(child))])
    got = read(st)
    assert (got["matched"], got["pairs"], got["entries"]) == (0, 0, {b"a": 2, b"b": 1})
    assert (got["parent_keys"], got["parent_rows"], got["max_count"]) == (2, 3, 2)
    st = T.State(plan_of())
    set_gathered(st, [b"a", b"b", b"a"])
    st.update([column(array(child))])
    assert read(st) == exact(child, [(b"a", 2), (b"b", 1)])
