"""A TGX_CHECK_KEY_PROBE spec on STRING keys (Plan.set_key_probe_strings) on the device, held against
tests/exact_key_probe_strings.py: every counter and every missing key with its rows are compared for equality with the
exact walk over bytes, and the three identities are checked on every read -- for every string layout and value length,
Arrow offsets and NULL rates, every shape of parent set (from a DISTINCT export and from hand-made fingerprints:
tests/fp_reference.py), every class of missing keys, dictionaries, every batching and every way a state travels, and end
to end through ForeignKeyConstraint on string columns."""
import ctypes
import functools
import json
import os
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_key_probe as exk  # (mix64: the splitmix64 finaliser on Python ints)
import exact_key_probe_strings as ex
import fp_reference as fpr
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

KEY = bytes(range(1, 17))
M64 = (1 << 64) - 1
SALT = 0x9E3779B97F4A7C15
HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = [0, 1, 7, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 300]  # the fingerprint's block edges; 12 | 13: a view's inline edge
LAYOUTS = [pa.string(), pa.large_string(), pa.string_view(), "dictionary"]
with open(os.path.join(HERE, "golden", "foreign_key_string_vectors.json")) as f:
    GOLDEN = json.load(f)


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


def cut(col, n, cuts):
    if cuts is None:
        return [[col]]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[col.sliced(lo, hi - lo)] for lo, hi in zip(bounds[:-1], bounds[1:])]


# ---- parent sets --------------------------------------------------------------------------------------------------------------
def records_of(fps):
    """32-byte {hash_a, hash_b, count, 0} records of the given (fa, fb) pairs in device memory"""
    recs = np.zeros((len(fps), 4), np.uint64)
    for i, (fa, fb) in enumerate(fps):
        recs[i] = (fa, fb, 1, 0)
    return to_device(recs.reshape(-1)) if len(fps) else None


def set_records(st, fps, i=0):
    d = records_of(fps)
    st.key_probe_set_parent(i, d.data_ptr() if d is not None else None, len(fps))


def set_hand_made(st, values, i=0, key=KEY):
    set_records(st, [fpr.fingerprint(key, v) for v in ex.as_bytes(values) if v is not None], i)


def set_exported(st, values, i=0, key=KEY, exact=False, layout=pa.string()):
    """the parent's column walked under a DISTINCT spec of a plan with the same key; its export goes in"""
    plan = T.Plan([spec(T.DISTINCT, 0, flags=T.FLAG_EXACT_KEYS if exact else 0)])
    plan.set_fingerprint_key(key)
    parent = T.State(plan)
    if len(values):
        parent.update([column(array(values, layout))])
    assert parent.distinct_record_bytes(0) == 32 or not len(values)  # (a state without a batch knows no key type)
    ptr, counts = parent.distinct_export(0, 1)
    st.key_probe_set_parent(i, ptr, counts[0])


def digest_of(values, key=KEY):
    return ex.parent_digest(key, values)


def plan_of(bounds=((10000, 256),), columns=None, extra=(), key=KEY):
    plan = T.Plan([spec(T.KEY_PROBE, columns[k] if columns else 0) for k in range(len(bounds))] + list(extra))
    plan.set_fingerprint_key(key)
    for k, (keys, size) in enumerate(bounds):
        plan.set_key_probe_strings(k, keys, size)
    return plan


def read(st, i=0):
    summary, entries = st.key_probe_strings(i)
    got = dict(summary, entries=entries)
    assert got["seen"] == got["non_null"] + got["null_rows"]
    assert got["non_null"] == got["matched"] + got["missing_rows"]
    assert got["missing_rows"] == got["counted"] + got["overflow_rows"] + got["long_rows"]
    assert got["counted"] == sum(entries.values()) and got["missing_keys"] == len(entries)
    return got


def exact(child, parent, max_value_bytes=256, key=KEY):
    want = ex.walk(child, parent, max_value_bytes)
    del want["within_bound"]
    want.update(max_value_bytes=max_value_bytes, parent_digest=digest_of(parent, key), route=5 if want["parent_keys"] else 0)
    return want


def check(child, parent, layout=pa.string(), max_value_bytes=256, bound=10000, mem=T.MEM_DEVICE, cuts=None, offset=0,
          exported=True):
    """child / parent: lists of bytes / str / None"""
    T.init()
    plan = plan_of(((bound, max_value_bytes),))
    st = T.State(plan)
    (set_exported if exported else set_hand_made)(st, parent)
    if len(child):  # (no rows: the state is read as it was made)
        arr = array([b"pad"] * offset + list(child), layout)
        col = column(arr, mem).sliced(offset, len(child))
        for b in cut(col, len(child), cuts):
            st.update(b)
    want = exact(child, parent, max_value_bytes)
    got = read(st)
    assert got == want and list(got["entries"]) == list(want["entries"])  # (the order too: ascending bytewise)
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.matches, r.distinct) == (want["seen"], want["non_null"], want["matched"], want["missing_keys"])
    return st, plan, want


def values_of(rng, n, n_distinct, null_rate=0.0, lengths=(1, 2, 3, 5, 8, 12, 13)):
    pool = [bytes(rng.integers(97, 123, lengths[i % len(lengths)], dtype=np.uint8)) + b"%d" % i for i in range(n_distinct)]
    picks = rng.integers(0, n_distinct, n)
    nulls = rng.random(n) < null_rate
    return [None if nulls[i] else pool[picks[i]] for i in range(n)], pool


# ---- lengths and layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exported", [True, False], ids=["export", "hand-made"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_lengths_at_the_fingerprints_block_edges(layout, exported):
    """every length among the matched and among the missing values; 300 bytes: matched when it is in the parent, a long
    row when it is not"""
    hit = [b"h" * n for n in LENGTHS]
    miss = [b"m" * n for n in LENGTHS if n]
    child = (hit + miss + [None]) * 3
    st, _, want = check(child, hit + [None], layout, exported=exported)
    assert want["matched"] == 3 * len(hit) and want["long_rows"] == 3 and b"m" * 33 in want["entries"]
    # values whose bytes all differ: the order of the bytes within a block and of the blocks (a dictionary's entries
    # and a view's inline values among them)
    rng = np.random.default_rng(21)
    hit = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in LENGTHS if n]
    miss = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in LENGTHS if n]
    swapped = [v[8:16] + v[:8] + v[16:] for v in hit if len(v) >= 16] + [v[::-1] for v in hit if len(v) > 1]
    child = hit + miss + swapped + [None] + hit
    st, _, want = check(child, hit + [None], layout, exported=exported)
    assert want["matched"] == 2 * len(hit) and want["long_rows"] == 3
    assert all(v in want["entries"] for v in swapped if len(v) <= 256)
    # the empty string missing, and a parent that holds nothing but it
    check([b"", b"a", b"", None], [b"a"], layout, exported=exported)
    check([b"", b"a", b"", None], [b""], layout, exported=exported)


@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_the_byte_bound(layout):
    child = [b"x" * 40, b"x" * 41, b"y" * 40, b"y" * 41, b"z" * 300, b"x" * 41]
    st, _, want = check(child, [b"y" * 41, b"z" * 300], layout, max_value_bytes=40)
    assert want["entries"] == {b"x" * 40: 1, b"y" * 40: 1} and want["long_rows"] == 2 and want["matched"] == 2
    st, _, want = check([b"ab", b"a", b""], [], layout, max_value_bytes=1)
    assert want["entries"] == {b"": 1, b"a": 1} and want["long_rows"] == 1
    check([b"q" * 256, b"q" * 257], [], layout, max_value_bytes=256)


# ---- offsets, validity, row counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
@pytest.mark.parametrize("offset", [1, 7, 63])
def test_sliced_arrays(layout, offset):
    rng = np.random.default_rng(offset)
    child, pool = values_of(rng, 700, 40, 0.3)
    check(child, pool[::2], layout, offset=offset)


@pytest.mark.parametrize("null_rate", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 70_001])
def test_row_counts_and_null_rates(n, null_rate):
    """0 % NULLs: a column without a validity buffer; 70 001 rows: several workgroups and a ragged tail"""
    rng = np.random.default_rng(n)
    child, pool = values_of(rng, n, 50, null_rate)
    check(child, pool[:30] + [None])


# ---- the set ----------------------------------------------------------------------------------------------------------------------
def test_the_empty_set_a_set_of_one_key_and_duplicate_records():
    rng = np.random.default_rng(1)
    child, pool = values_of(rng, 3000, 20, 0.2)
    for exported in (True, False):
        st, _, want = check(child, [], exported=exported)
        assert want["route"] == 0 and want["matched"] == 0 and want["parent_keys"] == 0
        st, _, want = check(child, [pool[3]], exported=exported)
        assert want["route"] == 5 and want["parent_keys"] == 1 and want["matched"] > 0
    st, _, want = check(child, [pool[3], pool[4], pool[3], pool[3], None, pool[4]], exported=False)
    assert want["parent_keys"] == 2


def test_a_record_with_a_marker_word_is_refused_and_the_state_is_left_without_a_set():
    T.init()
    st = T.State(plan_of())
    good = [fpr.fingerprint(KEY, b"a"), fpr.fingerprint(KEY, b"b")]
    set_records(st, good)
    for bad in ((M64, 5), (5, M64), (M64, M64)):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*1 records.*free-slot marker"):
            set_records(st, good + [bad])
        assert read(st)["route"] == 0
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
            st.update([column(array([b"a"]))])
        set_records(st, good)
    st.update([column(array([b"a", b"c"]))])
    got = read(st)
    assert got["matched"] == 1 and got["entries"] == {b"c": 1} and got["route"] == 5


def test_probe_chains_that_wrap_and_fingerprints_that_share_a_word():
    """hand-made records: eight fingerprints whose fa & mask is the table's last slot (the chain wraps past its end), and
    two that are equal in fa and differ in fb; the child holds the values of some of them"""
    T.init()
    child = [b"v%d" % i for i in range(40)]
    fps = [fpr.fingerprint(KEY, v) for v in child]
    slots = 64  # the smallest power of two >= 2 * 32 records
    crowd = [((fa & ~(slots - 1)) | (slots - 1), fb ^ 4) for fa, fb in fps[8:16]]    # not the fingerprints of any value
    twins = [(fps[0][0], fps[0][1] ^ 1), (fps[1][0], fps[1][1] ^ 2)]                  # fa of a child value, another fb
    present = fps[0:1] + fps[20:40]
    recs = crowd + twins + present + [fps[0]]                                          # 32 records, one a duplicate
    assert len(recs) == 32
    st = T.State(plan_of())
    set_records(st, recs)
    st.update([column(array(child))])
    got = read(st)
    assert got["parent_keys"] == 31 and got["route"] == 5
    assert got["parent_digest"] == sum(exk.mix64(exk.mix64(a ^ SALT) ^ b) for a, b in set(recs)) & M64
    assert got["matched"] == 21 and got["entries"] == {v: 1 for v in child[1:20]}
    # a table where every record shares fa & mask: the chain runs through the whole table, and a missing key still ends
    st = T.State(plan_of())
    set_records(st, [((fa & ~7) | 5, fb ^ 4) for fa, fb in fps[:4]])
    st.update([column(array(child))])
    assert read(st)["matched"] == 0 and read(st)["missing_keys"] == 40


def test_a_set_made_under_another_key_matches_nothing():
    T.init()
    child = [b"a", b"b", None, b"a"]
    st = T.State(plan_of())
    set_exported(st, [b"a", b"b"], key=bytes(16))
    st.update([column(array(child))])
    got = read(st)
    assert got["matched"] == 0 and got["entries"] == {b"a": 2, b"b": 1} and got["parent_keys"] == 2
    # the parent's spec with EXACT_KEYS exports fingerprints all the same
    st = T.State(plan_of())
    set_exported(st, [b"a", b"b", None], exact=True)
    st.update([column(array(child))])
    assert read(st) == exact(child, [b"a", b"b"])
    for layout in LAYOUTS[1:]:  # a parent of another layout than the child's
        st = T.State(plan_of())
        set_exported(st, [b"a", None, b"zz"], layout=layout)
        st.update([column(array(child))])
        assert read(st) == exact(child, [b"a", b"zz"])


# ---- missing keys -----------------------------------------------------------------------------------------------------------------
def test_64_distinct_missing_keys_in_one_wave():
    """past the four combining rounds: the other 60 lanes insert for themselves"""
    child = [b"k%02d" % (i % 64) for i in range(64 * 5)]
    check(child, [b"other"])
    check(child[:64], [child[5]])


@functools.lru_cache(maxsize=None)
def crowd_of_one_lds_place(n_values):
    """n_values distinct values whose fingerprints under KEY share fa & 1023, the place their probing of the workgroup's
    1024-slot table starts from: the first such crowd among b"c000000", b"c000001", .."""
    places = {}
    for i in range(200_000):
        v = b"c%06d" % i
        crowd = places.setdefault(fpr.fingerprint(KEY, v)[0] & 1023, [])
        crowd.append(v)
        if len(crowd) == n_values:
            return crowd
    raise AssertionError("no crowd found")


@pytest.mark.parametrize("layout", LAYOUTS[:3], ids=str)
def test_a_full_lds_neighbourhood_sends_keys_to_the_global_table(layout):
    """A workgroup takes one 256-row stride of a table of this size and its LDS table probes 8 slots from fa & 1023, so
    more distinct keys than a table of 1024 slots holds never meet in one workgroup here.  Twelve distinct missing values
    that share fa & 1023 do: the first eight take the neighbourhood, the other four find it full and go to the global
    table directly, with the bytes and the weight of the lane that leads them.  The twelve lie in ONE workgroup's 256
    rows, in every wave, repeated unevenly (so leaders carry weights above one), between matched rows and NULLs; the other workgroups hold them too, so direct inserts and the LDS tables' flushes meet in the global
    table."""
    crowd = crowd_of_one_lds_place(12)
    assert len(set(fpr.fingerprint(KEY, v)[0] & 1023 for v in crowd)) == 1 and len(set(crowd)) == 12
    rng = np.random.default_rng(31)
    block = []
    for wave in range(4):
        rows = [crowd[(wave + 5 * j) % 12] for j in range(40)] + [crowd[wave]] * 9 + [b"hit"] * 10 + [None] * 5
        block += [rows[i] for i in rng.permutation(64)]
    assert len(block) == 256
    child = block * 3 + block[:100]
    st, _, want = check(child, [b"hit"], layout)
    assert want["missing_keys"] == 12 and want["overflow_rows"] == 0
    # the same crowd with one of its values in the parent, at the byte bound of its values, in a sliced array
    check(child, [b"hit", crowd[0]], layout, max_value_bytes=7, offset=7)


def test_many_distinct_missing_keys_across_workgroups():
    """3000 distinct missing keys over 79 workgroups: every workgroup flushes a few hundred LDS slots into one global
    table; nothing overflows"""
    rng = np.random.default_rng(3)
    child, pool = values_of(rng, 20_000, 3000)
    st, _, want = check(child, pool[:10], bound=10000)
    assert want["missing_keys"] > 2 * 1024 and want["overflow_rows"] == 0


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_max_missing_keys_and_one_above(extra):
    n = 200 + extra
    child = [b"key-%04d" % i for i in np.random.default_rng(4).permutation(n)] * 2
    T.init()
    st = T.State(plan_of(((200, 256),)))  # 512 slots
    set_hand_made(st, [b"p"])
    st.update([column(array(child))])
    got, true = read(st), ex.walk(child, [b"p"])
    # (one above: the table has 2 x max_missing_keys slots, so the key has its slot and nothing overflows; missing_keys
    # reports it and the caller compares, as for integer keys)
    assert got["missing_keys"] == n and got["overflow_rows"] == 0
    assert got["entries"] == true["entries"] and list(got["entries"]) == list(true["entries"])


def test_more_missing_keys_than_the_global_table_has_slots():
    rng = np.random.default_rng(5)
    child, pool = values_of(rng, 30_000, 400, 0.1)
    T.init()
    st = T.State(plan_of(((16, 256),)))  # 32 slots
    set_hand_made(st, pool[:5])
    st.update([column(array(child))])
    got, true = read(st), ex.walk(child, pool[:5])
    assert got["overflow_rows"] > 0 and got["missing_keys"] <= 32
    assert (got["seen"], got["non_null"], got["matched"]) == (true["seen"], true["non_null"], true["matched"])
    assert all(0 < c <= true["entries"][k] for k, c in got["entries"].items())


# ---- dictionaries -----------------------------------------------------------------------------------------------------------------
def dictionary(indices, entries, mask=None):
    return pa.DictionaryArray.from_arrays(pa.array(indices, pa.int32(), mask=None if mask is None else ~np.asarray(mask)),
                                          pa.array(entries, pa.string()))


def test_dictionary_children():
    """repeated values among the entries, a NULL entry, an entry no row refers to, different dictionaries across batches"""
    T.init()
    rng = np.random.default_rng(6)
    entries = ["a", "b", "a", None, "unused", "c", "b"]
    idx = rng.integers(0, 7, 5000)
    idx[idx == 4] = 0
    mask = rng.random(5000) >= 0.1
    first = dictionary(idx, entries, mask)
    second = dictionary(rng.integers(0, 3, 3000), ["c", "zz", "a"])
    logical = first.to_pylist() + second.to_pylist()
    for mem in (T.MEM_DEVICE, T.MEM_HOST):
        st = T.State(plan_of())
        set_exported(st, ["a", "zz", "never"])
        st.update([column(first, mem)])
        st.update([column(second, mem)])
        want = exact(logical, ["a", "zz", "never"])
        assert read(st) == want and b"unused" not in want["entries"]


def test_dictionary_indices_outside_the_dictionary_are_null_rows():
    T.init()
    idx = np.array([0, 1, 5, -1, 2, 2**31 - 1, 1], np.int32)
    entries = on_device(T.Column.from_arrow(pa.array(["a", "b", "c"])))
    col = T.Column(T.DICT32_UTF8, len(idx), values=padded(idx), mem=T.MEM_DEVICE, dictionary=entries)
    st = T.State(plan_of())
    set_hand_made(st, ["a"])
    st.update([col])
    got = read(st)
    assert (got["seen"], got["null_rows"], got["matched"], got["entries"]) == (7, 3, 1, {b"b": 2, b"c": 1})


# ---- batching and feeding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=str)
def test_batching_independence(layout, mem):
    rng = np.random.default_rng(7)
    child, pool = values_of(rng, 40_000, 300, 0.05)
    for cuts in (None, [1, 64, 65, 5000, 5001, 39_999], 8192):
        check(child, pool[::3], layout, mem=mem, cuts=cuts)


def test_mixed_layouts_of_one_column_and_two_specs_on_it():
    """a state takes one layout per column (tgx_update's rule for every kind), so the layouts of one logical column meet
    as states that merge -- by bytes"""
    T.init()
    rng = np.random.default_rng(8)
    child, pool = values_of(rng, 8000, 100, 0.1)
    plan = plan_of(((10000, 256), (10000, 4)), columns=[0, 0])
    states = []
    for k, layout in enumerate(LAYOUTS):
        st = T.State(plan)
        set_exported(st, pool[:50], 0)
        set_hand_made(st, pool[50:], 1)
        st.update([column(array(child[2000 * k:2000 * (k + 1)], layout))])
        states.append(st)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*changed type between batches"):
        states[0].update([column(array(child[:10], LAYOUTS[1]))])
    states[0].merge(states[1:])
    assert read(states[0], 0) == exact(child, pool[:50]) and read(states[0], 1) == exact(child, pool[50:], 4)


# ---- the state algebra ----------------------------------------------------------------------------------------------------------------
def test_reset_half_way_reads_blobs_and_merges():
    T.init()
    rng = np.random.default_rng(9)
    child, pool = values_of(rng, 30_000, 200, 0.1)
    child[7] = b"L" * 40
    parent = pool[:120]
    plan = plan_of(((10000, 32),))
    want = exact(child, parent, 32)
    parts = [child[:10_000], child[10_000:20_000], child[20_000:]]
    st = T.State(plan)
    set_exported(st, parent)
    st.update([column(array(parts[0]))])
    assert read(st) == exact(parts[0], parent, 32)  # read half-way, then on
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*before the state's first batch"):
        set_exported(st, parent)
    for p in parts[1:]:
        st.update([column(array(p))])
    assert read(st) == want
    st.reset()  # keeps the set
    empty = read(st)
    assert (empty["seen"], empty["entries"], empty["route"], empty["parent_digest"]) == (0, {}, 5, want["parent_digest"])
    st.update([column(array(child))])
    assert read(st) == want
    states = []
    for p in parts:
        s = T.State(plan)
        set_hand_made(s, parent)
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
        set_hand_made(back, parent[:-1])
    set_hand_made(back, parent)
    back.update([column(array(child))])
    doubled = read(back)
    assert doubled["entries"] == {k: 2 * c for k, c in want["entries"].items()} and doubled["long_rows"] == 2
    other = T.State(plan)
    set_hand_made(other, parent[1:])
    other.update([column(array(parts[0]))])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different parent sets"):
        st.merge([other])
    # the blob carries the plan's key: a plan with another key refuses it; so does one with another max_value_bytes
    import struct

    assert struct.unpack_from("<I", blob, 36)[0] == 1 and blob[40:56] == KEY  # (the head's { u32 keyed, u8 key[16] })
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fingerprint key"):
        T.State.deserialize(plan_of(((10000, 32),), key=bytes(16)), blob)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(plan_of(((10000, 33),)), blob)


def test_threaded_ranks_share_a_fingerprint_key():
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    T.init()
    rng = np.random.default_rng(10)
    n, world = 40_000, 2
    child, pool = values_of(rng, n, 300, 0.1)
    parent = pool[:200]
    want = exact(child, parent)
    whole = [column(array(child))]
    plan = plan_of(extra=[spec(T.COUNT, 0)])
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(n, world, rank)
            st = T.State(plan)
            set_hand_made(st, parent)
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


def test_a_state_without_a_set_and_other_column_types():
    """the refused batches go to the very state that is read afterwards"""
    T.init()
    st = T.State(plan_of(((100, 16), (100, 16)), columns=[0, 0]))
    set_hand_made(st, ["a"], 0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*needs its parent set"):
        st.update([column(array(["a", "b"]))])
    set_hand_made(st, ["b"], 1)
    n = 1000
    refused = [(pa.array(np.arange(n, dtype=np.int64)), "integers"), (pa.array(np.arange(n, dtype=np.int32)), "integers"),
               (pa.array(np.arange(n, dtype=np.float64)), "Float64"), (pa.array(np.arange(n, dtype=np.float32)), "Float32"),
               (pa.array(np.arange(n, dtype=np.uint64)), "UInt64"), (pa.array(np.arange(n) % 2 == 0), "Boolean")]
    for arr, name in refused:
        for mem in (T.MEM_HOST, T.MEM_DEVICE):
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*KEY_PROBE.*" + name):
                st.update([column(arr, mem)])
    assert read(st)["seen"] == 0
    st.update([column(array(["a", "b", "c", None]))])
    assert read(st, 0)["entries"] == {b"b": 1, b"c": 1} and read(st, 1)["entries"] == {b"a": 1, b"c": 1}
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_key_probe_entries_bytes"):
        st.key_probe(0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not counted"):
        st.key_probe_pairs(0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*does not gather rows"):
        st.key_probe_rows(0)


# ---- the guarantee and its boundary ---------------------------------------------------------------------------------------------------
def test_two_values_of_one_fingerprint_count_as_matched():
    """All counts are exact over FINGERPRINTS.  Whoever knows the plan's key can write down two distinct values of one
    fingerprint (fp_reference.colliding_pair): with one in the parent and the other in the child, the child's row is
    MATCHED.  The data's producer does not know the key; under any other key the same two values are told apart."""
    T.init()
    a, b = fpr.colliding_pair(KEY, np.random.default_rng(11))
    assert a != b
    for exported in (True, False):
        st = T.State(plan_of())
        (set_exported if exported else set_hand_made)(st, [a])
        st.update([column(array([b, a, b"plain"]))])
        got = read(st)
        assert got["matched"] == 2 and got["entries"] == {b"plain": 1} and got["parent_keys"] == 1
    other = bytes(range(2, 18))
    st = T.State(plan_of(key=other))
    set_exported(st, [a], key=other)
    st.update([column(array([b, a, b"plain"]))])
    assert read(st)["matched"] == 1 and read(st)["entries"] == {b: 1, b"plain": 1}


# ---- no side effects -------------------------------------------------------------------------------------------------------------------
def test_the_kind_leaves_the_other_kinds_bit_for_bit():
    T.init()
    rng = np.random.default_rng(12)
    child, pool = values_of(rng, 50_000, 500, 0.1)
    cols = [column(array(child)), column(pa.array(rng.standard_normal(50_000)))]
    others = [spec(T.COUNT, 0), spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.NUMERIC_STATS, 1, flags=T.FLAG_VARIANCE),
              spec(T.VALUE_COUNTS, 0)]
    alone_plan = T.Plan(others)
    alone_plan.set_fingerprint_key(KEY)
    alone_plan.set_value_counts(3)
    alone = T.State(alone_plan)
    alone.update(cols)
    ref = alone.finalize()
    plan = plan_of(extra=others)
    plan.set_value_counts(4)
    st = T.State(plan)
    set_exported(st, pool[:100])
    st.update(cols)
    res = st.finalize()
    assert read(st) == exact(child, pool[:100])
    assert st.value_counts(4) == alone.value_counts(3)
    for got, r in zip(res[1:], ref):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(r), ctypes.sizeof(r))


def test_a_plan_without_a_strings_spec_profiles_no_such_launch():
    T.init()
    ints = pa.array(np.arange(5000, dtype=np.int64) % 50)
    launches = []
    for strings in (False, True):
        plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.COUNT, 0)] + ([spec(T.KEY_PROBE, 1)] if strings else []))
        plan.set_key_probe(0, 100)
        if strings:
            plan.set_key_probe_strings(2, 100, 16)
        st = T.State(plan)
        st.profile_enable(True)
        recs = np.ones((10, 2), np.uint64)
        recs[:, 0] = np.arange(10) * 1_000_003
        d = to_device(recs.reshape(-1))
        st.key_probe_set_parent(0, d.data_ptr(), 10)
        if strings:
            set_records(st, [fpr.fingerprint(plan.fingerprint_key(), b"a")], 2)
        cols = [column(ints)] + ([column(array(["a", "b"] * 2500))] if strings else [])
        st.update(cols)
        st.finalize()
        launches.append((st.profile_get("key_probe")["launches"], st.profile_get("key_probe_build")["launches"]))
    assert launches == [(1, 1), (2, 2)]


# ---- end to end: ForeignKeyConstraint through ValidationSuite.run(.., tables=..) ------------------------------------------------------
def run_constraint(constraint, tables, builder=False, as_json=False):
    """(status of the constraint, its metric, its message) of a one-constraint suite"""
    cb = S.Check.builder("c").level(S.Level.ERROR)
    cb = cb.foreign_key(constraint.child_column(), constraint.parent_column()) if builder else cb.constraint(constraint)
    suite = S.ValidationSuite.builder("s").check(cb.build()).build()
    if as_json:
        suite = S.ValidationSuite(json.loads(json.dumps(suite.spec)))
    r = suite.run(None, tables=tables)
    m = r.report.metrics
    assert m.total_checks == 1 and m.passed_checks + m.failed_checks == 1
    metric = m.custom_metrics.get("c.foreign_key")
    if m.passed_checks:
        assert r.is_success() and not r.report.issues
        return "success", metric, None
    assert len(r.report.issues) == 1 and r.report.issues[0].constraint_name == "foreign_key"
    message = r.report.issues[0].message
    return ("error" if message.startswith("Error evaluating constraint: ") else "failure"), metric, message


def table_of(name, values, layout):
    if layout == "dictionary":
        col = pa.array(values, pa.string()).dictionary_encode()
        col = col.cast(pa.dictionary(pa.int32(), pa.string()))
    else:
        col = pa.array(values, layout)
    return pa.table({name: col, "n": pa.array(range(len(values)), pa.int64())})


@pytest.mark.parametrize("layouts", [(pa.string(), pa.string()), (pa.large_string(), pa.string()),
                                     (pa.string_view(), pa.string()), ("dictionary", pa.string()),
                                     (pa.string(), pa.large_string()), (pa.string(), pa.string_view()),
                                     (pa.string(), "dictionary")], ids=str)
@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_the_golden_tables_through_the_suite(case, layouts):
    T.init()
    child, parent = GOLDEN["child_column"], GOLDEN["parent_column"]
    (ct, cc), (pt, pc) = child.split("."), parent.split(".")
    tables = {ct: table_of(cc, case["child"], layouts[0]), pt: table_of(pc, case["parent"], layouts[1])}
    c = S.ForeignKeyConstraint(child, parent)
    options = case["options"]
    if "allow_nulls" in options:
        c.allow_nulls(options["allow_nulls"])
    if "max_violations_reported" in options:
        c.max_violations_reported(options["max_violations_reported"])
    got = run_constraint(c, tables)
    examples = layouts[0] == pa.string()  # (the reference's collector downcasts to StringArray only)
    state = ex.walk(case["child"], case["parent"])
    assert got == ex.verdict(state, child, parent, options.get("allow_nulls", False),
                             options.get("max_violations_reported", 100), examples)
    if examples:
        assert got == (case["status"], case["metric"], case["message"])
        assert run_constraint(c, tables, as_json=True) == got
        if not options:
            assert run_constraint(c, tables, builder=True) == got
    else:
        assert got[:2] == (case["status"], case["metric"])


def test_bounds_that_are_overrun_through_the_suite():
    T.init()
    rng = np.random.default_rng(13)
    child, pool = values_of(rng, 20_000, 300, 0.05, lengths=(1, 30))
    child = [None if v is None else v.decode() for v in child]
    parent = [v.decode() for v in pool[:100]]
    tables = {"orders": table_of("code", child, pa.string()), "codes": table_of("code", parent, pa.string())}
    state = ex.walk(child, parent)
    total = float(state["missing_rows"] + state["null_rows"])
    for allow in (False, True):
        c = S.ForeignKeyConstraint("orders.code", "codes.code").allow_nulls(allow).max_violations_reported(3)
        assert run_constraint(c, tables) == ex.verdict(state, "orders.code", "codes.code", allow, 3)
    # max_missing_keys overrun: the verdict and the metric stand, unique reads "at least"
    status, metric, message = run_constraint(S.ForeignKeyConstraint("orders.code", "codes.code").max_missing_keys(16), tables)
    assert (status, metric) == ("failure", total) and "unique: at least " in message and "Examples: [" in message
    # max_value_bytes overrun: the long keys are counted, not kept
    c = S.ForeignKeyConstraint("orders.code", "codes.code").max_value_bytes(8)
    short = ex.walk(child, parent, 8)
    assert short["long_rows"] > 0
    assert run_constraint(c, tables) == ex.verdict(short, "orders.code", "codes.code")
    assert "unique: at least %d)" % short["missing_keys"] in run_constraint(c, tables)[2]
    # the mixed pair stays the old error; a Binary column is refused by this layer
    tables["orders"] = tables["orders"].append_column("id", pa.array(range(len(child)), pa.int64()))
    tables["orders"] = tables["orders"].append_column("raw", pa.array([b"x"] * len(child), pa.binary()))
    for pair, word in ((("orders.id", "codes.code"), "Utf8"), (("orders.code", "codes.n"), "Utf8"),
                       (("orders.raw", "codes.code"), "Binary")):
        status, _, message = run_constraint(S.ForeignKeyConstraint(*pair), tables)
        assert status == "error" and word in message and "not on the GPU path" in message
