"""TGX_CHECK_VALUE_COUNTS on the device, held against tests/exact_value_counts.py: the whole value -> count map and all
six counters are compared for equality with the exact per-row walk, on every route (integers through the workgroups'
LDS tables and their spill path, Utf8 / LargeUtf8 / Utf8View, dictionaries), every memory kind and batching, and every
way a state travels (read half-way, reset, merge, blob, tgx_allreduce).  Entropy and Gini figures are held to the
60-digit values within 2^-52 * ((n + 4) * H + 2)."""
import ctypes
import struct
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_value_counts as ex
import term_amd as T
from _lib_spec import spec
from gpu_util import to_device
from term_amd.value_counts import EntropyState, Histogram, OutOfBound

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
    col = T.Column.from_arrow(arr)
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


def plan_of(bounds=((10000, 256),), columns=None, extra=()):
    columns = columns or [0] * len(bounds)
    plan = T.Plan([spec(T.VALUE_COUNTS, c) for c in columns] + list(extra))
    for i, (max_distinct, max_value_bytes) in enumerate(bounds):
        plan.set_value_counts(i, max_distinct, max_value_bytes)
    return plan


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def read(st, i=0):
    summary, counts = st.value_counts(i)
    return dict(summary, counts=counts)


def check(arr, max_distinct=10000, max_value_bytes=256, mem=T.MEM_DEVICE, cuts=None, want=None):
    T.init()
    want = ex.walk(as_exact(arr.to_pylist()), max_value_bytes) if want is None else want
    plan = plan_of([(max_distinct, max_value_bytes)])
    st = feed(plan, cut([column(arr, mem)], len(arr), cuts))
    got = read(st)
    assert got == want and list(got["counts"]) == list(want["counts"])  # (the order too: ascending by value)
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.distinct, r.matches) == (want["seen"], want["non_null"], want["distinct"], want["counted"])
    return st, plan, want


def ints(values, type=pa.int64(), mask=None):
    return pa.array(values, type=type, mask=None if mask is None else ~np.asarray(mask))


# ---- integer columns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, SHARE - 1, SHARE, SHARE + 1])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    check(ints(rng.integers(-20, 20, n), mask=rng.random(n) >= 0.1))


def test_a_constant_column():
    check(ints(np.full(20_000, 42)))
    check(ints(np.full(20_000, 42), mask=np.arange(20_000) % 3 != 0))


@pytest.mark.parametrize("extra", [0, 1])
def test_all_rows_distinct_at_max_distinct_and_one_above(extra):
    n = 1000 + extra
    st, _, want = check(ints(np.random.default_rng(1).permutation(n) * 7 - 3000), max_distinct=1000)
    assert want["distinct"] == n and want["overflow_rows"] == 0  # one above: reported, the caller compares


def test_more_values_than_a_workgroups_lds_table_holds():
    """30 000 distinct values in 8 workgroups' shares of 15 000 rows: each share holds some 11 000 values, more than
    the 8192 LDS slots take, so rows go to the global table directly (the spill path); nothing overflows"""
    rng = np.random.default_rng(2)
    v = rng.integers(0, 30_000, 120_000) * 1_000_003 - 5
    st, _, want = check(ints(v), max_distinct=40_000)
    assert want["distinct"] > 2 * 8192 and want["overflow_rows"] == 0


def test_more_values_than_the_global_table_has_slots():
    rng = np.random.default_rng(3)
    v = rng.integers(0, 200, 30_000)
    T.init()
    st = feed(plan_of([(16, 256)]), [[column(ints(v))]])  # 32 slots
    got, true = read(st), ex.walk(v.tolist())
    assert got["overflow_rows"] > 0 and got["distinct"] <= 32
    assert got["counted"] + got["overflow_rows"] + got["long_rows"] == got["non_null"] == 30_000
    assert got["counted"] == sum(got["counts"].values())
    assert all(0 < c <= true["counts"][k] for k, c in got["counts"].items())


def test_the_marker_value_and_the_extremes():
    v = [-1, -1, I64_MIN, I64_MAX, 0, -1, I64_MAX, -2, 1, None, -1]
    check(ints(v * 50))
    check(ints([-1] * 300))
    check(ints([None, -1, None] * 100))


NARROW = [(pa.int8(), [-128, -1, 0, 127, -1]), (pa.int16(), [-32768, -1, 32767, 5]), (pa.int32(), [-2**31, -1, 2**31 - 1, 7]),
          (pa.uint8(), [0, 255, 128]), (pa.uint16(), [0, 65535, 32768]), (pa.uint32(), [0, 2**31, 2**32 - 1, 2**31 + 1]),
          (pa.date32(), [-1, 0, 19000])]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("type,values", NARROW, ids=[str(t) for t, _ in NARROW])
def test_narrow_types_are_widened(type, values, mem):
    rng = np.random.default_rng(5)
    picks = [values[i] for i in rng.integers(0, len(values), 700)]
    arr = pa.array([None if rng.random() < 0.1 else p for p in picks], type=pa.int32() if type == pa.date32() else type)
    want = ex.walk(as_exact(arr.to_pylist()))
    check(arr.cast(type) if type == pa.date32() else arr, mem=mem, want=want)


@pytest.mark.parametrize("nulls", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("offset", [0, 1, 8, 9])
def test_validity_and_arrow_offsets(offset, nulls):
    rng = np.random.default_rng(offset * 10 + int(nulls * 2))
    n = 3000
    arr = ints(rng.integers(0, 9, n), mask=rng.random(n) >= nulls).slice(offset)
    check(arr)
    check(arr, mem=T.MEM_HOST)


# ---- string columns -------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 12, 13, 15, 16, 17, 32, 33, 40, 41]
WORDS = ["x" * k for k in LENGTHS] + ["y" * k for k in LENGTHS[1:]] + ["Zoë", "a\x00b", "user@example.com"]


def words(rng, n, null=0.1):
    return [None if rng.random() < null else WORDS[i] for i in rng.integers(0, len(WORDS), n)]


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("type", [pa.string(), pa.large_string(), pa.string_view()], ids=str)
def test_string_layouts_and_lengths(type, mem):
    """the empty string is a value; lengths 15 / 16 / 17 / 32 / 33 straddle the fingerprint's blocks; 40 is
    max_value_bytes, 41 a long row; a Utf8View holds values of up to 12 bytes inline"""
    rng = np.random.default_rng(6)
    arr = pa.array(words(rng, 5000), type=type)
    _, _, want = check(arr, max_value_bytes=40, mem=mem)
    assert want["long_rows"] > 0 and b"" in want["counts"] and b"x" * 40 in want["counts"]
    check(arr.slice(3), max_value_bytes=40, mem=mem)


def test_a_view_column_with_two_data_buffers():
    rng = np.random.default_rng(7)
    vals = words(rng, 2000, null=0.0)
    bufs, fill, views = [bytearray(), bytearray()], 0, bytearray()
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
    st = feed(plan_of([(100, 40)]), [[col.sliced(0, len(vals))]])
    assert read(st) == ex.walk(as_exact(vals), 40)


def dictionary(indices, entries, mask=None):
    return pa.DictionaryArray.from_arrays(pa.array(indices, pa.int32(), mask=None if mask is None else ~np.asarray(mask)),
                                          pa.array(entries, pa.string()))


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
def test_a_dictionary_with_unused_null_and_repeated_entries(mem):
    rng = np.random.default_rng(8)
    entries = ["a", None, "b", "a", "unused", "", "x" * 41, "b"]  # 0 and 3, 2 and 7 repeat a value; 1 is NULL; 6 is long
    idx = rng.choice([0, 1, 2, 3, 5, 6, 7], 4000)
    arr = dictionary(idx, entries, mask=rng.random(4000) >= 0.1)
    _, _, want = check(arr, max_value_bytes=40, mem=mem)
    assert set(want["counts"]) == {b"a", b"b", b""} and want["long_rows"] > 0


def test_batches_with_different_dictionaries_unite_by_value():
    T.init()
    a = dictionary([0, 1, 1, 2], ["red", "green", "blue"])
    b = dictionary([0, 0, 1, 2, 2], ["blue", "yellow", "red"])
    st = feed(plan_of(), [[column(a)], [column(b)]])
    assert read(st) == ex.walk(as_exact(a.to_pylist() + b.to_pylist()))
    assert read(st)["counts"] == {b"blue": 3, b"green": 2, b"red": 3, b"yellow": 1}


def test_a_dictionary_above_16384_entries():
    rng = np.random.default_rng(9)
    entries = ["k%05d" % i for i in range(20_000)]
    check(dictionary(rng.integers(0, 20_000, 50_000), entries), max_distinct=30_000)


# ---- batching and the ways a state travels ---------------------------------------------------------------------------------
N_BIG = 300_000


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(10)
    iv = ints(rng.zipf(1.3, N_BIG) % 5000 - 100, mask=rng.random(N_BIG) >= 0.05)
    sv = pa.array(["c%d" % k if k % 7 else None for k in rng.integers(0, 300, N_BIG)], pa.string())
    dv = dictionary(rng.integers(0, 50, N_BIG), ["d%d" % (k % 40) for k in range(50)], mask=rng.random(N_BIG) >= 0.02)
    arrs = [iv, sv, dv]
    return arrs, [ex.walk(as_exact(a.to_pylist())) for a in arrs]


def big_plan(extra=()):
    return plan_of([(10000, 256)] * 3, columns=[0, 1, 2], extra=extra)


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192), (T.MEM_HOST_RETAINED, 8192),
                                      (T.MEM_HOST, [3, 8195, 8196, 200_001])])
def test_batching_independence(big, mem, cuts):
    arrs, want = big
    T.init()
    st = feed(big_plan(), cut([column(a, mem) for a in arrs], N_BIG, cuts))
    assert [read(st, i) for i in range(3)] == want


def test_state_algebra(big):
    arrs, want = big
    T.init()
    cols = [column(a) for a in arrs]
    parts = cut(cols, N_BIG, [100_000, 200_001])
    plan = big_plan()
    # read half-way, then on
    st = feed(plan, parts[:1])
    assert [read(st, i) for i in range(3)] == [ex.walk(as_exact(a.slice(0, 100_000).to_pylist())) for a in arrs]
    st.update(parts[1])
    st.update(parts[2])
    assert [read(st, i) for i in range(3)] == want
    # reset and refill
    st.reset()
    assert read(st)["seen"] == 0 and read(st)["counts"] == {}
    st.update(cols)
    assert [read(st, i) for i in range(3)] == want
    # merge of three states
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    assert [read(states[0], i) for i in range(3)] == want
    # a blob round trip into a fresh state; equal states give equal bytes
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    assert [read(back, i) for i in range(3)] == want and back.serialize() == blob == st.serialize()
    back.merge([st])
    assert read(back, 1)["counts"] == {k: 2 * c for k, c in want[1]["counts"].items()}
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(plan_of([(10000, 255)] * 3, columns=[0, 1, 2]), blob)


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(big, world, device_buffers):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    arrs, want = big
    T.init()
    whole = [column(a) for a in arrs]
    plan = big_plan(extra=[spec(T.COUNT, 0)])
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
            results[rank] = (res, [read(st, i) for i in range(3)])
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
        assert res[3].total == N_BIG


def test_two_specs_on_one_column_with_different_bounds(big):
    arrs, want = big
    T.init()
    st = feed(plan_of([(10000, 256), (64, 3)], columns=[0, 0]), [[column(arrs[1])]])
    assert read(st, 0) == want[1]
    tight = read(st, 1)
    assert tight["long_rows"] == ex.walk(as_exact(arrs[1].to_pylist()), 3)["long_rows"] > 0
    assert tight["counted"] + tight["overflow_rows"] + tight["long_rows"] == tight["non_null"]


def test_the_kind_leaves_the_other_kinds_bit_for_bit(big):
    arrs, want = big
    T.init()
    cols = [column(a) for a in arrs]
    others = [spec(T.COUNT, 0), spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.COUNT, 1), spec(T.DISTINCT, 1),
              spec(T.REGEX_MATCH, 1, pattern=r"^c1\d*$"), spec(T.DISTINCT, 2), spec(T.REGEX_MATCH, 2, pattern=r"^d[0-9]$")]
    alone = feed(T.Plan(others), [cols]).finalize()
    st = feed(big_plan(extra=others), [cols])
    res = st.finalize()
    assert [read(st, i) for i in range(3)] == want
    for got, ref in zip(res[3:], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))


def test_a_plan_without_the_kind_profiles_no_such_kernel(big):
    arrs, _ = big
    T.init()
    col = column(arrs[0])
    launches = []
    for plan in (T.Plan([spec(T.COUNT, 0)]), plan_of(extra=[spec(T.COUNT, 0)])):
        st = T.State(plan)
        st.profile_enable(True)
        st.update([col])
        st.finalize()
        launches.append(st.profile_get("value_counts")["launches"])
    assert launches == [0, 1]


def test_other_column_types_are_unsupported_and_the_state_stays_usable():
    """the refused batches go to the very state that is read afterwards"""
    T.init()
    n = 1000
    st = T.State(plan_of())
    for arr, name in ((pa.array(np.arange(n, dtype=np.float64)), "Float64"), (pa.array(np.arange(n, dtype=np.float32)), "Float32"),
                      (pa.array(np.arange(n, dtype=np.uint64)), "UInt64"), (pa.array(np.arange(n) % 2 == 0), "Boolean")):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*VALUE_COUNTS.*" + name):
            st.update([column(arr, T.MEM_HOST)])
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*VALUE_COUNTS.*" + name):
            st.update([column(arr, T.MEM_DEVICE)])
    assert read(st)["seen"] == 0
    st.update([column(ints(np.arange(n) % 10))])
    assert read(st)["counts"] == {k: 100 for k in range(10)} and read(st)["seen"] == n


# ---- end to end: the histogram and the entropy state of a pyarrow table ---------------------------------------------------------
def test_histogram_and_entropy_of_a_table(big):
    arrs, want = big
    T.init()
    table = pa.table({"n": arrs[0], "s": arrs[1], "d": arrs[2]})
    plan = big_plan()
    st = T.State(plan)
    for batch in table.to_batches(max_chunksize=8192):
        st.update([T.Column.from_arrow(batch.column(i)) for i in range(3)])
    for i in range(3):
        summary, counts = st.value_counts(i)
        hist = Histogram.from_counts(summary, counts, 10000)
        rows = ex.buckets(want[i])
        assert [(b.value, b.count, b.ratio) for b in hist.buckets] == rows
        assert (hist.total_count, hist.null_count) == (N_BIG, N_BIG - want[i]["non_null"])
        c = list(want[i]["counts"].values())
        nats, bits, gini = ex.exact_entropy(c), ex.exact_entropy(c, 2), ex.exact_gini(c)
        es = EntropyState.from_counts(summary, counts)
        assert es.value_counts == {t: n for t, n, _ in rows} and es.total_count == want[i]["counted"] and not es.truncated
        for got, exact in ((hist.entropy(), nats), (es.entropy(), bits), (es.gini_impurity(), gini)):
            print("value counts %d: %r against %s" % (i, got, exact))
            assert abs(got - float(exact)) <= ex.tolerance(len(c), exact)
        assert es.metrics()["unique_values"] == want[i]["distinct"]
        verdict = hist.most_common_ratio() < 0.5
        assert verdict == (rows[0][2] < 0.5)
        assert hist.failure_message("s", "no value holds half of the rows").startswith(
            "Histogram assertion 'no value holds half of the rows' failed for column 's'. Distribution: %d distinct values"
            % want[i]["distinct"])
    with pytest.raises(OutOfBound, match="%d distinct values \\(max_distinct 10\\)" % want[1]["distinct"]):
        Histogram.from_counts(*st.value_counts(1), max_distinct=10)


# ---- end to end: has_histogram and EntropyAnalyzer through the host layer ------------------------------------------------------
def run_checks(table, constraints, column_types=None):
    """every constraint in a check of its own -> [(status, metric, message)]"""
    import term_amd.suite as S

    T.init()
    sb = S.ValidationSuite.builder("histograms")
    for col, typ in (column_types or {}).items():
        sb.column_type(col, typ)
    for i, c in enumerate(constraints):
        sb.check(S.Check.builder("c%d" % i).level(S.Level.ERROR).constraint(c).build())
    res = sb.build().run(table)
    issues = {i.check_name: i for i in res.report.issues}
    out = []
    for i in range(len(constraints)):
        key = "c%d.histogram" % i
        if "c%d" % i in issues:
            out.append(("issue", issues["c%d" % i].metric, issues["c%d" % i].message))
        elif key in res.report.metrics.custom_metrics:
            out.append(("success", res.report.metrics.custom_metrics[key], None))
        else:
            out.append(("skipped", None, None))
    return out, res


def test_has_histogram_on_a_table(big):
    import term_amd.suite as S

    A, M = S.Assertion, S.HistogramMeasure
    arrs, want = big
    table = pa.table({"n": arrs[0], "s": arrs[1], "d": arrs[2], "f": pa.array(np.arange(N_BIG, dtype=np.float64)),
                      "day": pa.array(np.arange(N_BIG, dtype=np.int32)).cast(pa.date32()),
                      "nothing": pa.array([None] * N_BIG, pa.string())})
    rows = [ex.buckets(w) for w in want]
    top = rows[1][0][2]
    constraints = [
        S.HistogramConstraint("s", [M.most_common_ratio(A.LessThan(0.5)), M.bucket_count(A.Equals(want[1]["distinct"]))]),
        S.HistogramConstraint("s", [M.most_common_ratio(A.LessThan(top))], "no value above the top ratio"),
        S.HistogramConstraint("n", [M.value_ratio(rows[0][0][0], A.Equals(rows[0][0][2])), M.top_n_ratio(3, A.GreaterThan(0.3))]),
        S.HistogramConstraint("d", [M.null_ratio(A.Between(0.01, 0.03)), M.least_common_ratio(A.Equals(rows[2][-1][2]))]),
        S.HistogramConstraint("s", [M.bucket_count(A.GreaterThan(0))], max_distinct=10),
        S.HistogramConstraint("f", [M.bucket_count(A.GreaterThan(0))]),
        S.HistogramConstraint("day", [M.bucket_count(A.GreaterThan(0))]),
        S.HistogramConstraint("nothing", [M.bucket_count(A.GreaterThan(0))]),
        S.HistogramConstraint("missing", [M.bucket_count(A.GreaterThan(0))]),
    ]
    got, res = run_checks(table, constraints)
    for k, col in ((0, 1), (2, 0), (3, 2)):
        c = list(want[col]["counts"].values())
        exact = ex.exact_entropy(c)
        print("histogram metric %d: %r against %s" % (k, got[k][1], exact))
        assert got[k][0] == "success" and abs(got[k][1] - float(exact)) <= ex.tolerance(len(c), exact)
    assert got[1][0] == "issue" and got[1][2] == (
        "Histogram assertion 'no value above the top ratio' failed for column 's'. Distribution: %d distinct values, most "
        "common ratio: %.2f%%, null ratio: %.2f%%" % (want[1]["distinct"], top * 100.0, (N_BIG - want[1]["non_null"]) / N_BIG * 100.0))
    # (a table for 10 values has 32 slots: it holds 32 of the column's values and the other rows overflow)
    assert got[4][0] == "issue" and "32 distinct values (max_distinct 10)" in got[4][2] and " 0 overflow rows" not in got[4][2]
    for k, name in ((5, "Float64"), (6, "Date32")):
        assert got[k][0] == "issue" and name in got[k][2] and "not on the GPU path" in got[k][2]
    assert got[7][0] == "skipped" and res.report.metrics.skipped_checks == 1  # "No data to analyze"
    assert got[8][0] == "issue" and "No field named missing" in got[8][2]


def test_entropy_analyzer_on_a_table(big):
    import term_amd.suite as S

    arrs, want = big
    T.init()
    table = pa.table({"n": arrs[0], "s": arrs[1], "d": arrs[2], "f": pa.array(np.arange(N_BIG, dtype=np.float64))})
    runner = S.AnalysisRunner().add(S.EntropyAnalyzer("n")).add(S.EntropyAnalyzer("s")).add(S.EntropyAnalyzer("d"))
    runner.add(S.EntropyAnalyzer("f")).add(S.CompletenessAnalyzer("s"))
    ctx = runner.run(table)
    for col, w in zip("nsd", want):
        rows = ex.buckets(w)
        state = ctx.states["entropy." + col]
        assert state == {"value_counts": {t: c for t, c, _ in rows}, "total_count": w["counted"], "truncated": False}
        m = {k: v["value"] for k, v in ctx.get_metric("entropy." + col)["value"].items()}
        c = list(w["counts"].values())
        for got, exact in ((m["entropy"], ex.exact_entropy(c, 2)), (m["gini_impurity"], ex.exact_gini(c))):
            print("entropy analyzer %s: %r against %s" % (col, got, exact))
            assert abs(got - float(exact)) <= ex.tolerance(len(c), exact)
        assert (m["unique_values"], m["total_count"], m["truncated"]) == (w["distinct"], w["counted"], False)
        assert ("top_values" in m) == (w["distinct"] <= 100)
    assert ctx.get_metric("completeness.s")["value"] == want[1]["non_null"] / N_BIG
    assert [e["analyzer_name"] for e in ctx.errors()] == ["entropy"] and "not on the GPU path" in ctx.errors()[0]["error"]
    small = S.AnalysisRunner().add(S.EntropyAnalyzer("s", 20)).run(table)
    assert "64 distinct values (max_distinct 20)" in small.errors()[0]["error"]  # (64 slots; the other rows overflow)
