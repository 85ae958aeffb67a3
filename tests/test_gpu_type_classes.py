"""TGX_CHECK_TYPE_CLASSES and DataTypeAnalyzer on the device: all nine counters are compared for equality with the exact
reference (tests/exact_type_classes.py) -- undecided_rows among them -- over every string layout, slices, row counts,
NULL shares, the edge table cycled through every lane position, long DOUBLE values at odd byte offsets, batching from
DEVICE and HOST buffers, the ways a state travels, its neighbours in a plan, refused column types, and the analyzer end
to end.  Columns are built from raw buffers: the edge table holds bytes that are no UTF-8."""
import ctypes
import json
import os
import struct
import threading

import numpy as np
import pytest

import exact_type_classes as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from gpu_util import to_device

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_type_vectors.json")
with open(GOLDEN) as _f:
    G = json.load(_f)

GRID_PASS = 2048 * 256  # rows one full grid of the string kernel takes (grid_for)
EDGE_VALUES = [v for v, _ in ex.EDGES]
if len(EDGE_VALUES) % 2 == 0:  # an odd cycle: every value meets every lane of a wave
    EDGE_VALUES = EDGE_VALUES + [b"x"]
_CLASS = {}


def want(values):
    """ex.counts, with the class of a value looked up once"""
    out = dict.fromkeys(ex.COUNTERS, 0)
    for v in values:
        out["seen"] += 1
        if v is None:
            continue
        if v not in _CLASS:
            _CLASS[v] = ex.NAMES[ex.classify(v)] + "_rows"
        out["non_null"] += 1
        out[_CLASS[v]] += 1
    assert out["non_null"] == sum(out[n + "_rows"] for n in ex.NAMES) and out["seen"] >= out["non_null"]
    return out


def cycled(n, null_share=0.0, seed=1):
    """the edge table cycled over n rows; a NULL share of 0, about one half or all"""
    rng = np.random.default_rng(seed)
    nulls = rng.random(n) < null_share if 0.0 < null_share < 1.0 else np.full(n, null_share >= 1.0)
    return [None if nulls[i] else EDGE_VALUES[i % len(EDGE_VALUES)] for i in range(n)]


# ---- columns from raw buffers ---------------------------------------------------------------------------------------------
def bits(values):
    if all(v is not None for v in values):
        return None
    return np.packbits(np.array([v is not None for v in values], dtype=np.uint8), bitorder="little")


def padded(buf):
    """a device copy with 64 spare bytes behind it"""
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


def offsets_column(values, large=False, lead=0):
    """Utf8 / LargeUtf8; `lead`: bytes in front of the first value (moves every value's address)"""
    lens = np.array([0 if v is None else len(v) for v in values], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)]) + lead
    data = np.frombuffer(b"#" * lead + b"".join(v for v in values if v is not None) + b"\0" * 8, np.uint8)
    offs = offs.astype(np.int64 if large else np.int32)
    make = T.Column.large_utf8 if large else T.Column.utf8
    return make(offs, data, bits(values))


def view_column(values):
    """Utf8View: values of up to 12 bytes inline, longer ones spread over two data buffers"""
    bufs, views = [bytearray(), bytearray()], bytearray()
    for k, v in enumerate(values):
        b = v or b""
        if len(b) <= 12:
            views += struct.pack("<i12s", len(b), b)
        else:
            which = k % 2
            views += struct.pack("<i4sii", len(b), b[:4], which, len(bufs[which]))
            bufs[which] += b
    return T.Column.utf8_view(np.frombuffer(bytes(views) + b"\0" * 16, np.uint8)[:len(values) * 16 + 16],
                              [np.frombuffer(bytes(b) + b"\0" * 8, np.uint8) for b in bufs], bits(values), length=len(values))


def dict_column(indices, entries, row_valid=None):
    idx = np.asarray(indices, dtype=np.int32)
    validity = None if row_valid is None else np.packbits(np.asarray(row_valid, dtype=np.uint8), bitorder="little")
    return T.Column.dict32_utf8(idx, offsets_column(entries), validity)


def dict_rows(indices, entries, row_valid=None):
    """the rows a dictionary column stands for: a NULL row, a NULL entry and an index outside the dictionary are NULL"""
    return [None if (row_valid is not None and not row_valid[i]) or not 0 <= k < len(entries) else entries[k]
            for i, k in enumerate(indices)]


def place(col, mem):
    if mem == T.MEM_DEVICE:
        return on_device(col)
    col.c.mem = mem
    if col._keep[4] is not None:
        col._keep[4].c.mem = mem
    return col


LAYOUTS = {"utf8": offsets_column, "large_utf8": lambda v: offsets_column(v, large=True), "utf8_view": view_column}


def cut(col, n, cuts):
    if cuts is None:
        return [col]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [col.sliced(lo, hi - lo) for lo, hi in zip(bounds[:-1], bounds[1:])]


def run(col, parts=None, plan=None):
    T.init()
    plan = plan or T.Plan([spec(T.TYPE_CLASSES, 0)])
    st = T.State(plan)
    for p in parts or [col]:
        st.update([p])
    return st


def check(values, layout="utf8", mem=T.MEM_DEVICE, cuts=None):
    col = place(LAYOUTS[layout](values), mem)
    st = run(col, cut(col, len(values), cuts))
    w = want(values)
    assert st.type_classes(0) == w
    r = st.finalize()[0]
    assert (r.total, r.non_null) == (w["seen"], w["non_null"])
    return w


# ---- layouts, slices, row counts, NULL shares ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_string_layouts(layout, mem):
    w = check(cycled(2000, 0.1), layout, mem)
    assert all(w[n + "_rows"] > 0 for n in ex.NAMES)  # every class is met, undecided included


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
def test_a_dictionary_with_null_unused_and_out_of_range_entries(mem):
    rng = np.random.default_rng(3)
    entries = list(EDGE_VALUES[:60]) + [None, b"unused", None, b"2023-1-5x"]
    used = [k for k in range(len(entries)) if entries[k] != b"unused"]
    idx = rng.choice(used, 5000)
    idx[7], idx[8] = -1, len(entries)  # outside the dictionary: NULL rows
    valid = rng.random(5000) >= 0.1
    valid[:7] = True
    valid[9] = False  # a NULL-index row
    col = place(dict_column(idx, entries, valid), mem)
    st = run(col)
    w = want(dict_rows(idx, entries, valid))
    assert st.type_classes(0) == w and w["undecided_rows"] > 0
    st2 = run(col, [col.sliced(0, 2500), col.sliced(2500, 2500)])  # the dictionary again in a second batch
    assert st2.type_classes(0) == w


def test_a_dictionary_without_entries_is_all_null():
    col = place(dict_column([0, 1, 2], []), T.MEM_DEVICE)
    assert run(col).type_classes(0) == want([None] * 3)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("offset", [3, 9])
def test_a_slice_whose_validity_bit_offset_is_no_multiple_of_8(layout, offset):
    values = cycled(1000, 0.5, seed=4)
    col = on_device(LAYOUTS[layout](values))
    st = run(col.sliced(offset, 700))
    assert st.type_classes(0) == want(values[offset:offset + 700])


@pytest.fixture(scope="module")
def grid_rows():
    """one full grid pass plus a ragged tail, the edge table cycled, about one row in sixteen NULL"""
    n = GRID_PASS + 257
    values = cycled(n, 1 / 16, seed=5)
    return values, want(values)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_row_counts(n):
    check(cycled(n))


def test_a_full_grid_pass_and_a_ragged_tail(grid_rows):
    values, w = grid_rows
    col = on_device(offsets_column(values))
    assert run(col).type_classes(0) == w


@pytest.mark.parametrize("share", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("layout", ["utf8", "utf8_view"])
def test_null_shares(layout, share):
    w = check(cycled(3000, share, seed=6), layout)
    assert (w["non_null"] == 0) == (share == 1.0)


@pytest.mark.parametrize("lead", [0, 1, 2, 3, 5, 7])
def test_long_doubles_at_odd_byte_offsets(lead):
    """DOUBLE values of 1, 7, 8, 9, 16, 17 and 4096 digits (and the same with a byte that ends the grammar) wherever the
    value starts within its 4-byte word"""
    values = []
    for digits in (1, 7, 8, 9, 16, 17, 4096):
        body = b"7" * digits
        values += [body + b".", b"." + body, body + b"e1", body + b"x", b"-" + body + b".5", body]
    values = values * 3
    col = on_device(offsets_column(values, lead=lead))
    w = want(values)
    assert run(col).type_classes(0) == w and w["double_rows"] > 0 and w["string_rows"] > 0 and w["integer_rows"] > 0


# ---- batching -----------------------------------------------------------------------------------------------------------------
N_STREAM = 70_000


@pytest.fixture(scope="module")
def stream_rows():
    values = cycled(N_STREAM, 0.05, seed=7)
    return values, want(values)


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 30_001]), (T.MEM_DEVICE, 8192),
                                      (T.MEM_HOST, None), (T.MEM_HOST, 8192), (T.MEM_HOST, [3, 8195, 8196, 50_001])])
@pytest.mark.parametrize("layout", ["utf8", "utf8_view"])
def test_batching_independence(stream_rows, layout, mem, cuts):
    values, w = stream_rows
    col = place(LAYOUTS[layout](values), mem)
    assert run(col, cut(col, N_STREAM, cuts)).type_classes(0) == w


# ---- the ways a state travels -------------------------------------------------------------------------------------------------
def test_state_algebra(stream_rows):
    values, w = stream_rows
    T.init()
    col = on_device(offsets_column(values))
    parts = cut(col, N_STREAM, [20_000, 45_001])
    plan = T.Plan([spec(T.TYPE_CLASSES, 0), spec(T.COUNT, 0)])
    st = run(col, parts[:1], plan)  # read half-way
    assert st.type_classes(0) == want(values[:20_000])
    st.reset()
    assert st.type_classes(0) == dict.fromkeys(ex.COUNTERS, 0)
    for p in parts:  # ... after the reset the whole table
        st.update([p])
    assert st.type_classes(0) == w
    # a blob round trip mid-table, then the rest
    mid = run(col, parts[:2], plan)
    back = T.State.deserialize(plan, mid.serialize())
    assert back.type_classes(0) == want(values[:45_001])
    back.update([parts[2]])
    assert back.type_classes(0) == w and back.serialize() == st.serialize()
    # merge of two states
    a, b = run(col, parts[:1], plan), run(col, parts[1:], plan)
    a.merge([b])
    assert a.type_classes(0) == w
    a.merge([st])
    assert a.type_classes(0) == ex.add(w, w)


def test_allreduce_over_two_threaded_ranks(stream_rows):
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    values, w = stream_rows
    T.init()
    whole = on_device(offsets_column(values))
    plan = T.Plan([spec(T.TYPE_CLASSES, 0), spec(T.COUNT, 0)])
    world = 2
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(N_STREAM, world, rank)
            st = T.State(plan)
            comm = thread_comm(group, rank, device_buffers=True)
            res = sharded_suite_step(plan, st, [whole.sliced(lo, hi - lo)], comm)
            results[rank] = (res, st.type_classes(0))
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
        assert got == w and (res[0].total, res[0].non_null, res[1].total) == (w["seen"], w["non_null"], N_STREAM)


# ---- neighbours, two specs, unsupported types -----------------------------------------------------------------------------------
def test_the_kind_leaves_its_neighbours_unchanged(stream_rows):
    values, w = stream_rows
    T.init()
    col = on_device(offsets_column(values))
    others = [spec(T.LENGTH, 0, length_min=1, length_max=10), spec(T.REGEX_MATCH, 0, pattern=r"^\d+$"),
              spec(T.VALUE_COUNTS, 0), spec(T.COUNT, 0)]

    def with_bounds(specs, at):
        plan = T.Plan(specs)
        plan.set_value_counts(at, 10000, 256)
        return plan

    alone_st = run(col, plan=with_bounds(others, 2))
    alone, alone_counts = alone_st.finalize(), alone_st.value_counts(2)
    st = run(col, plan=with_bounds([spec(T.TYPE_CLASSES, 0)] + others + [spec(T.TYPE_CLASSES, 0)], 3))
    res = st.finalize()
    assert st.type_classes(0) == st.type_classes(5) == w  # two specs of the column: one task
    assert st.value_counts(3) == alone_counts
    for got, ref in zip(res[1:5], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))
    st.profile_enable(True)
    st.update([col])
    st.finalize()
    assert st.profile_get("type_classes")["launches"] == 1


def test_two_columns_are_two_tasks_of_one_launch(stream_rows):
    values, w = stream_rows
    T.init()
    other = cycled(N_STREAM, 0.5, seed=8)
    cols = [on_device(offsets_column(values)), on_device(view_column(other))]
    st = T.State(T.Plan([spec(T.TYPE_CLASSES, 0), spec(T.TYPE_CLASSES, 1)]))
    st.update(cols)
    assert st.type_classes(0) == w and st.type_classes(1) == want(other)


def test_numeric_columns_are_unsupported_and_the_state_stays_usable():
    import pyarrow as pa

    T.init()
    n = 1000
    st = T.State(T.Plan([spec(T.TYPE_CLASSES, 0)]))
    for arr in (pa.array(np.arange(n, dtype=np.int64)), pa.array(np.arange(n, dtype=np.float64)),
                pa.array(np.arange(n, dtype=np.int32)), pa.array(np.arange(n, dtype=np.uint64)), pa.array(np.arange(n) % 2 == 0)):
        col = T.Column.from_arrow(arr)
        for mem in (T.MEM_HOST, T.MEM_DEVICE):
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*TYPE_CLASSES takes"):
                st.update([place(col, mem)])
    assert st.type_classes(0) == dict.fromkeys(ex.COUNTERS, 0)
    values = cycled(500)
    st.update([on_device(offsets_column(values))])
    assert st.type_classes(0) == want(values)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_the_analysis_runner_in_the_reference_integration_shape():
    import pyarrow as pa

    T.init()
    g = G["mixed_type"]
    n = len(g["values"])
    ints = [0, 1, 1, 7, -5, 2**31 - 1, 2**31, None, -2**31, -2**31 - 1]
    table = pa.table({"mixed_type": pa.array(g["values"], pa.string()), "i32": pa.array([0, 1, 5, None, -3, 1, 0, 9, 2, 1], pa.int32()),
                      "i64": pa.array(ints, pa.int64()), "f": pa.array([1.0, 2.5, None] + [float(k) for k in range(7)], pa.float64()),
                      "dates": pa.array(["2023-01-01", "2023-1-5x", "x"] + ["7"] * 7, pa.string()),
                      "ts": pa.array([1] * n, pa.timestamp("ns")), "u64": pa.array([1] * n, pa.uint64())})
    runner = S.AnalysisRunner().add(S.SizeAnalyzer()).add(S.CompletenessAnalyzer("f")).add(S.MeanAnalyzer("f"))
    runner.add(S.HistogramAnalyzer("f", 4)).add(S.DataTypeAnalyzer("mixed_type")).add(S.DataTypeAnalyzer("i32"))
    runner.add(S.DataTypeAnalyzer("i64")).add(S.DataTypeAnalyzer("f")).add(S.DataTypeAnalyzer("dates"))
    runner.add(S.DataTypeAnalyzer("ts")).add(S.DataTypeAnalyzer("u64"))
    ctx = runner.run(table)
    # the golden column: the contract's answer, and what the reference's own test asserts of it
    assert ctx.states["data_type.mixed_type"] == g["contract"]
    metric = ctx.get_metric("data_type.mixed_type")
    assert metric == {"type": "Map", "value": {k: {"type": "Long", "value": c} for k, c in g["contract"]["type_counts"].items()}}
    assert set(g["reference_asserts"]["keys_present"]) <= set(metric["value"])
    assert '"data_type.mixed_type": {"type_counts": {"boolean": 3, "integer": 2, "double": 2, "date": 1, "string": 2}, ' \
           '"total_count": 10}' in ctx.text
    # an Int32, an Int64 and a Float64 column
    assert ctx.states["data_type.i32"] == {"type_counts": {"boolean": 5, "integer": 4}, "total_count": 9}
    assert ctx.states["data_type.i64"] == {"type_counts": {"boolean": 3, "integer": 4, "double": 2}, "total_count": 9}
    assert ctx.states["data_type.f"] == {"type_counts": {"double": 9}, "total_count": 9}
    # the rest of the run answers
    assert ctx.get_metric("size") == {"type": "Long", "value": n}
    assert ctx.get_metric("completeness.f")["value"] == 0.9 and ctx.get_metric("mean.f")["value"] == 24.5 / 9
    assert ctx.get_metric("histogram")["type"] == "Histogram"
    errors = {e["error"] for e in ctx.errors()}
    assert [e["analyzer_name"] for e in ctx.errors()] == ["data_type"] * 3
    assert any("column 'dates' is not on the GPU path: 1 values look like dates in a form this path does not decide" in e
               for e in errors)
    assert any("column 'ts' (Timestamp(Nanosecond, None)) is not on the GPU path" in e for e in errors)
    assert any("column 'u64' (UInt64) is not on the GPU path" in e for e in errors)
    assert "data_type.dates" not in ctx.states


def test_the_counters_through_python_give_the_analyzers_state():
    T.init()
    g = G["mixed_type"]
    values = [v.encode() for v in g["values"]]
    st = run(on_device(offsets_column(values)))
    a = S.DataTypeAnalyzer("mixed_type")
    state = json.loads(a.state_text_from_type_classes(st.type_classes(0)))
    assert state == g["contract"] and S.data_type_dominant_type(state) == ("boolean", 0.3)
    assert a.compute_metric_from_state(state)["value"]["date"] == {"type": "Long", "value": 1}
