"""-m gpu: TGX_CHECK_HISTOGRAM, the two scans behind HistogramAnalyzer (TG/analyzers/advanced/histogram.rs:184-330).
The reference is tests/exact_histogram.py -- plain Python floats, the literal CASE chain and rational sums, neither the
library nor the oracle.  Counts, n, min, max, else_rows and non_finite are compared for equality; the two sums are held
to the worst-case bound of any summation order (exact_histogram.sum_bounds)."""
import json
import math
import os
import threading
from fractions import Fraction

import numpy as np
import pytest

import exact_histogram as eh
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, to_device

pytestmark = pytest.mark.gpu

TYPE_OF = {np.dtype(np.int64): T.INT64, np.dtype(np.float64): T.FLOAT64, np.dtype(np.int32): T.INT32,
           np.dtype(np.float32): T.FLOAT32, np.dtype(np.int8): T.INT8, np.dtype(np.int16): T.INT16,
           np.dtype(np.uint8): T.UINT8, np.dtype(np.uint16): T.UINT16, np.dtype(np.uint32): T.UINT32}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "histogram_vectors.json")) as f:
    GOLDEN = json.load(f)


def column(vals, mask, mem=T.MEM_DEVICE):
    """one whole column in memory space `mem`; `mask`: numpy bools (True = valid) or None"""
    validity = None if mask is None else pad_validity(orc.pack_validity(mask))
    vals = np.ascontiguousarray(vals)
    type_id = TYPE_OF[vals.dtype]
    if mem == T.MEM_DEVICE:
        vals, validity = to_device(vals), to_device(validity)
    return T.Column(type_id, len(vals), values=vals, validity=validity, mem=mem)


def batches_of(cols, n, cuts):
    """`cuts`: None = one batch, an int = batches of that many rows, a list = row boundaries"""
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def python_values(vals, mask):
    out = vals.tolist()
    if mask is not None:
        out = [v if ok else None for v, ok in zip(out, mask.tolist())]
    return out


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def same_range(got, want):
    for k in ("total", "nulls", "non_finite", "n"):
        assert got[k] == want[k], k
    for k in ("min", "max"):
        if want[k] is None:
            assert math.isnan(got[k])
        else:
            assert got[k] == want[k], k
    bound_sum, bound_sq = eh.sum_bounds(want)
    for k, bound in (("sum", bound_sum), ("sum_squared", bound_sq)):
        diff = abs(Fraction(got[k]) - want[k])
        print("%s: got %.17g, |diff| %.3g, bound %.3g" % (k, got[k], float(diff), float(bound)))
        assert diff <= bound, k


def count_plan(edges, extra=()):
    plan = T.Plan([spec(T.HISTOGRAM, 0)] + list(extra))
    plan.set_histogram_edges(0, edges)
    return plan


def counts_under(edges, vals, mask, mem=T.MEM_DEVICE, cuts=None):
    """the count phase alone, under `edges`, against the literal CASE"""
    T.init()
    st = feed(count_plan(edges), batches_of([column(vals, mask, mem)], len(vals), cuts))
    got = st.histogram_counts(0)
    assert got == eh.counts_of(python_values(vals, mask), edges)
    return got


def two_passes(vals, mask, buckets, mem=T.MEM_DEVICE, cuts=None):
    """both phases on the device against exact_histogram; returns (counts, else_rows, non_finite, edges)"""
    T.init()
    n = len(vals)
    xs = python_values(vals, mask)
    bs = batches_of([column(vals, mask, mem)], n, cuts)
    st = feed(T.Plan([spec(T.HISTOGRAM, 0)]), bs)
    got = st.histogram_range(0)
    want = eh.value_range(xs)
    same_range(got, want)
    res = st.finalize()
    assert (res[0].total, res[0].non_null) == (n, want["n"] + want["non_finite"])
    if want["n"] == 0:
        return None
    edges = eh.edges_of(got["min"], got["max"], buckets)  # from the DEVICE's extremes
    st2 = feed(count_plan(edges), bs)
    counts, else_rows, non_finite = st2.histogram_counts(0)
    assert (counts, else_rows, non_finite) == eh.counts_of(xs, edges)
    assert sum(counts) == want["n"] and non_finite == want["non_finite"]
    r2 = st2.histogram_range(0)
    assert (r2["total"], r2["n"], r2["nulls"], r2["non_finite"]) == (n, want["n"], want["nulls"], want["non_finite"])
    return counts, else_rows, non_finite, edges


def mask_of(rng, n, rate):
    return None if rate is None else rng.random(n) >= rate


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("buckets", [1, 2, 5, 999, 1000])
def test_small_row_counts_and_bucket_counts(n, buckets):
    rng = np.random.default_rng(n * 1000 + buckets)
    two_passes(rng.standard_normal(n) * 100.0, mask_of(rng, n, 0.1), buckets)


@pytest.mark.parametrize("buckets", [5, 1000])
@pytest.mark.parametrize("dtype", ["i64", "f64", "i32", "f32", "i8", "i16", "u8", "u16", "u32"])
def test_types_and_many_workgroups(dtype, buckets):
    """about 300 000 rows of the 8-byte types: many workgroups flush into one set of global counters (the narrow types
    differ in the staging only, and take several workgroups)"""
    rng = np.random.default_rng(buckets)
    n = 300_000 + 37 if dtype in ("i64", "f64") else 40_000 + 37
    vals = {"i64": lambda: rng.integers(-10**9, 10**9, n, dtype=np.int64), "f64": lambda: np.exp(rng.standard_normal(n) * 2),
            "i32": lambda: rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32),
            "f32": lambda: rng.standard_normal(n).astype(np.float32), "i8": lambda: rng.integers(-128, 128, n).astype(np.int8),
            "i16": lambda: rng.integers(-2**15, 2**15, n).astype(np.int16), "u8": lambda: rng.integers(0, 256, n).astype(np.uint8),
            "u16": lambda: rng.integers(0, 2**16, n).astype(np.uint16),
            "u32": lambda: rng.integers(0, 2**32, n, dtype=np.int64).astype(np.uint32)}[dtype]()
    two_passes(vals, mask_of(rng, n, 0.05), buckets)


@pytest.mark.parametrize("rate", [None, 0.3, 1.1])
def test_null_rates(rate):
    rng = np.random.default_rng(3)
    n = 20_001
    two_passes(rng.integers(0, 1000, n, dtype=np.int64), mask_of(rng, n, rate), 10)


def test_sliced_column_with_a_bit_offset():
    T.init()
    rng = np.random.default_rng(4)
    n = 10_000
    vals, mask = rng.standard_normal(n), rng.random(n) >= 0.2
    whole = column(vals, mask)
    for lo, length in ((3, 5000), (13, n - 13), (64, 1), (7, 4097)):
        xs = python_values(vals[lo:lo + length], mask[lo:lo + length])
        st = feed(T.Plan([spec(T.HISTOGRAM, 0)]), [[whole.sliced(lo, length)]])
        want = eh.value_range(xs)
        same_range(st.histogram_range(0), want)
        if want["n"]:
            edges = eh.edges_of(want["min"], want["max"], 7)
            st2 = feed(count_plan(edges), [[whole.sliced(lo, length)]])
            assert st2.histogram_counts(0) == eh.counts_of(xs, edges)


@pytest.mark.parametrize("buckets", [2, 5, 999, 1000])
def test_values_on_and_just_below_every_edge(buckets):
    for mn, mx in ((0.0, 1.0), (-3.7, 12.9), (1e-9, 3e-9), (1.7e9, 1.7e9 + 1000.0), (-1e15, 1e15)):
        edges = eh.edges_of(mn, mx, buckets)
        vals = [mn, mx] + edges[:-1] + [math.nextafter(e, -math.inf) for e in edges[1:-1]]
        vals = np.array([v for v in vals if mn <= v <= mx] * 2, np.float64)
        assert two_passes(vals, None, buckets)[3] == edges


def test_constant_column_has_width_one():
    counts, else_rows, _, edges = two_passes(np.full(10_000, 42, np.int64), None, 5)
    assert edges == [42.0, 43.0, 44.0, 45.0, 46.0, 42.0 + 1.0 * 0.001]
    assert counts == [10_000, 0, 0, 0, 0] and else_rows == 0


def test_range_a_few_ulps_wide_reaches_the_last_bucket_through_else():
    g = [d for d in GOLDEN["degenerate"] if d["name"] == "three_ulps_wide"][0]
    lo = g["min"]
    steps = [lo, math.nextafter(lo, 2.0), math.nextafter(math.nextafter(lo, 2.0), 2.0), g["max"]]
    vals = np.array(steps * 500, np.float64)
    counts, else_rows, _, edges = two_passes(vals, None, g["num_buckets"])
    assert edges[-1] == g["max"]  # max + width * 0.001 == max
    assert else_rows > 0 and counts[-1] >= else_rows


def test_int64_beyond_2_53():
    rng = np.random.default_rng(5)
    n = 40_000
    vals = rng.integers(2**62 - 2**12, 2**62 + 2**12, n, dtype=np.int64)  # many integers share one double
    two_passes(vals, None, 10)
    two_passes(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64), None, 1000)


def test_denormal_range():
    rng = np.random.default_rng(6)
    vals = rng.integers(0, 11, 5000).astype(np.float64) * 5e-324
    for buckets in (5, 10, 1000):
        two_passes(vals, None, buckets)


def test_uneven_edges_take_the_fallback_search():
    rng = np.random.default_rng(7)
    n = 100_000
    vals = rng.random(n) * 1000.0
    geometric = [0.0] + [1000.0 * 0.99 ** (999 - i) for i in range(1000)]          # 1000 buckets that crowd towards 0
    steps = sorted(rng.random(499).tolist()) + [999.0, 1000.5]                      # 500 buckets crowded into [0, 1)
    repeated = [0.0] + [250.0] * 400 + [500.0] * 50 + [750.0] * 50 + [1000.0, 1000.0, 2000.0]  # equal interior edges
    for edges in (geometric, [0.0] + steps, repeated):
        counts_under(edges, vals, None)


def test_rows_outside_the_edges_of_another_table():
    """below edges[0] and at or above the last edge: the last bucket, through ELSE"""
    vals = np.array([-5.0, -0.5, 0.0, 0.5, 1.0, 9.99, 10.0, 10.5, 1e300, -1e300] * 7, np.float64)
    edges = eh.edges_of(0.0, 10.0, 4)
    counts, else_rows, _ = counts_under(edges, vals, None)
    assert else_rows == 7 * 5 and counts[-1] >= else_rows
    counts_under(eh.edges_of(0.0, 10.0, 1000), vals, None)
    counts_under([0.0, 1.0], vals, None)


def test_non_finite_rows_are_counted_apart():
    rng = np.random.default_rng(8)
    n = 30_000
    for vals in (rng.standard_normal(n), rng.standard_normal(n).astype(np.float32)):
        vals[rng.integers(0, n, 200)] = np.nan
        vals[rng.integers(0, n, 100)] = np.inf
        vals[rng.integers(0, n, 100)] = -np.inf
        got = two_passes(vals, mask_of(rng, n, 0.1), 10)
        assert got[2] > 250


@pytest.mark.parametrize("order", ["sorted", "reversed", "one_bucket"])
@pytest.mark.parametrize("buckets", [10, 1000])
def test_orders_that_meet_on_one_bucket(order, buckets):
    """every lane of a wave wants the same bucket: the wave-combine path"""
    n = 300_000 + 5
    vals = np.sort(np.random.default_rng(9).standard_normal(n))
    if order == "reversed":
        vals = vals[::-1].copy()
    if order == "one_bucket":
        vals = np.full(n, 0.25)
        vals[0], vals[-1] = 0.0, 1000.0
    two_passes(vals, None, buckets)


def every_field(result):
    """a tgx_result field by field, doubles by bit pattern (NaN included)"""
    return [(name, getattr(result, name).hex() if isinstance(getattr(result, name), float) else getattr(result, name))
            for name, _ in T.Result._fields_]


def test_two_specs_next_to_other_checks():
    """3 and 1000 buckets on two columns in one plan (one launch per phase, grid.y) beside NUMERIC_STATS, COMOMENTS and
    a JOINT_BINS spec.  Every plan is fed the same three batches, and every result -- of the other checks and of each
    histogram spec -- equals, field by field and bit by bit, what the spec gives in a plan without the others"""
    T.init()
    rng = np.random.default_rng(10)
    n = 300_000
    a, b = rng.integers(0, 10**6, n, dtype=np.int64), rng.standard_normal(n)
    am, bm = mask_of(rng, n, 0.05), mask_of(rng, n, 0.1)
    cols = [column(a, am), column(b, bm)]
    batches = batches_of(cols, n, [100_000, 100_064])
    pa, pb = python_values(a, am), python_values(b, bm)
    others = [spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE), spec(T.NUMERIC_STATS, 1), spec(T.COMOMENTS, 0, column2=1),
              spec(T.JOINT_BINS, 0, column2=1)]
    alone_state = feed(T.Plan(others), batches)
    alone, alone_joint = alone_state.finalize(), alone_state.joint_range(3)
    ra, rb = eh.value_range(pa), eh.value_range(pb)
    ea, eb = eh.edges_of(ra["min"], ra["max"], 3), eh.edges_of(rb["min"], rb["max"], 1000)
    plan = T.Plan([spec(T.HISTOGRAM, 0), spec(T.HISTOGRAM, 1), spec(T.HISTOGRAM, 1), spec(T.HISTOGRAM, 0)] + others)
    plan.set_histogram_edges(0, ea)
    plan.set_histogram_edges(1, eb)  # (specs 2 and 3 stay in their range phase)
    st = feed(plan, batches)
    res = st.finalize()
    assert st.histogram_counts(0) == eh.counts_of(pa, ea)
    assert st.histogram_counts(1) == eh.counts_of(pb, eb)
    same_range(st.histogram_range(2), rb)
    same_range(st.histogram_range(3), ra)
    # the other checks: what they are without the histogram specs
    for k in range(4):
        assert every_field(res[4 + k]) == every_field(alone[k]), k
    assert st.joint_range(7) == alone_joint
    # each histogram spec: what it is in a plan of its own, fed the same batches
    for k, (col, edges) in enumerate(((0, ea), (1, eb), (1, None), (0, None))):
        single = T.Plan([spec(T.HISTOGRAM, col)])
        if edges is not None:
            single.set_histogram_edges(0, edges)
        one = feed(single, [[bt[col]] if col == 0 else [bt[0], bt[1]] for bt in batches])
        assert every_field(one.finalize()[0]) == every_field(res[k]), k
        if edges is not None:
            assert one.histogram_counts(0) == st.histogram_counts(k)
        got, want = one.histogram_range(0), st.histogram_range(k)
        assert {x: (v.hex() if isinstance(v, float) else v) for x, v in got.items()} == \
               {x: (v.hex() if isinstance(v, float) else v) for x, v in want.items()}, k


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST, T.MEM_HOST_RETAINED])
@pytest.mark.parametrize("cuts", [None, [1, 64, 65, 4097, 70_001, 150_000], 8192])
def test_batching_and_memory_space(mem, cuts):
    rng = np.random.default_rng(11)
    n = 200_000 + 11
    two_passes(rng.random(n) * 100, mask_of(rng, n, 0.05), 1000, mem=mem, cuts=cuts)


def test_narrow_columns_in_small_host_batches():
    rng = np.random.default_rng(12)
    n = 100_000
    two_passes(rng.integers(-2**31, 2**31, n).astype(np.int32), mask_of(rng, n, 0.05), 10, mem=T.MEM_HOST, cuts=8192)
    two_passes(rng.standard_normal(n).astype(np.float32), None, 1000, mem=T.MEM_HOST, cuts=8192)


def test_reset_merge_serialize():
    T.init()
    rng = np.random.default_rng(13)
    n = 90_000
    vals, mask = rng.standard_normal(n) * 50, rng.random(n) >= 0.1
    xs = python_values(vals, mask)
    parts = batches_of([column(vals, mask)], n, [30_000, 60_000])
    want_range = eh.value_range(xs)
    edges = eh.edges_of(want_range["min"], want_range["max"], 100)
    want = eh.counts_of(xs, edges)
    # range phase: three states merged, then through a blob
    rplan = T.Plan([spec(T.HISTOGRAM, 0)])
    states = [feed(rplan, [p]) for p in parts]
    states[0].merge(states[1:])
    same_range(states[0].histogram_range(0), want_range)
    blob = states[0].serialize()
    back = T.State.deserialize(rplan, blob)
    same_range(back.histogram_range(0), want_range)
    assert back.serialize() == blob
    # count phase: the same
    plan = count_plan(edges)
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    assert states[0].histogram_counts(0) == want
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    assert back.histogram_counts(0) == want and back.serialize() == blob
    # a blob counted under other edges, or in the other phase, is refused
    for other in (count_plan(edges[:-1] + [edges[-1] + 1.0]), count_plan(edges[1:]), rplan):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(other, blob)
    # reset and reuse: the first part alone, after the whole table
    st = states[0]
    st.reset()
    assert st.histogram_counts(0) == ([0] * 100, 0, 0)
    st.update(parts[0])
    assert st.histogram_counts(0) == eh.counts_of(xs[:30_000], edges)
    assert st.finalize()[0].total == 30_000
    rst = feed(rplan, parts)
    rst.reset()
    assert rst.histogram_range(0)["n"] == 0 and math.isnan(rst.histogram_range(0)["min"])
    rst.update(parts[1])
    same_range(rst.histogram_range(0), eh.value_range(xs[30_000:60_000]))


def test_unsupported_columns_and_phase_misuse():
    T.init()
    n = 1000
    f = column(np.arange(n, dtype=np.float64), None, T.MEM_HOST)
    u64 = T.Column.narrow(T.UINT64, np.arange(n, dtype=np.uint64))
    boolean = T.Column.boolean(np.zeros(n // 8 + 8, np.uint8), n)
    offs, data, sval = orc.utf8_from_list(["a%d" % i for i in range(n)])
    text = T.Column.utf8(offs, np.concatenate([data, np.zeros(64, np.uint8)]))
    plan = T.Plan([spec(T.HISTOGRAM, 0)])
    for bad in (u64, boolean, text):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED"):
            T.State(plan).update([bad])
    st = feed(plan, [[f]])
    with pytest.raises(T.TgxError, match="range phase"):
        st.histogram_counts(0)
    with pytest.raises(T.TgxError, match="once a state"):
        plan.set_histogram_edges(0, [0.0, 1.0])
    r = feed(count_plan([0.0, 500.0, 1000.0]), [[f]]).histogram_range(0)
    assert (r["n"], r["total"]) == (n, n) and math.isnan(r["min"]) and math.isnan(r["sum"])


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(world, device_buffers):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's range and counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    T.init()
    rng = np.random.default_rng(14 + world)
    n = 250_000 + 3
    vals, mask = rng.standard_normal(n) * 10, rng.random(n) >= 0.05
    xs = python_values(vals, mask)
    whole = [column(vals, mask)]
    want_range = eh.value_range(xs)
    edges = eh.edges_of(want_range["min"], want_range["max"], 1000)
    want = eh.counts_of(xs, edges)
    plan = T.Plan([spec(T.HISTOGRAM, 0), spec(T.HISTOGRAM, 0), spec(T.COUNT, 0)])
    plan.set_histogram_edges(1, edges)
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(n, world, rank)
            shard = [c.sliced(lo, hi - lo) for c in whole]
            st = T.State(plan)
            comm = thread_comm(group, rank, device_buffers=device_buffers)
            for _ in range(2):
                res = sharded_suite_step(plan, st, shard, comm)
            results[rank] = (res, st.histogram_range(0), st.histogram_counts(1))
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
    for res, got_range, counts in results:
        assert (res[0].total, res[1].total, res[2].non_null) == (n, n, want_range["n"])
        same_range(got_range, want_range)
        assert counts == want


# ---- HistogramAnalyzer through AnalysisRunner.run ----------------------------------------------------------------
def check_analyzer(ctx, xs, buckets):
    want = eh.histogram_state(xs, buckets)
    state = ctx.states["histogram"]
    r = eh.value_range(xs)
    bound_sum, bound_sq = eh.sum_bounds(r)
    assert state["buckets"] == want["buckets"]
    assert (state["min_value"], state["max_value"], state["total_count"]) == (want["min_value"], want["max_value"], want["total_count"])
    assert abs(Fraction(state["sum"]) - r["sum"]) <= bound_sum and abs(Fraction(state["sum_squared"]) - r["sum_squared"]) <= bound_sq
    m = ctx.get_metric("histogram")
    assert m["type"] == "Histogram"
    v = m["value"]
    assert v["buckets"] == want["buckets"] and v["total_count"] == sum(b["count"] for b in want["buckets"])
    assert (v["min"], v["max"]) == (want["min_value"], want["max_value"])
    if r["n"]:
        # exactly what the reference's expressions give on the state's own doubles
        mean = state["sum"] / float(r["n"])
        assert v["mean"] == mean
        if r["n"] > 1:
            variance = state["sum_squared"] / float(r["n"]) - mean * mean
            assert v["std_dev"] == math.sqrt(variance) if variance >= 0 else v["std_dev"] is None
    return v


def test_analyzer_on_the_reference_table():
    pa = pytest.importorskip("pyarrow")
    import term_amd.suite as S

    g = GOLDEN["reference_table"]
    tbl = pa.table({"x": pa.array(g["values"], pa.float64())})
    ctx = S.AnalysisRunner().add(S.HistogramAnalyzer("x", g["num_buckets"])).run(tbl)
    assert not ctx.has_errors(), ctx.errors()
    v = check_analyzer(ctx, g["values"], g["num_buckets"])
    assert len(v["buckets"]) == g["buckets"] and v["total_count"] == g["total_count"]
    assert (v["min"], v["max"]) == (g["min"], g["max"])
    assert abs(v["mean"] - g["mean_numerator"] / g["mean_denominator"]) < 0.01  # the reference's own assertion
    assert v["mean"] == 33.0 / 9.0
    assert [b["count"] for b in v["buckets"]] == g["counts"]
    assert '"count": 3' in ctx.text and '"total_count": 9' in ctx.text


def test_analyzer_on_a_300_000_row_table_next_to_others():
    pa = pytest.importorskip("pyarrow")
    import term_amd.suite as S

    rng = np.random.default_rng(21)
    n = 300_000
    a = rng.integers(0, 5000, n, dtype=np.int64)
    b = a * 0.25 + rng.standard_normal(n) * 300.0
    am, bm = rng.random(n) >= 0.03, rng.random(n) >= 0.05
    tbl = pa.table({"a": pa.array(a, pa.int64(), mask=~am), "b": pa.array(b, pa.float64(), mask=~bm)})
    tbl = pa.Table.from_batches(tbl.to_batches(max_chunksize=50_000))
    others = [S.SizeAnalyzer(), S.MeanAnalyzer("b"), S.MutualInformationAnalyzer("a", "b"), S.CorrelationAnalyzer("a", "b")]
    runner = S.AnalysisRunner().add(S.HistogramAnalyzer("b", 1000))
    alone = S.AnalysisRunner()
    for an in others:
        runner.add(an)
        alone.add(an)
    ctx, ctx_alone = runner.run(tbl), alone.run(tbl)
    assert not ctx.has_errors(), ctx.errors()
    check_analyzer(ctx, python_values(b, bm), 1000)
    for key in ("size", "mean.b", "mutual_information_a_b", "correlation_pearson_a_b"):
        assert ctx.get_metric(key) == ctx_alone.get_metric(key) and ctx.get_metric(key) is not None, key
    assert ctx.states["mutual_information_a_b"] == ctx_alone.states["mutual_information_a_b"]
    # an Int64 column by cast, when the reference's downcast is not asked for
    ctx = S.AnalysisRunner().add(S.HistogramAnalyzer("a", 7, strict_reference_types=False)).run(tbl)
    assert not ctx.has_errors(), ctx.errors()
    check_analyzer(ctx, python_values(a, am), 7)


def test_analyzer_without_rows():
    pa = pytest.importorskip("pyarrow")
    import term_amd.suite as S

    empty = {"buckets": [], "min_value": 0.0, "max_value": 0.0, "total_count": 0, "sum": 0.0, "sum_squared": 0.0}
    for tbl in (pa.table({"x": pa.array([None, None, None], pa.float64())}), pa.table({"x": pa.array([], pa.float64())})):
        ctx = S.AnalysisRunner().add(S.HistogramAnalyzer("x", 5)).run(tbl)
        assert not ctx.has_errors(), ctx.errors()
        assert ctx.states["histogram"] == empty
        assert ctx.get_metric("histogram") == {"type": "Histogram", "value": {
            "buckets": [], "total_count": 0, "min": 0.0, "max": 0.0, "mean": 0.0, "std_dev": 0.0}}
    big = pa.table({"x": pa.array([-1.7e308, 1.7e308], pa.float64())})
    ctx = S.AnalysisRunner().add(S.HistogramAnalyzer("x", 5)).run(big)
    assert "overflows" in ctx.errors()[0]["error"]


def test_analyzer_on_an_int32_column_under_strict_types():
    pa = pytest.importorskip("pyarrow")
    import term_amd.suite as S

    tbl = pa.table({"i": pa.array([1, 2, 3, 4, None], pa.int32()), "x": pa.array([1.0, 2.0, 3.0, 4.0, 5.0], pa.float64())})
    ctx = (S.AnalysisRunner().add(S.HistogramAnalyzer("i", 2)).add(S.SizeAnalyzer()).add(S.MeanAnalyzer("x"))
           .add(S.MutualInformationAnalyzer("x", "x", 2)).run(tbl))
    assert ctx.errors() == [{"analyzer_name": "histogram", "error": "Invalid data: Expected Float64 for min"}]
    assert ctx.get_metric("histogram") is None
    assert ctx.get_metric("size")["value"] == 5 and ctx.get_metric("mean.x")["value"] == 3.0
    assert ctx.get_metric("mutual_information_x_x") is not None
