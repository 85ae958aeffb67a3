"""-m gpu: TGX_CHECK_TEMPORAL, the row predicates behind TemporalOrderingConstraint's three pure-scan modes
(TG/constraints/temporal_ordering.rs:346-453).  The reference is tests/exact_temporal.py -- Python integers, neither the
library nor the oracle -- and EVERY count (seen, considered, violations) is compared for equality; there are no
tolerances."""
import itertools
import threading

import numpy as np
import pytest

import exact_temporal as et
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, to_device

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = et.I64_MIN, et.I64_MAX
DAY_S = 86400


def column(vals, mask, mem=T.MEM_DEVICE, offset=0):
    """an Int64 column whose Arrow offset is `offset`: `offset` rows of other data (and set validity bits) lead the
    buffers, the view starts behind them"""
    vals = np.concatenate([np.full(offset, 0x5A5A5A5A5A5A5A5A, np.int64), np.ascontiguousarray(vals, np.int64)])
    validity = None
    if mask is not None:
        validity = pad_validity(orc.pack_validity(np.concatenate([np.ones(offset, bool), mask])))
    if mem == T.MEM_DEVICE:
        vals, validity = to_device(vals), to_device(validity)
    return T.Column(T.INT64, len(vals), values=vals, validity=validity, mem=mem).sliced(offset, len(vals) - offset)


def batches_of(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def set_params(plan, index, mode, params):
    plan.set_temporal(index, mode, flags=params.get("flags", 0), delta=params.get("delta", 0),
                      ticks_per_second=params.get("ticks_per_second", 0), tod_lo=params.get("tod_lo", 0),
                      tod_hi=params.get("tod_hi", 0), lo=params.get("lo", I64_MIN), hi=params.get("hi", I64_MAX))


def plan_of(tasks, extra=()):
    """tasks: [(mode, params)]; ORDER reads columns (0, 1), the other modes column 0"""
    specs = [spec(T.TEMPORAL, 0, column2=1 if mode == et.ORDER else -1) for mode, _ in tasks]
    plan = T.Plan(specs + list(extra))
    for i, (mode, params) in enumerate(tasks):
        set_params(plan, i, mode, params)
    return plan


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def lists(a, am, b, bm):
    return a.tolist(), b.tolist(), None if am is None else am.tolist(), None if bm is None else bm.tolist()


def want_of(tasks, a, am, b, bm):
    pa, pb, ma, mb = lists(a, am, b, bm)
    return [et.counts(mode, params, pa, pb if mode == et.ORDER else None, ma, mb if mode == et.ORDER else None)
            for mode, params in tasks]


def check(tasks, a, am, b, bm, offsets=(0, 0), mem=T.MEM_DEVICE, cuts=None):
    T.init()
    cols = [column(a, am, mem, offsets[0]), column(b, bm, mem, offsets[1])]
    plan = plan_of(tasks)
    st = feed(plan, batches_of(cols, len(a), cuts))
    got = [st.temporal_counts(i) for i in range(len(tasks))]
    want = want_of(tasks, a, am, b, bm)
    assert got == want
    for r, (seen, considered, violations) in zip(st.finalize(), want):
        assert (r.total, r.non_null, r.matches) == (seen, considered, considered - violations)
    return st, plan, want


# 09:00 .. 17:00 in seconds; the other units scale it
def tod_params(unit, flags=0, lo=9 * 3600, hi=17 * 3600):
    tps = et.TICKS[unit]
    return {"ticks_per_second": tps, "tod_lo": lo * tps, "tod_hi": hi * tps, "flags": flags}


def three_modes(flags=0):
    return [(et.ORDER, {"delta": 0, "flags": flags & et.KEEP_NULLS}), (et.TIME_OF_DAY, tod_params("ms", flags)),
            (et.RANGE, {"lo": -10**12, "hi": 10**12, "flags": flags & et.KEEP_NULLS})]


def table(rng, n, null_a=0.1, null_b=0.07):
    """millisecond instants over +-60 years around the epoch; `b` mostly a little after `a`"""
    a = rng.integers(-60 * 365 * DAY_S * 1000, 60 * 365 * DAY_S * 1000, n, dtype=np.int64)
    b = a + rng.integers(-3000, 30000, n, dtype=np.int64)
    am = None if null_a is None else rng.random(n) >= null_a
    bm = None if null_b is None else rng.random(n) >= null_b
    return a, am, b, bm


@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    a, am, b, bm = table(rng, n)
    for flags in (0, et.KEEP_NULLS):
        check(three_modes(flags), a, am, b, bm)


def test_more_than_one_sweep_of_the_launch():
    """Two tasks in the plan: each gets max(32, 4 * CUs / 2) = 512 workgroups of 512 lanes on the 256-CU part, and a lane
    takes 4 row PAIRS per sweep on the 16-byte path: one sweep is 4 * 512 * 512 * 2 = 2 097 152 rows.  2 097 152 + 5 rows
    start a second sweep there (and a fifth one on the one-row-per-load path, which the odd offset takes)."""
    n = 4 * 512 * 512 * 2 + 5
    rng = np.random.default_rng(1)
    a, am, b, bm = table(rng, n, 0.5, None)
    tasks = [(et.ORDER, {"delta": 1}), (et.RANGE, {"lo": 0})]
    T.init()
    want = want_of(tasks, a, am, b, bm)
    for offsets in ((0, 0), (1, 0)):
        cols = [column(a, am, T.MEM_DEVICE, offsets[0]), column(b, bm, T.MEM_DEVICE, offsets[1])]
        st = feed(plan_of(tasks), [cols])
        assert [st.temporal_counts(i) for i in range(2)] == want


@pytest.mark.parametrize("off_a,off_b", list(itertools.product([0, 1, 7, 8, 9], repeat=2)))
def test_arrow_offsets(off_a, off_b):
    rng = np.random.default_rng(100 + 10 * off_a + off_b)
    n = 8192 + 77
    a, am, b, bm = table(rng, n)
    check(three_modes(), a, am, b, bm, offsets=(off_a, off_b))


@pytest.mark.parametrize("nulls", ["none", "a", "b", "all_a", "all_both", "none_present"])
def test_validity_absent_present_all_null(nulls):
    rng = np.random.default_rng(5)
    n = 20_001
    fa, fb = {"none": (None, None), "a": (0.3, None), "b": (None, 0.3), "all_a": (1.1, 0.2), "all_both": (1.1, 1.1),
              "none_present": (0.0, 0.0)}[nulls]
    a, am, b, bm = table(rng, n, fa, fb)
    if nulls == "none_present":
        am, bm = np.ones(n, bool), np.ones(n, bool)
    for flags in (0, et.KEEP_NULLS, et.WEEKDAYS_ONLY, et.KEEP_NULLS | et.WEEKDAYS_ONLY):
        check(three_modes(flags), a, am, b, bm)


@pytest.mark.parametrize("delta", [0, 1, I64_MAX, -1, I64_MIN])
def test_order_at_the_ends_of_int64(delta):
    """a wrapping difference gives the wrong answer on every one of these pairs"""
    ends = [I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX]
    pairs = list(itertools.product(ends, repeat=2))
    before = np.array([p[0] for p in pairs] * 3, np.int64)
    after = np.array([p[1] for p in pairs] * 3, np.int64)
    check([(et.ORDER, {"delta": delta})], before, None, after, None)
    # (the reference itself, held against the one case everybody can do in their head)
    assert et.counts(et.ORDER, {"delta": 0}, [I64_MIN], [I64_MAX]) == (1, 1, 0)
    assert et.counts(et.ORDER, {"delta": 0}, [I64_MAX], [I64_MIN]) == (1, 1, 1)


@pytest.mark.parametrize("unit", ["s", "ms", "us", "ns"])
def test_time_of_day_edges(unit):
    """negative timestamps, the tick before / at / after tod_lo, tod_hi and midnight, in every unit"""
    tps = et.TICKS[unit]
    day = DAY_S * tps
    lo, hi = 9 * 3600 * tps, 17 * 3600 * tps
    days = [-20000, -366, -2, -1, 0, 1, 2, 19000]
    ts = [d * day + e + k for d in days for e in (0, lo, hi, day) for k in (-1, 0, 1)]
    ts += [I64_MIN, I64_MIN + 1, I64_MAX - 1, I64_MAX, -1, 0, 1]
    ts = np.array([t for t in ts if I64_MIN <= t <= I64_MAX], np.int64)
    mask = np.ones(len(ts), bool)
    mask[::7] = False
    tasks = [(et.TIME_OF_DAY, tod_params(unit)), (et.TIME_OF_DAY, tod_params(unit, et.WEEKDAYS_ONLY)),
             (et.TIME_OF_DAY, tod_params(unit, 0, lo=17 * 3600, hi=9 * 3600)),  # lo > hi: nothing passes
             (et.TIME_OF_DAY, tod_params(unit, 0, lo=0, hi=0)), (et.TIME_OF_DAY, tod_params(unit, 0, lo=0, hi=DAY_S))]
    _, _, want = check(tasks, ts, mask, ts, None)
    assert want[2][2] == want[2][1] > 0


@pytest.mark.parametrize("unit", ["s", "ns"])
def test_weekday_filter_over_three_weeks_spanning_the_epoch(unit):
    tps = et.TICKS[unit]
    hours = np.arange(-11 * 24, 10 * 24, dtype=np.int64)  # every hour from 1969-12-21 to 1970-01-10
    ts = hours * 3600 * tps + 1800 * tps
    for flags in (et.WEEKDAYS_ONLY, et.WEEKDAYS_ONLY | et.KEEP_NULLS):
        _, _, want = check([(et.TIME_OF_DAY, tod_params(unit, flags))], ts, None, ts, None)
        assert want[0][1] == 15 * 24  # fifteen weekdays in three weeks


def test_range_bounds():
    rng = np.random.default_rng(6)
    n = 10_000
    t = rng.integers(-10**6, 10**6, n, dtype=np.int64)
    t[:8] = [I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, -500, 500, -501, 501]
    mask = rng.random(n) >= 0.1
    tasks = [(et.RANGE, {"lo": -500}), (et.RANGE, {"hi": 500}), (et.RANGE, {"lo": -500, "hi": 500}),
             (et.RANGE, {"lo": I64_MIN, "hi": I64_MAX}), (et.RANGE, {"lo": I64_MAX}), (et.RANGE, {"hi": I64_MIN}),
             (et.RANGE, {"lo": 500, "hi": -500}), (et.RANGE, {"lo": I64_MIN + 1, "hi": I64_MAX - 1, "flags": et.KEEP_NULLS})]
    check(tasks, t, mask, t, None)


def test_null_truth_table():
    """KEEP_NULLS x WEEKDAYS_ONLY x (NULL / weekday / weekend) x (passes / fails), row by row"""
    thursday_noon, saturday_noon = 12 * 3600, 2 * DAY_S + 12 * 3600
    thursday_night, saturday_night = 3600, 2 * DAY_S + 3600
    ts = np.array([thursday_noon, saturday_noon, thursday_night, saturday_night] * 2, np.int64)
    mask = np.array([True] * 4 + [False] * 4)
    expected = {0: (8, 4, 2), et.KEEP_NULLS: (8, 8, 6), et.WEEKDAYS_ONLY: (8, 2, 1),
                et.KEEP_NULLS | et.WEEKDAYS_ONLY: (8, 2, 1)}
    for flags, want in expected.items():
        st, _, ref = check([(et.TIME_OF_DAY, tod_params("s", flags))], ts, mask, ts, None)
        assert ref[0] == want
    # order mode: a NULL on either side
    before = np.array([0, 0, 0, 0, 5, 5, 5, 5], np.int64)
    after = np.array([1, 1, 1, 1, 0, 0, 0, 0], np.int64)
    bm = np.array([True, False, True, False] * 2)
    am = np.array([True, True, False, False] * 2)
    for flags, want in ((0, (8, 2, 1)), (et.KEEP_NULLS, (8, 8, 7))):
        _, _, ref = check([(et.ORDER, {"delta": 0, "flags": flags})], before, bm, after, am)
        assert ref[0] == want


BATCH_N = 300_000


@pytest.fixture(scope="module")
def big_table():
    rng = np.random.default_rng(7)
    a, am, b, bm = table(rng, BATCH_N)
    tasks = three_modes(et.KEEP_NULLS) + [(et.TIME_OF_DAY, tod_params("ms", et.WEEKDAYS_ONLY))]
    return a, am, b, bm, tasks, want_of(tasks, a, am, b, bm)


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192),
                                      (T.MEM_HOST_RETAINED, 8192), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001, 150_000]),
                                      (T.MEM_HOST, [3, 8195, 8196, 200_001])])
def test_batching_independence(big_table, mem, cuts):
    a, am, b, bm, tasks, want = big_table
    T.init()
    cols = [column(a, am, mem, 0), column(b, bm, mem, 0)]
    st = feed(plan_of(tasks), batches_of(cols, BATCH_N, cuts))
    assert [st.temporal_counts(i) for i in range(len(tasks))] == want


def test_no_coalesce(big_table):
    a, am, b, bm, tasks, want = big_table
    T.init(flags=T.OPT_NO_COALESCE)
    try:
        cols = [column(a, am, T.MEM_HOST, 0), column(b, bm, T.MEM_HOST, 0)]
        st = feed(plan_of(tasks), batches_of(cols, BATCH_N, 8192))
        assert [st.temporal_counts(i) for i in range(len(tasks))] == want
    finally:
        T.init(flags=0)


def test_fusion_leaves_the_other_kinds_bit_for_bit(big_table):
    a, am, b, bm, tasks, want = big_table
    T.init()
    cols = [column(a, am), column(b, bm)]
    others = [spec(T.COUNT, 0), spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE), spec(T.NUMERIC_STATS, 1),
              spec(T.COMOMENTS, 0, column2=1)]
    alone = feed(T.Plan(others), [cols]).finalize()
    plan = plan_of(tasks[:3], extra=others)
    st = feed(plan, [cols])
    res = st.finalize()
    assert [st.temporal_counts(i) for i in range(3)] == want[:3]
    import ctypes

    for got, ref in zip(res[3:], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))


def test_state_algebra(big_table):
    a, am, b, bm, tasks, want = big_table
    T.init()
    cols = [column(a, am), column(b, bm)]
    parts = batches_of(cols, BATCH_N, [100_000, 200_001])
    plan = plan_of(tasks)
    k = range(len(tasks))
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    assert [states[0].temporal_counts(i) for i in k] == want
    # serialize -> deserialize -> merge
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    assert [back.temporal_counts(i) for i in k] == want and back.serialize() == blob
    twice = feed(plan, [cols])
    twice.merge([back])
    assert [twice.temporal_counts(i) for i in k] == [tuple(2 * v for v in w) for w in want]
    # a blob counted under other parameters is refused
    other = plan_of([(et.ORDER, {"delta": 1, "flags": et.KEEP_NULLS})] + tasks[1:])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(other, blob)
    # reset; finalize, feed more, finalize again
    st = states[0]
    st.reset()
    assert [st.temporal_counts(i) for i in k] == [(0, 0, 0)] * len(tasks)
    st.update(parts[0])
    first = want_of(tasks, a[:100_000], am[:100_000], b[:100_000], bm[:100_000])
    assert [(r.total, r.non_null, r.non_null - r.matches) for r in st.finalize()] == first
    st.update(parts[1])
    st.update(parts[2])
    assert [(r.total, r.non_null, r.non_null - r.matches) for r in st.finalize()] == want


@pytest.mark.parametrize("world,device_buffers", [(2, True), (3, False)])
def test_threaded_ranks(big_table, world, device_buffers):
    """the way _run_ranks of tests/test_gpu_distributed_sim.py drives them: every rank a thread with its own state and
    row shard, tgx_allreduce over the thread-barrier transport; every rank ends with the table's counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    a, am, b, bm, tasks, want = big_table
    T.init()
    whole = [column(a, am), column(b, bm)]
    plan = plan_of(tasks, extra=[spec(T.COUNT, 0)])
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(BATCH_N, world, rank)
            st = T.State(plan)
            comm = thread_comm(group, rank, device_buffers=device_buffers)
            for _ in range(2):
                res = sharded_suite_step(plan, st, [c.sliced(lo, hi - lo) for c in whole], comm)
            results[rank] = (res, [st.temporal_counts(i) for i in range(len(tasks))])
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
        assert res[len(tasks)].total == BATCH_N


def test_other_column_types_are_unsupported_and_the_state_stays_usable():
    T.init()
    n = 1000
    good = column(np.arange(n, dtype=np.int64), None, T.MEM_HOST)
    f64 = T.Column.float64(np.arange(n, dtype=np.float64))
    i32 = T.Column.int32(np.arange(n, dtype=np.int32))
    u64 = T.Column.narrow(T.UINT64, np.arange(n, dtype=np.uint64))
    boolean = T.Column.boolean(np.zeros(n // 8 + 8, np.uint8), n)
    offs, data, _ = orc.utf8_from_list(["a%d" % i for i in range(n)])
    text = T.Column.utf8(offs, np.concatenate([data, np.zeros(64, np.uint8)]))
    tasks = [(et.ORDER, {"delta": 0})]
    st = T.State(plan_of(tasks))
    for bad in (f64, i32, text, u64, boolean):
        for cols in ([good, bad], [bad, good]):
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED"):
                st.update(cols)
    single = T.State(plan_of([(et.RANGE, {"lo": 0})]))
    for bad in (f64, i32, text, u64, boolean):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED"):
            single.update([bad])
    st.update([good, good])
    single.update([good])
    assert st.temporal_counts(0) == (n, n, 0) and single.temporal_counts(0) == (n, n, 0)


# ---- end to end: ValidationSuite.run over pyarrow tables ------------------------------------------------------------
def run_suite(table, constraints):
    """every constraint in a check of its own; returns [(status, metric, message)] in order"""
    import term_amd.suite as S

    T.init()
    sb = S.ValidationSuite.builder("temporal")
    for i, c in enumerate(constraints):
        sb.check(S.Check.builder("c%d" % i).level(S.Level.ERROR).constraint(c).build())
    res = sb.build().run(table)
    issues = {i.check_name: i for i in res.report.issues}
    out = []
    for i in range(len(constraints)):
        if "c%d" % i in issues:
            out.append(("Failure", issues["c%d" % i].metric, issues["c%d" % i].message))
        else:
            out.append(("Success", res.report.metrics.custom_metrics["c%d.temporal_ordering" % i], None))
    return out


def ts_array(values, mask, unit):
    import pyarrow as pa

    return pa.array([v if ok else None for v, ok in zip(values, mask)], type=pa.timestamp(unit))


def expected(kind, mode, params, cols, before, after=None, valid_b=None, valid_a=None):
    _, considered, violations = et.counts(mode, params, before, after, valid_b, valid_a)
    return et.verdict(kind, considered, violations, *cols)


def test_suite_on_the_reference_tables():
    import json
    import os

    import pyarrow as pa
    import term_amd.suite as S

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_ordering_vectors.json")) as f:
        golden = json.load(f)
    for case in golden["evaluated"]:
        before_col, after_col = case["builder"]["before_after"]
        before = [et.literal_ns(r[before_col]) for r in case["rows"]]
        after = [et.literal_ns(r[after_col]) for r in case["rows"]]
        table = pa.table({"id": pa.array([r["id"] for r in case["rows"]], pa.int64()),
                          before_col: pa.array(before, pa.timestamp("ns")), after_col: pa.array(after, pa.timestamp("ns"))})
        c = S.TemporalOrderingConstraint(case["builder"]["table"]).before_after(before_col, after_col)
        (got,) = run_suite(table, [c])
        want = expected("before_after", et.ORDER, {"delta": 0}, (before_col, after_col), before, after)
        assert got == want and got[0] == case["status"] and (got[2] is not None) == case["message_is_some"]


@pytest.mark.parametrize("unit", ["ns", "us", "s"])
def test_suite_on_timestamp_tables(unit):
    """one table per message text, allow_nulls both ways, tolerance 60 s -- status, metric and message from exact_temporal"""
    import pyarrow as pa
    import term_amd.suite as S

    tps = et.TICKS[unit]
    rng = np.random.default_rng(40 + tps % 7)
    n = 20_003
    created = rng.integers(-40 * 365 * DAY_S, 40 * 365 * DAY_S, n, dtype=np.int64) * tps + rng.integers(0, tps, n)
    processed = created + rng.integers(-30, 200, n, dtype=np.int64) * tps
    cm, pm = rng.random(n) >= 0.05, rng.random(n) >= 0.08
    cl, pl, cml, pml = created.tolist(), processed.tolist(), cm.tolist(), pm.tolist()
    table = pa.table({"created_at": ts_array(cl, cml, unit), "processed_at": ts_array(pl, pml, unit),
                      "late": ts_array((created + 300 * tps).tolist(), [True] * n, unit)})
    lo_text, hi_text = "1975-03-01 12:00:00.5", "2001-09-09T01:46:40Z"
    lo, hi = et.range_bounds(et.literal_ns(lo_text), et.literal_ns(hi_text), tps)
    new = S.TemporalOrderingConstraint
    cases = []
    for nulls in (False, True):
        keep = et.KEEP_NULLS if nulls else 0
        cases += [
            (new("data").before_after("created_at", "processed_at").allow_nulls(nulls),
             ("before_after", et.ORDER, {"delta": 0, "flags": keep}, ("created_at", "processed_at"), cl, pl, cml, pml)),
            (new("data").before_or_equal("created_at", "processed_at").tolerance_seconds(60).allow_nulls(nulls),
             ("before_after", et.ORDER, {"delta": 60 * tps + 1, "flags": keep}, ("created_at", "processed_at"), cl, pl, cml, pml)),
            (new("data").business_hours("created_at", "09:00", "17:00").weekdays_only(True).allow_nulls(nulls),
             ("business_hours", et.TIME_OF_DAY, dict(tod_params(unit, keep | et.WEEKDAYS_ONLY)), ("created_at",), cl, None, cml)),
            (new("data").business_hours("created_at", "00:00", "23:59").allow_nulls(nulls),
             ("business_hours", et.TIME_OF_DAY, dict(tod_params(unit, keep, lo=0, hi=23 * 3600 + 59 * 60)), ("created_at",), cl, None, cml)),
            (new("data").date_range("created_at", lo_text, hi_text).allow_nulls(nulls),
             ("date_range", et.RANGE, {"lo": lo, "hi": hi, "flags": keep}, ("created_at",), cl, None, cml)),
        ]
    # a rule that holds: Success with metric 1.0
    cases.append((new("data").before_after("created_at", "late"),
                  ("before_after", et.ORDER, {"delta": 0}, ("created_at", "late"), cl, (created + 300 * tps).tolist(), cml, None)))
    got = run_suite(table, [c for c, _ in cases])
    want = [expected(*args) for _, args in cases]
    assert got == want
    assert want[-1] == ("Success", 1.0, None) and {w[0] for w in want[:-1]} == {"Failure"}


def test_suite_hands_back_what_the_device_does_not_take():
    """MaxTimeGap, a zone other than UTC and an Int64 column under business hours are this constraint's error; the
    constraint beside them still gets its verdict"""
    import pyarrow as pa
    import term_amd.suite as S

    t = [0, 3600, 7200, 10 * 3600]
    table = pa.table({"a": pa.array(t, pa.timestamp("s")), "b": pa.array([x + 1 for x in t], pa.timestamp("s")),
                      "paris": pa.array(t, pa.timestamp("s", tz="Europe/Paris")), "plain": pa.array(t, pa.int64())})
    new = S.TemporalOrderingConstraint
    got = run_suite(table, [new("data").before_after("a", "b"), new("data").max_time_gap("a", 60),
                            new("data").business_hours("paris", "09:00", "17:00"),
                            new("data").business_hours("plain", "09:00", "17:00"),
                            new("data").before_after("plain", "b"), S.TemporalOrderingConstraint("data")])
    assert got[0] == ("Success", 1.0, None) and got[4] == ("Success", 1.0, None)
    prefix = "Error evaluating constraint: Constraint evaluation failed for 'temporal_ordering': "
    assert got[1][2].startswith(prefix + "MaxTimeGap validation")
    assert got[2][2].startswith(prefix + "business hours validation needs a column without a time zone")
    assert got[3][2].startswith(prefix + "business hours validation needs a Timestamp")
    assert got[5][2].startswith("Error evaluating constraint: Security error")
