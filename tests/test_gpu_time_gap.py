"""-m gpu: TGX_CHECK_TIME_GAP, the LAG() window behind TemporalOrderingConstraint's MaxTimeGap mode
(TG/constraints/temporal_ordering.rs:454-481).  The reference is tests/exact_time_gap.py -- per partition sorted(),
Python integers, neither the library nor the oracle -- and ALL FIVE counters (seen, rows, gaps, violations, largest_gap)
are compared for equality; there are no tolerances."""
import functools
import threading

import numpy as np
import pytest

import exact_time_gap as eg
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, to_device

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = eg.I64_MIN, eg.I64_MAX
NP_TYPES = {T.INT64: np.int64, T.INT32: np.int32, T.UINT8: np.uint8, T.INT8: np.int8, T.INT16: np.int16,
            T.UINT16: np.uint16, T.UINT32: np.uint32}


def column(vals, mask, mem=T.MEM_DEVICE, type_id=T.INT64):
    vals = np.ascontiguousarray(vals, NP_TYPES[type_id])
    validity = None if mask is None else pad_validity(orc.pack_validity(np.asarray(mask, bool)))
    if mem == T.MEM_DEVICE:
        vals, validity = to_device(vals), to_device(validity)
    return T.Column(type_id, len(vals), values=vals, validity=validity, mem=mem)


def batches_of(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n] if isinstance(cuts, int) else [0] + list(cuts) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def plan_of(max_gaps, grouped, extra=()):
    """one TIME_GAP spec per threshold, all on (column 0, column 1 or none)"""
    plan = T.Plan([spec(T.TIME_GAP, 0, column2=1 if grouped else -1) for _ in max_gaps] + list(extra))
    for i, m in enumerate(max_gaps):
        plan.set_time_gap(i, m)
    return plan


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def lst(a):
    return None if a is None else np.asarray(a).tolist()


def want_of(max_gaps, t, tm, g=None, gm=None):
    return [eg.counts(m, lst(t), lst(tm), lst(g), lst(gm)) for m in max_gaps]


def check(max_gaps, t, tm=None, g=None, gm=None, mem=T.MEM_DEVICE, cuts=None, gtype=T.INT64, want=None):
    """feeds the table, reads every spec twice (the second read comes from the cached answer) and through tgx_finalize"""
    T.init()
    cols = [column(t, tm, mem)] + ([column(g, gm, mem, gtype)] if g is not None else [])
    plan = plan_of(max_gaps, g is not None)
    st = feed(plan, batches_of(cols, len(t), cuts))
    want = want_of(max_gaps, t, tm, g, gm) if want is None else want
    assert [st.time_gap_counts(i) for i in range(len(max_gaps))] == want
    assert [st.time_gap_counts(i) for i in range(len(max_gaps))] == want
    for r, (seen, _, gaps, violations, _) in zip(st.finalize(), want):
        assert (r.total, r.non_null, r.matches) == (seen, gaps, gaps - violations)
    return st, plan, want


# ---- edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 2047, 2048, 2049])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    t = rng.integers(-10**6, 10**6, n, dtype=np.int64)
    g = rng.integers(0, 3, n, dtype=np.int64)
    check([100, 0], t)
    check([100, 0], t, rng.random(n) >= 0.3, g, rng.random(n) >= 0.3)


def test_all_timestamps_null():
    n = 5000
    t = np.arange(n, dtype=np.int64)
    _, _, want = check([0], t, np.zeros(n, bool))
    assert want == [(n, 0, 0, 0, 0)]
    check([0], t, np.zeros(n, bool), t % 7, None)


def test_all_timestamps_equal():
    """the sort's equality bucket: every gap is 0"""
    n = 70_000
    t = np.full(n, 1_700_000_000_000, np.int64)
    _, _, want = check([0, -1], t)
    assert want == [(n, n, n - 1, 0, 0), (n, n, n - 1, n - 1, 0)]
    _, _, want = check([0, -1], t, None, np.arange(n, dtype=np.int64) % 9, None)
    assert want[0] == (n, n, n - 9, 0, 0)


def test_int64_extremes_are_an_unsigned_gap():
    t = np.array([I64_MAX, I64_MIN], np.int64)
    _, _, want = check([I64_MAX, -1, 0], t)
    assert want[0] == (2, 2, 1, 1, (1 << 64) - 1)
    t = np.array([5, I64_MAX, -7, I64_MIN, I64_MAX - 1, I64_MIN + 1, 0] * 3, np.int64)
    check([I64_MAX, I64_MAX - 8, 0], t)
    check([I64_MAX, I64_MAX - 8, 0], t, None, np.arange(len(t), dtype=np.int64) % 2, None)


def test_neighbours_above_2_53_stay_apart():
    """a CAST AS DOUBLE on the way into the sort would merge them"""
    base = 1 << 53
    t = np.array([base + 2, base, base + 1] * 1000, np.int64)
    _, _, want = check([0, 1], t)
    assert want[0] == (3000, 3000, 2999, 2, 1)
    far = (1 << 62) + np.random.default_rng(2).permutation(50_000).astype(np.int64)
    _, _, want = check([0, 1], far)
    assert want == [(50_000, 50_000, 49_999, 49_999, 1), (50_000, 50_000, 49_999, 0, 1)]


@pytest.mark.parametrize("max_gap", [-1, 0, I64_MAX, 1000, 999])
def test_thresholds(max_gap):
    """a gap at max_gap is none, one at max_gap + 1 is: the table has gaps of exactly 999, 1000 and 1001"""
    t = np.cumsum(np.array([0, 999, 1000, 1001, 0, 1000, 1, 5000] * 500, np.int64))
    rng = np.random.default_rng(3)
    _, _, want = check([max_gap], rng.permutation(t))
    if max_gap == 1000:
        assert want[0][3] == 2 * 500  # the 1001s and the 5000s


# ---- grouped ---------------------------------------------------------------------------------------------------------
def test_null_group_partition_beside_real_groups():
    rng = np.random.default_rng(4)
    n = 30_001
    t = rng.integers(0, 10**7, n, dtype=np.int64)
    g = rng.integers(-3, 4, n, dtype=np.int64)
    gm = rng.random(n) >= 0.25
    _, _, want = check([500, 5000], t, rng.random(n) >= 0.1, g, gm)
    per_row = eg.counts(500, t.tolist(), None, (np.arange(n) + 100).tolist(), None)
    assert want[0][2] > per_row[2] == 0  # (splitting the NULL group row by row would lose its gaps)
    # every group NULL: one partition, the ungrouped answer
    _, _, all_null = check([500], t, None, g, np.zeros(n, bool))
    assert all_null == want_of([500], t, None)


def test_group_keys_at_the_int64_extremes():
    rng = np.random.default_rng(5)
    n = 10_000
    t = rng.integers(-10**9, 10**9, n, dtype=np.int64)
    g = rng.choice(np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], np.int64), n)
    check([10**5], t, None, g, rng.random(n) >= 0.1)


def test_every_row_its_own_group_and_one_group_for_all():
    rng = np.random.default_rng(6)
    n = 40_000
    t = rng.integers(0, 10**6, n, dtype=np.int64)
    _, _, want = check([10], t, None, rng.permutation(n).astype(np.int64) - n // 2, None)
    assert want == [(n, n, 0, 0, 0)]
    _, _, one = check([10], t, None, np.full(n, 77, np.int64), None)
    assert one == want_of([10], t, None)


def test_interleaved_groups_with_overlapping_timestamps():
    n = 90_000
    i = np.arange(n, dtype=np.int64)
    t = (i // 3) * 10 + (i % 3)  # three sensors reporting in turn, their timestamps interleaved
    g = i % 3
    g[i % 3 == 2] = 40  # (group keys not in rank order of first appearance)
    t[7 * 3] += 3000  # one late report: one long gap before it, none after (it moved behind its successors)
    _, _, want = check([10, 9], t, None, g, None)
    assert want[0][2] == n - 3 and want[0][3] >= 1 and want[1][3] > want[0][3]


@pytest.mark.parametrize("gtype,lo,hi", [(T.INT32, -2**31, 2**31), (T.UINT8, 0, 256), (T.INT8, -2**7, 2**7),
                                         (T.INT16, -2**15, 2**15), (T.UINT16, 0, 2**16), (T.UINT32, 0, 2**32)])
def test_widened_group_columns(gtype, lo, hi):
    """every type the staging widens for the group column: the type's minimum, its maximum and a value next to each
    (an unsigned maximum read as signed, or a sign not extended, would merge or split partitions)"""
    rng = np.random.default_rng(7 + gtype)
    n = 25_000
    t = rng.integers(0, 10**6, n, dtype=np.int64)
    g = rng.choice(np.array([lo, lo + 1, -1 if lo < 0 else 128, hi - 2, hi - 1]), n)
    assert (g.astype(NP_TYPES[gtype]).astype(np.int64) == g).all() and {lo, lo + 1, hi - 2, hi - 1} <= set(g.tolist())
    for mem in (T.MEM_DEVICE, T.MEM_HOST):
        check([50], t, rng.random(n) >= 0.05, g, rng.random(n) >= 0.2, mem=mem, gtype=gtype)


def test_unsupported_column_types_and_the_state_stays_usable():
    T.init()
    n = 1000
    good = column(np.arange(n, dtype=np.int64), None, T.MEM_HOST)
    f64 = T.Column.float64(np.arange(n, dtype=np.float64))
    i32 = T.Column.int32(np.arange(n, dtype=np.int32))
    u64 = T.Column.narrow(T.UINT64, np.arange(n, dtype=np.uint64))
    boolean = T.Column.boolean(np.zeros(n // 8 + 8, np.uint8), n)
    offs, data, _ = orc.utf8_from_list(["a%d" % i for i in range(n)])
    text = T.Column.utf8(offs, np.concatenate([data, np.zeros(64, np.uint8)]))
    st = T.State(plan_of([5], True))
    for bad in (text, f64, u64, boolean):  # as the group column
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*TIME_GAP"):
            st.update([good, bad])
    for bad in (text, f64, u64, boolean, i32):  # as the timestamp column
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*TIME_GAP"):
            st.update([bad, good])
    st.update([good, good])
    assert st.time_gap_counts(0) == (n, n, 0, 0, 0)


# ---- every route of the sort at small n -----------------------------------------------------------------------------------
SORT_SHAPES = {
    "one_pass": (20_000, dict(TGX_SORT_TARGET="512", TGX_SORT_CAP="1024")),
    "two_passes": (60_000, dict(TGX_SORT_TARGET="32", TGX_SORT_CAP="128", TGX_SORT_SPLIT="31", TGX_SORT_SAMPLE="8")),
    "three_passes": (60_000, dict(TGX_SORT_TARGET="16", TGX_SORT_CAP="64", TGX_SORT_SPLIT="15")),
    "chunked_last_pass": (20_000, dict(TGX_SORT_TARGET="300", TGX_SORT_CAP="64", TGX_SORT_SLOWCAP="128",
                                       TGX_SORT_SPLIT="31", TGX_SORT_SAMPLE="2")),
    "many_stretches": (60_000, dict(TGX_SORT_TARGET="16", TGX_SORT_CAP="64", TGX_SORT_SPLIT="15", TGX_SORT_PARTS="64")),
    "shipped": (300_000, {}),
}
DATA_KINDS = ["shuffled", "sorted", "reversed", "heavy_ties"]
ROUTE_GAPS = [0, 40, -1]


@functools.lru_cache(maxsize=None)
def route_table(kind, n):
    """(t, t validity, g, g validity) and the exact counters without and with the group column: computed once per
    (kind, n), shared by the shapes"""
    rng = np.random.default_rng(n + DATA_KINDS.index(kind))
    if kind == "shuffled":
        t = rng.integers(-10**7, 10**7, n, dtype=np.int64)
    elif kind == "sorted":
        t = np.cumsum(rng.integers(0, 80, n, dtype=np.int64)) - 10**6
    elif kind == "reversed":
        t = (np.cumsum(rng.integers(0, 80, n, dtype=np.int64)) - 10**6)[::-1].copy()
    else:  # half the rows one instant, the rest on 50 more
        t = rng.integers(0, 50, n, dtype=np.int64) * 1000
        t[rng.random(n) < 0.5] = 25_500
    tm = rng.random(n) >= 0.05
    g = rng.integers(0, 37, n, dtype=np.int64) * 1_000_003 - 17
    gm = rng.random(n) >= 0.1
    return t, tm, g, gm, want_of(ROUTE_GAPS, t, tm), want_of(ROUTE_GAPS, t, tm, g, gm)


@pytest.mark.parametrize("grouped", [False, True], ids=["whole_table", "per_group"])
@pytest.mark.parametrize("kind", DATA_KINDS)
@pytest.mark.parametrize("shape", list(SORT_SHAPES))
def test_sort_routes(shape, kind, grouped, monkeypatch):
    n, env = SORT_SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t, tm, g, gm, plain, per_group = route_table(kind, n)
    if grouped:
        check(ROUTE_GAPS, t, tm, g, gm, want=per_group)
    else:
        check(ROUTE_GAPS, t, tm, want=plain)


@pytest.mark.parametrize("grouped", [False, True], ids=["whole_table", "per_group"])
@pytest.mark.parametrize("shape", ["two_passes", "three_passes"])
def test_room_from_the_sample(shape, grouped, monkeypatch, capfd):
    n, env = SORT_SHAPES[shape]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TGX_SORT_OPTIMISTIC_MIN", "1")
    monkeypatch.setenv("TGX_SORT_DEBUG", "1")
    t, tm, g, gm, plain, per_group = route_table("shuffled", n)
    if grouped:
        check(ROUTE_GAPS, t, tm, g, gm, want=per_group)
    else:
        check(ROUTE_GAPS, t, tm, want=plain)
    assert "room from the sample" in capfd.readouterr().err


@pytest.mark.parametrize("grouped", [False, True], ids=["whole_table", "per_group"])
def test_a_full_bucket_is_counted_again(grouped, monkeypatch, capfd):
    """no slack on the sample's estimate: a bucket is full, the job says so in its status word, and the counted rerun
    -- from the untouched rows -- answers"""
    n, env = SORT_SHAPES["two_passes"]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TGX_SORT_OPTIMISTIC_MIN", "1")
    monkeypatch.setenv("TGX_SORT_SIGMAS_X2", "0")
    monkeypatch.setenv("TGX_SORT_DEBUG", "1")
    t, tm, g, gm, plain, per_group = route_table("shuffled", n)
    if grouped:
        check(ROUTE_GAPS, t, tm, g, gm, want=per_group)
    else:
        check(ROUTE_GAPS, t, tm, want=plain)
    assert "again with counted buckets" in capfd.readouterr().err


# ---- batching -----------------------------------------------------------------------------------------------------------
BATCH_N = 100_000
BATCH_GAPS = [0, 25]


@pytest.fixture(scope="module")
def batch_table():
    rng = np.random.default_rng(8)
    t = rng.integers(-10**6, 10**6, BATCH_N, dtype=np.int64)
    tm = rng.random(BATCH_N) >= 0.1
    g = rng.integers(0, 500, BATCH_N, dtype=np.int64)
    gm = rng.random(BATCH_N) >= 0.15
    return t, tm, g, gm, want_of(BATCH_GAPS, t, tm), want_of(BATCH_GAPS, t, tm, g, gm)


@pytest.mark.parametrize("grouped", [False, True], ids=["whole_table", "per_group"])
@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_DEVICE, 8192), (T.MEM_HOST, 8192),
                                      (T.MEM_HOST, None), (T.MEM_DEVICE, [1, 64, 65, 4097, 70_001]),
                                      (T.MEM_HOST, [3, 8195, 8196, 60_001])])
def test_batching_independence(batch_table, mem, cuts, grouped):
    t, tm, g, gm, plain, per_group = batch_table
    if grouped:
        check(BATCH_GAPS, t, tm, g, gm, mem=mem, cuts=cuts, want=per_group)
    else:
        check(BATCH_GAPS, t, tm, mem=mem, cuts=cuts, want=plain)


def test_mixed_memory_spaces(batch_table):
    t, tm, g, gm, _, per_group = batch_table
    T.init()
    dev = [column(t, tm), column(g, gm)]
    host = [column(t, tm, T.MEM_HOST), column(g, gm, T.MEM_HOST)]
    bounds = [0, 5000, 13_192, 21_384, 60_000, BATCH_N]
    st = T.State(plan_of(BATCH_GAPS, True))
    for k, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        st.update([c.sliced(lo, hi - lo) for c in (dev if k % 2 else host)])
    assert [st.time_gap_counts(i) for i in range(2)] == per_group


@pytest.mark.parametrize("grouped", [False, True], ids=["whole_table", "per_group"])
def test_read_half_way_reset_and_reuse(batch_table, grouped):
    t, tm, g, gm, plain, per_group = batch_table
    T.init()
    cols = [column(t, tm)] + ([column(g, gm)] if grouped else [])
    half = BATCH_N // 2 + 13
    first, second = batches_of(cols, BATCH_N, [half])
    k = range(len(BATCH_GAPS))
    st = T.State(plan_of(BATCH_GAPS, grouped))
    st.update(first)
    want_half = want_of(BATCH_GAPS, t[:half], tm[:half], *((g[:half], gm[:half]) if grouped else ()))
    assert [st.time_gap_counts(i) for i in k] == want_half
    for b in batches_of(second, BATCH_N - half, 8192):  # (the arrays grow past their first size: the rows move)
        st.update(b)
    whole = per_group if grouped else plain
    assert [st.time_gap_counts(i) for i in k] == whole
    assert [st.time_gap_counts(i) for i in k] == whole  # a second read without a new batch
    st.reset()
    assert [st.time_gap_counts(i) for i in k] == [(0, 0, 0, 0, 0)] * len(BATCH_GAPS)
    st.update(first)
    assert [st.time_gap_counts(i) for i in k] == want_half


# ---- plans ----------------------------------------------------------------------------------------------------------------
def test_more_thresholds_than_one_pass_compares():
    """eleven specs on one (t, g): one retained copy, one sort, two neighbour passes"""
    rng = np.random.default_rng(9)
    n = 20_000
    t = rng.integers(0, 10**5, n, dtype=np.int64)
    g = rng.integers(0, 20, n, dtype=np.int64)
    gaps = [-1, 0, 1, 2, 5, 10, 50, 100, 1000, I64_MAX, 3]
    _, _, want = check(gaps, t, None, g, rng.random(n) >= 0.1)
    assert len({w[3] for w in want}) > 6
    check(gaps, t)


def test_beside_other_checks_on_the_same_column(batch_table):
    """TIME_GAP beside NUMERIC_STATS and TEMPORAL on the timestamp column: their answers are bit for bit what they are
    alone, and an ungrouped and a grouped task share the plan"""
    import ctypes

    t, tm, g, gm, plain, per_group = batch_table
    T.init()
    cols = [column(t, tm), column(g, gm)]
    others = [spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE), spec(T.TEMPORAL, 0), spec(T.COUNT, 1),
              spec(T.NUMERIC_STATS, 1)]
    alone_plan = T.Plan(others)
    alone_plan.set_temporal(1, T.TEMPORAL_RANGE, lo=0)
    alone = feed(alone_plan, [cols]).finalize()
    plan = T.Plan([spec(T.TIME_GAP, 0, column2=-1), spec(T.TIME_GAP, 0, column2=1)] + others)
    plan.set_time_gap(0, BATCH_GAPS[1])
    plan.set_time_gap(1, BATCH_GAPS[1])
    plan.set_temporal(3, T.TEMPORAL_RANGE, lo=0)
    st = feed(plan, batches_of(cols, BATCH_N, [40_000]))
    res = st.finalize()
    assert st.time_gap_counts(0) == plain[1] and st.time_gap_counts(1) == per_group[1]
    for got, ref in zip(res[2:], alone):
        assert ctypes.string_at(ctypes.addressof(got), ctypes.sizeof(got)) == \
            ctypes.string_at(ctypes.addressof(ref), ctypes.sizeof(ref))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a TIME_GAP"):
        st.time_gap_counts(2)


# ---- four tasks over three columns: every column in both roles, one task grouped by its own timestamps ---------------
FOUR_N = 30_011
FOUR_SPECS = [(0, 1, 5), (2, 2, 0), (0, -1, 0), (1, 0, 1), (0, 1, -1), (0, -1, 7), (2, 2, -1), (0, 1, 100), (1, 0, 40)]
FOUR_TASKS = [(0, -1), (0, 1), (1, 0), (2, 2)]
FOUR_CUTS = [1, 64, 65, 4097, 4100, 12_288, 20_481, 29_999]


@pytest.fixture(scope="module")
def four_tasks_table():
    """three Int64 columns a, b, c with NULLs in all of them, and the exact counters of every spec of FOUR_SPECS"""
    rng = np.random.default_rng(10)
    vals = [rng.integers(-1500, 1500, FOUR_N, dtype=np.int64) * 7, rng.integers(0, 400, FOUR_N, dtype=np.int64) - 200,
            rng.integers(-(2**40), 2**40, FOUR_N, dtype=np.int64)]
    vals[2][rng.random(FOUR_N) < 0.4] = vals[2][0]  # (one value of c many times over, the rest nearly distinct)
    masks = [rng.random(FOUR_N) >= rate for rate in (0.05, 0.1, 0.2)]
    want = [eg.counts(m, lst(vals[ct]), lst(masks[ct]), *((lst(vals[cg]), lst(masks[cg])) if cg >= 0 else (None, None)))
            for ct, cg, m in FOUR_SPECS]
    return vals, masks, want


def four_tasks_plan(specs):
    plan = T.Plan([spec(T.TIME_GAP, ct, column2=cg) for ct, cg, _ in specs])
    for i, (_, _, m) in enumerate(specs):
        plan.set_time_gap(i, m)
    return plan


@pytest.mark.parametrize("order", ["as_planned", "backwards"])
@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST], ids=["device", "host"])
def test_four_tasks_over_three_columns(four_tasks_table, mem, order):
    """(a, -), (a, b), (b, a), (c, c) in one plan, their specs interleaved: every spec's counters are the reference's
    and what its task gives in a plan of its own -- the tasks share the sort's work buffers and are answered one after
    the other, in the order they are first read"""
    vals, masks, want = four_tasks_table
    T.init()
    cols = [column(v, m, mem) for v, m in zip(vals, masks)]
    batches = batches_of(cols, FOUR_N, FOUR_CUTS)
    st = feed(four_tasks_plan(FOUR_SPECS), batches)
    reads = list(range(len(FOUR_SPECS)))
    if order == "backwards":
        reads.reverse()
    got = {i: st.time_gap_counts(i) for i in reads}
    assert [got[i] for i in range(len(FOUR_SPECS))] == want
    assert [st.time_gap_counts(i) for i in range(len(FOUR_SPECS))] == want  # the cached answers
    for r, (seen, _, gaps, violations, _) in zip(st.finalize(), want):
        assert (r.total, r.non_null, r.matches) == (seen, gaps, gaps - violations)
    for task in FOUR_TASKS:
        mine = [i for i, sp in enumerate(FOUR_SPECS) if sp[:2] == task]
        assert mine, task
        alone = feed(four_tasks_plan([FOUR_SPECS[i] for i in mine]), batches)
        assert [alone.time_gap_counts(k) for k in range(len(mine))] == [got[i] for i in mine], task


def test_grouped_by_its_own_timestamps(four_tasks_table):
    """(c, c): every partition holds one instant, so every gap is 0, there are as many gaps as rows beyond the first of
    each distinct value, and a NULL c is a NULL timestamp: dropped, never a NULL group"""
    vals, masks, want = four_tasks_table
    c, cm = vals[2], masks[2]
    rows, distinct = int(cm.sum()), len(set(c[cm].tolist()))
    assert rows - distinct > FOUR_N // 4
    for (ct, cg, max_gap), w in zip(FOUR_SPECS, want):
        if (ct, cg) == (2, 2):
            assert w == (FOUR_N, rows, rows - distinct, rows - distinct if max_gap < 0 else 0, 0)
    check([0, -1], c, cm, c, cm, cuts=FOUR_CUTS, want=[want[1], want[6]])


def test_merge_and_serialize_are_refused_on_a_state_that_holds_rows():
    T.init()
    plan = plan_of([5], True)
    cols = [column(np.arange(100, dtype=np.int64), None), column(np.arange(100, dtype=np.int64) % 3, None)]
    full, empty, other = feed(plan, [cols]), T.State(plan), T.State(plan)
    for call in (full.serialize, lambda: empty.merge([full])):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*TIME_GAP"):
            call()
    # an empty one passes, both ways
    blob = empty.serialize()
    empty.merge([other, T.State.deserialize(plan, blob)])
    full.merge([empty])
    assert full.time_gap_counts(0) == (100, 100, 97, 0, 3)
    # rows that were all NULL are rows seen: still not mergeable
    nulls = feed(plan, [[column(np.arange(8, dtype=np.int64), np.zeros(8, bool)), cols[1].sliced(0, 8)]])
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*TIME_GAP"):
        nulls.serialize()
    full.reset()
    assert full.serialize() == blob


def test_allreduce_is_refused_with_the_checks_name():
    import torch
    from term_amd.distributed import ThreadGroup, thread_comm

    T.init()
    world = 2
    plan = plan_of([5], False, extra=[spec(T.COUNT, 0)])
    whole = column(np.arange(4096, dtype=np.int64), None)
    group = ThreadGroup(world)
    refused, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            st = T.State(plan)
            st.update([whole.sliced(rank * 2048, 2048)])  # (every rank holds rows: every rank refuses before it exchanges)
            comm = thread_comm(group, rank)
            try:
                st.allreduce(comm)
            except T.TgxError as e:
                refused[rank] = str(e)
            assert st.time_gap_counts(0) == (2048, 2048, 2047, 0, 1)  # the state is as it was
            st.reset()
            st.allreduce(comm)  # an empty one passes
            assert st.time_gap_counts(0) == (0, 0, 0, 0, 0)
        except Exception:  # noqa: BLE001
            import traceback

            errors.append((rank, traceback.format_exc()))
            group.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not errors, errors
    assert not any(th.is_alive() for th in threads), "a rank is stuck"
    for text in refused:
        assert text is not None and "TGX_UNSUPPORTED" in text and "TIME_GAP" in text and "tgx_allreduce" in text


# ---- end to end: ValidationSuite.run over pyarrow tables ----------------------------------------------------------------
def run_suite(table, constraints):
    """every constraint in a check of its own; returns [(status, metric, message)] in order"""
    import term_amd.suite as S

    T.init()
    sb = S.ValidationSuite.builder("time_gap")
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


@pytest.mark.parametrize("unit", ["ms", "ns"])
def test_suite_with_the_window_on_the_device(unit):
    import pyarrow as pa
    import term_amd.suite as S

    tps = eg.TICKS[unit]
    rng = np.random.default_rng(30 + tps % 11)
    n = 20_003
    sensor = rng.integers(0, 40, n, dtype=np.int64)
    seconds = rng.integers(0, 86400 * 30, n, dtype=np.int64)
    ts = seconds * tps + rng.integers(0, tps, n)
    tm, sm = rng.random(n) >= 0.05, rng.random(n) >= 0.1
    tl, tml, sl, sml = ts.tolist(), tm.tolist(), sensor.tolist(), sm.tolist()
    table = pa.table({
        "ts": pa.array([v if ok else None for v, ok in zip(tl, tml)], pa.timestamp(unit, tz="Europe/Paris")),
        "sensor": pa.array([v if ok else None for v, ok in zip(sl, sml)], pa.int32()),
        "later": pa.array((ts + tps).tolist(), pa.timestamp(unit, tz="Europe/Paris")),
        "name": pa.array(["s%d" % v for v in sl], pa.string()),
        "day": pa.array(seconds.tolist(), pa.int64())})
    new = S.TemporalOrderingConstraint
    cases = [(new("data").max_time_gap("ts", 600).window_on_device(True), (600, None)),
             (new("data").max_time_gap("ts", 86400 * 40).window_on_device(True), (86400 * 40, None)),
             (new("data").max_time_gap("ts", 3600 * 6).group_by("sensor").window_on_device(True), (3600 * 6, "sensor")),
             (new("data").max_time_gap("ts", 86400 * 40).group_by("sensor").allow_nulls(True).window_on_device(True),
              (86400 * 40, "sensor"))]
    extra = [new("data").before_after("ts", "later"), new("data").max_time_gap("ts", 600),
             new("data").max_time_gap("day", 600).window_on_device(True),
             new("data").max_time_gap("ts", 600).group_by("name").window_on_device(True)]
    got = run_suite(table, [c for c, _ in cases] + extra)
    want = []
    for _, (secs, group) in cases:
        _, _, gaps, violations, _ = eg.counts(eg.max_gap_ticks(secs, unit), tl, tml, sl if group else None,
                                              sml if group else None)
        want.append(eg.verdict(gaps, violations))
    assert got[:4] == want
    assert [w[0] for w in want] == ["Failure", "Success", "Failure", "Success"]
    # the constraints beside them: BeforeAfter still gets its verdict (a NULL ts is dropped, the rest pass), the plain
    # MaxTimeGap and the columns the device path does not take keep their errors
    assert got[4] == ("Success", 1.0, None)
    prefix = "Error evaluating constraint: Constraint evaluation failed for 'temporal_ordering': "
    assert got[5][2].startswith(prefix + "MaxTimeGap validation is a LAG() OVER")
    assert got[6][2].startswith(prefix + "max time gap validation on the device needs a Timestamp")
    assert got[7][0] == "Failure" and "TIME_GAP" in got[7][2]
