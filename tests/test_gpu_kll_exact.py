"""-m gpu: KLL sketches against the exact ranks of tests/exact_quantiles.py, on every route a sketch can take.

Every sketch is held to check_sketch: its weight is the number of values exactly, every retained item is a value of
the column, the query answers what the library's rule gives on the exported levels bit for bit, the rank error stays
within the bound, and below 1024 values every quantile is the exact order statistic.  NULL rows hold a poison value
-- finite, and no value of the column -- so a sketch that reads one fails membership; NaN rows carry quiet, negative
and signalling payloads, scattered and in runs as long as a sampling group.

Routes (update.cpp, decide_fusion): below 2^23 rows a batch is sketched by kll_build_kernel as it is.  From 2^23 rows
on it is sampled: alone or next to NUMERIC_STATS the sampler rides on the scan (scan_kll_kernel), on a column of a
COMOMENTS pair on the pair scan (scan_pair_kernel), and next to APPROX_DISTINCT (the HyperLogLog lane has its own scan)
kll_build_kernel samples it itself.  The profile's "kll" bytes tell the two apart: the stand-alone build reads the
column (8 bytes a row), the scan route only sketches its picks and leftovers.

TGX_KLL_REPORT=<file>: the worst rank error seen per route and k is written there as JSON."""
import json
import os

import numpy as np
import pytest

import exact_quantiles as Q
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import numeric_column

pytestmark = pytest.mark.gpu

KS = [2, 8, 200, 2048, 65536]
FLOAT_KINDS = ["uniform", "sorted", "reversed", "ties", "constant", "lognormal", "inf_mix", "nan_payloads", "specials"]
INT_KINDS = ["i_small", "i_full", "i_above53", "i_epoch_ns"]
KINDS = FLOAT_KINDS + INT_KINDS
LAYOUTS = ["none", "rand5", "first_half", "runs64", "runs512", "all_null", "all_nan"]
F_POISON = 7.770000000000123e77
I_POISON = 3_141_592_653_589_793

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TGX_KLL_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({"%s k=%d" % key: v for key, v in sorted(WORST.items())}, f, indent=1)


def record(route, k, worst):
    WORST[(route, k)] = max(WORST.get((route, k), 0.0), worst)


NAN_BITS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FF4DEADBEEF0000, 0xFFF0000000000ABC]


def values(kind, m, rng):
    if kind == "uniform":
        return rng.random(m) * 1000
    if kind == "sorted":
        return np.arange(m, dtype=np.float64) * 0.5 - 7
    if kind == "reversed":
        return np.arange(m, 0, -1, dtype=np.float64)
    if kind == "ties":
        return rng.integers(0, 5, m).astype(np.float64) * 2.5
    if kind == "constant":
        return np.full(m, 42.25)
    if kind == "lognormal":  # about 600 decades
        return np.exp(rng.uniform(-690, 690, m)) * np.where(rng.random(m) < 0.3, -1, 1)
    if kind == "inf_mix":
        x = rng.standard_normal(m)
        x[rng.random(m) < 0.01] = np.inf
        x[rng.random(m) < 0.01] = -np.inf
        return x
    if kind == "nan_payloads":
        x = rng.standard_normal(m) * 100
        bits = x.view(np.uint64)
        at = rng.random(m) < 0.02
        bits[at] = np.array(NAN_BITS, dtype=np.uint64)[rng.integers(0, len(NAN_BITS), int(at.sum()))]
        for run in (2, 4, 8, 16, 1024, 4096):  # runs as long as a sampling group (2^top values) and longer
            if m > 4 * run:
                s = int(rng.integers(0, m - run))
                bits[s: s + run] = NAN_BITS[run % len(NAN_BITS)]
        return x
    if kind == "specials":  # +-0, denormals, +-DBL_MAX among ordinary values
        x = rng.standard_normal(m)
        pick = rng.integers(0, 8, m)
        sp = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072e-310, -1e-320, 1.7976931348623157e308,
                       -1.7976931348623157e308])
        at = rng.random(m) < 0.3
        x[at] = sp[pick[at]]
        return x
    if kind == "i_small":
        return rng.integers(-1000, 1000, m, dtype=np.int64)
    if kind == "i_full":
        x = rng.integers(-2 ** 63, 2 ** 63 - 1, m, dtype=np.int64, endpoint=True)
        if m:
            x[rng.integers(0, m, 3)] = np.iinfo(np.int64).min
            x[rng.integers(0, m, 3)] = np.iinfo(np.int64).max
        return x
    if kind == "i_above53":  # distinct integers that round to shared doubles
        return 2 ** 55 + rng.integers(0, 2 ** 14, m, dtype=np.int64)  # (8 integers a double)
    if kind == "i_epoch_ns":
        return 1_700_000_000_000_000_000 + rng.integers(0, 10 ** 9, m, dtype=np.int64)
    raise ValueError(kind)


def nulls(layout, m, rng):
    """validity mask over the m rows of the buffer"""
    r = np.arange(m)
    if layout in ("none", "all_nan"):
        return np.ones(m, bool)
    if layout == "rand5":
        return rng.random(m) >= 0.05
    if layout == "first_half":
        return r >= m // 2
    if layout == "runs64":  # NULL runs of whole 64-row words
        return (r // 64) % 3 != 1
    if layout == "runs512":  # NULL runs of whole 512-row scan tiles
        return (r // 512) % 2 == 0
    if layout == "all_null":
        return np.zeros(m, bool)
    raise ValueError(layout)


def table(kind, layout, n, offset=0, seed=0):
    """(values, validity, kept) of a column of n rows at Arrow offset `offset`; NULL slots hold a poison value"""
    rng = np.random.default_rng([seed, n, offset, KINDS.index(kind), LAYOUTS.index(layout)])
    m = n + offset
    vals = values(kind, m, rng)
    mask = nulls(layout, m, rng)
    if layout == "all_nan":
        if vals.dtype == np.int64:
            mask[:] = False  # (an Int64 column has no NaN: all NULL instead)
        else:
            vals = np.full(m, np.nan)
    poison = I_POISON if vals.dtype == np.int64 else F_POISON
    vals[~mask] = poison
    validity = None if mask.all() and layout in ("none", "all_nan") else orc.pack_validity(mask)
    kept = Q.kept(vals, validity, n=n, offset=offset)
    assert not (kept == float(poison)).any()
    return vals, validity, kept


def column(vals, validity, offset, n, device=True):
    return numeric_column(vals, validity, device, offset=offset, length=n)


def partner(n, offset):
    """a finite Float64 column laid out like the sketched one: the other side of a COMOMENTS pair"""
    rng = np.random.default_rng(n + 11)
    return numeric_column(rng.standard_normal(n + offset), None, True, offset=offset, length=n)


ROUTE_SPECS = {
    "alone": lambda k: [spec(T.KLL, 0, kll_k=k)],
    "stats": lambda k: [spec(T.KLL, 0, kll_k=k), spec(T.NUMERIC_STATS, 0)],
    "pair": lambda k: [spec(T.KLL, 0, kll_k=k), spec(T.COMOMENTS, 0, column2=1)],
    "hll": lambda k: [spec(T.KLL, 0, kll_k=k), spec(T.APPROX_DISTINCT, 0)],
}


def one_batch(route, k, vals, validity, offset, n):
    T.init()
    plan = T.Plan(ROUTE_SPECS[route](k))
    st = T.State(plan)
    st.profile_enable(True)
    cols = [column(vals, validity, offset, n)]
    if route == "pair":
        cols.append(partner(n, offset))
    st.update(cols)
    res = st.finalize()
    return plan, st, res


def check_route(route, st, n):
    """the route the batch took, from the profile (module docstring)"""
    if n == 0:
        return
    kll_bytes = st.profile_get("kll")["bytes"]
    sampled_on_scan = n >= 2 ** 23 and route != "hll"
    if sampled_on_scan:
        assert 0 < kll_bytes < 4 * n, (route, n, kll_bytes)
        assert st.profile_get("scan")["launches"] >= 1
        if route == "pair":
            assert st.profile_get("comoments")["launches"] == 0  # the pair rode on the scan
    else:
        assert kll_bytes >= 8 * n, (route, n, kll_bytes)  # kll_build_kernel read the column


# ---- one batch ----------------------------------------------------------------------------------------------------

SIZES = [0, 1, 2, 1023, 1024, 1025, 512 * 1024 - 1, 512 * 1024 + 1]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_one_batch(kind, layout):
    """every data kind x NULL layout at the sizes around level 0's capacity and a run boundary; offset 3 on every
    other size, the route and k rotate"""
    for i, n in enumerate(SIZES):
        offset = 3 * (i % 2)
        k = KS[i % len(KS)]
        route = ("alone", "stats", "pair", "hll")[i % 4]
        vals, validity, kept = table(kind, layout, n, offset)
        plan, st, res = one_batch(route, k, vals, validity, offset, n)
        worst = Q.check_sketch(st, 0, kept, k, result=res[0])
        check_route(route, st, n)
        record("build", k, worst)


@pytest.mark.parametrize("route", ["alone", "stats", "pair", "hll"])
@pytest.mark.parametrize("n", [2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 + 12345])
def test_sampler_threshold(n, route):
    """kll_top_for: sampling starts at 2^23 rows, the level rises again at 2^24; every route on both sides"""
    i = [2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 + 12345].index(n) + ["alone", "stats", "pair", "hll"].index(route)
    kind = ("uniform", "nan_payloads", "i_full", "ties", "lognormal", "specials", "i_epoch_ns")[i % 7]
    layout = ("rand5", "runs512", "none", "first_half", "runs64")[i % 5]
    k = KS[i % len(KS)]
    offset = 3 * (i % 2)
    vals, validity, kept = table(kind, layout, n, offset, seed=5)
    plan, st, res = one_batch(route, k, vals, validity, offset, n)
    check_route(route, st, n)
    worst = Q.check_sketch(st, 0, kept, k, result=res[0])
    record(("build" if n < 2 ** 23 else "sampled_build" if route == "hll" else "scan_" + route), k, worst)


@pytest.mark.parametrize("k", KS)
def test_k_values(k):
    """every k on a sampled batch and on an unsampled one: the device sketch does not depend on k, the bound does"""
    for n, kind in ((2 ** 23 + 77, "uniform"), (3_000_001, "lognormal")):
        vals, validity, kept = table(kind, "rand5", n, 0, seed=k)
        plan, st, res = one_batch("stats", k, vals, validity, 0, n)
        record("k_values", k, Q.check_sketch(st, 0, kept, k, result=res[0]))


# ---- batches, streams and the life of a state -----------------------------------------------------------------------

def feed(st, vals, validity, cuts, device=True, retained=False):
    keep = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        sub_v = vals[a:b]
        sub_valid = None if validity is None else orc.pack_validity(Q.valid_mask(len(vals), validity)[a:b])
        c = numeric_column(sub_v, sub_valid, device)
        if retained:
            c.c.mem = T.MEM_HOST_RETAINED
        keep.append((sub_v, sub_valid))
        st.update([c])
    return keep


@pytest.mark.parametrize("kind", ["uniform", "nan_payloads", "i_full", "specials"])
def test_ragged_batches(kind):
    n = 1_500_000
    vals, validity, kept = table(kind, "rand5", n, 0, seed=9)
    cuts = [0, 1, 8, 1031, 1031 + 4097, 70_000, 70_001, 600_000, 1_100_003, n]
    T.init()
    plan = T.Plan([spec(T.KLL, 0, kll_k=200), spec(T.NUMERIC_STATS, 0)])
    st = T.State(plan)
    feed(st, vals, validity, cuts)
    res = st.finalize()
    record("ragged", 200, Q.check_sketch(st, 0, kept, 200, result=res[0]))


@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("mem", ["device", "host", "retained"])
def test_streams(mem, coalesce):
    """8192-row batches (coalesced into bigger launches unless TGX_OPT_NO_COALESCE), and a stream of 37-row batches
    that stays below 1024 values: exact"""
    try:
        T.init(flags=0 if coalesce else T.OPT_NO_COALESCE)
        for n, step, kind, k in ((300_003, 8192, "nan_payloads", 2048), (1000, 37, "ties", 8), (1100, 37, "i_above53", 2)):
            vals, validity, kept = table(kind, "runs64", n, 0, seed=13)
            plan = T.Plan([spec(T.KLL, 0, kll_k=k)])
            st = T.State(plan)
            keep = feed(st, vals, validity, list(range(0, n, step)) + [n], device=mem == "device",
                        retained=mem == "retained")
            res = st.finalize()
            del keep
            record("stream_" + mem, k, Q.check_sketch(st, 0, kept, k, result=res[0]))
    finally:
        T.init()


@pytest.mark.parametrize("small", [False, True])
def test_finalize_half_way_sync_then_reset_onto_another_column(small):
    n = 900 if small else 2_000_000
    vals, validity, _ = table("lognormal", "runs512", n, 0, seed=21)
    cuts = [0, n // 7, n // 3, n // 2, 2 * n // 3, n - 5, n]
    T.init()
    plan = T.Plan([spec(T.KLL, 0, kll_k=200), spec(T.COUNT, 0)])
    st = T.State(plan)
    feed(st, vals, validity, cuts[:4])
    res = st.finalize()
    Q.check_sketch(st, 0, Q.kept(vals[: cuts[3]], orc.pack_validity(Q.valid_mask(n, validity)[: cuts[3]])), 200,
                   result=res[0])
    for a, b in zip(cuts[3:-1], cuts[4:]):
        feed(st, vals, validity, [a, b])
        st.sync()
    res = st.finalize()
    Q.check_sketch(st, 0, Q.kept(vals, validity), 200, result=res[0])
    # reset, then a different table: an Int64 column beyond 2^53
    st.reset()
    iv, iva, ikept = table("i_above53", "rand5", n // 2 + 1, 0, seed=22)
    feed(st, iv, iva, [0, n // 4, n // 2 + 1])
    res = st.finalize()
    record("resume_reset", 200, Q.check_sketch(st, 0, ikept, 200, result=res[0]))


@pytest.mark.parametrize("n", [1000, 2_500_000, 2 ** 23 + 9])
def test_five_states_merged_in_two_orders(n):
    vals, validity, kept = table("specials" if n < 2 ** 23 else "uniform", "rand5", n, 0, seed=31)
    T.init()
    plan = T.Plan([spec(T.KLL, 0, kll_k=2048), spec(T.NUMERIC_STATS, 0)])
    cuts = [0, n // 9, n // 4, n // 2, n // 2 + 1, n] if n < 2 ** 23 else [0, n - 1, n - 1, n - 1, n - 1, n]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = T.State(plan)
        feed(s, vals, validity, [a, b])
        parts.append(s)
    for order in ([0, 1, 2, 3, 4], [4, 2, 0, 3, 1]):
        m = T.State(plan)
        m.merge([parts[i] for i in order])
        res = m.finalize()
        record("merge", 2048, Q.check_sketch(m, 0, kept, 2048, result=res[0]))


@pytest.mark.parametrize("n", [1023, 3_000_000])
def test_blob_keeps_the_levels_bit_for_bit(n):
    vals, validity, kept = table("nan_payloads", "first_half", n, 0, seed=41)
    T.init()
    plan = T.Plan([spec(T.KLL, 0, kll_k=200)])
    st = T.State(plan)
    feed(st, vals, validity, [0, n // 3, n])
    st.finalize()
    back = T.State.deserialize(plan, st.serialize())
    s0, lv0 = Q.export(st, 0)
    s1, lv1 = Q.export(back, 0)
    assert s0 == s1
    assert [x.tobytes() for x in lv0.levels] == [x.tobytes() for x in lv1.levels]
    for phi in Q.phi_grid(len(kept)):
        assert np.float64(st.kll_quantile(0, phi)).tobytes() == np.float64(back.kll_quantile(0, phi)).tobytes()
    record("blob", 200, Q.check_sketch(back, 0, kept, 200))


@pytest.mark.parametrize("n", [1000, 1_200_000])
@pytest.mark.parametrize("world", [2, 3, 8])
def test_threaded_ranks(world, n):
    from test_gpu_distributed_sim import _run_ranks

    vals, validity, kept = table("i_epoch_ns" if n < 2000 else "inf_mix", "rand5", n, 0, seed=51 + world)
    mask = Q.valid_mask(n, validity)
    cuts = [n * r // world for r in range(world + 1)]
    T.init()
    plan = T.Plan([spec(T.KLL, 0, kll_k=200), spec(T.NUMERIC_STATS, 0)])

    def shards_of(rank):
        a, b = cuts[rank], cuts[rank + 1]
        return [numeric_column(vals[a:b], orc.pack_validity(mask[a:b]), True)]

    out = _run_ranks(world, plan, shards_of)
    for res, st in out:  # every rank holds the sketch of the whole table
        record("ranks", 200, Q.check_sketch(st, 0, kept, 200, result=res[0]))


@pytest.mark.parametrize("n", [1000, 2 ** 23 + 1])
def test_specs_with_different_k_keep_separate_sketches(n):
    vals, validity, kept = table("uniform", "rand5", n, 0, seed=61)
    T.init()
    plan = T.Plan([spec(T.KLL, 0, kll_k=200), spec(T.KLL, 0, kll_k=2048), spec(T.KLL, 0, kll_k=200)])
    st = T.State(plan)
    feed(st, vals, validity, [0, n])
    res = st.finalize()
    for si, k in ((0, 200), (1, 2048), (2, 200)):
        Q.check_sketch(st, si, kept, k, result=res[si])
    lv = [Q.export(st, si)[1] for si in range(3)]
    assert [x.tobytes() for x in lv[0].levels] == [x.tobytes() for x in lv[2].levels]  # equal k: one sketch
    if n >= 2 ** 23:  # the first rode on the scan, the other was built from the column: another sample
        assert [x.tobytes() for x in lv[0].levels] != [x.tobytes() for x in lv[1].levels]
