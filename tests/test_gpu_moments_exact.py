"""-m gpu: VARIANCE / STDDEV (NUMERIC_STATS with FLAG_VARIANCE) and the co-moments (COMOMENTS: CORR, COVAR_SAMP, the
correlation analyzer's sums) against the EXACT moments of tests/exact_moments.py -- not against a Welford restatement,
which is itself inexact on offset data.

Both kernels sum about a pivot picked on the device near the data (scan_pivot_kernel, como_pivot_kernel); these tests
feed the layouts where the first look at a batch sees no valid value: leading NULL runs of 4095 .. 200 000 rows, whole
all-NULL batches ahead of the data, sparse validity, masks and NaN / inf values that leave both looks without a
finite value (the first one lies past the search's first round, or in another workgroup's stretch); in one batch, in
coalesced 8192-row streams, across finalize / reset / a recycled state, merged, serialized and over threaded ranks.

Error budget of the variance.  One batch: the lanes sum x - p and (x - p)^2 about one pivot p near the data, and the
batch's M2 = s2 - s1^2 / n loses nothing worth counting when |mean - p| is about sigma: 1e-9 relative.  Every batch's
(n, mean, M2) then enters Chan's merge, whose delta of two means carries the rounding of those means, about eps |mean|
each (fuzz_plans.py, check_stats): relative to M2 that is 4 eps (|mean| / sigma) / sqrt(rows per merged part) in all
(`var_tol`).  Routes that merge parts of states or ranks are held to the north star's 1e-6 on data with
mean / sigma <= 1e8.  A constant column has a variance of exactly 0, as DataFusion's Welford gives."""
import math

import numpy as np
import pytest

import exact_moments as X
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, rel_err, to_device

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
NORTH_STAR = 1e-6
BIG = 1_048_576 + 37  # many workgroups and the reduce kernel
SMALL = 6_000         # one workgroup: the scan folds into the running state itself


def data(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "i64_epoch_ms":
        return 1_700_000_000_000 + rng.integers(0, 10 ** 8, size=n, dtype=np.int64)
    if kind == "i64_epoch_ns":
        return 1_700_000_000_000_000_000 + rng.integers(0, 3 * 10 ** 10, size=n, dtype=np.int64)
    if kind == "i64_wide":  # |x| in [2^62, 2^63): the 128-bit sum carries across partials, merges and ranks
        mag = rng.integers(2 ** 62, 2 ** 63 - 1, size=n, dtype=np.int64)
        return np.where(rng.random(n) < 0.7, mag, -mag)
    if kind == "f64_1e9":
        return 1e9 + rng.standard_normal(n)
    if kind == "f64_epoch":
        return 1.7e9 + 1000.0 * rng.standard_normal(n)
    if kind == "f64_int":  # integer-valued: every partial sum is exact below 2^53
        return (1_700_000_000 + rng.integers(0, 10 ** 6, size=n)).astype(np.float64)
    if kind == "f64_cancel":  # sum(|x|) / |sum(x)| near 1e15
        v = rng.standard_normal(n // 2) * 1e6
        x = np.concatenate([v, -v, [1e-3] * (n - 2 * (n // 2))])
        x = x[rng.permutation(n)]
        x[np.argmax(x > 0)] += 1e-3
        return x
    if kind == "f32_1e4":
        return (1e4 + rng.standard_normal(n)).astype(np.float32)
    if kind == "i32_high":
        return (2 ** 31 - 2 ** 20 + rng.integers(0, 2 ** 20 - 1, size=n)).astype(np.int32)
    if kind == "u32_epoch":  # a narrow type widened on the device
        return (1_700_000_000 + rng.integers(0, 10 ** 7, size=n)).astype(np.uint32)
    if kind == "control":
        return 1.0 + 3.0 * rng.standard_normal(n)
    if kind == "const0":
        return np.zeros(n)
    if kind == "const_epoch":
        return np.full(n, 1.7e9 + 0.1)
    if kind == "const_huge":  # the mean of 4096 of them overflows a plain sum
        return np.full(n, 1.5e305)
    if kind == "f64_nan":  # NaN among the valid values: SUM and VARIANCE are NaN
        x = 1e9 + rng.standard_normal(n)
        x[rng.random(n) < 0.001] = np.nan
        return x
    if kind == "f64_inf_lead":  # valid but infinite first rows (no finite value for the first look); SUM is inf
        x = 1.7e9 + 1000.0 * rng.standard_normal(n)
        x[:5000] = np.inf
        return x
    if kind == "f64_nan_stride":  # finite values only after row 300 000 and off look 1's rows: the search's value test
        x = np.full(n, np.nan)
        x[300_000:] = 1e9 + rng.standard_normal(n - 300_000)
        x[np.arange(4096) * (n // 4096)] = np.nan
        return x
    raise ValueError(kind)


KINDS = ["i64_epoch_ms", "i64_epoch_ns", "i64_wide", "f64_1e9", "f64_epoch", "f64_int", "f64_cancel", "f32_1e4",
         "i32_high", "u32_epoch", "control", "const0", "const_epoch", "const_huge", "f64_nan", "f64_inf_lead",
         "f64_nan_stride"]


def layout(name, n, seed=1):
    """validity as a bool mask (None: no bitmap)"""
    if name == "none":
        return None
    m = np.ones(n, dtype=bool)
    if name.startswith("lead"):
        m[: int(name[4:])] = False
    elif name == "sparse":
        m = np.random.default_rng(seed).random(n) < 0.001
    elif name == "stride":
        # valid everywhere EXCEPT the rows the co-moment pivot sampler reads today (k * (n // 4096)): chosen against
        # the current sampler to force a miss; what is asserted does not depend on it
        m[np.arange(4096) * (n // 4096)] = False
    elif name.startswith("search"):
        # valid from row int(name[6:]) on, except the rows of both looks today (the first 4096, k * (n // 4096)): the
        # first valid row lies past the first round of the search (and, from 600 000, in another workgroup's stretch)
        m[: int(name[6:])] = False
        m[np.arange(4096) * (n // 4096)] = False
    else:
        raise ValueError(name)
    return m


def packed(mask):
    return None if mask is None else orc.pack_validity(mask)


def column(vals, validity, device, offset=0, length=None):
    """a NUMERIC column view of any of the kinds above; validity: packed bits (or None)"""
    n = len(vals) - offset if length is None else length
    v = pad_validity(validity)
    buf = vals.view(np.int32) if vals.dtype == np.uint32 else vals  # (same bits; torch has no uint32 copies)
    if device:
        buf, v = to_device(buf), to_device(v)
    if vals.dtype == np.int64:
        return T.Column.int64(buf, v, length=n, offset=offset)
    if vals.dtype == np.float64:
        return T.Column.float64(buf, v, length=n, offset=offset)
    if vals.dtype == np.float32:
        return T.Column.float32(buf, v, length=n, offset=offset)
    if vals.dtype == np.int32:
        return T.Column.int32(buf, v, length=n, offset=offset)
    return T.Column.narrow(T.UINT32, buf, v, length=n, offset=offset)


def var_spec(col=0):
    return spec(T.NUMERIC_STATS, col, flags=T.FLAG_VARIANCE)


def var_tol(ref, rows_per_merge=None):
    """1e-9, plus Chan's budget when batches of about `rows_per_merge` rows are merged (module docstring)"""
    tol = 1e-9
    if rows_per_merge and ref.finite and ref.var_samp > 0:
        valid_per_part = max(1.0, rows_per_merge * ref.n / ref.total)  # (the rows of a part that have values)
        tol += 4 * EPS * abs(ref.mean) / math.sqrt(ref.var_samp) / math.sqrt(valid_per_part)
    return tol


def same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def check_stats(r, ref, tol, exact_float_sum=False):
    what = (r.var_samp, ref.var_samp, r.sum_f, ref.sum_f)
    assert (r.total, r.non_null, bool(r.has_variance)) == (ref.total, ref.n, ref.has_variance), what
    if ref.n == 0:
        return
    if ref.integer:
        assert (r.sum_i, r.sum_f) == (ref.sum_i_wrapping, ref.sum_f), (r.sum_i, ref.sum_i_wrapping, r.sum_f, ref.sum_f)
    elif exact_float_sum or not ref.finite or math.isinf(ref.sum_f):
        assert same(r.sum_f, ref.sum_f), what
    else:
        assert rel_err(r.sum_f, ref.sum_f) <= 1e-9, what
    if ref.finite and not math.isinf(ref.sum_f):
        assert rel_err(r.mean, ref.mean) <= 1e-9, (r.mean, ref.mean)
    if not ref.has_variance:
        return
    if not ref.finite:
        assert math.isnan(r.var_samp), what
    elif ref.var_samp == 0.0:
        assert (r.var_samp, r.stddev_samp) == (0.0, 0.0), what
    else:
        assert rel_err(r.var_samp, ref.var_samp) <= tol, what + (tol,)
        assert rel_err(r.stddev_samp, ref.stddev_samp) <= tol, (r.stddev_samp, ref.stddev_samp, tol)


def pair_data(n, seed=3, kind="f64"):
    rng = np.random.default_rng(seed)
    if kind == "i64":
        x = 1_700_000_000_000 + rng.integers(0, 10 ** 6, size=n, dtype=np.int64)
        y = 300_000_000_000 + (x - 1_700_000_000_000) // 2 + rng.integers(-1000, 1000, size=n, dtype=np.int64)
        return x, y
    x = 1.7e9 + 1000.0 * rng.standard_normal(n)
    y = 3e8 + 0.5 * (x - 1.7e9) + 100.0 * rng.standard_normal(n)
    return x, y


def check_como(r, ref):
    """CORR / COVAR_SAMP through the host's verdict code, the centred and the raw sums: all against the exact values"""
    from test_gpu_correlation import metrics_of

    assert (r.total, r.non_null) == (ref.total, ref.n)
    if ref.n < 2:
        return
    scale = math.sqrt(float(ref.m2_x) * float(ref.m2_y))
    assert rel_err(r.co_m2_x, float(ref.m2_x)) <= 1e-9, (r.co_m2_x, float(ref.m2_x))
    assert rel_err(r.co_m2_y, float(ref.m2_y)) <= 1e-9, (r.co_m2_y, float(ref.m2_y))
    assert abs(r.co_c_xy - float(ref.c_xy)) <= 1e-9 * scale, (r.co_c_xy, float(ref.c_xy))
    pearson, covar, _ = metrics_of(r)
    assert abs(pearson - ref.corr) <= 1e-9, (pearson, ref.corr)
    assert abs(covar - ref.covar_samp) <= 1e-9 * scale / (ref.n - 1), (covar, ref.covar_samp)
    for got, want in ((r.sum_x, ref.sum_x), (r.sum_y, ref.sum_y), (r.sum_x2, ref.sum_x2), (r.sum_y2, ref.sum_y2),
                      (r.sum_xy, ref.sum_xy)):
        assert rel_err(got, float(want)) <= 1e-9, (got, float(want))


@pytest.fixture(autouse=True)
def _init():
    T.init()


# ---- one DEVICE batch ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lay", ["none", "lead4095", "lead4096", "lead4097", "lead200000", "sparse", "search50000",
                                 "search600000"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_batch_variance(kind, lay):
    for n in (SMALL, BIG):
        if (lay == "lead200000" or lay.startswith("search") or kind == "f64_nan_stride") and n < 600_000:
            continue
        vals = data(kind, n, seed=n)
        v = packed(layout(lay, n))
        st = T.State(T.Plan([var_spec()]))
        st.update([column(vals, v, True)])
        check_stats(st.finalize()[0], X.moments(vals, v), var_tol(None), exact_float_sum=kind == "f64_int")


def test_wide_int64_sum_of_two_million():
    n = 2_000_003
    vals = data("i64_wide", n, seed=5)
    v = packed(layout("lead4096", n))
    ref = X.moments(vals, v)
    assert abs(int(ref.sum)) > 2 ** 80  # far outside Int64: the high word carries
    st = T.State(T.Plan([var_spec()]))
    st.update([column(vals, v, True)])
    check_stats(st.finalize()[0], ref, var_tol(None))


@pytest.mark.parametrize("lay", ["none", "lead4096", "lead200000", "sparse", "stride", "search50000", "search600000"])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_one_batch_comoments(kind, fused, lay):
    """COMOMENTS alone takes the stand-alone kernel; with NUMERIC_STATS of both columns a big batch rides on the scan"""
    specs = [spec(T.COMOMENTS, 0, column2=1)] + ([spec(T.NUMERIC_STATS, 0), spec(T.NUMERIC_STATS, 1)] if fused else [])
    for n in (SMALL, BIG):
        if (lay == "lead200000" or lay.startswith("search")) and n < 600_000:
            continue
        x, y = pair_data(n, seed=n, kind=kind)
        xv = packed(layout(lay, n))
        yv = packed(layout("sparse", n, seed=9)) if lay == "sparse" else None
        if lay == "sparse":
            xv = yv  # 0.1 % of the PAIRS valid
        st = T.State(T.Plan(specs))
        st.update([column(x, xv, True), column(y, yv, True)])
        check_como(st.finalize()[0], X.comoments(x, y, xv, yv))


# ---- whole all-NULL batches ahead of the data ------------------------------------------------------------------------

@pytest.mark.parametrize("empty", [1, 4, 5, 6])
@pytest.mark.parametrize("device", [True, False])
def test_all_null_batches_before_the_data(empty, device):
    """`empty` batches (each its own pass: 70 000 rows are not coalesced) whose x and y are all NULL, then the data:
    the variance of x and the co-moments of (x, y), stand-alone and riding on the scan"""
    rows, n_data = 70_000, 300_000
    n = empty * rows + n_data
    x, y = pair_data(n, seed=empty)
    m = np.ones(n, dtype=bool)
    m[: empty * rows] = False
    v = packed(m)
    cuts = [k * rows for k in range(empty + 1)] + [n]
    for specs in ([var_spec(0), spec(T.COMOMENTS, 0, column2=1)],
                  [spec(T.COMOMENTS, 0, column2=1), spec(T.NUMERIC_STATS, 0), spec(T.NUMERIC_STATS, 1)]):
        st = T.State(T.Plan(specs))
        for a, b in zip(cuts[:-1], cuts[1:]):
            st.update([column(x, v, device, a, b - a), column(y, v, device, a, b - a)])
        res = st.finalize()
        como = res[1] if specs[0].kind == T.NUMERIC_STATS else res[0]
        check_como(como, X.comoments(x, y, v, v))
        if specs[0].kind == T.NUMERIC_STATS:
            check_stats(res[0], X.moments(x, v), var_tol(X.moments(x, v), n_data))


# ---- coalesced 8192-row streams ---------------------------------------------------------------------------------------

STREAM_KINDS = ["i64_epoch_ms", "i64_epoch_ns", "i64_wide", "f64_1e9", "f64_epoch", "f64_int", "f64_cancel", "f32_1e4",
                "i32_high", "u32_epoch", "const_epoch", "const_huge"]


def feed(plan, cols, cuts, device, monkeypatch, flush_rows):
    if flush_rows:
        monkeypatch.setenv("TGX_COALESCE_FLUSH_ROWS", flush_rows)
    st = T.State(plan)
    if flush_rows:
        monkeypatch.delenv("TGX_COALESCE_FLUSH_ROWS")
    for a, b in zip(cuts[:-1], cuts[1:]):
        st.update([column(vals, v, device, a, b - a) for vals, v in cols])
    return st


@pytest.mark.parametrize("flush_rows", [None, "20000"])
@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("lay", ["none", "lead4096", "lead200000", "sparse"])
def test_coalesced_streams(lay, device, flush_rows, monkeypatch):
    """every stream kind's variance and a pair's co-moments, fed as 8192-row batches through the coalescer"""
    n = 400_000 + 123
    cols = []
    for i, kind in enumerate(STREAM_KINDS):
        cols.append((data(kind, n, seed=i), packed(layout(lay, n, seed=100 + i))))
    x, y = pair_data(n, seed=17)
    pv = packed(layout(lay, n, seed=99))
    cols += [(x, pv), (y, None)]
    k = len(STREAM_KINDS)
    plan = T.Plan([var_spec(i) for i in range(k)] + [spec(T.COMOMENTS, k, column2=k + 1)])
    cuts = list(range(0, n, 8192)) + [n]
    res = feed(plan, cols, cuts, device, monkeypatch, flush_rows).finalize()
    # Chan merges happen on every one of these routes: the UInt32 column keeps DEVICE batches on the immediate path (a
    # pass per 8192-row batch), and a HOST stream under the default flush goes up in pieces of a few MB; an 8192-row
    # batch is the smallest part any of them folds
    per_merge = 20_000 if flush_rows and not device else 8192
    for i, kind in enumerate(STREAM_KINDS):
        ref = X.moments(*cols[i])
        check_stats(res[i], ref, var_tol(ref, per_merge), exact_float_sum=kind == "f64_int")
    check_como(res[k], X.comoments(x, y, pv, None))


# ---- finalize half-way, reset, a recycled state --------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i64_epoch_ms", "f64_1e9", "u32_epoch"])
def test_finalize_half_way_then_more(kind):
    n = 600_000
    vals = data(kind, n, seed=4)
    v = packed(layout("lead4096", n))
    x, y = pair_data(n, seed=4)
    half = 300_032
    st = T.State(T.Plan([var_spec(0), spec(T.COMOMENTS, 1, column2=2)]))
    st.update([column(vals, v, True, 0, half), column(x, v, True, 0, half), column(y, None, True, 0, half)])
    res = st.finalize()
    check_stats(res[0], X.moments(vals, v, n=half), var_tol(None))
    check_como(res[1], X.comoments(x, y, v, None, n=half))
    st.update([column(vals, v, True, half, n - half), column(x, v, True, half, n - half),
               column(y, None, True, half, n - half)])
    res = st.finalize()
    ref = X.moments(vals, v)
    check_stats(res[0], ref, var_tol(ref, half))
    check_como(res[1], X.comoments(x, y, v, None))


def test_reset_then_a_table_elsewhere():
    """the pivots of the first table must not outlive a reset: the second table lies 5e12 away"""
    n = 500_000
    rng = np.random.default_rng(8)
    first, second = 1e9 + rng.standard_normal(n), -5e12 + rng.standard_normal(n)
    fy, sy = 2 * first + rng.standard_normal(n), 3 * second + rng.standard_normal(n)
    v = packed(layout("lead4097", n))
    st = T.State(T.Plan([var_spec(0), spec(T.COMOMENTS, 0, column2=1)]))
    st.update([column(first, v, True), column(fy, None, True)])
    res = st.finalize()
    check_stats(res[0], X.moments(first, v), var_tol(None))
    check_como(res[1], X.comoments(first, fy, v, None))
    st.reset()
    st.update([column(second, None, True), column(sy, None, True)])
    res = st.finalize()
    check_stats(res[0], X.moments(second), var_tol(None))
    check_como(res[1], X.comoments(second, sy))


def test_new_state_after_destroying_one_with_pivots():
    """device blocks are recycled: a state created right after one with pivots set must start without them"""
    n = 400_000
    rng = np.random.default_rng(12)
    first, second = 1e9 + rng.standard_normal(n), -5e12 + rng.standard_normal(n)
    fy, sy = 2 * first + rng.standard_normal(n), 3 * second + rng.standard_normal(n)
    plan = T.Plan([var_spec(0), spec(T.COMOMENTS, 0, column2=1)])
    for _ in range(2):
        st = T.State(plan)
        st.update([column(first, None, True), column(fy, None, True)])
        st.finalize()
        st.close()
        st = T.State(plan)
        st.update([column(second, None, True), column(sy, None, True)])
        res = st.finalize()
        check_stats(res[0], X.moments(second), var_tol(None))
        check_como(res[1], X.comoments(second, sy))
        st.close()


# ---- merge, serialize, ranks ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["i64_epoch_ms", "i64_wide", "f64_epoch", "f64_int", "f64_cancel"])
def test_merge_with_an_all_null_first_part_and_serialize(kind):
    n = 2_000_000 + 11
    vals = data(kind, n, seed=21)
    x, y = pair_data(n, seed=21)
    m = np.ones(n, dtype=bool)
    cuts = [0, 500_000, 1_200_000, n]
    m[: cuts[1]] = False  # the first part: all NULL
    m[cuts[1]: cuts[1] + 5000] = False  # the second: NULLs first
    v = packed(m)
    plan = T.Plan([var_spec(0), spec(T.COMOMENTS, 1, column2=2)])
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        s = T.State(plan)
        s.update([column(vals, v, True, a, b - a), column(x, v, True, a, b - a), column(y, None, True, a, b - a)])
        parts.append(s)
    merged = T.State(plan)
    merged.merge(parts)
    back = T.State.deserialize(plan, merged.serialize())
    ref, cref = X.moments(vals, v), X.comoments(x, y, v, None)
    for st in (merged, back):
        res = st.finalize()
        check_stats(res[0], ref, NORTH_STAR, exact_float_sum=kind == "f64_int")
        check_como(res[1], cref)


@pytest.mark.parametrize("rank0", ["all_null", "nulls_first"])
def test_threaded_ranks(rank0):
    from test_gpu_distributed_sim import _run_ranks
    from term_amd.distributed import shard_rows

    world, n = 4, 2_400_000 + 64 * 3
    kinds = ["i64_epoch_ms", "i64_wide", "f64_epoch", "f64_int", "u32_epoch", "f64_cancel"]
    cols = [data(k, n, seed=30 + i) for i, k in enumerate(kinds)]
    x, y = pair_data(n, seed=31)
    lo0, hi0 = shard_rows(n, world, 0)
    m = np.ones(n, dtype=bool)
    m[lo0: hi0 if rank0 == "all_null" else lo0 + 4096] = False
    v = packed(m)
    k = len(kinds)
    plan = T.Plan([var_spec(i) for i in range(k)] + [spec(T.COMOMENTS, k, column2=k + 1)])

    def shards_of(rank):
        lo, hi = shard_rows(n, world, rank)
        return [column(c, v, True, lo, hi - lo) for c in cols + [x]] + [column(y, None, True, lo, hi - lo)]

    results = _run_ranks(world, plan, shards_of)
    first = results[0][0]
    for i, kind in enumerate(kinds):
        check_stats(first[i], X.moments(cols[i], v), NORTH_STAR, exact_float_sum=kind == "f64_int")
    check_como(first[k], X.comoments(x, y, v, None))
    for res, _st in results[1:]:  # every rank ends with the whole table's state
        for a, b in zip(res, first):
            assert a.sum_i == b.sum_i
            assert all(same(getattr(a, f), getattr(b, f)) for f in ("var_samp", "sum_f", "co_c_xy", "co_m2_x"))


# ---- end to end -----------------------------------------------------------------------------------------------------

def test_suite_stddev_and_mean_on_a_nulls_first_epoch_column():
    import pyarrow as pa

    from term_amd.suite import Assertion, Check, Level, ValidationSuite

    n, lead = 1_500_000, 300_000
    vals = np.sort(1.7e9 + 86400.0 * np.random.default_rng(40).random(n))
    m = np.ones(n, dtype=bool)
    m[:lead] = False
    ref = X.moments(vals, packed(m))
    tbl = pa.table({"ts": pa.array(vals, mask=~m)})  # sorted NULLS FIRST

    def around(v):
        return Assertion.Between(v * (1 - 1e-6), v * (1 + 1e-6))

    chk = (Check.builder("chk").level(Level.ERROR)
           .has_standard_deviation("ts", around(ref.stddev_samp)).has_mean("ts", around(ref.mean)).build())
    r = ValidationSuite.builder("s").check(chk).build().run(tbl)
    assert r.is_success() and r.report.metrics.passed_checks == 2, r.to_json()
