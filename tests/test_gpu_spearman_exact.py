"""-m gpu: SPEARMAN against the independent rank reference of tests/exact_ranks.py, on every route the ranking takes.

Each result is held to the reference: n pairs exactly, the five sums of the default spec bit for bit the doubles of
the sums wrapped mod 2^64, those of a TGX_FLAG_EXACT_RANK_SUMS spec the doubles of the exact sums (one rounding to
nearest even of a 128-bit integer), and the coefficient CorrelationAnalyzer computes from them equal to the library
formula on those doubles and within the error their rounding allows of the exact rho.

Data: every special value and many NaN payloads of both signs, Int64 near +-2^63 and runs beyond 2^53 that tie under
CAST AS DOUBLE, Float32 with signalling NaNs (ranked as their quiet CAST), constant and two-valued columns, long tie
runs, NULLs on one side only.  Routes: the lent first batch, several batches, HOST and coalesced streams, a cached
finalize then more rows, reset, two pairs sharing the work arrays, threaded ranks through tgx_allreduce, and the sample
sort's pass and bucket edges under the shapes of tests/test_gpu_spearman.py."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import exact_ranks as R
import oracle_binding as orc
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from gpu_util import numeric_column
from test_gpu_numeric32 import col32
from test_gpu_spearman import SORT_SHAPES

pytestmark = pytest.mark.gpu

NAN_BITS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FF4DEADBEEF0000,
            0xFFF0000000000ABC, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF]
SPECIAL_BITS = NAN_BITS + [0x7FF0000000000000, 0xFFF0000000000000, 0, 1 << 63, 1, (1 << 63) | 1, 0x000FFFFFFFFFFFFF,
                           0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF]
F32_SPECIALS = [0x7F800001, 0x7FC00001, 0xFF800001, 0xFFC00001, 0x7FBFFFFF, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0,
                0x80000000, 1, 0x80000001, 0x7F7FFFFF]
KINDS = ["specials", "nan_payloads", "i64_ends", "i64_above53", "f32_snan", "constant", "two_values", "tie_runs",
         "normal", "i64_small"]


def values(kind, n, rng):
    if kind == "specials":
        x = rng.standard_normal(n)
        at = rng.random(n) < 0.3
        x.view(np.uint64)[at] = np.array(SPECIAL_BITS, np.uint64)[rng.integers(0, len(SPECIAL_BITS), int(at.sum()))]
        return x
    if kind == "nan_payloads":  # thousands of distinct payloads of both signs
        x = rng.standard_normal(n)
        at = rng.random(n) < 0.2
        pay = rng.integers(1, 1 << 52, int(at.sum()), dtype=np.uint64)
        sign = rng.integers(0, 2, int(at.sum()), dtype=np.uint64) << np.uint64(63)
        x.view(np.uint64)[at] = sign | np.uint64(0x7FF0000000000000) | pay
        return x
    if kind == "i64_ends":
        x = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64, endpoint=True)
        at = rng.random(n) < 0.2
        x[at] = np.array([-2 ** 63, -2 ** 63 + 1, -2 ** 63 + 512, -2 ** 63 + 513, 2 ** 63 - 1, 2 ** 63 - 512,
                          2 ** 63 - 513, 2 ** 63 - 1024], np.int64)[rng.integers(0, 8, int(at.sum()))]
        return x
    if kind == "i64_above53":  # runs of distinct integers that one double stands for
        return (2 ** 55 + rng.integers(0, 2 ** 12, n, dtype=np.int64)) * np.where(rng.random(n) < 0.5, 1, -1)
    if kind == "f32_snan":
        x = (rng.standard_normal(n) * 10).astype(np.float32)
        at = rng.random(n) < 0.25
        x.view(np.uint32)[at] = np.array(F32_SPECIALS, np.uint32)[rng.integers(0, len(F32_SPECIALS), int(at.sum()))]
        return x
    if kind == "constant":
        return np.full(n, 3.25)
    if kind == "two_values":
        return rng.integers(0, 2, n).astype(np.int64) * 7 - 3
    if kind == "tie_runs":  # a few long runs of one value, the rest spread
        x = np.round(rng.standard_normal(n), 3)
        for v in (0.0, -0.0, 1.5):
            s = int(rng.integers(0, max(1, n - n // 5)))
            x[s: s + n // 5] = v
        return x
    if kind == "normal":
        return rng.standard_normal(n)
    if kind == "i64_small":
        return rng.integers(-50, 50, n, dtype=np.int64)
    raise ValueError(kind)


def column(vals, validity, device=True, offset=0, length=None):
    if vals.dtype in (np.int32, np.float32):
        return col32(vals, validity, device, offset=offset, length=length)
    return numeric_column(vals, validity, device, offset=offset, length=length)


def metric(r):
    """the coefficient CorrelationAnalyzer reports for this result's state"""
    state = {"n": int(r.non_null), "sum_x": r.sum_x, "sum_y": r.sum_y, "sum_x2": r.sum_x2, "sum_y2": r.sum_y2,
             "sum_xy": r.sum_xy, "x_ranks": None, "y_ranks": None, "correlation_type": "Spearman"}
    return S.CorrelationAnalyzer("x", "y", "spearman").compute_metric_from_state(state)["value"]


def bits(d):
    return struct.pack("<d", d)


def check(r, want, exact_sums=False, n=None):
    """r: a SPEARMAN result; want: exact_ranks.RankSums of the same pairs"""
    got = (r.sum_x, r.sum_y, r.sum_x2, r.sum_y2, r.sum_xy)
    exp = want.doubles(exact_sums)
    assert int(r.non_null) == want.n, (r.non_null, want.n)
    if n is not None:
        assert r.total == n
    assert [bits(g) for g in got] == [bits(e) for e in exp], (exact_sums, got, exp, want.exact)
    if exact_sums and want.n >= 2:
        lib = metric(r)
        assert lib == R.rho_double(want.n, *exp) or (lib is None and want.n < 2)
        rho = want.rho()
        assert abs(Fraction(lib) - rho) <= Fraction(R.rho_error_bound(want.n, *exp)), (lib, float(rho))


def pair_plan():
    return T.Plan([spec(T.SPEARMAN, 0, column2=1), spec(T.SPEARMAN, 0, column2=1, flags=T.FLAG_EXACT_RANK_SUMS)])


def run_pair(x, y, xv=None, yv=None, cuts=None, device=True):
    n = len(x)
    cuts = cuts or [0, n]
    T.init()
    st = T.State(pair_plan())
    for a, b in zip(cuts[:-1], cuts[1:]):
        st.update([column(x, xv, device, offset=a, length=b - a), column(y, yv, device, offset=a, length=b - a)])
    return st.finalize(), st


def check_pair(res, x, y, xv=None, yv=None, n=None):
    want = R.spearman(x, y, xv, yv)
    check(res[0], want, False, n)
    check(res[1], want, True, n)
    return want


# ---- data ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ky", ["normal", "specials", "i64_small"])
@pytest.mark.parametrize("kx", KINDS)
def test_kinds(kx, ky):
    n = 150_001
    rng = np.random.default_rng([KINDS.index(kx), len(ky)])
    x, y = values(kx, n, rng), values(ky, n, rng)
    xv = orc.pack_validity(rng.random(n) >= 0.1)  # NULLs on x only
    res, _ = run_pair(x, y, xv, None)
    check_pair(res, x, y, xv, None, n)


def test_specials_brute_force_small():
    """a few hundred rows of nothing but special values: the reference's ranks are checked by counting as well"""
    rng = np.random.default_rng(3)
    n = 700
    xb = np.array(SPECIAL_BITS, np.uint64)[rng.integers(0, len(SPECIAL_BITS), n)]
    x = xb.view(np.float64)
    y = values("i64_ends", n, rng)
    want = R.spearman(x, y)
    assert want.rx.tolist() == R.min_ranks_brute([R.total_order_key(int(b)) for b in xb.tolist()])
    res, _ = run_pair(x, y)
    check(res[0], want)
    check(res[1], want, True)


@pytest.mark.parametrize("n", [1, 2, 3, 2047, 2048, 2049, 4097, 262_144, 262_145])
def test_sizes_around_the_pass_edges(n):
    rng = np.random.default_rng(n)
    x, y = values("tie_runs", n, rng), values("nan_payloads", n, rng)
    res, _ = run_pair(x, y)
    check_pair(res, x, y)


@pytest.mark.parametrize("shape", list(SORT_SHAPES))
def test_partition_shapes(shape, monkeypatch):
    for k, v in (SORT_SHAPES[shape] or {}).items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(len(shape))
    n = 60_000
    x, y = values("specials", n, rng), values("i64_above53", n, rng)
    yv = orc.pack_validity(rng.random(n) >= 0.05)
    res, _ = run_pair(x, y, None, yv)
    check_pair(res, x, y, None, yv)


def test_wrapping_and_rho_near_zero_at_five_million_pairs():
    """5 M pairs of two unrelated permutations: the sums of squares and products pass 2^64 (default wraps, the exact
    variant rounds once), and rho ~ 1e-4 is held to the rounding of the five sums; the AnalysisRunner's metric on the
    table is the same double"""
    import pyarrow as pa

    n = 5_000_000
    rng = np.random.default_rng(17)
    x = rng.permutation(n).astype(np.float64)
    y = rng.permutation(n).astype(np.int64)
    res, _ = run_pair(x, y)
    want = check_pair(res, x, y)
    assert want.exact[4] > 2 ** 64 and want.wrapped[4] != want.exact[4]
    assert abs(float(want.rho())) < 1e-2
    ctx = S.AnalysisRunner().add(S.CorrelationAnalyzer("x", "y", "spearman")).run(
        pa.table({"x": pa.array(x), "y": pa.array(y)}))
    got = ctx.get_metric("correlation_spearman_x_y")["value"]
    assert got == R.rho_double(n, *want.doubles())  # (the runner's SPEARMAN spec sums like the reference: wrapped)


def truncated(v):
    """v to a double by dropping the bits below the 53 leading ones (what a conversion that truncates gives)"""
    s = max(0, v.bit_length() - 53)
    return float((v >> s) << s)


def test_exact_sums_round_to_nearest_not_down():
    """x ascending against y descending, n picked so that the exact sums of squares and of products (beyond 2^53) are
    nearer the double above than the one below: the 128-bit sums must round to nearest, not be cut off"""
    def sums(n):
        sq = n * (n + 1) * (2 * n + 1) // 6
        return sq, (n + 1) * n * (n + 1) // 2 - sq  # (sum of i (n + 1 - i))

    n = next(n for n in range(400_000, 500_000) if all(float(v) != truncated(v) for v in sums(n)))
    x = np.arange(n, dtype=np.float64)
    y = np.arange(n, 0, -1, dtype=np.int64)
    res, _ = run_pair(x, y)
    want = check_pair(res, x, y)
    assert (want.exact[2], want.exact[4]) == sums(n)
    assert res[1].sum_x2 != truncated(want.exact[2]) and res[1].sum_xy != truncated(want.exact[4])


# ---- routes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["specials", "i64_ends", "f32_snan"])
def test_lent_first_batch(kind, monkeypatch):
    """a first DEVICE batch without NULLs is ranked from the caller's columns (Float32 never is: it is widened)"""
    monkeypatch.setenv("TGX_SORT_OPTIMISTIC_MIN", "1")
    rng = np.random.default_rng(len(kind))
    n = 300_000
    x, y = values(kind, n, rng), values("tie_runs", n, rng)
    res, st = run_pair(x, y)
    check_pair(res, x, y)
    again = st.finalize()
    check_pair(again, x, y)


@pytest.mark.parametrize("device", [True, False])
def test_several_batches(device, monkeypatch):
    monkeypatch.setenv("TGX_SORT_OPTIMISTIC_MIN", "1")
    rng = np.random.default_rng(int(device))
    n = 400_003
    x, y = values("nan_payloads", n, rng), values("i64_above53", n, rng)
    yv = orc.pack_validity(rng.random(n) >= 0.3)
    res, _ = run_pair(x, y, None, yv, cuts=[0, 200_000, 200_001, 333_333, n], device=device)
    check_pair(res, x, y, None, yv, n)


@pytest.mark.parametrize("coalesce", [True, False])
@pytest.mark.parametrize("device", [True, False])
def test_streams_of_8192_rows(device, coalesce):
    try:
        T.init(flags=0 if coalesce else T.OPT_NO_COALESCE)
        n = 200_003
        rng = np.random.default_rng([device, coalesce])
        x, y = values("f32_snan", n, rng), values("specials", n, rng)
        xv = orc.pack_validity(rng.random(n) >= 0.05)
        st = T.State(pair_plan())
        for a in range(0, n, 8192):
            b = min(n, a + 8192)
            st.update([column(x, xv, device, offset=a, length=b - a), column(y, None, device, offset=a, length=b - a)])
        check_pair(st.finalize(), x, y, xv, None, n)
    finally:
        T.init()


def test_cached_finalize_then_more_then_reset(monkeypatch):
    monkeypatch.setenv("TGX_SORT_OPTIMISTIC_MIN", "1")
    rng = np.random.default_rng(5)
    n, cut = 500_000, 300_000
    x, y = values("two_values", n, rng), values("tie_runs", n, rng)
    T.init()
    st = T.State(pair_plan())
    st.update([column(x, None, offset=0, length=cut), column(y, None, offset=0, length=cut)])
    check_pair(st.finalize(), x[:cut], y[:cut])
    check_pair(st.finalize(), x[:cut], y[:cut])  # (cached)
    st.update([column(x, None, offset=cut, length=n - cut), column(y, None, offset=cut, length=n - cut)])
    check_pair(st.finalize(), x, y, n=n)
    st.reset()
    x2, y2 = values("constant", 1000, rng), values("normal", 1000, rng)
    st.update([column(x2, None), column(y2, None)])
    res = st.finalize()
    check_pair(res, x2, y2)
    assert metric(res[1]) == 0.0  # a constant side


def test_two_pairs_share_the_work_arrays(monkeypatch):
    monkeypatch.setenv("TGX_SORT_OPTIMISTIC_MIN", "1000")
    rng = np.random.default_rng(404)
    n = 400_000
    a, b, c = values("specials", n, rng), values("i64_ends", n, rng), values("nan_payloads", n, rng)
    T.init()
    plan = T.Plan([spec(T.SPEARMAN, 0, column2=1, flags=T.FLAG_EXACT_RANK_SUMS), spec(T.SPEARMAN, 2, column2=0),
                   spec(T.SPEARMAN, 1, column2=2, flags=T.FLAG_EXACT_RANK_SUMS)])
    st = T.State(plan)
    cols = [column(v, None) for v in (a, b, c)]
    st.update(cols)
    for _ in range(2):
        res = st.finalize()
        check(res[0], R.spearman(a, b), True)
        check(res[1], R.spearman(c, a), False)
        check(res[2], R.spearman(b, c), True)


@pytest.mark.parametrize("world", [2, 5])
def test_threaded_ranks(world):
    """row shards over threaded ranks, tgx_allreduce: every rank ends with the ranks over the union"""
    from test_gpu_distributed_sim import _run_ranks

    rng = np.random.default_rng(60 + world)
    n = 300_000
    x, y = values("nan_payloads", n, rng), values("i64_above53", n, rng)
    mask = rng.random(n) >= 0.1
    xv = orc.pack_validity(mask)
    cuts = [n * r // world for r in range(world + 1)]
    cuts[1] = cuts[0]  # (rank 0 holds no rows)
    T.init()
    plan = pair_plan()

    def shards_of(rank):
        a, b = cuts[rank], cuts[rank + 1]
        return [numeric_column(x[a:b], orc.pack_validity(mask[a:b]), True), numeric_column(y[a:b], None, True)]

    want = R.spearman(x, y, xv, None)
    for res, _st in _run_ranks(world, plan, shards_of):
        check(res[0], want, False)
        check(res[1], want, True)
