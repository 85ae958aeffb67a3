"""-m gpu: TGX_CHECK_JOINT_BINS, the two scans behind MutualInformationAnalyzer's numeric x numeric branch
(TG/analyzers/advanced/mutual_information.rs:143-248).  The reference is tests/exact_joint.py -- plain Python floats and
integer counts, neither the library nor the oracle -- and EVERY count is compared for equality: the range phase's n,
non-finite rows and extremes, the count phase's (bins + 1)^2 cells and its rows outside [0, bins].  The analyzer's
metric is held to the 50-digit value of the same cells within a bound derived from the number of non-empty cells."""
import json
import math
import os
import threading

import numpy as np
import pytest

import exact_joint as ej
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, to_device

pytestmark = pytest.mark.gpu

TYPE_OF = {np.dtype(np.int64): T.INT64, np.dtype(np.float64): T.FLOAT64, np.dtype(np.int32): T.INT32,
           np.dtype(np.float32): T.FLOAT32, np.dtype(np.int8): T.INT8, np.dtype(np.int16): T.INT16,
           np.dtype(np.uint8): T.UINT8, np.dtype(np.uint16): T.UINT16, np.dtype(np.uint32): T.UINT32}


def column(vals, mask, mem):
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
    """the column as exact_joint takes it: Python ints / floats (a Float32 widens exactly), None for NULL"""
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
    assert (got["n"], got["non_finite"]) == (want["n"], want["non_finite"])
    for k in ("x_min", "x_max", "y_min", "y_max"):
        if want[k] is None:
            assert math.isnan(got[k])
        else:
            assert got[k] == want[k], k


def count_plan(binning, extra=()):
    plan = T.Plan([spec(T.JOINT_BINS, 0, column2=1)] + list(extra))
    plan.set_joint_binning(0, *binning)
    return plan


def two_passes(x, xm, y, ym, bins, mem=T.MEM_DEVICE, cuts=None):
    """both phases on the device against exact_joint; returns (state of the count phase, its plan, the binning)"""
    T.init()
    n = len(x)
    xs, ys = python_values(x, xm), python_values(y, ym)
    cols = [column(x, xm, mem), column(y, ym, mem)]
    bs = batches_of(cols, n, cuts)
    st = feed(T.Plan([spec(T.JOINT_BINS, 0, column2=1)]), bs)
    got = st.joint_range(0)
    want = ej.pair_range(xs, ys)
    assert got["total"] == n
    same_range(got, want)
    res = st.finalize()
    assert (res[0].total, res[0].non_null) == (n, want["n"])
    if want["n"] == 0:
        return None, None, None
    # the widths exactly as mutual_information.rs:219-233 derives them, from the DEVICE's extremes
    binning = (got["x_min"], ej.bin_width(got["x_min"], got["x_max"], bins), got["y_min"],
               ej.bin_width(got["y_min"], got["y_max"], bins), bins)
    assert binning == ej.binning_of(xs, ys, bins)
    plan = count_plan(binning)
    st2 = feed(plan, bs)
    cells, outside = st2.joint_counts(0)
    want_cells, want_outside = ej.joint_counts(xs, ys, binning)
    assert outside == want_outside == 0
    assert cells == ej.dense(want_cells, bins)
    r2 = st2.joint_range(0)
    assert (r2["total"], r2["n"], r2["non_finite"]) == (n, want["n"], want["non_finite"])
    return st2, plan, binning


def masks(rng, n, fx, fy):
    return (None if fx is None else rng.random(n) >= fx), (None if fy is None else rng.random(n) >= fy)


@pytest.mark.parametrize("bins", [2, 5, 10, 127])
@pytest.mark.parametrize("types", ["i64_f64", "f64_f64", "i32_f32", "i16_u8"])
def test_types_and_bins(types, bins):
    rng = np.random.default_rng(bins)
    n = 50_000 + 37
    if types == "i64_f64":
        x, y = rng.integers(-10**6, 10**6, n, dtype=np.int64), rng.standard_normal(n) * 1e3
    elif types == "f64_f64":
        x, y = rng.random(n) * 7.0 - 3.0, np.exp(rng.standard_normal(n) * 3)
    elif types == "i32_f32":
        x, y = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32), rng.standard_normal(n).astype(np.float32)
    else:
        x, y = rng.integers(-2**15, 2**15, n).astype(np.int16), rng.integers(0, 256, n).astype(np.uint8)
    xm, ym = masks(rng, n, 0.05, 0.1)
    two_passes(x, xm, y, ym, bins)


@pytest.mark.parametrize("nulls", ["x", "y", "both", "all_x", "all_both"])
def test_nulls(nulls):
    rng = np.random.default_rng(3)
    n = 20_001
    x, y = rng.integers(0, 1000, n, dtype=np.int64), rng.random(n)
    xm, ym = {"x": (0.3, None), "y": (None, 0.3), "both": (0.3, 0.4), "all_x": (1.1, 0.2), "all_both": (1.1, 1.1)}[nulls]
    xm, ym = masks(rng, n, xm, ym)
    two_passes(x, xm, y, ym, 10)


def test_non_finite_rows_are_counted_apart():
    rng = np.random.default_rng(4)
    n = 30_000
    x, y = rng.standard_normal(n), rng.standard_normal(n).astype(np.float32)
    x[rng.integers(0, n, 200)] = np.nan
    x[rng.integers(0, n, 100)] = np.inf
    y[rng.integers(0, n, 150)] = -np.inf
    y[rng.integers(0, n, 50)] = np.nan
    xm, ym = masks(rng, n, 0.1, 0.1)
    st, _, _ = two_passes(x, xm, y, ym, 10)
    assert st.joint_range(0)["non_finite"] > 300


def test_constant_column_has_width_one():
    n = 10_000
    x, y = np.full(n, 42, np.int64), np.random.default_rng(1).random(n)
    _, _, binning = two_passes(x, None, y, None, 5)
    assert binning[1] == 1.0


def test_int64_beyond_2_53():
    rng = np.random.default_rng(5)
    n = 40_000
    x = rng.integers(2**62 - 2**12, 2**62 + 2**12, n, dtype=np.int64)  # many integers share one double
    y = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    two_passes(x, None, y, None, 10)
    two_passes(x, None, y, None, 127)


@pytest.mark.parametrize("bins", [5, 10, 127])
def test_values_on_cell_borders(bins):
    """mn + k * w and its two neighbouring doubles, for every border, built from the reference's own arithmetic"""
    for mn, mx in ((0.0, 1.0), (-3.7, 12.9), (1e-9, 3e-9), (1.7e9, 1.7e9 + 1000.0), (-1e15, 1e15)):
        w = ej.bin_width(mn, mx, bins)
        vals = [mn, mx]
        for k in range(bins + 1):
            b = mn + k * w
            vals += [b, math.nextafter(b, math.inf), math.nextafter(b, -math.inf)]
        vals = [v for v in vals if mn <= v <= mx]
        x = np.array(vals * 3, np.float64)
        y = np.array(vals[::-1] * 3, np.float64)
        two_passes(x, None, y, None, bins)


@pytest.mark.parametrize("shape", ["sorted_dependent", "shuffled_independent"])
def test_many_workgroups_flush(shape):
    """4 Mi rows and more: many workgroups add their LDS counters to the global ones; on sorted y = 2x every lane of a
    wave meets on one cell"""
    n = (4 << 20) + 12_345
    rng = np.random.default_rng(6)
    if shape == "sorted_dependent":
        x = np.arange(n, dtype=np.int64)
        y = (2 * x).astype(np.float64)
        two_passes(x, None, y, None, 10)
    else:
        x = rng.integers(-10**9, 10**9, n, dtype=np.int64)
        y = rng.standard_normal(n)
        xm, _ = masks(rng, n, 0.02, None)
        two_passes(x, xm, y, None, 127)


@pytest.mark.parametrize("mem", [T.MEM_DEVICE, T.MEM_HOST, T.MEM_HOST_RETAINED])
@pytest.mark.parametrize("cuts", [None, [1, 64, 65, 4097, 70_001, 150_000], 8192])
def test_batching_and_memory_space(mem, cuts):
    rng = np.random.default_rng(8)
    n = 200_000 + 11
    x, y = rng.integers(-500, 500, n, dtype=np.int64), rng.random(n) * 100
    xm, ym = masks(rng, n, 0.05, 0.05)
    two_passes(x, xm, y, ym, 10, mem=mem, cuts=cuts)


def test_narrow_columns_in_small_host_batches():
    rng = np.random.default_rng(9)
    n = 100_000
    x, y = rng.integers(-2**31, 2**31, n).astype(np.int32), rng.standard_normal(n).astype(np.float32)
    xm, ym = masks(rng, n, 0.05, None)
    two_passes(x, xm, y, ym, 10, mem=T.MEM_HOST, cuts=8192)


def test_two_pairs_next_to_stats_and_comoments():
    """two pairs in one plan (one launch, grid.y) beside NUMERIC_STATS and COMOMENTS of the same columns, whose
    results stay what they are without the new checks"""
    T.init()
    rng = np.random.default_rng(10)
    n = 300_000
    a, b, c = rng.integers(0, 10**6, n, dtype=np.int64), rng.standard_normal(n), rng.random(n) * 50
    am, bm = masks(rng, n, 0.05, 0.1)
    cols = [column(a, am, T.MEM_DEVICE), column(b, bm, T.MEM_DEVICE), column(c, None, T.MEM_DEVICE)]
    pa, pb, pc = python_values(a, am), python_values(b, bm), python_values(c, None)
    others = [spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE), spec(T.NUMERIC_STATS, 1), spec(T.COMOMENTS, 0, column2=1),
              spec(T.COMOMENTS, 2, column2=1)]
    alone = feed(T.Plan(others), [cols]).finalize()
    b1, b2 = ej.binning_of(pa, pb, 10), ej.binning_of(pc, pb, 127)
    plan = T.Plan([spec(T.JOINT_BINS, 0, column2=1), spec(T.JOINT_BINS, 2, column2=1), spec(T.JOINT_BINS, 2, column2=1)]
                  + others)
    plan.set_joint_binning(0, *b1)
    plan.set_joint_binning(1, *b2)   # (spec 2 stays in its range phase)
    st = feed(plan, batches_of(cols, n, [100_000, 100_064]))
    res = st.finalize()
    assert st.joint_counts(0) == (ej.dense(ej.joint_counts(pa, pb, b1)[0], 10), 0)
    assert st.joint_counts(1) == (ej.dense(ej.joint_counts(pc, pb, b2)[0], 127), 0)
    same_range(st.joint_range(2), ej.pair_range(pc, pb))
    ints = ("total", "non_null", "min_i", "max_i", "sum_i", "min_f", "max_f")
    for got, want in zip(res[3:5], alone[0:2]):
        assert [getattr(got, k) for k in ints] == [getattr(want, k) for k in ints]
    for got, want in zip(res[5:7], alone[2:4]):
        assert (got.total, got.non_null) == (want.total, want.non_null)
        assert abs(got.co_c_xy - want.co_c_xy) <= 1e-9 * abs(want.co_c_xy)


def test_rows_outside_the_binning_are_counted_not_binned():
    """a table that changed between the passes: rows beyond the edges land in no cell"""
    T.init()
    x = np.array([0.0, 1.0, 2.0, 10.0, 10.5, 11.0, -0.5, 5.0], np.float64)
    y = np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 60.0], np.float64)
    binning = (0.0, 2.0, 0.0, 2.0, 5)  # covers [0, 12) on both sides
    st = feed(count_plan(binning), [[column(x, None, T.MEM_DEVICE), column(y, None, T.MEM_DEVICE)]])
    cells, outside = st.joint_counts(0)
    want, want_outside = ej.joint_counts(x.tolist(), y.tolist(), binning)
    assert (cells, outside) == (ej.dense(want, 5), want_outside) and outside == 2


def test_reset_merge_serialize():
    T.init()
    rng = np.random.default_rng(11)
    n = 90_000
    x, y = rng.integers(-1000, 1000, n, dtype=np.int64), rng.standard_normal(n)
    xm, ym = masks(rng, n, 0.1, 0.1)
    xs, ys = python_values(x, xm), python_values(y, ym)
    cols = [column(x, xm, T.MEM_DEVICE), column(y, ym, T.MEM_DEVICE)]
    parts = batches_of(cols, n, [30_000, 60_000])
    binning = ej.binning_of(xs, ys, 10)
    want = (ej.dense(ej.joint_counts(xs, ys, binning)[0], 10), 0)
    # range phase: three states merged, then through a blob
    rplan = T.Plan([spec(T.JOINT_BINS, 0, column2=1)])
    states = [feed(rplan, [p]) for p in parts]
    states[0].merge(states[1:])
    same_range(states[0].joint_range(0), ej.pair_range(xs, ys))
    back = T.State.deserialize(rplan, states[0].serialize())
    same_range(back.joint_range(0), ej.pair_range(xs, ys))
    assert back.joint_range(0)["total"] == n
    # count phase: the same
    plan = count_plan(binning)
    states = [feed(plan, [p]) for p in parts]
    states[0].merge(states[1:])
    assert states[0].joint_counts(0) == want
    blob = states[0].serialize()
    back = T.State.deserialize(plan, blob)
    assert back.joint_counts(0) == want and back.serialize() == blob
    # a blob counted under another binning is refused
    other = count_plan(binning[:4] + (5,))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(other, blob)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(rplan, blob)
    # reset and reuse: the first part alone, after the whole table
    st = states[0]
    st.reset()
    assert st.joint_counts(0) == ([0] * 121, 0)
    st.update(parts[0])
    first = 30_000
    assert st.joint_counts(0) == (ej.dense(ej.joint_counts(xs[:first], ys[:first], binning)[0], 10), 0)
    assert st.finalize()[0].total == first


def test_unsupported_columns_and_phases():
    T.init()
    n = 1000
    f = column(np.arange(n, dtype=np.float64), None, T.MEM_HOST)
    u64 = T.Column.narrow(T.UINT64, np.arange(n, dtype=np.uint64))
    boolean = T.Column.boolean(np.zeros(n // 8 + 8, np.uint8), n)
    offs, data, sval = orc.utf8_from_list(["a%d" % i for i in range(n)])
    text = T.Column.utf8(offs, np.concatenate([data, np.zeros(64, np.uint8)]))
    plan = T.Plan([spec(T.JOINT_BINS, 0, column2=1)])
    for bad in (u64, boolean, text):
        for cols in ([f, bad], [bad, f]):
            with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED"):
                T.State(plan).update(cols)
    st = feed(plan, [[f, f]])
    with pytest.raises(T.TgxError, match="range phase"):
        st.joint_counts(0)


@pytest.mark.parametrize("world,device_buffers", [(2, True), (5, False)])
def test_threaded_ranks(world, device_buffers):
    """the way _run_ranks of tests/test_gpu_distributed_sim.py drives them: every rank a thread with its own state and
    row shard, tgx_allreduce over the thread-barrier transport; every rank ends with the table's counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    T.init()
    rng = np.random.default_rng(12 + world)
    n = 250_000 + 3
    x, y = rng.integers(0, 10**5, n, dtype=np.int64), rng.standard_normal(n)
    xm, ym = masks(rng, n, 0.05, 0.02)
    xs, ys = python_values(x, xm), python_values(y, ym)
    whole = [column(x, xm, T.MEM_DEVICE), column(y, ym, T.MEM_DEVICE)]
    binning = ej.binning_of(xs, ys, 10)
    want_cells = ej.dense(ej.joint_counts(xs, ys, binning)[0], 10)
    plan = T.Plan([spec(T.JOINT_BINS, 0, column2=1), spec(T.JOINT_BINS, 0, column2=1), spec(T.COUNT, 0)])
    plan.set_joint_binning(1, *binning)
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
            results[rank] = (res, st.joint_range(0), st.joint_counts(1))
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
    want = ej.pair_range(xs, ys)
    for res, rng_got, counts in results:
        assert (res[0].total, res[0].non_null, res[1].non_null) == (n, want["n"], want["n"])
        same_range(rng_got, want)
        assert counts == (want_cells, 0)


# ---- MutualInformationAnalyzer through AnalysisRunner.run ---------------------------------------------------------
def metric_bound(cells, n):
    """|computed - exact| for sum p_xy ln(p_xy / (p_x p_y)) / LN_2 in doubles, from the cells themselves: per term two
    divisions by n for the marginals and one for p_xy, a product, a division, ln (within 1 ulp), a product -- 7
    roundings, each at most 2^-53 relative on a term (the roundings inside ln's argument move the term by the same
    relative amount times p_xy <= |term| only when |ln| >= 1, so they are charged against max(|term|, p_xy)); the
    running sum rounds once per term on a partial sum no larger than the sum of magnitudes; LN_2 and the last division
    one each."""
    import mpmath

    exact, magnitude, used = ej.mutual_information(cells, n)
    xc, yc = ej.marginals(cells)
    charged = mpmath.mpf(0)
    for (i, j), c in cells.items():
        p = mpmath.mpf(c) / n
        charged += max(abs(p * mpmath.log(p / (mpmath.mpf(xc[i]) / n * mpmath.mpf(yc[j]) / n))), p)
    u = 2.0 ** -53
    return float(exact), float((7 * charged + used * magnitude + 2 * magnitude) * u / mpmath.log(2)) + 2 * u * abs(float(exact))


def labelled(cells):
    return sorted(("%d.0" % i, "%d.0" % j, c) for (i, j), c in cells.items())


def check_analyzer_state(ctx, key, xs, ys, bins):
    binning = ej.binning_of(xs, ys, bins)
    cells, outside = ej.joint_counts(xs, ys, binning)
    assert outside == 0
    state = ctx.states[key]
    assert state["n"] == sum(cells.values()) and state["bins"] == bins
    assert sorted(map(tuple, state["joint_counts"])) == labelled(cells)
    xc, yc = ej.marginals(cells)
    assert state["x_counts"] == {"%d.0" % i: c for i, c in xc.items()}
    assert state["y_counts"] == {"%d.0" % j: c for j, c in yc.items()}
    exact, bound = metric_bound(cells, state["n"])
    got = ctx.get_metric(key)
    assert got["type"] == "Double"
    print("%s: metric %.17g, exact %.17g, |diff| %.3g, bound %.3g" % (key, got["value"], exact, abs(got["value"] - exact), bound))
    assert abs(got["value"] - exact) <= bound
    return got["value"]


def test_analyzer_on_the_reference_tables():
    pa = pytest.importorskip("pyarrow")
    import term_amd.suite as S

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mutual_information_vectors.json")) as f:
        golden = json.load(f)
    xs = [float(i) for i in range(100)]
    for name, ys in (("independent", [float((37 * i + 13) % 100) for i in range(100)]),
                     ("dependent", [2.0 * i for i in range(100)])):
        g = golden[name]
        tbl = pa.table({"x": pa.array(xs, pa.float64()), "y": pa.array(ys, pa.float64())})
        ctx = S.AnalysisRunner().add(S.MutualInformationAnalyzer("x", "y", g["bins"])).run(tbl)
        assert not ctx.has_errors(), ctx.errors()
        value = check_analyzer_state(ctx, "mutual_information_x_y", xs, ys, g["bins"])
        assert len(ctx.states["mutual_information_x_y"]["joint_counts"]) == g["non_empty_cells"]
        assert abs(value - float(g["metric"])) < 1e-13
        assert value < g["metric_below"] if name == "independent" else value > g["metric_above"]


def test_analyzer_on_a_300_000_row_table_next_to_others():
    pa = pytest.importorskip("pyarrow")
    import term_amd.suite as S

    rng = np.random.default_rng(21)
    n = 300_000
    a = rng.integers(0, 5000, n, dtype=np.int64)
    b = a * 0.25 + rng.standard_normal(n) * 300.0
    c = rng.standard_normal(n).astype(np.float32)
    am, bm = rng.random(n) >= 0.03, rng.random(n) >= 0.05
    tbl = pa.table({"a": pa.array(a, pa.int64(), mask=~am), "b": pa.array(b, pa.float64(), mask=~bm),
                    "c": pa.array(c, pa.float32()), "s": pa.array(["k%d" % (i % 7) for i in range(n)], pa.string())})
    tbl = pa.Table.from_batches(tbl.to_batches(max_chunksize=50_000))
    runner = (S.AnalysisRunner().add(S.SizeAnalyzer()).add(S.MutualInformationAnalyzer("a", "b"))
              .add(S.MutualInformationAnalyzer("c", "b", 127)).add(S.CorrelationAnalyzer("a", "b"))
              .add(S.MutualInformationAnalyzer("a", "s", 5)).add(S.MeanAnalyzer("b")))
    ctx = runner.run(tbl)
    pa_, pb, pc = python_values(a, am), python_values(b, bm), python_values(c, None)
    check_analyzer_state(ctx, "mutual_information_a_b", pa_, pb, 10)
    check_analyzer_state(ctx, "mutual_information_c_b", pc, pb, 127)
    # the string pair is the analyzer's own error; the others ran
    assert [e["analyzer_name"] for e in ctx.errors()] == ["mutual_information"]
    assert "TGX_UNSUPPORTED" in ctx.errors()[0]["error"]
    assert ctx.get_metric("size")["value"] == n and ctx.get_metric("mean.b") is not None
    alone = S.AnalysisRunner().add(S.CorrelationAnalyzer("a", "b")).add(S.MeanAnalyzer("b")).run(tbl)
    assert ctx.get_metric("correlation_pearson_a_b") == alone.get_metric("correlation_pearson_a_b")
    assert ctx.get_metric("mean.b") == alone.get_metric("mean.b")


def test_analyzer_without_rows_and_with_too_many_bins():
    pa = pytest.importorskip("pyarrow")
    import term_amd.suite as S

    tbl = pa.table({"x": pa.array([None, 1.0, None], pa.float64()), "y": pa.array([2.0, None, None], pa.float64())})
    ctx = S.AnalysisRunner().add(S.MutualInformationAnalyzer("x", "y", 5)).run(tbl)
    assert not ctx.has_errors(), ctx.errors()
    assert ctx.get_metric("mutual_information_x_y") == {"type": "Double", "value": 0.0}
    assert ctx.states["mutual_information_x_y"] == {"n": 0, "joint_counts": [], "x_counts": {}, "y_counts": {}, "bins": 5}
    tbl = pa.table({"x": pa.array([1.0, 2.0], pa.float64()), "y": pa.array([2.0, 3.0], pa.float64())})
    ctx = S.AnalysisRunner().add(S.MutualInformationAnalyzer("x", "y", 128)).add(S.SizeAnalyzer()).run(tbl)
    assert "at most 127" in ctx.errors()[0]["error"] and ctx.get_metric("size")["value"] == 2
    big = pa.table({"x": pa.array([-1.7e308, 1.7e308], pa.float64()), "y": pa.array([2.0, 3.0], pa.float64())})
    ctx = S.AnalysisRunner().add(S.MutualInformationAnalyzer("x", "y", 5)).run(big)
    assert "overflows" in ctx.errors()[0]["error"]
