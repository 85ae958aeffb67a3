"""-m gpu: JOINT_BINS, TEMPORAL and HISTOGRAM in ONE plan with NINE tasks of each kind -- one more than a launch takes, so
every kind's second launch, its slot arithmetic and its share of the counter buffers are in play -- over 20 000 rows
(three workgroups of 8192 rows), 10 % NULLs, one column at Arrow offset 1, DEVICE memory, every batch launched as it
arrives.  The references are tests/exact_histogram.py, exact_joint.py and exact_temporal.py (plain Python, neither the
library nor the oracle); every count is compared for equality, the histogram's two sums are held to
exact_histogram.sum_bounds.  Then reset and the first half alone; then two half-states merged and sent through a blob.

Below that, all six kinds of side_check.h in one plan, held against plans of one kind each; and the refusals of a
column that two kinds read, with their texts."""
import math
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

import exact_histogram as eh
import exact_joint as ej
import exact_temporal as et
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, to_device

pytestmark = pytest.mark.gpu

N = 20_000
HALF = N // 2
MS_DAY = 86400 * 1000
TOD = {"ticks_per_second": 1000, "tod_lo": 9 * 3600 * 1000, "tod_hi": 17 * 3600 * 1000}


def table():
    """column 0: Float64 with a few NaNs and infinities; columns 1, 2: Int64 instants in ms, 2 mostly a little after 1"""
    rng = np.random.default_rng(2025)
    x = rng.standard_normal(N) * 100.0
    x[::997] = np.nan
    x[5::1999] = np.inf
    a = rng.integers(-60 * 365 * MS_DAY, 60 * 365 * MS_DAY, N, dtype=np.int64)
    b = a + rng.integers(-3000, 30000, N, dtype=np.int64)
    return [x, a, b], [rng.random(N) >= 0.1 for _ in range(3)]


def device_column(vals, mask, offset):
    """the column in DEVICE memory at Arrow offset `offset`: that many rows of other data (and set validity bits) lead
    the buffers"""
    type_id = T.FLOAT64 if vals.dtype == np.float64 else T.INT64
    vals = np.concatenate([np.full(offset, 77, vals.dtype), vals])
    validity = pad_validity(orc.pack_validity(np.concatenate([np.ones(offset, bool), mask])))
    col = T.Column(type_id, len(vals), values=to_device(vals), validity=to_device(validity), mem=T.MEM_DEVICE)
    return col.sliced(offset, len(vals) - offset)


class Tasks:
    """the 27 specs, the three kinds interleaved, and what each answers over rows [lo, hi) of the table"""

    def __init__(self):
        vals, masks = table()
        self.cols = [[v if ok else None for v, ok in zip(vs.tolist(), m.tolist())] for vs, m in zip(vals, masks)]
        self.raw = [v.tolist() for v in vals]
        self.masks = [m.tolist() for m in masks]
        self.device = [device_column(v, m, 1 if c == 1 else 0) for c, (v, m) in enumerate(zip(vals, masks))]
        full = [eh.value_range(c) for c in self.cols[:2]]
        hist, joint, temporal = [], [], []
        # HISTOGRAM: 5 in the count phase with 10 buckets (two of them under edges that leave rows to ELSE), 4 ranged
        for i, c in enumerate((0, 1, 0, 1, 0)):
            shrink = (1.0, 1.0, 0.5, 0.25, 0.125)[i]
            hist.append(("hist", c, eh.edges_of(full[c]["min"] * shrink, full[c]["max"] * shrink, 10)))
        hist += [("hist", c, None) for c in (0, 1, 0, 1)]
        # JOINT_BINS: 5 binned with 10 bins (the last under half the x width: rows outside), 4 ranged
        for i, (cx, cy) in enumerate(((0, 1), (1, 2), (0, 2), (2, 1), (1, 0))):
            x0, xw, y0, yw, bins = ej.binning_of(self.cols[cx], self.cols[cy], 10)
            joint.append(("joint", cx, cy, (x0, xw / 2 if i == 4 else xw, y0, yw, bins)))
        joint += [("joint", cx, cy, None) for cx, cy in ((0, 1), (1, 2), (0, 2), (2, 0))]
        # TEMPORAL: the three modes, three times
        temporal = [("temporal", 1, 2, et.ORDER, {"delta": 0}),
                    ("temporal", 1, 2, et.ORDER, {"delta": 10000, "flags": et.KEEP_NULLS}),
                    ("temporal", 2, 1, et.ORDER, {"delta": -3000}),
                    ("temporal", 1, -1, et.TIME_OF_DAY, dict(TOD)),
                    ("temporal", 1, -1, et.TIME_OF_DAY, dict(TOD, flags=et.WEEKDAYS_ONLY)),
                    ("temporal", 2, -1, et.TIME_OF_DAY, dict(TOD, flags=et.KEEP_NULLS)),
                    ("temporal", 1, -1, et.RANGE, {"lo": -20 * 365 * MS_DAY, "hi": 20 * 365 * MS_DAY}),
                    ("temporal", 2, -1, et.RANGE, {"lo": 0, "flags": et.KEEP_NULLS}),
                    ("temporal", 1, -1, et.RANGE, {"hi": -1})]
        self.tasks = [t for triple in zip(hist, joint, temporal) for t in triple]
        assert len(self.tasks) == 27
        self.wants = {}

    def plan(self):
        specs = []
        for t in self.tasks:
            if t[0] == "hist":
                specs.append(spec(T.HISTOGRAM, t[1]))
            elif t[0] == "joint":
                specs.append(spec(T.JOINT_BINS, t[1], column2=t[2]))
            else:
                specs.append(spec(T.TEMPORAL, t[1], column2=t[2]))
        plan = T.Plan(specs)
        for i, t in enumerate(self.tasks):
            if t[0] == "hist" and t[2]:
                plan.set_histogram_edges(i, t[2])
            elif t[0] == "joint" and t[3]:
                plan.set_joint_binning(i, *t[3])
            elif t[0] == "temporal":
                p = t[4]
                plan.set_temporal(i, t[3], flags=p.get("flags", 0), delta=p.get("delta", 0),
                                  ticks_per_second=p.get("ticks_per_second", 0), tod_lo=p.get("tod_lo", 0),
                                  tod_hi=p.get("tod_hi", 0), lo=p.get("lo", et.I64_MIN), hi=p.get("hi", et.I64_MAX))
        return plan

    def batch(self, lo, hi):
        return [c.sliced(lo, hi - lo) for c in self.device]

    def want(self, lo, hi):
        """per spec what the exact references give over rows [lo, hi): computed once per range"""
        if (lo, hi) not in self.wants:
            out = []
            for t in self.tasks:
                if t[0] == "hist":
                    xs = self.cols[t[1]][lo:hi]
                    out.append(eh.counts_of(xs, t[2]) if t[2] else eh.value_range(xs))
                elif t[0] == "joint":
                    xs, ys = self.cols[t[1]][lo:hi], self.cols[t[2]][lo:hi]
                    out.append(ej.joint_counts(xs, ys, t[3]) + (ej.pair_range(xs, ys),) if t[3] else ej.pair_range(xs, ys))
                else:
                    pair = t[3] == et.ORDER
                    out.append(et.counts(t[3], t[4], self.raw[t[1]][lo:hi], self.raw[t[2]][lo:hi] if pair else None,
                                         self.masks[t[1]][lo:hi], self.masks[t[2]][lo:hi] if pair else None))
            self.wants[(lo, hi)] = out
        return self.wants[(lo, hi)]

    def check(self, st, lo, hi):
        rows = hi - lo
        totals = [(r.total, r.non_null, r.matches) for r in st.finalize()]
        for i, (t, want) in enumerate(zip(self.tasks, self.want(lo, hi))):
            if t[0] == "hist" and t[2]:
                counts, else_rows, non_finite = want
                assert st.histogram_counts(i) == want, i
                r = st.histogram_range(i)
                assert (r["total"], r["n"], r["non_finite"]) == (rows, sum(counts), non_finite), i
                assert totals[i] == (rows, sum(counts) + non_finite, 0), i
            elif t[0] == "hist":
                got = st.histogram_range(i)
                assert [got[k] for k in ("total", "nulls", "non_finite", "n", "min", "max")] == \
                    [want[k] for k in ("total", "nulls", "non_finite", "n", "min", "max")], i
                for k, bound in zip(("sum", "sum_squared"), eh.sum_bounds(want)):
                    diff = abs(Fraction(got[k]) - want[k])
                    print("spec %d %s: got %.17g, |diff| %.3g, bound %.3g" % (i, k, got[k], float(diff), float(bound)))
                    assert diff <= bound, (i, k)
                assert totals[i] == (rows, want["n"] + want["non_finite"], 0), i
            elif t[0] == "joint" and t[3]:
                cells, outside, rng = want
                assert st.joint_counts(i) == (ej.dense(cells, t[3][4]), outside), i
                r = st.joint_range(i)
                assert (r["total"], r["n"], r["non_finite"]) == (rows, rng["n"] - outside, rng["non_finite"]), i
                assert math.isnan(r["x_min"]) and totals[i] == (rows, rng["n"] - outside, 0), i
            elif t[0] == "joint":
                got = st.joint_range(i)
                assert got == dict(want, total=rows), i
                assert totals[i] == (rows, want["n"], 0), i
            else:
                seen, considered, violations = want
                assert st.temporal_counts(i) == want, i
                assert totals[i] == (seen, considered, considered - violations) and seen == rows, i


@pytest.fixture(scope="module")
def tasks():
    T.init(flags=T.OPT_NO_COALESCE)  # (the 20 000 rows reach the kernels as one batch, at the offset they were given)
    try:
        yield Tasks()
    finally:
        T.init(flags=0)


def test_nine_tasks_of_each_kind_against_the_exact_references(tasks):
    plan = tasks.plan()
    st = T.State(plan)
    st.update(tasks.batch(0, N))
    tasks.check(st, 0, N)
    # the expectations are worth something: rows on every side of every predicate
    wants = tasks.want(0, N)
    assert any(t[0] == "hist" and t[2] and w[1] > 0 for t, w in zip(tasks.tasks, wants))       # ELSE rows
    assert any(t[0] == "joint" and t[3] and w[1] > 0 for t, w in zip(tasks.tasks, wants))      # rows outside
    assert all(0 < w[2] < w[1] for t, w in zip(tasks.tasks, wants) if t[0] == "temporal")      # passes and violations
    # reset, then the first half alone
    st.reset()
    st.update(tasks.batch(0, HALF))
    tasks.check(st, 0, HALF)
    # two half-states merged, and the merged state through a blob
    other = T.State(plan)
    other.update(tasks.batch(HALF, N))
    tasks.check(other, HALF, N)
    st.merge([other])
    tasks.check(st, 0, N)
    blob = st.serialize()
    back = T.State.deserialize(plan, blob)
    tasks.check(back, 0, N)
    assert back.serialize() == blob


# ---- all six kinds of the skeleton in one plan ---------------------------------------------------------------------------
ROWS, FIRST = 1000, 600


class SixKinds:
    """1 000 rows in HOST memory and two specs of each of the six kinds, the kinds interleaved; each kind's two tasks differ
    in their parameters, so a task that reads its neighbour's counters, range slot or table answers wrongly (no table
    overflows: which keys an overflowing table keeps is decided by the order in which the lanes arrive).  The shapes
    are small because what is held here is host plumbing (word offsets, slot binding, the order of the blob's sections,
    the per-column flags); the kernels have their own tests on large shapes."""

    def __init__(self):
        rng = np.random.default_rng(46)
        x = rng.standard_normal(ROWS) * 50.0
        x[17], x[701] = np.nan, np.inf
        a = rng.integers(-30 * 365 * MS_DAY, 30 * 365 * MS_DAY, ROWS, dtype=np.int64)
        b = a + rng.integers(-3000, 30000, ROWS, dtype=np.int64)
        k = rng.integers(0, 20, ROWS, dtype=np.int64) * 3 - 7
        words = ["w%02d" % i + "x" * (i % 5) for i in range(20)]
        s = [words[i] for i in rng.integers(0, 20, ROWS)]
        self.x = [v if ok else None for v, ok in zip(x.tolist(), (rng.random(ROWS) >= 0.1).tolist())]
        arrays = [pa.array(self.x, pa.float64()), pa.array(a), pa.array(b), pa.array(k), pa.array(s, pa.string())]
        self.columns = []
        for arr in arrays:
            col = T.Column.from_arrow(arr)
            col.c.mem = T.MEM_HOST
            self.columns.append(col)
        self.edges = eh.edges_of(-100.0, 100.0, 6)
        # (kind, column, column2, how the plan is told the task's parameters)
        self.tasks = [
            (T.JOINT_BINS, 0, 1, lambda p, i: p.set_joint_binning(i, -150.0, 30.0, float(a.min()), 2e11, 10)),
            (T.TEMPORAL, 1, 2, lambda p, i: p.set_temporal(i, et.ORDER, delta=0)),
            (T.HISTOGRAM, 0, -1, lambda p, i: p.set_histogram_edges(i, self.edges)),
            (T.VALUE_RULE, 0, -1, lambda p, i: p.set_value_rule(i, T.RULE_GE_ZERO)),
            (T.VALUE_COUNTS, 3, -1, lambda p, i: p.set_value_counts(i, max_distinct=100, max_value_bytes=8)),
            (T.PAIR_COUNTS, 4, 3, lambda p, i: p.set_pair_counts(i, x="value", y=(-7.0, 6.0, 10), max_pairs=1000)),
            (T.JOINT_BINS, 2, 1, lambda p, i: None),  # stays in its range phase
            (T.TEMPORAL, 2, -1, lambda p, i: p.set_temporal(i, et.RANGE, flags=et.KEEP_NULLS, lo=0)),
            (T.HISTOGRAM, 0, -1, lambda p, i: None),  # stays in its range phase
            (T.VALUE_RULE, 3, -1, lambda p, i: p.set_value_rule(i, T.RULE_BETWEEN, lo_i=-1, hi_i=20)),
            (T.VALUE_COUNTS, 4, -1, lambda p, i: p.set_value_counts(i, max_distinct=16, max_value_bytes=5)),
            (T.PAIR_COUNTS, 3, 4, lambda p, i: p.set_pair_counts(i, x=(-7.0, 20.0, 3), y="value", max_pairs=64,
                                                                 max_value_bytes=5)),
        ]
        self.exact = {}

    def batch(self, lo, hi):
        return [c.sliced(lo, hi - lo) for c in self.columns]

    def plan(self, which):
        plan = T.Plan([spec(self.tasks[t][0], self.tasks[t][1], column2=self.tasks[t][2]) for t in which])
        for i, t in enumerate(which):
            self.tasks[t][3](plan, i)
        return plan

    def read(self, st, which, lo, hi):
        """per task of `which`: everything its kind's getters give (NaNs as text: they compare unequal to themselves);
        a ranged histogram's two sums are held to the exact sums' bounds here and left out"""
        results = st.finalize()
        out = {}
        for i, t in enumerate(which):
            kind, r = self.tasks[t][0], results[i]
            got = [(r.kind, r.total, r.non_null, r.distinct, r.matches)]
            if kind == T.JOINT_BINS:
                got += [st.joint_range(i), st.joint_counts(i) if t == 0 else None]
            elif kind == T.TEMPORAL:
                got.append(st.temporal_counts(i))
            elif kind == T.HISTOGRAM:
                rng = st.histogram_range(i)
                sums = [rng.pop("sum"), rng.pop("sum_squared")]
                if t == 8:
                    if (lo, hi) not in self.exact:
                        self.exact[(lo, hi)] = eh.value_range(self.x[lo:hi])
                    want = self.exact[(lo, hi)]
                    for name, have, bound in zip(("sum", "sum_squared"), sums, eh.sum_bounds(want)):
                        diff = abs(Fraction(have) - want[name])
                        print("rows [%d, %d) %s: got %.17g, |diff| %.3g, bound %.3g" % (lo, hi, name, have, float(diff),
                                                                                       float(bound)))
                        assert diff <= bound, (lo, hi, name)
                got += [rng, st.histogram_counts(i) if t == 2 else None]
            elif kind == T.VALUE_RULE:
                got.append(st.value_rule_counts(i))
            elif kind == T.VALUE_COUNTS:
                summary, counts = st.value_counts(i)
                got += [summary, list(counts.items())]
            else:
                summary, counts = st.pair_counts(i)
                got += [summary, list(counts.items())]
            out[t] = repr(got)
        return out

    def walk(self, which):
        """the four ways a state comes to its answer, each read through `read`: both batches; reset and the first batch
        alone; two states of one batch each, merged; that state through a blob (which must serialize to itself)"""
        plan = self.plan(which)
        st = T.State(plan)
        st.update(self.batch(0, FIRST))
        st.update(self.batch(FIRST, ROWS))
        out = {"both": self.read(st, which, 0, ROWS)}
        st.reset()
        st.update(self.batch(0, FIRST))
        out["first"] = self.read(st, which, 0, FIRST)
        other = T.State(plan)
        other.update(self.batch(FIRST, ROWS))
        out["second"] = self.read(other, which, FIRST, ROWS)
        st.merge([other])
        out["merged"] = self.read(st, which, 0, ROWS)
        blob = st.serialize()
        back = T.State.deserialize(plan, blob)
        out["blob"] = self.read(back, which, 0, ROWS)
        assert back.serialize() == blob
        return out


def test_six_kinds_in_one_plan_answer_as_each_kind_alone():
    T.init()
    six = SixKinds()
    together = six.walk(list(range(12)))
    assert together["both"] == together["merged"] == together["blob"]
    assert together["both"] != together["first"]
    for first in range(6):  # the two tasks of one kind, alone in a plan
        alone = six.walk([first, first + 6])
        for step, answers in alone.items():
            for t, answer in answers.items():
                assert together[step][t] == answer, (step, t)
    # the comparison is worth something: the two tasks of a kind answer differently
    assert all(together["both"][t] != together["both"][t + 6] for t in range(6))


# ---- refusals where two kinds read one column ----------------------------------------------------------------------------
def host_column(values, type):
    col = T.Column.from_arrow(pa.array(values, type))
    col.c.mem = T.MEM_HOST
    return col


WORDS8 = ["a", "b", "c", "a", "b", "a", "d", "a"]
FLOATS8 = [0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 7.5]
INTS8 = list(range(8))


def refused(plan, batch, text):
    st = T.State(plan)
    with pytest.raises(T.TgxError) as e:
        st.update(batch)
    assert e.value.status == "TGX_UNSUPPORTED" and str(e.value) == "TGX_UNSUPPORTED: " + text
    return st  # (the refused batch went to the very state that is read afterwards)


def test_a_string_column_under_joint_bins_and_histogram_is_refused_by_joint_bins():
    T.init()
    plan = T.Plan([spec(T.JOINT_BINS, 0, column2=1), spec(T.HISTOGRAM, 0)])
    st = refused(plan, [host_column(WORDS8, pa.string()), host_column(FLOATS8, pa.float64())],
                 "column 0: JOINT_BINS takes numeric columns (type 3)")
    st.update([host_column(FLOATS8, pa.float64()), host_column(FLOATS8, pa.float64())])
    assert st.joint_range(0)["n"] == 8 and st.histogram_range(1)["n"] == 8


def test_a_string_column_under_histogram_and_temporal_is_refused_by_temporal():
    T.init()
    plan = T.Plan([spec(T.HISTOGRAM, 0), spec(T.TEMPORAL, 0, column2=-1)])
    plan.set_temporal(1, et.RANGE, lo=2)
    # (the kinds are asked in the order of their registration, TEMPORAL before HISTOGRAM; before there was one, HISTOGRAM
    # was asked first and this read "column 0: HISTOGRAM takes numeric columns (type 3)")
    st = refused(plan, [host_column(WORDS8, pa.string())], "column 0: TEMPORAL takes Int64-shaped columns (type 3)")
    st.update([host_column(INTS8, pa.int64())])
    assert st.histogram_range(0)["n"] == 8
    assert st.temporal_counts(1) == et.counts(et.RANGE, {"lo": 2}, INTS8, None, [True] * 8, None) == (8, 8, 2)


def test_a_float_column_under_value_counts_and_a_binned_pair_side_is_refused_by_value_counts():
    T.init()
    plan = T.Plan([spec(T.VALUE_COUNTS, 0), spec(T.PAIR_COUNTS, 0, column2=1)])
    plan.set_value_counts(0)
    plan.set_pair_counts(1, x=(0.0, 2.0, 4), y="value")
    st = refused(plan, [host_column(FLOATS8, pa.float64()), host_column(WORDS8, pa.string())],
                 "column 0: VALUE_COUNTS takes integer and string columns, not Float64 (type 2)")
    st.update([host_column(INTS8, pa.int64()), host_column(WORDS8, pa.string())])
    assert st.value_counts(0)[1] == {v: 1 for v in range(8)}
    assert st.pair_counts(1)[1] == {(0, b"a"): 1, (0, b"b"): 1, (1, b"c"): 1, (1, b"a"): 1, (2, b"b"): 1, (2, b"a"): 1,
                                    (3, b"d"): 1, (3, b"a"): 1}
