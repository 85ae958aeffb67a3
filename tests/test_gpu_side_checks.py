"""-m gpu: JOINT_BINS, TEMPORAL and HISTOGRAM in ONE plan with NINE tasks of each kind -- one more than a launch takes, so
every kind's second launch, its slot arithmetic and its share of the counter buffers are in play -- over 20 000 rows
(three workgroups of 8192 rows), 10 % NULLs, one column at Arrow offset 1, DEVICE memory, every batch launched as it
arrives.  The references are tests/exact_histogram.py, exact_joint.py and exact_temporal.py (plain Python, neither the
library nor the oracle); every count is compared for equality, the histogram's two sums are held to
exact_histogram.sum_bounds.  Then reset and the first half alone; then two half-states merged and sent through a blob."""
import math
from fractions import Fraction

import numpy as np
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
