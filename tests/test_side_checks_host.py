"""JOINT_BINS, TEMPORAL and HISTOGRAM in ONE plan without a device: the three sections of a blob behind each other, in
both phases of the two phased kinds -- what a host-only state answers from it, that it writes the same bytes back, that
every proper prefix is refused, and that a merge adds every counter of every kind."""
import math

import pytest

import term_amd as T
from _lib_spec import spec
from term_amd import wire

BINNING = (0.0, 0.5, -1.0, 2.0, 2)  # x_origin, x_width, y_origin, y_width, bins: 9 cells
EDGES = [0.0, 1.0, 2.0, 4.0, 3.5]
TOD = dict(ticks_per_second=1000, tod_lo=9 * 3600 * 1000, tod_hi=17 * 3600 * 1000)
I64_MAX = (1 << 63) - 1


def plan_of_all_three():
    plan = T.Plan([spec(T.JOINT_BINS, 0, column2=1), spec(T.JOINT_BINS, 0, column2=1),
                   spec(T.TEMPORAL, 2, column2=3), spec(T.TEMPORAL, 2), spec(T.TEMPORAL, 3),
                   spec(T.HISTOGRAM, 0), spec(T.HISTOGRAM, 1), spec(T.COUNT, 0)])
    plan.set_joint_binning(1, *BINNING)
    plan.set_temporal(2, T.TEMPORAL_ORDER, flags=T.TEMPORAL_KEEP_NULLS, delta=5)
    plan.set_temporal(3, T.TEMPORAL_TIME_OF_DAY, flags=T.TEMPORAL_WEEKDAYS_ONLY, **TOD)
    plan.set_temporal(4, T.TEMPORAL_RANGE, lo=10)
    plan.set_histogram_edges(6, EDGES)
    return plan


def blob_of(k):
    """every counter a multiple of k, so that two blobs add to something neither holds"""
    cells = [k * c for c in (1, 2, 3, 4, 5, 6, 7, 8, 9)]
    buckets = [k * c for c in (5, 6, 7, 8)]
    return wire.pack(
        count=[wire.count_acc(100 * k, 90 * k)],
        joint=[wire.joint_range_state(100 * k, 70 * k, 2 * k, -1.5 * k, 2.5, -8.0, 4.0 * k),
               wire.joint_count_state(BINNING, 100 * k, cells, outside=3 * k, non_finite=4 * k)],
        temporal=[wire.temporal_state(1, T.TEMPORAL_KEEP_NULLS, 100 * k, 80 * k, 50 * k, delta=5),
                  wire.temporal_state(2, T.TEMPORAL_WEEKDAYS_ONLY, 100 * k, 60 * k, 40 * k, ticks_per_second=1000,
                                      lo=TOD["tod_lo"], hi=TOD["tod_hi"]),
                  wire.temporal_state(3, 0, 100 * k, 90 * k, 90 * k, lo=10, hi=I64_MAX)],
        hist=[wire.hist_range_state(100 * k, 70 * k, 5 * k, -1.5, 2.5 * k, 10.0 * k, 20.0 * k),
              wire.hist_count_state(EDGES, 100 * k, buckets, else_rows=3 * k, non_finite=4 * k)])


def answers(st):
    return dict(joint_range=st.joint_range(0), joint_counts=st.joint_counts(1),
                temporal=[st.temporal_counts(i) for i in (2, 3, 4)],
                hist_range=st.histogram_range(5), hist_counts=st.histogram_counts(6),
                totals=[(r.total, r.non_null, r.matches) for r in st.finalize()])


def expected(k, x_min, x_max_y, hist_max):
    """what a state holding blob_of(1) + ... (counters k times those of blob_of(1)) answers"""
    return dict(
        joint_range=dict(total=100 * k, n=70 * k, non_finite=2 * k, x_min=x_min, x_max=2.5, y_min=-8.0, y_max=x_max_y),
        joint_counts=([k * c for c in (1, 2, 3, 4, 5, 6, 7, 8, 9)], 3 * k),
        # KEEP_NULLS considers every row seen; the weekday filter and the plain range only the live ones
        temporal=[(100 * k, 100 * k, 50 * k), (100 * k, 60 * k, 20 * k), (100 * k, 90 * k, 0)],
        hist_range=dict(total=100 * k, nulls=25 * k, non_finite=5 * k, n=70 * k, min=-1.5, max=hist_max, sum=10.0 * k,
                        sum_squared=20.0 * k),
        hist_counts=([k * c for c in (5, 6, 7, 8)], 3 * k, 4 * k),
        totals=[(100 * k, 70 * k, 0), (100 * k, 45 * k, 0),
                (100 * k, 100 * k, 50 * k), (100 * k, 60 * k, 40 * k), (100 * k, 90 * k, 90 * k),
                (100 * k, 75 * k, 0), (100 * k, 30 * k, 0), (100 * k, 90 * k, 0)])


def test_three_sections_round_trip_and_answer_what_was_packed():
    plan = plan_of_all_three()
    blob = blob_of(1)
    assert blob.index(b"JNTB") < blob.index(b"TMPR") < blob.index(b"HIST")
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    assert answers(st) == expected(1, -1.5, 4.0, 2.5)
    assert st.serialize() == blob  # (reading changes nothing)
    st.reset()
    got = answers(st)
    assert got["joint_counts"] == ([0] * 9, 0) and got["temporal"] == [(0, 0, 0)] * 3
    assert got["hist_counts"] == ([0] * 4, 0, 0) and got["hist_range"]["n"] == 0 and math.isnan(got["hist_range"]["min"])
    assert got["joint_range"]["n"] == 0 and math.isnan(got["joint_range"]["x_max"])
    assert all(t == (0, 0, 0) for t in got["totals"])


def test_every_proper_prefix_is_refused():
    plan = plan_of_all_three()
    blob = blob_of(1)
    for n in range(len(blob)):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:n])
    # a section cut off at its end is a blob of another plan, not a shorter blob of this one
    for magic in (b"JNTB", b"TMPR", b"HIST"):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*(truncated|different plan)"):
            T.State.deserialize(plan, blob[:blob.index(magic)])
    # and the library goes on working
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob and answers(st) == expected(1, -1.5, 4.0, 2.5)


def test_merging_host_only_states_adds_every_counter():
    plan = plan_of_all_three()
    st = T.State.deserialize(plan, blob_of(1))
    st.merge([T.State.deserialize(plan, blob_of(2))])
    # counters and sums add, extremes go by min / max: x_min -1.5 and -3.0, y_max 4.0 and 8.0, the histogram's max 2.5 and 5.0
    assert answers(st) == expected(3, -3.0, 8.0, 5.0)
    # the merged state is one more blob of the plan
    again = T.State.deserialize(plan, st.serialize())
    assert answers(again) == expected(3, -3.0, 8.0, 5.0)
    st.merge([again, T.State.deserialize(plan, blob_of(1))])
    assert answers(st) == expected(7, -3.0, 8.0, 5.0)
