"""TGX_CHECK_HISTOGRAM and HistogramAnalyzer without a device: plan validation, what a host-only state answers from a
blob, the blob's section (term_amd/wire.py), and the analyzer's merge_states / metric_from_state on state JSON."""
import json
import math
import os
import re

import pytest

import exact_histogram as eh
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "histogram_vectors.json")) as f:
    GOLDEN = json.load(f)

EDGES = [0.0, 1.0, 2.0, 4.0, 3.5]  # 4 buckets; the last edge lies below the one before


def hist_plan(*extra):
    return T.Plan([spec(T.HISTOGRAM, 0)] + list(extra))


# ---- plan validation --------------------------------------------------------------------------------------------
def test_abi_version_and_constants():
    assert T.lib().tgx_abi_version() == 6
    assert (T.HISTOGRAM, T.HISTOGRAM_MAX_BUCKETS) == (12, 1000)
    assert {"tgx_plan_set_histogram_edges", "tgx_histogram_range_get", "tgx_histogram_counts"} <= set(T.abi_symbols())


def test_edges_are_validated():
    plan = hist_plan()
    for edges in ([0.0], [0.0] * 1002):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*between 1 and 1000"):
            plan.set_histogram_edges(0, edges)
    for edges in ([0.0, math.nan], [math.inf, 1.0], [0.0, 1.0, -math.inf], [0.0, 1.0, 2.0, math.nan]):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not finite"):
            plan.set_histogram_edges(0, edges)
    for edges in ([1.0, 0.5, 2.0], [0.0, 2.0, 1.0, 3.0], [0.0, 1.0, 2.0, 1.9999, 5.0]):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*non-decreasing"):
            plan.set_histogram_edges(0, edges)
    plan.set_histogram_edges(0, [0.0, 1.0])
    plan.set_histogram_edges(0, [0.0] * 1001)  # 1000 buckets; equal edges are in order; may be set again
    plan.set_histogram_edges(0, EDGES)           # a last edge below the one before is accepted
    for case in GOLDEN["degenerate"]:
        plan.set_histogram_edges(0, eh.edges_of(case["min"], case["max"], case["num_buckets"]))


def test_setter_is_refused_after_the_first_state_and_on_other_kinds():
    plan = hist_plan(spec(T.NUMERIC_STATS, 0), spec(T.JOINT_BINS, 0, column2=1))
    for other in (1, 2, 3):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a HISTOGRAM"):
            plan.set_histogram_edges(other, EDGES)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a JOINT_BINS"):
        plan.set_joint_binning(0, 0.0, 1.0, 0.0, 1.0, 5)
    plan.set_histogram_edges(0, EDGES)
    st = T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*once a state"):
        plan.set_histogram_edges(0, EDGES)
    st.close()


# ---- the blob's section -----------------------------------------------------------------------------------------
def two_phase_plan():
    plan = hist_plan(spec(T.HISTOGRAM, 1), spec(T.COUNT, 0))
    plan.set_histogram_edges(0, EDGES)
    return plan


def test_blob_roundtrip_through_a_host_only_state():
    counts = [5, 6, 7, 8]
    plan = two_phase_plan()
    blob = wire.pack(count=[wire.count_acc(9000, 8000)],
                     hist=[wire.hist_count_state(EDGES, 9000, counts, else_rows=3, non_finite=4),
                           wire.hist_range_state(9000, 7000, 5, -1.5, 2.5, 10.0, 20.0)])
    assert b"HIST" in blob
    st = T.State.deserialize(plan, blob)
    assert st.histogram_counts(0) == (counts, 3, 4)
    r = st.histogram_range(0)
    assert (r["total"], r["n"], r["non_finite"], r["nulls"]) == (9000, 26, 4, 9000 - 30)
    assert all(math.isnan(r[k]) for k in ("min", "max", "sum", "sum_squared"))
    assert st.histogram_range(1) == dict(total=9000, nulls=1995, non_finite=5, n=7000, min=-1.5, max=2.5, sum=10.0,
                                         sum_squared=20.0)
    res = st.finalize()
    assert [(x.total, x.non_null) for x in res] == [(9000, 30), (9000, 7005), (9000, 8000)]
    assert st.serialize() == blob
    # merged without a device: counts, n and the sums add, extremes by min / max
    other = T.State.deserialize(plan, wire.pack(count=[wire.count_acc(1, 1)],
                                                hist=[wire.hist_count_state(EDGES, 10, [1] * 4, else_rows=1),
                                                      wire.hist_range_state(10, 10, 0, -9.0, 0.0, 0.5, 0.25)]))
    st.merge([other])
    assert st.histogram_counts(0) == ([c + 1 for c in counts], 4, 4)
    assert st.histogram_range(1) == dict(total=9010, nulls=1995, non_finite=5, n=7010, min=-9.0, max=2.5, sum=10.5,
                                         sum_squared=20.25)
    st.reset()
    r = st.histogram_range(1)
    assert st.histogram_counts(0) == ([0] * 4, 0, 0) and (r["n"], r["sum"]) == (0, 0.0) and math.isnan(r["max"])
    with pytest.raises(T.TgxError, match="range phase"):
        st.histogram_counts(1)


def test_truncated_and_foreign_blobs_are_refused():
    plan = two_phase_plan()
    blob = wire.pack(count=[wire.count_acc(9, 8)], hist=[wire.hist_count_state(EDGES, 9, [1, 2, 3, 2]),
                                                         wire.hist_range_state(9, 0)])
    T.State.deserialize(plan, blob)
    for cut in (1, 8, 40, 100, len(blob) - 60):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    # states counted under other edges do not merge: their blobs are refused by a plan that holds different ones
    for edges in (EDGES[:-1] + [3.75], [0.0, 1.0, 2.0, 4.0], EDGES[:-1] + [4.0, 9.0]):
        other = hist_plan(spec(T.HISTOGRAM, 1), spec(T.COUNT, 0))
        other.set_histogram_edges(0, edges)
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other edges"):
            T.State.deserialize(other, blob)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other edges"):
        T.State.deserialize(hist_plan(spec(T.HISTOGRAM, 1), spec(T.COUNT, 0)), blob)  # (the range phase)
    # and a state of another plan does not merge at all
    same_edges = two_phase_plan()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*does not belong"):
        T.State.deserialize(plan, blob).merge([T.State.deserialize(same_edges, blob)])


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0), spec(T.COMOMENTS, 1, column2=2)])
    blob = wire.pack(count=[wire.count_acc(10, 7)], comoments=[wire.comoment_acc(10, 8, 1.0, 2.0, 3.0, 4.0, 5.0)])
    assert wire.pack(count=[wire.count_acc(10, 7)], comoments=[wire.comoment_acc(10, 8, 1.0, 2.0, 3.0, 4.0, 5.0)],
                     hist=()) == blob and b"HIST" not in blob
    assert T.State.deserialize(plan, blob).serialize() == blob


# ---- the analyzer's host half -----------------------------------------------------------------------------------
def test_analyzer_from_json_and_the_clamp():
    a = S.HistogramAnalyzer("x", 5)
    assert a.name() == "histogram" and a.metric_key() == "histogram"
    assert a.spec == {"type": "histogram", "column": "x", "num_buckets": 5}
    assert S.HistogramAnalyzer("x", 0).spec["num_buckets"] == 1 and S.HistogramAnalyzer("x", 5000).spec["num_buckets"] == 1000
    assert S.HistogramAnalyzer("x").spec["num_buckets"] == 10
    # the library clamps as HistogramAnalyzer::new does, whatever the JSON says
    for n in (0, 1, 1000, 10**6):
        assert S._Analyzer({"type": "histogram", "column": "x", "num_buckets": n}).merge_states([eh.histogram_state([1.0], 1)])
    with pytest.raises(T.TgxError, match="needs a column"):
        S._Analyzer({"type": "histogram"}).merge_states([{}])
    with pytest.raises(T.TgxError, match="unknown analyzer type 'entropy'"):
        S._Analyzer({"type": "entropy", "column": "x"}).merge_states([{}])


def test_metric_from_state_on_the_reference_table():
    g = GOLDEN["reference_table"]
    a = S.HistogramAnalyzer("x", g["num_buckets"])
    state = eh.histogram_state(g["values"], g["num_buckets"])
    m = a.compute_metric_from_state(state)
    assert m["type"] == "Histogram"
    v = m["value"]
    assert v["buckets"] == state["buckets"] and [b["count"] for b in v["buckets"]] == g["counts"]
    assert (v["total_count"], v["min"], v["max"]) == (g["total_count"], g["min"], g["max"])
    mean = 33.0 / 9.0
    assert v["mean"] == mean and v["std_dev"] == math.sqrt(177.0 / 9.0 - mean * mean)
    # total_count is the sum of the buckets (from_buckets), not the state's total_count
    assert a.compute_metric_from_state(dict(state, total_count=100))["value"]["total_count"] == 9
    # one row: no standard deviation -> unwrap_or(0.0); a negative variance -> NaN -> null
    one = eh.histogram_state([5.0], 3)
    assert a.compute_metric_from_state(one)["value"]["std_dev"] == 0.0
    assert a.compute_metric_from_state(dict(one, total_count=2, sum=10.0, sum_squared=49.0))["value"]["std_dev"] is None
    empty = eh.histogram_state([None], 3)
    assert a.compute_metric_from_state(empty) == {"type": "Histogram", "value": {
        "buckets": [], "total_count": 0, "min": 0.0, "max": 0.0, "mean": 0.0, "std_dev": 0.0}}


def test_merge_states_follows_the_reference():
    a = S.HistogramAnalyzer("x", 4)
    left, right = [1.0, 2.0, 2.5, 9.0], [0.5, 3.0, 3.0, 12.0, None]
    s1, s2 = eh.histogram_state(left, 4), eh.histogram_state(right, 4)
    merged = a.merge_states([s1, s2])
    # the first state's bucket structure, counts added index by index
    assert [(b["lower_bound"], b["upper_bound"]) for b in merged["buckets"]] == [(b["lower_bound"], b["upper_bound"]) for b in s1["buckets"]]
    assert [b["count"] for b in merged["buckets"]] == [x["count"] + y["count"] for x, y in zip(s1["buckets"], s2["buckets"])]
    assert (merged["min_value"], merged["max_value"], merged["total_count"]) == (0.5, 12.0, 8)
    assert (merged["sum"], merged["sum_squared"]) == (s1["sum"] + s2["sum"], s1["sum_squared"] + s2["sum_squared"])
    # another bucket count: the counts of that state are left out, everything else still adds
    s3 = eh.histogram_state(right, 3)
    other = a.merge_states([s1, s3])
    assert other["buckets"] == s1["buckets"] and other["total_count"] == 8 and other["max_value"] == 12.0
    # the empty state takes part with its zeros, as the reference's does
    assert a.merge_states([s2, eh.histogram_state([], 4)])["min_value"] == 0.0
    assert a.merge_states([s1]) == s1
    with pytest.raises(T.TgxError, match="Failed to merge states: No states to merge"):
        a.merge_states([])


def test_state_and_metric_token_kinds():
    """`count`, `total_count` are integer tokens (u64 fields); bounds and statistics are float tokens"""
    a = S.HistogramAnalyzer("x", 2)
    state = eh.histogram_state([1.0, 2.0, 3.0, 4.0], 2)
    text = a.merge_states_text([state, state])
    assert re.search(r'"count": 4[,}]', text) and re.search(r'"total_count": 8[,}]', text)
    assert '"lower_bound": 1.0' in text and '"min_value": 1.0' in text and '"sum": 20.0' in text and '"sum_squared": 60.0' in text
    big = {"buckets": [{"lower_bound": 0.0, "upper_bound": 1.0, "count": 2**60}], "min_value": 0.0, "max_value": 0.5,
           "total_count": 2**60, "sum": 1.0, "sum_squared": 1.0}
    text = a.merge_states_text([big, big])
    assert text.count(str(2**61)) == 2
    out = S.C.c_char_p()
    err = S._Error()
    S._host_check(S._host().tgx_host_metric_from_state_json(json.dumps(a.spec).encode(), json.dumps(big).encode(),
                                                            S.C.byref(out), S.C.byref(err)), err)
    metric = S._take(out)
    assert '"count": %d}' % 2**60 in metric and '"total_count": %d,' % 2**60 in metric and '"min": 0.0' in metric


def test_inconsistent_blobs_are_refused():
    """counts that do not add up, or a range that is none, would make the accessors answer nonsense"""
    plan = two_phase_plan()
    good_counts, good_range = wire.hist_count_state(EDGES, 100, [1, 2, 3, 4], else_rows=2), wire.hist_range_state(100, 50, 1, -1.0, 1.0)
    T.State.deserialize(plan, wire.pack(count=[wire.count_acc(1, 1)], hist=[good_counts, good_range]))
    n_at = 8 + 8 * len(EDGES) + 8  # u32 counted, u32 buckets, the edges, i64 total: then i64 n
    wrong_n = good_counts[:n_at] + (11).to_bytes(8, "little") + good_counts[n_at + 8:]
    bad = [(wire.hist_count_state(EDGES, 5, [1, 2, 3, 4]), good_range),              # more rows in buckets than seen
           (wrong_n, good_range),                                                    # n is not the sum of the buckets
           (wire.hist_count_state(EDGES, 100, [1, 2, 3, 4], else_rows=5), good_range),  # more ELSE rows than the last bucket
           (wire.hist_count_state(EDGES, 100, [1, 2, 3, 4], non_finite=91), good_range),
           (good_counts, wire.hist_range_state(100, 101)),
           (good_counts, wire.hist_range_state(100, -1)),
           (good_counts, wire.hist_range_state(100, 50, 51, -1.0, 1.0)),
           (good_counts, wire.hist_range_state(100, 50, 0, 2.0, 1.0)),                # min above max
           (good_counts, wire.hist_range_state(100, 50, 0, None, None)),             # rows without extremes
           (good_counts, wire.hist_range_state(100, 50, 0, math.nan, 1.0))]
    for counted, ranged in bad:
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*inconsistent"):
            T.State.deserialize(plan, wire.pack(count=[wire.count_acc(1, 1)], hist=[counted, ranged]))
