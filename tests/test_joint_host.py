"""TGX_CHECK_JOINT_BINS and MutualInformationAnalyzer without a device: plan validation, the analyzer's merge_states /
metric_from_state on the reference's own vectors (tests/golden/mutual_information_vectors.json), the token kinds of its
state text, and the state blob's section (term_amd/wire.py)."""
import json
import math
import os
import re

import pytest

import exact_joint as ej
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "mutual_information_vectors.json")) as f:
    GOLDEN = json.load(f)

BINNING = (0.0, 1.0, -2.0, 0.5, 10)


def joint_plan(*extra):
    return T.Plan([spec(T.JOINT_BINS, 0, column2=1)] + list(extra))


# ---- plan validation --------------------------------------------------------------------------------------------
def test_binning_is_validated():
    plan = joint_plan()
    for bins in (0, 1):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*at least 2"):
            plan.set_joint_binning(0, 0.0, 1.0, 0.0, 1.0, bins)
    for bins in (T.JOINT_MAX_BINS + 1, 1000):
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*at most 127.*LDS"):
            plan.set_joint_binning(0, 0.0, 1.0, 0.0, 1.0, bins)
    for bad in ((0.0, 0.0, 0.0, 1.0), (0.0, -1.0, 0.0, 1.0), (0.0, math.inf, 0.0, 1.0), (math.nan, 1.0, 0.0, 1.0),
                (0.0, 1.0, -math.inf, 1.0), (0.0, 1.0, 0.0, math.nan)):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*finite"):
            plan.set_joint_binning(0, *bad, 10)
    plan.set_joint_binning(0, 0.0, 1.0, 0.0, 1.0, 2)
    plan.set_joint_binning(0, 0.0, 1.0, 0.0, 1.0, T.JOINT_MAX_BINS)  # (may be set again until a state exists)


def test_column2_is_required():
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*column2"):
        T.Plan([spec(T.JOINT_BINS, 0)])


def test_setter_is_refused_after_the_first_state_and_on_other_kinds():
    plan = joint_plan(spec(T.COMOMENTS, 0, column2=1))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a JOINT_BINS"):
        plan.set_joint_binning(1, *BINNING)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a JOINT_BINS"):
        plan.set_joint_binning(2, *BINNING)
    plan.set_joint_binning(0, *BINNING)
    st = T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*once a state"):
        plan.set_joint_binning(0, *BINNING)
    st.close()


# ---- the analyzer's host half -----------------------------------------------------------------------------------
def label(i):
    return "%d.0" % i


def state_of(cells, bins):
    xc, yc = ej.marginals(cells)
    return {"n": sum(cells.values()), "bins": bins,
            "joint_counts": [[label(i), label(j), c] for (i, j), c in sorted(cells.items())],
            "x_counts": {label(i): c for i, c in sorted(xc.items())}, "y_counts": {label(j): c for j, c in sorted(yc.items())}}


def reference_table(name):
    xs = [float(i) for i in range(100)]
    ys = [float((37 * i + 13) % 100) for i in range(100)] if name == "independent" else [2.0 * i for i in range(100)]
    return xs, ys


@pytest.mark.parametrize("name", ["independent", "dependent"])
def test_metric_from_state_on_the_reference_vectors(name):
    g = GOLDEN[name]
    xs, ys = reference_table(name)
    cells, _ = ej.joint_counts(xs, ys, ej.binning_of(xs, ys, g["bins"]))
    a = S.MutualInformationAnalyzer("x", "y", g["bins"])
    m = a.compute_metric_from_state(state_of(cells, g["bins"]))
    assert m["type"] == "Double"
    exact, magnitude, used = ej.mutual_information(cells, 100)
    assert used == g["non_empty_cells"]
    # per term: two divisions, a product, a division, ln (1 ulp), a product; the running sum rounds once per term on a
    # partial sum below the sum of magnitudes; the division by LN_2 and LN_2 itself one more each
    bound = (8 * used + 4) * 2.0 ** -53 * float(magnitude)
    assert abs(m["value"] - float(exact)) <= bound
    assert abs(m["value"] - float(g["metric"])) < 1e-13
    assert (m["value"] < g["metric_below"]) if name == "independent" else (m["value"] > g["metric_above"])


def test_merge_states_on_the_reference_vector():
    g = GOLDEN["merge"]
    a = S.MutualInformationAnalyzer("x", "y", 5)
    assert a.name() == "mutual_information" and a.metric_key() == "mutual_information_x_y"
    assert a.merge_states(g["states"]) == g["merged"]
    other = dict(g["states"][1], bins=10)
    with pytest.raises(T.TgxError, match=g["different_bins_error"]):
        a.merge_states([g["states"][0], other])
    with pytest.raises(T.TgxError, match="Cannot merge empty states"):
        a.merge_states([])


def test_merge_adds_cells_label_by_label():
    xs, ys = reference_table("independent")
    binning = ej.binning_of(xs, ys, 5)
    halves = [ej.joint_counts(xs[lo:hi], ys[lo:hi], binning)[0] for lo, hi in ((0, 37), (37, 100))]
    whole = ej.joint_counts(xs, ys, binning)[0]
    a = S.MutualInformationAnalyzer("x", "y", 5)
    merged = a.merge_states([state_of(h, 5) for h in halves])
    want = state_of(whole, 5)
    assert merged["n"] == 100 and merged["bins"] == 5
    assert sorted(map(tuple, merged["joint_counts"])) == sorted(map(tuple, want["joint_counts"]))
    assert merged["x_counts"] == want["x_counts"] and merged["y_counts"] == want["y_counts"]
    assert a.compute_metric_from_state(merged)["value"] == pytest.approx(float(GOLDEN["independent"]["metric"]), abs=1e-13)


def test_empty_state_gives_zero():
    a = S.MutualInformationAnalyzer("x", "y")
    assert a.spec["bins"] == 10 and S.MutualInformationAnalyzer("x", "y", 1).spec["bins"] == 2
    empty = {"n": 0, "bins": 10, "joint_counts": [], "x_counts": {}, "y_counts": {}}
    assert a.compute_metric_from_state(empty) == {"type": "Double", "value": 0.0}


def test_state_text_token_kinds():
    """`n`, `bins` and every count are integer tokens (u64 / usize fields of the reference's struct)"""
    a = S.MutualInformationAnalyzer("x", "y", 5)
    text = a.merge_states_text(GOLDEN["merge"]["states"])
    assert re.search(r'"n": 100[,}]', text) and re.search(r'"bins": 5[,}]', text)
    assert '["0", "0", 25]' in text and '"x_counts": {"0": 25}' in text and '"y_counts": {"0": 25}' in text
    assert not re.search(r"\d\.\d", text)  # no float token anywhere
    big = {"n": 2**60, "bins": 5, "joint_counts": [["0.0", "1.0", 2**60]], "x_counts": {"0.0": 2**60}, "y_counts": {"1.0": 2**60}}
    assert str(2**61) in a.merge_states_text([big, big])


def test_other_analyzer_types_stay_as_they_were():
    with pytest.raises(T.TgxError, match="unknown analyzer type 'entropy'"):
        S._Analyzer({"type": "entropy", "column": "x"}).merge_states([{}])


# ---- the blob's section -----------------------------------------------------------------------------------------
def test_blob_roundtrip_through_a_host_only_state():
    cells = list(range(121))
    plan = joint_plan(spec(T.JOINT_BINS, 0, column2=1), spec(T.COUNT, 0))
    plan.set_joint_binning(0, *BINNING)
    blob = wire.pack(count=[wire.count_acc(9000, 8000)],
                     joint=[wire.joint_count_state(BINNING, 9000, cells, outside=3, non_finite=4),
                            wire.joint_range_state(9000, 7000, 5, -1.5, 2.5, 10.0, 20.0)])
    st = T.State.deserialize(plan, blob)
    assert st.joint_counts(0) == (cells, 3)
    r = st.joint_range(0)
    assert (r["total"], r["n"], r["non_finite"]) == (9000, sum(cells), 4) and math.isnan(r["x_min"])
    assert st.joint_range(1) == dict(total=9000, n=7000, non_finite=5, x_min=-1.5, x_max=2.5, y_min=10.0, y_max=20.0)
    res = st.finalize()
    assert (res[0].total, res[0].non_null, res[1].non_null, res[2].non_null) == (9000, sum(cells), 7000, 8000)
    assert st.serialize() == blob
    # merged without a device: counts and n add, extremes by min / max
    other = T.State.deserialize(plan, wire.pack(count=[wire.count_acc(1, 1)],
                                                joint=[wire.joint_count_state(BINNING, 10, [1] * 121),
                                                       wire.joint_range_state(10, 10, 0, -9.0, 0.0, 12.0, 30.0)]))
    st.merge([other])
    assert st.joint_counts(0) == ([c + 1 for c in cells], 3)
    assert st.joint_range(1) == dict(total=9010, n=7010, non_finite=5, x_min=-9.0, x_max=2.5, y_min=10.0, y_max=30.0)
    st.reset()
    assert st.joint_counts(0) == ([0] * 121, 0) and st.joint_range(1)["n"] == 0 and math.isnan(st.joint_range(1)["y_max"])
    # truncated, another binning, another phase
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plan, blob[:-8])
    plan5 = joint_plan(spec(T.JOINT_BINS, 0, column2=1), spec(T.COUNT, 0))
    plan5.set_joint_binning(0, *(BINNING[:4] + (5,)))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*another binning"):
        T.State.deserialize(plan5, blob)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*another binning"):
        T.State.deserialize(joint_plan(spec(T.JOINT_BINS, 0, column2=1), spec(T.COUNT, 0)), blob)
    with pytest.raises(T.TgxError, match="range phase"):
        st.joint_counts(1)


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0), spec(T.COMOMENTS, 1, column2=2)])
    blob = wire.pack(count=[wire.count_acc(10, 7)], comoments=[wire.comoment_acc(10, 8, 1.0, 2.0, 3.0, 4.0, 5.0)])
    assert wire.pack(count=[wire.count_acc(10, 7)], comoments=[wire.comoment_acc(10, 8, 1.0, 2.0, 3.0, 4.0, 5.0)],
                     joint=()) == blob and b"JNTB" not in blob
    assert T.State.deserialize(plan, blob).serialize() == blob
