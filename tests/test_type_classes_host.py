"""TGX_CHECK_TYPE_CLASSES and DataTypeAnalyzer without a device: the lexer the kernels compile (tgx_host_type_class)
against the exact reference, plan validation, host-only states from term_amd/wire.py blobs (answers, merges, round trips,
refusals) and the analyzer's plans, states, merges, metrics and errors through the C++ host ABI and the Python twin."""
import json
import os

import pytest

import exact_type_classes as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_type_vectors.json")
with open(GOLDEN) as _f:
    G = json.load(_f)

SEEDED = ex.seeded_strings(20000)


# ---- the lexer ------------------------------------------------------------------------------------------------------------
def test_abi_constants_and_symbols():
    assert T.TYPE_CLASSES == 21 and T.lib().tgx_abi_version() == 6
    assert (T.TYPE_CLASS_BOOLEAN, T.TYPE_CLASS_INTEGER, T.TYPE_CLASS_DOUBLE, T.TYPE_CLASS_DATE, T.TYPE_CLASS_DATETIME,
            T.TYPE_CLASS_STRING, T.TYPE_CLASS_UNDECIDED) == \
        (ex.BOOLEAN, ex.INTEGER, ex.DOUBLE, ex.DATE, ex.DATETIME, ex.STRING, ex.UNDECIDED) == tuple(range(7))
    assert T.TYPE_CLASS_NAMES == ex.NAMES
    for name in ("tgx_type_classes_get", "tgx_host_type_class", "tgx_host_data_type_state_json"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "tgx.h")) as f:
        header = f.read()
    assert "TGX_CHECK_TYPE_CLASSES = 21" in header and '"type_classes"' in header


def test_the_host_lexer_equals_the_reference_on_the_edge_table():
    wrong = [(v[:40], ex.NAMES[want], ex.NAMES[T.host_type_class(v)]) for v, want in ex.EDGES if T.host_type_class(v) != want]
    assert not wrong, wrong


def test_the_host_lexer_equals_the_reference_on_seeded_strings():
    wrong = [(v, ex.NAMES[ex.classify(v)], ex.NAMES[T.host_type_class(v)]) for v in SEEDED
             if T.host_type_class(v) != ex.classify(v)]
    assert not wrong, wrong[:10]


def test_the_host_lexer_takes_text_and_the_empty_value():
    assert T.host_type_class("") == T.host_type_class(b"") == ex.STRING
    assert T.host_type_class("é") == ex.STRING and T.host_type_class("TRUE") == ex.BOOLEAN
    assert T.lib().tgx_host_type_class(None, 0) == ex.STRING


# ---- plans ----------------------------------------------------------------------------------------------------------------
def test_plan_validation():
    T.Plan([spec(T.TYPE_CLASSES, 0)])
    T.Plan([spec(T.TYPE_CLASSES, 3), spec(T.COUNT, 0), spec(T.TYPE_CLASSES, 1)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*column2 must be -1"):
        T.Plan([spec(T.TYPE_CLASSES, 0, column2=1)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*no column list"):
        T.Plan([spec(T.TYPE_CLASSES, 0, columns=[0, 1])])
    one = spec(T.TYPE_CLASSES, 0)  # (spec() keeps lists from two columns on: a list of one is set by hand)
    import ctypes as C
    arr = (C.c_int32 * 1)(0)
    one.columns, one.n_columns = C.cast(arr, C.POINTER(C.c_int32)), 1
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*no column list"):
        T.Plan([one])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*negative column index"):
        T.Plan([spec(T.TYPE_CLASSES, -1)])


def blob_of(*tasks, count=(10, 9)):
    return wire.pack(count=[wire.count_acc(*count)], type_classes=[wire.type_classes_state(*t) for t in tasks])


A = (10, 9, 1, 2, 3, 1, 1, 1, 0)  # seen, non_null, boolean .. undecided
B = (7, 4, 0, 0, 0, 0, 0, 2, 2)


def as_dict(t):
    return dict(zip(ex.COUNTERS, t))


def test_two_specs_on_one_column_are_one_task():
    plan = T.Plan([spec(T.TYPE_CLASSES, 0), spec(T.COUNT, 0), spec(T.TYPE_CLASSES, 0), spec(T.TYPE_CLASSES, 1)])
    st = T.State.deserialize(plan, blob_of(A, B))  # two tasks: column 0 (specs 0 and 2), column 1
    assert st.type_classes(0) == st.type_classes(2) == as_dict(A) and st.type_classes(3) == as_dict(B)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*TYPE_CLASSES section"):
        T.State.deserialize(plan, blob_of(A, A, B))


def test_a_host_only_state_answers_zeros_merges_and_round_trips():
    plan = T.Plan([spec(T.TYPE_CLASSES, 0), spec(T.COUNT, 0), spec(T.TYPE_CLASSES, 1)])
    zero = blob_of((0,) * 9, (0,) * 9, count=(0, 0))
    st = T.State.deserialize(plan, zero)
    assert st.type_classes(0) == st.type_classes(2) == dict.fromkeys(ex.COUNTERS, 0)
    blob = blob_of(A, B)
    st = T.State.deserialize(plan, blob)
    assert st.type_classes(0) == as_dict(A) and st.type_classes(2) == as_dict(B)
    res = st.finalize()
    assert [(res[i].total, res[i].non_null) for i in (0, 2)] == [(10, 9), (7, 4)]
    assert st.serialize() == blob
    st.merge([T.State.deserialize(plan, blob), T.State.deserialize(plan, blob)])
    assert st.type_classes(0) == as_dict(tuple(3 * x for x in A)) and st.type_classes(2) == as_dict(tuple(3 * x for x in B))
    for i in (0, 2):  # the identities
        c = st.type_classes(i)
        assert c["non_null"] == sum(c[n + "_rows"] for n in ex.NAMES) <= c["seen"]
    st.reset()
    assert st.type_classes(0) == dict.fromkeys(ex.COUNTERS, 0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a TYPE_CLASSES check"):
        st.type_classes(1)


def test_malformed_blobs_are_refused():
    plan = T.Plan([spec(T.TYPE_CLASSES, 0), spec(T.COUNT, 0)])
    for bad in ((10, 9, 1, 2, 3, 1, 1, 1, 1),          # the classes make 10, not 9
                (10, 9, 1, 2, 3, 1, 1, 0, 0),          # ... 8
                (8, 9, 1, 2, 3, 1, 1, 1, 0),           # non_null above seen
                (10, 9, (1 << 64) - 1, 2, 3, 1, 1, 1, 11)):  # a sum that wraps to 9
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed.*TYPE_CLASSES task 0"):
            T.State.deserialize(plan, blob_of(bad))
    blob = blob_of(A)
    for cut in (1, 8, 40, 72):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):  # the section is missing
        T.State.deserialize(plan, wire.pack(count=[wire.count_acc(10, 9)]))


def test_blobs_of_plans_without_the_kind_keep_their_bytes_and_the_section_is_last():
    plan = T.Plan([spec(T.COUNT, 0), spec(T.VALUE_RULE, 0)])
    plan.set_value_rule(1, T.RULE_GE_ZERO)
    blob = wire.pack(count=[wire.count_acc(10, 9)], value_rules=[wire.value_rule_state(1, 0, 10, 9, 7)])
    assert T.State.deserialize(plan, blob).serialize() == blob
    both = T.Plan([spec(T.COUNT, 0), spec(T.VALUE_RULE, 0), spec(T.TYPE_CLASSES, 1)])
    both.set_value_rule(1, T.RULE_GE_ZERO)
    with_section = wire.pack(count=[wire.count_acc(10, 9)], value_rules=[wire.value_rule_state(1, 0, 10, 9, 7)],
                             type_classes=[wire.type_classes_state(*A)])
    assert with_section.startswith(blob[:8]) and with_section.endswith(wire.type_classes_state(*A))
    assert T.State.deserialize(both, with_section).serialize() == with_section
    assert wire.TYPE_CLASSES_MAGIC.to_bytes(4, "little") == b"TCLS"


# ---- the analyzer ---------------------------------------------------------------------------------------------------------
def counters(**kw):
    c = dict.fromkeys(ex.COUNTERS, 0)
    c.update(kw)
    return c


def test_spec_name_and_metric_key():
    a = S.DataTypeAnalyzer("mixed_type")
    assert a.spec == {"type": "data_type", "column": "mixed_type"}
    assert a.name() == "data_type" and a.metric_key() == "data_type.mixed_type"
    assert S.DataTypeAnalyzer("c", arrow_type="Int32").spec == {"type": "data_type", "column": "c", "arrow_type": "Int32"}
    assert T.DataTypeAnalyzer is S.DataTypeAnalyzer


def test_a_string_column_plans_one_type_classes_request():
    a = S.DataTypeAnalyzer("c")
    for t in (T.UTF8, T.LARGE_UTF8, T.UTF8_VIEW, T.DICT32_UTF8, 0):
        assert a.planned_requests([t]) == [{"kind": T.TYPE_CLASSES, "column": "c", "column2": ""}]


def test_state_tokens_labels_and_absent_classes():
    a = S.DataTypeAnalyzer("c")
    g = G["mixed_type"]
    text = a.state_text_from_type_classes(ex.counts([v.encode() for v in g["values"]]))
    assert json.loads(text) == g["contract"]
    assert text == '{"type_counts": {"boolean": 3, "integer": 2, "double": 2, "date": 1, "string": 2}, "total_count": 10}'
    assert "." not in text  # u64 fields are integer tokens
    # DATETIME is folded into date; a class without rows is absent; total_count is non_null
    text = a.state_text_from_type_classes(counters(seen=20, non_null=12, date_rows=2, datetime_rows=3, string_rows=7))
    assert text == '{"type_counts": {"date": 5, "string": 7}, "total_count": 12}'
    assert a.state_text_from_type_classes(counters(seen=5, non_null=5, datetime_rows=5)) == \
        '{"type_counts": {"date": 5}, "total_count": 5}'
    assert a.state_text_from_type_classes(counters(seen=4)) == '{"type_counts": {}, "total_count": 0}'


def test_undecided_rows_are_the_analyzers_error_with_the_count():
    a = S.DataTypeAnalyzer("c")
    with pytest.raises(T.TgxError, match=r"column 'c' is not on the GPU path: 3 values look like dates in a form this path "
                                         r"does not decide"):
        a.state_text_from_type_classes(counters(seen=9, non_null=9, string_rows=6, undecided_rows=3))


def test_merge_states_and_the_metric():
    a = S.DataTypeAnalyzer("c")
    s1 = {"type_counts": {"integer": 2, "string": 1}, "total_count": 3}
    s2 = {"type_counts": {"string": 4, "date": 1}, "total_count": 5}
    merged = a.merge_states([s1, s2])
    assert merged == {"type_counts": {"integer": 2, "string": 5, "date": 1}, "total_count": 8}
    assert a.merge_states_text([s1, s2]) == '{"type_counts": {"integer": 2, "string": 5, "date": 1}, "total_count": 8}'
    assert a.merge_states([]) == {"type_counts": {}, "total_count": 0}
    metric = a.compute_metric_from_state(merged)
    assert metric == {"type": "Map", "value": {"integer": {"type": "Long", "value": 2}, "string": {"type": "Long", "value": 5},
                                               "date": {"type": "Long", "value": 1}}}
    assert a.compute_metric_from_state({"type_counts": {}, "total_count": 0}) == {"type": "Map", "value": {}}
    assert S.data_type_dominant_type(merged) == ("string", 5 / 8) and S.data_type_consistency(merged) == 5 / 8
    assert S.data_type_dominant_type({"type_counts": {}, "total_count": 0}) is None
    assert S.data_type_consistency({"type_counts": {}, "total_count": 0}) == 1.0
    assert S._state_is_empty(a, {"type_counts": {}, "total_count": 0}) and not S._state_is_empty(a, merged)


INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def test_an_integer_column_plans_two_value_rules_and_the_three_way_arithmetic():
    a = S.DataTypeAnalyzer("n")
    for t in (T.INT64, T.INT32, T.INT8, T.UINT32):
        reqs = a.planned_requests([t])
        assert [(r["kind"], r["column"]) for r in reqs] == [(T.VALUE_RULE, "n")] * 2
        assert [(r["value_rule"]["mode"], r["value_rule"]["flags"], r["value_rule"]["lo_i"], r["value_rule"]["hi_i"])
                for r in reqs] == [(T.RULE_BETWEEN, 0, 0, 1), (T.RULE_BETWEEN, 0, INT32_MIN, INT32_MAX)]
    assert len(S.DataTypeAnalyzer("n", arrow_type="Int16").planned_requests([T.INT64])) == 2
    # 100 rows, 90 non-NULL: 20 are 0 / 1, 70 fit Int32 (those 20 among them), 20 do not
    results = {"results": [{"total": 100, "non_null": 90, "matches": 20}, {"total": 100, "non_null": 90, "matches": 70}]}
    assert a.state_text_from_type_classes(results) == \
        '{"type_counts": {"boolean": 20, "integer": 50, "double": 20}, "total_count": 90}'
    # a column whose every value is 0 or 1
    flags = {"results": [{"total": 8, "non_null": 8, "matches": 8}, {"total": 8, "non_null": 8, "matches": 8}]}
    assert a.state_text_from_type_classes(flags) == '{"type_counts": {"boolean": 8}, "total_count": 8}'
    empty = {"results": [{"total": 3, "non_null": 0, "matches": 0}] * 2}
    assert a.state_text_from_type_classes(empty) == '{"type_counts": {}, "total_count": 0}'


def test_a_float_column_plans_a_count_and_is_all_double():
    a = S.DataTypeAnalyzer("x")
    for t in (T.FLOAT64, T.FLOAT32):
        assert a.planned_requests([t]) == [{"kind": T.COUNT, "column": "x", "column2": ""}]
    assert S.DataTypeAnalyzer("x", arrow_type="Float32").planned_requests([T.FLOAT64])[0]["kind"] == T.COUNT
    assert a.state_text_from_type_classes({"results": [{"total": 12, "non_null": 11}]}) == \
        '{"type_counts": {"double": 11}, "total_count": 11}'


def test_declared_types_outside_the_path_are_the_analyzers_error():
    for declared, layout in (("Timestamp(Nanosecond, None)", T.INT64), ("Date32", T.INT32), ("decimal128(10, 2)", T.INT64),
                             ("Boolean", T.BOOL), ("Binary", T.UTF8), ("UInt64", T.UINT64), ("Float16", T.INT32),
                             ("Interval(DayTime)", T.INT64), ("time32[s]", T.INT32)):
        with pytest.raises(T.TgxError, match=r"column 'c' \(.*\) is not on the GPU path"):
            S.DataTypeAnalyzer("c", arrow_type=declared).planned_requests([layout])
    for layout in (T.UINT64, T.BOOL):  # the layout alone says it
        with pytest.raises(T.TgxError, match=r"column 'c' \(.*\) is not on the GPU path"):
            S.DataTypeAnalyzer("c").planned_requests([layout])


def test_entropy_is_still_an_unknown_analyzer_type():
    with pytest.raises(T.TgxError, match="unknown analyzer type 'entropy'"):
        S._Analyzer({"type": "entropy", "column": "c"}).merge_states([])
    with pytest.raises(T.TgxError, match="analyzer 'data_type' needs a column"):
        S._Analyzer({"type": "data_type"}).merge_states([])
