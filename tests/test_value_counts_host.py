"""TGX_CHECK_VALUE_COUNTS without a device: plan validation, what a host-only state answers from a blob, merging by
value, every malformed-blob refusal of the section (term_amd/wire.py), and the histogram / entropy figures of
term_amd/value_counts.py with their bound errors, held against tests/exact_value_counts.py."""
import ctypes as C
import json
import struct

import pytest

import exact_value_counts as ex
import term_amd as T
from _lib_spec import spec
from term_amd import wire
from term_amd.value_counts import EntropyState, Histogram, OutOfBound

INTS = {5: 3, -1: 2, 7: 4}
TEXT = {b"b": 3, b"": 2, b"ab": 1, b"\xff": 1}


def counts_plan(mvb=16):
    plan = T.Plan([spec(T.VALUE_COUNTS, 0), spec(T.VALUE_COUNTS, 1), spec(T.COUNT, 0)])
    plan.set_value_counts(0, 4, 8)
    plan.set_value_counts(1, 100, mvb)
    return plan


def counts_blob(first=None, second=None, mvb=16):
    first = wire.value_counts_state(4, 8, 10, INTS, nulls=1) if first is None else first
    second = wire.value_counts_state(100, mvb, 10, TEXT, nulls=1, overflow_rows=1, long_rows=1) if second is None else second
    return wire.pack(count=[wire.count_acc(10, 9)], value_counts=[first, second])


def test_abi_constants():
    assert T.VALUE_COUNTS == 15 and (T.VALUE_COUNTS_MAX_DISTINCT, T.VALUE_COUNTS_MAX_VALUE_BYTES) == (65536, 256)
    for name in ("tgx_plan_set_value_counts", "tgx_value_counts_get", "tgx_value_counts_entries"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)


def test_parameters_are_validated():
    plan = T.Plan([spec(T.VALUE_COUNTS, 0), spec(T.COUNT, 0)])
    for bad in (0, 65537, 2**32 - 1):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_distinct must be 1 \.\. 65536 \(%d\)" % bad):
            plan.set_value_counts(0, bad, 16)
    for bad in (0, 257):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_value_bytes must be 1 \.\. 256 \(%d\)" % bad):
            plan.set_value_counts(0, 10, bad)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1 is not a VALUE_COUNTS check"):
        plan.set_value_counts(1, 10, 16)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*VALUE_COUNTS reads one column: column2 must be -1"):
        T.Plan([spec(T.VALUE_COUNTS, 0, column2=1)])
    for ok in ((1, 1), (65536, 256)):
        plan.set_value_counts(0, *ok)


def test_a_spec_without_parameters_fails_state_create_and_deserialize():
    plan = T.Plan([spec(T.VALUE_COUNTS, 0), spec(T.VALUE_COUNTS, 0)])
    plan.set_value_counts(0, 10, 16)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*tgx_plan_set_value_counts"):
        T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_plan_set_value_counts"):
        T.State.deserialize(plan, wire.pack(value_counts=[wire.value_counts_state(10, 16, 0, {})] * 2))


def test_setter_is_refused_after_the_first_state():
    plan = counts_plan()
    st = T.State.deserialize(plan, counts_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_value_counts(0, 5, 8)
    del st


def test_a_host_only_state_answers_its_blob():
    plan = counts_plan()
    st = T.State.deserialize(plan, counts_blob())
    summary, counts = st.value_counts(0)
    assert summary == dict(seen=10, non_null=9, distinct=3, counted=9, overflow_rows=0, long_rows=0)
    assert list(counts.items()) == [(-1, 2), (5, 3), (7, 4)]  # ascending int64
    summary, counts = st.value_counts(1)
    assert summary == dict(seen=10, non_null=9, distinct=4, counted=7, overflow_rows=1, long_rows=1)
    assert list(counts.items()) == [(b"", 2), (b"ab", 1), (b"b", 3), (b"\xff", 1)]  # bytewise, a prefix first
    res = st.finalize()
    assert [(r.total, r.non_null, r.distinct, r.matches) for r in res[:2]] == [(10, 9, 3, 9), (10, 9, 4, 7)]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 2 is not a VALUE_COUNTS check"):
        st.value_counts(2)


def test_the_entries_call_follows_the_size_query_convention():
    plan = counts_plan()
    st = T.State.deserialize(plan, counts_blob())
    L, err = T.lib(), T._lib._Error()
    n, nb, kind = C.c_uint64(), C.c_uint64(), C.c_int32()
    assert L.tgx_value_counts_entries(plan.h, st.h, 1, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(kind), C.byref(err)) == 0
    assert (n.value, nb.value, kind.value) == (4, 4, 1)
    small = (T._lib.ValueCountEntry * 3)()
    buf = (C.c_uint8 * 8)()
    assert L.tgx_value_counts_entries(plan.h, st.h, 1, small, 3, C.byref(n), buf, 8, C.byref(nb), C.byref(kind), C.byref(err)) != 0
    assert b"entries holds 3 entries, 4 are needed" in err.msg and n.value == 4
    full = (T._lib.ValueCountEntry * 4)()
    assert L.tgx_value_counts_entries(plan.h, st.h, 1, full, 4, C.byref(n), buf, 3, C.byref(nb), C.byref(kind), C.byref(err)) != 0
    assert b"bytes holds 3 bytes, 4 are needed" in err.msg
    assert L.tgx_value_counts_entries(plan.h, st.h, 0, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(kind), C.byref(err)) == 0
    assert (n.value, nb.value, kind.value) == (3, 0, 0)


def test_blob_round_trip_and_merge_by_value():
    plan = counts_plan()
    blob = counts_blob()
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    # a task without values, with and without rows, beside one with values
    for empty in (wire.value_counts_state(4, 8, 0, {}), wire.value_counts_state(4, 8, 3, {}, nulls=3)):
        assert T.State.deserialize(plan, counts_blob(first=empty)).serialize() == counts_blob(first=empty)
    other = counts_blob(wire.value_counts_state(4, 8, 6, {7: 1, 9: 5}), wire.value_counts_state(100, 16, 4, {b"b": 1, b"c": 2}, nulls=1))
    st.merge([T.State.deserialize(plan, other), T.State.deserialize(plan, blob)])
    summary, counts = st.value_counts(0)
    assert counts == {-1: 4, 5: 6, 7: 9, 9: 5} and summary["distinct"] == 4 and summary["seen"] == 26
    summary, counts = st.value_counts(1)
    assert counts == {b"": 4, b"ab": 2, b"b": 7, b"c": 2, b"\xff": 2}
    assert summary == dict(seen=24, non_null=21, distinct=5, counted=17, overflow_rows=2, long_rows=2)
    again = T.State.deserialize(plan, st.serialize())  # equal states, equal bytes
    assert again.serialize() == st.serialize() and again.value_counts(1) == st.value_counts(1)
    st.reset()
    assert st.value_counts(1) == (dict(seen=0, non_null=0, distinct=0, counted=0, overflow_rows=0, long_rows=0), {})


def test_integer_and_string_states_do_not_merge():
    plan = counts_plan()
    a = T.State.deserialize(plan, counts_blob())
    b = T.State.deserialize(plan, counts_blob(first=wire.value_counts_state(4, 8, 3, {b"x": 3})))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*VALUE_COUNTS task 0.*different column types"):
        a.merge([b])
    empty = T.State.deserialize(plan, counts_blob(first=wire.value_counts_state(4, 8, 3, {}, nulls=3)))
    a.merge([empty])  # (a state without values merges with either)
    assert a.value_counts(0)[0]["seen"] == 13


def raw_task(max_distinct, mvb, kind, seen, non_null, overflow, long_rows, entries, n=None):
    out = struct.pack("<4I5Q", max_distinct, mvb, kind, 0, seen, non_null, overflow, long_rows, len(entries) if n is None else n)
    for v, c in entries:
        out += struct.pack("<qQ", v, c) if kind == 1 else struct.pack("<I", len(v)) + v + struct.pack("<Q", c)
    return out


MALFORMED = [
    ("other parameters", raw_task(5, 8, 1, 3, 3, 0, 0, [(1, 3)]), None),
    ("other parameters", None, raw_task(100, 17, 2, 3, 3, 0, 0, [(b"a", 3)])),
    ("out of order or repeated", raw_task(4, 8, 1, 7, 7, 0, 0, [(7, 3), (5, 4)]), None),
    ("out of order or repeated", raw_task(4, 8, 1, 7, 7, 0, 0, [(5, 3), (5, 4)]), None),
    ("out of order or repeated", None, raw_task(100, 16, 2, 7, 7, 0, 0, [(b"b", 3), (b"ab", 4)])),
    ("out of order or repeated", None, raw_task(100, 16, 2, 7, 7, 0, 0, [(b"", 3), (b"", 4)])),
    ("zero count", raw_task(4, 8, 1, 3, 3, 0, 0, [(5, 3), (7, 0)]), None),
    ("a value of 17 bytes, max_value_bytes is 16", None, raw_task(100, 16, 2, 3, 3, 0, 0, [(b"x" * 17, 3)])),
    ("!= non_null", raw_task(4, 8, 1, 10, 8, 0, 0, [(5, 3), (7, 4)]), None),          # counted 7, non_null 8
    ("!= non_null", raw_task(4, 8, 1, 10, 7, 1, 0, [(5, 3), (7, 4)]), None),          # overflow on top
    ("!= non_null", None, raw_task(100, 16, 2, 10, 9, 1, 2, [(b"a", 7)])),            # 7 + 1 + 2 != 9
    ("!= non_null", raw_task(4, 8, 1, 6, 7, 0, 0, [(5, 3), (7, 4)]), None),           # non_null above seen
    ("kind", raw_task(4, 8, 3, 0, 0, 0, 0, []), None),
    ("kind", raw_task(4, 8, 0, 3, 3, 0, 0, [], n=1), None),                           # entries without a kind
    ("counts", raw_task(4, 8, 1, 10, 9, 0, 0, [(5, 2**64 - 1), (7, 2)]), None),       # a sum that wraps
]


@pytest.mark.parametrize("what,first,second", MALFORMED, ids=["%d-%s" % (i, m[0][:12]) for i, m in enumerate(MALFORMED)])
def test_malformed_blobs_are_refused(what, first, second):
    import re

    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + re.escape(what)):
        T.State.deserialize(counts_plan(), counts_blob(first, second))


def test_truncated_and_foreign_blobs_are_refused():
    plan, blob = counts_plan(), counts_blob()
    for cut in (1, 8, 9, 20, 60, 100):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):  # an entry count far beyond the blob's bytes
        T.State.deserialize(plan, counts_blob(first=raw_task(4, 8, 1, 3, 3, 0, 0, [(5, 3)], n=2**60)))
    other = T.Plan([spec(T.VALUE_COUNTS, 0), spec(T.COUNT, 0)])
    other.set_value_counts(0, 4, 8)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different plan"):
        T.State.deserialize(other, blob)


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0)])
    blob = wire.pack(count=[wire.count_acc(10, 9)])
    assert T.State.deserialize(plan, blob).serialize() == blob


# ---- the histogram and the entropy state -------------------------------------------------------------------------------------
def state_of(column, mvb=256, max_distinct=100):
    """the library's host-only state of a column the exact walk has counted"""
    s = ex.walk(column, mvb)
    plan = T.Plan([spec(T.VALUE_COUNTS, 0)])
    plan.set_value_counts(0, max_distinct, mvb)
    st = T.State.deserialize(plan, wire.pack(value_counts=[wire.value_counts_state(
        max_distinct, mvb, s["seen"], s["counts"], nulls=s["seen"] - s["non_null"], long_rows=s["long_rows"])]))
    return st.value_counts(0), s


def test_histogram_follows_the_sql_order_and_the_reference_accessors():
    (summary, counts), s = state_of([b"A"] * 6 + [b"B"] * 2 + [b"C"] * 2 + [None] * 2)
    h = Histogram.from_counts(summary, counts)
    assert [(b.value, b.count, b.ratio) for b in h.buckets] == ex.buckets(s) == [("A", 6, 0.6), ("B", 2, 0.2), ("C", 2, 0.2)]
    assert (h.total_count, h.null_count, h.distinct_count, h.bucket_count()) == (12, 2, 3, 3)
    assert (h.most_common_ratio(), h.least_common_ratio(), h.null_ratio()) == (0.6, 0.2, 2 / 12)
    assert h.top_n(2) == [("A", 0.6), ("B", 0.2)] and h.get_value_ratio("C") == 0.2 and h.get_value_ratio("Z") is None
    assert h.follows_power_law(2, 0.8) and not h.is_roughly_uniform(1.5)
    assert abs(h.entropy() - float(ex.exact_entropy([6, 2, 2]))) <= ex.tolerance(3, ex.exact_entropy([6, 2, 2]))
    assert h.failure_message("test_col", "most common value appears less than 50%") == (
        "Histogram assertion 'most common value appears less than 50%' failed for column 'test_col'. Distribution: 3 "
        "distinct values, most common ratio: 60.00%, null ratio: 16.67%")


def test_integer_values_are_ordered_by_their_text():
    (summary, counts), s = state_of([10, 9, 9, 10, 100, 100, 2, -3, -3])
    h = Histogram.from_counts(summary, counts)
    assert [b.value for b in h.buckets] == ["-3", "10", "100", "9", "2"] == [t for t, _, _ in ex.buckets(s)]


def test_no_non_null_row_gives_an_empty_histogram():
    (summary, counts), _ = state_of([None, None, None])
    h = Histogram.from_counts(summary, counts)
    assert h.buckets == [] and summary["non_null"] == 0  # ("No data to analyze": the caller skips)
    assert (h.most_common_ratio(), h.entropy(), h.null_ratio(), h.is_roughly_uniform()) == (0.0, 0.0, 1.0, True)
    assert EntropyState.from_counts(summary, counts).is_empty()


def test_beyond_the_bounds_is_an_error_with_the_numbers():
    (summary, counts), _ = state_of([b"a", b"b", b"c", b"long value"], mvb=4)
    with pytest.raises(OutOfBound, match=r"histogram: .* 3 distinct values \(max_distinct 100\), 0 overflow rows, 1 rows longer"):
        Histogram.from_counts(summary, counts, 100)
    (summary, counts), _ = state_of([1, 2, 3])
    with pytest.raises(OutOfBound, match=r"entropy: .* 3 distinct values \(max_distinct 2\)"):
        EntropyState.from_counts(summary, counts, 2)
    with pytest.raises(OutOfBound, match="7 overflow rows"):
        Histogram.from_counts(dict(summary, overflow_rows=7), counts)


def test_entropy_state_metrics_merge_and_tokens():
    (summary, counts), s = state_of([b"A", b"B", b"A", b"C", b"B", b"A", b"D", b"E", b"A", b"F"])
    es = EntropyState.from_counts(summary, counts)
    assert (es.total_count, len(es.value_counts), es.truncated) == (10, 6, False)
    c = list(s["counts"].values())
    m = es.metrics()
    assert abs(m["entropy"] - float(ex.exact_entropy(c, 2))) <= ex.tolerance(6, ex.exact_entropy(c, 2))
    assert abs(m["gini_impurity"] - float(ex.exact_gini(c))) <= ex.tolerance(6, ex.exact_gini(c))
    assert m["effective_values"] == 2.0 ** m["entropy"] and 0.0 <= m["normalized_entropy"] <= 1.0
    assert (m["unique_values"], m["total_count"], m["truncated"]) == (6, 10, False)
    assert list(m["top_values"]) == ["A", "B", "C", "D", "E", "F"] and m["top_values"]["A"] == {"count": 4, "probability": 0.4}
    text = es.to_json()
    assert json.loads(text) == {"value_counts": {"A": 4, "B": 2, "C": 1, "D": 1, "E": 1, "F": 1}, "total_count": 10, "truncated": False}
    assert '"total_count": 10,' in text and '"A": 4' in text  # integers as integer tokens
    back = EntropyState.from_json(text)
    merged = EntropyState.merge([es, back, EntropyState({"Z": 5}, 5, True)])
    assert merged.value_counts["A"] == 8 and merged.value_counts["Z"] == 5 and merged.total_count == 25 and merged.truncated
    with pytest.raises(ValueError, match="integers"):
        EntropyState.from_json('{"value_counts": {"A": 4.0}, "total_count": 4, "truncated": false}')


# ---- HistogramConstraint and EntropyAnalyzer through the host layer (C++, the host ABI, term_amd/suite.py) ------------------
import term_amd.suite as S  # noqa: E402

A, M = S.Assertion, S.HistogramMeasure
GOLDEN = json.load(open(__import__("os").path.join(__import__("os").path.dirname(__file__), "golden", "value_counts_vectors.json")))


def counted(column, **extra):
    """the one VALUE_COUNTS aggregate of a column, as tgx_host_constraint_verdict_json takes it"""
    s = ex.walk([None if v is None else (v.encode() if isinstance(v, str) else v) for v in column])
    entries = {ex.value_text(v): c for v, c in s["counts"].items()}
    return [{"total": s["seen"], "non_null": s["non_null"], "value_counts": dict({"entries": entries}, **extra)}], s


def test_the_constraint_plans_one_value_counts_request():
    c = S.HistogramConstraint("status", [M.most_common_ratio(A.LessThan(0.5))], max_distinct=500)
    assert c.spec == {"type": "histogram", "column": "status", "max_distinct": 500,
                      "measures": [{"measure": "most_common_ratio", "assertion": {"kind": "less_than", "args": [0.5]}}]}
    plan = S.constraint_plan(c.spec)
    assert plan["name"] == "histogram" and len(plan["requests"]) == 1
    assert plan["requests"][0]["kind"] == T.VALUE_COUNTS and plan["requests"][0]["column"] == "status"
    assert plan["requests"][0]["value_counts"] == {"max_distinct": 500, "max_value_bytes": 256}
    assert S.constraint_plan(S.HistogramConstraint("c", [M.entropy(A.GreaterThan(0))]).spec)["requests"][0]["value_counts"]["max_distinct"] == 10000
    built = S.Check.builder("k").has_histogram("status", [M.bucket_count(A.Between(3, 5))]).has_histogram_with_description(
        "status", [M.null_ratio(A.LessThan(0.1))], "few NULLs", max_distinct=7).build()
    assert [c["type"] for c in built.spec["constraints"]] == ["histogram", "histogram"]
    assert built.spec["constraints"][1]["description"] == "few NULLs" and built.spec["constraints"][1]["max_distinct"] == 7
    assert json.loads(json.dumps(built.spec)) == built.spec  # the JSON round trip
    with pytest.raises(T.TgxError, match="unknown histogram measure 'mode'"):
        S.constraint_plan({"type": "histogram", "column": "c", "measures": [{"measure": "mode", "assertion": A.Equals(1).to_json()}]})
    with pytest.raises(T.TgxError, match="at least one measure"):
        S.constraint_plan({"type": "histogram", "column": "c", "measures": []})
    with pytest.raises(T.TgxError, match="Security error|identifier"):
        S.constraint_plan(S.HistogramConstraint("a; DROP TABLE t", [M.entropy(A.GreaterThan(0))]).spec)


def measures_of(check):
    kind, *args = check.get("assertion", ["greater_than", -1])
    a = {"less_than": A.LessThan, "greater_than": A.GreaterThan, "greater_than_or_equal": A.GreaterThanOrEqual,
         "between": A.Between}.get(kind)
    m = check["measure"]
    if kind == "between_exclusive":  # (two measures: a conjunction)
        return [getattr(M, m)(A.GreaterThan(args[0])), getattr(M, m)(A.LessThan(args[1]))]
    if m == "top_n_ratio": return [M.top_n_ratio(check["n"], a(*args))]
    if m == "value_ratio": return [M.value_ratio(check["value"], a(*args))]
    if m == "top_n": return [M.top_n_ratio(1, A.Equals(check["expect_ratios"][0])),
                             M.top_n_ratio(2, A.Equals(check["expect_ratios"][0] + check["expect_ratios"][1]))]
    if m == "is_roughly_uniform": return None
    if m == "any": return [M.bucket_count(A.GreaterThanOrEqual(0))]
    return [getattr(M, m)(a(*args))]


@pytest.mark.parametrize("vec", GOLDEN["histogram_constraints"], ids=lambda v: v["source"].split(":")[-1])
def test_verdicts_on_the_reference_vectors(vec):
    results, s = counted(vec["column"])
    for check in vec["checks"]:
        measures = measures_of(check)
        if measures is None:
            continue  # (is_roughly_uniform is no named measure: the C++ function form takes it)
        v = S.constraint_verdict(S.HistogramConstraint("test_col", measures).spec, results)
        assert v["status"] == check["status"] and v["name"] == "histogram"
        if check["status"] == "skipped":
            assert v["message"] == "No data to analyze" and v["metric"] is None
        else:
            exact = ex.exact_entropy(list(s["counts"].values()))
            assert abs(v["metric"] - float(exact)) <= ex.tolerance(s["distinct"], exact)  # entropy in nats
        if check.get("has_message"):
            assert v["message"] == ("Histogram assertion 'most_common_ratio less than 0.5' failed for column 'test_col'. "
                                    "Distribution: 3 distinct values, most common ratio: 60.00%, null ratio: 0.00%")


def test_the_failure_message_and_the_description():
    results, _ = counted(["A"] * 6 + ["B"] * 2 + ["C"] * 2 + [None] * 2)
    c = S.HistogramConstraint("test_col", [M.most_common_ratio(A.LessThan(0.5))], "most common value appears less than 50%")
    v = S.constraint_verdict(c.spec, results)
    assert v["status"] == "failure" and v["message"] == (
        "Histogram assertion 'most common value appears less than 50%' failed for column 'test_col'. Distribution: 3 "
        "distinct values, most common ratio: 60.00%, null ratio: 16.67%")
    both = S.HistogramConstraint("test_col", [M.top_n_ratio(2, A.GreaterThanOrEqual(0.8)), M.value_ratio("Z", A.Equals(0.0)),
                                              M.least_common_ratio(A.Equals(0.2)), M.null_ratio(A.Between(0.16, 0.17))])
    assert S.constraint_verdict(both.spec, results)["status"] == "success"
    one_fails = S.HistogramConstraint("test_col", [M.bucket_count(A.Equals(3)), M.value_ratio("A", A.LessThan(0.6))])
    v = S.constraint_verdict(one_fails.spec, results)
    assert v["status"] == "failure" and "'bucket_count equals 3 and value_ratio('A') less than 0.6'" in v["message"]


def test_integer_values_order_by_their_text_in_the_host_layer():
    results, _ = counted([10, 9, 9, 10, 100, 100, 2])  # buckets: "10", "100", "9", then "2"
    ok = S.HistogramConstraint("n", [M.top_n_ratio(3, A.Equals(6 / 7)), M.value_ratio("100", A.Equals(2 / 7))])
    assert S.constraint_verdict(ok.spec, results)["status"] == "success"


def test_beyond_the_bounds_and_unsupported_types_are_the_constraints_error():
    c = S.HistogramConstraint("c", [M.bucket_count(A.GreaterThan(0))], max_distinct=2)
    results, _ = counted(["a", "b", "c"])
    with pytest.raises(T.TgxError, match=r"'histogram': .*3 distinct values \(max_distinct 2\), 0 overflow rows, 0 rows longer"):
        S.constraint_verdict(c.spec, results)
    wide = S.HistogramConstraint("c", [M.bucket_count(A.GreaterThan(0))])
    for extra, text in (({"overflow_rows": 4}, "4 overflow rows"), ({"long_rows": 2}, "2 rows longer than 256 bytes")):
        with pytest.raises(T.TgxError, match="'histogram': .*" + text):
            S.constraint_verdict(wide.spec, counted(["a", "b"], **extra)[0])
    for arrow_type in ("Date32", "Date64", "Time64(Nanosecond)", "time32[s]", "Timestamp(Nanosecond, None)", "duration[ns]",
                       "Float32", "Float64", "decimal128(10, 2)", "Boolean", "Binary"):
        with pytest.raises(T.TgxError, match="'histogram': .*%s.*not on the GPU path" % __import__("re").escape(arrow_type)):
            S.constraint_verdict(dict(wide.spec, column_type=arrow_type), results)
    for arrow_type in ("Int64", "Int8", "UInt32", "Utf8", "LargeUtf8", "Utf8View"):
        assert S.constraint_verdict(dict(wide.spec, column_type=arrow_type), results)["status"] == "success"


def test_the_entropy_analyzer_and_its_tag():
    e = S.EntropyAnalyzer("category")
    assert e.spec == {"type": "value_entropy", "column": "category", "max_unique_values": 10000}
    assert e.name() == "entropy" and e.metric_key() == "entropy.category"
    assert S.EntropyAnalyzer("c", 3).spec["max_unique_values"] == 10  # (with_max_unique_values: at least 10)
    for unknown in ("entropy", "value_counts"):  # the tag "entropy" stays unknown
        with pytest.raises(T.TgxError, match="unknown analyzer type '%s'" % unknown):
            S._Analyzer({"type": unknown, "column": "c"}).merge_states([{}])
    vec = GOLDEN["entropy_analyzer"][0]
    s = ex.walk([v.encode() for v in vec["column"]])
    state = {"value_counts": {ex.value_text(v): c for v, c in s["counts"].items()}, "total_count": s["counted"], "truncated": False}
    m = e.compute_metric_from_state(state)
    assert m["type"] == "Map"
    v = {k: x["value"] for k, x in m["value"].items()}
    c = list(s["counts"].values())
    assert abs(v["entropy"] - float(ex.exact_entropy(c, 2))) <= ex.tolerance(6, ex.exact_entropy(c, 2))
    assert abs(v["gini_impurity"] - float(ex.exact_gini(c))) <= ex.tolerance(6, ex.exact_gini(c))
    assert v["effective_values"] == 2.0 ** v["entropy"] and v["normalized_entropy"] == v["entropy"] / __import__("math").log2(6)
    assert (v["unique_values"], v["total_count"], v["truncated"]) == (6, 10, False)
    assert [m["value"][k]["type"] for k in ("unique_values", "total_count", "truncated")] == ["Long", "Long", "Boolean"]
    top = v["top_values"]
    assert list(top) == ["A", "B", "C", "D", "E", "F"]
    assert top["A"] == {"type": "Map", "value": {"count": {"type": "Long", "value": 4},
                                                      "probability": {"type": "Double", "value": 0.4}}}
    uniform = {"value_counts": {k: 2 for k in "ABCDE"}, "total_count": 10, "truncated": False}  # tests.rs:276-314
    u = {k: x["value"] for k, x in e.compute_metric_from_state(uniform)["value"].items()}
    assert abs(u["entropy"] - __import__("math").log2(5)) < 0.001 and abs(u["normalized_entropy"] - 1.0) < 0.001
    empty = {"value_counts": {}, "total_count": 0, "truncated": False}
    z = {k: x["value"] for k, x in e.compute_metric_from_state(empty)["value"].items()}
    assert (z["entropy"], z["normalized_entropy"], z["gini_impurity"], z["unique_values"]) == (0.0, 0.0, 0.0, 0)
    many = {"value_counts": {"v%03d" % i: 1 for i in range(101)}, "total_count": 101, "truncated": False}
    assert "top_values" not in e.compute_metric_from_state(many)["value"]


def test_the_entropy_state_merges_and_keeps_integer_tokens():
    e = S.EntropyAnalyzer("c")
    a = {"value_counts": {"x": 3, "y": 1}, "total_count": 4, "truncated": False}
    b = {"value_counts": {"y": 2, "z": 2 ** 60}, "total_count": 2 + 2 ** 60, "truncated": True}
    text = e.merge_states_text([a, b])
    assert text == '{"value_counts": {"x": 3, "y": 3, "z": 1152921504606846976}, "total_count": 1152921504606846982, "truncated": true}'
    assert e.merge_states([a, a]) == {"value_counts": {"x": 6, "y": 2}, "total_count": 8, "truncated": False}
    assert e.merge_states([]) == {"value_counts": {}, "total_count": 0, "truncated": False}
