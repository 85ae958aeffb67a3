"""TGX_CHECK_VALUE_RULE and DataTypeConstraint without a device: plan validation, the counts a host-only state answers
from a blob, the blob's section (term_amd/wire.py), the constraint's constructors, descriptions, device parameters and
verdicts (C++ through the host ABI, and the Python twins), held against tests/exact_value_rule.py."""
import json
import math

import pytest

import exact_value_rule as ev
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

N, D, V = S.NumericValidation, S.DataTypeConstraint, S.DataTypeValidation


def rule_plan(hi=100):
    plan = T.Plan([spec(T.VALUE_RULE, 0), spec(T.VALUE_RULE, 0), spec(T.VALUE_RULE, 1), spec(T.COUNT, 0)])
    plan.set_value_rule(0, T.RULE_GE_ZERO)
    plan.set_value_rule(1, T.RULE_BETWEEN, lo_i=-5, hi_i=hi, lo_f=-5.0, hi_f=float(hi))
    plan.set_value_rule(2, T.RULE_INTEGER)
    return plan


def rule_blob(hi=100):
    return wire.pack(count=[wire.count_acc(10, 9)], value_rules=[
        wire.value_rule_state(1, 0, 10, 9, 7), wire.value_rule_state(3, 0, 10, 9, 4, lo_i=-5, hi_i=hi, lo_f=-5.0, hi_f=float(hi)),
        wire.value_rule_state(4, 0, 10, 8, 5, 2)])


def test_abi_constants():
    assert T.VALUE_RULE == 14
    assert (T.RULE_GE_ZERO, T.RULE_GT_ZERO, T.RULE_BETWEEN, T.RULE_INTEGER) == (ev.GE_ZERO, ev.GT_ZERO, ev.BETWEEN, ev.INTEGER) == (1, 2, 3, 4)
    assert T.RULE_BOUNDS_AS_DOUBLE == ev.BOUNDS_AS_DOUBLE == 1
    assert T.lib().tgx_abi_version() == 6
    for name in ("tgx_plan_set_value_rule", "tgx_value_rule_get", "tgx_host_value_rule_params_json"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)


def test_parameters_are_validated():
    plan = T.Plan([spec(T.VALUE_RULE, 0), spec(T.COUNT, 0)])
    for mode in (0, 5, -1):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*unknown VALUE_RULE mode"):
            plan.set_value_rule(0, mode)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*unknown VALUE_RULE flags"):
        plan.set_value_rule(0, T.RULE_BETWEEN, flags=2)
    for mode in (T.RULE_GE_ZERO, T.RULE_GT_ZERO, T.RULE_INTEGER):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*BOUNDS_AS_DOUBLE"):
            plan.set_value_rule(0, mode, flags=T.RULE_BOUNDS_AS_DOUBLE)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a VALUE_RULE check"):
        plan.set_value_rule(1, T.RULE_GE_ZERO)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*column2 must be -1"):
        T.Plan([spec(T.VALUE_RULE, 0, column2=1)])
    plan.set_value_rule(0, T.RULE_BETWEEN, lo_i=5, hi_i=1)  # lo > hi is allowed
    plan.set_value_rule(0, T.RULE_BETWEEN, flags=T.RULE_BOUNDS_AS_DOUBLE, lo_f=float("nan"), hi_f=float("inf"))


def test_a_spec_without_parameters_fails_state_create_and_deserialize():
    plan = T.Plan([spec(T.VALUE_RULE, 0), spec(T.VALUE_RULE, 0)])
    plan.set_value_rule(0, T.RULE_GE_ZERO)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*tgx_plan_set_value_rule"):
        T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_plan_set_value_rule"):
        T.State.deserialize(plan, wire.pack(value_rules=[wire.value_rule_state(1, 0, 3, 2, 1)] * 2))


def test_setter_is_refused_after_the_first_state():
    plan = rule_plan()
    st = T.State.deserialize(plan, rule_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_value_rule(0, T.RULE_GT_ZERO)
    del st


def test_counts_of_a_host_only_state_and_its_result():
    plan = rule_plan()
    st = T.State.deserialize(plan, rule_blob())
    assert [st.value_rule_counts(i) for i in range(3)] == [(10, 9, 7, 0), (10, 9, 4, 0), (10, 8, 5, 2)]
    res = st.finalize()
    assert [(r.total, r.non_null, r.matches, r.distinct) for r in res[:3]] == [(10, 9, 7, 0), (10, 9, 4, 0), (10, 8, 5, 2)]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a VALUE_RULE check"):
        st.value_rule_counts(3)


def test_blob_round_trip_and_merge_through_a_host_only_state():
    plan = rule_plan()
    blob = rule_blob()
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    st.merge([T.State.deserialize(plan, blob), T.State.deserialize(plan, blob)])
    assert [st.value_rule_counts(i) for i in range(3)] == [(30, 27, 21, 0), (30, 27, 12, 0), (30, 24, 15, 6)]
    st.reset()
    assert [st.value_rule_counts(i) for i in range(3)] == [(0, 0, 0, 0)] * 3


def test_malformed_and_foreign_blobs_are_refused():
    plan = rule_plan()
    blob = rule_blob()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):  # counted under other bounds
        T.State.deserialize(rule_plan(hi=101), blob)
    for cut in (1, 8, 40, 72):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    bad = wire.pack(count=[wire.count_acc(10, 9)], value_rules=[
        wire.value_rule_state(1, 0, 10, 11, 7), wire.value_rule_state(3, 0, 10, 9, 4, lo_i=-5, hi_i=100, lo_f=-5.0, hi_f=100.0),
        wire.value_rule_state(4, 0, 10, 8, 5, 2)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed"):
        T.State.deserialize(plan, bad)
    bad = wire.pack(count=[wire.count_acc(10, 9)], value_rules=[
        wire.value_rule_state(1, 0, 10, 9, 7), wire.value_rule_state(3, 0, 10, 9, 4, lo_i=-5, hi_i=100, lo_f=-5.0, hi_f=100.0),
        wire.value_rule_state(4, 0, 10, 8, 5, 4)])  # valid + cast errors above considered
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed"):
        T.State.deserialize(plan, bad)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):  # a plan whose section has other tasks
        other = T.Plan([spec(T.VALUE_RULE, 0), spec(T.COUNT, 0)])
        other.set_value_rule(0, T.RULE_GE_ZERO)
        T.State.deserialize(other, blob)


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0)])
    blob = wire.pack(count=[wire.count_acc(10, 9)])
    assert T.State.deserialize(plan, blob).serialize() == blob


# ---- the constraint ---------------------------------------------------------------------------------------------------
def test_constructors_and_their_errors():
    assert D.non_negative("amount").spec == {"type": "datatype", "column": "amount", "validation": "numeric", "numeric": "non_negative"}
    assert D.type_consistency("c", 0.95).spec["threshold"] == 0.95 and D.specific_type("c", "Int64").spec["data_type"] == "Int64"
    for t in (-0.1, 1.1, float("nan")):
        with pytest.raises(T.TgxError, match="Configuration error: Threshold must be between 0.0 and 1.0"):
            D.type_consistency("c", t)
        with pytest.raises(T.TgxError, match="Configuration error: Threshold must be between 0.0 and 1.0"):  # C++
            S.constraint_plan({"type": "datatype", "column": "c", "validation": "consistency", "threshold": t if t == t else 2.0})
    D.type_consistency("c", 0.0), D.type_consistency("c", 1.0)
    for bad in ("", "a b", "x; DROP TABLE t"):
        with pytest.raises(T.TgxError):
            D.non_negative(bad)
        with pytest.raises(T.TgxError):
            S.constraint_plan({"type": "datatype", "column": bad, "validation": "numeric", "numeric": "positive"})
    b = S.Check.builder("c").has_consistent_data_type("col", 0.9).build()
    assert b.spec["constraints"][-1] == D.type_consistency("col", 0.9).spec
    with pytest.raises(T.TgxError, match="Threshold"):
        S.Check.builder("c").has_consistent_data_type("col", 1.5)


def verdict(constraint, results, **extra):
    return S.constraint_verdict(dict(constraint.spec, **extra), results)


def counts(considered, valid, errors=0, seen=None):
    return [{"total": considered if seen is None else seen, "non_null": considered, "matches": valid, "distinct": errors}]


DESCRIBED = [(V.Numeric(N.NonNegative), "non-negative values"), (V.Numeric(N.Positive), "positive values"),
             (V.Numeric(N.Integer), "integer values"), (V.Numeric(N.Range(0.0, 100.0)), "values between 0 and 100"),
             (V.Numeric(N.Range(-0.0, 2.5)), "values between -0 and 2.5"),
             (V.Numeric(N.Range(1e-7, 2.0 ** 53)), "values between 0.0000001 and 9007199254740992")]


@pytest.mark.parametrize("validation,text", DESCRIBED, ids=[d[1] for d in DESCRIBED])
def test_descriptions_in_the_verdict_text(validation, text):
    """datatype.rs:95-128: the description is what the message ends with (Rust's `{}` for the bounds)"""
    c = D("col", validation)
    got = verdict(c, counts(8, 6))
    assert got == {"status": "failure", "metric": 0.75, "message": "75.0% of values satisfy " + text, "name": "datatype"}
    if validation["numeric"] == "range":
        assert text == ev.description("range", min=validation["min"], max=validation["max"])


def test_plan_of_a_numeric_validation():
    plan = S.constraint_plan(D.non_negative("amount").spec)
    assert plan["name"] == "datatype" and len(plan["requests"]) == 1
    r = plan["requests"][0]
    assert (r["kind"], r["column"], r["column2"]) == (T.VALUE_RULE, "amount", "")
    assert r["value_rule"] == {"mode": 1, "flags": 0, "lo_i": 0, "hi_i": 0, "lo_f": 0, "hi_f": 0}
    for c in (D.specific_type("amount", "Int64"), D.type_consistency("amount", 0.5)):  # no scan but the one for the column
        (r,) = S.constraint_plan(c.spec)["requests"]
        assert (r["kind"], r["column"]) == (T.COUNT, "amount") and "value_rule" not in r


def params_of(c):
    p = S.value_rule_params(c.spec)
    assert p.pop("column") == c.spec["column"] and p.pop("kind") == T.VALUE_RULE
    return p


def test_value_rule_params():
    assert params_of(D.non_negative("c")) == ev.rule(ev.GE_ZERO)
    assert params_of(D("c", V.Numeric(N.Positive))) == ev.rule(ev.GT_ZERO)
    assert params_of(D("c", V.Numeric(N.Integer))) == ev.rule(ev.INTEGER)
    for lo, hi in ((0.0, 100.0), (-2.0 ** 53, 2.0 ** 53), (-0.0, 7.0), (0.5, 100.0), (0.0, 99.5), (0.25, 0.75), (5.0, -5.0),
                   (-1e15 / 3, 1e15 / 7), (5e-324, 0.1)):
        assert params_of(D("c", V.Numeric(N.Range(lo, hi)))) == ev.range_params(lo, hi), (lo, hi)
    # bound classification: 2^53 is the last integral bound that is an Int64 literal
    p = params_of(D("c", V.Numeric(N.Range(2.0 ** 53, 2.0 ** 53))))
    assert (p["flags"], p["lo_i"], p["hi_i"]) == (0, 2**53, 2**53)
    p = params_of(D("c", V.Numeric(N.Range(-0.0, 1.0))))  # -0.0 prints "-0" and is 0
    assert (p["flags"], p["lo_i"], math.copysign(1.0, p["lo_f"])) == (0, 0, 1.0)
    # one integral and one fractional bound: the comparison is a double one
    p = params_of(D("c", V.Numeric(N.Range(1.0, 2.5))))
    assert (p["flags"], p["lo_f"], p["hi_f"]) == (T.RULE_BOUNDS_AS_DOUBLE, 1.0, 2.5)
    p = params_of(D("c", V.Numeric(N.Range(0.5, 3.0))))
    assert (p["flags"], p["lo_f"], p["hi_f"]) == (T.RULE_BOUNDS_AS_DOUBLE, 0.5, 3.0)
    prefix = "Constraint evaluation failed for 'datatype': "
    for lo, hi, what in ((2.0 ** 53 + 2, 2.0 ** 60, "beyond 2\\^53.*minimum is 9007199254740994"), (0.0, 1e300, "beyond 2\\^53.*maximum is 1000"),
                         (0.0, float("inf"), "not a SQL literal.*maximum is inf"), (-float("inf"), 0.0, "not a SQL literal.*minimum is -inf"),
                         (float("nan"), 1.0, "not a SQL literal.*minimum is NaN"), (0.0, float("nan"), "not a SQL literal.*maximum is NaN")):
        assert ev.range_params(lo, hi) is None
        with pytest.raises(T.TgxError, match=prefix + ".*not on the GPU path.*" + what.split(".*")[1]) as e:
            S.value_rule_params(D("c", V.Numeric(N.Range(lo, hi))).spec)
        assert __import__("re").search(what, str(e.value))
    with pytest.raises(T.TgxError, match="not a numeric datatype constraint"):
        S.value_rule_params(D.specific_type("c", "Int64").spec)


def test_the_verdict_from_given_counters():
    c = D.non_negative("amount")
    assert verdict(c, counts(4, 4, seen=5)) == {"status": "success", "metric": 1.0, "name": "datatype",
                                                "message": "100.0% of values satisfy non-negative values"}
    n = 10**7
    got = verdict(c, counts(n, n - 1))  # just below 1.0: a Failure, though it prints as 100.0%
    assert got["status"] == "failure" and got["metric"] == (n - 1) / n < 1.0
    assert got["message"] == "100.0% of values satisfy non-negative values"
    assert (got["status"].capitalize(), got["metric"], got["message"]) == ev.verdict(n, n - 1, "non-negative values")
    got = verdict(c, counts(0, 0, seen=3))  # no non-NULL row: 0 / 0
    assert got == {"status": "failure", "metric": None, "message": "NaN% of values satisfy non-negative values", "name": "datatype"}
    for considered, valid in ((3, 1), (3, 2), (7, 0), (1000, 995)):
        got = verdict(c, counts(considered, valid))
        assert (got["status"].capitalize(), got["metric"], got["message"]) == ev.verdict(considered, valid, "non-negative values")
    # cast errors: the constraint's error, with the count
    with pytest.raises(T.TgxError, match="Constraint evaluation failed for 'datatype': 2 rows do not fit Int32: the reference's query fails"):
        verdict(D("amount", V.Numeric(N.Integer)), counts(10, 8, 2))
    assert verdict(D("amount", V.Numeric(N.Integer)), counts(10, 10))["status"] == "success"


def test_specific_type_and_consistency_verdicts():
    c = D.specific_type("user_id", "Int64")
    assert verdict(c, counts(5, 5), column_type="Int64") == {"status": "success", "metric": 1.0, "name": "datatype",
                                                            "message": "Column 'user_id' has expected type Int64"}
    assert verdict(c, counts(5, 5), column_type="Utf8") == {"status": "failure", "metric": 0.0, "name": "datatype",
                                                           "message": "Column 'user_id' has type Utf8, expected Int64"}
    ts = D.specific_type("at", "Timestamp(Nanosecond, None)")
    assert verdict(ts, counts(1, 1), column_type="Timestamp(Nanosecond, None)")["status"] == "success"
    with pytest.raises(T.TgxError, match="'datatype': the Arrow type of column 'user_id' is not known"):
        verdict(c, counts(5, 5))
    ok = verdict(D.type_consistency("c", 0.95), counts(5, 5))
    assert ok == {"status": "success", "metric": 0.95, "name": "datatype", "message": "Type consistency 95.0% meets threshold 95.0%"}
    low = verdict(D.type_consistency("c", 0.951), counts(0, 0))
    assert low == {"status": "failure", "metric": 0.95, "name": "datatype", "message": "Type consistency 95.0% below threshold 95.1%"}


OFF_DEVICE = [V.Numeric(N.Finite), V.String(S.StringTypeValidation.NotEmpty), V.String(S.StringTypeValidation.ValidUtf8),
              V.String(S.StringTypeValidation.NotBlank), V.String(S.StringTypeValidation.MaxBytes(10)),
              V.Temporal(S.TemporalValidation.PastDate), V.Temporal(S.TemporalValidation.FutureDate),
              V.Temporal(S.TemporalValidation.DateRange("2020-01-01", "2021-01-01")),
              V.Temporal(S.TemporalValidation.ValidTimezone), V.Custom("{column} % 2 = 0")]


@pytest.mark.parametrize("validation", OFF_DEVICE, ids=[json.dumps(v, sort_keys=True)[:40] for v in OFF_DEVICE])
def test_what_stays_off_the_device_is_the_constraints_error(validation):
    c = D("col", validation)
    for call in (lambda: S.constraint_plan(c.spec), lambda: verdict(c, counts(1, 1)), lambda: S.value_rule_params(c.spec)):
        with pytest.raises(T.TgxError, match="Constraint evaluation failed for 'datatype': .*not on the GPU path"):
            call()


def test_json_round_trip():
    """every validation through the suite's JSON form: what the C++ side builds answers like what Python described"""
    suite = S.ValidationSuite.builder("s").check(
        S.Check.builder("c").constraint(D.non_negative("a")).constraint(D("a", V.Numeric(N.Range(0.5, float("inf")))))
        .constraint(D.specific_type("a", "Float64")).has_consistent_data_type("a", 0.5).build()).build()
    text = json.dumps(suite.spec)
    assert json.loads(text) == suite.spec and '"max": "inf"' in text
    for c in suite.spec["checks"][0]["constraints"]:
        assert c["type"] == "datatype"
    res = suite.run(None)  # no table registered: every constraint reports the planner's error, none a JSON one
    assert len(res.report.issues) == 4 and all("not found" in i.message for i in res.report.issues)
