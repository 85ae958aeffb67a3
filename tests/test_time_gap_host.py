"""TGX_CHECK_TIME_GAP without a device: the opt-in of the host layer (host/temporal.cpp, window_on_device), its
seconds -> ticks rules and verdicts, and the plan-side ABI (tgx_plan_set_time_gap, tgx_state_create)."""
import pytest

import exact_time_gap as eg
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec

PREFIX = "Constraint evaluation failed for 'temporal_ordering': "
UNITS = {"s": "Second", "ms": "Millisecond", "us": "Microsecond", "ns": "Nanosecond"}


def ts_type(unit, tz="None"):
    return "Timestamp(%s, %s)" % (UNITS[unit], tz)


def gap(column="ts", seconds=60, group=None, on=True):
    c = S.TemporalOrderingConstraint("events").max_time_gap(column, seconds)
    if group is not None:
        c = c.group_by(group)
    return c.window_on_device(on) if on is not None else c


def counted(seen, gaps, violations):
    return [{"total": seen, "non_null": gaps, "matches": gaps - violations}]


# ---- the opt-in ---------------------------------------------------------------------------------------------------------
def test_without_the_opt_in_the_plan_error_is_todays():
    want = ("TGX_INVALID_ARGUMENT: " + PREFIX +
            "MaxTimeGap validation is a LAG() OVER (ORDER BY ..) window query and is not on the GPU path")
    for c in (gap(on=None), gap(on=False), gap(group="g", on=None), gap(group="g", on=False),
              gap(on=True).window_on_device(False)):
        with pytest.raises(T.TgxError) as e:
            S.constraint_plan(c.spec)
        assert str(e.value) == want
        with pytest.raises(T.TgxError) as e:
            S.temporal_params(c.spec, {"ts": ts_type("ns"), "g": "Int64"})
        assert str(e.value) == want
    assert "window_on_device" not in gap(on=None).spec
    # max_time_gap called again starts from the default; the call acts on MaxTimeGap only, as weekdays_only does
    assert "window_on_device" not in gap(on=True).max_time_gap("ts", 5).spec
    other = S.TemporalOrderingConstraint("t").before_after("a", "b").window_on_device(True)
    assert "window_on_device" not in other.spec
    assert S.constraint_plan(other.spec)["requests"][0]["kind"] == T.TEMPORAL
    # ... and in the JSON: the key beside another validation changes nothing
    hours = dict(S.TemporalOrderingConstraint("t").business_hours("a", "09:00", "17:00").spec, window_on_device=True)
    assert S.constraint_plan(hours)["requests"][0]["kind"] == T.TEMPORAL


def test_the_planned_spec():
    assert T.TIME_GAP == 13
    plan = S.constraint_plan(gap("ts", 90).spec)
    (req,) = plan["requests"]
    assert plan["name"] == "temporal_ordering"
    assert (req["kind"], req["column"], req["column2"], req["flags"]) == (T.TIME_GAP, "ts", "", 0)
    assert req["temporal"]["max_gap_seconds"] == 90
    (req,) = S.constraint_plan(gap("ts", -3, group="sensor").spec)["requests"]
    assert (req["kind"], req["column"], req["column2"]) == (T.TIME_GAP, "ts", "sensor")
    assert req["temporal"]["max_gap_seconds"] == -3
    # allow_nulls is not read in this mode: the same request either way but for the stored flag
    a = S.temporal_params(gap().allow_nulls(True).spec, {"ts": ts_type("s")})
    assert a == S.temporal_params(gap().spec, {"ts": ts_type("s")})


@pytest.mark.parametrize("unit", ["s", "ms", "us", "ns"])
def test_seconds_become_ticks(unit):
    for seconds in (0, 1, 60, -1, 86400 * 365, eg.I64_MAX // eg.TICKS[unit], eg.I64_MIN // eg.TICKS[unit] + 1):
        p = S.temporal_params(gap("ts", seconds, group="g").spec, {"ts": ts_type(unit), "g": "Int32"})
        assert p == {"column": "ts", "column2": "g", "kind": T.TIME_GAP, "max_gap": eg.max_gap_ticks(seconds, unit),
                     "flags": 0}
        assert p["max_gap"] == seconds * eg.TICKS[unit]


@pytest.mark.parametrize("unit", ["ms", "us", "ns"])
def test_overflow_is_the_constraints_error(unit):
    for seconds in (eg.I64_MAX // eg.TICKS[unit] + 1, eg.I64_MAX, eg.I64_MIN // eg.TICKS[unit] - 1, eg.I64_MIN):
        assert eg.max_gap_ticks(seconds, unit) is None
        with pytest.raises(T.TgxError, match=PREFIX + "Temporal validation query failed: the maximum gap overflows"):
            S.temporal_params(gap("ts", seconds).spec, {"ts": ts_type(unit)})


def test_any_time_zone_is_accepted():
    for tz in ("None", 'Some("UTC")', 'Some("+00:00")', 'Some("Europe/Paris")', 'Some("-08:00")'):
        assert S.temporal_params(gap("ts", 2).spec, {"ts": ts_type("us", tz)})["max_gap"] == 2 * 10**6


def test_column_type_errors():
    for t in ("Date64", "Int64", "Date32", "Utf8", "Float64"):
        with pytest.raises(T.TgxError, match=PREFIX + "max time gap validation on the device needs a Timestamp.*the "
                                                      "column is " + t + r" \(not on the GPU path\)"):
            S.temporal_params(gap().spec, {"ts": t})
    with pytest.raises(T.TgxError, match=PREFIX + "max time gap validation on the device needs a Timestamp.*an unknown type"):
        S.temporal_params(gap().spec, {})
    for t in ("Utf8", "LargeUtf8", "Float64", "UInt64", "Boolean", "Binary", "Float32"):
        with pytest.raises(T.TgxError, match=PREFIX + "max time gap validation on the device needs a group column.*the "
                                                      "column is " + t + r" \(not on the GPU path\)"):
            S.temporal_params(gap(group="g").spec, {"ts": ts_type("ns"), "g": t})
    for t in ("Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "Date32", "Date64", ts_type("ms")):
        assert S.temporal_params(gap(group="g").spec, {"ts": ts_type("ns"), "g": t})["column2"] == "g"
    # a group column whose type the caller does not know: the device decides
    assert S.temporal_params(gap(group="g").spec, {"ts": ts_type("ns")})["column2"] == "g"


def test_identifiers_of_both_columns_are_validated():
    for c in (gap("ts; drop", 1), gap("ts", 1, group="g; drop"), gap("", 1), gap("ts", 1, group="")):
        with pytest.raises(T.TgxError, match="Security error"):
            S.constraint_plan(c.spec)
    bad_table = S.TemporalOrderingConstraint("bad table;").max_time_gap("ts", 1).window_on_device(True)
    with pytest.raises(T.TgxError, match="Security error"):
        S.constraint_plan(bad_table.spec)


def test_the_three_verdicts():
    c = gap(group="g")
    for seen, gaps, violations in ((10, 7, 0), (10, 0, 0), (0, 0, 0), (10, 7, 7), (10, 3, 1), (30000, 20000, 1)):
        got = S.constraint_verdict(c.spec, counted(seen, gaps, violations))
        status, metric, message = eg.verdict(gaps, violations)
        assert (got["status"], got["metric"], got["message"], got["name"]) == \
            (status.lower(), metric, message, "temporal_ordering")
    none = S.constraint_verdict(c.spec, counted(5, 0, 0))  # no gaps at all
    assert none == {"status": "success", "metric": 1.0, "message": None, "name": "temporal_ordering"}
    third = S.constraint_verdict(c.spec, counted(4, 3, 1))
    assert third["status"] == "failure" and third["metric"] == 2 / 3
    assert third["message"] == "Time gap violation: 1 gaps exceed maximum allowed (66.67% compliance)"
    allv = S.constraint_verdict(c.spec, counted(4, 3, 3))
    assert allv["message"] == "Time gap violation: 3 gaps exceed maximum allowed (0.00% compliance)"
    near = S.constraint_verdict(c.spec, counted(20001, 20000, 1))
    assert near["message"].endswith("(%.2f%% compliance)" % (19999 / 20000 * 100.0))


# ---- the plan side of the C ABI -------------------------------------------------------------------------------------------
def test_a_spec_without_its_threshold_fails_state_create():
    plan = T.Plan([spec(T.COUNT, 0), spec(T.TIME_GAP, 0, column2=-1), spec(T.TIME_GAP, 0, column2=-1),
                   spec(T.TIME_GAP, 0, column2=1)])
    plan.set_time_gap(1, 5)
    plan.set_time_gap(3, 5)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 2.*tgx_plan_set_time_gap"):
        T.State(plan)
    plan.set_time_gap(2, -1)  # (the failed create has not locked the plan)
    T.State(plan).close()


def test_the_setter_is_refused_on_other_kinds_and_after_the_first_state():
    plan = T.Plan([spec(T.TIME_GAP, 0, column2=-1), spec(T.TEMPORAL, 0), spec(T.COUNT, 0)])
    plan.set_temporal(1, T.TEMPORAL_RANGE, lo=0)
    for other in (1, 2, 3):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a TIME_GAP"):
            plan.set_time_gap(other, 1)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a TEMPORAL"):
        plan.set_temporal(0, T.TEMPORAL_RANGE)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*unknown TIME_GAP flags"):
        plan.set_time_gap(0, 1, flags=1)
    plan.set_time_gap(0, eg.I64_MAX)
    plan.set_time_gap(0, eg.I64_MIN)  # (may be set again until a state exists)
    st = T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*once a state"):
        plan.set_time_gap(0, 1)
    st.close()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*column2 is the group column or -1"):
        T.Plan([spec(T.TIME_GAP, 0, column2=-2)])


def test_a_state_that_saw_nothing_answers_zeros_and_combines():
    """no device is touched: nothing was retained, so reading, merging and serializing all pass"""
    plan = T.Plan([spec(T.TIME_GAP, 0, column2=1), spec(T.COUNT, 0)])
    plan.set_time_gap(0, 3)
    a, b = T.State(plan), T.State(plan)
    assert a.time_gap_counts(0) == (0, 0, 0, 0, 0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a TIME_GAP"):
        a.time_gap_counts(1)
    blob = a.serialize()
    plain = T.Plan([spec(T.COUNT, 0)])
    assert blob == T.State(plain).serialize()  # the kind adds no section: blobs of other plans keep their bytes
    a.merge([b])
    r = T.State.deserialize(plan, blob).finalize()
    assert (r[0].total, r[0].non_null, r[0].matches) == (0, 0, 0)
