"""TGX_CHECK_TEMPORAL without a device: plan validation, the counts a host-only state answers from a blob, the blob's
section (term_amd/wire.py) and that blobs of plans without the kind keep their bytes."""
import pytest

import exact_temporal as et
import term_amd as T
from _lib_spec import spec
from term_amd import wire

I64_MIN, I64_MAX = et.I64_MIN, et.I64_MAX
TOD = dict(ticks_per_second=1000, tod_lo=9 * 3600 * 1000, tod_hi=17 * 3600 * 1000)


def three_plan(keep=0, weekdays=0):
    plan = T.Plan([spec(T.TEMPORAL, 0, column2=1), spec(T.TEMPORAL, 0), spec(T.TEMPORAL, 1), spec(T.COUNT, 0)])
    plan.set_temporal(0, T.TEMPORAL_ORDER, flags=keep, delta=5)
    plan.set_temporal(1, T.TEMPORAL_TIME_OF_DAY, flags=keep | weekdays, **TOD)
    plan.set_temporal(2, T.TEMPORAL_RANGE, flags=keep, lo=10)
    return plan


def three_blob(keep=0, weekdays=0):
    return wire.pack(count=[wire.count_acc(10, 9)], temporal=[
        wire.temporal_state(1, keep, 10, 8, 5, delta=5),
        wire.temporal_state(2, keep | weekdays, 10, 6, 4, ticks_per_second=1000, lo=TOD["tod_lo"], hi=TOD["tod_hi"]),
        wire.temporal_state(3, keep, 10, 9, 9, lo=10, hi=I64_MAX)])


def test_abi_constants():
    assert (T.TEMPORAL, T.TEMPORAL_ORDER, T.TEMPORAL_TIME_OF_DAY, T.TEMPORAL_RANGE) == (11, 1, 2, 3)
    assert (T.TEMPORAL_KEEP_NULLS, T.TEMPORAL_WEEKDAYS_ONLY) == (et.KEEP_NULLS, et.WEEKDAYS_ONLY) == (1, 2)
    assert T.lib().tgx_abi_version() == 6


def test_parameters_are_validated():
    plan = T.Plan([spec(T.TEMPORAL, 0, column2=1), spec(T.TEMPORAL, 0)])
    for tps in (0, -1, 2, 60, 10**4, 10**12):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*ticks_per_second"):
            plan.set_temporal(1, T.TEMPORAL_TIME_OF_DAY, ticks_per_second=tps)
    for tps in (1, 10**3, 10**6, 10**9):
        plan.set_temporal(1, T.TEMPORAL_TIME_OF_DAY, ticks_per_second=tps, tod_lo=0, tod_hi=tps)
    for mode in (0, 4, -1):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*unknown TEMPORAL mode"):
            plan.set_temporal(1, mode)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*unknown TEMPORAL flags"):
        plan.set_temporal(1, T.TEMPORAL_RANGE, flags=4)
    for mode in (T.TEMPORAL_ORDER, T.TEMPORAL_RANGE):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*WEEKDAYS_ONLY"):
            plan.set_temporal(0 if mode == T.TEMPORAL_ORDER else 1, mode, flags=T.TEMPORAL_WEEKDAYS_ONLY)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*needs column2"):
        plan.set_temporal(1, T.TEMPORAL_ORDER)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*column2 goes with the order mode"):
        plan.set_temporal(0, T.TEMPORAL_RANGE)
    plan.set_temporal(0, T.TEMPORAL_ORDER, delta=I64_MAX)
    plan.set_temporal(0, T.TEMPORAL_ORDER, delta=I64_MIN)  # (may be set again until a state exists)


def test_setter_is_refused_after_the_first_state_and_on_other_kinds():
    plan = T.Plan([spec(T.TEMPORAL, 0), spec(T.COMOMENTS, 0, column2=1), spec(T.COUNT, 0)])
    for other in (1, 2, 3):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a TEMPORAL"):
            plan.set_temporal(other, T.TEMPORAL_RANGE)
    plan.set_temporal(0, T.TEMPORAL_RANGE, lo=0)
    st = T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*once a state"):
        plan.set_temporal(0, T.TEMPORAL_RANGE, lo=0)
    st.close()


def test_a_spec_without_parameters_fails_state_create():
    plan = T.Plan([spec(T.COUNT, 0), spec(T.TEMPORAL, 0), spec(T.TEMPORAL, 0)])
    plan.set_temporal(1, T.TEMPORAL_RANGE, lo=0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 2.*tgx_plan_set_temporal"):
        T.State(plan)
    plan.set_temporal(2, T.TEMPORAL_RANGE, hi=0)  # (the failed create has not locked the plan)
    T.State(plan).close()


@pytest.mark.parametrize("keep,weekdays", [(0, 0), (1, 0), (0, 2), (1, 2)])
def test_counts_of_a_host_only_state_follow_the_null_rules(keep, weekdays):
    """seen 10 / live 8, 6, 9 / passed 5, 4, 9: KEEP_NULLS considers every row seen -- except under the weekday filter,
    which a NULL row never passes"""
    plan = three_plan(keep, weekdays)
    st = T.State.deserialize(plan, three_blob(keep, weekdays))
    considered = [10 if keep else 8, 10 if keep and not weekdays else 6, 10 if keep else 9]
    want = [(10, c, c - p) for c, p in zip(considered, (5, 4, 9))]
    assert [st.temporal_counts(i) for i in range(3)] == want
    res = st.finalize()
    assert [(r.total, r.non_null, r.matches) for r in res[:3]] == [(10, c, p) for c, p in zip(considered, (5, 4, 9))]
    assert (res[3].total, res[3].non_null) == (10, 9)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a TEMPORAL"):
        st.temporal_counts(3)


def test_blob_round_trip_and_merge_through_a_host_only_state():
    plan = three_plan(1, 2)
    blob = three_blob(1, 2)
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    st.merge([T.State.deserialize(plan, blob), T.State.deserialize(plan, blob)])
    assert [st.temporal_counts(i) for i in range(3)] == [(30, 30, 15), (30, 18, 6), (30, 30, 3)]
    st.reset()
    assert [st.temporal_counts(i) for i in range(3)] == [(0, 0, 0)] * 3


def test_malformed_and_foreign_blobs_are_refused():
    plan = three_plan()
    blob = three_blob()
    for cut in (1, 8, 24, 25, 72, 73, 144):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    # counted under other parameters, or other flags
    other = three_plan()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other parameters"):
        T.State.deserialize(other, three_blob(keep=1))
    # passed <= live <= seen
    bad = wire.pack(temporal=[wire.temporal_state(3, 0, 10, 11, 5, lo=0, hi=I64_MAX)])
    rplan = T.Plan([spec(T.TEMPORAL, 0)])
    rplan.set_temporal(0, T.TEMPORAL_RANGE, lo=0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed"):
        T.State.deserialize(rplan, bad)
    # a plan without the kind does not take the section; a plan with it needs it
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(rplan, wire.pack())


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    parts = dict(count=[wire.count_acc(10, 7)], comoments=[wire.comoment_acc(10, 8, 1.0, 2.0, 3.0, 4.0, 5.0)])
    plain = T.Plan([spec(T.COUNT, 0), spec(T.COMOMENTS, 1, column2=2)])
    blob = wire.pack(**parts)
    assert wire.pack(temporal=(), **parts) == blob and b"TMPR" not in blob
    assert T.State.deserialize(plain, blob).serialize() == blob
    with_kind = T.Plan([spec(T.COUNT, 0), spec(T.COMOMENTS, 1, column2=2), spec(T.TEMPORAL, 0)])
    with_kind.set_temporal(2, T.TEMPORAL_RANGE, lo=0)
    section = wire.pack(temporal=[wire.temporal_state(3, 0, 5, 4, 3, lo=0, hi=I64_MAX)], **parts)
    assert section.startswith(blob) and len(section) == len(blob) + 8 + 64
    assert T.State.deserialize(with_kind, section).serialize() == section
    # behind the JOINT_BINS section where a plan holds both
    both = T.Plan([spec(T.JOINT_BINS, 0, column2=1), spec(T.TEMPORAL, 0)])
    both.set_temporal(1, T.TEMPORAL_RANGE, lo=0)
    b = wire.pack(joint=[wire.joint_range_state(5, 4, 0, 1.0, 2.0, 3.0, 4.0)],
                  temporal=[wire.temporal_state(3, 0, 5, 4, 3, lo=0, hi=I64_MAX)])
    st = T.State.deserialize(both, b)
    assert st.serialize() == b and st.temporal_counts(1) == (5, 4, 1)


# ---- the host layer: TemporalOrderingConstraint (host/temporal.cpp) through its JSON entry points --------------------
import json  # noqa: E402
import os  # noqa: E402

import term_amd.suite as S  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "temporal_ordering_vectors.json")) as f:
    GOLDEN = json.load(f)
NS, US, MS, SEC = ("Timestamp(%s, None)" % u for u in ("Nanosecond", "Microsecond", "Millisecond", "Second"))
PREFIX = "Constraint evaluation failed for 'temporal_ordering': "


def built(builder):
    """the golden file's builder calls applied to the Python class"""
    c = S.TemporalOrderingConstraint(builder["table"])
    for call, args in builder.items():
        if call != "table":
            c = getattr(c, call)(*args) if isinstance(args, list) else getattr(c, call)(args)
    return c


def counted(seen, considered, violations):
    return [{"total": seen, "non_null": considered, "matches": considered - violations}]


def test_golden_vectors_through_the_verdict():
    for case in GOLDEN["evaluated"]:
        c = built(case["builder"])
        before_col, after_col = case["builder"]["before_after"]
        params = S.temporal_params(c.spec, {before_col: case["column_type"], after_col: case["column_type"]})
        assert (params["mode"], params["delta"], params["flags"]) == (T.TEMPORAL_ORDER, 0, 0)
        before = [et.literal_ns(r[before_col]) for r in case["rows"]]
        after = [et.literal_ns(r[after_col]) for r in case["rows"]]
        seen, considered, violations = et.counts(et.ORDER, params, before, after)
        got = S.constraint_verdict(c.spec, counted(seen, considered, violations))
        want = et.verdict("before_after", considered, violations, before_col, after_col)
        assert got["name"] == "temporal_ordering" and got["status"] == case["status"].lower() == want[0].lower()
        assert (got["message"] is not None) == case["message_is_some"] and got["message"] == want[2]
        assert got["metric"] == want[1]


def test_golden_configuration():
    cfg = GOLDEN["configuration"]
    c = built(cfg["builder"])
    plan = S.constraint_plan(c.spec)
    (req,) = plan["requests"]
    assert plan["name"] == "temporal_ordering" and req["kind"] == T.TEMPORAL and req["column"] == "timestamp"
    t = req["temporal"]
    assert c.spec["table"] == cfg["fields"]["table_name"]
    assert t["allow_nulls"] is cfg["fields"]["allow_nulls"] and t["weekdays_only"] is cfg["fields"]["weekdays_only"]
    assert t["tolerance_seconds"] == cfg["fields"]["tolerance_seconds"] and t["mode"] == T.TEMPORAL_TIME_OF_DAY
    p = S.temporal_params(c.spec, {"timestamp": MS})
    assert p["flags"] == T.TEMPORAL_KEEP_NULLS | T.TEMPORAL_WEEKDAYS_ONLY
    assert (p["ticks_per_second"], p["tod_lo"], p["tod_hi"]) == (1000, 9 * 3600 * 1000, 17 * 3600 * 1000)


@pytest.mark.parametrize("unit,tps", [(NS, 10**9), (US, 10**6), (MS, 10**3), (SEC, 1)])
def test_the_four_comparison_strings_map_to_delta(unit, tps):
    """temporal_ordering.rs:352-368: allow_equal -> '>' (delta = tol + 1), else '>=' (delta = tol); inverted, kept"""
    types = {"a": unit, "b": unit}
    for allow_equal in (False, True):
        for tol in (0, 60, -5):
            c = S.TemporalOrderingConstraint("t")
            c = (c.before_or_equal if allow_equal else c.before_after)("a", "b").tolerance_seconds(tol)
            p = S.temporal_params(c.spec, types)
            assert p["delta"] == et.order_delta(allow_equal, tol, tps) == (tol * tps if tol > 0 else 0) + allow_equal
            assert (p["column"], p["column2"], p["mode"]) == ("a", "b", T.TEMPORAL_ORDER)


def test_unit_and_time_zone_rules():
    order = S.TemporalOrderingConstraint("t").before_after("a", "b")
    # tolerance 0: any Int64-shaped column, whatever its unit
    for types in ({}, {"a": "Int64", "b": "Date64"}, {"a": NS, "b": SEC}, {"a": 'Timestamp(Second, Some("Europe/Paris"))'}):
        assert S.temporal_params(order.spec, types)["delta"] == 0
    tol = S.TemporalOrderingConstraint("t").before_after("a", "b").tolerance_seconds(60)
    with pytest.raises(T.TgxError, match=PREFIX + "a tolerance in seconds needs a Timestamp.*the column is Int64"):
        S.temporal_params(tol.spec, {"a": "Int64", "b": NS})
    with pytest.raises(T.TgxError, match=PREFIX + "a tolerance in seconds needs a Timestamp.*an unknown type"):
        S.temporal_params(tol.spec, {"a": NS})
    with pytest.raises(T.TgxError, match=PREFIX + "a tolerance in seconds needs both columns in the same unit"):
        S.temporal_params(tol.spec, {"a": NS, "b": US})
    paris = 'Timestamp(Microsecond, Some("Europe/Paris"))'
    assert S.temporal_params(tol.spec, {"a": paris, "b": paris})["delta"] == 60 * 10**6  # (a difference has no zone)
    hours = S.TemporalOrderingConstraint("t").business_hours("a", "09:00", "17:00").with_timezone("Europe/Paris")
    rng = S.TemporalOrderingConstraint("t").date_range("a", "2024-01-01", None)
    for c, what in ((hours, "business hours validation"), (rng, "date range validation")):
        for tz in ("None", 'Some("UTC")', 'Some("+00:00")'):
            S.temporal_params(c.spec, {"a": "Timestamp(Second, %s)" % tz})
        with pytest.raises(T.TgxError, match=PREFIX + what + " needs a column without a time zone"):
            S.temporal_params(c.spec, {"a": paris})
        with pytest.raises(T.TgxError, match=PREFIX + what + " needs a Timestamp.*the column is Int64"):
            S.temporal_params(c.spec, {"a": "Int64"})
    # the stored timezone never reaches the query: it changes nothing here either
    plain = S.TemporalOrderingConstraint("t").business_hours("a", "09:00", "17:00")
    assert S.temporal_params(hours.spec, {"a": NS}) == S.temporal_params(plain.spec, {"a": NS})


def test_every_error_text():
    with pytest.raises(T.TgxError, match=PREFIX + "DateRange validation requires at least min_date or max_date"):
        S.constraint_plan(S.TemporalOrderingConstraint("t").date_range("a").spec)
    with pytest.raises(T.TgxError, match=PREFIX + "MaxTimeGap validation is a LAG.*not on the GPU path"):
        S.constraint_plan(S.TemporalOrderingConstraint("t").max_time_gap("a", 60).group_by("g").spec)
    seq = {"type": "temporal_ordering", "table": "t", "validation": "event_sequence", "event_column": "e",
           "timestamp_column": "a", "expected_sequence": ["x", "y"]}
    with pytest.raises(T.TgxError, match=PREFIX + "Event sequence validation not yet implemented"):
        S.constraint_plan(seq)
    # Check::Builder::temporal_ordering(table): the default object, empty column names
    default = S.Check.builder("c").temporal_ordering("events").build().spec["constraints"][0]
    with pytest.raises(T.TgxError, match="Security error"):
        S.constraint_plan(default)
    with pytest.raises(T.TgxError, match="Security error"):
        S.constraint_plan(S.TemporalOrderingConstraint("bad table;").before_after("a", "b").spec)
    with pytest.raises(T.TgxError, match="Security error"):
        S.constraint_plan(S.TemporalOrderingConstraint("t").max_time_gap("a", 60).group_by("g; drop").spec)
    for text in ("2024", "2024-13-01", "2023-02-29", "2024-01-01 24:00:00", "2024-01-01 10:00", "01/02/2024",
                 "2024-01-01 10:00:00+01:00", "2024-01-01 10:00:00.", "2024-01-01 10:00:00.1234567890", "9999-01-01"):
        assert et.literal_ns(text) is None or text == "9999-01-01"
        with pytest.raises(T.TgxError, match=PREFIX + "Temporal validation query failed: cannot parse"):
            S.temporal_params(S.TemporalOrderingConstraint("t").date_range("a", None, text).spec, {"a": NS})
    for hhmm in ("9:00", "24:00", "09:60", "0900", "09:00:00"):
        with pytest.raises(T.TgxError, match=PREFIX + "Temporal validation query failed: cannot parse.*TIME"):
            S.temporal_params(S.TemporalOrderingConstraint("t").business_hours("a", hhmm, "17:00").spec, {"a": NS})


@pytest.mark.parametrize("unit,tps", [(NS, 10**9), (US, 10**6), (MS, 10**3), (SEC, 1)])
def test_range_bounds_round_inwards_on_coarser_units(unit, tps):
    """a literal is a nanosecond instant: lo = ceil, hi = floor, at the exact multiple and one nanosecond off it"""
    for text in ("2024-01-01", "2024-03-05 10:20:30", "2024-03-05T10:20:30.000000001Z", "2024-03-05 10:20:30.999999999",
                 "1969-12-31 23:59:59.999999999", "1969-12-31 23:59:59.000000001", "1960-02-29 00:00:00.5",
                 "2024-03-05 10:20:30.001", "2024-03-05 10:20:30.000001"):
        ns = et.literal_ns(text)
        c = S.TemporalOrderingConstraint("t").date_range("a", text, text)
        p = S.temporal_params(c.spec, {"a": unit})
        assert (p["lo"], p["hi"]) == et.range_bounds(ns, ns, tps), text
        assert p["lo"] - p["hi"] == (0 if ns % (10**9 // tps) == 0 else 1)
    only_min = S.temporal_params(S.TemporalOrderingConstraint("t").date_range("a", "2024-01-01", None).spec, {"a": unit})
    assert only_min["hi"] == I64_MAX and only_min["lo"] == et.literal_ns("2024-01-01") // (10**9 // tps)
    only_max = S.temporal_params(S.TemporalOrderingConstraint("t").date_range("a", None, "2024-01-01").spec, {"a": unit})
    assert only_max["lo"] == I64_MIN


def test_literals_agree_with_the_reference_parser():
    import random

    rng = random.Random(9)
    for _ in range(300):
        secs = rng.randrange(-250 * 365 * 86400, 250 * 365 * 86400)
        import datetime as dt

        when = dt.datetime(1970, 1, 1) + dt.timedelta(seconds=secs)
        frac = "".join(rng.choice("0123456789") for _ in range(rng.randrange(0, 10)))
        text = when.strftime("%Y-%m-%d") + rng.choice(" T") + when.strftime("%H:%M:%S") + ("." + frac if frac else "")
        text += rng.choice(["", "Z"])
        p = S.temporal_params(S.TemporalOrderingConstraint("t").date_range("a", text, None).spec, {"a": NS})
        assert p["lo"] == et.literal_ns(text) == secs * 10**9 + int(frac.ljust(9, "0") or 0), text


def test_verdict_texts_and_two_decimal_places():
    kinds = {"before_after": S.TemporalOrderingConstraint("t").before_after("created_at", "processed_at"),
             "business_hours": S.TemporalOrderingConstraint("t").business_hours("ts", "09:00", "17:00"),
             "date_range": S.TemporalOrderingConstraint("t").date_range("ts", "2024-01-01")}
    for kind, c in kinds.items():
        cols = ("created_at", "processed_at") if kind == "before_after" else ("ts", None)
        # 0 %, 99.995 % (rounds to 100.00 or 99.99 as the double's exact value says), 100 % = success
        for considered, violations in ((4, 4), (20000, 1), (3, 1), (7, 0), (0, 0)):
            got = S.constraint_verdict(c.spec, counted(considered + 2, considered, violations))
            status, metric, message = et.verdict(kind, considered, violations, *cols)
            assert (got["status"], got["metric"], got["message"]) == (status.lower(), metric, message)
    zero = S.constraint_verdict(kinds["business_hours"].spec, counted(4, 4, 4))
    assert zero["message"] == "Business hours violation: 4 records with 'ts' outside business hours (0.00% compliance)"
    near = S.constraint_verdict(kinds["date_range"].spec, counted(20000, 20000, 1))
    assert near["metric"] == 19999 / 20000 and near["message"].endswith("(%.2f%% compliance)" % (19999 / 20000 * 100.0))
    assert S.constraint_verdict(kinds["date_range"].spec, counted(5, 0, 0)) == \
        {"status": "success", "metric": 1.0, "message": None, "name": "temporal_ordering"}


def test_builder_calls_follow_the_reference():
    """weekdays_only / with_timezone / group_by act only on their own validation type (:191-276)"""
    c = S.TemporalOrderingConstraint("t").before_after("a", "b").weekdays_only(True).with_timezone("UTC").group_by("g")
    assert "weekdays_only" not in c.spec and "timezone" not in c.spec and "group_by_column" not in c.spec
    c = S.TemporalOrderingConstraint("t").allow_nulls(True).business_hours("a", "09:00", "17:00").weekdays_only(True)
    assert c.spec["allow_nulls"] is True and c.spec["weekdays_only"] is True
    assert T.TemporalOrderingConstraint is S.TemporalOrderingConstraint and T.CheckBuilder is S.CheckBuilder
