"""TGX_CHECK_GROUP_COUNTS without a device: plan validation, what a host-only state answers from a blob, merging by
value and every malformed-blob refusal of the section (term_amd/wire.py)."""
import ctypes as C
import struct

import pytest

import term_amd as T
from _lib_spec import spec
from term_amd import wire

INTS = {5: (3, 1), -1: (2, 2), 7: (4, 0)}
TEXT = {b"b": (3, 3), b"": (2, 1), b"ab": (1, 0), b"\xff": (1, 1)}
ZERO = dict(seen=0, groups=0, counted=0, counted_non_null=0, null_group_rows=0, null_group_non_null=0, overflow_rows=0,
            overflow_non_null=0, long_rows=0, long_non_null=0)


def groups_plan(mvb=16):
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, column2=1), spec(T.GROUP_COUNTS, 0, column2=2), spec(T.COUNT, 0)])
    plan.set_group_counts(0, 4, 8)
    plan.set_group_counts(1, 100, mvb)
    return plan


def groups_blob(first=None, second=None, mvb=16):
    first = wire.group_counts_state(4, 8, INTS, null_group=(1, 1)) if first is None else first
    if second is None:
        second = wire.group_counts_state(100, mvb, TEXT, null_group=(1, 0), overflow=(1, 1), long=(1, 1))
    return wire.pack(count=[wire.count_acc(10, 4)], group_counts=[first, second])


def test_abi_constants():
    assert T.GROUP_COUNTS == 17 and (T.GROUP_COUNTS_MAX_GROUPS, T.GROUP_COUNTS_MAX_VALUE_BYTES) == (65536, 256)
    for name in ("tgx_plan_set_group_counts", "tgx_group_counts_get", "tgx_group_counts_entries"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)
    assert T.lib().tgx_abi_version() == 6  # (only entry points were added)


def test_parameters_are_validated():
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, column2=1), spec(T.COUNT, 0)])
    for bad in (0, 65537, 2**32 - 1):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_groups must be 1 \.\. 65536 \(%d\)" % bad):
            plan.set_group_counts(0, bad, 16)
    for bad in (0, 257):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_value_bytes must be 1 \.\. 256 \(%d\)" % bad):
            plan.set_group_counts(0, 10, bad)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1 is not a GROUP_COUNTS check"):
        plan.set_group_counts(1, 10, 16)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_COUNTS needs column2"):
        T.Plan([spec(T.GROUP_COUNTS, 0)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*only DISTINCT takes a column list"):
        T.Plan([spec(T.GROUP_COUNTS, 0, column2=1, columns=[1, 2])])  # several group columns: a spec list stays refused
    for ok in ((1, 1), (65536, 256)):
        plan.set_group_counts(0, *ok)


def test_a_spec_without_parameters_fails_state_create_and_deserialize():
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, column2=1), spec(T.GROUP_COUNTS, 0, column2=1)])
    plan.set_group_counts(0, 10, 16)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*tgx_plan_set_group_counts"):
        T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_plan_set_group_counts"):
        T.State.deserialize(plan, wire.pack(group_counts=[wire.group_counts_state(10, 16, {})] * 2))


def test_setter_is_refused_after_the_first_state():
    plan = groups_plan()
    st = T.State.deserialize(plan, groups_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_group_counts(0, 5, 8)
    del st


def test_a_host_only_state_answers_its_blob():
    plan = groups_plan()
    st = T.State.deserialize(plan, groups_blob())
    summary, groups = st.group_counts(0)
    assert summary == dict(ZERO, seen=10, groups=3, counted=9, counted_non_null=3, null_group_rows=1, null_group_non_null=1)
    assert list(groups.items()) == [(-1, (2, 2)), (5, (3, 1)), (7, (4, 0))]  # ascending int64
    summary, groups = st.group_counts(1)
    assert summary == dict(seen=10, groups=4, counted=7, counted_non_null=5, null_group_rows=1, null_group_non_null=0,
                           overflow_rows=1, overflow_non_null=1, long_rows=1, long_non_null=1)
    assert list(groups.items()) == [(b"", (2, 1)), (b"ab", (1, 0)), (b"b", (3, 3)), (b"\xff", (1, 1))]  # bytewise, a prefix first
    res = st.finalize()
    assert [(r.total, r.non_null, r.distinct, r.matches) for r in res[:2]] == [(10, 4, 3, 9), (10, 7, 4, 7)]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 2 is not a GROUP_COUNTS check"):
        st.group_counts(2)
    foreign = T.State.deserialize(groups_plan(), groups_blob())
    L, err, out = T.lib(), T._lib._Error(), T._lib.GroupCountsSummary()
    assert L.tgx_group_counts_get(plan.h, foreign.h, 0, C.byref(out), C.byref(err)) != 0  # a state of another plan


def test_the_entries_call_follows_the_size_query_convention():
    plan = groups_plan()
    st = T.State.deserialize(plan, groups_blob())
    L, err = T.lib(), T._lib._Error()
    n, nb, kind = C.c_uint64(), C.c_uint64(), C.c_int32()
    assert L.tgx_group_counts_entries(plan.h, st.h, 1, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(kind), C.byref(err)) == 0
    assert (n.value, nb.value, kind.value) == (4, 4, 1)
    small = (T._lib.GroupCountEntry * 3)()
    buf = (C.c_uint8 * 8)()
    assert L.tgx_group_counts_entries(plan.h, st.h, 1, small, 3, C.byref(n), buf, 8, C.byref(nb), C.byref(kind), C.byref(err)) != 0
    assert b"entries holds 3 entries, 4 are needed" in err.msg and n.value == 4
    assert all(e.total == 0 for e in small)  # nothing copied
    full = (T._lib.GroupCountEntry * 4)()
    assert L.tgx_group_counts_entries(plan.h, st.h, 1, full, 4, C.byref(n), buf, 3, C.byref(nb), C.byref(kind), C.byref(err)) != 0
    assert b"bytes holds 3 bytes, 4 are needed" in err.msg
    assert L.tgx_group_counts_entries(plan.h, st.h, 0, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(kind), C.byref(err)) == 0
    assert (n.value, nb.value, kind.value) == (3, 0, 0)


def test_blob_round_trip_and_merge_by_value():
    plan = groups_plan()
    blob = groups_blob()
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    # a task without keys, with and without rows, beside one with keys
    for empty in (wire.group_counts_state(4, 8, {}), wire.group_counts_state(4, 8, {}, null_group=(3, 2))):
        assert T.State.deserialize(plan, groups_blob(first=empty)).serialize() == groups_blob(first=empty)
    other = groups_blob(wire.group_counts_state(4, 8, {7: (1, 1), 9: (5, 2)}),
                        wire.group_counts_state(100, 16, {b"b": (1, 0), b"c": (2, 2)}, null_group=(1, 1)))
    st.merge([T.State.deserialize(plan, other), T.State.deserialize(plan, blob)])
    summary, groups = st.group_counts(0)
    assert groups == {-1: (4, 4), 5: (6, 2), 7: (9, 1), 9: (5, 2)}
    assert (summary["groups"], summary["seen"], summary["null_group_rows"], summary["null_group_non_null"]) == (4, 26, 2, 2)
    summary, groups = st.group_counts(1)
    assert groups == {b"": (4, 2), b"ab": (2, 0), b"b": (7, 6), b"c": (2, 2), b"\xff": (2, 2)}
    assert summary == dict(seen=24, groups=5, counted=17, counted_non_null=12, null_group_rows=3, null_group_non_null=1,
                           overflow_rows=2, overflow_non_null=2, long_rows=2, long_non_null=2)
    again = T.State.deserialize(plan, st.serialize())  # equal states, equal bytes
    assert again.serialize() == st.serialize() and again.group_counts(1) == st.group_counts(1)
    st.reset()
    assert st.group_counts(1) == (ZERO, {})


def test_tasks_that_share_a_walk_keep_their_own_counts():
    # tasks 0 and 1 group by column 3 under the same bounds and ride one walk (one table on the device); task 2 has a
    # walk of its own
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, column2=3), spec(T.GROUP_COUNTS, 1, column2=3), spec(T.GROUP_COUNTS, 2, column2=4)])
    for k in range(3):
        plan.set_group_counts(k, 8, 16)
    tasks = [({b"": (4, 4), b"a": (3, 1)}, (2, 2)), ({b"": (4, 0), b"a": (3, 3)}, (2, 0)), ({7: (5, 2), -3: (4, 4)}, (0, 0))]
    blob = wire.pack(group_counts=[wire.group_counts_state(8, 16, g, null_group=n) for g, n in tasks])
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    into = T.State(plan)
    into.merge([st])
    for state in (st, into):
        for k, (groups, null_group) in enumerate(tasks):
            summary, got = state.group_counts(k)
            assert got == groups
            assert summary["counted_non_null"] == sum(n for _, n in groups.values())
            assert (summary["null_group_rows"], summary["null_group_non_null"]) == null_group
    assert into.serialize() == blob
    into.merge([st])
    assert into.group_counts(1)[1] == {b"": (8, 0), b"a": (6, 6)} and into.group_counts(0)[1] == {b"": (8, 8), b"a": (6, 2)}


def test_integer_and_string_states_do_not_merge():
    plan = groups_plan()
    a = T.State.deserialize(plan, groups_blob())
    b = T.State.deserialize(plan, groups_blob(first=wire.group_counts_state(4, 8, {b"x": (3, 1)})))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_COUNTS task 0.*different group column types"):
        a.merge([b])
    empty = T.State.deserialize(plan, groups_blob(first=wire.group_counts_state(4, 8, {}, null_group=(3, 2))))
    a.merge([empty])  # (a state without keys merges with either)
    assert a.group_counts(0)[0]["seen"] == 13


def raw_task(max_groups, mvb, kind, seen, classes, entries, n=None):
    """classes: null_group_rows, null_group_non_null, overflow_rows, overflow_non_null, long_rows, long_non_null"""
    out = struct.pack("<4I8Q", max_groups, mvb, kind, 0, seen, *classes, len(entries) if n is None else n)
    for k, t, nn in entries:
        out += (struct.pack("<I", len(k)) + k if isinstance(k, bytes) else struct.pack("<q", k)) + struct.pack("<QQ", t, nn)
    return out


NONE = (0, 0, 0, 0, 0, 0)
MALFORMED = [
    ("other parameters", raw_task(5, 8, 1, 3, NONE, [(1, 3, 0)]), None),
    ("other parameters", None, raw_task(100, 17, 2, 3, NONE, [(b"a", 3, 0)])),
    ("non_null > total", raw_task(4, 8, 1, 7, NONE, [(5, 3, 4), (7, 4, 0)]), None),
    ("non_null > total", None, raw_task(100, 16, 2, 3, NONE, [(b"a", 3, 2**64 - 1)])),
    ("zero count", raw_task(4, 8, 1, 3, NONE, [(5, 3, 0), (7, 0, 0)]), None),
    ("out of order or repeated", raw_task(4, 8, 1, 7, NONE, [(7, 3, 0), (5, 4, 0)]), None),
    ("out of order or repeated", raw_task(4, 8, 1, 7, NONE, [(5, 3, 0), (5, 4, 0)]), None),
    ("out of order or repeated", None, raw_task(100, 16, 2, 7, NONE, [(b"b", 3, 0), (b"ab", 4, 0)])),
    ("out of order or repeated", None, raw_task(100, 16, 2, 7, NONE, [(b"", 3, 0), (b"", 4, 0)])),
    ("a key of 17 bytes, max_value_bytes is 16", None, raw_task(100, 16, 2, 3, NONE, [(b"x" * 17, 3, 0)])),
    ("!= seen", raw_task(4, 8, 1, 8, NONE, [(5, 3, 0), (7, 4, 0)]), None),                # counted 7, seen 8
    ("!= seen", raw_task(4, 8, 1, 7, (1, 0, 0, 0, 0, 0), [(5, 3, 0), (7, 4, 0)]), None),  # the NULL group on top
    ("!= seen", None, raw_task(100, 16, 2, 9, (0, 0, 1, 0, 2, 0), [(b"a", 7, 0)])),       # 7 + 1 + 2 != 9
    ("non_null > rows", raw_task(4, 8, 1, 9, (2, 3, 0, 0, 0, 0), [(5, 3, 0), (7, 4, 0)]), None),
    ("non_null > rows", raw_task(4, 8, 1, 9, (0, 0, 2, 3, 0, 0), [(5, 3, 0), (7, 4, 0)]), None),
    ("non_null > rows", None, raw_task(100, 16, 2, 9, (0, 0, 0, 0, 2, 3), [(b"a", 7, 0)])),
    ("kind", raw_task(4, 8, 3, 0, NONE, []), None),
    ("kind", raw_task(4, 8, 0, 3, NONE, [], n=1), None),                                  # entries without a kind
    ("counts", raw_task(4, 8, 1, 10, NONE, [(5, 2**64 - 1, 0), (7, 2, 0)]), None),        # a sum that wraps
]


@pytest.mark.parametrize("what,first,second", MALFORMED)
def test_malformed_blobs_are_refused(what, first, second):
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + what):
        T.State.deserialize(groups_plan(), groups_blob(first, second))


def test_truncated_and_foreign_blobs_are_refused():
    plan, blob = groups_plan(), groups_blob()
    for cut in (1, 8, 16, 17, 40, len(blob) - 60):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plan, groups_blob(first=raw_task(4, 8, 1, 3, NONE, [(5, 3, 0)], n=2**60)))
    other = T.Plan([spec(T.GROUP_COUNTS, 0, column2=1), spec(T.COUNT, 0)])
    other.set_group_counts(0, 4, 8)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different plan"):
        T.State.deserialize(other, blob)


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0)])
    blob = wire.pack(count=[wire.count_acc(10, 9)])
    assert T.State.deserialize(plan, blob).serialize() == blob  # (the blob version stays 3: no section, no bytes)
    assert wire.VERSION == 3


# ---- the host layer: CompletenessAnalyzer(c).with_grouping(GroupingConfig(..)) -------------------------------------------------
import json  # noqa: E402

import exact_group_counts as ex  # noqa: E402
import term_amd.suite as S  # noqa: E402


def grouped(column="sales", by=("region",), **kw):
    return S.CompletenessAnalyzer(column).with_grouping(S.GroupingConfig(list(by), **kw))


def state_of(analyzer, keyed, null_group=None, **summary):
    """the analyzer's state from {key: (total, non_null)} as the device would report it (ascending by key)"""
    entries = [(k, t, n) for k, (t, n) in sorted(keyed.items())]
    if null_group:
        summary.update(null_group_rows=null_group[0], null_group_non_null=null_group[1])
    return json.loads(analyzer.state_text_from_group_counts(summary, entries))


def exact_state(groups, null_group=None, by=("region",), **kw):
    keyed = {(k,): list(v) for k, v in groups.items()}
    if null_group:
        keyed[(None,)] = list(null_group)
    return ex.grouped_state(keyed, list(by), **kw)


def metric_of(analyzer, state):
    m = analyzer.compute_metric_from_state(state)
    assert m["type"] == "Map"
    return {k: v["value"] for k, v in m["value"].items()}, {k: v["type"] for k, v in m["value"].items()}


def test_names_keys_and_the_json_tag():
    a = grouped()
    assert a.name() == "completeness" and a.metric_key() == "completeness.sales_grouped_by_region"
    assert a.spec == {"type": "grouped_completeness", "column": "sales", "group_by": ["region"], "max_groups": 10000,
                      "include_overall": True}
    assert grouped(strict_reference_types=False).spec["strict_reference_types"] is False
    cfg = S.GroupingConfig("g").with_max_groups(5).with_overall(False)
    assert (cfg.columns, cfg.max_groups, cfg.include_overall, cfg.overflow_strategy) == (["g"], 5, False, "TopK")
    for other in (S.SizeAnalyzer(), S.MeanAnalyzer("x"), S.EntropyAnalyzer("x"), grouped()):
        with pytest.raises(TypeError, match="only CompletenessAnalyzer"):
            other.with_grouping(S.GroupingConfig(["g"]))
    req = a.planned_requests([T.INT64, T.UTF8])
    assert req == [{"kind": T.GROUP_COUNTS, "column": "sales", "column2": "region",
                    "group_counts": {"max_groups": 10000, "max_value_bytes": 256}}]
    assert grouped(max_groups=10**6).planned_requests([T.INT64, T.UTF8])[0]["group_counts"]["max_groups"] == 65536


def test_the_metric_map_of_the_reference_table():
    a = grouped()
    groups = {b"US": (3, 3), b"EU": (3, 2)}
    state = state_of(a, groups)
    assert state == {"groups": [{"key": ["EU"], "total_count": 3, "non_null_count": 2},
                                {"key": ["US"], "total_count": 3, "non_null_count": 3}],
                     "null_group": None, "overall": {"total_count": 6, "non_null_count": 5},
                     "metadata": {"group_columns": ["region"], "total_groups": 2, "included_groups": 2, "truncated": False,
                                  "overflow_strategy": None}}
    values, types = metric_of(a, state)
    assert values == ex.metric_map(exact_state(groups)) and list(values)[-2:] == ["__overall__", "__metadata__"]
    assert types == {"EU": "Double", "US": "Double", "__overall__": "Double", "__metadata__": "String"}
    assert values["__metadata__"] == ('{"group_columns":["region"],"total_groups":2,"included_groups":2,"truncated":false,'
                                      '"overflow_strategy":null}')
    text = a.state_text_from_group_counts({}, [(b"EU", 3, 2)])
    assert '"total_count": 3, "non_null_count": 2' in text  # integer tokens
    no_overall = grouped(include_overall=False)
    assert state_of(no_overall, groups)["overall"] is None
    assert "__overall__" not in metric_of(no_overall, state_of(no_overall, groups))[0]


@pytest.mark.parametrize("max_groups", [4, 3, 1])
def test_truncation_follows_the_reference(max_groups):
    groups = {b"a": (4, 4), b"b": (4, 2), b"c": (4, 3), b"d": (4, 1)}
    a = grouped(max_groups=max_groups)
    want = exact_state(groups, max_groups=max_groups)
    state = state_of(a, groups)
    assert state["metadata"] == want["metadata"]
    assert {tuple(g["key"]): (g["total_count"], g["non_null_count"]) for g in state["groups"]} == want["groups"]
    assert (state["overall"]["total_count"], state["overall"]["non_null_count"]) == want["overall"]  # the kept groups only
    assert metric_of(a, state)[0] == ex.metric_map(want)
    assert state["metadata"]["truncated"] == (max_groups < 4)


def test_ties_the_null_group_and_its_collision_with_the_empty_string():
    a = grouped(max_groups=3)
    groups = {b"z": (1, 1), b"b": (3, 3), b"": (5, 5)}
    state = state_of(a, groups, null_group=(2, 2))  # four rows tie at 1.0: the NULL group is the one that is cut
    assert [g["key"] for g in state["groups"]] == [[""], ["b"], ["z"]] and state["null_group"] is None
    assert state["metadata"]["total_groups"] == 4 and state["metadata"]["truncated"]
    a = grouped()
    groups = {b"": (4, 2), b"k": (1, 1)}
    want = exact_state(groups, null_group=(2, 1))
    state = state_of(a, groups, null_group=(2, 1))  # "" and NULL tie at 0.5: NULL is the later row and overwrites
    assert state["null_group"] == {"total_count": 2, "non_null_count": 1} and state["metadata"] == want["metadata"]
    assert (state["metadata"]["total_groups"], state["metadata"]["included_groups"], state["metadata"]["truncated"]) == (3, 2, True)
    assert state["overall"] == {"total_count": 7, "non_null_count": 4}
    assert metric_of(a, state)[0] == ex.metric_map(want)
    for null_group, empty, stays in (((4, 1), (4, 2), 0.25), ((4, 3), (4, 2), 0.5)):  # the less complete row is the later
        s = state_of(a, {b"": empty}, null_group=null_group)
        assert metric_of(a, s)[0][""] == stays == ex.metric_map(exact_state({b"": empty}, null_group=null_group))[""]
    alone = state_of(a, {b"k": (1, 1)}, null_group=(2, 0))
    assert metric_of(a, alone)[0][""] == 0.0 and alone["metadata"]["included_groups"] == 2


def test_the_reserved_keys_overwrite_a_group_of_their_name():
    a = grouped(by=("g",))
    groups = {b"__overall__": (2, 0), b"__metadata__": (2, 2), b"a": (4, 1)}
    values, types = metric_of(a, state_of(a, groups))
    assert values == ex.metric_map(exact_state(groups, by=("g",))) and len(values) == 3
    assert values["__overall__"] == 3 / 8 and types["__metadata__"] == "String"
    assert metric_of(a, {"groups": [], "null_group": None, "overall": {"total_count": 0, "non_null_count": 0},
                         "metadata": {"group_columns": ["g"], "total_groups": 0, "included_groups": 0, "truncated": False,
                                      "overflow_strategy": None}})[0]["__overall__"] == 1.0  # an empty state is complete


def test_integer_keys_print_as_decimal_text():
    a = grouped(by=("g",), strict_reference_types=False)
    state = state_of(a, {-5: (2, 1), 10: (2, 2), 9: (1, 1)})
    assert [g["key"] for g in state["groups"]] == [["-5"], ["10"], ["9"]]  # ascending by text
    assert metric_of(a, state)[0]["-5"] == 0.5


def test_merge_states_follows_the_reference():
    a = grouped()
    s1 = state_of(a, {b"EU": (3, 2), b"US": (3, 3)}, null_group=(1, 0))
    s2 = state_of(grouped(max_groups=1), {b"EU": (2, 2), b"APAC": (5, 1)})  # truncated: total_groups 2, one kept
    merged = a.merge_states([s1, s2])
    assert merged["groups"] == [{"key": ["EU"], "total_count": 5, "non_null_count": 4},
                                {"key": ["US"], "total_count": 3, "non_null_count": 3}]
    assert merged["null_group"] == {"total_count": 1, "non_null_count": 0}
    assert merged["overall"] == {"total_count": 9, "non_null_count": 7}
    assert merged["metadata"] == {"group_columns": ["region"], "total_groups": 3, "included_groups": 3, "truncated": False,
                                  "overflow_strategy": None}
    text = a.merge_states_text([s1, s2])
    assert '"total_count": 5, "non_null_count": 4' in text and "5.0" not in text  # integer tokens
    with pytest.raises(T.TgxError, match="Cannot merge empty states"):
        a.merge_states([])


def test_the_analyzers_errors():
    strict = grouped()
    for type, name in ((T.INT64, "tgx type 1"), (T.LARGE_UTF8, "LargeUtf8"), (T.DICT32_UTF8, "Dictionary")):
        with pytest.raises(T.TgxError, match="group column 'region' is %s.*whole key array.*strict_reference_types=false" % name):
            strict.planned_requests([T.INT64, type])
    assert grouped(strict_reference_types=False).planned_requests([T.INT64, T.INT64])[0]["kind"] == T.GROUP_COUNTS
    for by in ((), ("a", "b")):
        with pytest.raises(T.TgxError, match=r"groups by exactly one column on the GPU path \(%d given\)" % len(by)):
            grouped(by=by).planned_requests([T.INT64] * (1 + len(by)))
    with pytest.raises(T.TgxError, match="max_groups 16 holds.*32 groups held, 7 overflow rows, 0 long rows"):
        state_of(grouped(max_groups=16), {b"a": (1, 1)}, groups=32, overflow_rows=7)
    with pytest.raises(T.TgxError, match="0 overflow rows, 3 long rows"):
        state_of(grouped(), {b"a": (1, 1)}, groups=1, long_rows=3)
