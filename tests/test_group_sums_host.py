"""TGX_CHECK_GROUP_SUMS without a device: plan validation, what a host-only state answers from a blob, merging by value
(integer sums with wrap, float sums in state order) and every malformed-blob refusal of the section (term_amd/wire.py);
then the host layer's CrossTableSumConstraint: its name, JSON form and getters, the reference's qualified-name errors, and
the join, verdict and both message shapes on injected sums, held against tests/exact_group_sums.py and the golden vectors."""
import ctypes as C
import struct

import pytest

import term_amd as T
from _lib_spec import spec
from term_amd import wire

M64 = (1 << 64) - 1
INTS = {5: (3, 1, 40), -1: (2, 2, -7), 7: (4, 0, 0)}
TEXT = {b"b": (3, 3, 1.5), b"": (2, 1, -0.25), b"ab": (1, 0, 0.0), b"\xff": (1, 1, 2.0)}
NOTHING = (0, 0, 0)


def sums_plan(mvb=16):
    plan = T.Plan([spec(T.GROUP_SUMS, 0, column2=1), spec(T.GROUP_SUMS, 0, column2=2), spec(T.COUNT, 0)])
    plan.set_group_sums(0, 4, 8)
    plan.set_group_sums(1, 100, mvb)
    return plan


def sums_blob(first=None, second=None, mvb=16):
    first = wire.group_sums_state(4, 8, INTS, null_group=(1, 1, 9)) if first is None else first
    if second is None:
        second = wire.group_sums_state(100, mvb, TEXT, is_float=True, null_group=(1, 0, 0.0), overflow=(1, 1, 8.0),
                                       long=(1, 1, -1.0))
    return wire.pack(count=[wire.count_acc(10, 4)], group_sums=[first, second])


def test_abi_constants():
    assert T.GROUP_SUMS == 18 and (T.GROUP_SUMS_MAX_GROUPS, T.GROUP_SUMS_MAX_VALUE_BYTES) == (65536, 256)
    for name in ("tgx_plan_set_group_sums", "tgx_group_sums_get", "tgx_group_sums_entries"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)
    assert T.lib().tgx_abi_version() == 6  # (only entry points were added)
    assert C.sizeof(T._lib.GroupSumsSummary) == 24 + 4 * 32 and C.sizeof(T._lib.GroupSumEntry) == 56
    assert wire.GROUP_SUMS_MAGIC == struct.unpack("<I", b"GSUM")[0]


def test_parameters_are_validated():
    plan = T.Plan([spec(T.GROUP_SUMS, 0, column2=1), spec(T.COUNT, 0)])
    for bad in (0, 65537, 2**32 - 1):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_groups must be 1 \.\. 65536 \(%d\)" % bad):
            plan.set_group_sums(0, bad, 16)
    for bad in (0, 257):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_value_bytes must be 1 \.\. 256 \(%d\)" % bad):
            plan.set_group_sums(0, 10, bad)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1 is not a GROUP_SUMS check"):
        plan.set_group_sums(1, 10, 16)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS needs column2"):
        T.Plan([spec(T.GROUP_SUMS, 0)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*only DISTINCT takes a column list"):
        T.Plan([spec(T.GROUP_SUMS, 0, column2=1, columns=[1, 2])])  # several group columns: a spec list stays refused
    for ok in ((1, 1), (65536, 256)):
        plan.set_group_sums(0, *ok)
    same = T.Plan([spec(T.GROUP_SUMS, 0, column2=0)])  # the value column may be the group column
    same.set_group_sums(0, 10, 16)
    assert T.State(same).group_sums(0)[1] == {}


def test_a_spec_without_parameters_fails_state_create_and_deserialize():
    plan = T.Plan([spec(T.GROUP_SUMS, 0, column2=1), spec(T.GROUP_SUMS, 0, column2=1)])
    plan.set_group_sums(0, 10, 16)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*tgx_plan_set_group_sums"):
        T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_plan_set_group_sums"):
        T.State.deserialize(plan, wire.pack(group_sums=[wire.group_sums_state(10, 16, {})] * 2))


def test_setter_is_refused_after_the_first_state():
    plan = sums_plan()
    st = T.State.deserialize(plan, sums_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_group_sums(0, 5, 8)
    del st


def test_a_host_only_state_answers_its_blob():
    plan = sums_plan()
    st = T.State.deserialize(plan, sums_blob())
    summary, groups = st.group_sums(0)
    assert summary == dict(seen=10, groups=3, is_float=False, counted=(9, 3, 33), null_group=(1, 1, 9), overflow=NOTHING,
                           long_rows=NOTHING)
    assert list(groups.items()) == [(-1, (2, 2, -7)), (5, (3, 1, 40)), (7, (4, 0, 0))]  # ascending int64
    assert all(type(v[2]) is int for v in groups.values())
    summary, groups = st.group_sums(1)
    assert summary == dict(seen=10, groups=4, is_float=True, counted=(7, 5, 3.25), null_group=(1, 0, 0.0),
                           overflow=(1, 1, 8.0), long_rows=(1, 1, -1.0))
    assert list(groups.items()) == [(b"", (2, 1, -0.25)), (b"ab", (1, 0, 0.0)), (b"b", (3, 3, 1.5)),
                                    (b"\xff", (1, 1, 2.0))]  # bytewise, a prefix first
    res = st.finalize()
    assert [(r.total, r.non_null, r.distinct, r.matches, r.has_value) for r in res[:2]] == [(10, 4, 3, 9, 1),
                                                                                            (10, 7, 4, 7, 1)]
    assert (res[0].sum_i, res[0].sum_f) == (42, 42.0) and (res[1].sum_i, res[1].sum_f) == (0, 10.25)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 2 is not a GROUP_SUMS check"):
        st.group_sums(2)
    foreign = T.State.deserialize(sums_plan(), sums_blob())
    L, err, out = T.lib(), T._lib._Error(), T._lib.GroupSumsSummary()
    assert L.tgx_group_sums_get(plan.h, foreign.h, 0, C.byref(out), C.byref(err)) != 0  # a state of another plan
    # COUNT(col) = 0: the sum has no value
    none = T.State.deserialize(plan, sums_blob(first=wire.group_sums_state(4, 8, {3: (2, 0, 0)}, null_group=(1, 0, 0))))
    r = none.finalize()[0]
    assert (r.total, r.non_null, r.has_value, r.sum_i, r.sum_f) == (3, 0, 0, 0, 0.0)
    fresh = T.State(plan)
    assert fresh.group_sums(0) == (dict(seen=0, groups=0, is_float=False, counted=NOTHING, null_group=NOTHING,
                                        overflow=NOTHING, long_rows=NOTHING), {})
    assert fresh.finalize()[1].has_value == 0


def test_the_entries_call_follows_the_size_query_convention():
    plan = sums_plan()
    st = T.State.deserialize(plan, sums_blob())
    L, err = T.lib(), T._lib._Error()
    n, nb, kind = C.c_uint64(), C.c_uint64(), C.c_int32()
    assert L.tgx_group_sums_entries(plan.h, st.h, 1, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(kind), C.byref(err)) == 0
    assert (n.value, nb.value, kind.value) == (4, 4, 1)
    small = (T._lib.GroupSumEntry * 3)()
    buf = (C.c_uint8 * 8)()
    assert L.tgx_group_sums_entries(plan.h, st.h, 1, small, 3, C.byref(n), buf, 8, C.byref(nb), C.byref(kind), C.byref(err)) != 0
    assert b"entries holds 3 entries, 4 are needed" in err.msg and n.value == 4
    assert all(e.rows == 0 for e in small)  # nothing copied
    full = (T._lib.GroupSumEntry * 4)()
    assert L.tgx_group_sums_entries(plan.h, st.h, 1, full, 4, C.byref(n), buf, 3, C.byref(nb), C.byref(kind), C.byref(err)) != 0
    assert b"bytes holds 3 bytes, 4 are needed" in err.msg
    assert L.tgx_group_sums_entries(plan.h, st.h, 0, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(kind), C.byref(err)) == 0
    assert (n.value, nb.value, kind.value) == (3, 0, 0)
    ints = (T._lib.GroupSumEntry * 3)()
    assert L.tgx_group_sums_entries(plan.h, st.h, 0, ints, 3, C.byref(n), None, 0, C.byref(nb), C.byref(kind), C.byref(err)) == 0
    assert [(e.value, e.rows, e.non_null, e.sum_i, e.sum_f) for e in ints] == [(-1, 2, 2, -7, -7.0), (5, 3, 1, 40, 40.0),
                                                                                  (7, 4, 0, 0, 0.0)]


def test_blob_round_trip_and_merge_by_value():
    plan = sums_plan()
    blob = sums_blob()
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    # a task without keys -- without rows, with integer and with float sums -- beside one with keys
    for empty in (wire.group_sums_state(4, 8, {}), wire.group_sums_state(4, 8, {}, null_group=(3, 2, -5)),
                  wire.group_sums_state(4, 8, {}, is_float=True, null_group=(3, 2, 0.5))):
        assert T.State.deserialize(plan, sums_blob(first=empty)).serialize() == sums_blob(first=empty)
    ints_f = wire.group_sums_state(4, 8, {5: (3, 1, 0.5), -1: (2, 2, -7.25)}, is_float=True)  # float sums by integer keys
    assert T.State.deserialize(plan, sums_blob(first=ints_f)).serialize() == sums_blob(first=ints_f)
    big = (1 << 63) - 1
    other = sums_blob(wire.group_sums_state(4, 8, {7: (1, 1, big), 9: (5, 2, big)}),
                      wire.group_sums_state(100, 16, {b"b": (1, 0, 0.0), b"c": (2, 2, 0.5)}, is_float=True,
                                            null_group=(1, 1, 4.0)))
    st.merge([T.State.deserialize(plan, other), T.State.deserialize(plan, other), T.State.deserialize(plan, blob)])
    summary, groups = st.group_sums(0)
    # 9: 2 * INT64_MAX wraps to -2
    assert groups == {-1: (4, 4, -14), 5: (6, 2, 80), 7: (10, 2, -2), 9: (10, 4, -2)}
    assert (summary["groups"], summary["seen"], summary["null_group"]) == (4, 32, (2, 2, 18))
    assert summary["counted"] == (30, 12, 62)
    summary, groups = st.group_sums(1)
    assert groups == {b"": (4, 2, -0.5), b"ab": (2, 0, 0.0), b"b": (8, 6, 3.0), b"c": (4, 4, 1.0), b"\xff": (2, 2, 4.0)}
    assert summary == dict(seen=28, groups=5, is_float=True, counted=(20, 14, 7.5), null_group=(4, 2, 8.0),
                           overflow=(2, 2, 16.0), long_rows=(2, 2, -2.0))
    again = T.State.deserialize(plan, st.serialize())  # equal states, equal bytes
    assert again.serialize() == st.serialize() and again.group_sums(1) == st.group_sums(1)
    st.reset()
    assert st.group_sums(1)[1] == {} and st.group_sums(1)[0]["seen"] == 0


def test_non_finite_float_sums_travel_in_blobs_and_merges():
    plan = sums_plan()
    inf, nan = float("inf"), float("nan")
    a = T.State.deserialize(plan, sums_blob(second=wire.group_sums_state(100, 16, {b"i": (1, 1, inf), b"n": (1, 1, nan),
                                                                                     b"z": (1, 1, -0.0)}, is_float=True)))
    b = T.State.deserialize(plan, sums_blob(second=wire.group_sums_state(100, 16, {b"i": (1, 1, -inf), b"n": (1, 1, 1.0),
                                                                                     b"z": (1, 1, -0.0)}, is_float=True)))
    assert struct.pack("<d", a.group_sums(1)[1][b"z"][2]) == struct.pack("<d", -0.0)  # the blob's bits
    a.merge([b])
    groups = a.group_sums(1)[1]
    assert groups[b"i"][2] != groups[b"i"][2] and groups[b"n"][2] != groups[b"n"][2]  # inf - inf, NaN + 1
    assert groups[b"z"][:2] == (2, 2)


def test_integer_and_string_keys_and_integer_and_float_sums_do_not_merge():
    plan = sums_plan()
    a = T.State.deserialize(plan, sums_blob())
    b = T.State.deserialize(plan, sums_blob(first=wire.group_sums_state(4, 8, {b"x": (3, 1, 5)})))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS task 0.*different group column types"):
        a.merge([b])
    c = T.State.deserialize(plan, sums_blob(first=wire.group_sums_state(4, 8, {5: (3, 1, 5.0)}, is_float=True)))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS task 0.*different value column types"):
        a.merge([c])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS task 0.*different value column types"):
        c.merge([a])
    no_keys = T.State.deserialize(plan, sums_blob(first=wire.group_sums_state(4, 8, {}, null_group=(3, 2, 11))))
    a.merge([no_keys])  # (a state without keys merges with either kind of key)
    assert a.group_sums(0)[0]["seen"] == 13 and a.group_sums(0)[0]["null_group"] == (4, 3, 20)
    empty = T.State.deserialize(plan, sums_blob(first=wire.group_sums_state(4, 8, {})))
    c.merge([empty])  # (and a state without rows with either kind of sum)
    empty.merge([c])
    assert empty.group_sums(0) == c.group_sums(0) and c.group_sums(0)[0]["is_float"] is True


def raw_task(max_groups, mvb, kind, values, seen, classes, entries, n=None):
    """classes: rows, non_null, sum of the NULL group, of overflow, of the long rows"""
    out = struct.pack("<4I11Q", max_groups, mvb, kind, values, seen, *classes, len(entries) if n is None else n)
    for k, t, nn, s in entries:
        out += (struct.pack("<I", len(k)) + k if isinstance(k, bytes) else struct.pack("<q", k)) + struct.pack("<QQQ", t, nn, s)
    return out


NONE = (0,) * 9
MALFORMED = [
    ("other parameters", raw_task(5, 8, 1, 1, 3, NONE, [(1, 3, 0, 0)]), None),
    ("other parameters", None, raw_task(100, 17, 2, 2, 3, NONE, [(b"a", 3, 0, 0)])),
    ("non_null > rows", raw_task(4, 8, 1, 1, 7, NONE, [(5, 3, 4, 1), (7, 4, 0, 0)]), None),
    ("non_null > rows", None, raw_task(100, 16, 2, 2, 3, NONE, [(b"a", 3, 2**64 - 1, 0)])),
    ("a sum without a value", raw_task(4, 8, 1, 1, 7, NONE, [(5, 3, 0, 1), (7, 4, 0, 0)]), None),
    ("zero count", raw_task(4, 8, 1, 1, 3, NONE, [(5, 3, 0, 0), (7, 0, 0, 0)]), None),
    ("out of order or repeated", raw_task(4, 8, 1, 1, 7, NONE, [(7, 3, 0, 0), (5, 4, 0, 0)]), None),
    ("out of order or repeated", raw_task(4, 8, 1, 1, 7, NONE, [(5, 3, 0, 0), (5, 4, 0, 0)]), None),
    ("out of order or repeated", None, raw_task(100, 16, 2, 2, 7, NONE, [(b"b", 3, 0, 0), (b"ab", 4, 0, 0)])),
    ("out of order or repeated", None, raw_task(100, 16, 2, 2, 7, NONE, [(b"", 3, 0, 0), (b"", 4, 0, 0)])),
    ("a key of 17 bytes, max_value_bytes is 16", None, raw_task(100, 16, 2, 2, 3, NONE, [(b"x" * 17, 3, 0, 0)])),
    ("!= seen", raw_task(4, 8, 1, 1, 8, NONE, [(5, 3, 0, 0), (7, 4, 0, 0)]), None),                # counted 7, seen 8
    ("!= seen", raw_task(4, 8, 1, 1, 7, (1, 0, 0) + (0,) * 6, [(5, 3, 0, 0), (7, 4, 0, 0)]), None),  # the NULL group on top
    ("!= seen", None, raw_task(100, 16, 2, 2, 9, (0, 0, 0, 1, 0, 0, 2, 0, 0), [(b"a", 7, 0, 0)])),  # 7 + 1 + 2 != 9
    ("non_null > rows", raw_task(4, 8, 1, 1, 9, (2, 3, 0) + (0,) * 6, [(5, 3, 0, 0), (7, 4, 0, 0)]), None),
    ("non_null > rows", raw_task(4, 8, 1, 1, 9, (0, 0, 0, 2, 3, 0, 0, 0, 0), [(5, 3, 0, 0), (7, 4, 0, 0)]), None),
    ("non_null > rows", None, raw_task(100, 16, 2, 2, 9, (0,) * 6 + (2, 3, 0), [(b"a", 7, 0, 0)])),
    ("a sum without a value", raw_task(4, 8, 1, 1, 9, (2, 0, 5) + (0,) * 6, [(5, 3, 0, 0), (7, 4, 0, 0)]), None),
    ("kind", raw_task(4, 8, 3, 1, 0, NONE, []), None),
    ("kind", raw_task(4, 8, 1, 3, 3, NONE, [(5, 3, 0, 0)]), None),                              # an unknown kind of sum
    ("kind", raw_task(4, 8, 1, 0, 3, NONE, [(5, 3, 0, 0)]), None),                              # rows without a kind of sum
    ("kind", raw_task(4, 8, 0, 1, 3, NONE, [], n=1), None),                                     # entries without a kind
    ("counts", raw_task(4, 8, 1, 1, 10, NONE, [(5, 2**64 - 1, 0, 0), (7, 2, 0, 0)]), None),     # a count that wraps
]


@pytest.mark.parametrize("what,first,second", MALFORMED)
def test_malformed_blobs_are_refused(what, first, second):
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + what):
        T.State.deserialize(sums_plan(), sums_blob(first, second))


def test_truncated_and_foreign_blobs_are_refused():
    plan, blob = sums_plan(), sums_blob()
    for cut in (1, 8, 16, 17, 40, len(blob) - 60):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plan, sums_blob(first=raw_task(4, 8, 1, 1, 3, NONE, [(5, 3, 0, 0)], n=2**60)))
    other = T.Plan([spec(T.GROUP_SUMS, 0, column2=1), spec(T.COUNT, 0)])
    other.set_group_sums(0, 4, 8)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different plan"):
        T.State.deserialize(other, blob)
    # a GROUP_COUNTS section is not a GROUP_SUMS section
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different plan"):
        T.State.deserialize(plan, wire.pack(count=[wire.count_acc(10, 4)],
                                            group_counts=[wire.group_counts_state(4, 8, {}), wire.group_counts_state(100, 16, {})]))


def test_the_section_follows_the_group_counts_section():
    plan = T.Plan([spec(T.GROUP_SUMS, 0, column2=1), spec(T.GROUP_COUNTS, 0, column2=1)])
    plan.set_group_sums(0, 4, 8)
    plan.set_group_counts(1, 4, 8)
    blob = wire.pack(group_counts=[wire.group_counts_state(4, 8, {1: (2, 1)})],
                     group_sums=[wire.group_sums_state(4, 8, {1: (2, 1, -5)})])
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    assert st.group_sums(0)[1] == {1: (2, 1, -5)} and st.group_counts(1)[1] == {1: (2, 1)}


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0)])
    blob = wire.pack(count=[wire.count_acc(10, 9)])
    assert T.State.deserialize(plan, blob).serialize() == blob  # (the blob version stays 3: no section, no bytes)
    assert wire.VERSION == 3
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, column2=1)])
    plan.set_group_counts(0, 4, 8)
    blob = wire.pack(group_counts=[wire.group_counts_state(4, 8, {1: (2, 1)})])
    assert T.State.deserialize(plan, blob).serialize() == blob


# ---- the host layer: CrossTableSumConstraint ------------------------------------------------------------------------------------
import json  # noqa: E402
import math  # noqa: E402

import exact_group_sums as ex  # noqa: E402
import term_amd.suite as S  # noqa: E402
from test_exact_group_sums import golden_cases, golden_side  # noqa: E402


def side_json(sums):
    """exact_group_sums.side_sums() as tgx_host_cross_table_sum_json takes a side"""
    if not isinstance(sums, dict):
        return sums
    keys = sorted(k for k in sums if k is not None)
    return {"groups": [[k.decode() if isinstance(k, bytes) else k, sums[k]] for k in keys], "null_group": sums.get(None)}


def suite_of(constraint, level=S.Level.ERROR):
    return S.ValidationSuite.builder("s").check(S.Check.builder("c").level(level).constraint(constraint).build()).build()


def test_the_constraints_name_getters_and_json_round_trip():
    c = S.CrossTableSumConstraint("orders.total", "payments.amount")
    assert c.name() == "cross_table_sum" and S.constraint_plan(c.spec) == {"name": "cross_table_sum", "requests": []}
    assert c.spec == {"type": "cross_table_sum", "left_column": "orders.total", "right_column": "payments.amount",
                      "group_by": [], "tolerance": 0.0, "max_violations_reported": 100, "max_groups": 65536}
    assert (c.left_column(), c.right_column(), c.group_by_columns()) == ("orders.total", "payments.amount", [])
    c.group_by(["customer_id"]).tolerance(-0.25).max_violations_reported(7).max_groups(500)  # (tolerance: its magnitude)
    config = c.verdict_from_sums({"groups": []}, {"groups": []})["config"]  # what the C++ object's getters answer
    assert config == {"name": "cross_table_sum", "left_column": "orders.total", "right_column": "payments.amount",
                      "group_by": ["customer_id"], "tolerance": 0.25, "max_violations_reported": 7, "max_groups": 500}
    assert S.CrossTableSumConstraint("a.b", "c.d").group_by("g").group_by_columns() == ["g"]
    built = S.Check.builder("c").cross_table_sum("orders.total", "payments.amount").build()
    assert built.spec["constraints"] == [S.CrossTableSumConstraint("orders.total", "payments.amount").spec]
    assert json.loads(json.dumps(c.spec)) == c.spec


def test_qualified_name_errors_are_the_references():
    for bad in ("orders", "a.b.c", "", "x"):
        with pytest.raises(T.TgxError, match=r"Constraint evaluation failed for 'cross_table_sum': Column must be qualified "
                                             r"\(table.column\): '%s'" % bad):
            S.CrossTableSumConstraint(bad, "p.a").verdict_from_sums(1.0, 2.0)
        with pytest.raises(ValueError):
            ex.parse_qualified(bad)
    with pytest.raises(T.TgxError, match="Security error: Invalid SQL identifier format: 'b;'"):
        S.CrossTableSumConstraint("p.a", "a.b;").verdict_from_sums(1.0, 2.0)
    with pytest.raises(T.TgxError, match="Security error: SQL identifier cannot be empty"):
        S.CrossTableSumConstraint(".x", "p.a").verdict_from_sums(1.0, 2.0)
    # through a suite the error is the constraint's issue, as an Err from evaluate() reads
    r = suite_of(S.CrossTableSumConstraint("orders", "payments.amount")).run(None, tables={})
    assert [(i.constraint_name, i.message) for i in r.report.issues] == [
        ("cross_table_sum", "Error evaluating constraint: Constraint evaluation failed for 'cross_table_sum': Column must "
                            "be qualified (table.column): 'orders'")]
    assert r.is_failure()


def test_errors_that_need_no_device():
    def issue(constraint, tables=None):
        r = suite_of(constraint, S.Level.WARNING).run(None, tables=tables or {})
        assert r.is_success() and len(r.report.issues) == 1 and r.report.metrics.failed_checks == 1
        return r.report.issues[0].message
    head = "Error evaluating constraint: Constraint evaluation failed for 'cross_table_sum': "
    c = S.CrossTableSumConstraint("orders.total", "payments.amount")
    assert issue(c) == head + ("Cross-table sum validation query failed: Error during planning: table "
                               "'datafusion.public.orders' not found")
    import pyarrow as pa
    orders = pa.table({"id": pa.array([1], pa.int64())})
    assert issue(c, {"orders": orders}) == head + "Cross-table sum validation query failed: Schema error: No field named total."
    msg = issue(S.CrossTableSumConstraint("orders.id", "orders.id").group_by(["g"]), {"orders": orders})
    assert msg == head + "Cross-table sum validation query failed: Schema error: No field named g."
    msg = issue(S.CrossTableSumConstraint("orders.id", "orders.id").group_by(["a", "b"]), {"orders": orders})
    assert msg.startswith(head + "GROUP BY over 2 columns is not on the GPU path")
    msg = issue(S.CrossTableSumConstraint("orders.id", "orders.id").group_by(["a;"]), {"orders": orders})
    assert msg.startswith("Error evaluating constraint: Security error: Invalid SQL identifier format: 'a;'")
    for bad in (0, 65537):
        msg = issue(S.CrossTableSumConstraint("orders.id", "orders.id").group_by(["id"]).max_groups(bad), {"orders": orders})
        assert msg == head + "max_groups must be 1 .. 65536 (%d)" % bad


def test_both_message_shapes_from_injected_sums():
    c = S.CrossTableSumConstraint("orders.total", "payments.amount")
    v = c.verdict_from_sums(100.005, 100.001)
    assert (v["status"], v["metric"], v["total_groups"], v["violating_groups"]) == ("failure", abs(100.005 - 100.001), 1, 1)
    assert v["message"] == ("Cross-table sum mismatch: 1/1 overall totals failed validation (exact match required). Examples: "
                            "[Group 'ALL': orders.total = 100.0050, payments.amount = 100.0010 (diff: 0.0040)]")
    assert v["message"] == ex.cross_table_sum(100.005, 100.001)["message"]
    v = c.tolerance(0.001).max_violations_reported(0).verdict_from_sums(2.5, 1.0)
    assert v["message"] == ("Cross-table sum mismatch: 1/1 overall totals failed validation (tolerance: 0.0010), total sums: "
                            "2.5 vs 1 (max diff: 1.5000)")
    ok = c.tolerance(1.5).verdict_from_sums(2.5, 1.0)  # ABS(l - r) > tolerance: equality passes
    assert (ok["status"], ok["metric"], ok["message"]) == ("success", 1.5, None)
    g = S.CrossTableSumConstraint("o.t", "p.a").group_by(["region"]).tolerance(0.5)
    left = {"groups": [["eu", 10.0], ["us", 4611686018427387904.0]], "null_group": 3.0}
    right = {"groups": [["asia", 2.0], ["eu", 10.25]], "null_group": None}
    v = g.verdict_from_sums(left, right)
    want = ex.cross_table_sum({b"eu": 10.0, b"us": 2.0**62, None: 3.0}, {b"asia": 2.0, b"eu": 10.25}, 0.5, ["region"])
    assert v["message"] == want["message"] == (
        "Cross-table sum mismatch: 3/4 groups by [region] failed validation (tolerance: 0.5000), total sums: "
        "4611686018427388000 vs 12.25 (max diff: 4611686018427387904.0000)")
    assert {k: v[k] for k in ("total_groups", "violating_groups", "total_left_sum", "total_right_sum", "max_difference")} == \
        {k: want[k] for k in ("total_groups", "violating_groups", "total_left_sum", "total_right_sum", "max_difference")}


def test_non_finite_sums_from_injected_sums():
    g = S.CrossTableSumConstraint("o.t", "p.a").group_by(["k"])
    v = g.verdict_from_sums({"groups": [[1, math.nan], [2, 5.0]]}, {"groups": [[1, 1.0], [2, 1.0]]})
    want = ex.cross_table_sum({1: math.nan, 2: 5.0}, {1: 1.0, 2: 1.0}, group_by_columns=["k"])
    assert v["violating_groups"] == want["violating_groups"] == 1 and math.isnan(v["max_difference"]) and math.isnan(v["metric"])
    assert v["message"] == want["message"] and v["message"].endswith("total sums: NaN vs 2 (max diff: NaN)")
    v = g.verdict_from_sums({"groups": [[1, math.nan]]}, {"groups": [[1, 1.0]]})  # NaN > tolerance is false
    assert v["status"] == "success" and math.isnan(v["metric"])
    v = g.verdict_from_sums({"groups": [[1, math.inf]]}, {"groups": [[1, 1.0]]})
    assert v["status"] == "failure" and v["max_difference"] == math.inf and v["message"].endswith("inf vs 1 (max diff: inf)")


def test_bounds_and_key_kinds_are_errors_not_verdicts():
    g = S.CrossTableSumConstraint("o.t", "p.a").group_by(["k"]).max_groups(10)
    with pytest.raises(T.TgxError, match=r"'cross_table_sum': the left side has more groups than the bound max_groups = 10 "
                                         r"\(keys of at most 256 bytes\) holds: 3 overflow rows, 0 rows with a longer key"):
        g.verdict_from_sums({"groups": [[1, 1.0]], "overflow_rows": 3}, {"groups": [[1, 1.0]]})
    with pytest.raises(T.TgxError, match="the right side has more groups than the bound max_groups = 10.*2 rows with a longer key"):
        g.verdict_from_sums({"groups": [[1, 1.0]]}, {"groups": [[1, 1.0]], "long_rows": 2})
    with pytest.raises(T.TgxError, match="must both be integer or both be string columns"):
        g.verdict_from_sums({"groups": [[1, 1.0]]}, {"groups": [["1", 1.0]]})
    assert g.verdict_from_sums({"groups": []}, {"groups": [["1", 1.0]]})["total_groups"] == 1  # (a side without keys joins either)
    with pytest.raises(T.TgxError, match="a grouped constraint takes two sides of groups"):
        g.verdict_from_sums(1.0, 2.0)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_the_golden_vectors_through_the_host_layers_join(case):
    sides = [side_json(ex.side_sums(*golden_side(s, case["group_by"]))) for s in (case["left"], case["right"])]
    c = S.CrossTableSumConstraint("%s.%s" % (case["left"]["table"], case["left"]["column"]),
                                  "%s.%s" % (case["right"]["table"], case["right"]["column"]))
    c.group_by(case["group_by"]).tolerance(case["tolerance"]).max_violations_reported(case.get("max_violations_reported", 100))
    got = c.verdict_from_sums(*sides)
    assert {k: got[k] for k in case["expect"]} == case["expect"] and got["metric"] == case["expect"]["max_difference"]
