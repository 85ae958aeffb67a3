"""TGX_CHECK_KEY_PROBE and ForeignKeyConstraint without a device: plan validation, what a host-only state answers from a
blob, merging by value and by parent set, every malformed-blob refusal of the KPRB section (term_amd/wire.py), the JSON
form of the constraint, and every verdict and message branch through tgx_host_foreign_key_json, held against
tests/exact_key_probe.py and the golden vectors."""
import ctypes as C
import json
import os
import re
import struct

import pytest

import exact_key_probe as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

MISSING = {5: 3, -1: 2, 7: 4}
PARENT = (40, 0x1234567890ABCDEF)
HERE = os.path.dirname(os.path.abspath(__file__))


def probe_plan(second=100):
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 1), spec(T.COUNT, 0)])
    plan.set_key_probe(0, 4)
    plan.set_key_probe(1, second)
    return plan


def probe_blob(first=None, second=None):
    first = wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT) if first is None else first
    second = wire.key_probe_state(100, {9: 1}, matched=2, overflow_rows=3, parent=(0, 0)) if second is None else second
    return wire.pack(count=[wire.count_acc(20, 19)], key_probes=[first, second])


def read(st, i):
    summary, entries = st.key_probe(i)
    assert summary["seen"] == summary["non_null"] + summary["null_rows"]
    assert summary["non_null"] == summary["matched"] + summary["missing_rows"]
    assert summary["missing_rows"] == summary["counted"] + summary["overflow_rows"]
    return summary, entries


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def test_abi_constants():
    assert T.KEY_PROBE == 19 and T.KEY_PROBE_MAX_MISSING_KEYS == 65536
    for name in ("tgx_plan_set_key_probe", "tgx_key_probe_set_parent", "tgx_key_probe_get", "tgx_key_probe_entries",
                 "tgx_host_foreign_key_json"):
        assert name in T.abi_symbols()
    assert all(hasattr(T.lib(), n) for n in ("tgx_plan_set_key_probe", "tgx_key_probe_set_parent", "tgx_key_probe_get"))
    assert C.sizeof(T._lib.KeyProbeSummary) == 88 and C.sizeof(T._lib.KeyProbeEntry) == 16


def test_parameters_are_validated():
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.COUNT, 0)])
    for bad in (0, 65537, 2**32 - 1):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_missing_keys must be 1 \.\. 65536 \(%d\)" % bad):
            plan.set_key_probe(0, bad)
    with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*reserved must be 0 \(7\)"):
        plan.set_key_probe(0, 10, reserved=7)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1 is not a KEY_PROBE check"):
        plan.set_key_probe(1, 10)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*KEY_PROBE reads one column: column2 must be -1"):
        T.Plan([spec(T.KEY_PROBE, 0, column2=1)])
    for ok in (1, 65536):
        plan.set_key_probe(0, ok)


def test_a_plan_that_is_not_ready_fails_state_create_and_deserialize():
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 0)])
    plan.set_key_probe(0, 10)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*tgx_plan_set_key_probe"):
        T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_plan_set_key_probe"):
        T.State.deserialize(plan, wire.pack(key_probes=[wire.key_probe_state(10)] * 2))


def test_the_setter_is_refused_after_the_first_state():
    plan = probe_plan()
    st = T.State.deserialize(plan, probe_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_key_probe(0, 5)
    del st


# ---- a host-only state ------------------------------------------------------------------------------------------------------
def test_a_host_only_state_answers_its_blob():
    plan = probe_plan()
    st = T.State.deserialize(plan, probe_blob())
    summary, entries = read(st, 0)
    assert summary == dict(seen=20, non_null=19, null_rows=1, matched=10, missing_rows=9, counted=9, overflow_rows=0,
                           missing_keys=3, parent_keys=PARENT[0], parent_digest=PARENT[1], route=0)
    assert list(entries.items()) == [(-1, 2), (5, 3), (7, 4)]  # ascending int64
    summary, entries = read(st, 1)
    assert summary == dict(seen=6, non_null=6, null_rows=0, matched=2, missing_rows=4, counted=1, overflow_rows=3,
                           missing_keys=1, parent_keys=0, parent_digest=0, route=0)
    res = st.finalize()
    assert [(r.total, r.non_null, r.matches, r.distinct) for r in res[:2]] == [(20, 19, 10, 3), (6, 6, 2, 1)]


def test_getters_on_a_spec_of_another_kind_and_a_state_of_another_plan():
    plan, other = probe_plan(), probe_plan()
    st = T.State.deserialize(plan, probe_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 2 is not a KEY_PROBE check"):
        st.key_probe(2)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 9 is not a KEY_PROBE check"):
        st.key_probe(9)
    L, err = T.lib(), T._lib._Error()
    out, n = T._lib.KeyProbeSummary(), C.c_uint64()
    assert L.tgx_key_probe_get(other.h, st.h, 0, C.byref(out), C.byref(err)) != 0 and b"bad arguments" in err.msg
    assert L.tgx_key_probe_entries(other.h, st.h, 0, None, 0, C.byref(n), C.byref(err)) != 0 and b"bad arguments" in err.msg
    assert L.tgx_key_probe_set_parent(other.h, st.h, 0, None, 0, C.byref(err)) != 0 and b"bad arguments" in err.msg
    assert L.tgx_key_probe_get(plan.h, st.h, 0, None, C.byref(err)) != 0
    assert L.tgx_key_probe_entries(plan.h, st.h, 0, None, 0, None, C.byref(err)) != 0


def test_the_entries_call_follows_the_size_query_convention():
    plan = probe_plan()
    st = T.State.deserialize(plan, probe_blob())
    L, err, n = T.lib(), T._lib._Error(), C.c_uint64()
    assert L.tgx_key_probe_entries(plan.h, st.h, 0, None, 0, C.byref(n), C.byref(err)) == 0 and n.value == 3
    small = (T._lib.KeyProbeEntry * 2)()
    assert L.tgx_key_probe_entries(plan.h, st.h, 0, small, 2, C.byref(n), C.byref(err)) != 0
    assert b"entries holds 2 entries, 3 are needed" in err.msg and n.value == 3
    full = (T._lib.KeyProbeEntry * 3)()
    assert L.tgx_key_probe_entries(plan.h, st.h, 0, full, 3, C.byref(n), C.byref(err)) == 0
    assert [(e.value, e.count) for e in full] == [(-1, 2), (5, 3), (7, 4)]


def test_blob_round_trip_and_merge_by_value():
    plan = probe_plan()
    blob = probe_blob()
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    # a task that knows of no set, and one that knows an empty one, beside a counted one
    for first in (wire.key_probe_state(4), wire.key_probe_state(4, parent=(0, 0)), wire.key_probe_state(4, nulls=3, parent=PARENT)):
        assert T.State.deserialize(plan, probe_blob(first=first)).serialize() == probe_blob(first=first)
    other = probe_blob(wire.key_probe_state(4, {7: 1, 9: 5}, matched=1, parent=PARENT),
                       wire.key_probe_state(100, {8: 2}, nulls=1, parent=(0, 0)))
    st.merge([T.State.deserialize(plan, other), T.State.deserialize(plan, blob)])
    summary, entries = read(st, 0)
    assert entries == {-1: 4, 5: 6, 7: 9, 9: 5} and (summary["seen"], summary["matched"], summary["null_rows"]) == (47, 21, 2)
    assert (summary["parent_keys"], summary["parent_digest"]) == PARENT
    summary, entries = read(st, 1)
    assert entries == {8: 2, 9: 2} and summary["overflow_rows"] == 6 and summary["null_rows"] == 1
    again = T.State.deserialize(plan, st.serialize())  # equal states, equal bytes
    assert again.serialize() == st.serialize() and again.key_probe(0) == st.key_probe(0)
    # a state that knows of no set takes the identity of what is merged in
    fresh = T.State(plan)
    assert fresh.key_probe(0)[0]["parent_keys"] == 0
    fresh.merge([T.State.deserialize(plan, blob)])
    assert fresh.serialize() == blob
    st.reset()
    assert read(st, 0) == (dict(seen=0, non_null=0, null_rows=0, matched=0, missing_rows=0, counted=0, overflow_rows=0,
                                missing_keys=0, parent_keys=0, parent_digest=0, route=0), {})


def test_states_of_different_parent_sets_do_not_merge():
    plan = probe_plan()
    a = T.State.deserialize(plan, probe_blob())
    for parent in ((PARENT[0] + 1, PARENT[1]), (PARENT[0], PARENT[1] ^ 1), (0, 0)):
        b = T.State.deserialize(plan, probe_blob(first=wire.key_probe_state(4, {5: 1}, parent=parent)))
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*KEY_PROBE task 0.*different parent sets"):
            a.merge([b])
    a.merge([T.State.deserialize(plan, probe_blob(first=wire.key_probe_state(4)))])  # (no set known: merges with any)
    assert read(a, 0)[0]["seen"] == 20


def test_a_deserialized_state_takes_no_batch():
    """it holds no parent set (where there is no device either, tgx_update says that first); what it holds stays"""
    import numpy as np

    plan = probe_plan()
    st = T.State.deserialize(plan, probe_blob())
    cols = [T.Column.int64(np.arange(4, dtype=np.int64)), T.Column.int64(np.arange(4, dtype=np.int64))]
    with pytest.raises(T.TgxError, match="TGX_NO_DEVICE|TGX_INVALID_ARGUMENT.*spec 0.*needs its parent set"):
        st.update(cols)
    assert read(st, 0)[0]["seen"] == 20 and st.serialize() == probe_blob()


def raw_task(bound, reserved, known, pad, keys, digest, seen, non_null, matched, overflow, entries, n=None):
    out = struct.pack("<4I7Q", bound, reserved, known, pad, keys, digest, seen, non_null, matched, overflow,
                      len(entries) if n is None else n)
    for v, c in entries:
        out += struct.pack("<qQ", v, c)
    return out


MALFORMED = [
    ("other parameters", raw_task(5, 0, 1, 0, 1, 2, 3, 3, 0, 0, [(1, 3)]), None),
    ("other parameters", raw_task(4, 1, 1, 0, 1, 2, 3, 3, 0, 0, [(1, 3)]), None),
    ("other parameters", None, raw_task(101, 0, 1, 0, 1, 2, 3, 3, 0, 0, [(1, 3)])),
    ("out of order or repeated", raw_task(4, 0, 1, 0, 1, 2, 7, 7, 0, 0, [(7, 3), (5, 4)]), None),
    ("out of order or repeated", raw_task(4, 0, 1, 0, 1, 2, 7, 7, 0, 0, [(5, 3), (5, 4)]), None),
    ("zero count", raw_task(4, 0, 1, 0, 1, 2, 3, 3, 0, 0, [(5, 3), (7, 0)]), None),
    ("!= non_null", raw_task(4, 0, 1, 0, 1, 2, 10, 8, 0, 0, [(5, 3), (7, 4)]), None),   # counted 7, non_null 8
    ("!= non_null", raw_task(4, 0, 1, 0, 1, 2, 10, 7, 1, 0, [(5, 3), (7, 4)]), None),   # matched on top
    ("!= non_null", raw_task(4, 0, 1, 0, 1, 2, 10, 7, 0, 1, [(5, 3), (7, 4)]), None),   # overflow on top
    ("!= non_null", raw_task(4, 0, 1, 0, 1, 2, 6, 7, 0, 0, [(5, 3), (7, 4)]), None),    # non_null above seen
    ("!= non_null", raw_task(4, 0, 1, 0, 1, 2, 2**64 - 1, 5, 2**64 - 2, 0, [(5, 7)]), None),  # a sum that wraps
    ("parent set", raw_task(4, 0, 2, 0, 1, 2, 0, 0, 0, 0, []), None),                   # known is 0 or 1
    ("parent set", raw_task(4, 0, 1, 9, 1, 2, 0, 0, 0, 0, []), None),                   # padding
    ("parent set", raw_task(4, 0, 0, 0, 1, 0, 0, 0, 0, 0, []), None),                   # an identity without a set
    ("parent set", raw_task(4, 0, 0, 0, 0, 0, 3, 0, 0, 0, []), None),                   # rows without a set
    ("counts", raw_task(4, 0, 1, 0, 1, 2, 10, 9, 0, 0, [(5, 2**64 - 1), (7, 2)]), None),
]


@pytest.mark.parametrize("what,first,second", MALFORMED, ids=["%d-%s" % (i, m[0][:12]) for i, m in enumerate(MALFORMED)])
def test_malformed_blobs_are_refused(what, first, second):
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + re.escape(what)):
        T.State.deserialize(probe_plan(), probe_blob(first, second))


def test_truncated_and_foreign_blobs_are_refused():
    plan, blob = probe_plan(), probe_blob()
    for cut in (1, 8, 9, 20, 60, 100, 150):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):  # an entry count far beyond the blob's bytes
        T.State.deserialize(plan, probe_blob(first=raw_task(4, 0, 1, 0, 1, 2, 3, 3, 0, 0, [(5, 3)], n=2**60)))
    other = T.Plan([spec(T.KEY_PROBE, 0), spec(T.COUNT, 0)])
    other.set_key_probe(0, 4)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different plan"):
        T.State.deserialize(other, blob)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):  # another kind's section where KPRB belongs
        T.State.deserialize(plan, wire.pack(count=[wire.count_acc(20, 19)],
                                            value_counts=[wire.value_counts_state(4, 8, 0, {})] * 2))


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0), spec(T.VALUE_COUNTS, 0)])
    plan.set_value_counts(1, 4, 8)
    blob = wire.pack(count=[wire.count_acc(10, 9)], value_counts=[wire.value_counts_state(4, 8, 10, {5: 9}, nulls=1)])
    assert T.State.deserialize(plan, blob).serialize() == blob
    # and the section stands behind every other kind's
    both = T.Plan([spec(T.KEY_PROBE, 0), spec(T.VALUE_COUNTS, 0)])
    both.set_key_probe(0, 4)
    both.set_value_counts(1, 4, 8)
    blob = wire.pack(value_counts=[wire.value_counts_state(4, 8, 10, {5: 9}, nulls=1)],
                     key_probes=[wire.key_probe_state(4, MISSING, parent=PARENT)])
    assert T.State.deserialize(both, blob).serialize() == blob and blob.index(b"KPRB") > blob.index(b"VCNT")


# ---- the constraint -----------------------------------------------------------------------------------------------------------
def counts_of(state, examples=True):
    return {"null_rows": state["null_rows"], "missing_rows": state["missing_rows"], "overflow_rows": state["overflow_rows"],
            "missing_keys": state["missing_keys"], "entries": [[k, c] for k, c in state["entries"].items()],
            "examples": examples}


def verdict(c, state, examples=True):
    v = c.verdict_from_counts(counts_of(state, examples))
    return v["status"], v["metric"], v["message"]


def test_the_json_form_and_the_builders():
    c = S.ForeignKeyConstraint("orders.customer_id", "customers.id")
    assert c.name() == "foreign_key" and c.spec == {
        "type": "foreign_key", "child_column": "orders.customer_id", "parent_column": "customers.id", "allow_nulls": False,
        "use_left_join": True, "max_violations_reported": 100, "max_missing_keys": 10000}
    c.allow_nulls(True).use_left_join(False).max_violations_reported(50).max_missing_keys(77)
    config = c.verdict_from_counts({"null_rows": 0, "missing_rows": 0, "overflow_rows": 0, "entries": []})["config"]
    assert config == {"name": "foreign_key", "child_column": "orders.customer_id", "parent_column": "customers.id",
                      "allow_nulls": True, "use_left_join": False, "max_violations_reported": 50, "max_missing_keys": 77}
    built = S.Check.builder("c").foreign_key("a.b", "c.d").build()
    assert built.spec["constraints"] == [S.ForeignKeyConstraint("a.b", "c.d").spec]
    # the defaults of a bare JSON object are the reference's
    bare = C.c_char_p()
    err = S._Error()
    assert S._host().tgx_host_foreign_key_json(b'{"type": "foreign_key", "child_column": "a.b", "parent_column": "c.d"}',
                                               b'{"null_rows": 1}', C.byref(bare), C.byref(err)) == 0
    v = json.loads(S._take(bare))
    assert v["config"]["max_violations_reported"] == 100 and v["config"]["max_missing_keys"] == 10000
    assert (v["config"]["allow_nulls"], v["config"]["use_left_join"], v["status"], v["metric"]) == (False, True, "failure", 1)


@pytest.mark.parametrize("child,parent,what", [
    ("customer_id", "customers.id", "Foreign key column must be qualified (table.column): 'customer_id'"),
    ("orders.customer_id", "too.many.parts", "Foreign key column must be qualified (table.column): 'too.many.parts'"),
    ("orders.customer_id", "customers.id; DROP", "Security error"),
    ("ord ers.c", "customers.id", "Security error"),
])
def test_names_are_parsed_as_the_reference_parses_them(child, parent, what):
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + re.escape(what)):
        S.ForeignKeyConstraint(child, parent).verdict_from_counts({"missing_rows": 0})


def test_errors_of_the_json_entry_point():
    c = S.ForeignKeyConstraint("a.b", "c.d")
    for bad, what in (({"entries": [[2, 1], [1, 1]], "missing_rows": 2}, "ascending"),
                      ({"entries": [[1, 1], [1, 1]], "missing_rows": 2}, "ascending"),
                      ({"entries": [[1]], "missing_rows": 1}, "an entry is [key, count]"),
                      ({"entries": {"1": 1}}, "entries must be a JSON array"),
                      ({"entries": [[1, 2]], "missing_rows": 3}, "missing_rows the sum"),
                      ({"entries": [[1, 2]], "missing_rows": 2, "missing_keys": 2}, "missing_keys is the number of entries")):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + re.escape(what)):
            c.verdict_from_counts(bad)
    out, err = C.c_char_p(), S._Error()
    H = S._host()
    assert H.tgx_host_foreign_key_json(b'{"type": "completeness", "column": "x", "threshold": 1.0}', b"{}", C.byref(out), C.byref(err)) != 0
    assert b"not a foreign_key constraint" in err.msg
    assert H.tgx_host_foreign_key_json(json.dumps(c.spec).encode(), b"[1, 2", C.byref(out), C.byref(err)) != 0
    assert b"counts JSON" in err.msg
    assert H.tgx_host_foreign_key_json(None, b"{}", C.byref(out), C.byref(err)) != 0 and b"NULL argument" in err.msg


def test_every_verdict_and_message_branch():
    state = ex.walk(list(range(20)) * 2 + [0, 0], [True] * 40 + [False] * 2, [0, 1], None)
    c = lambda: S.ForeignKeyConstraint("orders.k", "customers.k")  # noqa: E731
    names = ("orders.k", "customers.k")
    # success: nothing missing, with and without NULL rows
    clean = ex.walk([0, 1, 1, 0], [True, True, True, False], [0, 1], None)
    assert verdict(c().allow_nulls(True), clean) == ("success", None, None) == ex.verdict(clean, *names, allow_nulls=True)
    assert verdict(c(), ex.walk([0, 1], None, [0, 1], None)) == ("success", None, None)
    # allow_nulls off: the NULL rows alone fail it, and there is nothing to list
    got = verdict(c(), clean)
    assert got == ex.verdict(clean, *names) and got[1] == 1 and got[2].endswith("(total: 1, unique: 0)")
    # no examples, up to 5, more than 5
    for reported in (0, 1, 5, 6, 17, 18, 100):
        got = verdict(c().max_violations_reported(reported), state)
        assert got == ex.verdict(state, *names, max_violations_reported=reported)
    assert "Examples" not in verdict(c().max_violations_reported(0), state)[2]
    assert verdict(c().max_violations_reported(5), state)[2].endswith(". Examples: [2, 3, 4, 5, 6]")
    assert verdict(c(), state)[2].endswith(". Examples: [2, 3, 4, 5, 6, ... (13 more)]")
    # allow_nulls on and off
    assert verdict(c(), state)[1] == 38 and verdict(c().allow_nulls(True), state)[1] == 36
    assert verdict(c().allow_nulls(True), state) == ex.verdict(state, *names, allow_nulls=True)
    # a child type the reference's collector does not read: no examples
    assert verdict(c(), state, examples=False) == ex.verdict(state, *names, examples=False)
    # overflow: the verdict and the metric stand, unique reads "at least", the examples come from the keys held
    over = dict(state, overflow_rows=4, missing_rows=state["missing_rows"] + 4)
    got = verdict(c(), over)
    assert got == ex.verdict(over, *names) and got[1] == 42 and "unique: at least 18). Examples: [2, 3, 4, 5, 6, ... (13 more)]" in got[2]
    # negative keys and the extremes print as integers
    wide = ex.walk([-2**63, 2**63 - 1, -1, 0], None, [0], None)
    assert verdict(c(), wide)[2].endswith("Examples: [-9223372036854775808, -1, 9223372036854775807]")


def golden_cases():
    with open(os.path.join(HERE, "golden", "foreign_key_vectors.json")) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", golden_cases(), ids=[c["name"] for c in golden_cases()])
def test_the_golden_vectors_verdicts(case):
    state = ex.walk([v or 0 for v in case["child"]], [v is not None for v in case["child"]],
                    [v or 0 for v in case["parent"]], [v is not None for v in case["parent"]])
    c = S.ForeignKeyConstraint(case["child_column"], case["parent_column"]).allow_nulls(case["allow_nulls"])
    status, metric, message = verdict(c, state)
    assert (status, metric, message) == ex.verdict(state, case["child_column"], case["parent_column"], case["allow_nulls"])
    assert (status, metric) == (case["status"], case["metric"])
    assert all(part in (message or "") for part in case["message_parts"])
