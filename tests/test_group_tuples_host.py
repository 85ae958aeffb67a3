"""GROUP BY several columns without a GPU: the plan shapes a TGX_CHECK_GROUP_COUNTS / TGX_CHECK_GROUP_SUMS spec with a
column list is accepted and refused in; the state blobs of tuple tasks (term_amd/wire.py) -- a host-only state answers
its blob, a blob of another arity or with keys that are no encoded tuples is refused, and the blob of a plan without
tuple tasks keeps its bytes; and the host layer with its opt-in: the grouped completeness analyzer's plan, state, merge
and metric map against tests/exact_group_counts.py's grouped_state, and CrossTableSumConstraint's join."""
import struct

import pytest

import exact_group_tuples as ext
import term_amd as T
from _lib_spec import spec
from term_amd import wire

E = ext.encode
COUNTS = {E((None, b"a")): (2, 1), E((b"", b"a")): (1, 1), E((None, None)): (3, 0), E((-1, b"zz")): (4, 4), E((5, None)): (1, 0)}
SUMS = {E((None, 7)): (2, 1, -5), E((-1, 7)): (4, 4, 2**63 - 1), E((b"k", None)): (1, 0, 0)}


# ---- plan shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [T.GROUP_COUNTS, T.GROUP_SUMS], ids=["counts", "sums"])
def test_a_column_list_without_column2_is_accepted_and_keeps_the_value_column(kind):
    s = spec(kind, 2, columns=[0, 1])
    assert (s.column, s.column2, s.n_columns) == (2, -1, 2)  # (the list does not overwrite the value column)
    plan = T.Plan([s, spec(kind, 0, columns=[0, 1, 2, 3, 4, 5, 6, 7]), spec(T.COUNT, 2)])
    setter = plan.set_group_counts if kind == T.GROUP_COUNTS else plan.set_group_sums
    setter(0, 100, 64)
    setter(1, 100, 64)
    st = T.State.deserialize(plan, T.State.deserialize(plan, blob_of(kind)).serialize())
    assert st.finalize()[0].total == 0
    # the other list-taking kinds still read `column` from the list
    assert spec(T.DISTINCT, 9, columns=[3, 4]).column == 3 and spec(T.KEY_PROBE, 9, columns=[3, 4]).column == 3


def blob_of(kind, first=None, second=None):
    if kind == T.GROUP_COUNTS:
        tasks = [wire.group_counts_state(100, 64, {}, arity=2) if first is None else first,
                 wire.group_counts_state(100, 64, {}, arity=8) if second is None else second]
        return wire.pack(count=[wire.count_acc(0, 0)], group_counts=tasks)
    tasks = [wire.group_sums_state(100, 64, {}, arity=2) if first is None else first,
             wire.group_sums_state(100, 64, {}, arity=8) if second is None else second]
    return wire.pack(count=[wire.count_acc(0, 0)], group_sums=tasks)


@pytest.mark.parametrize("kind,name", [(T.GROUP_COUNTS, "GROUP_COUNTS"), (T.GROUP_SUMS, "GROUP_SUMS")])
def test_the_shapes_that_stay_refused(kind, name):
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*only DISTINCT takes a column list"):
        T.Plan([spec(kind, 0, column2=1, columns=[1, 2])])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*%s needs column2" % name):
        T.Plan([spec(kind, 0)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*%s needs column2" % name):
        T.Plan([spec(kind, 0, columns=[1])])  # (a list of one column is no list)
    with pytest.raises(T.TgxError, match=r"TGX_UNSUPPORTED.*%s over 9 columns \(2\.\.8 supported\)" % name):
        T.Plan([spec(kind, 0, columns=list(range(9)))])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*negative column index"):
        T.Plan([spec(kind, 0, columns=[1, -2])])
    s = spec(kind, 0, columns=[1, 2])
    s.columns = None  # (a NULL list with n_columns 2)
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*%s over 2 columns" % name):
        T.Plan([s])
    plan = T.Plan([spec(kind, 0, columns=[1, 2])])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*needs its parameters"):
        T.State(plan)


# ---- blobs ------------------------------------------------------------------------------------------------------------------
def counts_plan(columns=(1, 2), mvb=32):
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, columns=list(columns)), spec(T.COUNT, 0)])
    plan.set_group_counts(0, 100, mvb)
    return plan


def counts_blob(groups=COUNTS, arity=2, mvb=32, **kw):
    task = wire.group_counts_state(100, mvb, groups, arity=arity, **kw)
    return wire.pack(count=[wire.count_acc(task_seen(task), 0)], group_counts=[task])


def task_seen(task):
    return struct.unpack_from("<Q", task, 16)[0]


def test_a_host_only_state_answers_its_blob_with_arity_2():
    plan = counts_plan()
    st = T.State.deserialize(plan, counts_blob(overflow=(2, 1), long=(1, 1)))
    summary, groups = st.group_counts(0)
    assert summary == dict(seen=14, groups=5, counted=11, counted_non_null=6, null_group_rows=0, null_group_non_null=0,
                           overflow_rows=2, overflow_non_null=1, long_rows=1, long_non_null=1)
    # ascending by encoded key: NULL before integers before strings, component by component
    assert [T.group_key.decode(k) for k in groups] == [(None, None), (None, b"a"), (-1, b"zz"), (5, None), (b"", b"a")]
    assert groups == COUNTS and st.serialize() == counts_blob(overflow=(2, 1), long=(1, 1))
    r = st.finalize()[0]
    assert (r.total, r.non_null, r.distinct, r.matches) == (14, 8, 5, 11)
    st.merge([T.State.deserialize(plan, counts_blob({E((5, None)): (1, 1), E((6, 6)): (2, 2)}))])
    _, merged = st.group_counts(0)
    assert merged[E((5, None))] == (2, 1) and merged[E((6, 6))] == (2, 2) and len(merged) == 6


def test_group_sums_blobs_carry_the_arity_too():
    plan = T.Plan([spec(T.GROUP_SUMS, 0, columns=[1, 2])])
    plan.set_group_sums(0, 100, 32)
    blob = wire.pack(group_sums=[wire.group_sums_state(100, 32, SUMS, arity=2)])
    st = T.State.deserialize(plan, blob)
    summary, groups = st.group_sums(0)
    assert groups == SUMS and list(groups) == sorted(SUMS) and summary["null_group"] == (0, 0, 0)
    assert summary["counted"] == (7, 5, 2**63 - 6) and st.serialize() == blob
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS task 0: the blob groups by 3 columns, the plan's task by 2"):
        T.State.deserialize(plan, wire.pack(group_sums=[wire.group_sums_state(100, 32, {}, arity=3)]))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_SUMS task 0: the blob groups by 0 columns"):
        T.State.deserialize(plan, wire.pack(group_sums=[wire.group_sums_state(100, 32, {}, arity=0)]))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not the encoded form of a tuple of 2 columns"):
        T.State.deserialize(plan, wire.pack(group_sums=[wire.group_sums_state(100, 32, {E((1,)): (1, 1, 1)}, arity=2)]))


def test_a_blob_of_another_arity_is_refused():
    for arity in (0, 3, 8):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*GROUP_COUNTS task 0: the blob groups by %d columns, "
                                             "the plan's task by 2" % arity):
            T.State.deserialize(counts_plan(), counts_blob({}, arity=arity))
    single = T.Plan([spec(T.GROUP_COUNTS, 0, column2=1), spec(T.COUNT, 0)])
    single.set_group_counts(0, 100, 32)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*the blob groups by 2 columns, the plan's task by 0"):
        T.State.deserialize(single, counts_blob())
    for junk in (1, 9, 2**31):  # (no arity at all)
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed state blob"):
            T.State.deserialize(counts_plan(), counts_blob({}, arity=junk))


LONG = E((b"x" * 20, b"y" * 20))  # 46 bytes, beyond max_value_bytes 32
MALFORMED = [
    ("unsorted", dict(groups=[(E((5, None)), (1, 0)), (E((None, None)), (1, 0))], ordered=False), "malformed state blob"),
    ("repeated", dict(groups=[(E((5, None)), (1, 0)), (E((5, None)), (1, 0))], ordered=False), "malformed state blob"),
    ("beyond max_value_bytes", dict(groups={LONG: (1, 1)}), "a key of 46 bytes, max_value_bytes is 32"),
    ("three components", dict(groups={E((1, 2, 3)): (1, 1)}), "not the encoded form of a tuple of 2 columns"),
    ("one component", dict(groups={E((1,)): (1, 1)}), "not the encoded form of a tuple of 2 columns"),
    ("an unknown tag", dict(groups={b"\x00\x07": (1, 1)}), "not the encoded form of a tuple of 2 columns"),
    ("a truncated integer", dict(groups={b"\x00\x01\x80\x00": (1, 1)}), "not the encoded form of a tuple of 2 columns"),
    ("a string past the end", dict(groups={b"\x00\x02\x00\x05ab": (1, 1)}), "not the encoded form of a tuple of 2 columns"),
    ("integer keys", dict(groups={5: (1, 1)}), "malformed state blob"),
    ("the empty key", dict(groups={b"": (1, 1)}), "not the encoded form of a tuple of 2 columns"),
]


@pytest.mark.parametrize("what,kw,message", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_tuple_blobs_are_refused(what, kw, message):
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + message):
        T.State.deserialize(counts_plan(), counts_blob(**kw))


def test_a_single_column_plans_blob_keeps_its_bytes():
    """against a blob packed by hand, field by field: the record of a task with one group column is what it was"""
    plan = T.Plan([spec(T.GROUP_COUNTS, 0, column2=1), spec(T.GROUP_SUMS, 0, column2=1)])
    plan.set_group_counts(0, 4, 8)
    plan.set_group_sums(1, 4, 8)
    counts = struct.pack("<4I8Q", 4, 8, 1, 0, 6, 1, 1, 0, 0, 0, 0, 2) + struct.pack("<qQQ", -1, 2, 2) + struct.pack("<qQQ", 5, 3, 1)
    sums = struct.pack("<4I11Q", 4, 8, 2, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1) + struct.pack("<I2sQQq", 2, b"ab", 3, 2, -9)
    assert counts == wire.group_counts_state(4, 8, {5: (3, 1), -1: (2, 2)}, null_group=(1, 1))
    assert sums == wire.group_sums_state(4, 8, {b"ab": (3, 2, -9)})
    blob = wire.pack(group_counts=[counts], group_sums=[sums])
    assert T.State.deserialize(plan, blob).serialize() == blob
    assert wire.VERSION == 3 and T.lib().tgx_abi_version() == 6


# ---- the host layer: CompletenessAnalyzer(c).with_grouping(GroupingConfig([..], composite_groups_on_device=True)) ---------------
import json  # noqa: E402
import os  # noqa: E402

import exact_group_counts as exc  # noqa: E402
import exact_group_sums as exs  # noqa: E402
import term_amd.suite as S  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def grouped(by=("region", "product"), composite=True, **kw):
    return S.CompletenessAnalyzer("sales").with_grouping(S.GroupingConfig(list(by), composite_groups_on_device=composite, **kw))


def state_of(analyzer, keyed, **summary):
    """the analyzer's state from {key tuple: (total, non_null)} as the device would report it: encoded keys, ascending"""
    entries = sorted((E(k), t, n) for k, (t, n) in keyed.items())
    return json.loads(analyzer.state_text_from_group_counts(summary, entries))


def text_map(state):
    """the reference's map from the state: its rows in the query's order (completeness descending, ties by key ascending
    with a NULL cell after any value), a NULL cell read as "", a later row replacing an earlier one of its text"""
    rows = sorted(state["groups"], key=lambda g: (-exc.completeness(g["total_count"], g["non_null_count"]),
                                                  tuple((1, "") if c is None else (0, c) for c in g["key"])))
    return {tuple("" if c is None else c for c in g["key"]): (g["total_count"], g["non_null_count"]) for g in rows}


def metric_of(analyzer, state):
    m = analyzer.compute_metric_from_state(state)
    assert m["type"] == "Map"
    return {k: v["value"] for k, v in m["value"].items()}


def same_as_the_reference(analyzer, keyed, by=("region", "product"), **kw):
    want = exc.grouped_state({k: list(v) for k, v in keyed.items()}, list(by), **kw)
    state = state_of(analyzer, keyed)
    assert text_map(state) == want["groups"] and state["metadata"] == want["metadata"] and state["null_group"] is None
    overall = state["overall"] and (state["overall"]["total_count"], state["overall"]["non_null_count"])
    assert overall == want["overall"]
    assert metric_of(analyzer, state) == exc.metric_map(want)
    return state, want


def test_the_analyzers_plan_with_and_without_the_opt_in():
    a = grouped()
    assert a.spec == {"type": "grouped_completeness", "column": "sales", "group_by": ["region", "product"], "max_groups": 10000,
                      "include_overall": True, "composite_groups_on_device": True}
    assert a.name() == "completeness" and a.metric_key() == "completeness.sales_grouped_by_region_product"
    assert a.planned_requests([T.INT32, T.UTF8, T.UTF8]) == [
        {"kind": T.GROUP_COUNTS, "column": "sales", "column2": "", "columns": ["region", "product"],
         "group_counts": {"max_groups": 10000, "max_value_bytes": 256}}]
    eight = grouped(by=["g%d" % i for i in range(8)], strict_reference_types=False)
    assert eight.planned_requests([T.INT64] * 9)[0]["columns"] == ["g%d" % i for i in range(8)]
    cfg = S.GroupingConfig(["a", "b"]).composite_groups_on_device()
    assert cfg.composite_on_device and "composite_groups_on_device" not in grouped(composite=False).spec
    # off or absent, or with 0 or more than 8 columns: the error text is what it was
    for analyzer, n in ((grouped(composite=False), 2), (grouped(by=()), 0), (grouped(by=["g%d" % i for i in range(9)]), 9)):
        with pytest.raises(T.TgxError, match=r"groups by exactly one column on the GPU path \(%d given\)" % n):
            analyzer.planned_requests([T.INT64] * (1 + n))
    one = grouped(by=("region",))  # one column: the single-column request, opt-in or not
    assert one.planned_requests([T.INT64, T.UTF8])[0]["column2"] == "region"
    # strict_reference_types: every group column is declared Utf8; the error names the first that is not
    with pytest.raises(T.TgxError, match="group column 'product' is LargeUtf8.*strict_reference_types=false"):
        a.planned_requests([T.INT64, T.UTF8, T.LARGE_UTF8])
    with pytest.raises(T.TgxError, match="group column 'region' is tgx type 1"):
        a.planned_requests([T.INT64, T.INT64, T.LARGE_UTF8])
    assert grouped(strict_reference_types=False).planned_requests([T.INT64, T.INT64, T.DICT32_UTF8])[0]["kind"] == T.GROUP_COUNTS


def test_the_reference_table_grouped_by_region_and_product():
    g = golden("grouped_completeness_tuple_vectors.json")
    table = g["table"]
    cols = [[v.encode() for v in table[c]] for c in g["group_by"]]
    keyed = {k: tuple(v) for k, v in exc.group_by(table[g["value_column"]], *cols).items()}
    a = grouped(by=g["group_by"])
    state, want = same_as_the_reference(a, keyed, by=g["group_by"])
    assert len(state["groups"]) == g["group_count"] == 4 and a.metric_key() == g["metric_key"]
    assert state["groups"] == [{k: e[k] for k in ("key", "total_count", "non_null_count")} for e in g["groups"]]
    assert state["overall"] == g["overall"] and state["metadata"] == g["metadata"]
    metrics = metric_of(a, state)
    assert {k: v for k, v in metrics.items() if k != "__metadata__"} == g["metrics"]
    assert metrics["US_A"] == 1.0 and metrics["EU_A"] == 0.5  # the reference's two assertions
    assert json.loads(metrics["__metadata__"]) == g["metadata"]


@pytest.mark.parametrize("max_groups", [5, 4, 2, 1])
def test_truncation_at_max_groups_follows_the_reference(max_groups):
    keyed = {(b"a", 1): (4, 4), (b"a", 2): (4, 2), (b"b", 1): (4, 3), (b"b", None): (4, 1), (None, 1): (4, 4)}
    a = grouped(by=("g", "h"), max_groups=max_groups, strict_reference_types=False)
    state, want = same_as_the_reference(a, keyed, by=("g", "h"), max_groups=max_groups)
    assert state["metadata"]["total_groups"] == min(5, max_groups + 1)
    assert state["metadata"]["truncated"] == (max_groups < 5) and len(state["groups"]) == min(5, max_groups)
    if max_groups == 1:  # two rows tie at 1.0: ("a", 1) comes before (NULL, 1), a NULL cell after any value
        assert state["groups"][0]["key"] == ["a", "1"]  # (integers print as decimal text)


def test_null_cells_in_the_state_and_their_collision_with_the_empty_string():
    keyed = {(None, b"a"): (2, 1), (b"", b"a"): (4, 2), (b"k", b"a"): (1, 1), (None, None): (1, 0)}
    a = grouped()
    state, want = same_as_the_reference(a, keyed)
    assert [g["key"] for g in state["groups"]] == [["", "a"], ["k", "a"], [None, "a"], [None, None]]  # a NULL cell is null
    # ("", a) and (NULL, a) tie at 0.5 and are one map key: the later row, NULL's, replaces the earlier; both count
    assert want["groups"][("", "a")] == (2, 1)
    assert (state["metadata"]["total_groups"], state["metadata"]["included_groups"], state["metadata"]["truncated"]) == (4, 3, True)
    assert state["overall"] == {"total_count": 8, "non_null_count": 4}
    assert metric_of(a, state)["_a"] == 0.5 and metric_of(a, state)["_"] == 0.0
    # the less complete of two colliding rows is the later one, whichever it is
    for null_counts, empty_counts, stays in (((4, 1), (4, 2), 0.25), ((4, 3), (4, 2), 0.5)):
        keyed = {(None, b"a"): null_counts, (b"", b"a"): empty_counts}
        state, want = same_as_the_reference(a, keyed)
        assert metric_of(a, state)["_a"] == stays
    cut = grouped(max_groups=2)
    state, _ = same_as_the_reference(cut, {(None, b"a"): (2, 1), (b"", b"a"): (4, 2), (b"k", b"a"): (1, 1)}, max_groups=2)
    assert [g["key"] for g in state["groups"]] == [["", "a"], ["k", "a"]]  # the NULL row is the one that is cut


def test_merge_states_and_the_metric_map_work_on_the_whole_key():
    a = grouped()
    s1 = state_of(a, {(b"EU", b"A"): (3, 2), (b"US", b"A"): (3, 3), (None, b"A"): (1, 0)})
    s2 = state_of(grouped(max_groups=1), {(b"EU", b"A"): (2, 2), (b"EU", b"B"): (5, 1), (b"", b"A"): (1, 1)})
    assert s2["metadata"]["total_groups"] == 2 and len(s2["groups"]) == 1  # truncated: ("", A) and (EU, A) tie, "" first
    s3 = state_of(a, {(b"EU", b"B"): (5, 1), (b"", b"A"): (1, 1)})
    merged = a.merge_states([s1, s2, s3])
    assert merged["groups"] == [{"key": ["", "A"], "total_count": 2, "non_null_count": 2},
                                {"key": ["EU", "A"], "total_count": 3, "non_null_count": 2},
                                {"key": ["EU", "B"], "total_count": 5, "non_null_count": 1},
                                {"key": ["US", "A"], "total_count": 3, "non_null_count": 3},
                                {"key": [None, "A"], "total_count": 1, "non_null_count": 0}]
    assert merged["null_group"] is None and merged["overall"] == {"total_count": 14, "non_null_count": 8}
    # (NULL, A) and ("", A) are two keys of the state and one text vector
    assert merged["metadata"] == {"group_columns": ["region", "product"], "total_groups": 3, "included_groups": 4,
                                  "truncated": False, "overflow_strategy": None}
    values = metric_of(a, merged)
    assert values["_A"] == 0.0 and values["EU_B"] == 0.2 and values["__overall__"] == 8 / 14
    assert list(values)[-2:] == ["__overall__", "__metadata__"]
    with pytest.raises(T.TgxError, match="Cannot merge empty states"):
        a.merge_states([])


def test_rows_beyond_the_bounds_and_keys_that_are_no_tuples_are_the_analyzers_errors():
    a = grouped(max_groups=16)
    with pytest.raises(T.TgxError, match=r"columns \[region, product\] have more groups than the table for max_groups 16 "
                                         "holds.*32 groups held, 7 overflow rows, 0 long rows"):
        state_of(a, {(b"a", b"b"): (1, 1)}, groups=32, overflow_rows=7)
    with pytest.raises(T.TgxError, match="0 overflow rows, 3 long rows"):
        state_of(a, {(b"a", b"b"): (1, 1)}, groups=1, long_rows=3)
    with pytest.raises(T.TgxError, match="not the encoded form of a tuple of 2 columns"):
        state_of(a, {(b"a",): (1, 1)})
    with pytest.raises(T.TgxError, match="not the encoded form of a tuple of 2 columns"):
        a.state_text_from_group_counts({}, [(5, 1, 1)])


# ---- the host layer: CrossTableSumConstraint.group_by([..]).composite_groups_on_device() ----------------------------------------
def side_json(sums):
    """{key tuple: sum} as tgx_host_cross_table_sum_json takes a tuple side: encoded keys, ascending"""
    return {"groups": [[list(E(k)), sums[k]] for k in sorted(sums, key=E)], "arity": 2}


def tuple_side(side, group_by):
    cols = side["columns"]
    kind, values = cols[side["column"]]
    keys = list(zip(*[[g.encode() if isinstance(g, str) else g for g in cols[c][1]] for c in group_by]))
    return exs.side_sums(values, keys, kind.startswith("float"))


def constraint(group_by=("customer_id", "order_date"), tolerance=0.0):
    return S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(list(group_by)).tolerance(tolerance) \
        .composite_groups_on_device()


@pytest.mark.parametrize("case", golden("cross_table_sum_tuple_vectors.json")["cases"], ids=lambda c: c["name"])
def test_the_join_on_the_golden_tables(case):
    c = constraint(case["group_by"], case["tolerance"])
    got = c.verdict_from_sums(side_json(tuple_side(case["left"], case["group_by"])),
                              side_json(tuple_side(case["right"], case["group_by"])))
    want = case["expect"]
    assert {k: got[k] for k in want} == want
    assert got["metric"] == want["max_difference"] and got["config"]["composite_groups_on_device"] is True


def test_null_bearing_and_one_sided_keys_never_join():
    c = constraint()
    left = {(1, b"a"): 5.0, (None, b"a"): 2.0, (None, None): 1.0}
    right = {(1, b"a"): 5.0, (None, b"a"): 2.0, (2, b"a"): 0.0}
    got = c.verdict_from_sums(side_json(left), side_json(right))
    # (1, a) joins; (2, a) is one-sided against 0.0 with no difference; the three NULL-bearing keys are groups of their own
    assert (got["total_groups"], got["violating_groups"], got["max_difference"]) == (5, 3, 2.0)
    assert (got["total_left_sum"], got["total_right_sum"]) == (8.0, 7.0)
    assert got["message"] == ("Cross-table sum mismatch: 3/5 groups by [customer_id, order_date] failed validation "
                              "(exact match required), total sums: 8 vs 7 (max diff: 2.0000)")
    both_empty = c.verdict_from_sums(side_json({}), side_json({}))
    assert (both_empty["status"], both_empty["total_groups"], both_empty["metric"]) == ("success", 0, 0.0)
    nan = c.verdict_from_sums(side_json({(1, b"a"): float("nan")}), side_json({(1, b"a"): 1.0}))
    assert nan["status"] == "success" and nan["max_difference"] != nan["max_difference"]  # NaN > tolerance is false


def test_the_constraints_own_errors():
    c = constraint()
    head = "Constraint evaluation failed for 'cross_table_sum': "
    with pytest.raises(T.TgxError, match=head + r"group column 0 \('customer_id'\) holds integers on the left side and "
                                                "strings on the right side"):
        c.verdict_from_sums(side_json({(1, b"a"): 1.0}), side_json({(b"1", b"a"): 1.0}))
    with pytest.raises(T.TgxError, match=r"group column 1 \('order_date'\) holds integers on the right side and strings on "
                                         "the left side"):
        c.verdict_from_sums(side_json({(1, b"a"): 1.0, (2, None): 1.0}), side_json({(1, 7): 1.0}))
    # a NULL cell holds neither: it fits both kinds
    assert c.verdict_from_sums(side_json({(None, b"a"): 1.0}), side_json({(b"1", b"a"): 1.0}))["total_groups"] == 2
    with pytest.raises(T.TgxError, match="the left side has more groups than the bound max_groups = 65536.*3 overflow rows"):
        c.verdict_from_sums(dict(side_json({}), overflow_rows=3), side_json({}))
    with pytest.raises(T.TgxError, match="a group key of the right side is not the encoded form of a tuple of 2 columns"):
        c.verdict_from_sums(side_json({}), {"groups": [[list(E((1,))), 1.0]], "arity": 2})

    def issue(constraint, tables=None):
        r = S.ValidationSuite.builder("s").check(S.Check.builder("c").level(S.Level.WARNING).constraint(constraint).build()) \
            .build().run(None, tables=tables or {})
        assert r.is_success() and len(r.report.issues) == 1
        return r.report.issues[0].message
    import pyarrow as pa
    orders = pa.table({"id": pa.array([1], pa.int64())})
    plain = S.CrossTableSumConstraint("orders.id", "orders.id").group_by(["a", "b"])
    assert "composite_groups_on_device" not in plain.spec
    # off or absent the error text is what it was; with the opt-in more than 8 columns keep it too
    assert issue(plain, {"orders": orders}).startswith(
        "Error evaluating constraint: " + head + "GROUP BY over 2 columns is not on the GPU path: TGX_CHECK_GROUP_SUMS "
        "groups by exactly one column")
    nine = S.CrossTableSumConstraint("orders.id", "orders.id").group_by(["g%d" % i for i in range(9)]).composite_groups_on_device()
    assert "GROUP BY over 9 columns is not on the GPU path" in issue(nine, {"orders": orders})
    missing = S.CrossTableSumConstraint("orders.id", "payments.id").group_by(["id", "b"]).composite_groups_on_device()
    assert "Schema error: No field named b." in issue(missing, {"orders": orders, "payments": orders})


def test_the_join_outside_the_opt_in_and_its_bound_is_the_one_it_was():
    """tgx_host_cross_table_sum_json reaches the join without evaluate_context's refusals: only the opt-in together with
    2 .. 8 columns makes it the tuple join; everything else is the single-column join of plain keys, as before"""
    empty = {"groups": []}
    for n in (9, 12, 64):
        by = ["g%d" % i for i in range(n)]
        for c in (S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(by).composite_groups_on_device(),
                  S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(by)):
            got = c.verdict_from_sums(empty, empty)
            assert (got["status"], got["total_groups"], got["metric"]) == ("success", 0, 0.0)
            got = c.verdict_from_sums({"groups": [["a", 1.0]]}, {"groups": [["a", 3.0], ["b", 1.0]]})  # plain string keys
            assert (got["total_groups"], got["violating_groups"], got["max_difference"]) == (2, 2, 2.0)
    plain = S.CrossTableSumConstraint("orders.total", "payments.amount").group_by(["a", "b"])  # two columns, no opt-in
    got = plain.verdict_from_sums({"groups": [[1, 5.0], [2, 1.0]], "null_group": 4.0}, {"groups": [[1, 5.0]]})
    assert (got["total_groups"], got["violating_groups"], got["total_left_sum"], got["total_right_sum"]) == (3, 2, 10.0, 5.0)
    assert "composite_groups_on_device" not in got["config"]
    # with the opt-in a side says how many columns it was grouped by, and another number is refused
    c = constraint()
    for bad in ({"groups": []}, {"groups": [], "arity": 3}):
        with pytest.raises(T.TgxError, match="the right side was grouped by %d columns, the constraint groups by 2"
                                             % bad.get("arity", 0)):
            c.verdict_from_sums(side_json({}), bad)
