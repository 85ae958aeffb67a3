"""The counted mode of TGX_CHECK_KEY_PROBE and JoinCoverageConstraint without a device: the plan calls, what a host-only
counted state answers from a blob, the blob layout against term_amd/wire.py, merging by the extended identity and under
the guard against a wrapping sum, the builder surface with its clamping and JSON form, every error of the constraint, and
every verdict and message branch through tgx_host_join_coverage_json, held against tests/exact_join_coverage.py and the
golden vectors."""
import json
import os
import struct

import pytest

import exact_join_coverage as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

HERE = os.path.dirname(os.path.abspath(__file__))
PARENT = (40, 0x1234567890ABCDEF)
COUNTED = (90, 0x0FEDCBA987654321, 7, 31)  # parent_rows, parent_count_digest, max_count, pairs
MISSING = {5: 3, -1: 2, 7: 4}


def plans():
    counted = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 1), spec(T.COUNT, 0)])
    counted.set_key_probe_counted(0, 4)
    counted.set_key_probe(1, 100)
    return counted


def blob(first=None, second=None):
    first = wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT, counted=COUNTED) if first is None else first
    second = wire.key_probe_state(100, {9: 1}, matched=2, parent=(0, 0)) if second is None else second
    return wire.pack(count=[wire.count_acc(20, 19)], key_probes=[first, second])


# ---- the plan calls -----------------------------------------------------------------------------------------------------------
def test_a_spec_takes_one_of_the_two_calls():
    plan = T.Plan([spec(T.KEY_PROBE, 0), spec(T.KEY_PROBE, 0), spec(T.COUNT, 0)])
    plan.set_key_probe_counted(0, 100)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*counted"):
        plan.set_key_probe(0, 100)
    plan.set_key_probe(1, 100)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*plain"):
        plan.set_key_probe_counted(1, 100)
    with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*reserved must be 0 \(7\)"):
        plan.set_key_probe_counted(0, 100, reserved=7)
    for bound in (0, T.KEY_PROBE_MAX_MISSING_KEYS + 1):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*max_missing_keys must be"):
            plan.set_key_probe_counted(0, bound)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        plan.set_key_probe_counted(2, 100)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*counted"):
        plan.set_key_probe_rows(0)
    T.State.deserialize(plan, wire.pack(count=[wire.count_acc(0, 0)],
                                        key_probes=[wire.key_probe_state(100, counted=(0, 0, 0, 0)), wire.key_probe_state(100)]))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_key_probe_counted(0, 100)
    rows = T.Plan([spec(T.KEY_PROBE, 0)])
    rows.set_key_probe_rows(0)
    for call in (rows.set_key_probe, rows.set_key_probe_counted):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*gather rows"):
            call(0, 100)


# ---- the blob -----------------------------------------------------------------------------------------------------------------
def test_the_blob_layout_of_a_counted_task():
    task = wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT, counted=COUNTED)
    plain = wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT)
    # a plain task's bytes are what they were; a counted one flags the second reserved word and adds four words
    assert plain == struct.pack("<4I7Q", 4, 0, 1, 0, PARENT[0], PARENT[1], 20, 19, 10, 0, 3) + struct.pack(
        "<qQqQqQ", -1, 2, 5, 3, 7, 4)
    assert task == struct.pack("<4I7Q", 4, 0, 1, 1, PARENT[0], PARENT[1], 20, 19, 10, 0, 3) + struct.pack(
        "<4Q", *COUNTED) + struct.pack("<qQqQqQ", -1, 2, 5, 3, 7, 4)
    st = T.State.deserialize(plans(), blob())
    assert st.serialize() == blob()
    summary, entries = st.key_probe(0)
    assert (summary["seen"], summary["matched"], summary["missing_rows"], summary["null_rows"]) == (20, 10, 9, 1)
    assert (summary["parent_keys"], summary["parent_digest"], summary["route"]) == PARENT + (0,) and entries == dict(sorted(MISSING.items()))
    assert st.key_probe_pairs(0) == {"pairs": 31, "join_rows": 31 + 9 + 1, "parent_rows": 90,
                                     "parent_count_digest": COUNTED[1], "max_count": 7}
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not counted"):
        st.key_probe_pairs(1)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        st.key_probe_pairs(2)
    r = st.finalize()
    assert (r[0].total, r[0].non_null, r[0].matches, r[0].distinct) == (20, 19, 10, 3)


def test_plain_and_counted_blobs_do_not_cross():
    plain_first = wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other mode"):
        T.State.deserialize(plans(), blob(first=plain_first))
    counted_second = wire.key_probe_state(100, {9: 1}, matched=2, parent=(0, 0), counted=(0, 0, 0, 0))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*other mode"):
        T.State.deserialize(plans(), blob(second=counted_second))


@pytest.mark.parametrize("what,counted", [
    ("pairs below the matched rows", (90, 1, 7, 9)),
    ("pairs above matched * max_count", (90, 1, 7, 71)),
    ("max_count above parent_rows", (6, 1, 7, 31)),
    ("parent_rows below parent_keys", (39, 1, 7, 31)),
    ("parent_rows of 2^63", (2**63, 1, 7, 31)),
    ("a set of keys without a count", (90, 1, 0, 0)),
])
def test_malformed_counted_blobs_are_refused(what, counted):
    first = wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT, counted=counted)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed state blob.*counted set and pairs"):
        T.State.deserialize(plans(), blob(first=first))
    unknown = wire.key_probe_state(4, counted=(0, 0, 0, 1))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed state blob"):
        T.State.deserialize(plans(), blob(first=unknown))
    assert len(blob()) == len(blob(first=wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT))) + 32
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(plans(), blob()[:-40])


def test_merging_by_the_extended_identity_and_under_the_guard():
    plan = plans()
    a = T.State.deserialize(plan, blob())
    a.merge([T.State.deserialize(plan, blob())])
    assert a.key_probe_pairs(0)["pairs"] == 62 and a.key_probe(0)[0]["matched"] == 20
    # the same keys with other counts: parent_rows or the count digest differ
    for counted in ((91, COUNTED[1], 7, 31), (90, COUNTED[1] + 1, 7, 31)):
        other = wire.key_probe_state(4, MISSING, nulls=1, matched=10, parent=PARENT, counted=counted)
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*different parent sets"):
            a.merge([T.State.deserialize(plan, blob(first=other))])
    assert a.key_probe_pairs(0)["pairs"] == 62
    # pairs add in checked arithmetic
    rows, most = 2**62, 2**61
    big = wire.key_probe_state(4, matched=4, parent=PARENT, counted=(rows, 5, most, 4 * most))
    x, y = T.State.deserialize(plan, blob(first=big)), T.State.deserialize(plan, blob(first=big))
    assert x.key_probe_pairs(0)["pairs"] == 2**64 // 2
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*2\\^64 - 1"):
        x.merge([y])
    assert x.key_probe_pairs(0)["pairs"] == 2**63 and x.key_probe(0)[0]["matched"] == 4  # nothing was added
    less = wire.key_probe_state(4, matched=4, parent=PARENT, counted=(rows, 5, most, 4 * most - 1))
    x.merge([T.State.deserialize(plan, blob(first=less))])
    assert x.key_probe_pairs(0) == {"pairs": 2**64 - 1, "join_rows": 2**64 - 1, "parent_rows": rows,
                                    "parent_count_digest": 5, "max_count": most}
    with_nulls = wire.key_probe_state(4, nulls=1, parent=PARENT, counted=(rows, 5, most, 0))
    x.merge([T.State.deserialize(plan, blob(first=with_nulls))])
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*more than 2\\^64 - 1 rows"):
        x.key_probe_pairs(0)


# ---- the constraint: builders, clamping, JSON ---------------------------------------------------------------------------------------
COUNTS = {"left": {"pairs": 2, "join_rows": 3}, "examples": {"missing_keys": 1, "null_rows": 0, "overflow_rows": 0}}


def test_the_builder_surface_and_the_json_round_trip():
    c = S.JoinCoverageConstraint("orders", "customers")
    assert c.spec == {"type": "join_coverage", "left_table": "orders", "right_table": "customers", "join_keys": [],
                      "expected_match_rate": 1.0, "coverage_type": "left", "distinct_only": False,
                      "max_examples_reported": 100, "max_missing_keys": 10000}
    assert c.name() == "join_coverage"
    c = c.on("a", "b").on("customer_id", "id")  # on() replaces
    assert c.spec["join_keys"] == [["customer_id", "id"]]
    assert c.on_multiple([("x", "y"), ("u", "v")]).spec["join_keys"] == [["x", "y"], ["u", "v"]]
    c.on("customer_id", "id")
    for given, kept in ((1.5, 1.0), (-0.25, 0.0), (0.95, 0.95), (1, 1.0)):
        assert c.expect_match_rate(given).spec["expected_match_rate"] == kept
    c = c.coverage_type(S.CoverageType.Bidirectional).distinct_only(True).max_examples_reported(50).max_missing_keys(77)
    with pytest.raises(ValueError):
        c.coverage_type("sideways")
    config = c.expect_match_rate(0.5).verdict_from_counts(dict(COUNTS, right={"pairs": 2, "join_rows": 2}))["config"]
    assert config == dict({k: v for k, v in c.spec.items() if k != "type"}, name="join_coverage")
    again = S.JoinCoverageConstraint.from_spec(json.loads(json.dumps(c.spec)))
    assert again.spec == c.spec
    # the C++ reader clamps as the builder does, and has the reference's defaults
    raw = {"type": "join_coverage", "left_table": "l", "right_table": "r", "join_keys": [["a", "b"]], "expected_match_rate": 7.0}
    bare = S.JoinCoverageConstraint("l", "r")
    bare.spec = raw
    config = bare.verdict_from_counts(COUNTS)["config"]
    assert (config["expected_match_rate"], config["coverage_type"], config["distinct_only"]) == (1.0, "left", False)
    assert (config["max_examples_reported"], config["max_missing_keys"]) == (100, 10000)
    # the check builder pushes JoinCoverageConstraint::new(left, right), without keys
    check = S.Check.builder("c").join_coverage("orders", "customers").build()
    text = json.dumps(check.spec)
    assert '"type": "join_coverage"' in text and '"join_keys": []' in text and '"left_table": "orders"' in text


def verdict(c, counts):
    v = c.verdict_from_counts(counts)
    return v["status"], v["metric"], v["message"]


def test_every_error_of_the_constraint():
    def refused(c, counts=COUNTS):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT") as e:
            c.verdict_from_counts(counts)
        return str(e.value)

    new = S.JoinCoverageConstraint
    assert "No join keys specified. Use .on() or .on_multiple() to set join keys" in refused(new("l", "r"))
    text = refused(new("l", "r").on_multiple([("a", "b"), ("c", "d")]))
    assert "2 key pairs" in text and "l.a" in text and "not on the GPU path" in text
    text = refused(new("l", "r").on("a", "b").coverage_type(S.CoverageType.Right).distinct_only(True),
                   {"right": {"pairs": 1, "join_rows": 1}})
    assert "distinct_only with RightCoverage" in text and "common to both sides" in text
    assert "has no rows" in refused(new("l", "r").on("a", "b"), {"left": {"pairs": 0, "join_rows": 0}})
    assert "has no rows" in refused(new("l", "r").on("a", "b").coverage_type(S.CoverageType.Bidirectional),
                                    {"left": {"pairs": 0, "join_rows": 4}, "right": {"pairs": 0, "join_rows": 0}})
    assert "has no rows" in refused(new("l", "r").on("a", "b").distinct_only(True),
                                    {"left": {"pairs": 0, "join_rows": 4}, "left_distinct": 0})
    assert "max_missing_keys must be 1 .. 65536" in refused(new("l", "r").on("a", "b").max_missing_keys(0))
    assert refused(new("l; drop", "r").on("a", "b"))   # identifiers are validated first, as in the reference
    assert refused(new("l", "r").on("a b", "b"))
    assert "missing" in refused(new("l", "r").on("a", "b").coverage_type(S.CoverageType.Right))  # the side it reads
    assert "needs the left side's missing keys" in refused(new("l", "r").on("a", "b"), {"left": {"pairs": 1, "join_rows": 2}})
    assert "join_rows is pairs" in refused(new("l", "r").on("a", "b"), {"left": {"pairs": 3, "join_rows": 2}})
    assert "not an object" in refused(new("l", "r").on("a", "b"), [])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a join_coverage constraint"):
        S.ForeignKeyConstraint("a.b", "c.d").__class__.verdict_from_counts(S.ForeignKeyConstraint("a.b", "c.d"), COUNTS) \
            if False else new("l", "r").__class__.verdict_from_counts(S.ForeignKeyConstraint("a.b", "c.d"), COUNTS)


def test_the_verdict_branches_and_the_message():
    new = S.JoinCoverageConstraint
    c = new("orders", "customers").on("customer_id", "id")
    assert verdict(c.expect_match_rate(0.6), COUNTS) == ("success", 2 / 3, None)
    assert verdict(c.expect_match_rate(2 / 3), COUNTS) == ("success", 2 / 3, None)  # >=
    head = "Join coverage constraint failed: orders %s customers coverage is "
    assert verdict(c.expect_match_rate(0.9), COUNTS) == (
        "failure", 2 / 3, head % "->" + "66.67% (expected: 90.00%) (1 unmatched examples found)")
    # {:.2} at 99.995 %: the double's exact value decides
    from decimal import Decimal

    rate = 19999 / 20000
    text = str(Decimal(rate * 100.0).quantize(Decimal("0.01")))
    got = verdict(c.expect_match_rate(1.0).max_examples_reported(0), {"left": {"pairs": 19999, "join_rows": 20000}})
    assert got == ("failure", rate, head % "->" + text + "% (expected: 100.00%)")
    # the examples suffix: without and with a NULL row, at the limit, with overflow
    def suffix(limit, keys, nulls, overflow=0):
        counts = {"left": {"pairs": 1, "join_rows": 10}, "examples": {"missing_keys": keys, "null_rows": nulls, "overflow_rows": overflow}}
        return verdict(c.max_examples_reported(limit), counts)[2].split("%)")[-1]

    assert suffix(100, 3, 0) == " (3 unmatched examples found)"
    assert suffix(100, 3, 5) == " (4 unmatched examples found)"   # a NULL is one distinct value
    assert suffix(100, 0, 5) == " (1 unmatched examples found)"
    assert suffix(100, 0, 0) == ""
    assert suffix(3, 3, 1) == " (3 unmatched examples found)" and suffix(3, 2, 1) == " (3 unmatched examples found)"
    assert suffix(0, 3, 1) == ""
    assert suffix(100, 3, 1, overflow=9) == " (at least 4 unmatched examples found)"
    assert suffix(4, 3, 1, overflow=9) == " (4 unmatched examples found)"  # the limit is reached: exact
    # the three coverage types and distinct_only
    both = {"left": {"pairs": 6, "join_rows": 8}, "right": {"pairs": 6, "join_rows": 12}, "left_distinct": 4,
            "examples": {"missing_keys": 0, "null_rows": 0, "overflow_rows": 0}}
    c = new("l", "r").on("a", "b").expect_match_rate(0.0)
    assert verdict(c.coverage_type(S.CoverageType.Left), both)[1] == 0.75
    assert verdict(c.coverage_type(S.CoverageType.Right), both)[1] == 0.5
    assert verdict(c.coverage_type(S.CoverageType.Bidirectional), both)[1] == 0.5
    assert verdict(c.coverage_type(S.CoverageType.Bidirectional).distinct_only(True), both)[1] == 0.5  # ignored
    assert verdict(c.coverage_type(S.CoverageType.Left).distinct_only(True), both)[1] == 1.5          # above 1
    c = new("l", "r").on("a", "b").expect_match_rate(0.9).distinct_only(False)
    assert verdict(c.coverage_type(S.CoverageType.Right), both)[2] == "Join coverage constraint failed: l <- r coverage is 50.00% (expected: 90.00%)"
    assert verdict(c.coverage_type(S.CoverageType.Bidirectional), both)[2] == "Join coverage constraint failed: l <-> r coverage is 50.00% (expected: 90.00%)"


# ---- the golden vectors and the exact walk ----------------------------------------------------------------------------------------
def golden_cases():
    with open(os.path.join(HERE, "golden", "join_coverage_vectors.json")) as f:
        return json.load(f)["cases"]


def counts_of(lv, lm, rv, rm):
    """the counts JSON of two table sides, from the exact walk"""
    ls, lp = ex.walk(lv, lm, ex.records_of(rv, rm))
    _, rp = ex.walk(rv, rm, ex.records_of(lv, lm))
    return {"left": {"pairs": lp["pairs"], "join_rows": lp["join_rows"]},
            "right": {"pairs": rp["pairs"], "join_rows": rp["join_rows"]}, "left_distinct": len(ex.records_of(lv, lm)),
            "examples": {"missing_keys": ls["missing_keys"], "null_rows": ls["null_rows"], "overflow_rows": 0}}


@pytest.mark.parametrize("case", golden_cases(), ids=[c["name"] for c in golden_cases()])
def test_the_golden_vectors_verdicts(case):
    lv, lm = [v or 0 for v in case["left"]], [v is not None for v in case["left"]]
    rv, rm = [v or 0 for v in case["right"]], [v is not None for v in case["right"]]
    c = S.JoinCoverageConstraint(case["left_table"], case["right_table"]).on(case["left_column"], case["right_column"])
    c = c.expect_match_rate(case["expected"]).coverage_type(case["coverage_type"]).distinct_only(case["distinct_only"])
    c = c.max_examples_reported(case.get("max_examples", 100))
    got = verdict(c, counts_of(lv, lm, rv, rm))
    assert got == ex.coverage(case["left_table"], case["right_table"], lv, lm, rv, rm, case["coverage_type"],
                              case["distinct_only"], case["expected"], case.get("max_examples", 100))
    assert (got[0], got[2]) == (case["status"], case["message"]) and abs(got[1] - case["metric"]) <= 1e-12
