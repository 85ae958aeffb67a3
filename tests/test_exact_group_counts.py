"""tests/exact_group_counts.py against itself (the list walk and its numpy twin) and against the reference's own test
table (tests/golden/grouped_completeness_vectors.json), plus the rules it restates: truncation, ties, the "" / NULL
collision and the reserved keys."""
import json
import os

import numpy as np

import exact_group_counts as ex

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "grouped_completeness_vectors.json")) as f:
    GOLDEN = json.load(f)
TABLE = GOLDEN["table"]


def as_rows(groups):
    return sorted(({"key": list(k), "total_count": t, "non_null_count": n} for k, (t, n) in groups.items()),
                  key=lambda r: r["key"])


def test_the_reference_table_by_two_columns():
    want = GOLDEN["by_region_product"]
    got = ex.group_by(TABLE["sales"], TABLE["region"], TABLE["product"])
    assert len(got) == want["group_count"] == 4
    assert as_rows(got) == [{k: g[k] for k in ("key", "total_count", "non_null_count")} for g in want["groups"]]
    for g in want["groups"]:
        assert ex.completeness(g["total_count"], g["non_null_count"]) == g["completeness"]
    assert ex.completeness(*got[("US", "A")]) == 1.0 and ex.completeness(*got[("EU", "A")]) == 0.5


def test_the_reference_table_by_one_column_and_overall():
    assert as_rows(ex.group_by(TABLE["sales"], TABLE["region"])) == GOLDEN["by_region"]["groups"]
    assert as_rows(ex.group_by(TABLE["sales"], TABLE["product"])) == GOLDEN["by_product"]["groups"]
    assert ex.group_by(TABLE["sales"]) == {(): [GOLDEN["overall"]["total_count"], GOLDEN["overall"]["non_null_count"]]}
    state = ex.grouped_state(ex.group_by(TABLE["sales"], TABLE["region"]), ["region"])
    assert state["overall"] == (6, 5) and state["groups"] == {("US",): (3, 3), ("EU",): (3, 2)}
    assert list(state["groups"]) == [("US",), ("EU",)]  # completeness descending
    m = ex.metric_map(state)
    assert list(m) == ["US", "EU", "__overall__", "__metadata__"]
    assert (m["US"], m["EU"], m["__overall__"]) == (1.0, 2 / 3, 5 / 6)
    assert json.loads(m["__metadata__"]) == {"group_columns": ["region"], "total_groups": 2, "included_groups": 2,
                                             "truncated": False, "overflow_strategy": None}


def test_the_defaults_and_the_metadata_text():
    d = GOLDEN["defaults"]
    state = ex.grouped_state({("US", "NYC"): [20, 19], ("US", "LA"): [25, 23]}, ["country", "city"])
    assert state["metadata"] == d["metadata_of_2_groups_of_2"]
    assert ex.metric_map(state)["__metadata__"] == ('{"group_columns":["country","city"],"total_groups":2,'
                                                    '"included_groups":2,"truncated":false,"overflow_strategy":null}')
    assert ex.grouped_state.__defaults__ == (d["max_groups"], d["include_overall"])


def test_the_walk_and_its_numpy_twin_agree():
    rng = np.random.default_rng(1)
    for n, keys_n, null_v, null_g in ((0, 1, 0.0, 0.0), (1, 1, 0.0, 0.0), (5000, 1, 0.5, 0.3), (5000, 300, 0.1, 0.0),
                                      (20_000, 7000, 0.9, 1.0), (20_000, 64, 1.0, 0.5)):
        keys = rng.integers(-keys_n, keys_n, n) * 1_000_003
        valid, key_valid = rng.random(n) >= null_v, rng.random(n) >= null_g
        values = [1 if v else None for v in valid]
        groups = [int(k) if ok else None for k, ok in zip(keys, key_valid)]
        a, b = ex.walk(values, groups), ex.walk_np(valid, keys, key_valid)
        assert a == b and list(a["entries"]) == list(b["entries"])
        assert a["counted"] + a["null_group_rows"] + a["long_rows"] == n
        assert a["counted_non_null"] + a["null_group_non_null"] + a["long_non_null"] == int(valid.sum())


def test_the_null_key_is_a_group_and_long_keys_are_apart():
    values = [1, None, 1, 1, None, 1, 1]
    groups = [b"a", b"a", None, None, b"", b"x" * 5, b"x" * 4]
    w = ex.walk(values, groups, max_value_bytes=4)
    assert w["entries"] == {b"": (1, 0), b"a": (2, 1), b"xxxx": (1, 1)} and list(w["entries"]) == [b"", b"a", b"xxxx"]
    assert (w["null_group_rows"], w["null_group_non_null"], w["long_rows"], w["long_non_null"]) == (2, 2, 1, 1)
    assert (w["seen"], w["groups"], w["counted"], w["counted_non_null"]) == (7, 3, 4, 2)
    multi = ex.group_by(values, groups, [1, 1, None, 2, None, 1, 1])
    assert multi[(None, None)] == [1, 1] and multi[(None, 2)] == [1, 1] and multi[(b"", None)] == [1, 0] and len(multi) == 6


def test_truncation_at_max_groups_and_one_above():
    groups = {(b"a",): [4, 4], (b"b",): [4, 2], (b"c",): [4, 3], (b"d",): [4, 1]}
    at = ex.grouped_state(groups, ["g"], max_groups=4)
    assert at["metadata"] == {"group_columns": ["g"], "total_groups": 4, "included_groups": 4, "truncated": False,
                              "overflow_strategy": None} and at["overall"] == (16, 10)
    above = ex.grouped_state(groups, ["g"], max_groups=3)
    assert list(above["groups"]) == [("a",), ("c",), ("b",)] and above["overall"] == (12, 9)  # the kept groups only
    assert (above["metadata"]["total_groups"], above["metadata"]["included_groups"], above["metadata"]["truncated"]) == (4, 3, True)
    far = ex.grouped_state(groups, ["g"], max_groups=1)
    assert (far["metadata"]["total_groups"], far["metadata"]["included_groups"]) == (2, 1)  # LIMIT max_groups + 1
    assert ex.grouped_state(groups, ["g"], include_overall=False)["overall"] is None


def test_ties_break_by_key_ascending_with_the_null_group_last():
    groups = {(None,): [2, 2], (b"z",): [1, 1], (b"b",): [3, 3], (b"",): [5, 5], (7,): [1, 0]}
    state = ex.grouped_state({k: v for k, v in groups.items() if k != (7,)}, ["g"], max_groups=3)
    assert list(state["groups"]) == [("",), ("b",), ("z",)]  # the NULL group is the one that is cut
    assert state["metadata"]["total_groups"] == 4 and state["metadata"]["truncated"]


def test_a_null_key_reads_as_the_empty_string_and_collides_with_it():
    groups = {(None,): [2, 1], (b"",): [4, 2], (b"k",): [1, 1]}  # "" and NULL tie at 0.5: "" first, NULL later
    state = ex.grouped_state(groups, ["g"])
    assert state["groups"] == {("k",): (1, 1), ("",): (2, 1)}  # the later of the two overwrote the earlier
    assert state["overall"] == (7, 4)
    assert (state["metadata"]["total_groups"], state["metadata"]["included_groups"], state["metadata"]["truncated"]) == (3, 2, True)


def test_the_reserved_keys_overwrite_a_group_of_their_name():
    groups = {(b"__overall__",): [2, 0], (b"__metadata__",): [2, 2], (b"a", ): [4, 1]}
    m = ex.metric_map(ex.grouped_state(groups, ["g"]))
    assert m["__overall__"] == 3 / 8 and m["__metadata__"].startswith('{"group_columns":["g"]') and m["a"] == 0.25
    assert len(m) == 3
    assert ex.completeness(0, 0) == 1.0
    assert ex.metric_map(ex.grouped_state({(3, b"x"): [1, 1]}, ["a", "b"]))["3_x"] == 1.0  # integers as decimal text
