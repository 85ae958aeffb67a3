"""tests/exact_key_probe.py against itself and against the golden vectors: the plain walk and its numpy twin agree on
seeded tables, the digest and the route rule are pinned to hand-computed values, and the verdict restates what the
reference's own tests assert (tests/golden/foreign_key_vectors.json)."""
import json
import os

import numpy as np
import pytest

import exact_key_probe as ex

I64_MIN, I64_MAX = -2**63, 2**63 - 1
HERE = os.path.dirname(os.path.abspath(__file__))


def golden_cases():
    with open(os.path.join(HERE, "golden", "foreign_key_vectors.json")) as f:
        return json.load(f)["cases"]


def golden_state(case):
    child_mask = [v is not None for v in case["child"]]
    parent_mask = [v is not None for v in case["parent"]]
    return ex.walk([v or 0 for v in case["child"]], child_mask, [v or 0 for v in case["parent"]], parent_mask)


@pytest.mark.parametrize("seed", range(6))
def test_the_walk_and_its_twin_agree(seed):
    rng = np.random.default_rng(seed)
    n, m = int(rng.integers(0, 4000)), int(rng.integers(0, 600))
    scale = [1, 1, 1_000_003, 2**40][seed % 4]
    child = rng.integers(-50, 700, n) * scale
    parent = rng.integers(0, 600, m) * scale
    cm = rng.random(n) >= [0.0, 0.3, 1.0][seed % 3]
    pm = rng.random(m) >= 0.2
    if seed % 2:
        child[: n // 7] = -1  # the marker key is a key like any other
        parent[: m // 5] = -1
    for cmask, pmask in ((cm, pm), (None, None), (cm, None)):
        a = ex.walk(child.tolist(), None if cmask is None else cmask.tolist(), parent.tolist(),
                    None if pmask is None else pmask.tolist(), 100)
        b = ex.walk_np(child, cmask, parent, pmask, 100)
        assert a == b and list(a["entries"]) == list(b["entries"]) == sorted(a["entries"])
        assert a["seen"] == a["non_null"] + a["null_rows"] == n
        assert a["non_null"] == a["matched"] + a["missing_rows"] and a["missing_rows"] == a["counted"] + a["overflow_rows"]
        assert a["within_bound"] == (a["missing_keys"] <= 100)


def test_the_digest():
    # splitmix64's finaliser: the first output of the generator seeded with 0 is mix64(0x9e3779b97f4a7c15)
    assert ex.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert ex.mix64(0) == 0 and int(ex.mix64_np(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert ex.digest([]) == 0 == ex.digest_np(np.zeros(0, np.int64))
    assert ex.digest([0]) == 0xE220A8397B1DCDAF  # 0 ^ salt
    keys = [5, -1, I64_MIN, I64_MAX, 0, 5, -1]
    want = sum(ex.mix64((k & ex.M64) ^ ex.DIGEST_SALT) for k in {5, -1, I64_MIN, I64_MAX, 0}) & ex.M64
    assert ex.digest(keys) == want == ex.digest_np(np.array(keys, np.int64))      # duplicates count once
    assert ex.digest(keys[::-1]) == want                                          # no order
    assert ex.digest([1, 2]) != ex.digest([1, 3])


def test_the_route_rule():
    assert ex.route_of([]) == ex.ROUTE_EMPTY
    assert ex.route_of([7]) == ex.ROUTE_BITMAP
    assert ex.route_of([0, 100, 300, 511]) == ex.ROUTE_BITMAP      # range 512 == 128 * 4
    assert ex.route_of([0, 100, 300, 512]) == ex.ROUTE_HASH        # one key beyond it
    assert ex.route_of([0, 100, 300, 512, 512]) == ex.ROUTE_BITMAP  # the RECORDS count: 128 * 5
    assert ex.route_of([0, 512], n_records=5) == ex.ROUTE_BITMAP
    assert ex.route_of([I64_MIN, I64_MAX]) == ex.ROUTE_HASH        # the range wraps to 0: not dense
    assert ex.route_of([I64_MIN, I64_MAX - 1]) == ex.ROUTE_HASH
    assert ex.route_of([-1, 0, 1]) == ex.ROUTE_BITMAP
    assert [ex.hash_slots(n) for n in (1, 2, 3, 4, 5, 8, 9)] == [2, 4, 8, 8, 16, 16, 32]
    twin = ex.walk_np([1], None, [0, 100, 300, 512], None)
    assert twin["route"] == ex.ROUTE_HASH and ex.walk_np([1], None, [0, 100, 300, 511], None)["route"] == ex.ROUTE_BITMAP


@pytest.mark.parametrize("case", golden_cases(), ids=[c["name"] for c in golden_cases()])
def test_the_golden_vectors(case):
    state = golden_state(case)
    status, metric, message = ex.verdict(state, case["child_column"], case["parent_column"], case["allow_nulls"])
    assert (status, metric) == (case["status"], case["metric"])
    if status == "success":
        assert message is None
        return
    assert all(part in message for part in case["message_parts"])
    total = state["missing_rows"] + (0 if case["allow_nulls"] else state["null_rows"])
    assert (total, state["missing_keys"]) == (case["total"], case["unique"])
    assert message.startswith("Foreign key constraint violation: %d values in '%s' do not exist in '%s' (total: %d, unique: %d)"
                               % (total, case["child_column"], case["parent_column"], total, case["unique"]))


def test_the_examples_and_the_overflow_wording():
    state = ex.walk(list(range(20)) * 2 + [None], [True] * 40 + [False], [0, 1], None)
    assert state["missing_keys"] == 18 and state["null_rows"] == 1
    _, metric, message = ex.verdict(state, "c.k", "p.k")
    assert metric == 37.0 and message.endswith("(total: 37, unique: 18). Examples: [2, 3, 4, 5, 6, ... (13 more)]")
    assert ex.verdict(state, "c.k", "p.k", max_violations_reported=5)[2].endswith("Examples: [2, 3, 4, 5, 6]")
    assert ex.verdict(state, "c.k", "p.k", max_violations_reported=6)[2].endswith("Examples: [2, 3, 4, 5, 6, ... (1 more)]")
    assert ex.verdict(state, "c.k", "p.k", max_violations_reported=0)[2].endswith("unique: 18)")
    assert ex.verdict(state, "c.k", "p.k", examples=False)[2].endswith("unique: 18)")
    assert ex.verdict(state, "c.k", "p.k", allow_nulls=True)[1] == 36.0
    over = dict(state, overflow_rows=4, missing_rows=state["missing_rows"] + 4)
    assert "(total: 41, unique: at least 18). Examples: [2, 3," in ex.verdict(over, "c.k", "p.k")[2]
