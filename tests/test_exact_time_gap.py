"""tests/exact_time_gap.py held against hand-worked vectors (tests/golden/time_gap_vectors.json: the reference has no
unit test of its MaxTimeGap mode, so these are the project's own) and shown to tell single perturbations of the rules
apart.  No device, no library: tests/test_gpu_time_gap.py holds the kernels to this module."""
import json
import os
import random

import numpy as np
import pytest

import exact_time_gap as eg

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "time_gap_vectors.json")) as f:
    VECTORS = json.load(f)["vectors"]


def columns(case):
    """(t, valid_t, g, valid_g) of a vector: null -> a 0 slot that is not valid"""
    t = [0 if x is None else x for x in case["t"]]
    vt = [x is not None for x in case["t"]]
    if case["g"] is None:
        return t, vt, None, None
    return t, vt, [0 if x is None else x for x in case["g"]], [x is not None for x in case["g"]]


@pytest.mark.parametrize("case", VECTORS, ids=[v["name"] for v in VECTORS])
def test_hand_worked_vectors(case):
    assert list(eg.counts(case["max_gap"], *columns(case))) == case["expect"]


def test_the_vectors_cover_the_rules():
    names = {v["name"] for v in VECTORS}
    assert len(names) == len(VECTORS) >= 15
    assert any(v["expect"][4] == (1 << 64) - 1 for v in VECTORS)  # the unsigned difference
    assert any(v["g"] is not None and None in v["g"] for v in VECTORS)  # the NULL group
    assert any(v["max_gap"] < 0 for v in VECTORS)


def test_the_answer_depends_on_the_multiset_only():
    rng = random.Random(3)
    t = [rng.randrange(-50, 50) for _ in range(200)]
    g = [rng.randrange(0, 5) for _ in range(200)]
    vt = [rng.random() > 0.1 for _ in range(200)]
    vg = [rng.random() > 0.2 for _ in range(200)]
    want = eg.counts(3, t, vt, g, vg)
    order = list(range(200))
    for _ in range(5):
        rng.shuffle(order)
        pick = lambda a: [a[i] for i in order]  # noqa: E731
        assert eg.counts(3, pick(t), pick(vt), pick(g), pick(vg)) == want
    assert want[2] == want[1] - len(eg.partitions(t, vt, g, vg))  # gaps = rows - non-empty partitions


# ---- the numpy twin (the differential tester's reference) is the plain walk -------------------------------------------
def both(max_gap, t, vt=None, g=None, vg=None):
    """counts_np's answer, after holding it equal to the plain walk's"""
    arr = lambda a, dt: None if a is None else np.array(a, dt)  # noqa: E731
    got = eg.counts_np(max_gap, arr(t, np.int64), arr(vt, bool), arr(g, np.int64), arr(vg, bool))
    assert got == eg.counts(max_gap, t, vt, g, vg), (max_gap, got)
    assert all(type(x) is int for x in got)
    return got


@pytest.mark.parametrize("case", VECTORS, ids=[v["name"] for v in VECTORS])
def test_numpy_twin_on_the_hand_worked_vectors(case):
    assert list(both(case["max_gap"], *columns(case))) == case["expect"]


@pytest.mark.parametrize("seed", range(6))
def test_numpy_twin_on_random_tables_with_nulls_in_both_columns(seed):
    rng = random.Random(seed)
    n = rng.choice([0, 1, 2, 3, 50, 700])
    span = rng.choice([3, 40, 10**6, 1 << 62])
    t = [rng.randrange(-span, span) for _ in range(n)]
    g = [rng.randrange(-2, rng.choice([1, 9])) for _ in range(n)]
    vt = [rng.random() > 0.2 for _ in range(n)]
    vg = [rng.random() > 0.3 for _ in range(n)]
    gaps = sorted(eg.gaps_of(t, vt, g, vg))
    seen, rows, twin = eg.gaps_np(np.array(t, np.int64), np.array(vt, bool), np.array(g, np.int64), np.array(vg, bool))
    assert (seen, rows, [int(x) for x in twin]) == (n, sum(vt), gaps)
    for max_gap in [-1, 0, 1, eg.I64_MAX] + [x for v in gaps[:: max(1, len(gaps) // 4)] for x in (min(v, eg.I64_MAX), v - 1)]:
        both(max_gap, t, vt, g, vg)
        both(max_gap, t, vt)
        both(max_gap, t, None, g, None)
        both(max_gap, t, None, g, vg)


def test_numpy_twin_at_the_int64_extremes():
    lo, hi = eg.I64_MIN, eg.I64_MAX
    t = [5, hi, -7, lo, hi - 1, lo + 1, 0, hi, lo]
    g = [lo, hi, lo, hi, -1, 0, lo, hi - 1, lo + 1]
    for max_gap in (-1, 0, 1, hi - 8, hi):
        both(max_gap, t)
        both(max_gap, t, None, g, None)
        both(max_gap, t, None, g, [True, True, False, True, False, True, True, True, True])
    assert both(hi, [hi, lo])[3:] == (1, (1 << 64) - 1)
    assert both(hi, [hi, lo], None, [hi, lo], None)[2:] == (0, 0, 0)  # the group keys themselves do not wrap together


def test_numpy_twin_on_all_null_groups_and_narrow_group_types():
    rng = random.Random(11)
    t = [rng.randrange(0, 1000) for _ in range(300)]
    g = [rng.randrange(0, 4) for _ in range(300)]
    vt = [rng.random() > 0.1 for _ in range(300)]
    none = [False] * 300
    for max_gap in (-1, 0, 2, 7):
        assert both(max_gap, t, vt, g, none) == both(max_gap, t, vt)  # one partition: the ungrouped answer
        assert both(max_gap, t, none, g, none) == (300, 0, 0, 0, 0)
    for dt, keys in ((np.int8, [-128, -127, 126, 127]), (np.uint8, [0, 1, 254, 255]), (np.int32, [-2**31, 2**31 - 1]),
                     (np.uint32, [0, 2**32 - 1])):
        narrow = [rng.choice(keys) for _ in range(300)]
        assert eg.counts_np(3, np.array(t, np.int64), np.array(vt), np.array(narrow, dt), None) == eg.counts(3, t, vt, narrow, None)


# ---- single perturbations of the rules: each must change the answer on some vector ------------------------------------
def perturbed(rule, max_gap, t, vt, g, vg):
    parts = {}
    for i, ts in enumerate(t):
        if not vt[i]:
            continue
        if g is None:
            key = None
        elif not vg[i]:
            key = ("null", i) if rule == "null_group_per_row" else "null"
        else:
            key = g[i]
        parts.setdefault(key, []).append(ts)
    gaps = []
    for stamps in parts.values():
        stamps.sort()
        for a, b in zip(stamps, stamps[1:]):
            d = b - a
            if rule == "wrapped_difference":  # a signed 64-bit subtraction
                d = (d + (1 << 63)) % (1 << 64) - (1 << 63)
            gaps.append(d)
    above = (lambda x: x >= max_gap) if rule == "equal_is_a_violation" else (lambda x: x > max_gap)
    return [len(t), sum(vt), len(gaps), sum(1 for x in gaps if above(x)), max(gaps) if gaps else 0]


@pytest.mark.parametrize("rule,caught_by", [
    ("equal_is_a_violation", "gap_equal_to_max_gap_is_no_violation"),
    ("null_group_per_row", "null_groups_form_one_partition"),
    ("wrapped_difference", "int64_extremes_do_not_wrap"),
])
def test_single_perturbations_fail_the_vectors(rule, caught_by):
    failing = [v["name"] for v in VECTORS if perturbed(rule, v["max_gap"], *columns(v)) != v["expect"]]
    assert caught_by in failing
    # ... and the unperturbed restatement passes them all: the difference is the rule, not the restatement
    assert all(perturbed(None, v["max_gap"], *columns(v)) == v["expect"] for v in VECTORS)


def test_host_rules():
    assert eg.max_gap_ticks(60, "ms") == 60000 and eg.max_gap_ticks(-1, "ns") == -10**9
    assert eg.max_gap_ticks(eg.I64_MAX, "s") == eg.I64_MAX and eg.max_gap_ticks(eg.I64_MAX // 1000 + 1, "ms") is None
    assert eg.verdict(0, 0) == ("Success", 1.0, None) and eg.verdict(7, 0) == ("Success", 1.0, None)
    assert eg.verdict(3, 1) == ("Failure", 2 / 3, "Time gap violation: 1 gaps exceed maximum allowed (66.67% compliance)")
