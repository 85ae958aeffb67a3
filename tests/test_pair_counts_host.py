"""TGX_CHECK_PAIR_COUNTS without a device: plan validation, what a host-only state answers from a blob, merging by value,
every malformed-blob refusal of the section (term_amd/wire.py), the size-query convention of the entries call, and
MutualInformationAnalyzer's opt-in: what it plans, the state it builds from given pair counts, its parse guard and its
own errors."""
import ctypes as C
import re
import struct

import pytest

import term_amd as T
from _lib_spec import spec
from term_amd import wire

INF = float("inf")
TEXT = {(b"b", b"x"): 3, (b"", b"x"): 2, (b"ab", b"c"): 1, (b"a", b"bc"): 1, (b"\xff", b""): 1}
MIXED = {(0, b"u"): 4, (3, b"u"): 1, (3, b""): 2}
VALUE, RANGE = wire.pair_side(0), wire.pair_side(1)
BINNED = wire.pair_side(2, 3, 1.0, 3.0)


def pairs_plan(mvb=16, bins=3):
    """spec 0: string x string; spec 1: binned x string; spec 2: string x range"""
    plan = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1), spec(T.PAIR_COUNTS, 2, column2=1), spec(T.PAIR_COUNTS, 0, column2=2),
                   spec(T.COUNT, 0)])
    plan.set_pair_counts(0, max_pairs=100, max_value_bytes=mvb)
    plan.set_pair_counts(1, x=(1.0, 3.0, bins), max_pairs=4, max_value_bytes=8)
    plan.set_pair_counts(2, y="range", max_pairs=4, max_value_bytes=8)
    return plan


def pairs_blob(first=None, second=None, third=None):
    first = wire.pair_counts_state(100, 16, VALUE, VALUE, 12, TEXT, overflow_rows=1, long_rows=1) if first is None else first
    second = wire.pair_counts_state(4, 8, BINNED, VALUE, 12, MIXED, non_finite=2, out_of_range=1) if second is None else second
    third = wire.pair_counts_state(4, 8, VALUE, RANGE, 12, both_non_null=9, non_finite=2, n=7, lo=-2.5, hi=40.0) if third is None else third
    return wire.pack(count=[wire.count_acc(12, 11)], pair_counts=[first, second, third])


def test_abi_constants():
    assert T.PAIR_COUNTS == 16 and (T.PAIR_COUNTS_MAX_PAIRS, T.PAIR_COUNTS_MAX_VALUE_BYTES) == (65536, 256)
    assert (T.PAIR_SIDE_VALUE, T.PAIR_SIDE_RANGE, T.PAIR_SIDE_BINNED) == (0, 1, 2)
    for name in ("tgx_plan_set_pair_counts", "tgx_pair_counts_get", "tgx_pair_range_get", "tgx_pair_counts_entries"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)
    assert C.sizeof(T._lib.PairCountsParams) == 56 and C.sizeof(T._lib.PairCountEntry) == 56


def test_parameters_are_validated():
    plan = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1), spec(T.COUNT, 0)])
    for bad in (0, 65537, 2**32 - 1):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_pairs must be 1 \.\. 65536 \(%d\)" % bad):
            plan.set_pair_counts(0, max_pairs=bad, max_value_bytes=16)
    for bad in (0, 257):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_value_bytes must be 1 \.\. 256 \(%d\)" % bad):
            plan.set_pair_counts(0, max_pairs=10, max_value_bytes=bad)
    for bad in (1, 128):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*bins of the x side must be 2 \.\. 127 \(%d\)" % bad):
            plan.set_pair_counts(0, x=(0.0, 1.0, bad))
    for origin, width in ((INF, 1.0), (0.0, 0.0), (0.0, -1.0), (0.0, INF), (float("nan"), 1.0), (0.0, float("nan"))):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*the y side's origin must be finite and its width"):
            plan.set_pair_counts(0, y=(origin, width, 10))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*unknown mode 3 of the x side"):
        plan.set_pair_counts(0, x=T._lib.PairSide(3, 0, 0.0, 0.0))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1 is not a PAIR_COUNTS check"):
        plan.set_pair_counts(1)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*PAIR_COUNTS needs column2"):
        T.Plan([spec(T.PAIR_COUNTS, 0)])
    for ok in (dict(max_pairs=1, max_value_bytes=1), dict(max_pairs=65536, max_value_bytes=256),
               dict(x=(0.0, 1.0, 2)), dict(y=(-5.0, 1e-300, 127)), dict(x="range"), dict(y="range")):
        plan.set_pair_counts(0, **ok)


def test_two_numeric_sides_are_refused_and_point_to_joint_bins():
    plan = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1)])
    b = (0.0, 1.0, 10)
    for x, y in ((b, b), ("range", b), (b, "range"), ("range", "range")):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*both sides are numeric.*JOINT_BINS"):
            plan.set_pair_counts(0, x=x, y=y)


def test_a_spec_without_parameters_fails_state_create_and_deserialize():
    plan = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1), spec(T.PAIR_COUNTS, 0, column2=1)])
    plan.set_pair_counts(0, max_pairs=10, max_value_bytes=16)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*tgx_plan_set_pair_counts"):
        T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_plan_set_pair_counts"):
        T.State.deserialize(plan, wire.pack(pair_counts=[wire.pair_counts_state(10, 16, VALUE, VALUE, 0)] * 2))


def test_setter_is_refused_after_the_first_state():
    plan = pairs_plan()
    st = T.State.deserialize(plan, pairs_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_pair_counts(0, max_pairs=5)
    del st


def test_a_host_only_state_answers_its_blob():
    plan = pairs_plan()
    st = T.State.deserialize(plan, pairs_blob())
    summary, counts = st.pair_counts(0)
    assert summary == dict(seen=12, both_non_null=10, distinct=5, counted=8, overflow_rows=1, long_rows=1, non_finite=0,
                           out_of_range=0)
    # bytewise, a prefix first, x before y: ("a", "bc") and ("ab", "c") are two pairs, ("", "x") and ("\xff", "") too
    assert list(counts.items()) == [((b"", b"x"), 2), ((b"a", b"bc"), 1), ((b"ab", b"c"), 1), ((b"b", b"x"), 3),
                                    ((b"\xff", b""), 1)]
    summary, counts = st.pair_counts(1)
    assert summary == dict(seen=12, both_non_null=10, distinct=3, counted=7, overflow_rows=0, long_rows=0, non_finite=2,
                           out_of_range=1)
    assert list(counts.items()) == [((0, b"u"), 4), ((3, b""), 2), ((3, b"u"), 1)]  # bins as integers
    assert st.pair_range(2) == dict(seen=12, both_non_null=9, n=7, non_finite=2, min=-2.5, max=40.0)
    assert st.pair_counts(2) == (dict(seen=12, both_non_null=9, distinct=0, counted=0, overflow_rows=0, long_rows=0,
                                      non_finite=0, out_of_range=0), {})
    res = st.finalize()
    assert [(r.total, r.non_null, r.distinct, r.matches) for r in res[:3]] == [(12, 10, 5, 8), (12, 10, 3, 7), (12, 9, 0, 0)]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 3 is not a PAIR_COUNTS check"):
        st.pair_counts(3)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0 is in its count phase"):
        st.pair_range(0)


def test_the_entries_call_follows_the_size_query_convention():
    plan = pairs_plan()
    st = T.State.deserialize(plan, pairs_blob())
    L, err = T.lib(), T._lib._Error()
    n, nb = C.c_uint64(), C.c_uint64()
    assert L.tgx_pair_counts_entries(plan.h, st.h, 0, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(err)) == 0
    assert (n.value, nb.value) == (5, 10)
    small = (T._lib.PairCountEntry * 4)()
    buf = (C.c_uint8 * 16)()
    assert L.tgx_pair_counts_entries(plan.h, st.h, 0, small, 4, C.byref(n), buf, 16, C.byref(nb), C.byref(err)) != 0
    assert b"entries holds 4 entries, 5 are needed" in err.msg and n.value == 5
    full = (T._lib.PairCountEntry * 5)()
    assert L.tgx_pair_counts_entries(plan.h, st.h, 0, full, 5, C.byref(n), buf, 9, C.byref(nb), C.byref(err)) != 0
    assert b"bytes holds 9 bytes, 10 are needed" in err.msg
    assert L.tgx_pair_counts_entries(plan.h, st.h, 0, full, 5, C.byref(n), None, 0, C.byref(nb), C.byref(err)) != 0
    assert b"string values need a byte buffer" in err.msg
    assert L.tgx_pair_counts_entries(plan.h, st.h, 0, full, 5, C.byref(n), buf, 16, C.byref(nb), C.byref(err)) == 0
    e = full[1]  # ("a", "bc"): a byte range per string side
    raw = bytes(buf)
    assert (raw[e.x_offset:e.x_offset + e.x_length], raw[e.y_offset:e.y_offset + e.y_length], e.count) == (b"a", b"bc", 1)
    assert (e.x_bin, e.y_bin) == (0, 0)
    assert L.tgx_pair_counts_entries(plan.h, st.h, 1, full, 5, C.byref(n), buf, 16, C.byref(nb), C.byref(err)) == 0
    assert (n.value, nb.value) == (3, 2)
    assert [(x.x_bin, x.x_offset, x.x_length, x.y_length, x.count) for x in full[:3]] == [(0, 0, 0, 1, 4), (3, 0, 0, 0, 2), (3, 0, 0, 1, 1)]
    assert L.tgx_pair_counts_entries(plan.h, st.h, 2, None, 0, C.byref(n), None, 0, C.byref(nb), C.byref(err)) == 0
    assert (n.value, nb.value) == (0, 0)  # a range phase has no entries


def test_blob_round_trip_and_merge_by_value():
    plan = pairs_plan()
    blob = pairs_blob()
    st = T.State.deserialize(plan, blob)
    assert st.serialize() == blob
    other = pairs_blob(wire.pair_counts_state(100, 16, VALUE, VALUE, 5, {(b"b", b"x"): 1, (b"c", b"c"): 2}),
                       wire.pair_counts_state(4, 8, BINNED, VALUE, 5, {(3, b"u"): 2, (1, b"u"): 1}),
                       wire.pair_counts_state(4, 8, VALUE, RANGE, 5, both_non_null=3, n=3, lo=-7.0, hi=1.0))
    st.merge([T.State.deserialize(plan, other), T.State.deserialize(plan, blob)])
    summary, counts = st.pair_counts(0)
    assert counts == {(b"", b"x"): 4, (b"a", b"bc"): 2, (b"ab", b"c"): 2, (b"b", b"x"): 7, (b"c", b"c"): 2, (b"\xff", b""): 2}
    assert summary == dict(seen=29, both_non_null=23, distinct=6, counted=19, overflow_rows=2, long_rows=2, non_finite=0,
                           out_of_range=0)
    summary, counts = st.pair_counts(1)
    assert list(counts.items()) == [((0, b"u"), 8), ((1, b"u"), 1), ((3, b""), 4), ((3, b"u"), 4)]
    assert (summary["non_finite"], summary["out_of_range"], summary["both_non_null"]) == (4, 2, 23)
    assert st.pair_range(2) == dict(seen=29, both_non_null=21, n=17, non_finite=4, min=-7.0, max=40.0)
    again = T.State.deserialize(plan, st.serialize())  # equal states, equal bytes
    assert again.serialize() == st.serialize() and again.pair_counts(0) == st.pair_counts(0)
    st.reset()
    empty = dict(seen=0, both_non_null=0, distinct=0, counted=0, overflow_rows=0, long_rows=0, non_finite=0, out_of_range=0)
    assert st.pair_counts(0) == (empty, {}) and st.pair_counts(1) == (empty, {})
    r = st.pair_range(2)
    assert (r["seen"], r["n"]) == (0, 0) and r["min"] != r["min"] and r["max"] != r["max"]  # NaN without rows


def test_a_plan_without_the_kind_keeps_its_blob_bytes():
    plain = T.Plan([spec(T.COUNT, 0)])
    blob = wire.pack(count=[wire.count_acc(12, 11)])
    assert T.State.deserialize(plain, blob).serialize() == blob
    assert struct.pack("<I", wire.PAIR_COUNTS_MAGIC) not in blob
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(pairs_plan(), blob)  # (a plan with the kind needs the section)


def raw_task(max_pairs, mvb, x_side, y_side, counters, entries, n=None, rng=(0, INF, -INF)):
    """counters: seen, both_non_null, overflow_rows, long_rows, non_finite, out_of_range"""
    out = struct.pack("<2I", max_pairs, mvb) + x_side + y_side + struct.pack("<6Q", *counters)
    out += struct.pack("<Q2dQ", rng[0], rng[1], rng[2], len(entries) if n is None else n)
    for (cx, cy), c in entries:
        for cell in (cx, cy):
            out += struct.pack("<q", cell) if isinstance(cell, int) else struct.pack("<I", len(cell)) + cell
        out += struct.pack("<Q", c)
    return out


def text(counters, entries, mvb=16, max_pairs=100, **kw):
    return raw_task(max_pairs, mvb, VALUE, VALUE, counters, entries, **kw)


def mixed(counters, entries, x_side=BINNED, **kw):
    return raw_task(4, 8, x_side, VALUE, counters, entries, **kw)


def ranged(counters, rng, entries=(), **kw):
    return raw_task(4, 8, VALUE, RANGE, counters, list(entries), rng=rng, **kw)


MALFORMED = [
    ("other parameters", text((3, 3, 0, 0, 0, 0), [((b"a", b"b"), 3)], max_pairs=99), None, None),
    ("other parameters", text((3, 3, 0, 0, 0, 0), [((b"a", b"b"), 3)], mvb=17), None, None),
    ("other parameters", None, mixed((3, 3, 0, 0, 0, 0), [((0, b"u"), 3)], x_side=wire.pair_side(2, 4, 1.0, 3.0)), None),
    # the binning compared by its bits: 3.0000000000000004 is another width, 0.9999999999999999 another origin
    ("other parameters", None, mixed((3, 3, 0, 0, 0, 0), [((0, b"u"), 3)], x_side=wire.pair_side(2, 3, 1.0, 3.0000000000000004)), None),
    ("other parameters", None, mixed((3, 3, 0, 0, 0, 0), [((0, b"u"), 3)], x_side=wire.pair_side(2, 3, 0.9999999999999999, 3.0)), None),
    ("other parameters", None, mixed((0, 0, 0, 0, 0, 0), [], x_side=VALUE), None),  # another mode
    ("other parameters", None, None, raw_task(4, 8, VALUE, VALUE, (0, 0, 0, 0, 0, 0), [])),  # a count phase for a range-phase spec
    ("out of order or repeated", text((7, 7, 0, 0, 0, 0), [((b"b", b"x"), 3), ((b"ab", b"x"), 4)]), None, None),
    ("out of order or repeated", text((7, 7, 0, 0, 0, 0), [((b"a", b"y"), 3), ((b"a", b"x"), 4)]), None, None),
    ("out of order or repeated", text((7, 7, 0, 0, 0, 0), [((b"", b""), 3), ((b"", b""), 4)]), None, None),
    ("out of order or repeated", None, mixed((7, 7, 0, 0, 0, 0), [((2, b"u"), 3), ((1, b"u"), 4)]), None),
    ("zero count", text((3, 3, 0, 0, 0, 0), [((b"a", b"x"), 3), ((b"b", b"x"), 0)]), None, None),
    ("a value of 17 bytes, max_value_bytes is 16", text((3, 3, 0, 0, 0, 0), [((b"x" * 17, b"y"), 3)]), None, None),
    ("a value of 17 bytes, max_value_bytes is 16", text((3, 3, 0, 0, 0, 0), [((b"y", b"x" * 17), 3)]), None, None),
    ("bin 4 lies outside [0, 3]", None, mixed((3, 3, 0, 0, 0, 0), [((4, b"u"), 3)]), None),
    ("bin -1 lies outside [0, 3]", None, mixed((3, 3, 0, 0, 0, 0), [((-1, b"u"), 3)]), None),
    ("!= both_non_null", text((10, 8, 0, 0, 0, 0), [((b"a", b"x"), 3), ((b"b", b"x"), 4)]), None, None),   # counted 7 of 8
    ("!= both_non_null", text((10, 7, 1, 0, 0, 0), [((b"a", b"x"), 3), ((b"b", b"x"), 4)]), None, None),   # overflow on top
    ("!= both_non_null", text((10, 9, 1, 2, 0, 0), [((b"a", b"x"), 7)]), None, None),                       # 7 + 1 + 2 != 9
    ("!= both_non_null", None, mixed((10, 9, 0, 0, 2, 1), [((0, b"u"), 7)]), None),                         # 7 + 2 + 1 != 9
    ("!= both_non_null", None, mixed((10, 9, 0, 0, 0, 3), [((0, b"u"), 7)]), None),
    ("!= both_non_null", text((6, 7, 0, 0, 0, 0), [((b"a", b"x"), 3), ((b"b", b"x"), 4)]), None, None),    # both above seen
    ("counts", text((10, 9, 0, 0, 0, 0), [((b"a", b"x"), 2**64 - 1), ((b"b", b"x"), 2)]), None, None),     # a sum that wraps
    ("a count phase with a range", text((3, 3, 0, 0, 0, 0), [((b"a", b"b"), 3)], rng=(1, 0.0, 0.0)), None, None),
    ("a range phase", None, None, ranged((10, 9, 0, 0, 3, 0), (7, 0.0, 1.0))),          # 7 + 3 != 9
    ("a range phase", None, None, ranged((10, 9, 0, 0, 2, 0), (7, 2.0, 1.0))),          # min above max
    ("a range phase", None, None, ranged((10, 9, 0, 0, 2, 0), (7, 0.0, INF))),          # an infinite extreme
    ("a range phase", None, None, ranged((10, 2, 0, 0, 2, 0), (0, 0.0, 1.0))),          # extremes without rows
    ("a range phase", None, None, ranged((10, 9, 0, 1, 2, 0), (7, 0.0, 1.0))),          # long rows in a range phase
    ("a range phase", None, None, ranged((8, 9, 0, 0, 2, 0), (7, 0.0, 1.0))),           # both above seen
    ("a range phase", None, None, ranged((10, 9, 0, 0, 2, 0), (7, 0.0, 1.0), n=1)),     # entries
]


@pytest.mark.parametrize("what,first,second,third", MALFORMED, ids=["%d-%s" % (i, m[0][:12]) for i, m in enumerate(MALFORMED)])
def test_malformed_blobs_are_refused(what, first, second, third):
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + re.escape(what)):
        T.State.deserialize(pairs_plan(), pairs_blob(first, second, third))


def test_the_hand_made_sections_are_accepted_when_well_formed():
    """the builders of MALFORMED, used once on a blob that is in order: what they refuse is the damage, not the builder"""
    blob = pairs_blob(text((12, 10, 1, 1, 0, 0), sorted(TEXT.items())), mixed((12, 10, 0, 0, 2, 1), sorted(MIXED.items())),
                      ranged((12, 9, 0, 0, 2, 0), (7, -2.5, 40.0)))
    assert blob == pairs_blob()
    assert T.State.deserialize(pairs_plan(), blob).serialize() == blob


def test_truncated_blobs_are_refused():
    plan, blob = pairs_plan(), pairs_blob()
    for cut in (1, 8, 9, 20, 60, 100, 200):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])


# ---- MutualInformationAnalyzer's opt-in, without a device -------------------------------------------------------------------
import json  # noqa: E402

import term_amd.suite as S  # noqa: E402

UTF8, INT64, FLOAT64, DICT, VIEW = 3, 1, 2, 5, 6  # tgx_type (include/tgx.h)


def test_absence_of_max_pairs_leaves_the_planned_spec_a_joint_bins_one():
    plain = S.MutualInformationAnalyzer("a", "s", 5)
    assert plain.spec == {"type": "mutual_information", "column1": "a", "column2": "s", "bins": 5}
    for types in ([INT64, FLOAT64], [INT64, UTF8], [UTF8, UTF8], [DICT, VIEW]):
        assert plain.planned_requests(types) == [{"kind": T.JOINT_BINS, "column": "a", "column2": "s"}]
    opted = S.MutualInformationAnalyzer("a", "s", 5, max_pairs=100)
    assert opted.planned_requests([INT64, FLOAT64]) == [{"kind": T.JOINT_BINS, "column": "a", "column2": "s"}]
    modes = {(UTF8, UTF8): (0, 0), (INT64, UTF8): (1, 0), (VIEW, FLOAT64): (0, 1), (DICT, DICT): (0, 0)}
    for types, (mx, my) in modes.items():
        assert opted.planned_requests(list(types)) == [
            {"kind": T.PAIR_COUNTS, "column": "a", "column2": "s",
             "pair_counts": {"max_pairs": 100, "max_value_bytes": 256, "x_mode": mx, "y_mode": my}}]
    assert S.MutualInformationAnalyzer("a", "s", 5, max_pairs=7, max_value_bytes=9).planned_requests([UTF8, UTF8])[0][
        "pair_counts"] == {"max_pairs": 7, "max_value_bytes": 9, "x_mode": 0, "y_mode": 0}


def test_a_declared_binary_column_and_bounds_outside_the_device_are_the_analyzers_errors():
    with pytest.raises(T.TgxError, match="column 's' is declared LargeBinary.*not on the GPU path"):
        S.MutualInformationAnalyzer("a", "s", 5, max_pairs=10, arrow_types=["Utf8", "LargeBinary"]).planned_requests([UTF8, UTF8])
    for kw in (dict(max_pairs=0), dict(max_pairs=65537), dict(max_pairs=5, max_value_bytes=257)):
        with pytest.raises(T.TgxError, match=r"max_pairs must be 1 \.\. 65536"):
            S.MutualInformationAnalyzer("a", "s", 5, **kw).planned_requests([UTF8, UTF8])


def test_the_state_token_by_token():
    an = S.MutualInformationAnalyzer("c", "v", 10, max_pairs=100)
    text = an.state_text_from_pair_counts(dict(seen=9, both_non_null=8, distinct=3, counted=8),
                                          [("A", "High", 3), ("A", "Low", 1), ("Zoë", "High", 4)])
    assert text == ('{"n": 8, "joint_counts": [["A", "High", 3], ["A", "Low", 1], ["Zoë", "High", 4]], '
                    '"x_counts": {"A": 4, "Zoë": 4}, "y_counts": {"High": 7, "Low": 1}, "bins": 10}')  # integer tokens: no 8.0
    mixed = an.state_text_from_pair_counts(dict(seen=4, both_non_null=4, distinct=2, counted=4), [(0, "u", 2), (10, "v", 2)])
    assert json.loads(mixed) == {"n": 4, "joint_counts": [["0.0", "u", 2], ["10.0", "v", 2]], "x_counts": {"0.0": 2, "10.0": 2},
                                 "y_counts": {"u": 2, "v": 2}, "bins": 10}
    assert an.compute_metric_from_state(json.loads(mixed)) == {"type": "Double", "value": 1.0}
    empty = json.loads(an.state_text_from_pair_counts({}, []))
    assert empty == {"n": 0, "joint_counts": [], "x_counts": {}, "y_counts": {}, "bins": 10}


def test_merge_states_of_two_categorical_states():
    an = S.MutualInformationAnalyzer("c", "v", 10, max_pairs=100)
    a = json.loads(an.state_text_from_pair_counts(dict(distinct=2), [("A", "High", 25), ("B", "Low", 25)]))
    b = json.loads(an.state_text_from_pair_counts(dict(distinct=3), [("A", "High", 5), ("A", "Low", 30), ("B", "High", 15)]))
    merged = an.merge_states([a, b])
    assert merged == {"n": 100, "joint_counts": [["A", "High", 30], ["B", "Low", 25], ["A", "Low", 30], ["B", "High", 15]],
                      "x_counts": {"A": 60, "B": 40}, "y_counts": {"High": 45, "Low": 55}, "bins": 10}
    assert merged == S.MutualInformationAnalyzer("c", "v", 10).merge_states([a, b])  # (merge_states is what it was)


@pytest.mark.parametrize("value", ["1e5", " 12 ", "-inf", "NaN", "1_000", "+Infinity", "\t.5\n", "--1"])
def test_the_parse_guard_trips(value):
    an = S.MutualInformationAnalyzer("c", "v", 10, max_pairs=100)
    with pytest.raises(T.TgxError, match="a value of v may parse as a number: the reference would bin this column \\(not on the GPU path\\)"):
        an.state_text_from_pair_counts(dict(distinct=2), [("A", "ok", 1), ("B", value, 1)])
    with pytest.raises(T.TgxError, match="a value of c may parse as a number"):
        an.state_text_from_pair_counts(dict(distinct=1), [(value, "ok", 1)])


def test_the_parse_guard_lets_text_through():
    an = S.MutualInformationAnalyzer("c", "v", 10, max_pairs=100)
    values = ["A", "e", "-", "", "k7", "e-", "+", "infinit", "nano", "1 2", "0x10"]
    state = json.loads(an.state_text_from_pair_counts(dict(distinct=len(values)), [(v, "y", 1) for v in values]))
    assert [c[0] for c in state["joint_counts"]] == values


def test_beyond_the_bounds_and_bad_text_are_the_analyzers_errors():
    an = S.MutualInformationAnalyzer("c", "v", 10, max_pairs=2, max_value_bytes=8)
    ok = [("A", "x", 1)]
    with pytest.raises(T.TgxError, match=r"3 distinct pairs \(max_pairs 2\), 0 overflow rows, 0 rows with a value longer than 8 bytes"):
        an.state_text_from_pair_counts(dict(distinct=3), ok)
    with pytest.raises(T.TgxError, match=r"1 distinct pairs \(max_pairs 2\), 5 overflow rows"):
        an.state_text_from_pair_counts(dict(distinct=1, overflow_rows=5), ok)
    with pytest.raises(T.TgxError, match="7 rows with a value longer than 8 bytes"):
        an.state_text_from_pair_counts(dict(distinct=1, long_rows=7), ok)
    with pytest.raises(T.TgxError, match="4 rows outside the bins"):
        an.state_text_from_pair_counts(dict(distinct=1, out_of_range=4), ok)
    with pytest.raises(T.TgxError, match="a value of c is not valid UTF-8"):
        an.state_text_from_pair_counts(dict(distinct=1), [(b"\xff\xfe", "x", 1)])
    with pytest.raises(T.TgxError, match="a value of v is not valid UTF-8"):
        an.state_text_from_pair_counts(dict(distinct=1), [("A", b"\xc3", 1)])
    assert json.loads(an.state_text_from_pair_counts(dict(distinct=1, non_finite=9), ok))["n"] == 1  # (left out, as JOINT_BINS does)
