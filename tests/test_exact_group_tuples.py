"""tests/exact_group_tuples.py held against itself and against term_amd.group_key: the codec's injectivity and order, the
long-row rule, and the plain walk against its numpy twin -- for counts and for sums."""
import math
import random

import numpy as np
import pytest

import exact_group_sums as exs
import exact_group_tuples as ext
from term_amd import group_key

I64_MIN, I64_MAX = -2**63, 2**63 - 1

HAND = [(None, b""), (b"", None), (b"", b""), (None, None), (-1,), (I64_MAX, I64_MIN), (I64_MIN, I64_MAX), (5,), (5, 5),
        (None, 5), (5, None), (b"a", b"b"), (b"ab", b""), (b"a", b"", b"b"), (b"\x00", None), (None, b"\x00"), (0,), (1,),
        (b"\x01" + bytes(8),), (b"x" * 255, 7), (None,), (b"",)]


def test_the_encoding_is_injective_on_the_hand_list():
    keys = [ext.encode(t) for t in HAND]
    assert len(set(keys)) == len(HAND)
    for t, k in zip(HAND, keys):
        assert ext.decode(k) == t and group_key.encode(t) == k and group_key.decode(k) == t
        assert len(k) == ext.encoded_length(t)
    assert ext.encode((-1,)) == b"\x01\x7f" + b"\xff" * 7
    assert ext.encode((None, b"")) == b"\x00\x02\x00\x00" and ext.encode((b"", None)) == b"\x02\x00\x00\x00"
    assert ext.encode((I64_MAX, I64_MIN)) == b"\x01" + b"\xff" * 8 + b"\x01" + bytes(8)


def test_a_narrow_and_a_wide_five_have_the_same_bytes():
    for narrow in (np.int8(5), np.uint8(5), np.int16(5), np.int32(5), np.uint32(5)):
        assert group_key.encode((narrow, None)) == ext.encode((5, None)) == ext.encode((int(np.int64(5)), None))
    assert ext.encode((int(np.uint8(255)),)) == ext.encode((255,)) != ext.encode((-1,))


def test_bytewise_order_is_the_stated_component_order():
    rng = random.Random(1)
    cells = [None, I64_MIN, -2, -1, 0, 1, 255, 256, I64_MAX, b"", b"\x00", b"a", b"b", b"\xff", b"a\x00", b"ab", b"a" * 20]
    for arity in (1, 2, 3):
        tuples = {tuple(rng.choice(cells) for _ in range(arity)) for _ in range(600)}
        by_bytes = sorted(tuples, key=ext.encode)
        assert by_bytes == sorted(tuples, key=ext.component_order)
    one = sorted(((c,) for c in cells), key=ext.encode)
    assert one == [(c,) for c in cells]  # NULL, the integers in numeric order, the strings by length and then bytewise


def test_the_codec_round_trips_seeded_tuples_and_refuses_what_is_no_key():
    rng = random.Random(2)
    for _ in range(2000):
        t = tuple(rng.choice([None, rng.randint(I64_MIN, I64_MAX), rng.randbytes(rng.choice([0, 1, 2, 40, 300]))])
                  for _ in range(rng.randint(0, 8)))
        k = ext.encode(t)
        assert group_key.encode(t) == k and group_key.decode(k) == t == ext.decode(k)
    for bad in (b"\x03", b"\x01" + bytes(7), b"\x02\x00", b"\x02\x00\x02a", b"\x00\x01", b"\xff"):
        with pytest.raises(ValueError):
            group_key.decode(bad)
    with pytest.raises(ValueError):
        group_key.encode((2**63,))
    with pytest.raises(ValueError):
        group_key.encode((b"x" * 65536,))
    with pytest.raises(TypeError):
        group_key.encode((1.5,))


def test_the_long_row_rule_at_max_value_bytes_and_one_above():
    # (int, string of k bytes): 9 + 3 + k bytes
    values = [1, None, 3, 4]
    cols = [[7, 7, 7, 7], [b"x" * 20, b"x" * 21, b"x" * 21, None]]
    at = ext.walk(values, cols, max_value_bytes=33)
    assert at["long_rows"] == 0 and at["groups"] == 3 and max(map(len, at["entries"])) == 33
    above = ext.walk(values, cols, max_value_bytes=32)
    assert (above["long_rows"], above["long_non_null"], above["groups"]) == (2, 1, 2)
    assert above["counted"] + above["long_rows"] == above["seen"] == 4
    # a string of 65 536 bytes has no form, and is a long row by its length alone
    huge = ext.walk([1], [[b"y" * 65536], [None]], max_value_bytes=256)
    assert (huge["long_rows"], huge["long_non_null"], huge["groups"]) == (1, 1, 0)
    sums = ext.walk_sums(values, cols, max_value_bytes=32)
    assert sums["long_rows"] == (2, 1, 3) and sums["counted"] == (2, 2, 5) and sums["null_group"] == (0, 0, 0)


def test_null_is_a_value():
    w = ext.walk([1, 1, None, 1], [[None, b"", None, None], [b"a", b"a", None, b"a"]])
    assert w["entries"] == {ext.encode((None, None)): (1, 0), ext.encode((None, b"a")): (2, 2), ext.encode((b"", b"a")): (1, 1)}
    assert list(w["entries"]) == [ext.encode((None, None)), ext.encode((None, b"a")), ext.encode((b"", b"a"))]
    assert w["null_group_rows"] == 0 and w["counted"] == w["seen"] == 4


def tables(seed, n, arity):
    rng = np.random.default_rng(seed)
    cols = [rng.integers(-3, 4, n) * (1 if c % 2 else 2**61) for c in range(arity)]
    masks = [rng.random(n) >= 0.2 for _ in range(arity)]
    lists = [[int(v) if ok else None for v, ok in zip(col, m)] for col, m in zip(cols, masks)]
    return rng, cols, masks, lists


@pytest.mark.parametrize("n,arity", [(0, 2), (1, 2), (500, 2), (3000, 3), (800, 8)])
def test_the_walk_and_its_numpy_twin_agree(n, arity):
    rng, cols, masks, lists = tables(n + arity, n, arity)
    valid = rng.random(n) >= 0.3
    values = [1 if ok else None for ok in valid]
    for mvb in (256, 9 * arity - 8):
        a, b = ext.walk(values, lists, mvb), ext.walk_np(valid, cols, masks, mvb)
        assert a == b and list(a["entries"]) == list(b["entries"])
        assert a["counted"] + a["long_rows"] == n and a["counted_non_null"] + a["long_non_null"] == int(valid.sum())


@pytest.mark.parametrize("n,arity", [(0, 2), (700, 2), (900, 8)])
def test_the_sums_walk_and_its_numpy_twin_agree_and_wrap(n, arity):
    rng, cols, masks, lists = tables(50 + n + arity, n, arity)
    valid = rng.random(n) >= 0.3
    vals = rng.choice(np.array([I64_MAX, I64_MIN, -1, 1, 2**62], np.int64), n)
    values = [int(v) if ok else None for v, ok in zip(vals, valid)]
    a, b = ext.walk_sums(values, lists), ext.walk_sums_np(vals, valid, cols, masks)
    assert a == b and list(a["entries"]) == list(b["entries"])
    total = exs.wrap(sum(v for v in values if v is not None))
    assert exs.wrap(a["counted"][2] + a["long_rows"][2]) == total


def test_float_sums_keep_fsum_and_magnitudes_for_the_any_order_bound():
    values = [0.1, 0.2, None, 1e300, -1e300, math.inf, 3.0]
    cols = [[1, 1, 1, 2, 2, 3, None], [b"a", b"a", b"a", None, None, b"", b"z"]]
    w = ext.walk_sums(values, cols, is_float=True)
    e = w["entries"]
    rows, nn, fsum, mags = e[ext.encode((1, b"a"))]
    assert (rows, nn) == (3, 2) and exs.float_failure(0.1 + 0.2, ("bound", None), nn, fsum, mags) is None
    assert exs.float_failure(0.31, ("bound", None), nn, fsum, mags) is not None
    assert e[ext.encode((2, None))][:3] == (2, 2, 0.0) and e[ext.encode((3, b""))][2] == math.inf
    assert w["counted"] == (7, 6) and w["is_float"] and w["null_group"] == exs.float_class(0, [])
