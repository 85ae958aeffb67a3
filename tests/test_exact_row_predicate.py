"""tests/exact_row_predicate.py held to what it is the reference FOR: Kleene's 3x3 tables, and the edge values of the
comparison rules of include/tgx.h (TGX_CHECK_ROW_PREDICATE).  No device, no library."""
import struct

import exact_row_predicate as ex

T, F, U = True, False, None
NAN_POS, NAN_NEG = ex.from_bits(0x7FF8000000000000), ex.from_bits(0xFFF8000000000000)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def test_kleene_tables():
    vals = [T, F, U]
    assert [[ex.k_and(a, b) for b in vals] for a in vals] == [[T, F, U], [F, F, F], [U, F, U]]
    assert [[ex.k_or(a, b) for b in vals] for a in vals] == [[T, T, T], [T, F, U], [T, U, U]]
    assert [ex.k_not(a) for a in vals] == [F, T, U]
    # De Morgan holds in Kleene's logic, UNKNOWN included
    for a in vals:
        for b in vals:
            assert ex.k_not(ex.k_and(a, b)) == ex.k_or(ex.k_not(a), ex.k_not(b))


def test_the_walk_follows_the_tables_on_the_exhaustive_two_column_table():
    types = {"a": "int", "b": "int"}
    leaf = lambda c: ("cmp", c, "=", 1)  # noqa: E731
    truth = {None: U, 0: F, 1: T}
    for x in (None, 0, 1):
        for y in (None, 0, 1):
            row = {"a": x, "b": y}
            assert ex.walk(("and", leaf("a"), leaf("b")), row, types) == ex.k_and(truth[x], truth[y])
            assert ex.walk(("or", leaf("a"), leaf("b")), row, types) == ex.k_or(truth[x], truth[y])
            assert ex.walk(("not", leaf("a")), row, types) == ex.k_not(truth[x])
            assert ex.walk(("isnull", "a"), row, types) == (x is None)


def test_total_order_keys():
    order = [NAN_NEG, -float("inf"), -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, float("inf"), NAN_POS]
    keys = [ex.key(x) for x in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert ex.key(0.0) == 0 and ex.key(-0.0) == -1
    assert struct.pack("<d", ex.from_bits(ex.bits_of(NAN_NEG))) == struct.pack("<d", NAN_NEG)


def test_zeros_and_nans_compare_by_their_keys():
    types = {"x": "float"}
    val = lambda v, op, lit: ex.walk(("cmp", "x", op, lit), {"x": v}, types)  # noqa: E731
    assert val(-0.0, "=", 0.0) is False and val(-0.0, "<", 0.0) is True and val(0.0, "=", 0.0) is True
    assert val(-0.0, "=", -0.0) is True and val(0.0, ">=", 0) is True and val(-0.0, ">=", 0) is False
    assert val(NAN_POS, "=", NAN_POS) is True and val(NAN_NEG, "=", NAN_POS) is False
    assert val(NAN_POS, ">", float("inf")) is True and val(NAN_NEG, "<", -float("inf")) is True
    assert val(None, "=", NAN_POS) is None


def test_an_int64_column_against_integer_and_double_literals():
    types = {"a": "int"}
    val = lambda v, op, lit: ex.walk(("cmp", "a", op, lit), {"a": v}, types)  # noqa: E731
    # 2^53 + 1 is not a double: the conversion rounds to even, to 2^53
    assert val(2**53 + 1, "=", 2.0**53) is True and val(2**53 + 1, "=", 2**53) is False
    assert val(2**53 + 1, ">", 2.0**53) is False and val(2**53 + 1, ">", 2**53) is True
    assert val(2**53 + 3, "=", 2.0**53 + 4) is True  # (ties to even: up)
    assert val(I64_MIN, "<", I64_MIN + 1) is True and val(I64_MIN, "=", -(2.0**63)) is True
    assert val(I64_MAX, "=", 2.0**63) is True and val(I64_MAX, "<", I64_MAX) is False
    assert val(0, "=", -0.0) is False and val(0, ">", -0.0) is True  # (the int 0 is +0.0)
    assert val(None, "<", 5) is None


def test_column_pairs_and_strings():
    types = {"a": "int", "b": "int", "x": "float", "s": "str", "u": "str"}
    row = {"a": 2**53 + 1, "b": 2**53, "x": 2.0**53, "s": b"ab", "u": b"ab"}
    w = lambda t: ex.walk(t, row, types)  # noqa: E731
    assert w(("cmpcol", "a", ">", "b")) is True and w(("cmpcol", "a", "=", "x")) is True and w(("cmpcol", "x", "<", "a")) is False
    assert w(("cmpcol", "s", "=", "u")) is True and w(("streq", "s", b"ab")) is True
    assert w(("streq", "s", b"a")) is False and w(("streq", "s", b"abc")) is False and w(("streq", "s", b"")) is False
    assert ex.walk(("streq", "s", b""), dict(row, s=b""), types) is True
    assert ex.walk(("cmpcol", "s", "=", "u"), dict(row, u=None), types) is None


def test_sqls_definitions_of_what_is_no_leaf():
    types = {"a": "int", "s": "str"}
    for v, want_in, want_not_in in ((1, T, F), (5, F, T), (None, U, U)):
        row = {"a": v, "s": None}
        assert ex.walk(ex.isin("a", [1, 2, 3]), row, types) == want_in
        assert ex.walk(("not", ex.isin("a", [1, 2, 3])), row, types) == want_not_in
    assert ex.walk(ex.between("a", 5, 1), {"a": 3, "s": None}, types) is False  # lo > hi matches nothing
    assert ex.walk(("not", ex.between("a", 5, 1)), {"a": 3, "s": None}, types) is True
    assert ex.walk(ex.ne("s", b"x"), {"a": 0, "s": None}, types) is None
    assert ex.counts(ex.ne("a", 1), ex.table_rows({"a": [1, 2, None], "s": [None] * 3}), types) == (3, 1, 1, 1)


def test_the_lowering_and_the_interpreter_agree_with_the_walk():
    """leaves_and_program is the tests' own lowering for the C ABI; run through run_compiled's interpreter it must give
    what the walk gives"""
    types = {"a": "int", "x": "float", "s": "str"}
    tree = ("or", ("and", ex.between("a", -1, 1.5), ("not", ("streq", "s", b"k"))), ("cmpcol", "a", "<=", "x"))
    cols = ["a", "x", "s"]
    leaves, program, pool = ex.leaves_and_program(tree, cols)
    compiled = {"columns": cols, "program": [list(p) for p in program], "literals_hex": pool.hex(),
                "leaves": [dict({"op": 0, "col2": 0, "flags": 0, "lit_i": 0, "lit_offset": 0, "lit_len": 0}, **dict(
                    l, lit_f_bits=ex.bits_of(l.get("lit_f", 0.0)) & ((1 << 64) - 1))) for l in leaves]}
    for a in (None, -1, 0, 2):
        for x in (None, -0.0, 1.5, NAN_POS):
            for s in (None, b"k", b"kk"):
                row = {"a": a, "x": x, "s": s}
                assert ex.run_compiled(compiled, row, types) == ex.walk(tree, row, types)
