"""The string leaves of TGX_CHECK_ROW_PREDICATE (STR_CMP, STR_LENGTH, STR_LIKE, STR_BLANK) without a device: the
constants and symbols, every new refusal of the setter, the functions the kernel compiles run on the host
(tgx_host_string_leaf) against tests/exact_string_predicates.py, the compiler's dialect `string_functions` held to
hand-written trees, its refusals by name, the opt-in that keeps today's answers without it, the superset property, the
DataTypeConstraint plans and verdicts, and blobs through term_amd/wire.py."""
import json
import os
import random

import pytest

import exact_row_predicate as ex
import exact_string_predicates as xs
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "custom_sql_vectors.json")) as _f:
    G = json.load(_f)

PUSH0 = [(T.PRED_PUSH, 0)]
OPS = {"<": T.PRED_LT, "<=": T.PRED_LE, ">": T.PRED_GT, ">=": T.PRED_GE, "=": T.PRED_EQ}


def one_spec_plan(n_columns=1):
    return T.Plan([spec(T.ROW_PREDICATE, 0, columns=list(range(n_columns))), spec(T.COUNT, 0)])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_constants_and_symbols():
    assert T.lib().tgx_abi_version() == 6
    assert (T.PRED_STR_CMP, T.PRED_STR_LENGTH, T.PRED_STR_LIKE, T.PRED_STR_BLANK) == \
        (xs.STR_CMP, xs.STR_LENGTH, xs.STR_LIKE, xs.STR_BLANK) == (6, 7, 8, 9)
    assert T.PRED_LENGTH_IN_BYTES == xs.LENGTH_IN_BYTES == 2
    for name in ("tgx_host_string_leaf", "tgx_host_row_predicate_json_ex"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)
    with open(os.path.join(HERE, "..", "include", "tgx.h")) as f:
        header = f.read()
    assert "KIND 5 IS UNASSIGNED" in header and "TGX_PRED_STR_BLANK = 9" in header


def test_every_new_refusal_of_the_setter_and_what_is_allowed():
    plan = one_spec_plan(2)
    cmp_, length = dict(kind=T.PRED_STR_CMP, col=0, op=T.PRED_LT), dict(kind=T.PRED_STR_LENGTH, col=0, op=T.PRED_EQ)
    like, blank = dict(kind=T.PRED_STR_LIKE, col=0), dict(kind=T.PRED_STR_BLANK, col=0)
    bad = [
        (dict(leaves=[dict(kind=0, col=0)], program=PUSH0), "unknown leaf kind 0"),
        (dict(leaves=[dict(kind=5, col=0)], program=PUSH0), "unknown leaf kind 5"),
        (dict(leaves=[dict(kind=10, col=0)], program=PUSH0), "unknown leaf kind 10"),
        (dict(leaves=[dict(kind=77, col=0)], program=PUSH0), "unknown leaf kind 77"),
        (dict(leaves=[dict(cmp_, op=T.PRED_EQ)], program=PUSH0), "use STR_EQ"),
        (dict(leaves=[dict(cmp_, op=0)], program=PUSH0), "unknown comparison 0"),
        (dict(leaves=[dict(cmp_, op=6)], program=PUSH0), "unknown comparison 6"),
        (dict(leaves=[dict(length, op=0)], program=PUSH0), "unknown comparison 0"),
        (dict(leaves=[dict(length, op=6)], program=PUSH0), "unknown comparison 6"),
        (dict(leaves=[dict(length, flags=1)], program=PUSH0), "unknown flags 0x1"),
        (dict(leaves=[dict(length, flags=6)], program=PUSH0), "unknown flags 0x6"),
        (dict(leaves=[dict(cmp_, flags=2)], program=PUSH0), "unknown flags 0x2"),
        (dict(leaves=[dict(like, flags=2)], program=PUSH0), "unknown flags 0x2"),
        (dict(leaves=[dict(blank, flags=2)], program=PUSH0), "unknown flags 0x2"),
        (dict(leaves=[dict(kind=T.PRED_CMP_LITERAL, op=T.PRED_EQ, col=0, flags=2)], program=PUSH0), "unknown flags 0x2"),
        (dict(leaves=[dict(cmp_, lit_offset=2, lit_len=3)], program=PUSH0, literals=b"abcd"),
         r"names literal bytes \[2, 2 \+ 3\) of a pool of 4"),
        (dict(leaves=[dict(like, lit_offset=5, lit_len=0)], program=PUSH0, literals=b"abcd"), "names literal bytes"),
        (dict(leaves=[dict(like, lit_offset=0, lit_len=257)], program=PUSH0, literals=bytes(256)), "names literal bytes"),
        (dict(leaves=[dict(like, lit_offset=1, lit_len=2)], program=PUSH0, literals=b"a\\%b"), r"backslash \(0x5C\)"),
        (dict(leaves=[dict(like, lit_offset=0, lit_len=1)], program=PUSH0, literals=b"\\"), r"backslash \(0x5C\)"),
        (dict(leaves=[dict(like, col=2)], program=PUSH0), "names column slot 2 of a list of 2"),
    ]
    for args, message in bad:
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + message):
            plan.set_row_predicate(0, **args)
    # what is allowed: a 256-byte pattern, the empty pattern at the pool's end, a backslash outside the pattern's range,
    # a backslash in STR_CMP's and STR_EQ's literal, every op of each kind, the byte flag
    plan.set_row_predicate(0, [dict(like, lit_offset=0, lit_len=256)], PUSH0, b"%" + b"a" * 255)
    plan.set_row_predicate(0, [dict(like, lit_offset=256, lit_len=0)], PUSH0, bytes(256))
    plan.set_row_predicate(0, [dict(like, lit_offset=1, lit_len=2)], PUSH0, b"\\a%\\")
    plan.set_row_predicate(0, [dict(cmp_, lit_offset=0, lit_len=1), dict(kind=T.PRED_STR_EQ, col=1, lit_len=1)],
                           PUSH0 + [(T.PRED_PUSH, 1), (T.PRED_AND, 0)], b"\\")
    for op in (T.PRED_LT, T.PRED_LE, T.PRED_GT, T.PRED_GE):
        plan.set_row_predicate(0, [dict(cmp_, op=op)], PUSH0)
    for op in (T.PRED_EQ, T.PRED_LT, T.PRED_LE, T.PRED_GT, T.PRED_GE):
        plan.set_row_predicate(0, [dict(length, op=op, flags=T.PRED_LENGTH_IN_BYTES, lit_i=-(1 << 63))], PUSH0)
    plan.set_row_predicate(0, [dict(blank, op=3, lit_i=9)], PUSH0)  # (what a leaf does not read is dropped, not refused)


LEAVES = [dict(kind=T.PRED_STR_LIKE, col=0, lit_offset=0, lit_len=3), dict(kind=T.PRED_STR_LENGTH, col=0, op=T.PRED_GE, lit_i=2),
          dict(kind=T.PRED_STR_CMP, col=0, op=T.PRED_LT, lit_offset=3, lit_len=1), dict(kind=T.PRED_STR_BLANK, col=0)]
PROGRAM = [(T.PRED_PUSH, 0), (T.PRED_PUSH, 1), (T.PRED_AND, 0), (T.PRED_PUSH, 2), (T.PRED_OR, 0), (T.PRED_PUSH, 3), (T.PRED_NOT, 0),
           (T.PRED_AND, 0)]


def leaf_plan(pool=b"a%bq"):
    plan = T.Plan([spec(T.ROW_PREDICATE, 0, columns=[0]), spec(T.COUNT, 0)])
    plan.set_row_predicate(0, LEAVES, PROGRAM, pool)
    return plan


def leaf_blob(pool=b"a%bq", leaves=LEAVES, counts=(10, 5, 2)):
    return wire.pack(count=[wire.count_acc(10, 9)], row_predicates=[wire.row_predicate_state(leaves, PROGRAM, pool, *counts)])


def test_a_blob_of_the_new_kinds_round_trips_and_one_under_another_pattern_is_refused():
    plan = leaf_plan()
    blob = leaf_blob()
    st = T.State.deserialize(plan, blob)
    assert st.row_predicate_counts(0) == (10, 5, 2, 3)
    assert st.serialize() == blob
    st.merge([T.State.deserialize(plan, blob)])
    assert st.row_predicate_counts(0) == (20, 10, 4, 6)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*task 0.*other literal bytes"):  # another pattern
        T.State.deserialize(plan, leaf_blob(pool=b"a_bq"))
    other_length = [LEAVES[0], dict(LEAVES[1], flags=T.PRED_LENGTH_IN_BYTES)] + LEAVES[2:]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*task 0.*other leaves"):
        T.State.deserialize(plan, leaf_blob(leaves=other_length))
    # what the setter drops of a leaf is zero in the blob: a state of a plan set with stray fields writes the same bytes
    stray = T.Plan([spec(T.ROW_PREDICATE, 0, columns=[0]), spec(T.COUNT, 0)])
    stray.set_row_predicate(0, [dict(LEAVES[0], op=3, lit_i=5), LEAVES[1], LEAVES[2], dict(LEAVES[3], lit_len=2)], PROGRAM, b"a%bq")
    assert T.State.deserialize(stray, blob).serialize() == blob


# ---- the kernel's functions on the host -------------------------------------------------------------------------------------
VALUES = xs.seeded_values()
PATTERNS = xs.seeded_patterns()
TYPES = {"s": "str"}


def host(tree, value, align=0):
    """a leaf tree of exact_string_predicates through tgx_host_string_leaf"""
    head = tree[0]
    if head == "strcmp":
        return T.host_string_leaf(T.PRED_STR_CMP, value, op=OPS[tree[2]], pattern=tree[3], align=align)
    if head == "strlen":
        return T.host_string_leaf(T.PRED_STR_LENGTH, value, op=OPS[tree[2]], lit_i=tree[3],
                                  flags=T.PRED_LENGTH_IN_BYTES if tree[4] else 0, align=align)
    if head == "like":
        return T.host_string_leaf(T.PRED_STR_LIKE, value, pattern=tree[2], align=align)
    return T.host_string_leaf(T.PRED_STR_BLANK, value, align=align)


def test_the_host_leaf_equals_the_exact_reference_on_the_seeded_set():
    for k, p in enumerate(PATTERNS):
        tree = ("like", "s", p)
        for i, v in enumerate(VALUES):
            assert host(tree, v, (i + k) & 3) is xs.leaf(tree, {"s": v}, TYPES), (p, v)


def test_length_order_and_blank_on_the_seeded_values_at_every_alignment():
    literals = [b"", b"a", b"ab", "é".encode(), "日".encode(), b"b", b" ", b"a\n", "a日b".encode(), b"aaaa", b"aaaab"]
    for i, v in enumerate(VALUES[:500]):
        row = {"s": v}
        for align in range(4):
            for tree in (("strlen", "s", "=", xs.characters(v), False), ("strlen", "s", "<", 3, False),
                         ("strlen", "s", ">=", 4, True), ("blank", "s"),
                         ("strcmp", "s", ("<", "<=", ">", ">=")[i & 3], literals[(i + align) % len(literals)])):
                assert host(tree, v, align) is xs.leaf(tree, row, TYPES), (tree, v, align)


NOT_UTF8 = [b"\x80", b"\x80\x80", b"\x80a", b"a\x80", b"a\x80\x80", b"\xe6\x97", b"\xe6\x97a", b"\xe6", b"a\xe6", b"\xc3", b"\xc3\xc3",
            b"\xf0\x9f\x98", b"\xff\xfe", b"\xbf\xbf\xbfa\xbf", b"ab\xe6\x97", b"\xe6\x97\xa5\xa5", b"\x80 \x80", b"  \xa0", b"\x00", b""]
NOT_UTF8_PATTERNS = [b"_", b"__", b"___", b"%", b"_%", b"%_", b"%\x97", b"%\xe6_", b"\xe6%", b"\xe6%\xa5", b"a_", b"%\x80", b"\x80%",
                     b"%\x80%", b"_\x80", b"%a", b"%\xbf_", b"%_\xbf", b"%\xbf%\xbf", b"", b"\xe6\x97", b"%\x98", b"%\xa5\xa5"]


def test_the_host_leaf_equals_the_exact_reference_on_bytes_that_are_no_utf8():
    for v in NOT_UTF8:
        row = {"s": v}
        for align in range(4):
            for p in NOT_UTF8_PATTERNS:
                assert host(("like", "s", p), v, align) is xs.like(v, p), (p, v, align)
            for tree in (("strlen", "s", "=", xs.characters(v), False), ("strlen", "s", "=", len(v), True), ("blank", "s"),
                         ("strcmp", "s", "<", b"\x80"), ("strcmp", "s", ">=", b"\xe6\x97"), ("strcmp", "s", "<=", b"a\x80")):
                assert host(tree, v, align) is xs.leaf(tree, row, TYPES), (tree, v, align)


def test_long_values_and_random_bytes_at_every_alignment():
    rng = random.Random(7)
    for n in (255, 256, 257, 4099):
        v = bytes(rng.choice((0x61, 0x62, 0x20, 0xC3, 0xA9, 0x97)) for _ in range(n))
        lit = v[:n - 1] + bytes([v[n - 1] ^ 1])
        for align in range(4):
            assert host(("strlen", "s", "=", xs.characters(v), False), v, align)
            assert host(("strcmp", "s", ">=", v), v, align) and not host(("strcmp", "s", "<", v), v, align)
            assert host(("strcmp", "s", "<", lit), v, align) is (v < lit)
            assert host(("strcmp", "s", ">", v[:200]), v, align) and host(("strcmp", "s", "<", v + b"\x00"), v[:200], align)
            assert host(("blank", "s"), b" " * n, align) and not host(("blank", "s"), b" " * (n - 1) + b"\t", align)
            for p in (b"%" + v[-3:], v[:2] + b"%", b"%" + v[100:104] + b"%", b"%_", b"_%_", v[:5] + b"%" + v[-5:], b"%\x00"):
                assert host(("like", "s", p), v, align) is xs.like(v, p), (p, n, align)


def test_the_host_leaf_refuses_what_the_setter_refuses():
    for args in (dict(kind=T.PRED_STR_CMP, op=T.PRED_EQ), dict(kind=T.PRED_STR_CMP, op=0), dict(kind=T.PRED_STR_LENGTH, op=0),
                 dict(kind=T.PRED_STR_LENGTH, op=1, flags=1), dict(kind=T.PRED_STR_LIKE, pattern=b"a\\"), dict(kind=T.PRED_STR_EQ),
                 dict(kind=5), dict(kind=10), dict(kind=T.PRED_STR_BLANK, flags=2), dict(kind=T.PRED_STR_LIKE, flags=2)):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.host_string_leaf(args.pop("kind"), b"abc", **args)


# ---- the compiler's dialect -------------------------------------------------------------------------------------------------
ROWS = [{"s": s, "t": t, "a": a} for s in (None, b"", b" ", b"  ", b"F", b"Foo", "fée".encode(), "日本語".encode(), b"4111", b"a@b.com",
                                           b"1998-09-01", b"1998-12-01", b"x\ny")
        for t in (None, b"F") for a in (None, 0, 5)]
ROW_TYPES = {"s": "str", "t": "str", "a": "int"}
like_, nlike = (lambda c, p: ("like", c, p)), (lambda c, p: ("not", ("like", c, p)))
ln = lambda c, op, n, b=False: ("strlen", c, op, n, b)  # noqa: E731

ATOMS = [
    ("s LIKE 'F%'", like_("s", b"F%")), ("s NOT LIKE '%@b.com'", nlike("s", b"%@b.com")), ("s like '4%'", like_("s", b"4%")),
    ("s LIKE ''", like_("s", b"")), ("s LIKE '%'", like_("s", b"%")), ("s LIKE 'x_y'", like_("s", b"x_y")),
    ("s LIKE '_本%'", like_("s", "_本%".encode())), ("s LIKE 'it''s'", like_("s", b"it's")), ('"s" LIKE \'F__\'', like_("s", b"F__")),
    ("NOT s LIKE 'F%'", nlike("s", b"F%")), ("NOT s NOT LIKE 'F%'", ("not", nlike("s", b"F%"))),
    ("LENGTH(s) >= 5", ln("s", ">=", 5)), ("length(s) = 3", ln("s", "=", 3)), ("CHAR_LENGTH(s) < 4", ln("s", "<", 4)),
    ("CHARACTER_LENGTH(s) <= 3", ln("s", "<=", 3)), ("OCTET_LENGTH(s) <= 4", ln("s", "<=", 4, True)),
    ("octet_length(s) > 8", ln("s", ">", 8, True)), ("LENGTH(s) <> 3", ("not", ln("s", "=", 3))),
    ("LENGTH(s) != 0", ("not", ln("s", "=", 0))), ("LENGTH(s) > -1", ln("s", ">", -1)), ('LENGTH("s") > 0', ln("s", ">", 0)),
    ("5 <= LENGTH(s)", ln("s", ">=", 5)), ("3 > OCTET_LENGTH(s)", ln("s", "<", 3, True)), ("3 = LENGTH(s)", ln("s", "=", 3)),
    ("3 <> LENGTH(s)", ("not", ln("s", "=", 3))),
    ("LENGTH(s) BETWEEN 1 AND 3", xs.len_between("s", 1, 3)), ("LENGTH(s) NOT BETWEEN 1 AND 3", ("not", xs.len_between("s", 1, 3))),
    ("OCTET_LENGTH(s) BETWEEN 4 AND 9", xs.len_between("s", 4, 9, True)),
    ("TRIM(s) = ''", ("blank", "s")), ("TRIM(s) <> ''", ("not", ("blank", "s"))), ("trim(s) != ''", ("not", ("blank", "s"))),
    ("'' = TRIM(s)", ("blank", "s")), ("'' <> TRIM(s)", ("not", ("blank", "s"))),
    ("s < 'G'", ("strcmp", "s", "<", b"G")), ("s <= '1998-09-01'", ("strcmp", "s", "<=", b"1998-09-01")),
    ("s > 'F'", ("strcmp", "s", ">", b"F")), ("s >= 'Foo'", ("strcmp", "s", ">=", b"Foo")), ("'G' > s", ("strcmp", "s", "<", b"G")),
    ("'F' <= s", ("strcmp", "s", ">=", b"F")), ("s < ''", ("strcmp", "s", "<", b"")),
    ("s BETWEEN '1998-01-01' AND '1998-09-30'", xs.str_between("s", b"1998-01-01", b"1998-09-30")),
    ("s NOT BETWEEN 'A' AND 'Z'", ("not", xs.str_between("s", b"A", b"Z"))),
    ("s LIKE 'F%' AND (LENGTH(s) > 1 OR a >= 5) AND t = 'F'",
     ("and", ("and", like_("s", b"F%"), ("or", ln("s", ">", 1), ("cmp", "a", ">=", 5))), ("streq", "t", b"F"))),
    ("s IS NOT NULL AND TRIM(s) <> '' AND s <> 'F' AND NOT t LIKE '_'",
     ("and", ("and", ("and", ("not", ("isnull", "s")), ("not", ("blank", "s"))), ("not", ("streq", "s", b"F"))), nlike("t", b"_"))),
]


@pytest.mark.parametrize("expression,tree", ATOMS, ids=[e for e, _ in ATOMS])
def test_the_compiled_program_equals_the_tree(expression, tree):
    compiled = S.row_predicate(expression, string_functions=True)
    for row in ROWS:
        assert xs.run_compiled(compiled, row, ROW_TYPES) == xs.walk(tree, row, ROW_TYPES), row
    # ... and the setter takes what the compiler makes
    plan = one_spec_plan(len(compiled["columns"]))
    leaves = [{k: v for k, v in lf.items() if k not in ("lit_f_bits",)} for lf in compiled["leaves"]]
    plan.set_row_predicate(0, leaves, [tuple(op) for op in compiled["program"]], bytes.fromhex(compiled["literals_hex"]))


def test_the_answers_over_the_rows_are_not_all_one():
    seen = set()
    for expression, tree in ATOMS:
        seen |= {xs.walk(tree, row, ROW_TYPES) for row in ROWS}
        assert len({xs.walk(tree, row, ROW_TYPES) for row in ROWS}) >= 2, expression
    assert seen == {True, False, None}


def test_the_lowering_is_the_hand_written_one():
    c = S.row_predicate("s LIKE 'a%' AND OCTET_LENGTH(s) <= 7 AND s >= 'a' AND TRIM(s) <> ''", string_functions=True)
    tree = ("and", ("and", ("and", like_("s", b"a%"), ln("s", "<=", 7, True)), ("strcmp", "s", ">=", b"a")), ("not", ("blank", "s")))
    leaves, program, pool = xs.leaves_and_program(tree, ["s"])
    assert c["columns"] == ["s"] and bytes.fromhex(c["literals_hex"]) == pool == b"a%a"
    assert [list(p) for p in program] == c["program"]
    for mine, theirs in zip(leaves, c["leaves"]):
        assert {k: theirs[k] for k in mine} == mine
        assert all(theirs[k] == 0 for k in theirs if k not in mine)


REFUSED = [
    ("s ILIKE 'f%'", "ILIKE"), ("s NOT ILIKE 'f%'", "ILIKE"), ("s SIMILAR TO 'f'", "SIMILAR"), ("s LIKE 'a!%' ESCAPE '!'", "an ESCAPE clause"),
    ("s LIKE 'a\\%'", "a LIKE pattern with a backslash"), ("s NOT LIKE '\\'", "a LIKE pattern with a backslash"),
    ("s LIKE t", "where LIKE's pattern should stand"), ("s LIKE 5", "where LIKE's pattern should stand"), ("'a' LIKE s", "LIKE of a literal"),
    ("s LIKE 'a' || 'b'", "arithmetic"), ("LENGTH(s) > 1.5", "a length compared with a float literal"),
    ("LENGTH(s) = 1e0", "a length compared with a float literal"), ("LENGTH(s) > a", "a length compared with a column"),
    ("a < LENGTH(s)", "a length compared with a column"), ("LENGTH(s) = LENGTH(t)", "a length compared with a function call"),
    ("LENGTH(s) = '3'", "a length compared with a string literal"), ("LENGTH(s) BETWEEN 1 AND 2.5", "a length compared with a float literal"),
    ("LENGTH(TRIM(s)) > 0", "a nested function call"), ("TRIM(LENGTH(s)) = ''", "a nested function call"),
    ("LENGTH(UPPER(s)) > 0", r"a function call \(UPPER"), ("LENGTH(s) IN (1, 2)", "IN on a length"), ("LENGTH(s) NOT IN (1)", "IN on a length"),
    ("LENGTH(s) IS NULL", "IS .NOT. NULL of a function call"), ("LENGTH('abc') = 3", "LENGTH of a literal"), ("LENGTH(s, t) = 3", "several arguments"),
    ("LENGTH(s) + 1 > 2", "arithmetic"), ("LENGTH(s)", "where a comparison should stand"), ("LENGTH(s) LIKE '1'", "LIKE on a length"),
    ("TRIM(s) = 'x'", "TRIM.col. compared with anything but ''"), ("TRIM(s) = ' '", "anything but ''"), ("TRIM(s) = t", "anything but ''"),
    ("TRIM(s) = 5", "anything but ''"), ("TRIM(s) < ''", "TRIM.col. under an order comparison"), ("TRIM(s) IN ('')", "IN on TRIM"),
    ("TRIM(s) BETWEEN '' AND ''", "anything but ''"), ("LTRIM(s) = ''", "LTRIM"), ("RTRIM(s) <> ''", "RTRIM"), ("BTRIM(s) = ''", "BTRIM"),
    ("TRIM(BOTH ' ' FROM s) = ''", r"TRIM\(\.\. FROM \.\.\)"), ("TRIM(' ' FROM s) = ''", r"TRIM\(\.\. FROM \.\.\)"),
    ("TRIM(LEADING FROM s) = ''", r"TRIM\(\.\. FROM \.\.\)"), ("UPPER(s) = 'A'", r"a function call \(UPPER\(\.\.\)\)"),
    ("ABS(a) = 1", r"a function call \(ABS"), ("s < t", None), ("s BETWEEN 'a' AND 5", "a BETWEEN that mixes strings and numbers"),
    ("s IN (LENGTH(s))", "a function call where a literal should stand"),
    ("s LIKE '%s'" % ("y" * 257), "more than 256 literal bytes"),
]


@pytest.mark.parametrize("expression,message", [r for r in REFUSED if r[1]], ids=[e[:40] for e, m in REFUSED if m])
def test_what_stays_outside_the_dialect_is_refused_with_its_name(expression, message):
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED: the expression is not on the GPU path: .*(" + message + ")"):
        S.row_predicate(expression, string_functions=True)


def test_two_string_columns_are_ordered_by_nothing():
    # the compiler has no types: `s < t` is a CMP_COLUMNS leaf in both dialects, and the device refuses it on strings
    assert S.row_predicate("s < t", string_functions=True) == S.row_predicate("s < t")
    assert S.row_predicate("s < t")["leaves"][0]["kind"] == T.PRED_CMP_COLUMNS


def test_without_the_opt_in_the_refusals_are_todays():
    today = {"LENGTH(s) > 3": "a function call (LENGTH(..))", "s LIKE 'F%'": "LIKE", "s NOT LIKE 'F%'": "LIKE",
             "s < 'F'": "a string order comparison (only = and <> compare strings)",
             "s BETWEEN 'A' AND 'Z'": "a string order comparison (BETWEEN on a string literal)",
             "TRIM(s) <> ''": "a function call (TRIM(..))", "OCTET_LENGTH(s) <= 9": "a function call (OCTET_LENGTH(..))"}
    for expression, what in today.items():
        for compile_ in (S.row_predicate, lambda e: S.row_predicate(e, string_functions=False)):
            with pytest.raises(T.TgxError) as e:
                compile_(expression)
            assert str(e.value) == "TGX_UNSUPPORTED: the expression is not on the GPU path: " + what
        with pytest.raises(T.TgxError) as e:
            S.constraint_plan({"type": "custom_sql", "expression": expression})
        assert str(e.value).endswith("'custom_sql': the expression is not on the GPU path: %s. Expression: '%s'" % (what, expression))
        with pytest.raises(T.TgxError) as e:
            S.constraint_plan({"type": "custom_sql", "expression": expression, "string_functions_on_device": False})
        assert "not on the GPU path: " + what in str(e.value)
        with pytest.raises(T.TgxError, match="Invalid configuration: Invalid predicate .*not on the GPU path"):
            S.ComplianceAnalyzer("n", expression).planned_requests([T.UTF8])
        # ... and with it they plan
        plan = S.constraint_plan({"type": "custom_sql", "expression": expression, "string_functions_on_device": True})
        assert plan["requests"][0]["row_predicate"] == S.row_predicate(expression, string_functions=True)
        assert S.ComplianceAnalyzer("n", expression, string_functions_on_device=True).planned_requests([T.UTF8]) == \
            [{"kind": T.ROW_PREDICATE, "column": "s", "column2": ""}]


def golden_expressions():
    g = G["custom_sql"]
    out = list(g["accepted"]) + [sql for sql, _ in g["rejected"]] + [c["expression"] for c in g["cases"]]
    out += [G["compliance"]["predicate"]] + [p for p, _ in G["compliance"]["rejected"]]
    return out


def test_the_dialect_is_a_superset_of_the_base():
    import test_row_predicate_host as base_tests

    expressions = golden_expressions() + [e for e, _, _ in base_tests.EXPRESSIONS]
    accepted = 0
    for expression in expressions:
        try:
            base = S.row_predicate(expression)
        except T.TgxError:
            continue
        assert S.row_predicate(expression, string_functions=True) == base, expression
        accepted += 1
    assert accepted >= 40
    # what the base refuses for a reason the dialect does not lift keeps its text
    for expression, _ in base_tests.REFUSED:
        try:
            S.row_predicate(expression, string_functions=True)
        except T.TgxError as extended:
            with pytest.raises(T.TgxError) as e:
                S.row_predicate(expression)
            if not any(w in str(e.value) for w in ("a function call", "LIKE", "a string order comparison")):
                assert str(extended) == str(e.value), expression


# ---- the surfaces -----------------------------------------------------------------------------------------------------------
def test_the_opt_in_is_written_only_when_called():
    assert S.CustomSqlConstraint("LENGTH(s) > 3").spec == {"type": "custom_sql", "expression": "LENGTH(s) > 3"}
    assert S.CustomSqlConstraint("LENGTH(s) > 3", "h").string_functions_on_device().spec == \
        {"type": "custom_sql", "expression": "LENGTH(s) > 3", "hint": "h", "string_functions_on_device": True}
    assert S.CustomSqlConstraint("a = 1").string_functions_on_device(False).spec["string_functions_on_device"] is False
    check = S.Check.builder("c").satisfies("s LIKE 'a%'").satisfies("s LIKE 'a%'", None, True).build()
    specs = check.spec["constraints"]
    assert "string_functions_on_device" not in specs[0] and specs[1]["string_functions_on_device"] is True
    assert S.ComplianceAnalyzer("n", "a = 1").spec == {"type": "compliance", "name": "n", "predicate": "a = 1"}
    assert S.ComplianceAnalyzer("n", "a = 1", string_functions_on_device=True).spec["string_functions_on_device"] is True
    d = S.DataTypeConstraint("c", S.DataTypeValidation.String(S.StringTypeValidation.NotEmpty))
    assert "string_functions_on_device" not in d.spec and d.string_functions_on_device().spec["string_functions_on_device"] is True


def test_one_expression_one_spec_whatever_the_dialect():
    base = S.constraint_plan({"type": "custom_sql", "expression": "a >= 3 AND s = 'F'"})
    opted = S.constraint_plan({"type": "custom_sql", "expression": "a >= 3 AND s = 'F'", "string_functions_on_device": True})
    assert base["requests"] == opted["requests"]


def test_verdicts_and_messages_are_the_constraints_own():
    spec_ = {"type": "custom_sql", "expression": "email NOT LIKE '%@competitor.com'", "string_functions_on_device": True}
    v = S.constraint_verdict(spec_, [{"total": 5, "matches": 4, "non_null": 5}])
    assert (v["status"], v["metric"]) == ("failure", 0.8)
    assert v["message"] == "Custom SQL condition not satisfied for 1 rows. Expression: 'email NOT LIKE '%@competitor.com''"
    v = S.constraint_verdict(dict(spec_, hint="No competitor addresses"), [{"total": 5, "matches": 5, "non_null": 5}])
    assert (v["status"], v["metric"], v["message"]) == ("success", 1.0, None)
    assert S.constraint_verdict(spec_, [{"total": 0, "matches": 0}])["status"] == "skipped"
    # the reference's validation comes first, with or without the opt-in
    with pytest.raises(T.TgxError, match="Validation failed: SQL expression contains forbidden operation: DROP"):
        S.constraint_plan({"type": "custom_sql", "expression": "s LIKE 'DROP' OR drop = 1", "string_functions_on_device": True})


SV, DV = S.StringTypeValidation, S.DataTypeValidation
STRING_VALIDATIONS = [
    (SV.NotEmpty, "non-empty strings", ln("name", ">", 0)),
    (SV.ValidUtf8, "valid UTF-8 strings", ("not", ("isnull", "name"))),
    (SV.NotBlank, "non-blank strings", ("not", ("blank", "name"))),
    (SV.MaxBytes(5), "strings with max 5 bytes", ln("name", "<=", 5, True)),
]


@pytest.mark.parametrize("validation,description,tree", STRING_VALIDATIONS, ids=[d for _, d, _ in STRING_VALIDATIONS])
def test_the_string_validations_of_datatype_plan_one_row_predicate_and_keep_the_references_verdict(validation, description, tree):
    plain = S.DataTypeConstraint("name", DV.String(validation))
    today = "Constraint evaluation failed for 'datatype': %s validation reads a string column (not on the GPU path)" % description
    for call in (lambda: S.constraint_plan(plain.spec), lambda: S.constraint_verdict(plain.spec, [{"total": 4, "matches": 4, "non_null": 4}]),
                 lambda: S.constraint_plan(dict(plain.spec, string_functions_on_device=False))):
        with pytest.raises(T.TgxError) as e:
            call()
        assert str(e.value) == "TGX_INVALID_ARGUMENT: " + today
    opted = S.DataTypeConstraint("name", DV.String(validation)).string_functions_on_device(True)
    plan = S.constraint_plan(opted.spec)
    assert plan["name"] == "datatype" and len(plan["requests"]) == 1
    request = plan["requests"][0]
    assert request["kind"] == T.ROW_PREDICATE and request["column"] == "name" and request["row_predicate"]["columns"] == ["name"]
    rows = [{"name": v} for v in (None, b"", b" ", b"  ", b"abc", b"abcdef", "日本".encode(), None)]
    for row in rows:
        assert xs.run_compiled(request["row_predicate"], row, {"name": "str"}) == xs.walk(tree, row, {"name": "str"})
    # considered: the non-NULL rows; valid: the satisfied rows
    seen, satisfied, unknown, _ = xs.counts(tree, rows, {"name": "str"})
    considered = 6
    v = S.constraint_verdict(opted.spec, [{"total": seen, "matches": satisfied, "non_null": seen - unknown}])
    rate = satisfied / considered
    assert v["metric"] == rate and v["status"] == ("success" if rate >= 1.0 else "failure")
    assert v["message"] == "%.1f%% of values satisfy %s" % (rate * 100.0, description)
    v = S.constraint_verdict(opted.spec, [{"total": 3, "matches": 0, "non_null": 0}])  # every row NULL: 0 / 0
    assert (v["status"], v["metric"], v["message"]) == ("failure", None, "NaN% of values satisfy " + description)
    v = S.constraint_verdict(opted.spec, [{"total": 3, "matches": 3, "non_null": 3}])
    assert (v["status"], v["metric"], v["message"]) == ("success", 1.0, "100.0% of values satisfy " + description)
    for declared in ("Utf8", "LargeUtf8", "Utf8View", "Dictionary(Int32, Utf8)"):
        assert S.constraint_verdict(dict(opted.spec, column_types=[declared]), [{"total": 3, "matches": 3, "non_null": 3}])["status"] == "success"
    for declared in ("Int64", "Binary", "Date32"):
        with pytest.raises(T.TgxError, match="'datatype': %s validation reads a string column: column 'name' is declared %s"
                                             % (description, declared)):
            S.constraint_verdict(dict(opted.spec, column_types=[declared]), [{"total": 3, "matches": 3, "non_null": 3}])


def test_the_other_validations_of_datatype_answer_as_before_with_the_opt_in():
    cases = [DV.Numeric(S.NumericValidation.Finite), DV.Temporal(S.TemporalValidation.PastDate), DV.Custom("x > 0"),
             DV.Temporal(S.TemporalValidation.DateRange("2024-01-01", "2024-12-31"))]
    for validation in cases:
        errors = []
        for opt in (False, True):
            c = S.DataTypeConstraint("x", validation)
            if opt:
                c.string_functions_on_device(True)
            with pytest.raises(T.TgxError) as e:
                S.constraint_plan(c.spec)
            errors.append(str(e.value))
        assert errors[0] == errors[1] and "not on the GPU path" in errors[0]
    numeric = S.DataTypeConstraint.non_negative("x")
    assert S.constraint_plan(numeric.spec) == S.constraint_plan(numeric.string_functions_on_device(True).spec)


def test_the_golden_fixtures_counts_are_the_exact_references():
    """tests/golden/string_predicate_vectors.json is counted by hand: the exact reference counts the same, and the
    verdict layer gives the fixture's status, metric and message on those counts"""
    with open(os.path.join(HERE, "golden", "string_predicate_vectors.json")) as f:
        g = json.load(f)
    names = list(g["table"])
    rows = ex.table_rows({c: [None if v is None else v.encode("utf-8") for v in g["table"][c]] for c in names})
    types = {c: "str" for c in names}
    for case in g["custom_sql"]:
        assert case["ref"]
        compiled = S.row_predicate(case["expression"], string_functions=True)
        satisfied = sum(xs.run_compiled(compiled, row, types) is True for row in rows)
        assert (satisfied, len(rows)) == (case["satisfied"], case["total"]), case["expression"]
        spec_ = {"type": "custom_sql", "expression": case["expression"], "string_functions_on_device": True}
        if case["hint"] is not None:
            spec_["hint"] = case["hint"]
        v = S.constraint_verdict(spec_, [{"total": len(rows), "matches": satisfied, "non_null": len(rows)}])
        assert (v["status"], v["metric"], v["message"]) == (case["status"], case["metric"], case["message"])
    c = g["compliance"]
    compiled = S.row_predicate(c["predicate"], string_functions=True)
    assert sum(xs.run_compiled(compiled, row, types) is True for row in rows) == c["compliant_count"]
    assert len(rows) == c["total_count"] and c["metric"] == c["compliant_count"] / c["total_count"]
    for case in g["datatype"]:
        v = SV.MaxBytes(case["max_bytes"]) if case["string"] == "max_bytes" else {"string": case["string"]}
        d = S.DataTypeConstraint("name", DV.String(v)).string_functions_on_device(True)
        compiled = S.constraint_plan(d.spec)["requests"][0]["row_predicate"]
        answers = [xs.run_compiled(compiled, row, types) for row in rows]
        considered = sum(row["name"] is not None for row in rows)
        assert (answers.count(True), considered) == (case["valid"], case["considered"]), case["string"]
        out = S.constraint_verdict(d.spec, [{"total": len(rows), "matches": answers.count(True),
                                             "non_null": len(rows) - answers.count(None)}])
        assert (out["status"], out["metric"], out["message"]) == (case["status"], case["metric"], case["message"])
