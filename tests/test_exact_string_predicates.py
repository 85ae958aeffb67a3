"""tests/exact_string_predicates.py held to independent references on valid UTF-8: pyarrow's match_like (backslash-free
patterns), utf8_length, binary_length, utf8_trim, and Python's own order of bytes.  No device, no library."""
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import exact_row_predicate as ex
import exact_string_predicates as xs

VALUES = xs.seeded_values()
PATTERNS = xs.seeded_patterns()
TEXTS = pa.array([v.decode("utf-8") for v in VALUES], type=pa.string())


@pytest.fixture(scope="module")
def like_table():
    """the exact reference on the seeded set, once: like_table[p][v]"""
    return [[xs.like(v, p) for v in VALUES] for p in PATTERNS]


def test_the_seeded_set_is_a_census_of_both_answers(like_table):
    assert len(PATTERNS) == 200 and len(VALUES) == 2000
    assert all(0x5C not in p for p in PATTERNS)
    total = len(PATTERNS) * len(VALUES)
    true = sum(sum(row) for row in like_table)
    assert true >= 0.2 * total and total - true >= 0.2 * total, (true, total)
    # multi-byte characters, blanks and line feeds all occur, in patterns and in values
    for needle in ("é".encode(), "日".encode(), b" ", b"\n"):
        assert any(needle in p for p in PATTERNS) and any(needle in v for v in VALUES)
    assert any(b"_" in p for p in PATTERNS) and any(b"%" in p for p in PATTERNS) and b"" in VALUES


def test_like_agrees_with_arrow_on_the_seeded_set(like_table):
    for p, row in zip(PATTERNS, like_table):
        got = pc.match_like(TEXTS, p.decode("utf-8")).to_pylist()
        assert got == row, p


@pytest.mark.parametrize("pattern, value, want", [
    ("", "", True), ("", "a", False), ("%", "", True), ("%", "a\nb", True), ("%%", "", True), ("_", "", False),
    ("_", "a", True), ("_", "é", True), ("_", "日", True), ("_", "ab", False), ("__", "é", False), ("_", "\n", True),
    ("x_y", "x\ny", True), ("a", "a", True), ("a", "A", False), ("a%", "a", True), ("a%", "ba", False), ("%a", "ba", True),
    ("%a%", "bab", True), ("a%b", "ab", True), ("a%b", "a\n\nb", True), ("a%b", "aba", False), ("a_c", "abc", True),
    ("a_c", "a日c", True), ("a_c", "ac", False), ("_%", "", False), ("_%", "é", True), ("%_", "日", True), ("__%", "é", False),
    ("__%", "é日", True), ("%aa%aa%", "aaa", False), ("%aa%aa%", "aaaa", True), ("a%ab", "aaab", True),
    ("%日_語%", "日本語", True), ("%日_語%", "日語", False), ("%日_語%", "x日本語y", True), ("%日_語%", "日本本語", False),
])
def test_like_by_hand_and_by_arrow(pattern, value, want):
    assert xs.like(value.encode(), pattern.encode()) is want
    assert pc.match_like(pa.array([value]), pattern).to_pylist() == [want]


def test_units_on_bytes_that_are_no_utf8():
    # a lone continuation byte at offset 0 opens a unit; behind a unit's first byte it belongs to that unit
    assert xs.like(b"\x80", b"_") and xs.like(b"\x80\x80", b"_") and not xs.like(b"\x80a", b"_")
    assert xs.like(b"\x80a", b"__") and xs.like(b"a\x80\x80", b"_") and not xs.like(b"a\x80", b"__")
    # a truncated sequence is a unit of its own; % may end inside a unit, _ may not begin there
    assert xs.like(b"\xe6\x97a", b"__") and xs.like(b"\xe6\x97", b"%\x97") and not xs.like(b"\xe6\x97", b"%\xe6_")
    assert xs.like(b"\xe6\x97", b"\xe6%") and xs.like(b"\xe6\x97\xa5", b"\xe6%\xa5") and not xs.like(b"a\x80", b"a_")
    assert xs.characters(b"\x80\x80a\xc3") == 2 and xs.characters(b"") == 0


def test_lengths_and_blank_agree_with_arrow():
    assert [xs.characters(v) for v in VALUES] == pc.utf8_length(TEXTS).to_pylist()
    assert [len(v) for v in VALUES] == pc.binary_length(TEXTS).to_pylist()
    trimmed = pc.equal(pc.utf8_trim(TEXTS, characters=" "), "").to_pylist()
    assert [xs.blank(v) for v in VALUES] == trimmed
    assert xs.blank(b"") and xs.blank(b"   ") and not xs.blank(b" \t") and not xs.blank(b"\n") and not xs.blank(" ".encode())
    assert sum(trimmed) >= 20 and sum(trimmed) < len(VALUES)


def test_order_is_pythons_and_arrows():
    literals = [b"", b"a", b"ab", "é".encode(), "日".encode(), b"b", b" ", b"a\n"]
    types = {"s": "str"}
    for lit in literals:
        for op, fn in (("<", pc.less), ("<=", pc.less_equal), (">", pc.greater), (">=", pc.greater_equal)):
            mine = [xs.leaf(("strcmp", "s", op, lit), {"s": v}, types) for v in VALUES]
            assert mine == fn(TEXTS, pa.scalar(lit.decode("utf-8"))).to_pylist(), (op, lit)
    # the first differing byte decides as UNSIGNED, and a proper prefix is smaller
    w = lambda v, op, lit: xs.leaf(("strcmp", "s", op, lit), {"s": v}, types)  # noqa: E731
    assert w(b"\x7f", "<", b"\x80") and w(b"\xff", ">", b"\x00\xff") and w(b"ab", "<", b"abc") and w(b"", "<", b"\x00")
    assert w(b"abc", "<=", b"abc") and w(b"abc", ">=", b"abc") and not w(b"abc", "<", b"abc") and w(None, "<", b"a") is None


def test_null_rows_kleene_and_sqls_definitions():
    types = {"s": "str", "n": "int"}
    row, null = {"s": "éa ".encode(), "n": 3}, {"s": None, "n": None}
    for tree in (("strcmp", "s", "<", b"x"), ("strlen", "s", "=", 3, False), ("like", "s", b"%"), ("blank", "s")):
        assert xs.walk(tree, null, types) is None and xs.walk(("not", tree), null, types) is None
        assert xs.walk(("or", tree, ("isnull", "s")), null, types) is True
    assert xs.walk(("strlen", "s", "=", 3, False), row, types) and xs.walk(("strlen", "s", "=", 4, True), row, types)
    assert xs.walk(xs.len_between("s", 3, 3), row, types) and not xs.walk(xs.len_between("s", 4, 9), row, types)
    assert xs.walk(xs.str_between("s", b"a", "ê".encode()), row, types) and not xs.walk(xs.str_between("s", b"a", b"z"), row, types)
    assert xs.walk(("and", ("like", "s", "é%".encode()), ("cmp", "n", ">", 2)), row, types) is True
    with pytest.raises(TypeError):
        xs.walk(("like", "n", b"%"), row, types)


def test_the_trees_lowering_keeps_the_pool_in_leaf_order():
    tree = ("and", ("or", ("like", "s", b"a%"), ("streq", "s", b"xy")), ("and", ("strcmp", "s", "<", b"q"), ("cmp", "n", ">=", 1)))
    leaves, program, pool = xs.leaves_and_program(tree, ["s", "n"])
    assert pool == b"a%xyq" and [lf["kind"] for lf in leaves] == [xs.STR_LIKE, ex.STR_EQ, xs.STR_CMP, ex.CMP_LITERAL]
    assert [(lf.get("lit_offset", 0), lf.get("lit_len", 0)) for lf in leaves] == [(0, 2), (2, 2), (4, 1), (0, 0)]
    compiled = {"columns": ["s", "n"], "leaves": [dict(dict(kind=0, op=0, col=0, col2=0, flags=0, lit_offset=0, lit_len=0, lit_i=0,
                                                            lit_f_bits=0), **lf) for lf in leaves],
                "program": [list(p) for p in program], "literals_hex": pool.hex()}
    types = {"s": "str", "n": "int"}
    for s in (b"abc", b"xy", b"zz", None):
        for n in (0, 5, None):
            row = {"s": s, "n": n}
            assert xs.run_compiled(compiled, row, types) == xs.walk(tree, row, types)
