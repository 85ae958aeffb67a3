"""TGX_CHECK_ROW_PREDICATE, Check::satisfies and ComplianceAnalyzer without a device: the constants and symbols, every
refusal of the setter and of the predicate compiler, host-only states from term_amd/wire.py blobs, the compiler's output
held to hand-written trees on an exhaustive table (tests/exact_row_predicate.py), and the constructors, verdicts and
messages of the constraint and the analyzer against tests/golden/custom_sql_vectors.json -- through the C++ host ABI
and through the Python twins."""
import json
import os

import pytest

import exact_row_predicate as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from term_amd import wire

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "custom_sql_vectors.json")
with open(GOLDEN) as _f:
    G = json.load(_f)

GE3 = [dict(kind=T.PRED_CMP_LITERAL, op=T.PRED_GE, col=0, lit_i=3, lit_f=3.0)]
PUSH0 = [(T.PRED_PUSH, 0)]


def one_spec_plan(n_columns=1):
    return T.Plan([spec(T.ROW_PREDICATE, 0, columns=list(range(n_columns))), spec(T.COUNT, 0)])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_abi_constants_and_symbols():
    assert T.ROW_PREDICATE == 20 and T.lib().tgx_abi_version() == 6
    assert (T.PRED_IS_NULL, T.PRED_CMP_LITERAL, T.PRED_CMP_COLUMNS, T.PRED_STR_EQ) == \
        (ex.IS_NULL, ex.CMP_LITERAL, ex.CMP_COLUMNS, ex.STR_EQ) == (1, 2, 3, 4)
    assert (T.PRED_EQ, T.PRED_LT, T.PRED_LE, T.PRED_GT, T.PRED_GE) == (ex.EQ, ex.LT, ex.LE, ex.GT, ex.GE) == (1, 2, 3, 4, 5)
    assert (T.PRED_PUSH, T.PRED_AND, T.PRED_OR, T.PRED_NOT) == (ex.PUSH, ex.AND, ex.OR, ex.NOT) == (1, 2, 3, 4)
    assert T.PRED_LITERAL_IS_DOUBLE == ex.LITERAL_IS_DOUBLE == 1
    assert (T.PRED_MAX_COLUMNS, T.PRED_MAX_LEAVES, T.PRED_MAX_OPS, T.PRED_MAX_DEPTH, T.PRED_MAX_LITERAL_BYTES) == (8, 32, 64, 32, 256)
    for name in ("tgx_plan_set_row_predicate", "tgx_row_predicate_get", "tgx_host_row_predicate_json"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "..", "include", "tgx.h")) as f:
        header = f.read()
    assert "TGX_CHECK_ROW_PREDICATE = 20" in header and '"row_predicate"' in header


def test_column_lists_at_plan_creation():
    one_spec_plan(1), one_spec_plan(8)
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*column list of 1..8"):
        one_spec_plan(9)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*column list of 1..8"):
        T.Plan([spec(T.ROW_PREDICATE, 0)])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*column2 must be -1"):
        T.Plan([spec(T.ROW_PREDICATE, 0, column2=1, columns=[0])])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*negative column index"):
        T.Plan([spec(T.ROW_PREDICATE, 0, columns=[0, -1])])
    for kind in (T.VALUE_RULE, T.COUNT, T.NUMERIC_STATS, T.VALUE_COUNTS):  # the other kinds go on refusing lists
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*takes a column list"):
            T.Plan([spec(kind, 0, columns=[0, 1])])


def test_every_refusal_of_the_setter():
    plan = one_spec_plan(2)
    lit = dict(kind=T.PRED_CMP_LITERAL, op=T.PRED_EQ, col=0)
    bad = [
        (dict(leaves=[], program=PUSH0), "1..32 leaves"),
        (dict(leaves=GE3 * 33, program=PUSH0, n_leaves=33), "1..32 leaves"),
        (dict(leaves=GE3, program=[]), "1..64 ops"),
        (dict(leaves=GE3, program=PUSH0 * 64, n_ops=65), "1..64 ops"),
        (dict(leaves=GE3, program=PUSH0, n_literal_bytes=257), "up to 256 literal bytes"),
        (dict(leaves=[dict(kind=0, col=0)], program=PUSH0), "unknown leaf kind 0"),
        (dict(leaves=[dict(kind=5, col=0)], program=PUSH0), "unknown leaf kind 5"),
        (dict(leaves=[dict(lit, op=0)], program=PUSH0), "unknown comparison 0"),
        (dict(leaves=[dict(lit, op=6)], program=PUSH0), "unknown comparison 6"),
        (dict(leaves=[dict(lit, flags=2)], program=PUSH0), "unknown flags 0x2"),
        (dict(leaves=[dict(lit, col=2)], program=PUSH0), "names column slot 2 of a list of 2"),
        (dict(leaves=[dict(lit, col=-1)], program=PUSH0), "names column slot -1"),
        (dict(leaves=[dict(kind=T.PRED_CMP_COLUMNS, op=1, col=0, col2=2)], program=PUSH0), "names column slot 2 of a list of 2"),
        (dict(leaves=[dict(kind=T.PRED_STR_EQ, col=0, lit_offset=2, lit_len=3)], program=PUSH0, literals=b"abcd"),
         r"names literal bytes \[2, 2 \+ 3\) of a pool of 4"),
        (dict(leaves=[dict(kind=T.PRED_STR_EQ, col=0, lit_offset=5, lit_len=0)], program=PUSH0, literals=b"abcd"),
         "names literal bytes"),
        (dict(leaves=GE3, program=[(T.PRED_PUSH, 1)]), "op 0 pushes leaf 1 of 1"),
        (dict(leaves=GE3, program=[(T.PRED_NOT, 0)]), "op 0: the program underflows its stack"),
        (dict(leaves=GE3, program=PUSH0 + [(T.PRED_AND, 0)]), "op 1: the program underflows its stack"),
        (dict(leaves=GE3, program=PUSH0 + [(T.PRED_OR, 0)]), "op 1: the program underflows its stack"),
        (dict(leaves=GE3, program=PUSH0 * 2), "the program leaves 2 values, not one"),
        (dict(leaves=GE3, program=PUSH0 * 33 + [(T.PRED_AND, 0)] * 31), "op 32: the program exceeds depth 32"),
        (dict(leaves=GE3, program=[(0, 0)]), "unknown op code 0"),
        (dict(leaves=GE3, program=[(5, 0)]), "unknown op code 5"),
        (dict(leaves=GE3, program=PUSH0 + [(T.PRED_NOT, 1)]), "only PUSH takes an argument"),
    ]
    for args, message in bad:
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*" + message):
            plan.set_row_predicate(0, **args)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a ROW_PREDICATE check"):
        plan.set_row_predicate(1, GE3, PUSH0)
    # what is allowed: depth 32 exactly, 64 ops, a pool of 256 bytes, the empty literal at the pool's end
    plan.set_row_predicate(0, GE3, PUSH0 * 32 + [(T.PRED_OR, 0)] * 31)
    plan.set_row_predicate(0, GE3, PUSH0 + [(T.PRED_NOT, 0)] * 63)
    plan.set_row_predicate(0, [dict(kind=T.PRED_STR_EQ, col=1, lit_offset=256, lit_len=0)], PUSH0, bytes(256))


def test_a_spec_without_its_predicate_fails_state_create_and_deserialize():
    plan = T.Plan([spec(T.ROW_PREDICATE, 0, columns=[0]), spec(T.ROW_PREDICATE, 0, columns=[0])])
    plan.set_row_predicate(0, GE3, PUSH0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1.*tgx_plan_set_row_predicate"):
        T.State(plan)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*tgx_plan_set_row_predicate"):
        T.State.deserialize(plan, wire.pack(row_predicates=[wire.row_predicate_state(GE3, PUSH0, b"", 3, 2, 1)] * 2))


def pred_plan(lit=3):
    plan = T.Plan([spec(T.ROW_PREDICATE, 0, columns=[0]), spec(T.ROW_PREDICATE, 0, columns=[1, 0]), spec(T.COUNT, 0)])
    plan.set_row_predicate(0, [dict(GE3[0], lit_i=lit, lit_f=float(lit))], PUSH0)
    plan.set_row_predicate(1, STR_LEAVES, STR_PROGRAM, b"FO")
    return plan


STR_LEAVES = [dict(kind=T.PRED_STR_EQ, col=0, lit_offset=0, lit_len=1), dict(kind=T.PRED_STR_EQ, col=0, lit_offset=1, lit_len=1),
              dict(kind=T.PRED_IS_NULL, col=1)]
STR_PROGRAM = [(T.PRED_PUSH, 0), (T.PRED_PUSH, 1), (T.PRED_OR, 0), (T.PRED_PUSH, 2), (T.PRED_NOT, 0), (T.PRED_AND, 0)]


def pred_blob(lit=3, program=STR_PROGRAM, pool=b"FO", counts=((10, 5, 2), (10, 4, 0))):
    return wire.pack(count=[wire.count_acc(10, 9)], row_predicates=[
        wire.row_predicate_state([dict(GE3[0], lit_i=lit, lit_f=float(lit))], PUSH0, b"", *counts[0]),
        wire.row_predicate_state(STR_LEAVES, program, pool, *counts[1])])


def test_the_setter_is_refused_after_the_first_state():
    plan = pred_plan()
    st = T.State.deserialize(plan, pred_blob())
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*fixed once a state"):
        plan.set_row_predicate(0, GE3, PUSH0)
    del st


def test_a_host_only_state_answers_from_a_blob_merges_and_round_trips():
    plan = pred_plan()
    blob = pred_blob()
    st = T.State.deserialize(plan, blob)
    assert [st.row_predicate_counts(i) for i in range(2)] == [(10, 5, 2, 3), (10, 4, 0, 6)]
    res = st.finalize()
    assert [(r.total, r.matches, r.non_null) for r in res[:2]] == [(10, 5, 8), (10, 4, 10)]
    assert st.serialize() == blob
    st.merge([T.State.deserialize(plan, blob), T.State.deserialize(plan, blob)])
    assert [st.row_predicate_counts(i) for i in range(2)] == [(30, 15, 6, 9), (30, 12, 0, 18)]
    st.reset()
    assert [st.row_predicate_counts(i) for i in range(2)] == [(0, 0, 0, 0)] * 2
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*not a ROW_PREDICATE check"):
        st.row_predicate_counts(2)


def test_blobs_counted_under_another_predicate_and_malformed_blobs_are_refused():
    plan = pred_plan()
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*task 0.*other leaves"):  # another literal
        T.State.deserialize(plan, pred_blob(lit=4))
    swapped = [STR_PROGRAM[1], STR_PROGRAM[0]] + STR_PROGRAM[2:]
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*task 1.*another program"):
        T.State.deserialize(plan, pred_blob(program=swapped))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*task 1.*other literal bytes"):
        T.State.deserialize(plan, pred_blob(pool=b"FP"))
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*task 1.*another predicate"):
        T.State.deserialize(plan, pred_blob(program=STR_PROGRAM + [(T.PRED_NOT, 0)]))
    for counts in (((10, 11, 0), (10, 4, 0)), ((10, 5, 6), (10, 4, 0))):  # satisfied + unknown above seen
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*malformed"):
            T.State.deserialize(plan, pred_blob(counts=counts))
    blob = pred_blob()
    for cut in (1, 8, 24, 60):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            T.State.deserialize(plan, blob[:-cut])
    other = T.Plan([spec(T.ROW_PREDICATE, 0, columns=[0]), spec(T.COUNT, 0)])  # a plan whose section has other tasks
    other.set_row_predicate(0, GE3, PUSH0)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
        T.State.deserialize(other, blob)


def test_blobs_of_plans_without_the_kind_keep_their_bytes():
    plan = T.Plan([spec(T.COUNT, 0), spec(T.VALUE_RULE, 0)])
    plan.set_value_rule(1, T.RULE_GE_ZERO)
    blob = wire.pack(count=[wire.count_acc(10, 9)], value_rules=[wire.value_rule_state(1, 0, 10, 9, 7)])
    assert T.State.deserialize(plan, blob).serialize() == blob


# ---- the compiler ---------------------------------------------------------------------------------------------------------
# the exhaustive table: 3 columns x {NULL, 3 values}
VALUES = {"a": [None, 0, 1, 5], "x": [None, -0.0, 0.5, 10.0], "s": [None, b"", b"F", b"it's"]}
TYPES = {"a": "int", "x": "float", "s": "str"}
ROWS = [{"a": a, "x": x, "s": s} for a in VALUES["a"] for x in VALUES["x"] for s in VALUES["s"]]

A1, A5, X0, SF = ("cmp", "a", "=", 1), ("cmp", "a", "=", 5), ("cmp", "x", ">", 0.0), ("streq", "s", b"F")
# (expression, hand-written tree, {name in the expression: column of the table})
EXPRESSIONS = [
    ("a = 1", A1, {}),
    ("a <> 1", ("not", A1), {}),
    ("a != 1", ("not", A1), {}),
    ("a < 1", ("cmp", "a", "<", 1), {}),
    ("a <= 1", ("cmp", "a", "<=", 1), {}),
    ("a > 1", ("cmp", "a", ">", 1), {}),
    ("a >= 1", ("cmp", "a", ">=", 1), {}),
    ("1 < a", ("cmp", "a", ">", 1), {}),                                  # lit op col is turned round
    ("1 >= a", ("cmp", "a", "<=", 1), {}),
    ("0.5 = x", ("cmp", "x", "=", 0.5), {}),
    ("1 <> a", ("not", A1), {}),
    ("a = 1.0", ("cmp", "a", "=", 1.0), {}),                              # a float token is a double literal
    ("a < 5e-1", ("cmp", "a", "<", 0.5), {}),
    ("x >= 0", ("cmp", "x", ">=", 0), {}),                                # -0.0 is below the integer literal 0
    ("x = -0.0", ("cmp", "x", "=", -0.0), {}),
    ("x > -1", ("cmp", "x", ">", -1), {}),                                # a leading - belongs to the literal
    ("a IS NULL", ("isnull", "a"), {}),
    ("s IS NOT NULL", ("not", ("isnull", "s")), {}),
    ("a BETWEEN 1 AND 5", ex.between("a", 1, 5), {}),
    ("a NOT BETWEEN 1 AND 5", ("not", ex.between("a", 1, 5)), {}),
    ("a BETWEEN 5 AND 1", ex.between("a", 5, 1), {}),                     # lo > hi matches nothing
    ("a NOT BETWEEN 5 AND 1", ("not", ex.between("a", 5, 1)), {}),
    ("x BETWEEN 0.0 AND 0.10", ex.between("x", 0.0, 0.10), {}),
    ("a BETWEEN 0 AND 1.5", ex.between("a", 0, 1.5), {}),
    ("a IN (1)", ex.isin("a", [1]), {}),
    ("a IN (1, 5, 7)", ex.isin("a", [1, 5, 7]), {}),
    ("a NOT IN (1, 5)", ("not", ex.isin("a", [1, 5])), {}),               # UNKNOWN on a NULL
    ("s IN ('F', 'O', 'P')", ex.isin("s", [b"F", b"O", b"P"]), {}),
    ("s NOT IN ('F', '')", ("not", ex.isin("s", [b"F", b""])), {}),
    ("x IN (0.5, -0.0, 3)", ex.isin("x", [0.5, -0.0, 3]), {}),
    ("s = 'F'", SF, {}),
    ("s <> 'F'", ("not", SF), {}),
    ("'F' = s", SF, {}),
    ("s = ''", ("streq", "s", b""), {}),
    ("s = 'it''s'", ("streq", "s", b"it's"), {}),                         # '' is a quote
    ("a = x", ("cmpcol", "a", "=", "x"), {}),
    ("a <= x", ("cmpcol", "a", "<=", "x"), {}),
    ("x <> a", ("not", ("cmpcol", "x", "=", "a")), {}),
    ("s = s", ("cmpcol", "s", "=", "s"), {}),
    ("a < a", ("cmpcol", "a", "<", "a"), {}),
    ("a = 1 AND x > 0.0", ("and", A1, X0), {}),
    ("a = 1 OR x > 0.0", ("or", A1, X0), {}),
    ("NOT a = 1", ("not", A1), {}),
    ("NOT NOT a = 1", ("not", ("not", A1)), {}),
    ("a = 1 OR x > 0.0 AND NOT s = 'F'", ("or", A1, ("and", X0, ("not", SF))), {}),       # NOT over AND over OR
    ("(a = 1 OR x > 0.0) AND NOT s = 'F'", ("and", ("or", A1, X0), ("not", SF)), {}),
    ("NOT (a = 1 OR x > 0.0) AND s = 'F'", ("and", ("not", ("or", A1, X0)), SF), {}),
    ("a = 1 AND a = 5 OR a = 1 AND x > 0.0", ("or", ("and", A1, A5), ("and", A1, X0)), {}),
    ("a = 1 OR a = 5 OR x > 0.0", ("or", ("or", A1, A5), X0), {}),                           # left to right
    ("((a = 1))", A1, {}),
    ("a = 1 and X > 0.0 Or not S is Null", ("or", ("and", A1, X0), ("not", ("isnull", "s"))), {}),  # keywords, identifiers
    ("A = 1", A1, {}),                                                                        # unquoted: lowercased
    ('"Mixed Case" = 1 AND "a" = 5', ("and", ("cmp", "Mixed Case", "=", 1), A5), {"Mixed Case": "x2"}),
    ('"say ""hi""" IS NULL', ("isnull", 'say "hi"'), {'say "hi"': "x2"}),
    ("date >= 5 AND time < 3", ("and", ("cmp", "date", ">=", 5), ("cmp", "time", "<", 3)), {"date": "a", "time": "x2"}),
    ("status = 'active' AND price >= 10", ("and", ("streq", "status", b"active"), ("cmp", "price", ">=", 10)),
     {"status": "s", "price": "x"}),
    ("l_discount >= 0.0 AND l_discount <= 0.10", ex.between("l_discount", 0.0, 0.10), {"l_discount": "x"}),
    ("order_date <= ship_date", ("cmpcol", "order_date", "<=", "ship_date"), {"order_date": "a", "ship_date": "x2"}),
]


def renamed(tree, names):
    if tree[0] in ("and", "or"):
        return (tree[0], renamed(tree[1], names), renamed(tree[2], names))
    if tree[0] == "not":
        return ("not", renamed(tree[1], names))
    if tree[0] == "cmpcol":
        return ("cmpcol", names.get(tree[1], tree[1]), tree[2], names.get(tree[3], tree[3]))
    return (tree[0], names.get(tree[1], tree[1])) + tuple(tree[2:])


def test_there_are_at_least_40_expressions():
    assert len(EXPRESSIONS) >= 40 and len(set(e for e, _, _ in EXPRESSIONS)) == len(EXPRESSIONS)


@pytest.mark.parametrize("expression,tree,names", EXPRESSIONS, ids=[e for e, _, _ in EXPRESSIONS])
def test_the_compiled_program_equals_the_tree_on_the_exhaustive_table(expression, tree, names):
    compiled = S.row_predicate(expression)
    assert 1 <= len(compiled["columns"]) <= 8 and 1 <= len(compiled["leaves"]) <= 32 and 1 <= len(compiled["program"]) <= 64
    # "x2": a second integer column for the expressions that name more than the table's three
    rows = [dict(r, x2=v) for r in ROWS for v in ((None, 0, 3) if "x2" in names.values() else (0,))]
    types = dict(TYPES, x2="int")
    compiled["columns"] = [names.get(c, c) for c in compiled["columns"]]
    tree = renamed(tree, names)
    for row in rows:
        assert ex.run_compiled(compiled, row, types) == ex.walk(tree, row, types), row
    # and the C ABI takes what the compiler made
    plan = T.Plan([spec(T.ROW_PREDICATE, 0, columns=list(range(len(compiled["columns"]))))])
    leaves = [{k: v for k, v in leaf.items() if k != "lit_f_bits"} for leaf in compiled["leaves"]]
    for leaf, full in zip(leaves, compiled["leaves"]):
        leaf["lit_f"] = ex.from_bits(full["lit_f_bits"])
    plan.set_row_predicate(0, leaves, [tuple(p) for p in compiled["program"]], bytes.fromhex(compiled["literals_hex"]))


def test_columns_come_in_order_of_first_appearance_and_literals_in_a_pool():
    c = S.row_predicate("b = 'xy' AND (a > 1 OR b = '') AND c IS NULL AND a < 2.5")
    assert c["columns"] == ["b", "a", "c"] and c["literals_hex"] == b"xy".hex()
    assert [(l["kind"], l["col"]) for l in c["leaves"]] == [(4, 0), (2, 1), (4, 0), (1, 2), (2, 1)]
    assert [l["flags"] for l in c["leaves"]] == [0, 0, 0, 0, 1] and c["leaves"][2]["lit_len"] == 0
    assert c["leaves"][1]["lit_i"] == 1 and c["leaves"][1]["lit_f"] == 1.0 and c["leaves"][4]["lit_f"] == 2.5
    assert S.row_predicate("a = -9223372036854775808")["leaves"][0]["lit_i"] == -(1 << 63)
    assert S.row_predicate("a = 9223372036854775807")["leaves"][0]["lit_i"] == (1 << 63) - 1


REFUSED = [
    ("a + 1 > 2", r"arithmetic \('\+'\)"), ("a - 1 > 2", r"arithmetic \('-'\)"), ("a * 2 = 4", "arithmetic"),
    ("a / 2 = 4", "arithmetic"), ("a % 2 = 0", "arithmetic"), ("a = -b", "arithmetic"), ("s || 'x' = 'y'", "arithmetic"),
    ("LENGTH(s) > 3", r"a function call \(LENGTH\(\.\.\)\)"), ("ABS(a) = 1", r"a function call \(ABS"),
    ("x < now()", r"a function call \(now"), ("s LIKE 'F%'", "LIKE"), ("s NOT LIKE 'F%'", "LIKE"), ("s ILIKE 'f'", "ILIKE"),
    ("CASE WHEN a = 1 THEN 1 END = 1", "CASE"), ("CAST(a AS INT) = 1", "a function call|CAST"), ("a::int = 1", r"a cast \(::\)"),
    ("a = TRUE", "TRUE"), ("FALSE", "FALSE"), ("a = NULL", "a NULL literal"), ("s < 'F'", "a string order comparison"),
    ("s >= 'F'", "a string order comparison"), ("'F' < s", "a string order comparison"),
    ("s BETWEEN 'A' AND 'Z'", "a string order comparison"), ("1 = 1", "a comparison of two literals"),
    ("'a' = 'a'", "a comparison of two literals"), ("1 IS NULL", "IS .NOT. NULL of a literal"), ("1 IN (1, 2)", "IN of a literal"),
    ("a IN (1, 'F')", "an IN list that mixes strings and numbers"), ("a IN ('F', 2.5)", "an IN list that mixes strings and numbers"),
    ("a IN (b)", "a column where a literal should stand"), ("a BETWEEN b AND 2", "a column where a literal should stand"),
    ("a IN ()", "where a column or a literal should stand"), ("a IN (SELECT 1)", "a subquery"), ("t.a = 1", r"a qualified identifier \(t\.\)"),
    ('"t"."a" = 1', "a qualified identifier"), ("a = 9223372036854775808", "an integer literal outside int64"),
    ("a = -9223372036854775809", "an integer literal outside int64"), ("a = 1e999", "a float literal that is not finite"),
    ("a = 12abc", "a malformed number"), ("a", "where a comparison should stand"), ("a =", "the end of the expression where a column"),
    ("", "the end of the expression where a column"), ("(a = 1", r"where '\)' should stand"), ("a = 1)", r"'\)' after the end"),
    ("a = 1 b = 2", "'b' after the end of the predicate"), ("a = 'unterminated", "an unterminated string literal"),
    ('"unterminated = 1', "an unterminated quoted identifier"), ('"" = 1', "an empty quoted identifier"),
    ("a IS TRUE", "only IS .NOT. NULL"), ("a NOT = 1", "only NOT BETWEEN and NOT IN"), ("(a) = 1", "where a comparison should stand"),
    ("(a = 1) = (x > 0.0)", "a parenthesised operand"), ("a = DATE '2024-01-01'", r"a typed literal \(DATE"),
    ("AND a = 1", "'AND' where a column or a literal should stand"), ("a = 1 AND", "the end of the expression"),
    ("a = 1 OR OR x = 2", "'OR' where a column"), ("a ~ 'x'", "where a comparison should stand"), ("a == 1", "where a column or a literal"),
    (" OR ".join("c%d = 1" % i for i in range(9)), "more than 8 columns"),
    ("a IN (%s)" % ", ".join(str(i) for i in range(33)), "more than 32 leaves"),
    (" AND ".join(["NOT NOT NOT a = 1"] * 17), "more than 64 ops"),
    ("s IN ('%s', '%s')" % ("y" * 200, "z" * 57), "more than 256 literal bytes"),
    ("(" * 70 + "a = 1" + ")" * 70, "nesting deeper than 64"),
]


@pytest.mark.parametrize("expression,message", REFUSED, ids=[e[:40] for e, _ in REFUSED])
def test_what_is_outside_the_subset_is_refused_with_its_name(expression, message):
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED: the expression is not on the GPU path: .*(" + message + ")"):
        S.row_predicate(expression)


def test_the_limits_themselves_are_inside():
    assert len(S.row_predicate(" OR ".join("c%d = 1" % i for i in range(8)))["columns"]) == 8
    assert len(S.row_predicate("a IN (%s)" % ", ".join(str(i) for i in range(32)))["leaves"]) == 32
    assert len(S.row_predicate("s IN ('%s', '%s')" % ("y" * 200, "z" * 56))["literals_hex"]) == 512
    assert len(S.row_predicate("a IN (%s) AND NOT x > 1" % ", ".join(str(i) for i in range(31)))["program"]) == 64
    right = "a = 0" + "".join(" OR (a = %d" % i for i in range(1, 32)) + ")" * 31  # right-nested: depth 32
    assert len(S.row_predicate(right)["leaves"]) == 32


# ---- the constraint -------------------------------------------------------------------------------------------------------
def test_the_constructor_applies_the_references_validation_in_both_layers():
    for sql in G["custom_sql"]["accepted"]:
        assert S.CustomSqlConstraint(sql).spec == {"type": "custom_sql", "expression": sql}
        try:
            S.constraint_plan({"type": "custom_sql", "expression": sql})
        except T.TgxError as e:  # (accepted by the validation; the subset's refusal comes from plan())
            assert "not on the GPU path" in str(e)
    for sql, message in G["custom_sql"]["rejected"]:
        with pytest.raises(T.TgxError, match="Validation failed: " + message):
            S.CustomSqlConstraint(sql)
        with pytest.raises(T.TgxError, match="Validation failed: " + message):
            S.CustomSqlConstraint.try_new(sql, "a hint")
        with pytest.raises(T.TgxError, match="Validation failed: " + message):  # C++
            S.constraint_plan({"type": "custom_sql", "expression": sql})
        with pytest.raises(T.TgxError, match="Validation failed: " + message):
            S.Check.builder("c").satisfies(sql)
    # of several forbidden words the first in the list's written order is named, in both layers
    several = "x = 1 OR LOCK = 2 OR COMMIT = 3 OR EXEC = 4 OR EXECUTE = 5"
    for make in (S.CustomSqlConstraint, lambda e: S.constraint_plan({"type": "custom_sql", "expression": e})):
        with pytest.raises(T.TgxError, match="forbidden operation: EXECUTE$"):
            make(several)
    assert len(S.CustomSqlConstraint.FORBIDDEN) == 25
    for word in S.CustomSqlConstraint.FORBIDDEN:
        for make in (S.CustomSqlConstraint, lambda e: S.constraint_plan({"type": "custom_sql", "expression": e})):
            with pytest.raises(T.TgxError, match="forbidden operation: %s$" % word):
                make("a = 1 OR %s = 2" % word.lower())
            try:
                make("%s_at = 1 AND is_%sd = 2" % (word.lower(), word.lower()))  # part of a larger word
            except T.TgxError as e:
                assert "not on the GPU path" in str(e)


def test_name_plan_and_metadata():
    c = S.CustomSqlConstraint("status = 'active' AND price >= 10", "Active items must have price >= 10")
    assert c.name() == "custom_sql"
    assert c.metadata() == {"description": "Checks that all rows satisfy the SQL expression: status = 'active' AND price >= 10",
                            "expression": "status = 'active' AND price >= 10", "constraint_type": "custom",
                            "hint": "Active items must have price >= 10"}
    assert "hint" not in S.CustomSqlConstraint("a = 1").metadata()
    plan = S.constraint_plan(c.spec)
    assert plan["name"] == "custom_sql" and len(plan["requests"]) == 1
    r = plan["requests"][0]
    assert r["kind"] == T.ROW_PREDICATE and r["column"] == "status" and r["row_predicate"] == S.row_predicate(c.expression)
    # the same expression, one spec: the request's parameters are equal bytes
    again = S.constraint_plan({"type": "custom_sql", "expression": c.expression, "hint": "another hint"})
    assert again["requests"] == plan["requests"]
    with pytest.raises(T.TgxError, match="Constraint evaluation failed for 'custom_sql': the expression is not on the GPU path: "
                                         r"a function call \(LENGTH\(\.\.\)\)\. Expression: 'LENGTH\(name\) > 3'"):
        S.constraint_plan({"type": "custom_sql", "expression": "LENGTH(name) > 3"})


def test_verdicts_and_every_message_against_the_golden_vectors():
    table = ex.table_rows({c: [v.encode() if isinstance(v, str) else v for v in vals]
                           for c, vals in G["custom_sql"]["table"].items()})
    types = {"price": "float", "quantity": "int", "status": "str"}
    metrics = []
    for case in G["custom_sql"]["cases"]:
        if case["total"] is None:
            continue
        # the golden counts are what the compiled expression gives on the golden table
        compiled = S.row_predicate(case["expression"])
        satisfied = sum(ex.run_compiled(compiled, row, types) is True for row in table)
        assert (satisfied, len(table)) == (case["satisfied"], case["total"])
        spec_ = {"type": "custom_sql", "expression": case["expression"]}
        if case["hint"] is not None:
            spec_["hint"] = case["hint"]
        cxx = S.constraint_verdict(spec_, [{"total": case["total"], "matches": case["satisfied"], "non_null": case["total"]}])
        twin = S.CustomSqlConstraint(case["expression"], case["hint"]).verdict(case["satisfied"], case["total"])
        assert (cxx["status"], cxx["metric"], cxx["message"]) == twin
        assert cxx["status"] == case["status"] and cxx["metric"] == case["metric"]
        for fragment in case["message_contains"]:
            assert fragment in cxx["message"]
        metrics.append(cxx["metric"])
    assert metrics == [0.8, 1.0, 0.8, 0.6, 0.8]
    # no rows: Skipped, in both layers
    cxx = S.constraint_verdict({"type": "custom_sql", "expression": "a = 1"}, [{"total": 0, "matches": 0}])
    assert (cxx["status"], cxx["metric"], cxx["message"]) == ("skipped", None, "No data to validate") == \
        S.CustomSqlConstraint("a = 1").verdict(0, 0)
    # the two message forms, verbatim
    assert S.CustomSqlConstraint("q > 0", "Quantity must be positive").verdict(4, 5)[2] == \
        "Quantity must be positive (1 rows failed the condition)"
    assert S.CustomSqlConstraint("q > 0").verdict(2, 5)[2] == "Custom SQL condition not satisfied for 3 rows. Expression: 'q > 0'"


def test_a_literal_comparison_on_a_declared_temporal_decimal_boolean_or_binary_column_is_a_failure():
    results = [{"total": 5, "matches": 5}]
    for declared in ("Date32", "Timestamp(Nanosecond, None)", "Decimal128(10, 2)", "Boolean", "Binary", "Time64(Microsecond)"):
        v = S.constraint_verdict({"type": "custom_sql", "expression": "d >= 5 AND n = 1", "column_types": [declared, "Int64"]},
                                 results)
        assert v["status"] == "failure" and v["metric"] is None
        assert v["message"].startswith("SQL expression error: column 'd' is declared " + declared)
        assert v["message"].endswith("Expression: 'd >= 5 AND n = 1'")
    # two columns of the same declared type compare; IS NULL reads no value
    for expression in ("order_date <= ship_date", "order_date IS NOT NULL AND ship_date IS NOT NULL"):
        v = S.constraint_verdict({"type": "custom_sql", "expression": expression, "column_types": ["Date32", "Date32"]}, results)
        assert v["status"] == "success" and v["metric"] == 1.0


# ---- the analyzer ---------------------------------------------------------------------------------------------------------
def test_the_analyzers_names_state_merge_and_metric():
    g = G["compliance"]
    a = S.ComplianceAnalyzer("score_check", g["predicate"])
    assert a.name() == "compliance" and a.metric_key() == "compliance"
    assert a.planned_requests([T.FLOAT64]) == [{"kind": T.ROW_PREDICATE, "column": "score", "column2": ""}]
    states = [{"compliant_count": 3, "total_count": 4}, {"compliant_count": 4, "total_count": 6}]
    assert a.merge_states(states) == {"compliant_count": g["compliant_count"], "total_count": g["total_count"]}
    assert a.merge_states_text(states) == '{"compliant_count": 7, "total_count": 10}'  # integer tokens
    assert a.compute_metric_from_state(a.merge_states(states)) == {"type": "Double", "value": g["metric"]}
    assert a.compute_metric_from_state({"compliant_count": 0, "total_count": 0}) == {"type": "Double", "value": 1.0}
    big = [{"compliant_count": 2**63, "total_count": 2**63 + 5}] * 1 + [{"compliant_count": 1, "total_count": 1}]
    assert a.merge_states(big) == {"compliant_count": 2**63 + 1, "total_count": 2**63 + 6}


def test_validate_predicate_is_the_references_substring_test():
    for predicate, word in G["compliance"]["rejected"]:
        assert S.compliance_forbidden_keyword(predicate) == word
        with pytest.raises(T.TgxError, match="Invalid configuration: Predicate contains forbidden keyword: " +
                                             word.replace("*", r"\*")):
            S.ComplianceAnalyzer("n", predicate).planned_requests([T.INT64])
    assert S.compliance_forbidden_keyword("score >= 20 AND status = 'ok'") is None
    assert S.COMPLIANCE_FORBIDDEN == ("drop", "delete", "insert", "update", "create", "alter", "grant", "revoke", "exec",
                                      "execute", "union", "select", "--", "/*", "*/")
    with pytest.raises(T.TgxError, match=r"Invalid configuration: Invalid predicate 'ABS\(score\) > 1': not on the GPU path: "
                                         r"a function call \(ABS\(\.\.\)\)"):
        S.ComplianceAnalyzer("n", "ABS(score) > 1").planned_requests([T.FLOAT64])
