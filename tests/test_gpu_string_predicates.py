"""-m gpu: the string leaves of TGX_CHECK_ROW_PREDICATE (STR_CMP, STR_LENGTH, STR_LIKE, STR_BLANK).  The reference is
tests/exact_string_predicates.py -- plain Python over bytes, a recursive LIKE over units, neither the library nor its
compiler -- and EVERY counter (seen, satisfied, unknown, failed) is compared for equality; there are no tolerances.
The leaves and the program a tree becomes are the tests' own lowering, except where a test is about the compiler."""
import json
import os

import numpy as np
import pyarrow as pa
import pytest

import exact_row_predicate as ex
import exact_string_predicates as xs
import term_amd as T
import term_amd.suite as S
import test_gpu_row_predicate as base
from _lib_spec import spec
from term_amd import wire

pytestmark = pytest.mark.gpu

UTF8, LARGE, VIEW, DICT, STRINGS, I64, F64 = base.UTF8, base.LARGE, base.VIEW, base.DICT, base.STRINGS, base.I64, base.F64
Table, nullable = base.Table, base.nullable
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "string_predicate_vectors.json")
VALUES = xs.seeded_values()
PATTERNS = xs.seeded_patterns()

like = lambda c, p: ("like", c, p.encode() if isinstance(p, str) else p)  # noqa: E731
ln = lambda c, op, n, b=False: ("strlen", c, op, n, b)  # noqa: E731
lt = lambda c, op, lit: ("strcmp", c, op, lit.encode() if isinstance(lit, str) else lit)  # noqa: E731


def plan_of(trees, table, extra=()):
    specs, preds = [], []
    for tree in trees:
        cols = base.columns_of_tree(tree, table.names)
        specs.append(spec(T.ROW_PREDICATE, 0, columns=[table.names.index(c) for c in cols]))
        preds.append(xs.leaves_and_program(tree, cols))
    plan = T.Plan(specs + list(extra))
    for i, (leaves, program, pool) in enumerate(preds):
        plan.set_row_predicate(i, leaves, program, pool)
    return plan


def check(trees, table, mem=T.MEM_DEVICE, cuts=None, offsets=None, want=None):
    T.init()
    want = [xs.counts(t, table.rows, table.types) for t in trees] if want is None else want
    plan = plan_of(trees, table)
    st = base.feed(plan, base.batches_of(table.columns(mem, offsets), table.n, cuts))
    got = [st.row_predicate_counts(i) for i in range(len(trees))]
    assert got == want
    for r, (seen, sat, unk, failed) in zip(st.finalize(), want):
        assert (r.total, r.matches, r.non_null) == (seen, sat, seen - unk) and sat + unk + failed == seen
    return st, plan, want


def both_answers(want):
    """a case in which every row has one answer shows little: rows are satisfied and rows fail"""
    return any(w[1] > 0 for w in want) and any(w[3] > 0 for w in want)


# one tree of every kind and a few shapes, for values over the seeded alphabet
TREES = [like("s", "%a%"), like("s", "a_%"), like("s", "%日_"), ("not", like("s", "%b")), ln("s", ">=", 3), ln("s", "=", 2),
         ln("s", "<=", 4, True), lt("s", "<", "b"), lt("s", ">=", "a日"), ("blank", "s"), ("not", ("blank", "s")),
         ("and", like("s", "_%"), ("or", ln("s", "<", 3), lt("s", ">", "é"))), xs.str_between("s", b"a", b"b"), xs.len_between("s", 1, 3)]


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 2049])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    t = Table({"s": (UTF8, nullable(rng, VALUES[:n] + VALUES[:max(0, n - len(VALUES))], 0.2))})
    assert t.n == n
    _, _, want = check(TREES, t)
    assert n < 63 or both_answers(want)


@pytest.mark.parametrize("null", [0.0, 0.2, 1.0])
def test_null_rates(null):
    rng = np.random.default_rng(5)
    t = Table({"s": (UTF8, nullable(rng, VALUES[:700], null))})
    _, _, want = check(TREES, t)
    if null == 1.0:  # every leaf UNKNOWN on every row
        assert all(w == (700, 0, 700, 0) for w in want)


def straddlers():
    """lengths 0 .. 20 and 255 .. 257 in ASCII, blanks and multi-byte characters (cut to the length: the last character
    of some is truncated, and the device takes bytes), so that over the four alignments a character straddles every word
    boundary; 12 / 13 bytes: the inline boundary of a view"""
    out = []
    for n in list(range(21)) + [255, 256, 257]:
        out += [b"a" * n, b" " * n, ("é" * n).encode()[:n], ("日" * n).encode()[:n], (b"ab " * n)[:n], ("a日é " * n).encode()[:n]]
    out += [b"twelve bytes", b"thirteen byte", b"            ", b"             ", "日本語日".encode(), "日本語日a".encode(),
            b"aaa", b"aaaa", b"aaab", "日本語".encode(), "x日本語y".encode(), "日語".encode(), b"x\ny", b"abc", b"ab", b"ac", b""]
    return out


LAYOUT_TREES = TREES + [like("s", "a%a"), like("s", "%é"), like("s", "%é日%"), like("s", "____________"), like("s", "_____________%"),
                        ln("s", "=", 12), ln("s", "=", 13, True), ln("s", ">=", 255), ln("s", "<=", 256, True), lt("s", "<=", b"a" * 256),
                        lt("s", ">", "日" * 6), lt("s", "<", b"twelve bytes!"), lt("s", ">=", b"a" * 13), ("blank", "s")]


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", STRINGS, ids=str)
def test_every_layout_at_every_alignment(layout, shift):
    """`shift` rows of the 3-byte filler stand before the slice: the column's first value begins at byte 3 * shift of
    its buffer, and the values' own lengths move the rest over every alignment"""
    rng = np.random.default_rng(shift)
    values = straddlers()
    order = rng.permutation(len(values))
    t = Table({"s": (layout, nullable(rng, [values[i] for i in order], 0.1))})
    _, _, want = check(LAYOUT_TREES, t, offsets={"s": shift})
    assert both_answers(want)


def test_every_start_alignment_of_one_value():
    """the same value behind 0 .. 7 bytes of prefix rows: its first byte at every place in a word, for every kind"""
    value = "日本語 é ab".encode()
    rows = []
    for k in range(8):
        rows += [b"x" * k, value]
    t = Table({"s": (UTF8, rows)})
    trees = [like("s", "日_語%"), like("s", "%_ ab"), ln("s", "=", 8), ln("s", "=", 15, True), lt("s", "<=", value), lt("s", ">", value[:-1]),
             lt("s", "<", value[:4] + b"\xff"), ("blank", "s"), like("s", "日本語 é ab")]
    _, _, want = check(trees, t)
    assert [w[1] for w in want] == [8, 8, 8, 8, 16, 8, 16, 1, 8]


def test_values_of_4099_bytes():
    rng = np.random.default_rng(4099)
    body = bytes(rng.choice(np.frombuffer("ab é日".encode(), np.uint8), 4099).tolist())
    rows = [body, body[:4098] + b"!", b" " * 4099, b" " * 4098 + b"\t", body[1:], b"q" + body, None, body[:2048]]
    for layout in (UTF8, VIEW):
        t = Table({"s": (layout, rows)})
        trees = [ln("s", "=", xs.characters(body)), ln("s", ">=", 4099, True), lt("s", "<=", body[:200]), lt("s", ">=", body[:200]),
                 ("blank", "s"), like("s", body[:3] + b"%" + body[-3:]), like("s", b"%" + body[-4:]), like("s", b"%!"),
                 like("s", body[:100] + b"%"), like("s", b"%" + body[2000:2004] + b"%")]
        _, _, want = check(trees, t, offsets={"s": 1})
        assert both_answers(want)


def test_a_dictionary_with_a_null_entry_and_an_index_outside_it():
    T.init()
    entries = pa.array([b"xa", None, "日y".encode(), b"  "], pa.binary()).cast(pa.string(), safe=False)
    idx = pa.array([0, 1, 2, 7, None, 0, -1, 2, 3], pa.int32())
    strings = pa.DictionaryArray.from_arrays(idx, entries, safe=False)
    values = [b"xa", None, "日y".encode(), None, None, b"xa", None, "日y".encode(), b"  "]  # (such rows are NULL rows)
    t = Table({"s": (DICT, values)})
    trees = [like("s", "x%"), ("not", like("s", "_y")), ln("s", "=", 2), lt("s", ">", "x"), ("blank", "s"), ("isnull", "s")]
    plan = plan_of(trees, t)
    st = base.feed(plan, [[base.column(strings)]])
    want = [xs.counts(tr, t.rows, t.types) for tr in trees]
    assert [st.row_predicate_counts(i) for i in range(len(trees))] == want
    assert want[0] == (9, 2, 4, 3) and want[4] == (9, 1, 4, 4) and want[5] == (9, 4, 0, 5)


# ---- LIKE -------------------------------------------------------------------------------------------------------------------
NAMED = ["", "%", "%%", "_", "a", "a%", "%a", "%a%", "a%b", "a_c", "_%", "%_", "__%", "%aa%aa%", "a%ab", "%日_語%"]


def test_the_named_patterns():
    rows = VALUES[:400] + [b"aaa", b"aaaa", b"aaab", "日本語".encode(), "x日本語y".encode(), "日語".encode(), "日本本語".encode(), b"abc",
                           "a日c".encode(), b"ac", b"ab", b"a\nb", b"", b"a", "é".encode(), None]
    t = Table({"s": (UTF8, rows)})
    _, _, want = check([like("s", p) for p in NAMED], t)
    by = dict(zip(NAMED, want))
    assert by["%"][1] == by["%%"][1] == t.n - 1 and by[""][1] == rows.count(b"")
    one = lambda p, v: xs.like(v.encode(), p.encode())  # noqa: E731
    assert not one("%aa%aa%", "aaa") and one("%aa%aa%", "aaaa") and one("a%ab", "aaab") and one("%日_語%", "x日本語y")
    # the same as two-row tables, so that the device's answer on exactly these values is held
    for p, v, sat in (("%aa%aa%", "aaa", 0), ("%aa%aa%", "aaaa", 1), ("a%ab", "aaab", 1), ("%日_語%", "日本語", 1), ("%日_語%", "日語", 0)):
        _, _, w = check([like("s", p)], Table({"s": (UTF8, [v.encode(), None])}))
        assert w == [(2, sat, 1, 1 - sat)]


def test_a_256_byte_pattern():
    pattern = b"%" + b"ab" * 60 + b"_" * 7 + b"%" + b"b" * 126 + b"%"
    assert len(pattern) == 256
    hit = b"x" + b"ab" * 60 + "é日a    ".encode() + b"zz" + b"b" * 126
    rows = [hit, hit + b"tail", hit[1:], hit[:-1], hit.replace(b"zz", b""), b"ab" * 60 + b"1234567" + b"b" * 126, None, b"", b"ab" * 200]
    t = Table({"s": (UTF8, rows)})
    _, _, want = check([like("s", pattern), ("not", like("s", pattern))], t)
    assert want[0] == (9, 5, 1, 3)


def test_the_seeded_set():
    """200 patterns x 2000 values: a spec per pattern on one column"""
    rng = np.random.default_rng(2000)
    rows = nullable(rng, VALUES, 0.05)
    t = Table({"s": (UTF8, rows)})
    T.init()
    plan = plan_of([like("s", p) for p in PATTERNS], t)
    st = base.feed(plan, [t.columns()])
    nulls = rows.count(None)
    total_true = 0
    for i, p in enumerate(PATTERNS):
        sat = sum(xs.like(v, p) for v in rows if v is not None)
        assert st.row_predicate_counts(i) == (t.n, sat, nulls, t.n - sat - nulls), p
        total_true += sat
    assert 0.2 <= total_true / (len(PATTERNS) * (t.n - nulls)) <= 0.8


def test_32_like_leaves_in_one_program():
    """one of the 16 patterns that match most often, and none of the 16 that match least: 32 leaves, 64 ops"""
    patterns = [p for p in dict.fromkeys(PATTERNS) if p.strip(b"%") and len(p) <= 8][:32]
    assert len(patterns) == 32 and sum(len(p) for p in patterns) <= 256
    rate = {p: sum(xs.like(v, p) for v in VALUES[:1500]) for p in patterns}
    ranked = sorted(patterns, key=lambda p: (rate[p], p))
    tree = ("and", ex.any_of(*[like("s", p) for p in ranked[16:]]), ("not", ex.any_of(*[like("s", p) for p in ranked[:16]])))
    rng = np.random.default_rng(32)
    t = Table({"s": (LARGE, nullable(rng, VALUES[:1500], 0.1))})
    leaves, program, pool = xs.leaves_and_program(tree, ["s"])
    assert len(leaves) == 32 and len(program) == 64 and pool == b"".join(ranked[16:] + ranked[:16])
    _, _, want = check([tree], t)
    assert both_answers(want)


# ---- beside the other leaves, tasks and batchings -----------------------------------------------------------------------------
def mixed_table(n, seed=9):
    rng = np.random.default_rng(seed)
    s = nullable(rng, [VALUES[i % len(VALUES)] for i in range(n)], 0.15)
    u = nullable(rng, [(b"F", b"O", b"", "é".encode())[int(x)] for x in rng.integers(0, 4, n)], 0.1)
    a = nullable(rng, [int(x) for x in rng.integers(-5, 6, n)], 0.1)
    x = nullable(rng, [float(v) for v in np.round(rng.standard_normal(n), 1)], 0.1)
    return Table({"s": (UTF8, s), "u": (VIEW, u), "a": (I64, a), "x": (F64, x)})


MIXED = [
    ("and", like("s", "%a%"), ("or", ("cmp", "a", ">=", 0), ("streq", "u", b"F"))),
    ("or", ("and", ln("s", ">", 2), ("cmp", "x", "<", 0.5)), ("and", ("not", ("blank", "s")), ("cmpcol", "a", "<", "x"))),
    ("and", ("and", lt("s", ">=", "a"), ex.isin("u", [b"F", b"O"])), ("not", ("isnull", "a"))),
    ("or", ("cmpcol", "s", "=", "u"), ("and", like("u", "_"), ln("s", "=", 0, True))),
]


def test_new_leaves_beside_numeric_leaves_and_str_eq():
    _, _, want = check(MIXED, mixed_table(2500))
    assert both_answers(want) and any(w[2] > 0 for w in want)


def test_9_tasks_in_one_plan_are_two_launches():
    t = mixed_table(1200, seed=10)
    trees = [like("s", "%a%"), ln("s", ">=", 2), lt("s", "<", "b"), ("blank", "s"), MIXED[0], MIXED[1], like("u", "_"), ("cmp", "a", ">", 0),
             ("not", like("s", "_%_"))]
    assert len(trees) == 9
    check(trees, t)


@pytest.fixture(scope="module")
def big():
    t = mixed_table(9001, seed=11)
    trees = MIXED + [like("s", "%日%"), ln("s", "<=", 3)]
    return t, trees, [xs.counts(tr, t.rows, t.types) for tr in trees]


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_HOST, None), (T.MEM_HOST, 8192), (T.MEM_DEVICE, 8192)],
                         ids=["device", "host", "host-8192", "device-8192"])
def test_every_batching_gives_one_answer(big, mem, cuts):
    t, trees, want = big
    check(trees, t, mem=mem, cuts=cuts, want=want)


def test_reset_merge_and_a_blob_round_trip(big):
    t, trees, want = big
    st, plan, _ = check(trees, t, want=want)
    blob = st.serialize()
    back = T.State.deserialize(plan, blob)
    assert [back.row_predicate_counts(i) for i in range(len(trees))] == want and back.serialize() == blob
    leaves, program, pool = xs.leaves_and_program(trees[4], ["s"])
    assert wire.row_predicate_state(leaves, program, pool, *want[4][:3]) in blob
    halves = base.batches_of(t.columns(), t.n, 4500)
    a, b = base.feed(plan, halves[:1]), base.feed(plan, halves[1:])
    a.merge([b, back])
    assert [a.row_predicate_counts(i) for i in range(len(trees))] == [tuple(2 * x for x in w) for w in want]
    st.reset()
    assert [st.row_predicate_counts(i) for i in range(len(trees))] == [(0, 0, 0, 0)] * len(trees)
    st.update(t.columns())
    assert [st.row_predicate_counts(i) for i in range(len(trees))] == want
    other = plan_of(trees[:4] + [like("s", "%語%")] + trees[5:], t)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*ROW_PREDICATE task 4.*other literal bytes"):
        T.State.deserialize(other, blob)


def test_a_new_leaf_on_a_numeric_column_is_unsupported_and_the_state_stays_usable():
    T.init()
    t = Table({"a": (I64, [1, 2, None]), "s": (UTF8, [b"x", None, b"y"])})
    good = xs.counts(like("s", "x"), t.rows, t.types)
    for tree in (like("a", "x"), ln("a", ">", 0), ln("a", ">", 0, True), lt("a", "<", "x"), ("blank", "a")):
        plan = plan_of([like("s", "x"), tree], t)
        st = T.State(plan)
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*a string leaf.*numeric column"):
            st.update(t.columns())
        assert st.row_predicate_counts(0) == (0, 0, 0, 0)
        st.update([t.columns()[1], t.columns()[1]])  # a batch whose column fits: the state goes on
        assert st.row_predicate_counts(0) == good
    st = T.State(plan_of([("cmpcol", "s", "<", "s")], t))  # ordering two string COLUMNS stays what it was
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*orders two string columns"):
        st.update(t.columns())


# ---- end to end -------------------------------------------------------------------------------------------------------------
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return g, pa.table({name: pa.array(vals, pa.string()) for name, vals in g["table"].items()})


def datatype_of(case):
    v = S.StringTypeValidation.MaxBytes(case["max_bytes"]) if case["string"] == "max_bytes" else {"string": case["string"]}
    return S.DataTypeConstraint("name", S.DataTypeValidation.String(v))


def test_the_constraints_end_to_end_through_validation_suite_run():
    g, table = golden()
    for case in g["custom_sql"]:
        check_ = S.Check.builder("c").level(S.Level.Error).satisfies(case["expression"], case["hint"],
                                                                     string_functions_on_device=True).build()
        result = S.ValidationSuite.builder("s").check(check_).build().run(table)
        issues = result.report.issues
        if case["status"] == "success":
            assert not issues and result.report.metrics.passed_checks == 1, case["ref"]
        else:
            assert len(issues) == 1 and issues[0].constraint_name == "custom_sql", case["ref"]
            assert issues[0].message == case["message"] and issues[0].metric == case["metric"], case["ref"]
    for case in g["datatype"]:
        check_ = S.Check.builder("c").level(S.Level.Error).constraint(datatype_of(case).string_functions_on_device(True)).build()
        result = S.ValidationSuite.builder("s").check(check_).build().run(table)
        issues = result.report.issues
        if case["status"] == "success":
            assert not issues and result.report.metrics.passed_checks == 1, case["ref"]
        else:
            assert len(issues) == 1 and issues[0].constraint_name == "datatype", case["ref"]
            assert issues[0].message == case["message"] and issues[0].metric == case["metric"], case["ref"]
    # all of them in one suite: one pass over the table
    b = S.Check.builder("all").level(S.Level.Error)
    for case in g["custom_sql"]:
        b = b.satisfies(case["expression"], case["hint"], string_functions_on_device=True)
    for case in g["datatype"]:
        b = b.constraint(datatype_of(case).string_functions_on_device(True))
    result = S.ValidationSuite.builder("s").check(b.build()).build().run(table)
    want = [c["message"] for c in g["custom_sql"] + g["datatype"] if c["status"] == "failure"]
    assert [i.message for i in result.report.issues] == want
    # a new leaf on a column that is no string is the failure a misfit leaf always was
    numbers = pa.table({"name": pa.array([1, 2, 3], pa.int64())})
    check_ = S.Check.builder("c").satisfies("name LIKE 'a%'", None, string_functions_on_device=True).build()
    messages = [i.message for i in S.ValidationSuite.builder("s").check(check_).build().run(numbers).report.issues]
    assert len(messages) == 1 and messages[0].startswith("SQL expression error: ") and messages[0].endswith("Expression: 'name LIKE 'a%''")


def test_without_the_opt_in_the_suite_reports_todays_errors():
    g, table = golden()
    b = S.Check.builder("all").level(S.Level.Error)
    for case in g["custom_sql"]:
        b = b.satisfies(case["expression"], case["hint"])
    for case in g["datatype"]:
        b = b.constraint(datatype_of(case))
    result = S.ValidationSuite.builder("s").check(b.build()).build().run(table)
    messages = [i.message for i in result.report.issues]
    assert len(messages) == len(g["custom_sql"]) + len(g["datatype"]) and result.report.metrics.passed_checks == 0
    assert all(m.startswith("Error evaluating constraint") and "not on the GPU path" in m for m in messages)
    for m, what in zip(messages, ("LIKE", "LIKE", "a function call (LENGTH(..))", "a string order comparison", "a function call (OCTET_LENGTH(..))")):
        assert "the expression is not on the GPU path: " + what in m
    for m in messages[len(g["custom_sql"]):]:
        assert "validation reads a string column (not on the GPU path)" in m


def test_the_analyzer_end_to_end_through_analysis_runner():
    g, table = golden()
    c = g["compliance"]
    ctx = (S.AnalysisRunner().add(S.ComplianceAnalyzer("emails", c["predicate"], string_functions_on_device=True))
           .add(S.SizeAnalyzer()).run(table))
    assert ctx.states["compliance"] == {"compliant_count": c["compliant_count"], "total_count": c["total_count"]}
    assert ctx.metrics["compliance"] == {"type": "Double", "value": c["metric"]} and not ctx.errors()
    ctx = S.AnalysisRunner().add(S.ComplianceAnalyzer("emails", c["predicate"])).add(S.SizeAnalyzer()).run(table)
    errors = ctx.errors()
    assert len(errors) == 1 and "not on the GPU path: LIKE" in errors[0]["error"] and "compliance" not in ctx.metrics
