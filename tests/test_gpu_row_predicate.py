"""-m gpu: TGX_CHECK_ROW_PREDICATE, the row predicates behind Check::satisfies and ComplianceAnalyzer.  The reference is
tests/exact_row_predicate.py -- a per-row walk of an expression tree, neither the library nor its compiler -- and EVERY
counter (seen, satisfied, unknown, failed) is compared for equality; there are no tolerances.  The leaves and the program
a tree becomes are the tests' own lowering (exact_row_predicate.leaves_and_program), except where a test is about the
library's compiler."""
import json
import os
import threading

import numpy as np
import pyarrow as pa
import pytest

import exact_row_predicate as ex
import term_amd as T
import term_amd.suite as S
from _lib_spec import spec
from gpu_util import to_device
from term_amd import wire

pytestmark = pytest.mark.gpu

I64, I32, I8, U32, U64, F64, F32, BOOL = (pa.int64(), pa.int32(), pa.int8(), pa.uint32(), pa.uint64(), pa.float64(),
                                          pa.float32(), pa.bool_())
UTF8, LARGE, VIEW, DICT = pa.string(), pa.large_string(), pa.string_view(), "dictionary"
STRINGS = (UTF8, LARGE, VIEW, DICT)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "custom_sql_vectors.json")
NAN_POS, NAN_NEG = ex.from_bits(0x7FF8000000000000), ex.from_bits(0xFFF8000000000000)
NAN_PAYLOAD = ex.from_bits(0x7FF0000000000123)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
INT_EDGES = [I64_MIN, -1, 0, 1, I64_MAX, 2**31, -2**31, 2**53, 2**53 + 1, -2**53 - 1, 2**53 + 2, 1000, -1000]
FLOAT_EDGES = [0.0, -0.0, 5e-324, -5e-324, float("inf"), -float("inf"), NAN_POS, NAN_NEG, NAN_PAYLOAD, 0.5, -0.5, 2.0,
               2.0**53, 1e300, -1e300, 0.1, 0.10000000000000002]


# ---- columns --------------------------------------------------------------------------------------------------------------
def kind_of(typ):
    if typ in STRINGS:
        return "str"
    return "float" if typ in (F64, F32) else "int"


def array(values, typ):
    if typ in (F64, F32):  # (through numpy: a NaN keeps its sign and payload)
        mask = np.array([v is None for v in values], bool)
        vals = np.array([ex.bits_of(0.0 if v is None else v) for v in values], np.int64).view(np.float64)
        arr = pa.array(vals, F64, mask=mask if mask.any() else None)
        return arr if typ == F64 else arr.cast(F32, safe=False)
    if typ not in STRINGS:
        return pa.array(values, typ)
    values = [None if v is None else bytes(v) for v in values]
    if typ == DICT:
        entries = sorted(set(v for v in values if v is not None)) or [b"unused"]
        at = {v: i for i, v in enumerate(entries)}
        idx = pa.array([None if v is None else at[v] for v in values], pa.int32())
        return pa.DictionaryArray.from_arrays(idx, pa.array(entries, pa.binary()).cast(pa.string(), safe=False))
    return pa.array(values, {UTF8: pa.binary(), LARGE: pa.large_binary(), VIEW: pa.binary_view()}[typ])


def padded(buf):
    if buf is None:
        return None
    raw = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return to_device(np.concatenate([raw, np.zeros(64, np.uint8)]))


def on_device(col):
    values, validity, offsets, data, dictionary, variadic = col._keep[:6]
    return T.Column(col.c.type, col.c.length, values=padded(values), validity=padded(validity), offsets=padded(offsets),
                    data=padded(data), offset=col.c.offset, mem=T.MEM_DEVICE,
                    dictionary=None if dictionary is None else on_device(dictionary),
                    variadic=None if variadic is None else [padded(b) for b in variadic])


def column(arr, mem=T.MEM_DEVICE):
    col = T.Column.from_arrow(arr)
    if mem == T.MEM_DEVICE:
        return on_device(col)
    col.c.mem = mem
    return col


def filler(typ):
    return b"pad" if typ in STRINGS else 1.5 if typ in (F64, F32) else 1


class Table:
    """named columns: {name: (arrow type, values)}; a value is None, an int, a float or bytes"""

    def __init__(self, columns):
        self.names = list(columns)
        self.arrow = {c: columns[c][0] for c in self.names}
        self.values = {c: list(columns[c][1]) for c in self.names}
        self.n = len(self.values[self.names[0]])
        self.types = {c: kind_of(self.arrow[c]) for c in self.names}
        # what a widened Float32 holds is what the walk must see
        for c in self.names:
            if self.arrow[c] == F32:
                self.values[c] = [None if v is None else float(np.float32(v)) for v in self.values[c]]
        self.rows = ex.table_rows(self.values)

    def columns(self, mem=T.MEM_DEVICE, offsets=None):
        offsets = offsets or {}
        cols = []
        for c in self.names:
            off = offsets.get(c, 0)
            arr = array([filler(self.arrow[c])] * off + self.values[c], self.arrow[c])
            cols.append(column(arr, mem).sliced(off, self.n))
        return cols


def columns_of_tree(tree, names):
    """the columns a tree names, in table order"""
    found = set()

    def visit(t):
        if t[0] in ("and", "or"):
            visit(t[1]), visit(t[2])
        elif t[0] == "not":
            visit(t[1])
        else:
            found.add(t[1])
            if t[0] == "cmpcol":
                found.add(t[3])
    visit(tree)
    return [c for c in names if c in found]


def plan_of(trees, table, extra=()):
    specs, preds = [], []
    for tree in trees:
        cols = columns_of_tree(tree, table.names)
        specs.append(spec(T.ROW_PREDICATE, 0, columns=[table.names.index(c) for c in cols]))
        preds.append(ex.leaves_and_program(tree, cols))
    plan = T.Plan(specs + list(extra))
    for i, (leaves, program, pool) in enumerate(preds):
        plan.set_row_predicate(i, leaves, program, pool)
    return plan


def batches_of(cols, n, cuts):
    if cuts is None:
        return [cols]
    bounds = list(range(0, n, cuts)) + [n]
    return [[c.sliced(lo, hi - lo) for c in cols] for lo, hi in zip(bounds[:-1], bounds[1:])]


def feed(plan, batches):
    st = T.State(plan)
    for b in batches:
        st.update(b)
    return st


def check(trees, table, mem=T.MEM_DEVICE, cuts=None, offsets=None, want=None):
    T.init()
    want = [ex.counts(t, table.rows, table.types) for t in trees] if want is None else want
    plan = plan_of(trees, table)
    st = feed(plan, batches_of(table.columns(mem, offsets), table.n, cuts))
    got = [st.row_predicate_counts(i) for i in range(len(trees))]
    assert got == want
    for r, (seen, sat, unk, failed) in zip(st.finalize(), want):
        assert (r.total, r.matches, r.non_null) == (seen, sat, seen - unk) and sat + unk + failed == seen
    return st, plan, want


def nullable(rng, values, frac):
    return [None if rng.random() < frac else v for v in values]


def numeric_table(rng, n, n_cols=8, null=0.15):
    """n_cols columns a .. h: Int64 and Float64 alternating, the odd ones without NULLs where null is None for them"""
    cols = {}
    for k in range(n_cols):
        name = "abcdefgh"[k]
        if k % 2 == 0:
            v = [int(x) for x in rng.integers(-50, 50, n)]
            for i in range(min(n, len(INT_EDGES))):
                v[(i * 7 + k) % n] = INT_EDGES[i]
            cols[name] = (I64, nullable(rng, v, null if k % 4 == 0 else 0.0))
        else:
            v = [float(x) for x in np.round(rng.standard_normal(n) * 20.0)]
            for i in range(min(n, len(FLOAT_EDGES))):
                v[(i * 5 + k) % n] = FLOAT_EDGES[i]
            cols[name] = (F64, nullable(rng, v, null))
    return Table(cols)


ONE = [("cmp", "a", ">=", 0), ("not", ("cmp", "a", "=", 2.0**53)), ("isnull", "a")]
TWO = [("and", ("cmp", "a", "<=", 10), ("cmp", "b", ">", -0.0)), ("cmpcol", "a", "<", "b"),
       ("or", ("isnull", "a"), ("cmpcol", "b", "=", "b"))]
FOUR = [ex.all_of(ex.between("a", -20, 20), ("cmpcol", "c", ">=", "a"), ("not", ("cmp", "b", "=", NAN_POS)),
                  ("or", ("cmp", "d", "<", 0.5), ("isnull", "d")))]
EIGHT = [ex.any_of(ex.all_of(("cmp", "a", ">", 0), ("cmp", "b", ">", 0.0), ("cmpcol", "c", "<=", "e"), ("cmpcol", "d", ">=", "f")),
                   ("not", ("cmpcol", "g", "=", "h")), ("isnull", "h"))]


# ---- sizes, offsets, validity ---------------------------------------------------------------------------------------------
# one short of, exactly and one over: a pair, a wave of rows (general route) and of pairs, a workgroup's first loads (256
# pairs) and its trip at 1, 2 and 4 pairs in flight (512, 1024, 2048 rows), and a second workgroup (4096 rows)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
                               2049, 4095, 4096, 4097])
def test_row_counts(n):
    rng = np.random.default_rng(n)
    t = numeric_table(rng, max(n, 1))
    if n == 0:
        t = Table({c: (t.arrow[c], []) for c in t.names})
        t.n = 0
    check(ONE + TWO + FOUR + EIGHT, t)
    s = Table({"s": (UTF8, nullable(rng, [b"v%d" % (i % 5) for i in range(n)], 0.2) if n else []),
               "a": (I64, nullable(rng, list(range(n)), 0.2) if n else [])})
    s.n = n
    check([("and", ex.isin("s", [b"v1", b"v3"]), ("cmp", "a", ">=", 2))], s)


@pytest.mark.parametrize("offsets", [(0, 1), (1, 0), (7, 8), (8, 9), (9, 7), (1, 1), (8, 8)], ids=str)
def test_arrow_offsets_chosen_per_column(offsets):
    """0 and 8 keep a column on 16-byte loads, 1, 7 and 9 put it on 8-byte loads; even and odd offsets read the pair's two
    validity bits from one byte or from two"""
    rng = np.random.default_rng(sum(offsets) * 31 + offsets[0])
    t = numeric_table(rng, 2049 + 77, 4)
    offs = {"a": offsets[0], "b": offsets[1], "c": offsets[1], "d": offsets[0]}
    check(ONE + TWO + FOUR, t, offsets=offs)
    s = Table({"s": (VIEW, nullable(rng, [b"value-%d-longer-than-twelve" % (i % 7) if i % 3 else b"v%d" % (i % 7)
                                         for i in range(300)], 0.2)),
               "a": (I64, nullable(rng, list(range(300)), 0.2))})
    check([("or", ("streq", "s", b"v2"), ("and", ("streq", "s", b"value-4-longer-than-twelve"), ("cmp", "a", "<", 200)))], s,
          offsets={"s": offsets[0], "a": offsets[1]})


def test_columns_with_and_without_a_validity_bitmap_side_by_side():
    rng = np.random.default_rng(3)
    n = 5001
    t = Table({"a": (I64, [int(x) for x in rng.integers(-9, 9, n)]),                 # no bitmap
               "b": (F64, nullable(rng, [float(x) for x in rng.integers(-9, 9, n)], 0.3)),
               "c": (I64, [None] * n),                                                # all NULL
               "d": (F64, [float(x) for x in rng.integers(-9, 9, n)])})              # no bitmap
    _, _, want = check(TWO + FOUR + [("isnull", "c"), ("cmp", "c", "=", 1), ("or", ("cmp", "c", "=", 1), ("cmp", "a", ">", 0))], t)
    assert want[-3] == (n, n, 0, 0) and want[-2] == (n, 0, n, 0)


# ---- Kleene's logic on the device ----------------------------------------------------------------------------------------
def test_the_27_row_kleene_table_for_every_two_and_three_leaf_program_shape():
    """three columns x {NULL, 0, 1}: every combination of TRUE / FALSE / UNKNOWN of three leaves, under every shape a
    program of two or three leaves can have"""
    vals = [None, 0, 1]
    rows = [(x, y, z) for x in vals for y in vals for z in vals]
    t = Table({"a": (I64, [r[0] for r in rows]), "b": (I64, [r[1] for r in rows]), "c": (I64, [r[2] for r in rows])})
    A, B, C = (("cmp", c, "=", 1) for c in "abc")
    nots = lambda x: (x, ("not", x))  # noqa: E731
    trees = []
    for a in nots(A):
        for b in nots(B):
            for op in ("and", "or"):
                trees.extend(nots((op, a, b)))
                for c in nots(C):
                    for op2 in ("and", "or"):
                        trees.append((op2, (op, a, b), c))
                        trees.append((op2, a, (op, b, c)))
                        trees.append(("not", (op2, ("not", (op, a, b)), c)))
    assert len(trees) == 2 * 2 * 2 * (2 + 2 * 2 * 3)
    for at in range(0, len(trees), 28):
        check(trees[at:at + 28], t)
    # (and the tables themselves, spelled out once: a AND b, a OR b over TRUE / FALSE / UNKNOWN)
    two = Table({"a": (I64, [1, 1, 1, 0, 0, 0, None, None, None]), "b": (I64, [1, 0, None] * 3)})
    _, _, want = check([("and", A, B), ("or", A, B), ("not", A)], two)
    assert want == [(9, 1, 3, 5), (9, 5, 3, 1), (9, 3, 3, 3)]


def test_8_columns_32_leaves_and_a_program_of_depth_32():
    rng = np.random.default_rng(8)
    t = numeric_table(rng, 3000)
    leaves = [("cmp", "abcdefgh"[j % 8], OPS[j % 5], (j - 16) if j % 8 % 2 == 0 else float(j) - 15.5) for j in range(32)]
    # right-nested: all 32 leaves are pushed before the first operator runs
    deep = leaves[31]
    for j in range(30, -1, -1):
        deep = ("or" if j % 3 else "and", leaves[j], deep)
    flat = leaves[0]
    for j in range(1, 32):
        flat = ("and" if j % 4 == 0 else "or", flat, leaves[j])
    _, program, _ = ex.leaves_and_program(deep, list("abcdefgh"))
    assert [p[0] for p in program[:32]] == [ex.PUSH] * 32 and len(program) == 63
    check([deep, flat], t)
    s = Table(dict({c: (t.arrow[c], t.values[c]) for c in "abcdefg"}, h=(UTF8, [b"k%d" % (i % 4) for i in range(t.n)])))
    mixed = ("and", ("or", deep_without_h(leaves), ("streq", "h", b"k1")), ("not", ("streq", "h", b"k3")))
    check([mixed], s)


OPS = ex.OPS


def deep_without_h(leaves):
    keep = [l for l in leaves if l[1] != "h"]
    tree = keep[-1]
    for l in reversed(keep[:-1]):
        tree = ("or", l, tree)
    return tree


def test_9_tasks_in_one_plan_are_two_launches():
    rng = np.random.default_rng(9)
    t = numeric_table(rng, 4100, 4)
    trees = ONE + TWO + FOUR + [("cmp", "b", "<", 1.5), ("cmpcol", "c", ">", "d")]
    assert len(trees) == 9
    T.init()
    plan = plan_of(trees, t)
    st = T.State(plan)
    st.profile_enable()
    st.update(t.columns())
    assert [st.row_predicate_counts(i) for i in range(9)] == [ex.counts(tr, t.rows, t.types) for tr in trees]
    assert st.profile_get("row_predicate")["launches"] == 2


# ---- types ---------------------------------------------------------------------------------------------------------------
def tiled(values):
    values = list(values)
    if len(values) % 2 == 0:
        values.append(values[0])
    return values * 64


def test_int64_and_float64_edges_at_every_lane():
    """-0.0 / +0.0, both NaNs, 2^53 + 1 against a double literal, INT64_MIN: every comparison, int and double literal"""
    n = len(tiled(INT_EDGES))
    t = Table({"a": (I64, tiled(INT_EDGES)), "b": (F64, (tiled(FLOAT_EDGES) * 2)[:n])})
    trees = []
    for op in OPS:
        trees += [("cmp", "a", op, 2**53), ("cmp", "a", op, 2.0**53), ("cmp", "a", op, I64_MIN), ("cmp", "a", op, -0.5),
                  ("cmp", "b", op, 0), ("cmp", "b", op, -0.0), ("cmp", "b", op, 0.0), ("cmp", "b", op, NAN_POS),
                  ("cmp", "b", op, NAN_NEG), ("cmp", "b", op, 0.1), ("cmpcol", "a", op, "b"), ("cmpcol", "b", op, "a"),
                  ("cmpcol", "a", op, "a"), ("cmpcol", "b", op, "b")]
    for at in range(0, len(trees), 24):
        check(trees[at:at + 24], t)
    # 2^53 + 1 equals the double literal 2^53 (the conversion rounds to even) and not the integer literal
    small = Table({"a": (I64, [2**53, 2**53 + 1, 2**53 + 2, None])})
    _, _, want = check([("cmp", "a", "=", 2.0**53), ("cmp", "a", "=", 2**53)], small)
    assert want == [(4, 2, 1, 1), (4, 1, 1, 2)]
    zeros = Table({"b": (F64, [0.0, -0.0, NAN_POS, NAN_NEG])})
    _, _, want = check([("cmp", "b", "=", 0.0), ("cmp", "b", ">=", 0), ("cmp", "b", "=", NAN_POS), ("cmp", "b", "<", -float("inf"))], zeros)
    assert want == [(4, 1, 0, 3), (4, 2, 0, 2), (4, 1, 0, 3), (4, 1, 0, 3)]


@pytest.mark.parametrize("typ", [I32, F32, I8, U32], ids=str)
def test_narrow_columns_through_widening(typ):
    rng = np.random.default_rng(len(str(typ)))
    n = 3001
    if typ == F32:
        v = [float(x) for x in np.round(rng.standard_normal(n) * 4.0, 1)]
        v[:6] = [0.0, -0.0, NAN_POS, NAN_NEG, float("inf"), 0.1]
    elif typ == I8:
        v = [int(x) for x in rng.integers(-128, 128, n)]
    elif typ == U32:
        v = [int(x) for x in rng.integers(0, 2**32, n)]
        v[:3] = [0, 2**32 - 1, 2**31]
    else:
        v = [int(x) for x in rng.integers(-2**31, 2**31, n)]
        v[:3] = [-2**31, 2**31 - 1, 0]
    t = Table({"a": (typ, nullable(rng, v, 0.2)), "b": (I64, [int(x) for x in rng.integers(-100, 2**32, n)])})
    lit = 0.1 if typ == F32 else 2**31
    check([("cmp", "a", ">=", 0), ("cmp", "a", "<", lit), ("cmp", "a", "=", float(np.float32(0.1))), ("cmpcol", "a", "<=", "b"),
           ("isnull", "a")], t, offsets={"a": 3})


def test_cmp_columns_in_all_three_type_pairings():
    rng = np.random.default_rng(33)
    n = 2500
    t = Table({"a": (I64, nullable(rng, [int(x) for x in rng.integers(-5, 5, n)], 0.2)),
               "b": (I64, nullable(rng, [int(x) for x in rng.integers(-5, 5, n)], 0.2)),
               "x": (F64, nullable(rng, [float(x) for x in rng.integers(-5, 5, n)], 0.2)),
               "s": (UTF8, nullable(rng, [b"k%d" % x for x in rng.integers(0, 4, n)], 0.2)),
               "u": (DICT, nullable(rng, [b"k%d" % x for x in rng.integers(0, 4, n)], 0.2))})
    trees = [("cmpcol", "a", op, "b") for op in OPS] + [("cmpcol", "a", op, "x") for op in OPS] + \
            [("cmpcol", "x", op, "a") for op in OPS] + [("cmpcol", "s", "=", "u"), ("not", ("cmpcol", "u", "=", "s"))]
    check(trees, t)


# ---- strings --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", STRINGS, ids=str)
def test_strings_in_every_layout(layout):
    """inline (<= 12 bytes) and long views, the empty string as a value and as a literal, a literal that is a proper
    prefix or an extension of the value"""
    rng = np.random.default_rng(STRINGS.index(layout))
    pool = [b"", b"a", b"ab", b"abc", b"twelve-bytes", b"thirteen-byte", b"thirteen-bytes", b"a-value-that-is-long-enough-for-a-view",
            b"a-value-that-is-long-enough-for-a-vieW", b"F", b"O", b"P"]
    v = nullable(rng, [pool[int(x)] for x in rng.integers(0, len(pool), 1500)], 0.2)
    t = Table({"s": (layout, v), "a": (I64, list(range(1500)))})
    trees = [("streq", "s", lit) for lit in (b"", b"a", b"ab", b"abcd", b"twelve-bytes", b"thirteen-byte", b"thirteen-bytes!",
                                             b"a-value-that-is-long-enough-for-a-view", b"absent")]
    trees += [ex.isin("s", [b"F", b"O", b"P"]), ("not", ex.isin("s", [b"F", b"", b"abc"])), ("isnull", "s"),
              ("and", ("streq", "s", b"ab"), ("cmp", "a", ">=", 700))]
    check(trees, t)
    check(trees, t, offsets={"s": 5, "a": 1}, cuts=401)


def test_a_dictionary_with_a_null_entry_and_an_index_outside_it():
    T.init()
    entries = pa.array([b"x", None, b"y"], pa.binary()).cast(pa.string(), safe=False)
    idx = pa.array([0, 1, 2, 7, None, 0, -1, 2], pa.int32())
    strings = pa.DictionaryArray.from_arrays(idx, entries, safe=False)
    values = [b"x", None, b"y", None, None, b"x", None, b"y"]  # (the rule of VALUE_COUNTS: such rows are NULL rows)
    t = Table({"s": (DICT, values)})
    trees = [("streq", "s", b"x"), ("not", ("streq", "s", b"y")), ("isnull", "s"), ("cmpcol", "s", "=", "s")]
    plan = plan_of(trees, t)
    st = feed(plan, [[column(strings)]])
    want = [ex.counts(tr, t.rows, t.types) for tr in trees]
    assert [st.row_predicate_counts(i) for i in range(4)] == want
    assert want[0] == (8, 2, 4, 2) and want[2] == (8, 4, 0, 4)


# ---- the golden table and batchings --------------------------------------------------------------------------------------
def golden_table():
    with open(GOLDEN) as f:
        g = json.load(f)["custom_sql"]["table"]
    return Table({"price": (F64, g["price"]), "quantity": (I64, g["quantity"]),
                  "status": (UTF8, [None if s is None else s.encode() for s in g["status"]])})


def test_a_mixed_predicate_on_the_golden_table():
    t = golden_table()
    tree = ("and", ("streq", "status", b"active"), ("cmp", "price", ">=", 10))
    _, _, want = check([tree, ("cmp", "price", ">", 0), ("cmp", "quantity", ">=", 0), ("not", ("isnull", "price"))], t)
    assert want == [(5, 3, 0, 2), (5, 4, 1, 0), (5, 5, 0, 0), (5, 4, 0, 1)]


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(77)
    n = 70_001
    t = numeric_table(rng, n, 4)
    t = Table(dict({c: (t.arrow[c], t.values[c]) for c in t.names},
                   s=(UTF8, nullable(rng, [b"k%d" % x for x in rng.integers(0, 6, n)], 0.1))))
    trees = [ONE[0], TWO[0], FOUR[0], ("and", ex.isin("s", [b"k1", b"k4"]), ("cmp", "a", ">=", 0))]
    return t, trees, [ex.counts(tr, t.rows, t.types) for tr in trees]


@pytest.mark.parametrize("mem,cuts", [(T.MEM_DEVICE, None), (T.MEM_HOST, None), (T.MEM_HOST, 8192), (T.MEM_DEVICE, 8192)],
                         ids=["device", "host", "host-8192", "device-8192"])
def test_70001_rows_in_every_batching_give_one_answer(big, mem, cuts):
    t, trees, want = big
    check(trees, t, mem=mem, cuts=cuts, want=want)


def test_a_table_of_300000_rows_takes_more_than_one_trip_per_lane():
    rng = np.random.default_rng(300)
    n = 300_000
    a = rng.integers(-100, 100, n)
    b = np.round(rng.standard_normal(n) * 50.0) + 0.0  # (no -0.0: numpy's < and the totalOrder keys then agree)
    am, bm = rng.random(n) >= 0.1, rng.random(n) >= 0.1
    # (numpy's own arithmetic here: the walk over 300 000 rows would take the test's seconds)
    sat = int(np.sum(am & bm & (a >= 0) & (a.astype(np.float64) < b)))
    unk = int(np.sum(~(am & bm) & ~(am & (a < 0)) & ~(am & bm & (a.astype(np.float64) >= b))))
    tree = ("and", ("cmp", "a", ">=", 0), ("cmpcol", "a", "<", "b"))
    t = Table({"a": (I64, [int(x) if m else None for x, m in zip(a[:2000], am[:2000])]),
               "b": (F64, [float(x) if m else None for x, m in zip(b[:2000], bm[:2000])])})
    check([tree], t)  # (the numpy form below is held to the walk on the first 2000 rows)
    head = ex.counts(tree, t.rows, t.types)
    hs = int(np.sum(am[:2000] & bm[:2000] & (a[:2000] >= 0) & (a[:2000].astype(np.float64) < b[:2000])))
    assert head[1] == hs
    T.init()
    cols = [column(pa.array(a, I64, mask=~am)), column(pa.array(b, F64, mask=~bm))]
    big_t = Table({"a": (I64, [0]), "b": (F64, [0.0])})
    st = feed(plan_of([tree], big_t), [cols])
    assert st.row_predicate_counts(0) == (n, sat, unk, n - sat - unk)


# ---- the state: reset, merge, blobs, ranks --------------------------------------------------------------------------------
def test_reset_merge_and_a_blob_round_trip(big):
    t, trees, want = big
    st, plan, _ = check(trees, t, want=want)
    blob = st.serialize()
    back = T.State.deserialize(plan, blob)
    assert [back.row_predicate_counts(i) for i in range(len(trees))] == want and back.serialize() == blob
    leaves, program, pool = ex.leaves_and_program(trees[0], columns_of_tree(trees[0], t.names))
    assert wire.row_predicate_state(leaves, program, pool, *want[0][:3]) in blob
    halves = batches_of(t.columns(), t.n, 35_000)
    a, b = feed(plan, halves[:1]), feed(plan, halves[1:])
    a.merge([b, back])
    assert [a.row_predicate_counts(i) for i in range(len(trees))] == [tuple(2 * x for x in w) for w in want]
    st.reset()
    assert [st.row_predicate_counts(i) for i in range(len(trees))] == [(0, 0, 0, 0)] * len(trees)
    st.update(t.columns())
    assert [st.row_predicate_counts(i) for i in range(len(trees))] == want
    other = plan_of([("cmp", "a", ">=", 1)] + trees[1:], t)
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*ROW_PREDICATE task 0.*other leaves"):
        T.State.deserialize(other, blob)


def test_allreduce_on_threaded_ranks_at_world_2(big):
    """every rank a thread with its own state and row shard, tgx_allreduce over the thread-barrier transport; every rank
    ends with the table's counts"""
    import torch
    from term_amd.distributed import ThreadGroup, shard_rows, sharded_suite_step, thread_comm

    t, trees, want = big
    T.init()
    whole = t.columns()
    plan = plan_of(trees, t, [spec(T.COUNT, 0)])
    world = 2
    group = ThreadGroup(world)
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            lo, hi = shard_rows(t.n, world, rank)
            st = T.State(plan)
            comm = thread_comm(group, rank, device_buffers=True)
            res = sharded_suite_step(plan, st, [c.sliced(lo, hi - lo) for c in whole], comm)
            results[rank] = (res, [st.row_predicate_counts(i) for i in range(len(trees))])
        except Exception:  # noqa: BLE001
            import traceback

            errors.append((rank, traceback.format_exc()))
            group.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=150)
    assert not errors, errors
    assert not any(th.is_alive() for th in threads), "a rank is stuck"
    for res, got in results:
        assert got == want
        assert res[len(trees)].total == t.n


# ---- refusals and neighbours ---------------------------------------------------------------------------------------------
def test_a_mismatched_leaf_is_unsupported_and_the_state_stays_usable():
    T.init()
    t = Table({"a": (I64, [1, 2, None]), "s": (UTF8, [b"x", None, b"y"])})
    good = ex.counts(("cmp", "a", ">=", 2), t.rows, t.types)
    for tree, columns, msg in (
            (("streq", "a", b"x"), None, "a string leaf.*numeric column"),
            (("cmp", "s", ">=", 2), None, "a numeric leaf.*string column"),
            (("cmpcol", "a", "=", "s"), None, "a string column with a numeric one"),
            (("cmpcol", "s", "<", "s"), None, "orders two string columns")):
        plan = plan_of([("cmp", "a", ">=", 2), tree], t)
        st = T.State(plan)
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*" + msg):
            st.update(t.columns())
        assert st.row_predicate_counts(0) == (0, 0, 0, 0)
    # UInt64, Boolean and validity-only columns take IS NULL and nothing else; the state goes on with a batch that fits
    u = Table({"a": (U64, [1, None, 3]), "b": (BOOL, [True, None, False])})
    st, _, want = check([("isnull", "a"), ("not", ("isnull", "b"))], u)
    assert want == [(3, 1, 0, 2), (3, 2, 0, 1)]
    for col, word in (("a", "UInt64"), ("b", "Boolean")):
        st = T.State(plan_of([("cmp", col, "=", 1)], u))
        with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*%s.*IS NULL only" % word):
            st.update(u.columns())
    plan = plan_of([("cmp", "a", ">=", 2), ("isnull", "a")], t)
    st = T.State(plan)
    bare = T.Column(T.INT64, 3, values=None, validity=to_device(np.array([0b011] + [0] * 63, np.uint8)), mem=T.MEM_DEVICE)
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*validity-only|TGX_INVALID_ARGUMENT.*values is NULL"):
        st.update([bare, t.columns()[1]])
    st.update(t.columns())
    assert st.row_predicate_counts(0) == good
    only_null = T.State(plan_of([("isnull", "a")], t))
    only_null.update([bare, t.columns()[1]])
    assert only_null.row_predicate_counts(0) == (3, 1, 0, 2)


def test_beside_count_numeric_stats_and_value_rule_on_the_same_column():
    rng = np.random.default_rng(12)
    n = 9000
    t = Table({"a": (I64, nullable(rng, [int(x) for x in rng.integers(-40, 40, n)], 0.2))})
    tree = ex.between("a", -10, 10)
    want = ex.counts(tree, t.rows, t.types)
    extra = [spec(T.COUNT, 0), spec(T.NUMERIC_STATS, 0), spec(T.VALUE_RULE, 0)]

    def alone(s, rule=False):
        plan = T.Plan([s])
        if rule:
            plan.set_value_rule(0, T.RULE_BETWEEN, lo_i=-10, hi_i=10, lo_f=-10.0, hi_f=10.0)
        st = feed(plan, [t.columns()])
        r = st.finalize()[0]
        return (r.total, r.non_null, r.matches, r.min_i, r.max_i, r.sum_i)
    T.init()
    plan = plan_of([tree], t, extra)
    plan.set_value_rule(3, T.RULE_BETWEEN, lo_i=-10, hi_i=10, lo_f=-10.0, hi_f=10.0)
    st = feed(plan, [t.columns()])
    assert st.row_predicate_counts(0) == want
    res = st.finalize()
    for i, s in enumerate(extra):
        r = res[1 + i]
        assert (r.total, r.non_null, r.matches, r.min_i, r.max_i, r.sum_i) == alone(s, rule=s.kind == T.VALUE_RULE)
    assert res[3].matches == want[1]  # (the same predicate, as VALUE_RULE's BETWEEN counts it)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def arrow_golden(which):
    with open(GOLDEN) as f:
        g = json.load(f)[which]["table"]
    cols = {}
    for name, vals in g.items():
        if any(isinstance(v, str) for v in vals):
            cols[name] = pa.array(vals, pa.string())
        elif any(isinstance(v, float) for v in vals):
            cols[name] = pa.array(vals, F64)
        else:
            cols[name] = pa.array(vals, I64)
    return pa.table(cols)


def test_the_constraint_end_to_end_through_validation_suite_run():
    with open(GOLDEN) as f:
        cases = json.load(f)["custom_sql"]["cases"]
    table = arrow_golden("custom_sql")
    for case in cases:
        check_ = S.Check.builder("c").level(S.Level.Error).satisfies(case["expression"], case.get("hint")).build()
        result = S.ValidationSuite.builder("s").check(check_).build().run(table)
        issues = result.report.issues
        if case["status"] == "success":
            assert not issues and result.report.metrics.passed_checks == 1
        else:
            assert len(issues) == 1 and issues[0].constraint_name == "custom_sql"
            for fragment in case["message_contains"]:
                assert fragment in issues[0].message
            if case["metric"] is not None:
                assert issues[0].metric == case["metric"]
    # an expression outside the subset is the constraint's own error; the others keep their verdicts
    check_ = (S.Check.builder("c").satisfies("LENGTH(status) > 3").satisfies("quantity >= 0")
              .satisfies("status >= 2").build())
    result = S.ValidationSuite.builder("s").check(check_).build().run(table)
    messages = [i.message for i in result.report.issues]
    assert len(messages) == 2 and result.report.metrics.passed_checks == 1
    assert "not on the GPU path: a function call (LENGTH(..))" in messages[0] and messages[0].startswith("Error evaluating constraint")
    assert messages[1].startswith("SQL expression error: ") and messages[1].endswith("Expression: 'status >= 2'")


def test_the_analyzer_end_to_end_through_analysis_runner():
    with open(GOLDEN) as f:
        g = json.load(f)["compliance"]
    table = arrow_golden("compliance")
    ctx = (S.AnalysisRunner().add(S.ComplianceAnalyzer("score_check", g["predicate"])).add(S.SizeAnalyzer())
           .add(S.ComplianceAnalyzer("bad", "score > 0 UNION SELECT 1")).add(S.ComplianceAnalyzer("off", "ABS(score) > 1")).run(table))
    assert ctx.states["compliance"] == {"compliant_count": g["compliant_count"], "total_count": g["total_count"]}
    assert ctx.metrics["compliance"] == {"type": "Double", "value": g["compliant_count"] / g["total_count"]}
    assert ctx.metrics["size"] == {"type": "Long", "value": g["total_count"]}
    errors = ctx.errors()
    assert len(errors) == 2 and all(e["analyzer_name"] == "compliance" for e in errors)
    assert "Predicate contains forbidden keyword: union" in errors[0]["error"]
    assert "not on the GPU path: a function call (ABS(..))" in errors[1]["error"]
