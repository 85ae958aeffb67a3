"""The exact reference of TGX_CHECK_ROW_PREDICATE: neither the library nor its compiler.

A predicate is an expression tree of nested tuples, walked row by row; UNKNOWN is None.  Comparisons are done on Python
ints and on IEEE totalOrder keys taken from a double's bits -- the contract of include/tgx.h:

    ("isnull", col)                      never UNKNOWN
    ("cmp", col, op, literal)            op one of "=", "<", "<=", ">", ">="; an int literal is an integer literal, a float
                                         literal one written with a point or exponent; UNKNOWN when col is NULL
    ("cmpcol", col1, op, col2)           UNKNOWN when either side is NULL; two string columns: "=" only
    ("streq", col, bytes)                UNKNOWN when col is NULL
    ("and", a, b)  ("or", a, b)  ("not", a)     Kleene's logic

and SQL's own definitions of the rest, as helpers that build such trees: ne, between, isin.

A row is {column: None | int | float | bytes}; `types` is {column: "int" | "float" | "str"} (a NULL tells no type).

run_compiled() is a postfix interpreter for the JSON tgx_host_row_predicate_json returns: the compiler's output is held
against a hand-written tree by running both on the same rows."""
import struct

T, F, U = True, False, None
OPS = ("=", "<", "<=", ">", ">=")
# include/tgx.h
IS_NULL, CMP_LITERAL, CMP_COLUMNS, STR_EQ = 1, 2, 3, 4
EQ, LT, LE, GT, GE = 1, 2, 3, 4, 5
LITERAL_IS_DOUBLE = 1
PUSH, AND, OR, NOT = 1, 2, 3, 4
OP_OF = {EQ: "=", LT: "<", LE: "<=", GT: ">", GE: ">="}


def bits_of(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b & ((1 << 64) - 1)))[0]


def key(x):
    """the totalOrder key of a double: -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN"""
    b = bits_of(x)
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)


def as_double(v):
    """CAST(int64 AS DOUBLE): round to nearest, ties to even (what Python's int -> float does)"""
    return float(v)


def k_not(a):
    return None if a is None else not a


def k_and(a, b):
    if a is False or b is False:
        return False
    if a is None or b is None:
        return None
    return True


def k_or(a, b):
    if a is True or b is True:
        return True
    if a is None or b is None:
        return None
    return False


def compare(op, a, b):
    return {"=": a == b, "<": a < b, "<=": a <= b, ">": a > b, ">=": a >= b}[op]


def cmp_literal(value, col_type, op, literal):
    if value is None:
        return None
    if col_type == "str":
        raise TypeError("a numeric leaf on a string column")
    if col_type == "int" and isinstance(literal, int):
        return compare(op, value, literal)
    x = as_double(value) if col_type == "int" else value
    return compare(op, key(x), key(float(literal)))


def cmp_columns(a, a_type, op, b, b_type):
    if a is None or b is None:
        return None
    if a_type == "str" or b_type == "str":
        if a_type != b_type or op != "=":
            raise TypeError("strings compare with strings, by = only")
        return bytes(a) == bytes(b)
    if a_type == "int" and b_type == "int":
        return compare(op, a, b)
    xa = as_double(a) if a_type == "int" else a
    xb = as_double(b) if b_type == "int" else b
    return compare(op, key(xa), key(xb))


def str_eq(value, col_type, literal):
    if value is None:
        return None
    if col_type != "str":
        raise TypeError("a string leaf on a numeric column")
    return bytes(value) == bytes(literal)


def walk(tree, row, types):
    """the tree's value on one row: True, False or None"""
    head = tree[0]
    if head == "and":
        return k_and(walk(tree[1], row, types), walk(tree[2], row, types))
    if head == "or":
        return k_or(walk(tree[1], row, types), walk(tree[2], row, types))
    if head == "not":
        return k_not(walk(tree[1], row, types))
    if head == "isnull":
        return row[tree[1]] is None
    if head == "cmp":
        return cmp_literal(row[tree[1]], types[tree[1]], tree[2], tree[3])
    if head == "cmpcol":
        return cmp_columns(row[tree[1]], types[tree[1]], tree[2], row[tree[3]], types[tree[3]])
    if head == "streq":
        return str_eq(row[tree[1]], types[tree[1]], tree[2])
    raise ValueError("unknown node %r" % (head,))


# ---- SQL's definitions of what is no leaf ---------------------------------------------------------------------------------
def ne(col, literal):
    return ("not", eq(col, literal))


def eq(col, literal):
    return ("streq", col, literal) if isinstance(literal, (bytes, bytearray)) else ("cmp", col, "=", literal)


def between(col, lo, hi):
    return ("and", ("cmp", col, ">=", lo), ("cmp", col, "<=", hi))


def isin(col, literals):
    tree = eq(col, literals[0])
    for lit in literals[1:]:
        tree = ("or", tree, eq(col, lit))
    return tree


def any_of(*trees):
    out = trees[0]
    for t in trees[1:]:
        out = ("or", out, t)
    return out


def all_of(*trees):
    out = trees[0]
    for t in trees[1:]:
        out = ("and", out, t)
    return out


def counts(tree, rows, types):
    """(seen, satisfied, unknown, failed) of the tree over the rows: tgx_row_predicate_get's answer"""
    sat = unk = 0
    n = 0
    for row in rows:
        v = walk(tree, row, types)
        sat += v is True
        unk += v is None
        n += 1
    return n, sat, unk, n - sat - unk


def table_rows(columns):
    """{column: list of values} -> the rows as dicts"""
    names = list(columns)
    n = len(columns[names[0]]) if names else 0
    return [{c: columns[c][i] for c in names} for i in range(n)]


# ---- the compiler's JSON, interpreted ----------------------------------------------------------------------------------
def run_leaf(leaf, pool, columns, row, types):
    col = columns[leaf["col"]]
    if leaf["kind"] == IS_NULL:
        return row[col] is None
    if leaf["kind"] == CMP_LITERAL:
        literal = from_bits(leaf["lit_f_bits"]) if leaf["flags"] & LITERAL_IS_DOUBLE else leaf["lit_i"]
        return cmp_literal(row[col], types[col], OP_OF[leaf["op"]], literal)
    if leaf["kind"] == CMP_COLUMNS:
        col2 = columns[leaf["col2"]]
        return cmp_columns(row[col], types[col], OP_OF[leaf["op"]], row[col2], types[col2])
    if leaf["kind"] == STR_EQ:
        return str_eq(row[col], types[col], pool[leaf["lit_offset"]:leaf["lit_offset"] + leaf["lit_len"]])
    raise ValueError("unknown leaf kind %r" % (leaf["kind"],))


def run_compiled(compiled, row, types):
    """the postfix program of a compiled predicate (tgx_host_row_predicate_json's dict) on one row"""
    pool = bytes.fromhex(compiled["literals_hex"])
    stack = []
    for code, arg in compiled["program"]:
        if code == PUSH:
            stack.append(run_leaf(compiled["leaves"][arg], pool, compiled["columns"], row, types))
        elif code == NOT:
            stack.append(k_not(stack.pop()))
        elif code in (AND, OR):
            b, a = stack.pop(), stack.pop()
            stack.append(k_and(a, b) if code == AND else k_or(a, b))
        else:
            raise ValueError("unknown op %r" % (code,))
        assert len(stack) <= 32
    assert len(stack) == 1
    return stack[0]


def leaves_and_program(tree, columns):
    """a tree as the C ABI takes it: (leaf dicts, [(code, arg)], literal pool), columns named by position in `columns`.
    A straight post-order walk, one leaf per leaf node: the tests' own lowering, independent of the library's compiler"""
    leaves, program, pool = [], [], bytearray()

    def emit(t):
        head = t[0]
        if head in ("and", "or"):
            emit(t[1])
            emit(t[2])
            program.append((AND if head == "and" else OR, 0))
        elif head == "not":
            emit(t[1])
            program.append((NOT, 0))
        else:
            if head == "isnull":
                leaf = dict(kind=IS_NULL, col=columns.index(t[1]))
            elif head == "cmp":
                lit = t[3]
                leaf = dict(kind=CMP_LITERAL, op=OPS.index(t[2]) + 1, col=columns.index(t[1]))
                if isinstance(lit, int):
                    leaf.update(lit_i=lit, lit_f=float(lit))
                else:
                    leaf.update(flags=LITERAL_IS_DOUBLE, lit_f=lit)
            elif head == "cmpcol":
                leaf = dict(kind=CMP_COLUMNS, op=OPS.index(t[2]) + 1, col=columns.index(t[1]), col2=columns.index(t[3]))
            else:
                leaf = dict(kind=STR_EQ, col=columns.index(t[1]), lit_offset=len(pool), lit_len=len(t[2]))
                pool.extend(t[2])
            leaves.append(leaf)
            program.append((PUSH, len(leaves) - 1))

    emit(tree)
    return leaves, program, bytes(pool)
