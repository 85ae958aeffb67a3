"""The exact reference of the string leaves of TGX_CHECK_ROW_PREDICATE (STR_CMP, STR_LENGTH, STR_LIKE, STR_BLANK):
neither the library nor its compiler.  Plain Python over `bytes`, the contract of include/tgx.h restated:

    ("strcmp", col, op, bytes)          op one of "<", "<=", ">", ">=": bytewise lexicographic, a proper prefix is smaller
    ("strlen", col, op, int, in_bytes)  the bytes that are not 10xxxxxx (in_bytes: all the bytes) against the int
    ("like", col, bytes)                LIKE without escapes: % any run of bytes, _ exactly one unit
    ("blank", col)                      every byte is 0x20, the empty value included

Each is UNKNOWN (None) on a NULL row.  Kleene's logic, the other leaves and the trees are exact_row_predicate's.

LIKE is a recursive matcher over UNITS, deliberately not the kernel's two-pointer walk: a unit is one byte that is not
10xxxxxx plus all 10xxxxxx bytes directly behind it, and at offset 0 the first byte opens a unit whatever it is.  A `%`
may end anywhere, a `_` takes one whole unit from that unit's first byte, any other byte takes itself.

seeded_patterns() / seeded_values() are the shared generator: about 200 patterns and 2000 values over a small alphabet,
so that matches are common (test_exact_string_predicates.py asserts the census)."""
import functools
import random

import exact_row_predicate as ex

STR_CMP, STR_LENGTH, STR_LIKE, STR_BLANK = 6, 7, 8, 9
LENGTH_IN_BYTES = 2
KIND_OF = {"strcmp": STR_CMP, "strlen": STR_LENGTH, "like": STR_LIKE, "blank": STR_BLANK}


def is_continuation(b):
    return (b & 0xC0) == 0x80


def characters(value):
    return sum(1 for b in value if not is_continuation(b))


def unit_end(value, start):
    """the end of the unit that byte `start` opens"""
    end = start + 1
    while end < len(value) and is_continuation(value[end]):
        end += 1
    return end


def like(value, pattern):
    value, pattern = bytes(value), bytes(pattern)
    n, m = len(value), len(pattern)

    @functools.lru_cache(maxsize=None)
    def match(p, t):
        if p == m:
            return t == n
        c = pattern[p]
        if c == 0x25:  # %
            if p + 1 == m:
                return True
            return any(match(p + 1, u) for u in range(t, n + 1))
        if t >= n:
            return False
        if c == 0x5F:  # _
            if t != 0 and is_continuation(value[t]):
                return False  # (no unit starts here)
            return match(p + 1, unit_end(value, t))
        return value[t] == c and match(p + 1, t + 1)

    return match(0, 0)


def blank(value):
    return all(b == 0x20 for b in value)


def _string(value, col_type):
    if col_type != "str":
        raise TypeError("a string leaf on a numeric column")
    return bytes(value)


def leaf(tree, row, types):
    """one of the four leaves on one row"""
    head, col = tree[0], tree[1]
    if row[col] is None:
        return None
    v = _string(row[col], types[col])
    if head == "strcmp":
        assert tree[2] in ("<", "<=", ">", ">=")
        return ex.compare(tree[2], v, bytes(tree[3]))  # (Python orders bytes as the contract does)
    if head == "strlen":
        return ex.compare(tree[2], len(v) if tree[4] else characters(v), tree[3])
    if head == "like":
        assert 0x5C not in bytes(tree[2])
        return like(v, tree[2])
    if head == "blank":
        return blank(v)
    raise ValueError("unknown node %r" % (head,))


def walk(tree, row, types):
    head = tree[0]
    if head == "and":
        return ex.k_and(walk(tree[1], row, types), walk(tree[2], row, types))
    if head == "or":
        return ex.k_or(walk(tree[1], row, types), walk(tree[2], row, types))
    if head == "not":
        return ex.k_not(walk(tree[1], row, types))
    if head in KIND_OF:
        return leaf(tree, row, types)
    return ex.walk(tree, row, types)


def counts(tree, rows, types):
    """(seen, satisfied, unknown, failed) of the tree over the rows: tgx_row_predicate_get's answer"""
    sat = unk = n = 0
    for row in rows:
        v = walk(tree, row, types)
        sat += v is True
        unk += v is None
        n += 1
    return n, sat, unk, n - sat - unk


# ---- SQL's definitions of what is no leaf -------------------------------------------------------------------------------
def str_between(col, lo, hi):
    return ("and", ("strcmp", col, ">=", lo), ("strcmp", col, "<=", hi))


def len_between(col, lo, hi, in_bytes=False):
    return ("and", ("strlen", col, ">=", lo, in_bytes), ("strlen", col, "<=", hi, in_bytes))


# ---- the compiler's JSON, interpreted -----------------------------------------------------------------------------------
def run_leaf(lf, pool, columns, row, types):
    col = columns[lf["col"]]
    lit = pool[lf["lit_offset"]:lf["lit_offset"] + lf["lit_len"]]
    if lf["kind"] == STR_CMP:
        return leaf(("strcmp", col, ex.OP_OF[lf["op"]], lit), row, types)
    if lf["kind"] == STR_LENGTH:
        return leaf(("strlen", col, ex.OP_OF[lf["op"]], lf["lit_i"], bool(lf["flags"] & LENGTH_IN_BYTES)), row, types)
    if lf["kind"] == STR_LIKE:
        return leaf(("like", col, lit), row, types)
    if lf["kind"] == STR_BLANK:
        return leaf(("blank", col), row, types)
    return ex.run_leaf(lf, pool, columns, row, types)


def run_compiled(compiled, row, types):
    """exact_row_predicate.run_compiled with the four kinds: the postfix program of a compiled predicate on one row"""
    pool = bytes.fromhex(compiled["literals_hex"])
    stack = []
    for code, arg in compiled["program"]:
        if code == ex.PUSH:
            stack.append(run_leaf(compiled["leaves"][arg], pool, compiled["columns"], row, types))
        elif code == ex.NOT:
            stack.append(ex.k_not(stack.pop()))
        elif code in (ex.AND, ex.OR):
            b, a = stack.pop(), stack.pop()
            stack.append(ex.k_and(a, b) if code == ex.AND else ex.k_or(a, b))
        else:
            raise ValueError("unknown op %r" % (code,))
        assert len(stack) <= 32
    assert len(stack) == 1
    return stack[0]


def leaves_and_program(tree, columns):
    """a tree as the C ABI takes it: (leaf dicts, [(code, arg)], literal pool) -- exact_row_predicate's lowering with the
    four kinds; the pool is filled in the order of the leaves"""
    leaves, program, pool = [], [], bytearray()

    def emit(t):
        head = t[0]
        if head in ("and", "or"):
            emit(t[1])
            emit(t[2])
            program.append((ex.AND if head == "and" else ex.OR, 0))
        elif head == "not":
            emit(t[1])
            program.append((ex.NOT, 0))
        else:
            if head == "strcmp":
                lf = dict(kind=STR_CMP, op=ex.OPS.index(t[2]) + 1, col=columns.index(t[1]), lit_offset=len(pool), lit_len=len(t[3]))
                pool.extend(t[3])
            elif head == "strlen":
                lf = dict(kind=STR_LENGTH, op=ex.OPS.index(t[2]) + 1, col=columns.index(t[1]), lit_i=t[3],
                          flags=LENGTH_IN_BYTES if t[4] else 0)
            elif head == "like":
                lf = dict(kind=STR_LIKE, col=columns.index(t[1]), lit_offset=len(pool), lit_len=len(t[2]))
                pool.extend(t[2])
            elif head == "blank":
                lf = dict(kind=STR_BLANK, col=columns.index(t[1]))
            else:
                sub, _, sub_pool = ex.leaves_and_program(t, columns)
                lf = dict(sub[0])
                if lf["kind"] == ex.STR_EQ:
                    lf["lit_offset"] = len(pool)
                    pool.extend(sub_pool)
            leaves.append(lf)
            program.append((ex.PUSH, len(leaves) - 1))

    emit(tree)
    return leaves, program, bytes(pool)


# ---- the seeded set -----------------------------------------------------------------------------------------------------
ALPHABET = ("a", "b", "é", "日", " ", "\n")


def seeded_values(n=2000, seed=20261021):
    """n values (bytes, valid UTF-8) of 0 .. 6 characters over ALPHABET; short, so that a pattern often matches"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.choice((0, 1, 1, 2, 2, 3, 3, 4, 5, 6))
        weights = (5, 3, 2, 2, 2, 1)
        out.append("".join(rng.choices(ALPHABET, weights, k=k)).encode("utf-8"))
    return out


def seeded_patterns(n=200, seed=1021):
    """n backslash-free patterns (bytes, valid UTF-8): a value of the same distribution in which characters are
    replaced by `_`, runs by `%`, and into which `%`s are inserted -- so the pattern matches that value and its like"""
    rng = random.Random(seed)
    base = seeded_values(n, seed + 1)
    out = []
    for v in base:
        chars = list(v.decode("utf-8"))
        elems = []
        i = 0
        while i < len(chars):
            r = rng.random()
            if r < 0.30:
                elems.append("%")
                i += rng.choice((1, 1, 2, 3))
            elif r < 0.50:
                elems.append("_")
                i += 1
            else:
                elems.append(chars[i])
                i += 1
        if rng.random() < 0.5:
            elems.insert(rng.randrange(len(elems) + 1), "%")
        if rng.random() < 0.25:
            elems.insert(rng.randrange(len(elems) + 1), "%")
        out.append("".join(elems).encode("utf-8"))
    return out
