"""GROUP BY several columns, exactly: what a TGX_CHECK_GROUP_COUNTS / TGX_CHECK_GROUP_SUMS spec with a column list answers
when nothing overflows -- the canonical bytes of a tuple key (include/tgx.h), written here a second time and on its own,
and the summary and entries of a tuple task as a plain walk on exact_group_counts.group_by / exact_group_sums.group_by,
with a numpy twin for integer tuples.

A key is its components one behind the other: NULL 0x00; an integer 0x01 and the 8 big-endian bytes of value ^ 2^63; a
string 0x02, its length as 2 big-endian bytes and its bytes.  NULL is a value: there is no NULL group."""
import numpy as np

import exact_group_counts as exc
import exact_group_sums as exs


def encoded_length(cells):
    """in unbounded integers: a string of 65 536 bytes or more has a length although it has no form"""
    return sum(1 if c is None else 3 + len(c) if isinstance(c, bytes) else 9 for c in cells)


def encode(cells):
    out = b""
    for c in cells:
        if c is None:
            out += b"\x00"
        elif isinstance(c, bytes):
            assert len(c) < 65536
            out += b"\x02" + len(c).to_bytes(2, "big") + c
        else:
            assert -2**63 <= c < 2**63
            out += b"\x01" + ((c + 2**63) % 2**64).to_bytes(8, "big")
    return out


def decode(key):
    cells, at = [], 0
    while at < len(key):
        tag = key[at]
        if tag == 0:
            cells.append(None)
            at += 1
        elif tag == 1:
            assert at + 9 <= len(key)
            cells.append(int.from_bytes(key[at + 1:at + 9], "big") - 2**63)
            at += 9
        else:
            assert tag == 2 and at + 3 <= len(key)
            n = int.from_bytes(key[at + 1:at + 3], "big")
            assert at + 3 + n <= len(key)
            cells.append(key[at + 3:at + 3 + n])
            at += 3 + n
    return tuple(cells)


def component_order(cells):
    """the stated order of keys of one arity: lexicographic by component, NULL before integers before strings, integers
    numerically, strings by length and then bytewise (the length stands in front of the bytes)"""
    return tuple((0, 0, b"") if c is None else (2, len(c), c) if isinstance(c, bytes) else (1, c, b"") for c in cells)


def walk(values, group_columns, max_value_bytes=256):
    """tgx_group_counts_summary's ten counters and `entries`, encoded key -> (total, non_null) ascending by key, for
    one value column (a list; None = NULL) and the group columns (lists of None / int / bytes)"""
    s = dict(seen=len(values), groups=0, counted=0, counted_non_null=0, null_group_rows=0, null_group_non_null=0,
             overflow_rows=0, overflow_non_null=0, long_rows=0, long_non_null=0)
    entries = {}
    for key, (total, non_null) in exc.group_by(values, *group_columns).items():
        if encoded_length(key) > max_value_bytes:
            s["long_rows"] += total
            s["long_non_null"] += non_null
        else:
            entries[encode(key)] = (total, non_null)
            s["counted"] += total
            s["counted_non_null"] += non_null
    s["entries"] = {k: entries[k] for k in sorted(entries)}
    s["groups"] = len(entries)
    return s


def _unique_rows(key_columns, key_valids):
    """the distinct integer tuples of the rows: (tuples as lists of cells, inverse)"""
    n = len(key_columns[0])
    cols = []
    for k, v in zip(key_columns, key_valids):
        v = np.ones(n, bool) if v is None else np.asarray(v, bool)
        cols += [v.astype(np.int64), np.where(v, np.asarray(k, np.int64), 0)]
    table = np.stack(cols, axis=1) if n else np.zeros((0, len(cols)), np.int64)
    uniq, inverse = np.unique(table, axis=0, return_inverse=True)
    tuples = [tuple(int(row[2 * c + 1]) if row[2 * c] else None for c in range(len(key_columns))) for row in uniq]
    return tuples, np.asarray(inverse).reshape(-1)


def walk_np(valid, key_columns, key_valids=None, max_value_bytes=256):
    """walk() for integer tuples over arrays: `valid` the value column's non-NULL mask, `key_columns` int64 arrays,
    `key_valids` their masks (None: no NULLs)"""
    valid = np.asarray(valid, bool)
    key_valids = key_valids or [None] * len(key_columns)
    tuples, inverse = _unique_rows(key_columns, key_valids)
    totals = np.bincount(inverse, minlength=len(tuples))
    non_null = np.bincount(inverse, weights=valid, minlength=len(tuples)).astype(np.int64)
    s = dict(seen=len(valid), groups=0, counted=0, counted_non_null=0, null_group_rows=0, null_group_non_null=0,
             overflow_rows=0, overflow_non_null=0, long_rows=0, long_non_null=0)
    entries = {}
    for key, t, nn in zip(tuples, totals.tolist(), non_null.tolist()):
        if encoded_length(key) > max_value_bytes:
            s["long_rows"] += t
            s["long_non_null"] += nn
        else:
            entries[encode(key)] = (t, nn)
            s["counted"] += t
            s["counted_non_null"] += nn
    s["entries"] = {k: entries[k] for k in sorted(entries)}
    s["groups"] = len(entries)
    return s


def walk_sums(values, group_columns, max_value_bytes=256, is_float=False):
    """exact_group_sums.walk for a tuple task: seen, groups, is_float, the four classes and `entries`, encoded key ->
    class ascending by key.  A class is (rows, non_null, wrapping sum) for integers and (rows, non_null, fsum, sum of
    magnitudes) for floats, where `counted` is (rows, non_null) alone"""
    cls = exs.float_class if is_float else exs.int_class
    nothing = cls(0, [])
    s = dict(seen=len(values), is_float=bool(is_float) and len(values) > 0, null_group=nothing, overflow=nothing)
    entries, longs = {}, [0, []]
    for key, (rows, vals) in exs.group_by(values, list(zip(*group_columns))).items():
        if encoded_length(key) > max_value_bytes:
            longs[0] += rows
            longs[1] += vals
        else:
            entries[encode(key)] = cls(rows, vals)
    s["long_rows"] = cls(*longs)
    s["entries"] = {k: entries[k] for k in sorted(entries)}
    s["groups"] = len(entries)
    s["counted"] = (sum(e[0] for e in entries.values()), sum(e[1] for e in entries.values()))
    if not is_float:
        s["counted"] += (exs.wrap(sum(e[2] for e in entries.values())),)
    return s


def walk_sums_np(values, valid, key_columns, key_valids=None, max_value_bytes=256):
    """walk_sums for INTEGER values and integer tuples over arrays (sums wrap in uint64)"""
    values, valid = np.asarray(values, np.int64), np.asarray(valid, bool)
    key_valids = key_valids or [None] * len(key_columns)
    tuples, inverse = _unique_rows(key_columns, key_valids)
    rows = np.bincount(inverse, minlength=len(tuples))
    non_null = np.bincount(inverse, weights=valid, minlength=len(tuples)).astype(np.int64)
    sums = np.zeros(len(tuples), np.uint64)
    np.add.at(sums, inverse, np.where(valid, values, 0).view(np.uint64))
    nothing = exs.int_class(0, [])
    s = dict(seen=len(values), is_float=False, null_group=nothing, overflow=nothing)
    entries, longs = {}, [0, 0, 0]
    for key, r, nn, t in zip(tuples, rows.tolist(), non_null.tolist(), sums.tolist()):
        if encoded_length(key) > max_value_bytes:
            longs = [longs[0] + r, longs[1] + nn, longs[2] + t]
        else:
            entries[encode(key)] = (r, nn, exs.wrap(t))
    s["long_rows"] = (longs[0], longs[1], exs.wrap(longs[2]))
    s["entries"] = {k: entries[k] for k in sorted(entries)}
    s["groups"] = len(entries)
    s["counted"] = (sum(e[0] for e in entries.values()), sum(e[1] for e in entries.values()),
                    exs.wrap(sum(e[2] for e in entries.values())))
    return s
