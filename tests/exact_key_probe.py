"""Exact reference for TGX_CHECK_KEY_PROBE and the verdict ForeignKeyConstraint derives from it
(TG/constraints/foreign_key.rs:152-176, 334-410): a plain walk with Python sets and dicts, and a numpy twin of it.
Nothing here looks at the library.

A table side is (values, mask): integer values and a bool array (True: the row is non-NULL; None: every row is).  The
SQL is a LEFT JOIN on child.c = parent.p filtered to parent.p IS NULL: a NULL child row matches nothing (it is a
violation unless allow_nulls), and a NULL parent row matches nothing either, so it is not a key of the set.  The walk
gives what the library's state holds,

    seen, non_null, null_rows, matched, missing_rows, counted, overflow_rows (always 0 here: the walk has no table),
    missing_keys, parent_keys, parent_digest, route, entries (missing key -> rows, ascending)

with seen == non_null + null_rows, non_null == matched + missing_rows, missing_rows == counted + overflow_rows.
max_missing_keys is the library's bound: the walk keeps every key and says in `within_bound` whether they fit it."""
import numpy as np

M64 = (1 << 64) - 1
DIGEST_SALT = 0x9E3779B97F4A7C15
ROUTE_EMPTY, ROUTE_BITMAP, ROUTE_HASH = 0, 1, 2


# ---- the digest -----------------------------------------------------------------------------------------------------------
def mix64(x):
    """the splitmix64 finaliser on a Python int, modulo 2^64"""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def mix64_np(x):
    x = np.asarray(x).astype(np.uint64)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return x


def digest(keys):
    """the wrapping 64-bit sum of mix64(key ^ salt) over the DISTINCT keys (ints in int64 range)"""
    return sum(mix64((int(k) & M64) ^ DIGEST_SALT) for k in set(int(k) for k in keys)) & M64


def digest_np(keys):
    uniq = np.unique(np.asarray(keys, np.int64))
    with np.errstate(over="ignore"):
        return int(mix64_np(uniq.view(np.uint64) ^ np.uint64(DIGEST_SALT)).sum(dtype=np.uint64))


# ---- the route rule -------------------------------------------------------------------------------------------------------
def route_of(keys, n_records=None):
    """keys: the records' keys (duplicates allowed); n_records defaults to their number.  Empty: 0.  A bitmap over
    [min, max] when range = max - min + 1, in unsigned 64-bit arithmetic, is not 0 and <= 128 * n_records; else a hash
    table"""
    keys = [int(k) for k in keys]
    n = len(keys) if n_records is None else n_records
    if n == 0:
        return ROUTE_EMPTY
    rng = (max(keys) - min(keys) + 1) & M64
    return ROUTE_BITMAP if rng != 0 and rng <= 128 * n else ROUTE_HASH


def hash_slots(n_records):
    """slots of the hash route's table: the smallest power of two >= 2 * n_records"""
    s = 2
    while s < 2 * n_records:
        s <<= 1
    return s


# ---- the walk -------------------------------------------------------------------------------------------------------------
def summary(seen, non_null, matched, entries, parent, max_missing_keys, n_records=None):
    entries = dict(sorted(entries.items()))
    counted = sum(entries.values())
    return {"seen": seen, "non_null": non_null, "null_rows": seen - non_null, "matched": matched,
            "missing_rows": counted, "counted": counted, "overflow_rows": 0, "missing_keys": len(entries),
            "parent_keys": len(set(parent)), "parent_digest": digest(parent), "route": route_of(parent, n_records),
            "entries": entries, "within_bound": len(entries) <= max_missing_keys}


def walk(child, child_mask, parent, parent_mask, max_missing_keys=10000, n_records=None):
    """n_records: the records the set is built from when that is not one per non-NULL parent row (a DISTINCT export
    hands out one per distinct key)"""
    keys = [int(p) for i, p in enumerate(parent) if parent_mask is None or parent_mask[i]]
    key_set = set(keys)
    seen = non_null = matched = 0
    entries = {}
    for i, c in enumerate(child):
        seen += 1
        if child_mask is not None and not child_mask[i]:
            continue
        non_null += 1
        if int(c) in key_set:
            matched += 1
        else:
            entries[int(c)] = entries.get(int(c), 0) + 1
    return summary(seen, non_null, matched, entries, keys, max_missing_keys, n_records)


def walk_np(child, child_mask, parent, parent_mask, max_missing_keys=10000, n_records=None):
    child = np.asarray(child).astype(np.int64)
    parent = np.asarray(parent).astype(np.int64)
    cm = np.ones(len(child), bool) if child_mask is None else np.asarray(child_mask, bool)
    pm = np.ones(len(parent), bool) if parent_mask is None else np.asarray(parent_mask, bool)
    keys = parent[pm]
    kept = child[cm]
    hit = np.isin(kept, keys)
    uniq, n = np.unique(kept[~hit], return_counts=True)
    uk = np.unique(keys)
    if n_records is None:
        n_records = len(keys)
    route = ROUTE_EMPTY
    if n_records:
        rng = (int(uk[-1]) - int(uk[0]) + 1) & M64
        route = ROUTE_BITMAP if rng != 0 and rng <= 128 * n_records else ROUTE_HASH
    counted = int(n.sum())
    return {"seen": len(child), "non_null": int(cm.sum()), "null_rows": int((~cm).sum()), "matched": int(hit.sum()),
            "missing_rows": counted, "counted": counted, "overflow_rows": 0, "missing_keys": len(uniq),
            "parent_keys": len(uk), "parent_digest": digest_np(keys), "route": route,
            "entries": {int(u): int(c) for u, c in zip(uniq, n)}, "within_bound": len(uniq) <= max_missing_keys}


# ---- the verdict (foreign_key.rs:334-410) -----------------------------------------------------------------------------------
def verdict(state, child, parent, allow_nulls=False, max_violations_reported=100, examples=True):
    """(status, metric, message) from a walk's state.  child / parent: the qualified column names.  The examples are the
    max_violations_reported smallest missing keys (a NULL takes no slot); the message lists up to 5 of them.  `examples`:
    the child column is of a type the reference's collector downcasts (Int64, Int32)"""
    total = state["missing_rows"] + (0 if allow_nulls else state["null_rows"])
    if total == 0:
        return "success", None, None
    unique = ("at least %d" % state["missing_keys"]) if state["overflow_rows"] else "%d" % state["missing_keys"]
    msg = "Foreign key constraint violation: %d values in '%s' do not exist in '%s' (total: %d, unique: %s)" % (
        total, child, parent, total, unique)
    shown = [str(k) for k in sorted(state["entries"])[:max_violations_reported]] if examples else []
    if shown:
        msg += ". Examples: [%s]" % (", ".join(shown) if len(shown) <= 5 else
                                     "%s, ... (%d more)" % (", ".join(shown[:5]), len(shown) - 5))
    return "failure", float(total), msg
