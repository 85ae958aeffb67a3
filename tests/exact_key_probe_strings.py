"""Exact reference for a TGX_CHECK_KEY_PROBE spec on STRING keys (Plan.set_key_probe_strings) and the verdict
ForeignKeyConstraint derives from it (TG/constraints/foreign_key.rs:152-176, 334-410): a plain walk over Python `bytes`
with a set and a dict.  Nothing here looks at the library, and no fingerprint is involved: the walk compares the values
themselves, which is what the library's counts are exact over unless two values share all 128 bits of a keyed
fingerprint.  (The one exception is `parent_digest`, the set's identity: that is DEFINED over fingerprints, and is
restated here with tests/fp_reference.py.)  `walk_np` is a numpy twin of the walk over a column given as (codes, words,
mask), the form tests/fuzz_plans.py keeps its string columns in.

A table side is a list whose items are `bytes` (or str, taken as UTF-8) or None for a NULL row.  The SQL is a LEFT JOIN on
child.c = parent.p filtered to parent.p IS NULL: a NULL child row matches nothing (it is a violation unless allow_nulls)
and a NULL parent row is no key of the set.  The walk gives what the library's state holds,

    seen, non_null, null_rows, matched, missing_rows, counted, overflow_rows (always 0 here: the walk has no table),
    long_rows, missing_keys, parent_keys, entries (missing key -> rows, ascending bytewise)

with seen == non_null + null_rows, non_null == matched + missing_rows, missing_rows == counted + overflow_rows +
long_rows.  long_rows are the MISSING rows whose value is longer than max_value_bytes: they are counted, their keys are
not kept.  A long value that is in the parent is matched like any other."""


def as_bytes(values):
    return [None if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in values]


def walk(child, parent, max_value_bytes=256, max_missing_keys=10000):
    keys = set(v for v in as_bytes(parent) if v is not None)
    seen = non_null = matched = long_rows = 0
    entries = {}
    for v in as_bytes(child):
        seen += 1
        if v is None:
            continue
        non_null += 1
        if v in keys:
            matched += 1
        elif len(v) > max_value_bytes:
            long_rows += 1
        else:
            entries[v] = entries.get(v, 0) + 1
    entries = dict(sorted(entries.items()))  # (bytes compare as unsigned bytes, a prefix first)
    counted = sum(entries.values())
    return {"seen": seen, "non_null": non_null, "null_rows": seen - non_null, "matched": matched,
            "missing_rows": counted + long_rows, "counted": counted, "overflow_rows": 0, "long_rows": long_rows,
            "missing_keys": len(entries), "parent_keys": len(keys), "entries": entries,
            "within_bound": len(entries) <= max_missing_keys}


def walk_np(codes, words, mask, parent, max_value_bytes=256, max_missing_keys=10000):
    """the walk's state for the column whose row i holds words[codes[i]] (bytes; the words are distinct) where mask[i],
    a NULL otherwise; `parent` as for walk"""
    import numpy as np

    codes, mask = np.asarray(codes, np.int64), np.asarray(mask, bool)
    keys = set(v for v in as_bytes(parent) if v is not None)
    per_word = np.bincount(codes[mask], minlength=len(words))
    in_set = np.array([w in keys for w in words] + [False], bool)[:-1]
    too_long = np.array([len(w) > max_value_bytes for w in words] + [False], bool)[:-1] & ~in_set
    kept = ~in_set & ~too_long & (per_word > 0)
    entries = {words[k]: int(per_word[k]) for k in sorted(np.flatnonzero(kept).tolist(), key=words.__getitem__)}
    counted, long_rows = int(per_word[kept].sum()), int(per_word[too_long].sum())
    non_null = int(mask.sum())
    return {"seen": len(codes), "non_null": non_null, "null_rows": len(codes) - non_null,
            "matched": int(per_word[in_set].sum()), "missing_rows": counted + long_rows, "counted": counted,
            "overflow_rows": 0, "long_rows": long_rows, "missing_keys": len(entries), "parent_keys": len(keys),
            "entries": entries, "within_bound": len(entries) <= max_missing_keys}


def parent_digest(key, parent):
    """the identity of a set of string keys under the 16-byte fingerprint key `key` (include/tgx.h): the wrapping sum
    over the DISTINCT fingerprints (fa, fb) of mix64(mix64(fa ^ salt) ^ fb)"""
    import exact_key_probe as kp
    import fp_reference as fpr

    fps = set(fpr.fingerprint(key, v) for v in as_bytes(parent) if v is not None)
    return sum(kp.mix64(kp.mix64(fa ^ kp.DIGEST_SALT) ^ fb) for fa, fb in fps) & kp.M64


def verdict(state, child, parent, allow_nulls=False, max_violations_reported=100, examples=True):
    """(status, metric, message) from a walk's state.  child / parent: the qualified column names.  The examples are the
    max_violations_reported bytewise-smallest missing keys, printed raw and joined by ", "; the message lists up to 5 of
    them.  `examples`: the child column is Utf8, the one string type the reference's collector downcasts (:265-291)"""
    total = state["missing_rows"] + (0 if allow_nulls else state["null_rows"])
    if total == 0:
        return "success", None, None
    partial = state["overflow_rows"] or state["long_rows"]
    unique = ("at least %d" % state["missing_keys"]) if partial else "%d" % state["missing_keys"]
    msg = "Foreign key constraint violation: %d values in '%s' do not exist in '%s' (total: %d, unique: %s)" % (
        total, child, parent, total, unique)
    shown = [k.decode() for k in sorted(state["entries"])[:max_violations_reported]] if examples else []
    if shown:
        msg += ". Examples: [%s]" % (", ".join(shown) if len(shown) <= 5 else
                                     "%s, ... (%d more)" % (", ".join(shown[:5]), len(shown) - 5))
    return "failure", float(total), msg
