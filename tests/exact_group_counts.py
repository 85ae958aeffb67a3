"""Grouped completeness, exactly: SELECT g.., COUNT(*) AS total_count, COUNT(col) AS non_null_count FROM t GROUP BY g..
as a plain dictionary walk over Python lists -- any number of group columns, the NULL key a group as in SQL -- with a
numpy twin for big tables, the summary TGX_CHECK_GROUP_COUNTS gives for one group column, and the rules the analyzer
restates from the reference (TG/analyzers/basic/grouped_completeness.rs:160-200, TG/analyzers/grouped.rs:135-156):
order by completeness descending, keep max_groups, NULL keys read as "", the reserved map keys."""
import json

import numpy as np


def group_by(values, *group_columns):
    """{key tuple: [total_count, non_null_count]}; a key's cell is None for a NULL; insertion order = first occurrence"""
    out = {}
    for row, v in enumerate(values):
        key = tuple(g[row] for g in group_columns)
        c = out.setdefault(key, [0, 0])
        c[0] += 1
        c[1] += v is not None
    return out


def walk(values, groups, max_value_bytes=256):
    """what TGX_CHECK_GROUP_COUNTS answers for one value column and one group column when nothing overflows:
    tgx_group_counts_summary's ten counters and `entries`, key -> (total, non_null) ascending by key.  A key is an int or
    bytes; bytes longer than max_value_bytes are long rows"""
    s = dict(seen=len(values), groups=0, counted=0, counted_non_null=0, null_group_rows=0, null_group_non_null=0,
             overflow_rows=0, overflow_non_null=0, long_rows=0, long_non_null=0)
    entries = {}
    for (key,), (total, non_null) in group_by(values, groups).items():
        if key is None:
            s["null_group_rows"], s["null_group_non_null"] = total, non_null
        elif isinstance(key, bytes) and len(key) > max_value_bytes:
            s["long_rows"] += total
            s["long_non_null"] += non_null
        else:
            entries[key] = (total, non_null)
            s["counted"] += total
            s["counted_non_null"] += non_null
    # (ascending by key: integers numerically, bytes bytewise with a prefix first)
    s["entries"] = {k: entries[k] for k in sorted(entries)}
    s["groups"] = len(entries)
    return s


def walk_np(valid, keys, key_valid=None):
    """the numpy twin for integer keys: `valid` the value column's non-NULL mask, `keys` an int64 array, `key_valid` the
    group column's mask (None: no NULL keys)"""
    valid = np.asarray(valid, bool)
    keys = np.asarray(keys, np.int64)
    key_valid = np.ones(len(keys), bool) if key_valid is None else np.asarray(key_valid, bool)
    uniq, inverse = np.unique(keys[key_valid], return_inverse=True)
    totals = np.bincount(inverse, minlength=len(uniq))
    non_null = np.bincount(inverse, weights=valid[key_valid], minlength=len(uniq)).astype(np.int64)
    s = dict(seen=len(keys), groups=len(uniq), counted=int(totals.sum()), counted_non_null=int(non_null.sum()),
             null_group_rows=int((~key_valid).sum()), null_group_non_null=int(valid[~key_valid].sum()),
             overflow_rows=0, overflow_non_null=0, long_rows=0, long_non_null=0)
    s["entries"] = {int(k): (int(t), int(n)) for k, t, n in zip(uniq, totals, non_null)}
    return s


def completeness(total, non_null):
    """CompletenessState::completeness (TG/analyzers/basic/completeness.rs:67-73): an empty state is complete"""
    return 1.0 if total == 0 else non_null / total


def text_of(cell):
    """a key cell as the reference's StringArray::value reads it: a NULL is the empty string"""
    if cell is None:
        return ""
    return cell.decode() if isinstance(cell, bytes) else str(cell)


def grouped_state(groups, group_columns, max_groups=10000, include_overall=True):
    """the analyzer's state from {key tuple: [total, non_null]}: the query's ORDER BY completeness DESC LIMIT
    max_groups + 1 with ties broken by key ascending and NULL cells last, the first max_groups rows kept
    (grouped_completeness.rs:160-200); `overall` sums the kept rows only; total_groups = min(actual, max_groups + 1).
    A later row whose text key equals an earlier one's overwrites it in the map, yet both count"""
    def order(item):
        key, (total, non_null) = item
        return (-completeness(total, non_null), tuple((1, 0) if c is None else (0, c) for c in key))
    rows = sorted(groups.items(), key=order)[:max_groups + 1]
    kept = rows[:max_groups]
    state_groups, overall = {}, [0, 0]
    for key, (total, non_null) in kept:
        state_groups[tuple(text_of(c) for c in key)] = (total, non_null)
        overall[0] += total
        overall[1] += non_null
    included = len(state_groups)
    return {"groups": state_groups, "overall": tuple(overall) if include_overall else None,
            "metadata": {"group_columns": list(group_columns), "total_groups": len(rows), "included_groups": included,
                         "truncated": len(rows) > included, "overflow_strategy": None}}


def metric_map(state):
    """GroupedMetrics::to_metric_value (grouped.rs:135-156): one Double per group under key.join("_"), then
    "__overall__", then "__metadata__" (serde_json of GroupedMetadata): the reserved names overwrite a group of theirs"""
    out = {}
    for key, (total, non_null) in state["groups"].items():
        out["_".join(key)] = completeness(total, non_null)
    if state["overall"] is not None:
        out["__overall__"] = completeness(*state["overall"])
    out["__metadata__"] = json.dumps(state["metadata"], separators=(",", ":"))
    return out
