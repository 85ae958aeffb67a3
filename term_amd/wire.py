"""Wire form of a tgx state (tgx_state_serialize / tgx_state_deserialize), version 3.

The blob is what ranks exchange (one all-gather of a few KiB) and what a checkpoint stores; it is the
counterpart of the serde_json analyzer states of the reference's IncrementalAnalysisRunner
(analyzers/incremental/runner.rs:71-111).  Layout, little-endian, in plan-task order:

    u32 magic 'TGXS', u32 version, u32 n_scan, n_count, n_comoments, n_distinct, n_kll, n_regex, n_hll
    u32 keyed, u8 key[16]      keyed = 1: the blob holds string / tuple keys as fingerprints made under `key`
                               (tgx_plan_set_fingerprint_key); 0: no such keys, key = zeros
    n_scan      x ScanAcc      i64 total, non_null, min_key, max_key; u64 sum_lo; i64 sum_hi; f64 sum, comp;
                               i64 var_n; f64 var_mean, var_m2; i32 is_float, pad                    (96 B)
    n_count     x CountAcc     i64 total, non_null                                                      (16 B)
    n_comoments x ComomentAcc  i64 total, n; f64 s[5]; f64 c[5]; f64 px, py; i32 pivot_set, pad          (120 B)
                               s + c = sums of x', y', x'x', y'y', x'y' with x' = x - px, y' = y - py: about the
                               pivots (px, py); (0, 0) makes them the raw sum_x, sum_y, sum_x2, sum_y2, sum_xy
    n_distinct  x { u32 owner_partitioned, u32 wide_keys; u64 total, non_null, distinct, twice, empty_rows;
                    u64 n_records; records (16 B {key, count} or 32 B {hash_a, hash_b, count, 0}) }
    n_kll       x { u32 k, u32 n_levels; u64 n; f64 min, max; n_levels x { u32 count; f64 items[count] } }
    n_regex     x { u64 total, u64 matches }
    n_hll       x { u32 mode (0 nothing seen, 1 registers, 2 the exact key set answers), u32 has_registers;
                    has_registers x 16384 u8 HyperLogLog registers (rank 0 .. 33) }
    and ONLY for plans with JOINT_BINS checks (blobs of every other plan keep the bytes they had):
    u32 magic 'JNTB', u32 n_joint
    n_joint     x { u32 binned, u32 bins; f64 x_origin, x_width, y_origin, y_width      (the plan's binning; zeros in the
                    i64 total, n, non_finite; f64 x_min, x_max, y_min, y_max              range phase; extremes: +inf / -inf
                    u64 n_words; u64 words[n_words] }                                     when n = 0 and in the count phase)
                               n_words = (bins + 1)^2 + 1 in the count phase: the cells, row-major, then the rows whose
                               index fell outside [0, bins]; 0 in the range phase.  n = the sum of the cells there.
    and ONLY for plans with TEMPORAL checks, behind the JOINT_BINS section if there is one:
    u32 magic 'TMPR', u32 n_temporal
    n_temporal  x { i32 mode, u32 flags; i64 delta, ticks_per_second, lo, hi     (the plan's parameters: tod_lo / tod_hi
                    u64 seen, live, passed }                                      travel as lo / hi; fields of other modes 0)
                               live = rows that are non-NULL (both sides in order mode) and through the weekday filter,
                               passed = those of them that satisfy the predicate: passed <= live <= seen.
    and ONLY for plans with HISTOGRAM checks, behind the TEMPORAL section if there is one:
    u32 magic 'HIST', u32 n_hist
    n_hist      x { u32 counted, u32 buckets; f64 edges[buckets + 1]   (the plan's edges; count phase only)
                    i64 total, n, non_finite; f64 min, max, sum, sum_squared   (extremes +inf / -inf when n = 0 and in
                    u64 n_words; u64 words[n_words] }                           the count phase, where the sums are 0)
                               n_words = buckets + 1 in the count phase: the buckets, then the rows that reached the
                               last bucket through ELSE; 0 in the range phase.  n = the sum of the buckets there.
    and ONLY for plans with VALUE_RULE checks, behind the HISTOGRAM section if there is one:
    u32 magic 'VVRL', u32 n_rules
    n_rules     x { i32 mode, u32 flags; i64 lo_i, hi_i; f64 lo_f, hi_f    (the plan's parameters as they were set: the
                    u64 seen, considered, valid, cast_errors }              bounds are zeros outside the between mode)
                               considered = the non-NULL rows, valid = those of them that pass, cast_errors = those of
                               them CAST(col AS INT) fails on: valid + cast_errors <= considered <= seen.
    and ONLY for plans with VALUE_COUNTS checks, behind the VALUE_RULE section if there is one:
    u32 magic 'VCNT', u32 n_tasks
    n_tasks     x { u32 max_distinct, max_value_bytes            (the plan's parameters)
                    u32 kind (0 no values, 1 int64, 2 bytes), u32 0
                    u64 seen, non_null, overflow_rows, long_rows, n_entries
                    n_entries x { i64 value; u64 count }                      kind 1, ascending int64
                             or { u32 length; u8 bytes[length]; u64 count } } kind 2, ascending bytewise
                               every count > 0, every length <= max_value_bytes, no value twice, and
                               sum(counts) + overflow_rows + long_rows == non_null <= seen.
    and ONLY for plans with PAIR_COUNTS checks, behind the VALUE_COUNTS section if there is one:
    u32 magic 'PCNT', u32 n_tasks
    n_tasks     x { u32 max_pairs, max_value_bytes                   (the plan's parameters: a blob counted under other
                    2 x { i32 mode, u32 bins, f64 origin, width }     ones is refused, binnings compared by their bits;
                                                                      mode 0 value, 1 range, 2 binned; what a mode does
                                                                      not read is zero)
                    u64 seen, both_non_null, overflow_rows, long_rows, non_finite, out_of_range
                    u64 n, f64 min, max                               the range phase (a side of mode 1): the numeric
                                                                      side over the rows with both sides non-NULL;
                                                                      n + non_finite == both_non_null, no entries;
                                                                      min / max are +inf / -inf while n is 0, and n is 0
                                                                      in a count phase
                    u64 n_entries
                    n_entries x { per side { u32 length; u8 bytes[length] }   a value side
                                        or { i64 bin }                        a binned side, 0 <= bin <= bins
                                  u64 count } }                      ascending by (x cell, y cell): bytewise, bins as ints
                               every count > 0, every length <= max_value_bytes, no pair twice, and
                               sum(counts) + overflow_rows + long_rows + non_finite + out_of_range == both_non_null <= seen.
    and ONLY for plans with GROUP_COUNTS checks, behind the PAIR_COUNTS section if there is one:
    u32 magic 'GCNT', u32 n_tasks
    n_tasks     x { u32 max_groups, max_value_bytes              (the plan's parameters)
                    u32 kind (0 no keys, 1 int64, 2 bytes), u32 0
                    u64 seen, null_group_rows, null_group_non_null, overflow_rows, overflow_non_null, long_rows,
                        long_non_null, n_entries
                    n_entries x { i64 key; u64 total, non_null }                      kind 1, ascending int64
                             or { u32 length; u8 bytes[length]; u64 total, non_null } } kind 2, ascending bytewise
                               every total > 0, every non_null <= its total (its rows, for the three classes), every
                               length <= max_value_bytes, no key twice, and
                               sum(totals) + null_group_rows + overflow_rows + long_rows == seen.
    and ONLY for plans with GROUP_SUMS checks, behind the GROUP_COUNTS section if there is one:
    u32 magic 'GSUM', u32 n_tasks
    n_tasks     x { u32 max_groups, max_value_bytes              (the plan's parameters)
                    u32 kind (0 no keys, 1 int64, 2 bytes), u32 values (0 no rows, 1 integer sums, 2 double sums)
                    u64 seen, then { u64 rows, non_null, sum } of the NULL group, of overflow and of the long rows,
                    u64 n_entries
                    n_entries x { i64 key; u64 rows, non_null, sum }                      kind 1, ascending int64
                             or { u32 length; u8 bytes[length]; u64 rows, non_null, sum } } kind 2, ascending bytewise
                               a sum is the Int64 that wrapped (values 1) or the bits of the double (values 2); every
                               rows > 0, every non_null <= its rows, a sum of 0 where non_null is 0, every length <=
                               max_value_bytes, no key twice, values 0 only with seen 0 and no keys, and
                               sum(rows) + null_group_rows + overflow_rows + long_rows == seen.
    and ONLY for plans with ROW_PREDICATE checks, behind the sections above:
    u32 magic 'RRPD', u32 n_tasks
    n_tasks     x { u32 n_leaves, n_ops, n_literal_bytes, 0            (the plan's predicate as it was set: a blob counted
                    n_leaves x { i32 kind, op, col, col2; u32 flags,    under another program, other leaves or other literal
                                 lit_offset, lit_len, 0; i64 lit_i;     bytes is refused; what a leaf does not read is zero)
                                 f64 lit_f }
                    n_ops x u16 (code | arg << 8); u8 literals[n_literal_bytes]
                    u64 seen, satisfied, unknown }
                               satisfied + unknown <= seen; the failed rows are the rest.
    and ONLY for plans with TYPE_CLASSES checks, behind every other section (the ROW_PREDICATE one included):
    u32 magic 'TCLS', u32 n_tasks                                 (a task is a COLUMN: its specs share it)
    n_tasks     x { u64 seen, non_null, boolean, integer, double, date, datetime, string, undecided }
                               non_null <= seen, and the seven classes add up to non_null.

min_key / max_key are the Int64 values themselves, or the IEEE totalOrder keys of Float64 values
(bits ^ ((bits >> 63) >>> 1)).  This module packs partial states from plain numbers; libtgx does the parsing.
"""
import struct

MAGIC, VERSION = 0x53584754, 3
JOINT_MAGIC = 0x42544E4A  # 'JNTB'
TEMPORAL_MAGIC = 0x52504D54  # 'TMPR'
HIST_MAGIC = 0x54534948  # 'HIST'
VALUE_RULE_MAGIC = 0x4C525656  # 'VVRL'
VALUE_COUNTS_MAGIC = 0x544E4356  # 'VCNT'
PAIR_COUNTS_MAGIC = 0x544E4350  # 'PCNT'
GROUP_COUNTS_MAGIC = 0x544E4347  # 'GCNT'
GROUP_SUMS_MAGIC = 0x4D555347  # 'GSUM'
KEY_PROBE_MAGIC = 0x4252504B  # 'KPRB'
ROW_PREDICATE_MAGIC = 0x44505252  # 'RRPD'
TYPE_CLASSES_MAGIC = 0x534C4354  # 'TCLS'
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def f64_total_key(x):
    bits = struct.unpack("<q", struct.pack("<d", x))[0]
    return bits ^ ((bits >> 63) & 0x7FFFFFFFFFFFFFFF)


def scan_acc(total, non_null, minimum=None, maximum=None, total_sum=0, is_float=False, var=None):
    """var = (n, mean, m2) or None.  total_sum: exact int for Int64 columns, float for Float64 columns."""
    if non_null == 0 or minimum is None:
        mn, mx = I64_MAX, I64_MIN
    elif is_float:
        mn, mx = f64_total_key(float(minimum)), f64_total_key(float(maximum))
    else:
        mn, mx = int(minimum), int(maximum)
    if is_float:
        lo, hi, s = 0, 0, float(total_sum)
    else:
        v = int(total_sum) & ((1 << 128) - 1)
        lo, hi = v & ((1 << 64) - 1), v >> 64
        hi = hi - (1 << 64) if hi >= (1 << 63) else hi
        s = 0.0
    vn, vmean, vm2 = var if var else (0, 0.0, 0.0)
    return struct.pack("<qqqqQqddqddii", total, non_null, mn, mx, lo, hi, s, 0.0, vn, vmean, vm2,
                       1 if is_float else 0, 0)


def count_acc(total, non_null):
    return struct.pack("<qq", total, non_null)


def comoment_acc(total, n, sum_x, sum_y, sum_x2, sum_y2, sum_xy, px=0.0, py=0.0):
    """the five sums are taken about the pivots (px, py); the default (0, 0) means raw sums"""
    return struct.pack("<qq5d5dddii", total, n, sum_x, sum_y, sum_x2, sum_y2, sum_xy, 0.0, 0.0, 0.0, 0.0, 0.0,
                       px, py, 1, 0)


def distinct_counts(total, non_null, distinct, twice=0):
    """an owner-partitioned partial: this rank's keys are disjoint from every other rank's"""
    return struct.pack("<II5QQ", 1, 0, total, non_null, distinct, twice, 0, 0)


def kll_state(k, n, minimum, maximum, levels):
    out = struct.pack("<IIQdd", k, len(levels), n, minimum, maximum)
    for items in levels:
        out += struct.pack("<I", len(items)) + struct.pack("<%dd" % len(items), *items)
    return out


def regex_counts(total, matches):
    return struct.pack("<QQ", total, matches)


def hll_state(registers=None, mode=1):
    """registers: 16384 bytes (or None: nothing seen yet)"""
    if registers is None:
        return struct.pack("<II", mode, 0)
    assert len(registers) == 16384
    return struct.pack("<II", mode, 1) + bytes(registers)


def joint_range_state(total, n, non_finite=0, x_min=None, x_max=None, y_min=None, y_max=None):
    """a JOINT_BINS task in its range phase (extremes None: no rows)"""
    inf = float("inf")
    ext = [inf if x_min is None else x_min, -inf if x_max is None else x_max, inf if y_min is None else y_min,
           -inf if y_max is None else y_max]
    return struct.pack("<II4d3q4dQ", 0, 0, 0.0, 0.0, 0.0, 0.0, total, n, non_finite, *ext, 0)


def joint_count_state(binning, total, cells, outside=0, non_finite=0):
    """a JOINT_BINS task in its count phase: binning = (x_origin, x_width, y_origin, y_width, bins), `cells` the
    (bins + 1)^2 counts, row-major"""
    x0, xw, y0, yw, bins = binning
    assert len(cells) == (bins + 1) ** 2
    inf = float("inf")
    words = list(cells) + [outside]
    return (struct.pack("<II4d3q4dQ", 1, bins, x0, xw, y0, yw, total, sum(cells), non_finite, inf, -inf, inf, -inf,
                        len(words)) + struct.pack("<%dQ" % len(words), *words))


def temporal_state(mode, flags, seen, live, passed, delta=0, ticks_per_second=0, lo=0, hi=0):
    """a TEMPORAL task: the plan's parameters as the device holds them (time of day: lo / hi = tod_lo / tod_hi; the
    fields of other modes 0) and its three counters"""
    return struct.pack("<iI4q3Q", mode, flags, delta, ticks_per_second, lo, hi, seen, live, passed)


def hist_range_state(total, n, non_finite=0, min=None, max=None, sum=0.0, sum_squared=0.0):
    """a HISTOGRAM task in its range phase (extremes None: no rows)"""
    inf = float("inf")
    return struct.pack("<II3q4dQ", 0, 0, total, n, non_finite, inf if min is None else min, -inf if max is None else max,
                       sum, sum_squared, 0)


def hist_count_state(edges, total, counts, else_rows=0, non_finite=0):
    """a HISTOGRAM task in its count phase: the plan's buckets + 1 `edges` and the bucket `counts`"""
    buckets = len(edges) - 1
    assert len(counts) == buckets
    inf = float("inf")
    words = list(counts) + [else_rows]
    return (struct.pack("<II%dd3q4dQ" % len(edges), 1, buckets, *edges, total, sum(counts), non_finite, inf, -inf, 0.0, 0.0,
                        len(words)) + struct.pack("<%dQ" % len(words), *words))


def value_rule_state(mode, flags, seen, considered, valid, cast_errors=0, lo_i=0, hi_i=0, lo_f=0.0, hi_f=0.0):
    """a VALUE_RULE task: the plan's parameters as they were set and its four counters"""
    return struct.pack("<iI2q2d4Q", mode, flags, lo_i, hi_i, lo_f, hi_f, seen, considered, valid, cast_errors)


def value_counts_state(max_distinct, max_value_bytes, seen, counts, nulls=0, overflow_rows=0, long_rows=0,
                       ordered=True):
    """a VALUE_COUNTS task: the plan's parameters, the counters and the entries of `counts` (value -> count; every key an
    int, or every key bytes).  non_null is what the invariant makes it: sum(counts) + overflow_rows + long_rows, and
    seen - nulls must equal it.  `ordered=False` keeps the entries in the order given (for a blob that is to be refused)."""
    items = list(counts.items()) if hasattr(counts, "items") else list(counts)
    is_bytes = bool(items) and isinstance(items[0][0], (bytes, bytearray))
    if ordered:
        items.sort(key=lambda kv: kv[0])
    non_null = sum(c for _, c in items) + overflow_rows + long_rows
    if seen - nulls != non_null:
        raise ValueError("seen - nulls must be sum(counts) + overflow_rows + long_rows")
    out = struct.pack("<4I5Q", max_distinct, max_value_bytes, (2 if is_bytes else 1) if items else 0, 0, seen, non_null,
                      overflow_rows, long_rows, len(items))
    for v, c in items:
        out += (struct.pack("<I", len(v)) + bytes(v) + struct.pack("<Q", c)) if is_bytes else struct.pack("<qQ", v, c)
    return out


def pair_side(mode=0, bins=0, origin=0.0, width=0.0):
    """one side of a PAIR_COUNTS task's parameters: mode 0 value, 1 range, 2 binned"""
    return struct.pack("<iI2d", mode, bins, origin, width)


def pair_counts_state(max_pairs, max_value_bytes, x_side, y_side, seen, counts=(), both_non_null=None, overflow_rows=0,
                      long_rows=0, non_finite=0, out_of_range=0, n=0, lo=float("inf"), hi=float("-inf"), ordered=True):
    """a PAIR_COUNTS task: the plan's parameters (x_side / y_side from pair_side), the counters and the entries of
    `counts` ((x cell, y cell) -> count; a cell is bytes on a value side and an int on a binned side).  both_non_null
    defaults to what the invariant makes it.  n / lo / hi: the range phase.  `ordered=False` keeps the entries in the
    order given (for a blob that is to be refused)."""
    items = list(counts.items()) if hasattr(counts, "items") else list(counts)
    if ordered:
        items.sort(key=lambda kv: kv[0])
    if both_non_null is None:
        both_non_null = sum(c for _, c in items) + overflow_rows + long_rows + non_finite + out_of_range + n
    out = struct.pack("<2I", max_pairs, max_value_bytes) + x_side + y_side
    out += struct.pack("<7Q2dQ", seen, both_non_null, overflow_rows, long_rows, non_finite, out_of_range, n, lo, hi,
                       len(items))
    for (cx, cy), c in items:
        for cell in (cx, cy):
            out += struct.pack("<q", cell) if isinstance(cell, int) else struct.pack("<I", len(cell)) + bytes(cell)
        out += struct.pack("<Q", c)
    return out


def group_counts_state(max_groups, max_value_bytes, groups, seen=None, null_group=(0, 0), overflow=(0, 0), long=(0, 0),
                       ordered=True, arity=0):
    """a GROUP_COUNTS task: the plan's parameters, the counters and the entries of `groups` (key -> (total, non_null);
    every key an int, or every key bytes).  null_group / overflow / long: (rows, non-NULL values among them).  seen
    defaults to what the invariant makes it.  `ordered=False` keeps the entries in the order given (for a blob that is to
    be refused).  arity: 2 .. 8 for a task that groups by a tuple of columns, whose keys are term_amd.group_key's encoded
    tuples; 0 for a task with one group column."""
    items = list(groups.items()) if hasattr(groups, "items") else list(groups)
    is_bytes = bool(items) and isinstance(items[0][0], (bytes, bytearray))
    if ordered:
        items.sort(key=lambda kv: kv[0])
    if seen is None:
        seen = sum(t for _, (t, _n) in items) + null_group[0] + overflow[0] + long[0]
    out = struct.pack("<4I8Q", max_groups, max_value_bytes, (2 if is_bytes else 1) if items else 0, arity, seen, *null_group,
                      *overflow, *long, len(items))
    for k, (t, n) in items:
        out += (struct.pack("<I", len(k)) + bytes(k) if is_bytes else struct.pack("<q", k)) + struct.pack("<QQ", t, n)
    return out


def group_sums_state(max_groups, max_value_bytes, groups, is_float=False, seen=None, null_group=(0, 0, 0),
                     overflow=(0, 0, 0), long=(0, 0, 0), ordered=True, values=None, arity=0):
    """a GROUP_SUMS task: the plan's parameters, the classes and the entries of `groups` (key -> (rows, non_null, sum);
    every key an int, or every key bytes).  null_group / overflow / long: (rows, non-NULL values among them, their sum).
    A sum is an int (taken modulo 2^64) or, with is_float, a float.  seen defaults to what the invariant makes it, values
    (the blob's value kind) to what is_float says, 0 for a state without rows.  `ordered=False` keeps the entries in the
    order given (for a blob that is to be refused).  arity: as in group_counts_state; it rides the upper half of the key
    kind word."""
    items = list(groups.items()) if hasattr(groups, "items") else list(groups)
    is_bytes = bool(items) and isinstance(items[0][0], (bytes, bytearray))
    if ordered:
        items.sort(key=lambda kv: kv[0])
    if seen is None:
        seen = sum(v[0] for _, v in items) + null_group[0] + overflow[0] + long[0]
    if values is None:
        values = 0 if seen == 0 else (2 if is_float else 1)

    def cls(c):
        return struct.pack("<QQ", c[0], c[1]) + (struct.pack("<d", c[2]) if is_float else
                                                  struct.pack("<Q", c[2] & ((1 << 64) - 1)))
    out = struct.pack("<4IQ", max_groups, max_value_bytes, ((2 if is_bytes else 1) if items else 0) | arity << 16, values,
                      seen)
    out += cls(null_group) + cls(overflow) + cls(long) + struct.pack("<Q", len(items))
    for k, v in items:
        out += (struct.pack("<I", len(k)) + bytes(k) if is_bytes else struct.pack("<q", k)) + cls(v)
    return out


def key_probe_state(max_missing_keys, missing=(), seen=None, nulls=0, matched=0, overflow_rows=0, parent=None,
                    ordered=True, non_null=None, counted=None, strings=None):
    """a KEY_PROBE task: the plan's parameter, the identity of the parent set the counts were taken under (`parent`:
    (parent_keys, parent_digest), or None for a state that knows of none), the counters and the entries of `missing`
    (key -> rows).  non_null defaults to what the invariant makes it -- matched + sum(missing) + overflow_rows -- and seen
    to non_null + nulls.  `ordered=False` keeps the entries in the order given (for a blob that is to be refused).
    `counted`: (parent_rows, parent_count_digest, max_count, pairs) of a counted task (Plan.set_key_probe_counted) -- the
    rest of its set's identity, the set's largest count and the matched pairs; the task's second reserved word is then 1
    and the four words stand before the entries.  None: a plain task, whose bytes are the ones they always were.
    `strings`: (max_value_bytes, long_rows) of a task on string keys (Plan.set_key_probe_strings): the second reserved
    word is then 2, { u32 max_value_bytes, u32 0, u64 long_rows } stand before the entries, the keys of `missing` are
    bytes and an entry is { u32 length, bytes, u64 rows }, ascending bytewise; long_rows count towards non_null.  A blob
    that holds such a task with a non-empty parent set carries the plan's fingerprint key (pack's fingerprint_key).
    `counted` and `strings` together: a counted task on string keys (Plan.set_key_probe_strings_counted) -- the second
    reserved word is 4, the counted task's four words stand first, then the strings task's three, then its entries."""
    items = list(missing.items()) if hasattr(missing, "items") else list(missing)
    if ordered:
        items.sort(key=lambda kv: kv[0])
    if non_null is None:
        non_null = matched + sum(c for _, c in items) + overflow_rows + (strings[1] if strings is not None else 0)
    if seen is None:
        seen = non_null + nulls
    keys, digest = parent if parent is not None else (0, 0)
    mode = (4 if strings is not None else 1) if counted is not None else 2 if strings is not None else 0
    out = struct.pack("<4I7Q", max_missing_keys, 0, 1 if parent is not None else 0, mode, keys, digest, seen, non_null,
                      matched, overflow_rows, len(items))
    if counted is not None:
        out += struct.pack("<4Q", *counted)
    if strings is not None:
        out += struct.pack("<IIQ", strings[0], 0, strings[1])
    for k, c in items:
        out += struct.pack("<I", len(k)) + bytes(k) + struct.pack("<Q", c) if strings is not None else struct.pack("<qQ", k, c)
    return out


def row_predicate_state(leaves, program, literals, seen, satisfied, unknown=0):
    """a ROW_PREDICATE task: the plan's predicate as it was set (`leaves`: dicts with the fields of
    tgx_row_predicate_leaf, those left out 0; `program`: (code, arg) pairs or packed ints; `literals`: the pool's
    bytes) and its three counters"""
    out = struct.pack("<4I", len(leaves), len(program), len(literals), 0)
    for leaf in leaves:
        g = leaf.get
        out += struct.pack("<4i4Iqd", g("kind", 0), g("op", 0), g("col", 0), g("col2", 0), g("flags", 0),
                           g("lit_offset", 0), g("lit_len", 0), 0, g("lit_i", 0), g("lit_f", 0.0))
    out += b"".join(struct.pack("<H", op if isinstance(op, int) else (op[0] | (op[1] << 8))) for op in program)
    return out + bytes(literals) + struct.pack("<3Q", seen, satisfied, unknown)


def type_classes_state(seen, non_null, boolean=0, integer=0, double=0, date=0, datetime=0, string=0, undecided=0):
    """a TYPE_CLASSES task (one column): rows seen, the non-NULL rows and the seven classes they fall into"""
    return struct.pack("<9Q", seen, non_null, boolean, integer, double, date, datetime, string, undecided)


def pack(scan=(), count=(), comoments=(), distinct=(), kll=(), regex=(), hll=(), joint=(), temporal=(), hist=(),
         value_rules=(), value_counts=(), pair_counts=(), group_counts=(), group_sums=(), key_probes=(),
         fingerprint_key=None, row_predicates=(), type_classes=()):
    head = struct.pack("<9I", MAGIC, VERSION, len(scan), len(count), len(comoments), len(distinct), len(kll), len(regex),
                       len(hll))
    # (no string keys in a state packed from plain numbers, unless a KEY_PROBE task on string keys knows its parent set:
    # `fingerprint_key`, the 16 bytes of the plan's key)
    head += struct.pack("<I16s", 0, bytes(16)) if fingerprint_key is None else struct.pack("<I16s", 1, bytes(fingerprint_key))
    tail = struct.pack("<II", JOINT_MAGIC, len(joint)) + b"".join(joint) if joint else b""
    if temporal:
        tail += struct.pack("<II", TEMPORAL_MAGIC, len(temporal)) + b"".join(temporal)
    if hist:
        tail += struct.pack("<II", HIST_MAGIC, len(hist)) + b"".join(hist)
    if value_rules:
        tail += struct.pack("<II", VALUE_RULE_MAGIC, len(value_rules)) + b"".join(value_rules)
    if value_counts:
        tail += struct.pack("<II", VALUE_COUNTS_MAGIC, len(value_counts)) + b"".join(value_counts)
    if pair_counts:
        tail += struct.pack("<II", PAIR_COUNTS_MAGIC, len(pair_counts)) + b"".join(pair_counts)
    if group_counts:
        tail += struct.pack("<II", GROUP_COUNTS_MAGIC, len(group_counts)) + b"".join(group_counts)
    if group_sums:
        tail += struct.pack("<II", GROUP_SUMS_MAGIC, len(group_sums)) + b"".join(group_sums)
    if key_probes:
        tail += struct.pack("<II", KEY_PROBE_MAGIC, len(key_probes)) + b"".join(key_probes)
    if row_predicates:
        tail += struct.pack("<II", ROW_PREDICATE_MAGIC, len(row_predicates)) + b"".join(row_predicates)
    if type_classes:
        tail += struct.pack("<II", TYPE_CLASSES_MAGIC, len(type_classes)) + b"".join(type_classes)
    return (head + b"".join(scan) + b"".join(count) + b"".join(comoments) + b"".join(distinct) + b"".join(kll) +
            b"".join(regex) + b"".join(hll) + tail)
