"""A seeded differential tester for the whole C ABI path: random plans over random tables in random batchings, the
device's answers against the CPU oracle's on the logical table (tests/test_gpu_fuzz.py runs a fixed set of seeds;
tools/fuzz_device.py any range).  One seed fixes everything: columns (type, shape of the values, NULL rate), checks,
how the rows are cut into tgx_update calls (one batch, ragged cuts, a stream of DataFusion-sized batches; DEVICE or
HOST buffers; Arrow offsets), and what happens to the state before it is read (finalize / blob round trip / several
states merged).  Bit-exact wherever the reference is (counts, MIN / MAX, integer sums, DISTINCT, HyperLogLog
registers -> estimate); 1e-6 relative for floating-point aggregates (north star).

The two-phase kinds (HISTOGRAM, JOINT_BINS) make a case run TWICE: pass one has their specs in the range phase, pass
two is a fresh plan with edges / binnings set -- derived from the exact references' ranges, never from what the device
said in pass one -- fed the same table through the same batching and state sequence.  TEMPORAL is complete in pass
one.  These three are compared with tests/exact_histogram.py, exact_joint.py and exact_temporal.py: every count, extreme
and counter for equality, the histogram's two plain double sums within exact_histogram.sum_bounds (or by its overflow
rule, sum_rules).

TIME_GAP (the one kind that keeps rows on the device between batches) is drawn last, from a stream of its own, for cases
that are simply finalized: one or two tasks (timestamp column, group column or none -- any Int64-shaped or widened
integer column, the timestamp column itself included), each with 1 to 3 thresholds (sometimes more than one neighbour
pass compares) taken from the gaps tests/exact_time_gap.py finds in the whole table, some under one of the environments
of tests/test_gpu_time_gap.py that force the sort's other routes.  It changes nothing an earlier stream drew.  All five
counters of every spec are compared for equality.

VALUE_RULE and the four counting kinds (VALUE_COUNTS, PAIR_COUNTS, GROUP_COUNTS, GROUP_SUMS) are drawn after it, from a
stream of their own again, for tables of at most 400 000 rows and every `after` and `seq` -- the five kinds are additive:
one to three rules (now and then nine) on a numeric column, BETWEEN with bounds from the column's own values; a key column
of kind Int64, Int32, a narrow presentation or a string in any layout, with max_value_bytes that sometimes cuts real
words; one to three GROUP_COUNTS members on one walk; a GROUP_SUMS over integer or float values; a PAIR_COUNTS of two
string sides or of a string and a numeric one, which makes the case run twice as the two-phase kinds above do (RANGE,
then BINNED with the binning of the exact range, sometimes moved).  The bounds are drawn against the exact number of keys
d: with d <= bound include/tgx.h promises no overflow, and the entries, their order and every counter are compared for
equality with tests/exact_value_counts.py, exact_pair_counts.py, exact_group_counts.py and exact_group_sums.py (float
sums within exact_group_sums.float_bound, or by its float_rule); so is a table of more keys that reports no overflow;
one that reports overflow is held to the identities of include/tgx.h, to holding only keys of the table, none counted too
often, and to the slots it has.  The four VALUE_RULE counters are compared with exact_value_rule.counts_np.

KEY_PROBE is drawn last of all, from a stream of its own once more (and what is random when the case RUNS from a second
private stream: run_device_inner draws from the case's own stream exactly what it drew before), for about half of the
tables of at most 400 000 rows: one to three specs, now and then nine on one column and route.  The plain, counted and
strings modes for every `after` and `seq`; a rows spec for a state that is simply finalized, its records read back after
the last batch and compared as a multiset with the column's non-NULL keys.  A parent set (class ParentSet) is a column
drawn from the child's own distinct values -- none, a few, half or all of them, strangers, the key -1, duplicates,
multiplicities up to a few thousand and now and then 2^40, the empty set -- shaped so that routes 0 to 5 and the 128 x n
and 4 x n thresholds occur, or another integer column of the table in its own Arrow type; it reaches every state that
is fed as hand-made records, as the DISTINCT export of a second plan and state (under the child plan's fingerprint key),
or as what a rows spec gathers.  States that are merged into or deserialized hold no set and read `route` 0 under the
set's identity; a state rebuilt from a blob taken mid-table must refuse the next batch (TGX_INVALID_ARGUMENT naming the
spec), take it once the same sets are given again, and every other check of the plan must still equal its reference.
The bounds are drawn against the exact number of missing keys d; with d <= bound, or without overflow, every counter, the
set's digests and route, the entries with their order and, counted, pairs, join_rows, parent_rows, parent_count_digest
and max_count equal tests/exact_key_probe.py, exact_join_coverage.py and exact_key_probe_strings.py; matched, pairs,
non_null, null_rows and long_rows never depend on the bound.
tests/test_fuzz_cases.py tests this tester without a device."""
import math
import sys

import numpy as np

import exact_group_counts as EGC
import exact_group_sums as EGS
import exact_histogram as EH
import exact_hll as H
import exact_join_coverage as EJC
import exact_joint as EJ
import exact_key_probe as EKP
import exact_key_probe_strings as EKS
import exact_pair_counts as EP
import exact_temporal as ET
import exact_time_gap as EG
import exact_quantiles as Q
import exact_ranks as R
import exact_value_counts as EVC
import exact_value_rule as EV
import exact_widening as W
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import numeric_column, pad_validity, rel_err, to_device

TOL = 1e-6


# ---- tables -----------------------------------------------------------------------------------------------------------
def int_values(rng, n, shape):
    if shape == "permutation":
        return rng.permutation(n).astype(np.int64) * int(rng.integers(1, 4)) + int(rng.integers(-10**6, 10**12))
    if shape == "ascending":
        return np.arange(n, dtype=np.int64) * int(rng.integers(1, 5)) + int(rng.integers(-10**9, 10**9))
    if shape == "descending":
        return int(rng.integers(0, 10**10)) - np.arange(n, dtype=np.int64) * int(rng.integers(1, 3))
    if shape == "few":
        return rng.integers(-3, int(rng.integers(1, 200)), size=n, dtype=np.int64)  # (includes -1: the all-ones key)
    if shape == "tenth":
        return rng.integers(0, max(2, n // 10), size=n, dtype=np.int64)
    if shape == "wide":
        return rng.integers(-(2**62), 2**62, size=n, dtype=np.int64)
    if shape == "constant":
        return np.full(n, int(rng.integers(-5, 5)), dtype=np.int64)
    if shape == "strays":  # dense and in order, a few keys from far away
        v = np.arange(n, dtype=np.int64)
        m = rng.random(n) < 0.002
        v[m] = rng.integers(-(2**40), 2**40, size=int(m.sum()), dtype=np.int64)
        return v
    if shape == "blocks":  # sorted blocks, shuffled
        v = np.arange(n, dtype=np.int64)
        cut = list(range(0, n, 7919)) or [0]
        return np.concatenate([v[c:c + 7919] for c in (cut[k] for k in rng.permutation(len(cut)))]) if n else v
    raise AssertionError(shape)


INT_SHAPES = ["permutation", "ascending", "descending", "few", "tenth", "wide", "constant", "strays", "blocks"]


def float_values(rng, n, shape):
    if shape == "uniform":
        return rng.random(n) * 1000.0
    if shape == "normal":
        return rng.standard_normal(n) * float(rng.choice([1.0, 1e-3, 1e6])) + float(rng.choice([0.0, 1e9]))
    if shape == "rounded":
        v = np.round(rng.standard_normal(n), 2)
        v[rng.random(n) < 0.01] = -0.0
        return v
    if shape == "ints":
        return rng.integers(-1000, 1000, size=n).astype(np.float64)
    if shape == "ascending":
        return np.arange(n, dtype=np.float64) * 0.5
    if shape == "specials":  # NaN (two payloads), infinities, signed zeros, denormals among ordinary values
        v = np.round(rng.standard_normal(n) * 10, 1)
        pool = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1e308], dtype=np.float64)
        m = rng.random(n) < 0.05
        v[m] = pool[rng.integers(0, len(pool), size=int(m.sum()))]
        return v
    raise AssertionError(shape)


FLOAT_SHAPES = ["uniform", "normal", "rounded", "ints", "ascending", "specials"]


def f32_bit_patterns(rng, n):
    """a Float32 column of the patterns no cast of a Float64 gives: NaN payloads, signalling and quiet, of both signs
    (some payload both ways: two keys of DISTINCT), and subnormals, among ordinary values"""
    u = (rng.standard_normal(n) * 10).astype(np.float32).view(np.uint32)
    pick = rng.random(n)
    sign = rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(31)
    payload = rng.integers(1, 2 ** 23, size=n, dtype=np.uint64)
    rep = rng.random(n) < 0.5
    payload[rep] = rng.integers(1, 8, size=int(rep.sum()), dtype=np.uint64)  # a few payloads repeat
    quiet = np.where(rng.random(n) < 0.5, np.uint64(0x400000), np.uint64(0))
    nan = (sign | np.uint64(0x7F800000) | quiet | payload).astype(np.uint32)
    sub = (sign | rng.integers(1, 2 ** 23, size=n, dtype=np.uint64)).astype(np.uint32)
    u = np.where(pick < 0.06, nan, np.where(pick < 0.12, sub, u))
    return u.view(np.float32)


# ---- strings ----------------------------------------------------------------------------------------------------------
WORD_PARTS = ["a", "Z", "user", "@", ".", "com", "é", "ß", "你", "🦀", " ", "0", "42", "-", "_", "x" * 17]
PATTERNS = [("@", 0), (r"^[a-zA-Z0-9]+$", 0), (r"^\s*user", 0), (r"(?i)^USER", 0), (r"[0-9]{2}", 0), (r"^$", 0),
            (r"é|你", 0), (r"^[^@]+@[^@]+\.[a-z]+$", 0), (r"com$", "trim"), (r"^user", "ci"), (r"\d", "nullvalid")]


def string_values(rng, n, vocab):
    """n strings drawn from `vocab` distinct words -> (offsets int32/int64-able, data uint8, list of the words, picks)"""
    words = []
    seen = set()
    while len(words) < vocab:
        k = int(rng.integers(0, 7))
        w = "".join(WORD_PARTS[int(j)] for j in rng.integers(0, len(WORD_PARTS), size=k)) + (
            "" if len(words) < 3 else "#%d" % len(words))
        if w in seen:
            continue
        seen.add(w)
        words.append(w)
    enc = [w.encode("utf-8") for w in words]
    picks = rng.integers(0, vocab, size=n)
    lens = np.array([len(e) for e in enc], dtype=np.int64)[picks]
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    data = np.frombuffer(b"".join(enc[k] for k in picks) or b"\0", dtype=np.uint8).copy()
    return offsets, data, words, picks


class Buffers:
    """the Arrow buffers of one column, on the host and (uploaded once, on first use) on the device"""

    def __init__(self, kind, vals, vb, extra, mask, seed, present=None):
        self.kind = kind
        self.present = present  # (round 5) an Int64 column handed over as a narrower / unsigned / Boolean Arrow type
        self.host = {"validity": pad_validity(vb)}
        self.layout = "plain"
        if kind == "s" and extra[2] != "plain":
            # Utf8View / Dictionary<Int32, Utf8>: built per batch from the Python values (tests/test_gpu_utf8view.py,
            # tests/test_gpu_dictionary.py); small tables only
            self.layout = extra[2]
            self.values = [extra[3][k] if m else None for k, m in zip(extra[4], mask)]
            self.rng = np.random.default_rng(seed)
        if kind == "s":
            self.large = extra[1]
            self.host["offsets"] = vals if self.large else vals.astype(np.int32)
            self.host["data"] = np.concatenate([extra[0], np.zeros(16, np.uint8)])
        elif present == "bool":
            self.host["values"] = np.concatenate([orc.pack_validity(vals != 0), np.zeros(64, np.uint8)])
        elif present is not None:
            narrow = vals.astype(present)
            assert (narrow.astype(np.int64) == vals).all() or present == np.uint64
            self.host["values"] = np.concatenate([narrow, np.zeros(64, narrow.dtype)]).view(np.uint8)
        else:
            self.host["values"] = vals
        self.dev = None

    def column(self, on_device, offset, length):
        if self.layout == "view":
            from test_gpu_utf8view import view_column

            lead = int(self.rng.integers(0, 70))  # (an Arrow offset into a longer array)
            return view_column([None] * lead + self.values[offset:offset + length], self.rng, on_device, offset=lead,
                               length=length)
        if self.layout == "dict":
            from test_gpu_dictionary import encode

            return encode(self.values[offset:offset + length], self.rng, repeat_entries=bool(self.rng.integers(0, 2)),
                          large=self.large, device=on_device)
        if on_device and self.dev is None:
            self.dev = {k: to_device(v) for k, v in self.host.items()}
        b = self.dev if on_device else self.host
        if self.kind == "s":
            return T.Column(T.LARGE_UTF8 if self.large else T.UTF8, length, offsets=b["offsets"], data=b["data"],
                            validity=b["validity"], offset=offset)
        if self.present is not None:
            type_id = {"bool": T.BOOL, np.int8: T.INT8, np.int16: T.INT16, np.uint8: T.UINT8, np.uint16: T.UINT16,
                       np.uint32: T.UINT32, np.uint64: T.UINT64}[self.present]
            return T.Column(type_id, length, values=b["values"], validity=b["validity"], offset=offset)
        ctor = {"i": T.Column.int64, "f": T.Column.float64, "i32": T.Column.int32, "f32": T.Column.float32}[self.kind]
        return ctor(b["values"], b["validity"], length=length, offset=offset)


def make_validity(rng, n, rate):
    if rate == 0.0:
        return None, np.ones(n, dtype=bool)
    mask = rng.random(n) >= rate if rate < 1.0 else np.zeros(n, dtype=bool)
    return orc.pack_validity(mask), mask


class ParentSet:
    """the parent side of one KEY_PROBE spec: a column (values, valid) and how its keys reach the state --
    "a": hand-made records, one per non-NULL row (integers: {key, count} with `counts`; strings: fingerprints);
    "b": the DISTINCT export of a second plan and state that walk the column (one record per distinct key, count 1);
    "c": the records a rows spec gathers from it (one {key, 1} record per non-NULL row; counted specs).
    Integers: `values` are the int64 keys, handed over as a column of `kind` / `present`.  Strings: `values` index
    `words`, and the column has `layout` (layout, LargeUtf8?)."""

    def __init__(self, source, values, valid, counts, what, kind="i", present=None, width=8, words=None, layout=None,
                 near=()):
        self.source, self.values, self.valid, self.counts, self.what = source, np.asarray(values, np.int64), valid, counts, what
        self.kind, self.present, self.width, self.words, self.layout = kind, present, width, words, layout
        # strings, "a": values that are NOT in the set, each of which gives two records that share one word of its
        # fingerprint -- (hash_a, hash_b ^ 1) and (hash_a ^ 1, hash_b): keys of the set that no value has
        self.near = list(near) if source == "a" else []

    def fingerprints(self, key):
        """strings, "a": the records' (hash_a, hash_b) under the fingerprint key `key`"""
        import fp_reference

        fps = [fp_reference.fingerprint(key, w) for w in self.record_values()]
        for fa, fb in (fp_reference.fingerprint(key, w) for w in self.near):
            fps += [(fa, fb ^ 1), (fa ^ 1, fb)]
        return fps

    def __repr__(self):
        return "<%s: %s, %d rows, %d keys%s>" % (self.source, self.what, len(self.values), len(np.unique(self.values[self.valid])),
                                                 ", %d near" % len(self.near) if self.near else "")

    def records(self):
        """(keys, counts) of the records the set is built from (integers)"""
        live = self.values[self.valid]
        if self.source == "b":
            live = np.unique(live)
        return live, (self.counts if self.source == "a" else np.ones(len(live), np.uint64))

    def n_records(self):
        return len(self.records()[0]) + 2 * len(self.near)

    def max_count(self):
        keys, counts = self.records()
        if not len(keys):
            return 0
        _, inv = np.unique(keys, return_inverse=True)
        return int(np.bincount(inv, weights=counts.astype(np.float64)).max())  # (a bound's worth of precision)

    def duplicates(self):
        keys = self.records()[0]
        return len(np.unique(keys)) < len(keys)

    def on_threshold(self, limit):
        """does the set sit exactly on a route's threshold -- range == limit * n_records -- or just beyond it?"""
        keys = self.records()[0]
        return len(keys) > 0 and int(keys.max()) - int(keys.min()) + 1 - limit * len(keys) in (0, 1)

    def record_values(self):
        """strings, "a": the value of every record"""
        return [self.words[int(k)].encode("utf-8") for k in self.values[self.valid]]

    def distinct_values(self):
        return [self.words[int(k)].encode("utf-8") for k in np.unique(self.values[self.valid])]

    def buffers(self, seed):
        vb = None if self.valid.all() else orc.pack_validity(self.valid)
        if self.words is None:
            vals = self.values.astype(np.int32) if self.kind == "i32" else self.values
            return Buffers(self.kind, vals, vb, None, self.valid, seed, self.present)
        enc = [w.encode("utf-8") for w in self.words]
        offsets = np.zeros(len(self.values) + 1, np.int64)
        np.cumsum(np.array([len(w) for w in enc], np.int64)[self.values], out=offsets[1:])
        data = np.frombuffer(b"".join(enc[int(k)] for k in self.values) or b"\0", dtype=np.uint8).copy()
        return Buffers("s", offsets, vb, (data, self.layout[1], self.layout[0], self.words, self.values), self.valid, seed)


# ---- one case ---------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, seed, max_rows=2_600_000, host_only=False):
        rng = self.rng = np.random.default_rng(seed)
        self.seed = seed
        size_class = rng.choice(["tiny", "small", "medium", "big"], p=[0.15, 0.3, 0.3, 0.25])
        n = {"tiny": int(rng.integers(0, 70)), "small": int(rng.integers(70, 20_000)),
             "medium": int(rng.integers(20_000, 400_000)), "big": int(rng.integers(min(1_050_000, max_rows - 1), max_rows))}[size_class]
        self.n = n
        self.cols = []  # (kind 'i'/'f', values, validity bytes or None, mask)
        self.shapes = []  # per column: the shape of an Int64 column's values (INT_SHAPES), None for the other kinds
        for _ in range(int(rng.integers(1, 4))):
            rate = float(rng.choice([0.0, 0.0, 0.02, 0.3, 1.0], p=[0.3, 0.2, 0.25, 0.2, 0.05]))
            kind = str(rng.choice(["i", "f", "i32", "f32", "s"], p=[0.45, 0.25, 0.08, 0.07, 0.15]))
            extra = None
            self.shapes.append(None)
            if kind == "i":
                self.shapes[-1] = str(rng.choice(INT_SHAPES))
                vals = int_values(rng, n, self.shapes[-1])
            elif kind == "f":
                vals = np.ascontiguousarray(float_values(rng, n, str(rng.choice(FLOAT_SHAPES))), dtype=np.float64)
            elif kind == "i32":
                vals = int_values(rng, n, str(rng.choice(["permutation", "ascending", "few", "tenth", "constant"])))
                vals = (vals % (2**31)).astype(np.int32) if rng.random() < 0.5 else vals.astype(np.int32)
            elif kind == "f32":
                shape = str(rng.choice(["uniform", "rounded", "ints", "specials", "bits"]))
                with np.errstate(over="ignore"):  # (1e308 becomes inf: one more special value)
                    vals = f32_bit_patterns(rng, n) if shape == "bits" else float_values(rng, n, shape).astype(np.float32)
            else:
                vocab = int(rng.choice([1, 3, 100, max(1, n // 10), max(1, n)]))
                vocab = min(vocab, 200_000)
                offsets, data, words, picks = string_values(rng, n, vocab)
                # (data, LargeUtf8?, layout, the values as a Python list for the layouts built row by row)
                layout = str(rng.choice(["plain", "view", "dict"], p=[0.6, 0.2, 0.2])) if n <= 20_000 else "plain"
                vals, extra = offsets, (data, bool(rng.integers(0, 2)), layout, words, picks)
            vb, mask = make_validity(rng, n, rate)
            self.cols.append((kind, vals, vb, mask, extra))
        # checks
        self.specs, self.expect = [], []
        for ci, (kind, vals, vb, mask, extra) in enumerate(self.cols):
            numeric = kind != "s"
            menu = ["count", "stats", "var", "distinct", "mult", "approx"] if numeric else \
                   ["count", "distinct", "mult", "approx", "length", "regex", "regex"]
            picks = [str(x) for x in rng.choice(menu, size=int(rng.integers(1, 4)), replace=False)]
            if "count" in picks:
                self.add(spec(T.COUNT, ci), ("count", ci))
            if "var" in picks:
                self.add(spec(T.NUMERIC_STATS, ci, flags=T.FLAG_VARIANCE), ("stats", ci, True))
            elif "stats" in picks:
                self.add(spec(T.NUMERIC_STATS, ci), ("stats", ci, False))
            exact = not numeric  # (a string column's approximate count is its key set's)
            if "mult" in picks:
                self.add(spec(T.DISTINCT, ci, flags=T.FLAG_MULTIPLICITY), ("distinct", ci, True))
                exact = True
            elif "distinct" in picks:
                self.add(spec(T.DISTINCT, ci), ("distinct", ci, False))
                exact = True
            if "approx" in picks:
                # the lane's estimate -- or the exact count where the key set answers (an exact DISTINCT check or
                # variance lanes on the same column, any string column: tests/test_gpu_hll.py)
                self.add(spec(T.APPROX_DISTINCT, ci), ("approx", ci, exact or "var" in picks))
            if "length" in picks:
                lo = int(rng.integers(0, 6))
                hi = None if rng.random() < 0.4 else lo + int(rng.integers(0, 30))
                self.add(spec(T.LENGTH, ci, length_min=lo, length_max=hi), ("length", ci, lo, hi))
            for _ in range(picks.count("regex")):
                pat, opt = PATTERNS[int(rng.integers(0, len(PATTERNS)))]
                flags = {0: 0, "trim": T.FLAG_TRIM, "ci": T.FLAG_CASE_INSENSITIVE, "nullvalid": T.FLAG_NULL_IS_VALID}[opt]
                if rng.random() < 0.5:
                    flags |= T.FLAG_NULL_IS_VALID
                self.add(spec(T.REGEX_MATCH, ci, flags=flags, pattern=pat), ("regex", ci, pat, flags))
        numeric_cols = [ci for ci, c in enumerate(self.cols) if c[0] in ("i", "f")]
        if len(numeric_cols) >= 2 and rng.random() < 0.4:
            self.add(spec(T.COMOMENTS, numeric_cols[0], column2=numeric_cols[1]), ("comoments", numeric_cols[0], numeric_cols[1]))
        if len(numeric_cols) >= 2 and n <= 300_000 and rng.random() < 0.25:
            self.add(spec(T.SPEARMAN, numeric_cols[0], column2=numeric_cols[1]), ("spearman", numeric_cols[0], numeric_cols[1]))
        # (plain layouts here; tuples over Utf8View / dictionary columns are drawn further down, from a stream of their own)
        key_cols = [ci for ci, c in enumerate(self.cols) if c[0] in ("i", "f") or (c[0] == "s" and c[4][2] == "plain")]
        if len(key_cols) >= 2 and n <= 400_000 and rng.random() < 0.3:  # (the check counts tuples in a Python dict)
            mult = bool(rng.integers(0, 2))
            self.add(spec(T.DISTINCT, key_cols[0], columns=key_cols[:int(rng.integers(2, len(key_cols) + 1))],
                          flags=T.FLAG_MULTIPLICITY if mult else 0), ("tuple", tuple(key_cols), mult))
            self.expect[-1] = ("tuple", tuple(self.tuple_columns()), mult)
        for ci, (kind, vals, vb, mask, extra) in enumerate(self.cols):
            if kind in ("f", "i") and rng.random() < 0.15:
                self.add(spec(T.KLL, ci, kll_k=int(rng.choice([200, 2048]))), ("kll", ci))
        # (round 5, from a stream of its own -- earlier seeds keep their cases: tuples whose components are Utf8View or
        #  dictionary columns: the component is the row's string whatever the layout)
        rng6 = np.random.default_rng([seed, 6])
        laid_out = [ci for ci, c in enumerate(self.cols) if c[0] == "s" and c[4][2] != "plain"]
        if laid_out and len(self.cols) >= 2 and n <= 400_000 and not any(e[0] == "tuple" for e in self.expect) and rng6.random() < 0.35:
            first = laid_out[int(rng6.integers(0, len(laid_out)))]
            others = [ci for ci in range(len(self.cols)) if ci != first]
            rng6.shuffle(others)
            cols6 = [first] + others[:int(rng6.integers(1, min(3, len(others)) + 1))]
            rng6.shuffle(cols6)
            mult = bool(rng6.integers(0, 2))
            self.add(spec(T.DISTINCT, cols6[0], columns=cols6, flags=T.FLAG_MULTIPLICITY if mult else 0), ("tuple", tuple(cols6), mult))
            self.expect[-1] = ("tuple", tuple(self.tuple_columns()), mult)
        # thresholds that steer small batches into the big-batch paths (read per call / per state by the library)
        self.env = {}
        if rng.random() < 0.3:
            self.env["TGX_FP_LISTS_MIN_ROWS"] = str(int(rng.choice([1, 3000, 50_000])))
        if rng.random() < 0.3:
            self.env["TGX_PARTITION_MIN_ROWS"] = str(int(rng.choice([1, 5000, 100_000])))
        if rng.random() < 0.3:
            self.env["TGX_COALESCE_FLUSH_ROWS"] = str(int(rng.choice([10_000, 20_000, 100_000])))
        # batching
        self.mode = str(rng.choice(["one", "cuts", "stream"], p=[0.35, 0.4, 0.25]))
        self.device = str(rng.choice(["device", "host", "mixed"], p=[0.5, 0.3, 0.2]))
        has_spearman = any(e[0] == "spearman" for e in self.expect)
        self.after = str(rng.choice(["finalize", "blob", "merge", "ranks"], p=[0.4, 0.15, 0.25, 0.2]))
        if host_only:  # (no torch in the process: HOST buffers only, no threaded ranks -- tools/run_gpu_host_asan.sh)
            self.device = "host"
            if self.after == "ranks":
                self.after = "finalize"
        if has_spearman and self.after in ("blob", "merge"):
            self.after = "finalize"  # (not mergeable: TG/analyzers/advanced/correlation.rs:103-109)
        if self.mode == "one" or n == 0 or self.after == "ranks":
            self.cuts = [0, n]
        elif self.mode == "cuts":
            inner = sorted(int(x) for x in rng.integers(0, n + 1, size=int(rng.integers(1, 6))))
            self.cuts = [0] + inner + [n]
        else:
            step = int(rng.choice([8192, 8192, 65536, 1000]))
            self.cuts = list(range(0, n, step)) + [n]
        # what else happens to a state that is simply finalized: nothing / read half-way and fed on ("the state stays
        # usable", include/tgx.h) / tgx_state_sync between batches / reset and fed the same table again, backwards
        self.seq = str(rng.choice(["plain", "resume", "sync", "reuse"], p=[0.4, 0.25, 0.15, 0.2])) \
            if self.after == "finalize" else "plain"
        if self.after == "ranks":
            self.world = int(rng.integers(2, 5))
            inner = sorted(int(x) // 64 * 64 for x in rng.integers(0, n + 1, size=self.world - 1))
            self.cuts = [0] + inner + [n]  # one shard per rank (validity bytes are shared: shards start on whole words)
        # ---- round 6, from a stream of its own: the DISTINCT checks ask for EXACT key sets (TGX_FLAG_EXACT_KEYS: string /
        # tuple keys kept with their bytes, equal fingerprints confirmed on them) -- nothing about the results may change,
        # whatever else happens to the state (lists, flushes, merges, blobs, ranks, resume / sync / reuse)
        rng7 = np.random.default_rng([seed, 7])
        self.exact_keys = bool(rng7.random() < 0.5)
        if self.exact_keys:
            for sp in self.specs:
                if sp.kind == T.DISTINCT:
                    sp.flags |= T.FLAG_EXACT_KEYS
        # ---- round 5, drawn from a stream of their own (the cases of earlier seeds stay what they were) ----
        rng5 = np.random.default_rng([seed, 5])
        # HOST batches handed over as TGX_MEM_HOST_RETAINED (kept until the flush): nothing about the results may change
        self.retain = bool(rng5.random() < 0.4)
        # an Int64 column presented as the narrowest Arrow type that holds its values (Int8 .. UInt32: widened on the
        # device; UInt64 / Boolean: COUNT and DISTINCT only) -- the oracle keeps seeing the Int64 values
        self.present = [None] * len(self.cols)
        for ci, (kind, vals, vb, mask, extra) in enumerate(self.cols):
            if kind != "i" or rng5.random() >= 0.3:
                continue
            lo, hi = (int(vals.min()), int(vals.max())) if n else (0, 0)
            keys_only = all(e[0] in ("count", "distinct", "tuple") for e in self.expect if ci in self.columns_of_expect(e))
            fits = [t for t in (np.int8, np.uint8, np.int16, np.uint16, np.uint32)
                    if np.iinfo(t).min <= lo and hi <= np.iinfo(t).max]
            if keys_only and lo >= 0 and hi <= 1 and rng5.random() < 0.5:
                self.present[ci] = "bool"
            elif keys_only and lo >= 0 and rng5.random() < 0.5:
                self.present[ci] = np.uint64
            elif fits:
                self.present[ci] = fits[int(rng5.integers(0, len(fits)))]
        self.draw_two_phase_and_temporal(np.random.default_rng([seed, 8]))
        self.draw_time_gap(np.random.default_rng([seed, 9]))
        self.draw_rules_and_counts(np.random.default_rng([seed, 10]))
        self.host_only = host_only
        self.draw_key_probes(np.random.default_rng([seed, 11]))

    HISTOGRAM_BUCKETS = [1, 2, 5, 10, 100, 999, 1000]
    JOINT_BINS = [2, 5, 10, 127]
    NEW_KINDS_MAX_ROWS = 400_000  # (the references walk the table in Python and numpy; the limit of the tuples)

    def draw_two_phase_and_temporal(self, rng8):
        """HISTOGRAM, JOINT_BINS and TEMPORAL checks, from a stream of their own: every earlier draw of the seed -- rng5's
        presentations above included, which saw the older expectations only -- is what it was.  A column presented as
        UInt64 or Boolean is TGX_UNSUPPORTED for the two-phase kinds and is not drawn for them (Int8 .. UInt32 are
        widened and stay); a column a TEMPORAL check reads arrives as Int64 whatever rng5 drew for it."""
        self.phase, self.pass_two, self._cache, self.tables = 1, {}, {}, 1
        n = self.n
        if n > self.NEW_KINDS_MAX_ROWS:
            return
        numeric = [ci for ci, c in enumerate(self.cols) if c[0] in ("i", "f", "i32", "f32")
                   and not (self.present[ci] == "bool" or self.present[ci] is np.uint64)]
        ints = [ci for ci, c in enumerate(self.cols) if c[0] == "i"]
        if numeric and rng8.random() < 0.45:
            for _ in range(1 + int(rng8.random() < 0.3)):
                ci = numeric[int(rng8.integers(0, len(numeric)))]
                buckets = int(rng8.choice(self.HISTOGRAM_BUCKETS))
                edges = str(rng8.choice(["exact", "shifted", "uneven"]))
                # (the last field seeds the sample of the uneven edges, drawn when pass two knows the finite values)
                self.add(spec(T.HISTOGRAM, ci), ("histogram", ci, buckets, edges, int(rng8.integers(0, 2**31))))
        if len(numeric) >= 2 and rng8.random() < 0.5:
            cx, cy = (int(c) for c in rng8.permutation(numeric)[:2])
            self.add(spec(T.JOINT_BINS, cx, column2=cy),
                     ("joint", cx, cy, int(rng8.choice(self.JOINT_BINS)), bool(rng8.integers(0, 2))))
        if ints and rng8.random() < 0.5:
            modes = ["time_of_day", "range"] + (["order", "order"] if len(ints) >= 2 else [])
            mode = modes[int(rng8.integers(0, len(modes)))]
            cols = [int(c) for c in rng8.permutation(ints)]
            ci, cj = cols[0], (cols[1] if mode == "order" else -1)
            keep, weekdays = bool(rng8.integers(0, 2)), bool(rng8.integers(0, 2))
            delta = [0, 1, -1, int(rng8.integers(-(2**39), 2**39)), ET.I64_MAX, ET.I64_MIN][int(rng8.integers(0, 6))]
            tps = [1, 10**3, 10**6, 10**9][int(rng8.integers(0, 4))]
            tod_lo, tod_hi = sorted(int(x) for x in rng8.integers(0, 86400 * tps, size=2))
            vals = self.cols[ci][1]
            lo, hi = ((int(vals[int(rng8.integers(0, n))]) if n and rng8.random() < 0.7 else None) for _ in range(2))
            flags = (T.TEMPORAL_KEEP_NULLS if keep else 0) | (T.TEMPORAL_WEEKDAYS_ONLY if weekdays and mode == "time_of_day" else 0)
            if mode == "order":
                params = dict(mode=T.TEMPORAL_ORDER, flags=flags, delta=delta)
            elif mode == "time_of_day":
                params = dict(mode=T.TEMPORAL_TIME_OF_DAY, flags=flags, ticks_per_second=tps, tod_lo=tod_lo, tod_hi=tod_hi)
            else:
                params = dict(mode=T.TEMPORAL_RANGE, flags=flags)
                if lo is not None:
                    params["lo"] = lo
                if hi is not None:
                    params["hi"] = hi
            self.add(spec(T.TEMPORAL, ci, column2=cj), ("temporal", ci, cj, mode, params))
        for e in self.expect:
            if e[0] == "temporal":
                for ci in self.columns_of_expect(e):
                    self.present[ci] = None
            if e[0] in ("histogram", "joint"):
                assert not any(self.present[ci] == "bool" or self.present[ci] is np.uint64 for ci in self.columns_of_expect(e))

    FORCED_SORT_ROUTES = ("two_passes", "three_passes", "chunked_last_pass", "many_stretches")

    def draw_time_gap(self, rng9):
        """TIME_GAP checks, from a stream of their own and without touching anything drawn before (no presentation
        changes: a group column keeps its narrow type, the widened route).  Only for a case that is simply finalized -- a
        state that holds rows refuses blob, merge and allreduce -- and has an Int64 column to serve as timestamps."""
        self.sort_env, self.sort_route = {}, "shipped"
        stamps = [ci for ci, c in enumerate(self.cols) if c[0] == "i" and self.present[ci] is None]
        if self.after != "finalize" or self.n > self.NEW_KINDS_MAX_ROWS or not stamps or rng9.random() >= 0.7:
            return
        groups = [ci for ci, c in enumerate(self.cols) if c[0] == "i32" or (
            c[0] == "i" and not (self.present[ci] == "bool" or self.present[ci] is np.uint64))]

        def pick(a):
            return a[int(rng9.integers(0, len(a)))]

        def group():  # (the timestamp columns are group columns too: `groups` is never empty)
            return pick(groups) if rng9.random() < 0.65 else -1

        t = pick(stamps)
        if rng9.random() < 0.5:
            tasks = [(t, group())]
        elif len(stamps) < 2 or rng9.random() < 0.6:  # the whole table and per group, over one retained column
            tasks = [(t, -1), (t, pick(groups))]
        else:
            tasks = [(t, group()), (pick([ci for ci in stamps if ci != t]), group())]
        many = int(rng9.integers(0, len(tasks))) if rng9.random() < 0.1 else -1  # more than kTimeGapThresholds (8)
        for k, (ct, cg) in enumerate(tasks):
            _, _, gaps = self.reference(("time_gap", ct, cg))
            for _ in range(int(rng9.integers(9, 12)) if k == many else int(rng9.integers(1, 4))):
                how = int(rng9.integers(0, 5)) if len(gaps) else int(rng9.integers(2, 4))
                some = int(gaps[int(rng9.integers(0, len(gaps)))]) if how < 2 else 0  # a gap that occurs (up to 2^64 - 1)
                max_gap = [min(some, EG.I64_MAX), min(some, EG.I64_MAX) - 1, 0, -1, EG.I64_MAX][how]
                self.add(spec(T.TIME_GAP, ct, column2=cg), ("time_gap", ct, cg, max_gap))
        if rng9.random() < 1 / 3:
            from test_gpu_time_gap import SORT_SHAPES  # (the hand tests' forcing environments: read per sort call)

            self.sort_route = pick(self.FORCED_SORT_ROUTES)
            self.sort_env = dict(SORT_SHAPES[self.sort_route][1])

    COUNTING = ("value_counts", "pair_counts", "group_counts", "group_sums")
    RULES_AND_COUNTS = ("rule",) + COUNTING
    MAX_VALUE_BYTES = [256, 256, 20, 4, 1]  # (the shorter ones cut real words: those rows are long rows)
    BOUND_LIMIT = 65536  # TGX_VALUE_COUNTS_MAX_DISTINCT, .._MAX_PAIRS, .._MAX_GROUPS
    LOW_BOUND = 16  # a bound far below most columns' number of keys: 32 slots

    def unsupported_as_key(self, ci):
        return self.present[ci] == "bool" or self.present[ci] is np.uint64

    def draw_rules_and_counts(self, rng10):
        """VALUE_RULE, VALUE_COUNTS, PAIR_COUNTS, GROUP_COUNTS and GROUP_SUMS checks, from a stream of their own and
        without touching anything drawn before (no presentation changes: a column presented as UInt64 or Boolean is
        TGX_UNSUPPORTED as a key or rule column and is not drawn in those roles).  Every `after` and every `seq`: the
        five kinds are additive.  The bounds are drawn against the exact number of keys d of the references -- d, d + 1,
        10000, 65536, sometimes LOW_BOUND -- and key columns (pairs) with d <= 65536 are preferred, so that most tasks
        are compared for full equality (tests/test_fuzz_cases.py holds the share of the others to a quarter)."""
        n = self.n
        if n > self.NEW_KINDS_MAX_ROWS:
            return
        numeric = [ci for ci, c in enumerate(self.cols) if c[0] in ("i", "f", "i32", "f32") and not self.unsupported_as_key(ci)]
        keys = [ci for ci, c in enumerate(self.cols) if c[0] == "s" or (c[0] in ("i", "i32") and not self.unsupported_as_key(ci))]
        strings = [ci for ci, c in enumerate(self.cols) if c[0] == "s"]
        if not (numeric or keys) or rng10.random() >= 0.55:
            return

        def pick(a):
            return a[int(rng10.integers(0, len(a)))]

        def max_value_bytes():
            return int(pick(self.MAX_VALUE_BYTES))

        def bound_for(d):
            how = str(rng10.choice(["d", "d+1", "10000", "65536", "low"], p=[0.27, 0.27, 0.09, 0.33, 0.04]))
            bound = {"d": d, "d+1": d + 1, "10000": 10000, "65536": self.BOUND_LIMIT, "low": self.LOW_BOUND}[how]
            return min(max(bound, 1), self.BOUND_LIMIT)

        def key_column(mvb):
            """a key column, one with at most BOUND_LIMIT keys if there is one (nine times in ten)"""
            ci = pick(keys)
            fits = [c for c in keys if self.reference(("value_counts", c, mvb))["distinct"] <= self.BOUND_LIMIT]
            if fits and ci not in fits and rng10.random() < 0.9:
                ci = pick(fits)
            return ci

        kinds = [k for k, possible in (("rule", numeric), ("value_counts", keys), ("pair_counts", strings),
                                       ("group_counts", keys), ("group_sums", keys and numeric)) if possible]
        # (a table none of whose key columns has at most BOUND_LIMIT keys can only overflow: those tasks are drawn, but
        #  less often, so that three tasks in four of a kind stay pinned by their references)
        tight = bool(keys) and all(self.reference(("value_counts", c, 256))["distinct"] > self.BOUND_LIMIT for c in keys)
        often = {k: 0.12 if tight and k in ("value_counts", "group_counts", "group_sums") else 0.5 for k in kinds}
        chosen = [k for k in kinds if rng10.random() < often[k]] or [pick([k for k in kinds if often[k] == 0.5] or kinds)]
        if "rule" in chosen:
            ci = pick(numeric)
            is_float = self.cols[ci][0] in ("f", "f32")
            wide, live = self.wide_of(ci), np.flatnonzero(self.cols[ci][3])
            for _ in range(9 if rng10.random() < 0.12 else int(rng10.integers(1, 4))):  # (nine: a second launch group)
                mode = int(pick([T.RULE_GE_ZERO, T.RULE_GT_ZERO, T.RULE_BETWEEN, T.RULE_BETWEEN, T.RULE_INTEGER]))
                rule = EV.rule(mode)
                if mode == T.RULE_BETWEEN:
                    # bounds from the column's own values (NaN and both zeros included on float columns), in order by the
                    # rule's own comparison three times in four -- lo > hi matches nothing
                    a, b = ((wide[int(pick(live))] if len(live) and rng10.random() < 0.9 else wide.dtype.type(0)) for _ in range(2))
                    as_double = is_float or bool(rng10.integers(0, 2))
                    if as_double:
                        a, b = float(a), float(b)
                        ka, kb = EV.key(EV.bits_of(a)), EV.key(EV.bits_of(b))
                    else:
                        ka, kb = a, b = int(a), int(b)
                    if (ka > kb) != (rng10.random() < 0.25):
                        a, b = b, a
                    flags = T.RULE_BOUNDS_AS_DOUBLE if as_double and (not is_float or rng10.random() < 0.5) else 0
                    rule = EV.rule(mode, flags, *((0, 0, a, b) if as_double else (a, b, 0.0, 0.0)))
                self.add(spec(T.VALUE_RULE, ci), ("rule", ci, rule))
        if "value_counts" in chosen:
            mvb = max_value_bytes()
            ci = key_column(mvb)
            bound = bound_for(self.reference(("value_counts", ci, mvb))["distinct"])
            self.add(spec(T.VALUE_COUNTS, ci), ("value_counts", ci, bound, mvb))
        if "group_counts" in chosen:
            mvb = max_value_bytes()
            ck = key_column(mvb)
            bound = bound_for(self.reference(("value_counts", ck, mvb))["distinct"])
            # (specs that share the group column and both bounds share one walk: its members)
            for _ in range(int(rng10.integers(1, 4))):
                cv = ck if rng10.random() < 0.2 else int(rng10.integers(0, len(self.cols)))
                self.add(spec(T.GROUP_COUNTS, cv, column2=ck), ("group_counts", cv, ck, bound, mvb))
        if "group_sums" in chosen:
            mvb = max_value_bytes()
            ck = key_column(mvb)
            bound = bound_for(self.reference(("value_counts", ck, mvb))["distinct"])
            cv = ck if ck in numeric and rng10.random() < 0.2 else pick(numeric)
            if self.cols[cv][0] in ("f", "f32"):
                # (a NaN, an infinity or magnitudes that add up beyond DBL_MAX leave a group to the overflow rule: such
                #  a column keeps its task half the time, so that the sum bound decides three float tasks in four)
                with np.errstate(over="ignore", invalid="ignore"):
                    total = float(np.abs(self.doubles_of(cv)[self.cols[cv][3]]).sum())
                if not math.isfinite(total) and rng10.random() < 0.5:
                    cv = pick(numeric)
            self.add(spec(T.GROUP_SUMS, cv, column2=ck), ("group_sums", cv, ck, bound, mvb))
        if "pair_counts" in chosen:
            mvb = max_value_bytes()
            for attempt in range(3):
                cx = pick(strings)
                cy = pick(numeric) if numeric and rng10.random() < 0.6 else pick(strings)
                if cy in numeric and rng10.random() < 0.5:
                    cx, cy = cy, cx
                e = ("pair_counts", cx, cy, 1, mvb, int(pick(self.JOINT_BINS)), bool(rng10.integers(0, 2)))
                d = self.reference(("pair_counts", cx, cy, mvb, self.pair_binning(e)))["distinct"]
                if d <= self.BOUND_LIMIT or rng10.random() >= 0.9:  # (pairs with at most BOUND_LIMIT keys preferred)
                    break
            self.add(spec(T.PAIR_COUNTS, cx, column2=cy), e[:3] + (bound_for(d),) + e[4:])

    # ---- KEY_PROBE -------------------------------------------------------------------------------------------------------
    KP_PROBING = ("plain", "counted", "strings")
    KP_MODES = KP_PROBING + ("rows",)
    KP_MAX_STRING_KEYS = 20_000  # (a set's digest is a Python fingerprint per distinct key)
    KP_BIG_COUNT = 1 << 40

    def draw_key_probes(self, rng11):
        """KEY_PROBE checks, drawn last, from a stream of their own and without touching anything drawn before.  The
        probing modes (plain, counted, strings) for every `after` and `seq`; a rows spec only for a state that is simply
        finalized (it neither merges nor serializes).  The parent set of a spec is drawn from the child column's own
        distinct values -- none, a few, about half or all of them, strangers, the key -1, duplicates, multiplicities --
        and shaped so that every route occurs; the bound against the exact number of missing keys d of the references.
        What is random when the case RUNS (how a parent column is cut into batches, TGX_FLAG_EXACT_KEYS on its DISTINCT
        spec) comes from kp_rng, never from self.rng: run_device_inner draws what it drew without the dimension."""
        self.kp_rng = np.random.default_rng([self.seed, 12])
        self.kp_set_held, self.kp_key = True, None
        n = self.n
        ints = [ci for ci, c in enumerate(self.cols) if c[0] in ("i", "i32") and not self.unsupported_as_key(ci)]
        strings = [ci for ci, c in enumerate(self.cols) if c[0] == "s"]
        if n > self.NEW_KINDS_MAX_ROWS or not (ints or strings) or rng11.random() >= 0.5:
            return

        def pick(a, p=None):
            return a[int(rng11.choice(len(a), p=p))]

        modes = (["plain", "counted"] if ints else []) + (["strings"] if strings else []) + (
            ["rows"] if ints and self.after == "finalize" else [])
        used = {}  # mode class -> the column of the last spec of it

        def column_for(mode):
            """a column of the mode's type: now and then the one another spec probes; one with at most BOUND_LIMIT keys
            if there is one (nine times in ten), so that most tasks are compared for full equality"""
            of = strings if mode == "strings" else ints
            if (mode == "strings") in used and rng11.random() < 0.4:
                return used[mode == "strings"]
            ci = pick(of)
            fits = [c for c in of if self.reference(("value_counts", c, 256))["distinct"] <= self.BOUND_LIMIT]
            if fits and ci not in fits and rng11.random() < 0.9:
                ci = pick(fits)
            return ci

        def bound_for(d):
            how = pick(["d", "d+1", "10000", "65536", "low"], p=[0.27, 0.27, 0.09, 0.33, 0.04])
            bound = {"d": d, "d+1": d + 1, "10000": 10000, "65536": self.BOUND_LIMIT, "low": self.LOW_BOUND}[how]
            return min(max(bound, 1), self.BOUND_LIMIT)

        def one(mode, ci, shape=None, parent=None, bound=None):
            used[mode == "strings"] = ci
            if mode == "rows":
                self.add(spec(T.KEY_PROBE, ci), ("key_probe", ci, "rows", None, 0, 0))
                return None
            mvb = int(pick(self.MAX_VALUE_BYTES)) if mode == "strings" else 0
            if parent is None:
                parent = (self.draw_string_parent if mode == "strings" else self.draw_int_parent)(rng11, ci, mode, shape)
            e = ("key_probe", ci, mode, parent, 1, mvb)
            if bound is None:
                bound = bound_for(self.reference(self.kp_reference_key(e))["missing_keys"])
            self.add(spec(T.KEY_PROBE, ci), e[:4] + (bound, mvb))
            return self.expect[-1]

        how = rng11.random()
        if how < 0.08:  # nine specs on one column and route: the route's second launch (kSidePerLaunch is 8)
            mode = pick([m for m in modes if m != "rows"])
            ci, shape = column_for(mode), pick(["dense", "stray"])
            for _ in range(9):
                one(mode, ci, shape=shape)
        elif how < 0.23 and ints:  # a plain and a counted spec on the same column and records: they agree apart from the route
            ci = column_for("counted")
            e = one("counted", ci, parent=self.draw_int_parent(rng11, ci, "counted", None, sources=("a", "b")))
            one("plain", ci, parent=e[3], bound=e[4])
            if rng11.random() < 0.5:
                mode = pick(modes)
                one(mode, column_for(mode))
        else:
            for _ in range(int(rng11.integers(1, 4))):
                mode = pick(modes)
                one(mode, column_for(mode))

    def kp_child(self, ci):
        """(keys as int64, validity) of an integer child column: the sign- or zero-extended values"""
        return np.asarray(self.wide_of(ci)).astype(np.int64), self.cols[ci][3]

    def draw_int_parent(self, rng, ci, mode, shape, sources=None):
        counted = mode == "counted"
        child, mask = self.kp_child(ci)
        own = np.unique(child[mask])

        def pick(a, p=None):
            return a[int(rng.choice(len(a), p=p))]

        others = [cj for cj, c in enumerate(self.cols) if cj != ci and c[0] in ("i", "i32") and not self.unsupported_as_key(cj)]
        if shape is None and sources is None and others and rng.random() < 0.2:
            # another column of the table as the parent, in its own Arrow type: an Int32 or narrow export joins an Int64
            # child and the reverse.  A counted set takes its rows (the export knows a key as seen once or more often)
            cj = pick(others)
            values, valid = self.kp_child(cj)
            return ParentSet("c" if counted else "b", values, valid, None, "column %d" % cj, kind=self.cols[cj][0],
                             present=self.present[cj], width=self.kp_width(cj))
        share = pick(["none", "few", "half", "all"], p=[0.15, 0.2, 0.4, 0.25])
        held = {"none": own[:0], "few": own[rng.permutation(len(own))[:int(rng.integers(1, 6))]],
                "half": own[rng.random(len(own)) < 0.5], "all": own}[share]
        lo = int(own[0]) if len(own) else int(rng.integers(-1000, 1000))
        if shape is None:
            shape = pick(["as is", "dense", "stray", "threshold", "empty"], p=[0.3, 0.24, 0.2, 0.2, 0.06])
        limit = 4 if counted else 128  # exact_join_coverage.route_of, exact_key_probe.route_of
        if shape == "empty":
            keys = own[:0]
        elif shape == "as is":  # and strangers below everything the child holds
            m = int(pick([0, 1, 50]))
            keys = np.concatenate([held, lo - 1 - np.arange(m, dtype=np.int64) * int(rng.integers(1, 4))])
        elif shape == "dense":  # a dense range about the child's smallest key: the bitmap, the count array
            m = int(pick([1, 5, 1000, max(1, len(own))]))
            keys = np.concatenate([held, lo - int(pick([0, 1, m // 2])) + np.arange(m, dtype=np.int64)])
        elif shape == "stray":  # a dense range and one key from far away: the hash routes
            m = int(pick([5, 1000]))
            far = lo - (1 << 50) - int(rng.integers(0, 1000))
            while far in own:
                far -= 1
            keys = np.concatenate([held, lo + np.arange(m, dtype=np.int64), [far]])
        else:  # exactly on the route's threshold, or one key's width beyond it
            m = int(pick([2, 7, 1000]))
            keys = np.concatenate([lo + np.arange(m - 1, dtype=np.int64), [lo + limit * m - 1 + int(rng.integers(0, 2))]])
        free = shape not in ("threshold", "empty")
        if free and rng.random() < 0.15:
            keys = np.concatenate([keys, [-1]])  # the table's free-slot marker: an ordinary key
        keys = np.unique(keys.astype(np.int64))
        source = pick(list(sources or (("a", "b", "c") if counted else ("a", "b"))))
        repeat = free and rng.random() < 0.4  # duplicate records, repeated rows
        big = counted and source == "a" and len(keys) > 0 and rng.random() < 0.2
        top = int(pick([2, 6, 3000]))
        nulls = rng.random() < 0.3
        if self.host_only and source == "a":  # (no torch in the process: the records come from an export)
            source, repeat = "b", repeat and not counted
        counts = None
        if source == "a":
            values = np.concatenate([keys, keys[rng.random(len(keys)) < 0.3]]) if repeat else keys
            values = values[rng.permutation(len(values))]
            valid = np.ones(len(values), bool)
            counts = rng.integers(1, top, size=len(values)).astype(np.uint64) if counted else np.ones(len(values), np.uint64)
            if big:
                counts[int(rng.integers(0, len(counts)))] = self.KP_BIG_COUNT
        else:
            if source == "c" and repeat:
                values = np.repeat(keys, rng.integers(1, 4, size=len(keys)))
            elif source == "b" and repeat and not counted:  # (a counted set from an export: every key once)
                values = np.concatenate([keys, keys[rng.random(len(keys)) < 0.3]])
            else:
                values = keys
            values = values[rng.permutation(len(values))]
            valid = rng.random(len(values)) >= 0.1 if nulls and free else np.ones(len(values), bool)
            if source == "b" and counted:  # (a NULL row must not take a key out of the set's one row)
                valid[:] = True
        parent = ParentSet(source, values, valid, counts, "%s of the child's keys, %s" % (share, shape))
        # the matched pairs stay far below 2^64 whatever the rows hold: rows * the largest multiplicity
        assert self.n * max(parent.max_count(), 1) < 1 << 62, (self.seed, self.n, parent.max_count())
        return parent

    def kp_width(self, ci):
        kind, p = self.cols[ci][0], self.present[ci]
        return 4 if kind == "i32" else 8 if p is None else 1 if p == "bool" else np.dtype(p).itemsize

    def draw_string_parent(self, rng, ci, mode, shape):
        codes, words, mask = self.string_keys(ci)
        text = self.cols[ci][4][3]
        own = np.flatnonzero(np.bincount(codes[mask], minlength=len(words)))

        def pick(a, p=None):
            return a[int(rng.choice(len(a), p=p))]

        share = pick(["none", "few", "half", "all"], p=[0.15, 0.2, 0.4, 0.25])
        held = {"none": own[:0], "few": own[rng.permutation(len(own))[:int(rng.integers(1, 6))]],
                "half": own[rng.random(len(own)) < 0.5], "all": own}[share]
        if len(held) > self.KP_MAX_STRING_KEYS:
            held = held[rng.permutation(len(held))[:self.KP_MAX_STRING_KEYS]]
        strangers = ["stranger %d" % k for k in range(int(pick([0, 1, 20])))] + (["y" * 300] if rng.random() < 0.3 else [])
        empty = shape is None and rng.random() < 0.06
        pwords = [] if empty else [text[int(k)] for k in held] + strangers
        source = pick(["a", "b"])
        repeat, nulls = rng.random() < 0.4, rng.random() < 0.3
        layout = pick([("plain", False), ("plain", True), ("view", False), ("dict", False), ("dict", True)])
        if self.host_only and source == "a":
            source, layout = "b", ("plain", False)
        picks = np.arange(len(pwords))
        if repeat:
            picks = np.concatenate([picks, picks[rng.random(len(picks)) < 0.3]])
        picks = picks[rng.permutation(len(picks))]
        valid = rng.random(len(picks)) >= 0.1 if nulls and source == "b" else np.ones(len(picks), bool)
        if len(picks) > 20_000 and layout[0] != "plain":  # (layouts built row by row: small columns only)
            layout = ("plain", layout[1])
        near = []
        if not empty and rng.random() < 0.3:  # (drawn whatever the source is: the draws after it stay what they are)
            missing = np.setdiff1d(own, held)
            near = [words[int(k)] for k in missing[rng.permutation(len(missing))[:3]]]
        return ParentSet(source, picks, valid, None, "%s of the child's words%s" % (share, ", empty" if empty else ""),
                         words=pwords, layout=layout, near=near)

    def kp_reference_key(self, e):
        return ("key_probe", e[1], e[2], e[3], e[5])

    def kp_specs(self):
        return [(si, e) for si, e in enumerate(self.expect) if e[0] == "key_probe" and e[2] != "rows"]

    def kp_digest(self, parent):
        """parent_digest of a set of strings under the running plan's fingerprint key"""
        cache = self.__dict__.setdefault("_kp_digests", {})
        k = (self.kp_key, id(parent))
        if k not in cache:
            import fp_reference

            near = [fp_reference.fingerprint(self.kp_key, w) for w in parent.near]
            cache[k] = (EKS.parent_digest(self.kp_key, parent.distinct_values()) + sum(
                EKP.mix64(EKP.mix64(a ^ EKP.DIGEST_SALT) ^ b) for fa, fb in near for a, b in ((fa, fb ^ 1), (fa ^ 1, fb)))) & EKP.M64
        return cache[k]

    def kp_build_sets(self, plan):
        """[(spec index, device pointer, n_records)] of the plan's probing specs: the records of every parent set, made
        once per run -- by hand, by a DISTINCT export of a second plan and state that walk the parent's column (the
        production path of foreign_key.cpp), or by a rows spec that gathers it (join_coverage.cpp's).  What owns the
        records stays in self.kp_keep until the run is over"""
        self.kp_key, self.kp_keep = plan.fingerprint_key(), []
        made, sets = {}, []
        for si, e in self.kp_specs():
            parent = e[3]
            if id(parent) not in made:
                made[id(parent)] = self.kp_records(parent)
            ptr, n = made[id(parent)]
            assert n == parent.n_records(), (e, "records handed out", n, "expected", parent.n_records())
            sets.append((si, ptr, n))
        return sets

    def kp_records(self, parent):
        rng = self.kp_rng
        if parent.source == "a":
            if parent.words is not None:
                fps = parent.fingerprints(self.kp_key)
                recs = np.zeros((len(fps), 4), np.uint64)
                recs[:, :2] = np.array(fps, np.uint64).reshape(len(fps), 2)
                recs[:, 2] = 1
            else:
                recs = np.stack([parent.values.view(np.uint64), parent.counts], axis=1)
            if not len(recs):
                return None, 0
            d = to_device(np.ascontiguousarray(recs).reshape(-1))
            self.kp_keep.append(d)
            return d.data_ptr(), len(recs)
        if parent.source == "b":
            flags = T.FLAG_EXACT_KEYS if rng.random() < 0.5 else 0
            pplan = T.Plan([spec(T.DISTINCT, 0, flags=flags | (T.FLAG_MULTIPLICITY if rng.random() < 0.5 else 0))])
            if parent.words is not None:
                pplan.set_fingerprint_key(self.kp_key)
        else:
            pplan = T.Plan([spec(T.KEY_PROBE, 0)])
            pplan.set_key_probe_rows(0)
        pst = T.State(pplan)
        buf, rows = parent.buffers(self.seed), len(parent.values)
        cuts = [0] + sorted(int(x) for x in rng.integers(0, rows + 1, size=int(rng.integers(0, 3)))) + [rows]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if hi > lo:
                cols = [buf.column(self.device != "host", lo, hi - lo)]
                self.kp_keep.append(cols)
                pst.update(cols)
        self.kp_keep += [pplan, pst, buf]
        if parent.source == "b":
            ptr, counts = pst.distinct_export(0, 1)
            return ptr, counts[0]
        return pst.key_probe_rows(0)

    @staticmethod
    def kp_host_records(ptr, n):
        """a rows spec's {key, 1} records; FakeState hands them over as an array, the device as a pointer"""
        if isinstance(ptr, np.ndarray):
            return ptr
        if not n:
            return np.zeros((0, 2), np.uint64)
        import torch

        class P:
            __cuda_array_interface__ = {"shape": (n * 16,), "typestr": "|u1", "data": (ptr, False), "version": 2}

        return torch.as_tensor(P(), device="cuda").clone().cpu().numpy().view(np.uint64).reshape(n, 2)

    def check_key_probe(self, e, si, r, st):
        _, ci, mode, parent, bound, mvb = e
        if mode == "rows":
            child, mask = self.kp_child(ci)
            summary, entries = st.key_probe(si)
            want = dict(dict.fromkeys(summary, 0), seen=self.n, non_null=int(mask.sum()), null_rows=int((~mask).sum()))
            assert (summary, entries) == (want, {}), (e, summary, entries, want)
            assert (r.total, r.non_null) == (self.n, want["non_null"]), (e, "tgx_finalize", r.total, r.non_null)
            ptr, count = st.key_probe_rows(si)
            assert count == want["non_null"], (e, "records gathered", count, want["non_null"])
            if not self.host_only:  # the records as a multiset: the column's non-NULL keys, each with count 1
                recs = self.kp_host_records(ptr, count)
                assert len(recs) == count and (recs[:, 1] == 1).all(), (e, "counts other than 1")
                got = np.sort(np.ascontiguousarray(recs[:, 0]).view(np.int64))
                assert np.array_equal(got, np.sort(child[mask])), (e, "the gathered keys are not the column's")
            return
        want = dict(self.reference(self.kp_reference_key(e)))
        pairs_want = want.pop("pairs_summary", None)
        want_entries = want.pop("entries")
        want.pop("within_bound", None)
        if mode == "strings":
            want.update(max_value_bytes=mvb, parent_digest=self.kp_digest(parent), route=5 if want["parent_keys"] else 0)
        if not self.kp_set_held:  # a merged-into or deserialized state: the set's identity, no set
            want["route"] = 0
        for read in ("first read", "second read"):
            summary, entries = (st.key_probe_strings if mode == "strings" else st.key_probe)(si)
            long_rows = summary.get("long_rows", 0)
            # the three identities of include/tgx.h, and the summary against its entries
            assert summary["seen"] == summary["non_null"] + summary["null_rows"], (e, read, summary)
            assert summary["non_null"] == summary["matched"] + summary["missing_rows"], (e, read, summary)
            assert summary["missing_rows"] == summary["counted"] + summary["overflow_rows"] + long_rows, (e, read, summary)
            assert (summary["missing_keys"], summary["counted"]) == (len(entries), sum(entries.values())), (e, read, summary, len(entries))
            assert (r.total, r.non_null, r.matches, r.distinct) == (
                summary["seen"], summary["non_null"], summary["matched"], summary["missing_keys"]), (
                e, "tgx_finalize", r.total, r.non_null, r.matches, r.distinct, summary)
            # what never depends on the bound, and the set
            for k in ("seen", "non_null", "null_rows", "matched", "missing_rows", "parent_keys", "parent_digest", "route") + (
                    ("long_rows", "max_value_bytes") if mode == "strings" else ()):
                assert summary[k] == want[k], (e, read, k, summary[k], want[k])
            if self.by_equality(e, want["missing_keys"], bound, summary["overflow_rows"]):
                assert summary == want, (e, read, summary, want)
                self.same_map(e, entries, want_entries)
            else:
                self.held_entries(e, entries, want_entries, bound)
            if mode == "counted":
                pairs = st.key_probe_pairs(si)
                assert pairs == pairs_want, (e, read, pairs, pairs_want)
                assert pairs["join_rows"] == pairs["pairs"] + summary["missing_rows"] + summary["null_rows"], (e, read, pairs)
        # a plain and a counted spec over the same records and bound agree apart from the route
        for sj, o in enumerate(self.expect[:si]):
            if o[0] == "key_probe" and o[3] is parent and o[1:2] + o[4:] == e[1:2] + e[4:] and {o[2], mode} == {"plain", "counted"}:
                other, other_entries = st.key_probe(sj)
                if other["overflow_rows"] == 0 == summary["overflow_rows"]:  # (else: which keys found a slot may differ)
                    assert dict(other, route=0) == dict(summary, route=0) and list(other_entries.items()) == list(entries.items()), (
                        e, "differs from spec", sj, other, summary)

    def pair_numeric_side(self, e):
        """0 / 1: the side of a PAIR_COUNTS expectation that is a numeric column (the spec has two phases); None: none"""
        sides = [k for k in (0, 1) if self.cols[e[1 + k]][0] != "s"]
        assert len(sides) < 2, e
        return sides[0] if sides else None

    def pair_binning(self, e):
        """the numeric side's (origin, width, bins) for pass two, from the exact reference's range of the whole table
        (mutual_information.rs:219-233), sometimes with the origin half a width up; None: no numeric side, or no finite
        row"""
        side = self.pair_numeric_side(e)
        if side is None:
            return None
        b = EP.binning_of_range(self.reference(("pair_range", e[1 + side], e[2 - side])), e[5])
        if b is not None and e[6]:
            b = (b[0] + b[1] / 2, b[1], b[2])
        return b

    @staticmethod
    def columns_of_expect(e):
        if e[0] in ("pair_counts", "group_counts", "group_sums"):
            return (e[1],) if e[1] == e[2] else (e[1], e[2])
        if e[0] == "tuple":
            return tuple(e[1])
        if e[0] == "time_gap":
            return (e[1],) if e[2] < 0 or e[2] == e[1] else (e[1], e[2])
        if e[0] in ("comoments", "spearman", "joint") or (e[0] == "temporal" and e[2] >= 0):
            return (e[1], e[2])
        return (e[1],)

    def prefix_case(self, m):
        """the same case over the table's first m rows (what a state read half-way must report)"""
        import copy

        c = copy.copy(self)
        c.n = m
        c.cols = [(k, (v[:m + 1] if k == "s" else v[:m]), vb, mask[:m], extra) for k, v, vb, mask, extra in self.cols]
        c._cache = {}  # (the references of the prefix; pass two's edges and binnings stay the whole table's)
        return c

    def tuple_columns(self):
        s = self.specs[-1]
        return [s.columns[k] for k in range(s.n_columns)]

    def add(self, s, e):
        self.specs.append(s)
        self.expect.append(e)

    def describe(self):
        cols = ", ".join("%s%s/nulls=%d" % (c[0], "" if p is None else "as" + (p if isinstance(p, str) else p.__name__),
                                            int((~c[3]).sum())) for c, p in zip(self.cols, self.present))
        checks = [e[0] if e[0] not in ("histogram", "joint", "temporal", "time_gap", "key_probe") + self.RULES_AND_COUNTS
                  else "%s%r" % (e[0], e[1:]) for e in self.expect]
        return "seed %d: n=%d cols=[%s] checks=%s pass=%d batching=%s(%d) buffers=%s after=%s env=%s%s" % (
            self.seed, self.n, cols, checks, self.phase, self.mode, len(self.cuts) - 1, self.device,
            self.after + ("" if self.seq == "plain" else "/" + self.seq) + (" kept" if self.retain else "") +
            (" exact-keys" if self.exact_keys else ""), self.env,
            " sort=%s%s" % (self.sort_route, self.sort_env) if self.sort_env else "")

    # ---- the device side ----
    def columns_of(self, lo, hi, on_device):
        if not hasattr(self, "buffers"):
            self.buffers = [Buffers(kind, vals, vb, extra, mask, self.seed + k, self.present[k])
                            for k, (kind, vals, vb, mask, extra) in enumerate(self.cols)]
        cols = [b.column(on_device, lo, hi - lo) for b in self.buffers]
        if self.retain and not on_device:
            for c in cols:
                if c.c.mem == T.MEM_HOST:
                    c.c.mem = T.MEM_HOST_RETAINED
                if c.c.dictionary and c.c.dictionary.contents.mem == T.MEM_HOST:
                    c.c.dictionary.contents.mem = T.MEM_HOST_RETAINED
        return cols

    def run_device(self):
        import os

        for k, v in list(self.env.items()) + list(self.sort_env.items()):
            os.environ[k] = v
        try:
            return self.run_device_inner()
        finally:
            for k in list(self.env) + list(self.sort_env):
                os.environ.pop(k, None)

    def draw_sequence(self, rng):
        """what a run that is not sharded over ranks draws before its first batch, in this order: (the number of states,
        the range hints, the batch a resumed state is read before or -1, the batch a blob is taken before or -1)"""
        n_states = int(rng.integers(2, 4)) if self.after == "merge" else 1
        # a declared value range (tgx_distinct_range_hint: what ranks agree on before a sharded run) for some of the
        # single-column uniqueness checks over Int64 columns: the column's true MIN / MAX
        hints = []
        for k, e in enumerate(self.expect):
            if e[0] == "distinct" and self.cols[e[1]][0] == "i" and self.cols[e[1]][3].any() and rng.random() < 0.2:
                v = self.cols[e[1]][1][self.cols[e[1]][3]]
                if int(v.max()) - int(v.min()) < 2**33:
                    hints.append((k, int(v.min()), int(v.max())))
        n_batches = len(self.cuts) - 1
        stop_at = int(rng.integers(0, n_batches + 1)) if self.seq == "resume" else -1
        # a blob taken half-way: the rest of the table is fed to the state rebuilt from it (what an incremental run does
        # with a stored partial state); Spearman states hold their pairs on the device and stay as they are
        blob_at = int(rng.integers(0, n_batches + 1)) if self.after == "blob" and not any(
            e[0] == "spearman" for e in self.expect) else -1
        return n_states, hints, stop_at, blob_at

    def kp_refusal_step(self):
        """will the first pass of this case, as built, take a blob before a batch and meet the refusal of a state without
        its parent sets?  (a look at what draw_sequence will draw, on a copy of the stream)"""
        import copy

        if self.after != "blob" or not self.kp_specs():
            return False
        blob_at = self.draw_sequence(copy.deepcopy(self.rng))[3]
        return 0 <= blob_at < len(self.cuts) - 1

    def run_device_inner(self):
        T.init()
        plan = T.Plan(self.specs)
        self.set_parameters(plan)
        self.tables = 1  # (the tables that counted rows into the state that is read: slots_held)
        # KEY_PROBE: the parent sets' records, once; every state that is FED gets its own set from them
        kp_sets, self.kp_set_held = self.kp_build_sets(plan), True

        def give_sets(state):
            for si, ptr, n_records in kp_sets:
                state.key_probe_set_parent(si, ptr, n_records)

        if self.after == "ranks":
            self.tables = max(1, sum(1 for r in range(self.world) if self.cuts[r + 1] > self.cuts[r]))
            from test_gpu_distributed_sim import _run_ranks

            on_device = self.device != "host"
            shards_of = lambda rank: self.columns_of(self.cuts[rank], self.cuts[rank + 1], on_device)  # noqa: E731
            # every rank's view of the whole table, and its state (which holds the rank's own copy of every set)
            return _run_ranks(self.world, plan, shards_of, prepare=give_sets if kp_sets else None)
        n_states, hints, stop_at, blob_at = self.draw_sequence(self.rng)
        states = [T.State(plan) for _ in range(n_states)]
        for st_k in states:
            give_sets(st_k)
        for st_k in states:
            for k, lo, hi in hints:
                st_k.distinct_range_hint(k, lo, hi)
        keep = []  # device tensors stay alive until the states have been read
        n_batches = len(self.cuts) - 1
        order = list(range(n_batches))
        if self.after == "merge":  # (the states that are given rows)
            self.tables = max(1, len({b * n_states // max(1, n_batches) for b in order if self.cuts[b + 1] > self.cuts[b]}))
        elif blob_at >= 0 and 0 < self.cuts[min(blob_at, n_batches)] < self.n:  # (rows before the blob and a table after it)
            self.tables = 2
        if self.seq == "reuse":  # a first round in the other order, read and thrown away
            for b in reversed(order):
                on_device = self.device == "device" or (self.device == "mixed" and bool(self.rng.integers(0, 2)))
                cols = self.columns_of(self.cuts[b], self.cuts[b + 1], on_device)
                keep.append(cols)
                states[0].update(cols)
            self.check_one(states[0].finalize(), states[0])
            states[0].reset()
            for k, lo, hi in hints:
                states[0].distinct_range_hint(k, lo, hi)
        for b in order:
            if b == stop_at:  # the table so far
                self.prefix_case(self.cuts[b]).check_one(states[0].finalize(), states[0])
            if b == blob_at:
                states[0] = T.State.deserialize(plan, states[0].serialize())
            lo, hi = self.cuts[b], self.cuts[b + 1]
            on_device = self.device == "device" or (self.device == "mixed" and bool(self.rng.integers(0, 2)))
            cols = self.columns_of(lo, hi, on_device)
            keep.append(cols)
            if b == blob_at and kp_sets:
                # the state that came back holds no set: it refuses the batch, naming the first such spec, BEFORE the
                # batch is noted -- so once the same sets are given again every other check of the plan must still come
                # out equal to its reference, coalesced and retained batches included
                try:
                    states[0].update(cols)
                except T.TgxError as err:
                    assert "TGX_INVALID_ARGUMENT" in str(err) and "spec %d:" % kp_sets[0][0] in str(err), err
                else:
                    raise AssertionError("a deserialized state without its parent sets took a batch")
                give_sets(states[0])
            states[b * n_states // max(1, n_batches)].update(cols)
            if self.seq == "sync" and self.rng.random() < 0.3:
                states[0].sync()
        st = states[0]
        if self.after == "merge":
            order = list(self.rng.permutation(n_states))
            st = T.State(plan)  # (it is given no set: it reads `route` 0 under the identity the merged states bring)
            st.merge([states[k] for k in order])
            self.kp_set_held = False
        elif self.after == "blob":
            st = T.State.deserialize(plan, st.serialize())
            self.kp_set_held = False
        res = st.finalize()
        del keep
        return [(res, st)]

    # ---- the two-phase kinds and TEMPORAL: parameters, references ----
    def set_parameters(self, plan):
        """what goes into a plan before its first state: TEMPORAL parameters, and in pass two the edges and binnings"""
        for si, e in enumerate(self.expect):
            if e[0] == "temporal":
                plan.set_temporal(si, **e[4])
            elif e[0] == "time_gap":
                plan.set_time_gap(si, e[3])
            elif e[0] == "rule":
                plan.set_value_rule(si, **e[2])
            elif e[0] == "value_counts":
                plan.set_value_counts(si, max_distinct=e[2], max_value_bytes=e[3])
            elif e[0] == "group_counts":
                plan.set_group_counts(si, max_groups=e[3], max_value_bytes=e[4])
            elif e[0] == "group_sums":
                plan.set_group_sums(si, max_groups=e[3], max_value_bytes=e[4])
            elif e[0] == "key_probe":
                if e[2] == "rows":
                    plan.set_key_probe_rows(si)
                elif e[2] == "strings":
                    plan.set_key_probe_strings(si, max_missing_keys=e[4], max_value_bytes=e[5])
                else:
                    (plan.set_key_probe if e[2] == "plain" else plan.set_key_probe_counted)(si, max_missing_keys=e[4])
            elif e[0] == "pair_counts":
                side = self.pair_numeric_side(e)
                sides = [None, None]
                if side is not None:
                    b = self.pass_two.get(si) if self.phase == 2 else None
                    if b is not None and not self.valid_binning(b):
                        # a range without a finite positive width: refused, as include/tgx.h promises; the spec stays in
                        # its range phase and is compared as in pass one
                        sides[side] = b
                        try:
                            plan.set_pair_counts(si, x=sides[0], y=sides[1], max_pairs=e[3], max_value_bytes=e[4])
                        except T.TgxError as err:
                            assert "TGX_INVALID_ARGUMENT" in str(err), err
                        else:
                            raise AssertionError("%r: set_pair_counts took %r" % (e, b))
                        b = self.pass_two[si] = None
                    sides[side] = "range" if b is None else b
                plan.set_pair_counts(si, x=sides[0], y=sides[1], max_pairs=e[3], max_value_bytes=e[4])
            elif self.phase == 2 and e[0] == "histogram":
                plan.set_histogram_edges(si, self.pass_two[si])
            elif self.phase == 2 and e[0] == "joint":
                b = self.pass_two[si]
                if all(math.isfinite(v) for v in b[:4]) and b[1] > 0.0 and b[3] > 0.0:
                    plan.set_joint_binning(si, *b)
                    continue
                # a range without a finite positive width: refused, as include/tgx.h promises; the spec stays in its
                # range phase and is compared as in pass one
                try:
                    plan.set_joint_binning(si, *b)
                except T.TgxError as err:
                    assert "TGX_INVALID_ARGUMENT" in str(err), err
                else:
                    raise AssertionError("%r: set_joint_binning took %r" % (e, b))
                self.pass_two[si] = None

    @staticmethod
    def valid_binning(b):
        return math.isfinite(b[0]) and math.isfinite(b[1]) and b[1] > 0.0

    def has_two_phases(self):
        return any(e[0] in ("histogram", "joint") or (e[0] == "pair_counts" and self.pair_numeric_side(e) is not None)
                   for e in self.expect)

    def enter_pass_two(self):
        """edges and binnings for every HISTOGRAM / JOINT_BINS / two-phase PAIR_COUNTS spec, from the exact references' ranges
        of the whole table"""
        for si, e in enumerate(self.expect):
            if e[0] == "histogram":
                self.pass_two[si] = self.histogram_edges(e)
            elif e[0] == "joint":
                b = EJ.binning_of_range(self.reference(("joint_range", e[1], e[2])), e[3])
                if b is None:  # no live row: counts over nothing
                    b = (0.0, 1.0, 0.0, 1.0, e[3])
                elif e[4]:  # the origin half a width up: the rows of the lowest half bin fall outside
                    b = (b[0] + b[1] / 2, b[1], b[2] + b[3] / 2, b[3], b[4])
                self.pass_two[si] = b
            elif e[0] == "pair_counts":  # (None: no numeric side, or no finite row -- the spec stays in its range phase)
                self.pass_two[si] = self.pair_binning(e)
        self.phase = 2

    def histogram_edges(self, e):
        _, ci, buckets, how, sample_seed = e
        r = self.reference(("histogram_range", ci))
        if r["n"] == 0:
            return [float(i) for i in range(buckets + 1)]  # 0.0 .. float(buckets)
        exact = EH.edges_of(r["min"], r["max"], buckets)
        assert all(math.isfinite(x) for x in exact), (e, r["min"], r["max"])
        if how == "shifted":  # another table's edges: rows below the first edge take ELSE
            w = EH.bucket_width(r["min"], r["max"], buckets)
            lo, w = r["min"] + 0.37 * w, w * 1.9
            edges = [lo + float(i) * w for i in range(buckets + 1)]
            return edges if all(math.isfinite(x) for x in edges) else exact  # (1e308 in the column: the stretch overflows)
        if how == "uneven":  # a sorted sample of the column's finite values, repeats included: the fallback search
            d = self.doubles_of(ci)[self.cols[ci][3]]
            d = d[np.isfinite(d)]
            return sorted(np.random.default_rng(sample_seed).choice(d, size=buckets + 1).tolist())
        return exact

    def string_keys(self, ci):
        """(index of each row's word, the words as bytes, validity) of a string column, whatever its layout"""
        key = ("string_keys", ci)
        if key not in self._cache:
            extra = self.cols[ci][4]
            self._cache[key] = (np.asarray(extra[4][:self.n], np.int64), [w.encode("utf-8") for w in extra[3]])
        return self._cache[key] + (self.cols[ci][3],)

    def wide_of(self, ci):
        """the 8-byte values the device widens column ci to (exact_widening.py: nothing converted by a float unit)"""
        kind, vals = self.cols[ci][0], self.cols[ci][1]
        return (vals if kind in ("i", "f", "s") else W.widen_int(vals, "int32") if kind == "i32"
                else W.widen_f32_bits(vals).view(np.float64))

    def doubles_of(self, ci):
        """column ci CAST AS DOUBLE (an Int64 beyond 2^53 rounds to nearest even)"""
        return self.wide_of(ci).astype(np.float64)

    def reference(self, key):
        """the exact modules' answers for this case's table, computed once per table"""
        if key not in self._cache:
            what = key[0]
            if what == "histogram_range":
                ci = key[1]
                self._cache[key] = EH.value_range_np(self.doubles_of(ci), self.cols[ci][3])
            elif what == "histogram_counts":
                ci = key[1]
                self._cache[key] = EH.counts_of_np(self.doubles_of(ci), self.cols[ci][3], list(key[2]))
            elif what == "joint_range":
                self._cache[key] = EJ.pair_range_np(self.doubles_of(key[1]), self.doubles_of(key[2]),
                                                    self.cols[key[1]][3] & self.cols[key[2]][3])
            elif what == "joint_counts":
                self._cache[key] = EJ.joint_counts_np(self.doubles_of(key[1]), self.doubles_of(key[2]),
                                                      self.cols[key[1]][3] & self.cols[key[2]][3], key[3])
            elif what == "time_gap":  # (seen, rows, the task's gaps in order): shared by all its thresholds
                ct, cg = key[1], key[2]
                self._cache[key] = EG.gaps_np(self.cols[ct][1], self.cols[ct][3], *(
                    (self.cols[cg][1], self.cols[cg][3]) if cg >= 0 else (None, None)))
            elif what == "value_counts":  # (column, max_value_bytes)
                ci = key[1]
                if self.cols[ci][0] != "s":
                    self._cache[key] = EVC.twin_ints(self.wide_of(ci), self.cols[ci][3])
                else:  # a bincount of the picks over the words, which are distinct by construction
                    codes, words, mask = self.string_keys(ci)
                    per_word = np.bincount(codes[mask], minlength=len(words)).tolist()
                    held = {w: c for w, c in zip(words, per_word) if c and len(w) <= key[2]}
                    long_rows = sum(c for w, c in zip(words, per_word) if len(w) > key[2])
                    self._cache[key] = EVC.summary(self.n, int(mask.sum()), held, long_rows)
            elif what == "group_counts":  # (value column, key column, max_value_bytes)
                cv, ck, mvb = key[1:]
                valid = self.cols[cv][3]
                if self.cols[ck][0] != "s":
                    self._cache[key] = EGC.walk_np(valid, self.wide_of(ck), self.cols[ck][3])
                else:  # the words ranked bytewise stand in for the keys; the rows of long words are a class of their own
                    codes, words, mask = self.string_keys(ck)
                    order = sorted(range(len(words)), key=words.__getitem__)
                    rank = np.empty(len(words), np.int64)
                    rank[order] = np.arange(len(words))
                    is_long = mask & np.array([len(w) > mvb for w in words] + [False], bool)[:-1][codes]
                    s = EGC.walk_np(valid, rank[codes], mask & ~is_long)
                    s["long_rows"], s["long_non_null"] = int(is_long.sum()), int((is_long & valid).sum())
                    s["null_group_rows"] -= s["long_rows"]
                    s["null_group_non_null"] -= s["long_non_null"]
                    s["entries"] = {words[order[k]]: v for k, v in s["entries"].items()}
                    self._cache[key] = s
            elif what == "group_sums":  # (value column, key column, max_value_bytes)
                cv, ck, mvb = key[1:]
                values = self.wide_of(cv)
                if self.cols[ck][0] != "s":
                    codes, words, mask = self.wide_of(ck), None, self.cols[ck][3]
                else:
                    codes, words, mask = self.string_keys(ck)
                self._cache[key] = EGS.walk_np(values, self.cols[cv][3], codes, mask, words, mvb, rules=True)
            elif what == "key_probe":  # (child column, mode, parent set, max_value_bytes)
                ci, mode, parent, mvb = key[1:]
                if mode == "strings":
                    codes, words, mask = self.string_keys(ci)
                    w = EKS.walk_np(codes, words, mask, parent.distinct_values(), mvb)
                    w["parent_keys"] += 2 * len(parent.near)  # (keys of the set that no value has)
                    self._cache[key] = w
                else:
                    child, mask = self.kp_child(ci)
                    keys, counts = parent.records()
                    if mode == "plain":  # (counts are ignored; the route goes by the records handed over)
                        self._cache[key] = EKP.walk_np(child, mask, keys, None, n_records=len(keys))
                    else:
                        s, p = EJC.walk_np(child, mask, list(zip(keys.tolist(), counts.tolist())))
                        self._cache[key] = dict(s, pairs_summary=p)
            elif what == "pair_range":  # (numeric column, the other side's column)
                self._cache[key] = EP.side_range_np(self.doubles_of(key[1]), self.cols[key[1]][3] & self.cols[key[2]][3])
            elif what == "pair_counts":  # (x column, y column, max_value_bytes, the numeric side's binning or None)
                cx, cy, mvb, binning = key[1:]
                sides, args, numeric = [], [], False
                for ci in (cx, cy):
                    if self.cols[ci][0] == "s":
                        codes, words, _ = self.string_keys(ci)
                        sides.append(None)
                        args.append((codes, words))
                    else:
                        numeric = True
                        sides.append(binning)
                        args.append(self.doubles_of(ci))
                if numeric and (binning is None or not self.valid_binning(binning)):
                    # (a numeric side without a binning the library takes: the spec never leaves its range phase)
                    self._cache[key] = dict(distinct=0)
                else:
                    self._cache[key] = EP.walk_np(args[0], args[1], self.cols[cx][3] & self.cols[cy][3], sides[0], sides[1], mvb)
            elif what == "pair_zeros":  # +0.0 AND -0.0 among the finite values of the rows with both sides non-NULL?
                d = self.doubles_of(key[1])[self.cols[key[1]][3] & self.cols[key[2]][3]]
                z = d[d == 0.0]
                self._cache[key] = bool(len(z)) and bool(np.signbit(z).any()) and not bool(np.signbit(z).all())
            elif what == "both_zeros":  # does the column hold +0.0 AND -0.0 among the rows `key[2]` names?
                d = self.doubles_of(key[1])[self.live_mask(key[2])]
                z = d[d == 0.0]
                self._cache[key] = bool(len(z)) and bool(np.signbit(z).any()) and not bool(np.signbit(z).all())
        return self._cache[key]

    def live_mask(self, cols):
        m = np.ones(self.n, bool)
        for ci in cols:
            m &= self.cols[ci][3] & np.isfinite(self.doubles_of(ci))
        return m

    def same_extreme(self, e, name, got, want, ci, live_cols, zeros_key=None):
        """an extreme bit for bit (float.hex: -0.0 is not 0.0).  Only where +0.0 and -0.0 both occur among the rows it
        runs over and it IS zero, either zero stands: they compare equal, and no MIN / MAX is pinned on which it keeps"""
        if want is None:
            assert math.isnan(got), (e, name, got)
        elif want == 0.0 and got == 0.0 and self.reference(zeros_key or ("both_zeros", ci, tuple(live_cols))):
            pass
        else:
            assert float(got).hex() == float(want).hex(), (e, name, got, want)

    def check_histogram(self, e, si, r, st):
        _, ci, buckets, _, _ = e
        want = self.reference(("histogram_range", ci))
        assert (r.total, r.non_null) == (want["total"], want["n"] + want["non_finite"]), (e, r.total, r.non_null, want["total"])
        got = st.histogram_range(si)
        for k in ("total", "nulls", "non_finite"):
            assert got[k] == want[k], (e, k, got[k], want[k])
        if self.phase == 2:
            edges = self.pass_two[si]
            counts = self.reference(("histogram_counts", ci, tuple(edges)))
            have = st.histogram_counts(si)
            if have[0] != counts[0]:
                bad = [(i, a, b) for i, (a, b) in enumerate(zip(have[0], counts[0])) if a != b]
                raise AssertionError((e, "buckets (index, device, exact)", bad[:8], "edges", edges[:4], "..", edges[-2:]))
            assert have[1:] == counts[1:], (e, "else_rows, non_finite", have[1:], counts[1:])
            assert got["n"] == sum(counts[0]) == want["n"], (e, got["n"], want["n"])
            return
        assert got["n"] == want["n"], (e, "n", got["n"], want["n"])
        for k in ("min", "max"):
            self.same_extreme(e, k, got[k], want[k], ci, (ci,))
        bounds, rules = EH.sum_bounds(want), EH.sum_rules(want)
        for k, bound, rule in zip(("sum", "sum_squared"), bounds, rules):
            why = EH.sum_failure(got[k], want[k], bound, rule)
            assert why is None, (e, k, why)

    def check_joint(self, e, si, r, st):
        _, cx, cy, bins, _ = e
        want = self.reference(("joint_range", cx, cy))
        assert r.total == self.n, (e, r.total)
        if self.phase == 2 and self.pass_two[si] is not None:
            cells, outside = self.reference(("joint_counts", cx, cy, self.pass_two[si]))
            have, have_outside = st.joint_counts(si)
            dense = EJ.dense(cells, max(bins, 2))
            if have != dense:
                side = max(bins, 2) + 1
                bad = [((k // side, k % side), a, b) for k, (a, b) in enumerate(zip(have, dense)) if a != b]
                raise AssertionError((e, "cells ((i, j), device, exact)", bad[:8], "binning", self.pass_two[si], len(have)))
            assert have_outside == outside, (e, "outside", have_outside, outside)
            return
        got = st.joint_range(si)
        assert (got["total"], got["n"], got["non_finite"]) == (self.n, want["n"], want["non_finite"]), (e, got, want)
        assert r.non_null == want["n"], (e, r.non_null, want["n"])
        for k, ci in (("x_min", cx), ("x_max", cx), ("y_min", cy), ("y_max", cy)):
            self.same_extreme(e, k, got[k], want[k], ci, (cx, cy))

    def check_temporal(self, e, si, r, st):
        _, ci, cj, _, params = e
        p = dict(params)
        mode = p.pop("mode")
        want = ET.counts_np(mode, p, self.cols[ci][1], self.cols[cj][1] if cj >= 0 else None, self.cols[ci][3],
                            self.cols[cj][3] if cj >= 0 else None)
        got = tuple(st.temporal_counts(si))
        assert got == want, (e, "seen, considered, violations", got, want)
        assert (r.total, r.non_null, r.matches) == (want[0], want[1], want[1] - want[2]), (e, r.total, r.non_null, r.matches, want)

    def check_time_gap(self, e, si, r, st):
        _, ct, cg, max_gap = e
        want = EG.counts_of_gaps(max_gap, *self.reference(("time_gap", ct, cg)))
        for read in ("first read", "cached read"):
            got = tuple(st.time_gap_counts(si))
            assert got == want, (e, read, "seen, rows, gaps, violations, largest_gap", got, want)
        seen, _, gaps, violations, _ = want
        assert (r.total, r.non_null, r.matches) == (seen, gaps, gaps - violations), (e, r.total, r.non_null, r.matches, want)

    # ---- VALUE_RULE and the four counting kinds ----
    def check_rule(self, e, si, r, st):
        _, ci, rule = e
        want = EV.counts_np(rule, self.wide_of(ci), self.cols[ci][3])
        got = tuple(st.value_rule_counts(si))
        assert got == want, (e, "seen, considered, valid, cast_errors", got, want)
        assert (r.total, r.non_null, r.matches, r.distinct) == want, (e, "tgx_finalize", r.total, r.non_null, r.matches, r.distinct, want)

    def slots_held(self, bound):
        """the entries a state can hold at the most: the slots of its table (the smallest power of two >= 2 * bound), once
        per table that counted rows into it -- one, unless states that were given rows are merged, ranks with rows are
        reduced, or a blob taken half-way is fed on: tgx_merge, blobs and tgx_allreduce unite the entries of every
        state (counted_state.h keeps them beside the table), and include/tgx.h promises no limit for the union"""
        slots = 2
        while slots < 2 * bound:
            slots <<= 1
        return slots * self.tables

    def by_equality(self, e, d, bound, overflow_rows):
        """is a counting task compared for full equality?  With d <= bound keys include/tgx.h promises no overflow; with
        more the table may still hold them all, and then nothing is left to invariants either"""
        if d <= bound:
            assert overflow_rows == 0, (e, "overflow_rows with", d, "keys under a bound of", bound, overflow_rows)
        return overflow_rows == 0

    @staticmethod
    def same_map(e, got, want, what="entries"):
        """two maps with their order; the message names the first difference, not 65536 entries"""
        if got != want:
            missing = [k for k in want if k not in got][:4]
            extra = [k for k in got if k not in want][:4]
            other = [(k, got[k], want[k]) for k in want if k in got and got[k] != want[k]][:4]
            raise AssertionError((e, what, "missing", missing, "not in the table", extra, "(key, device, exact)", other,
                                  len(got), len(want)))
        if list(got) != list(want):
            at = next(k for k, (a, b) in enumerate(zip(got, want)) if a != b)
            raise AssertionError((e, what, "order differs at", at, list(got)[at:at + 3], list(want)[at:at + 3]))

    def held_entries(self, e, got, want, bound, count=lambda v: v):
        """a table that overflowed: what it holds are keys of the table, in order, none counted too often"""
        # The integer key -1 takes no slot: its bits are the tables' free-slot marker, so the kernels count its rows in a
        # word of the task beside the table (kernels/valuecounts.hip, groupcounts.hip, groupsums.hip, keyprobe.hip: `marker`)
        # and the readers hand it out as one more entry -- whatever the table holds, and once however many tables were
        # united.  A full table of 32 slots and the key -1 are 33 entries (seeds 3541 and 4275 of the fifth set: a bound of
        # 16 on a column of small integers).  Byte and pair keys have no such entry.
        beside = int(-1 in got)
        assert len(got) - beside <= self.slots_held(bound), (e, "entries held", len(got), "slots", self.slots_held(bound))
        keys = list(got)
        assert all(a < b for a, b in zip(keys, keys[1:])), (e, "entries out of order")
        for k, v in got.items():
            assert k in want, (e, "a key that is not in the table", k, v)
            assert 0 < count(v) <= count(want[k]), (e, "count of", k, v, want[k])

    def check_value_counts(self, e, si, r, st):
        _, ci, bound, mvb = e
        want = self.reference(("value_counts", ci, mvb))
        summary, counts = st.value_counts(si)
        assert (r.total, r.non_null, r.distinct, r.matches) == (
            summary["seen"], summary["non_null"], summary["distinct"], summary["counted"]), (
            e, "tgx_finalize", r.total, r.non_null, r.distinct, r.matches, summary)
        if self.by_equality(e, want["distinct"], bound, summary["overflow_rows"]):
            assert summary == {k: want[k] for k in summary}, (e, summary, {k: want[k] for k in summary})
            self.same_map(e, counts, want["counts"])
            return
        for k in ("seen", "non_null", "long_rows"):
            assert summary[k] == want[k], (e, k, summary[k], want[k])
        assert summary["counted"] + summary["overflow_rows"] + summary["long_rows"] == summary["non_null"], (e, summary)
        assert (summary["distinct"], summary["counted"]) == (len(counts), sum(counts.values())), (e, summary, len(counts))
        self.held_entries(e, counts, want["counts"], bound)

    def check_group_counts(self, e, si, r, st):
        _, cv, ck, bound, mvb = e
        want = self.reference(("group_counts", cv, ck, mvb))
        count_col = int(self.cols[cv][3].sum())
        summary, groups = st.group_counts(si)
        assert (r.total, r.non_null, r.distinct, r.matches) == (summary["seen"], count_col, summary["groups"], summary["counted"]), (
            e, "tgx_finalize", r.total, r.non_null, r.distinct, r.matches, summary)
        if self.by_equality(e, want["groups"], bound, summary["overflow_rows"]):
            assert summary == {k: want[k] for k in summary}, (e, summary, {k: want[k] for k in summary})
            self.same_map(e, groups, want["entries"])
            return
        for k in ("seen", "null_group_rows", "null_group_non_null", "long_rows", "long_non_null"):
            assert summary[k] == want[k], (e, k, summary[k], want[k])
        assert sum(summary[k] for k in ("counted", "null_group_rows", "overflow_rows", "long_rows")) == self.n, (e, summary)
        assert sum(summary[k] for k in ("counted_non_null", "null_group_non_null", "overflow_non_null",
                                        "long_non_null")) == count_col, (e, summary)
        assert (summary["groups"], summary["counted"], summary["counted_non_null"]) == (
            len(groups), sum(g[0] for g in groups.values()), sum(g[1] for g in groups.values())), (e, summary)
        self.held_entries(e, groups, want["entries"], bound, count=lambda v: v[0])
        for k, (total, non_null) in groups.items():
            assert non_null <= min(total, want["entries"][k][1]), (e, "non_null of", k, (total, non_null), want["entries"][k])

    def check_group_sums(self, e, si, r, st):
        _, cv, ck, bound, mvb = e
        want = self.reference(("group_sums", cv, ck, mvb))
        values, valid = self.wide_of(cv), self.cols[cv][3]
        count_col = int(valid.sum())
        is_float = values.dtype == np.float64
        summary, groups = st.group_sums(si)
        classes = ("counted", "null_group", "overflow", "long_rows")
        assert summary["is_float"] == want["is_float"], (e, "is_float", summary["is_float"], want["is_float"])
        assert (r.total, r.non_null, r.distinct, r.matches, bool(r.has_value)) == (
            summary["seen"], count_col, summary["groups"], summary["counted"][0], count_col > 0), (
            e, "tgx_finalize", r.total, r.non_null, r.distinct, r.matches, r.has_value, summary)
        # the identities, overflow or not: every row, every non-NULL value and (integers, wrapping) the sum is in one class
        assert sum(summary[c][0] for c in classes) == summary["seen"] == self.n, (e, summary)
        assert sum(summary[c][1] for c in classes) == count_col, (e, summary)
        assert (summary["groups"], summary["counted"][0], summary["counted"][1]) == (
            len(groups), sum(g[0] for g in groups.values()), sum(g[1] for g in groups.values())), (e, summary)
        if is_float and self.n:
            assert r.sum_i == 0, (e, "sum_i of a float sum", r.sum_i)
            why = self.float_failure(want, "all", r.sum_f)
            assert why is None, (e, "tgx_finalize sum_f", why)
        elif self.n:
            total = EGS.wrap(int(values[valid].view(np.uint64).sum(dtype=np.uint64)))
            assert EGS.wrap(sum(summary[c][2] for c in classes)) == total, (e, "the classes' sums", summary, total)
            assert summary["counted"][2] == EGS.wrap(sum(g[2] for g in groups.values())), (e, "counted sum", summary["counted"])
            assert (r.sum_i, r.sum_f) == (total, float(total)), (e, "tgx_finalize sum", r.sum_i, r.sum_f, total)
        equal = self.by_equality(e, want["groups"], bound, summary["overflow"][0])
        for c in ("null_group", "long_rows") + (("overflow",) if equal else ()):
            self.same_class(e, c, summary[c], want, c, is_float)
        if equal:
            assert summary["groups"] == want["groups"], (e, "groups", summary["groups"], want["groups"])
            if is_float:
                self.same_map(e, {k: g[:2] for k, g in groups.items()}, {k: w[:2] for k, w in want["entries"].items()})
                for k, g in groups.items():
                    self.same_class(e, k, g, want, k, True)
                self.same_class(e, "counted", summary["counted"], want, "counted_class", True)
            else:
                self.same_map(e, groups, want["entries"])
                assert summary["counted"] == want["counted"], (e, "counted", summary["counted"], want["counted"])
            return
        self.held_entries(e, groups, want["entries"], bound, count=lambda v: v[0])
        for k, g in groups.items():
            w = want["entries"][k]
            assert g[1] <= min(g[0], w[1]), (e, "non_null of", k, g, w)
            if g[:2] == w[:2]:  # every row of the group is in the entry: so is its sum
                self.same_class(e, k, g, want, k, is_float)

    def float_failure(self, want, name, got):
        """EGS.float_failure for the entry or class `name` of a GROUP_SUMS reference"""
        c = want["entries"][name] if name in want["entries"] else want[name]
        return EGS.float_failure(got, want["rules"].get(name, ("bound", None)), c[1], c[2], c[3])

    def same_class(self, e, label, got, want, name, is_float):
        """(rows, non_null, sum) of an entry or a class: the counts and an integer sum for equality, a float sum within
        float_bound of math.fsum, or by the overflow rule (exact_group_sums.float_rule)"""
        c = want["entries"][name] if name in want["entries"] else want[name]
        assert tuple(got[:2]) == tuple(c[:2]), (e, label, "rows, non_null", got, c)
        if not is_float:
            assert got[2] == c[2], (e, label, "sum", got, c)
        else:
            why = self.float_failure(want, name, got[2])
            assert why is None, (e, label, "sum", why, got, c)

    def check_pair_counts(self, e, si, r, st):
        _, cx, cy, bound, mvb, _, _ = e
        side = self.pair_numeric_side(e)
        binning = self.pass_two.get(si) if self.phase == 2 else None
        summary, counts = st.pair_counts(si)
        assert (r.total, r.non_null, r.distinct, r.matches) == (
            summary["seen"], summary["both_non_null"], summary["distinct"], summary["counted"]), (
            e, "tgx_finalize", r.total, r.non_null, r.distinct, r.matches, summary)
        if side is not None and binning is None:  # the range phase
            num, other = (cx, cy) if side == 0 else (cy, cx)
            want = self.reference(("pair_range", num, other))
            assert summary == dict(dict.fromkeys(summary, 0), seen=want["seen"], both_non_null=want["both_non_null"]), (e, summary, want)
            assert counts == {}, (e, "entries in the range phase", len(counts))
            got = st.pair_range(si)
            for k in ("seen", "both_non_null", "n", "non_finite"):
                assert got[k] == want[k], (e, k, got[k], want[k])
            for k in ("min", "max"):
                self.same_extreme(e, k, got[k], want[k], num, (), zeros_key=("pair_zeros", num, other))
            return
        want = self.reference(("pair_counts", cx, cy, mvb, binning))
        if self.by_equality(e, want["distinct"], bound, summary["overflow_rows"]):
            assert summary == {k: want[k] for k in summary}, (e, summary, {k: want[k] for k in summary})
            self.same_map(e, counts, want["counts"], "pairs")
            return
        for k in ("seen", "both_non_null", "long_rows", "non_finite", "out_of_range"):
            assert summary[k] == want[k], (e, k, summary[k], want[k])
        assert sum(summary[k] for k in ("counted", "overflow_rows", "long_rows", "non_finite",
                                        "out_of_range")) == summary["both_non_null"], (e, summary)
        assert (summary["distinct"], summary["counted"]) == (len(counts), sum(counts.values())), (e, summary, len(counts))
        self.held_entries(e, counts, want["counts"], bound)

    # ---- the oracle side + comparison ----
    def key_bits(self, ci):
        """(values as the 64-bit patterns DISTINCT compares, validity) of a numeric column"""
        kind, vals, vb, _, _ = self.cols[ci]
        if kind == "i32":
            return vals.astype(np.int64).view(np.uint64), vb
        if kind == "f32":  # (bit-preserving: a signalling NaN is a key of its own, exact_widening.py)
            return W.widen_f32_bits(vals), vb
        return vals.view(np.uint64), vb

    def exact_distinct(self, ci):
        kind, vals, vb, _, extra = self.cols[ci]
        if kind == "s":
            return orc.distinct_utf8(vals.astype(np.int32) if not extra[1] else self.offsets32(vals), extra[0], vb, n=self.n)
        bits, vb = self.key_bits(ci)
        return orc.distinct_bits64(bits, vb, n=self.n)

    @staticmethod
    def offsets32(offsets):
        assert offsets[-1] < 2**31
        return offsets.astype(np.int32)

    def check(self, all_res):
        for res, st in all_res:
            self.check_one(res, st)

    def check_one(self, res, st):
        """res: the results of the case's table; st: the state that gave them (read for its KLL sketches)"""
        n = self.n
        for si, (r, e) in enumerate(zip(res, self.expect)):
            what = e[0]
            if what == "tuple":
                self.check_tuple(r, e)
                continue
            if what in ("histogram", "joint", "temporal", "time_gap", "key_probe") + self.RULES_AND_COUNTS:
                {"key_probe": self.check_key_probe, "histogram": self.check_histogram, "joint": self.check_joint, "temporal": self.check_temporal,
                 "time_gap": self.check_time_gap, "rule": self.check_rule, "value_counts": self.check_value_counts,
                 "pair_counts": self.check_pair_counts, "group_counts": self.check_group_counts,
                 "group_sums": self.check_group_sums}[what](e, si, r, st)
                continue
            kind, vals, vb, mask, extra = self.cols[e[1]]
            wide = (vals if kind in ("i", "f", "s") else W.widen_int(vals, "int32") if kind == "i32"
                    else W.widen_f32_bits(vals).view(np.float64))
            if what == "count":
                c = orc.count(vb, n)
                assert (r.total, r.non_null) == (c.total, c.non_null), (e, r.total, r.non_null)
            elif what == "stats":
                exact_var = None
                if e[2] and int(mask.sum()) > 1 and np.isfinite(wide[mask].astype(np.float64)).all():
                    x = wide[mask].astype(np.longdouble)  # two passes in extended precision
                    exact_var = float(((x - x.mean()) ** 2).sum() / (len(x) - 1))
                self.check_stats(r, orc.stats(wide, vb, n=n), e[2], e, exact_var)
            elif what == "distinct":
                d = self.exact_distinct(e[1])
                assert (r.total, r.non_null, r.distinct) == (d.total, d.non_null, d.distinct), (e, r.distinct, d.distinct)
                if e[2]:
                    assert r.groups_once == d.groups_once, (e, r.groups_once, d.groups_once)
            elif what == "approx":
                c = orc.count(vb, n)
                assert (r.total, r.non_null) == (c.total, c.non_null), e
                if e[2]:
                    want = self.exact_distinct(e[1]).distinct
                else:  # (the independent reference: registers of the widened bits, the estimate in doubles)
                    bits, _ = self.key_bits(e[1])
                    want = H.estimate_double(H.registers(bits, vb, n=n))
                    true = self.exact_distinct(e[1]).distinct
                    assert abs(want - true) <= H.rel_bound(true) * true, (e, want, true)
                assert r.distinct == want, (e, r.distinct, want)
            elif what == "length":
                want = orc.length_count_utf8(self.offsets32(vals), extra[0], vb, n=n, min_chars=e[2], max_chars=e[3])
                assert (r.total, r.matches) == (n, want.matches), (e, r.matches, want.matches)
            elif what == "regex":
                rx = orc.Regex(e[2], case_insensitive=bool(e[3] & T.FLAG_CASE_INSENSITIVE))
                want = rx.count_utf8(self.offsets32(vals), extra[0], vb, n=n, trim=bool(e[3] & T.FLAG_TRIM),
                                     null_is_valid=bool(e[3] & T.FLAG_NULL_IS_VALID))
                assert (r.total, r.matches) == (n, want.matches), (e, r.matches, want.matches)
            elif what == "kll":  # weight, membership, the query rule, rank error; exact below 1024 values
                Q.check_sketch(st, si, Q.kept(wide[mask]), self.specs[si].kll_k, result=r)
            elif what == "comoments":
                _, y, yb, _, _ = self.cols[e[2]]
                o = orc.comoments(vals, y, vb, yb, n=n)
                assert int(r.non_null) == o.n, (e, r.non_null, o.n)
                with np.errstate(all="ignore"):
                    xa, ya = np.abs(np.asarray(vals, dtype=np.float64)), np.abs(np.asarray(y, dtype=np.float64))
                    overflowing = bool(np.isinf(xa).any() or np.isinf(ya).any() or np.isinf(xa.max(initial=0.0) * ya.max(initial=0.0))
                                       or np.isinf(xa.max(initial=0.0) ** 2) or np.isinf(ya.max(initial=0.0) ** 2))
                with np.errstate(all="ignore"):
                    mx, my = float(xa.max(initial=0.0)), float(ya.max(initial=0.0))
                    scales = (mx, my, mx * mx, my * my, mx * my)
                for (got, want), scale in zip(((r.sum_x, o.sum_x), (r.sum_y, o.sum_y), (r.sum_x2, o.sum_x2),
                                               (r.sum_y2, o.sum_y2), (r.sum_xy, o.sum_xy)), scales):
                    # what ANY sum of n doubles of that magnitude can be off by: terms next to DBL_MAX that cancel (seed
                    # 1244830: x = 1e308 twice, against y = -0.47 and 0.47 -- the oracle's extended precision cancels
                    # them exactly, sum_xy = 0.84; products about a pivot of 1e307 leave -35.5, an error of 1e-306 of
                    # the terms) are not a difference between two implementations in doubles
                    # (a product of magnitudes beyond DBL_MAX: the terms are as large as doubles get)
                    slack = 64.0 * max(1, o.n) * 2.0 ** -53 * (scale if math.isfinite(scale) else sys.float_info.max)
                    if math.isfinite(want) and math.isfinite(got) and abs(got - want) <= slack:
                        pass
                    elif math.isinf(got) and overflowing:
                        # (whatever the oracle's extended precision makes of it -- NaN, an infinity, or a finite sum of
                        #  raw products next to DBL_MAX, seed 2302961: -1e307 -- the products about a pivot, and the
                        #  re-basing of a merge, pass through infinity with the sign the pivot's side gives them)
                        pass
                    elif math.isnan(want) and math.isinf(got) and overflowing:
                        # an infinity (or a product beyond DBL_MAX) among the pairs: the raw products the oracle -- and
                        # DataFusion -- adds come out as +inf and -inf and cancel to NaN, the kernels' products about
                        # the pair's pivot overflow with other signs and stay infinite (seed 2001332)
                        pass
                    elif math.isinf(want) and math.isinf(got) and overflowing:
                        # the same with ONE such pair: the raw product is an infinity of the product's sign, the product
                        # about the pivot one of the other sign when the pivot lies on the other side of the small
                        # factor (seed 1006038: x = 2.5, y = 1e308, pivot of x above 2.5: -inf for +inf)
                        pass
                    elif math.isnan(want) or math.isinf(want):
                        assert math.isnan(got) or got == want, (e, got, want)
                    elif abs(want) > 1e300 and math.isinf(got) and (got > 0) == (want > 0):
                        # values next to DBL_MAX (the pool's 1e308, several times): the oracle adds in extended
                        # precision, a sum in doubles -- the kernels', DataFusion's -- passes through infinity for
                        # some orders of the same rows and stays there (seed 705910: -inf for -1.6e308)
                        pass
                    else:
                        assert rel_err(got, want) < TOL or abs(got - want) < 1e-6, (e, got, want)
            elif what == "spearman":
                _, y, yb, _, _ = self.cols[e[2]]
                want = R.spearman(vals, y, vb, yb, n=n)  # RANK() over the totalOrder keys, sums wrapped mod 2^64
                got = (int(r.non_null), r.sum_x, r.sum_y, r.sum_x2, r.sum_y2, r.sum_xy)
                assert got == (want.n,) + want.doubles(), (e, got, want.n, want.wrapped)

    def check_tuple(self, r, e):
        """COUNT(DISTINCT (a, b, ...)): a tuple is a value of its own, NULL components included"""
        n = self.n
        parts = []
        for ci in e[1]:
            kind, vals, vb, mask, extra = self.cols[ci]
            if kind == "s":
                data = extra[0].tobytes()
                col = [data[vals[i]:vals[i + 1]] if mask[i] else None for i in range(n)]
            else:
                bits, _ = self.key_bits(ci)
                col = [int(bits[i]) if mask[i] else None for i in range(n)]
            parts.append(col)
        counts = {}
        for t in zip(*parts):
            counts[t] = counts.get(t, 0) + 1
        assert (r.total, r.distinct) == (n, len(counts)), (e, r.total, r.distinct, len(counts))
        if e[2]:
            once = sum(1 for v in counts.values() if v == 1)
            assert r.groups_once == once, (e, r.groups_once, once)

    @staticmethod
    def check_stats(r, st, variance, e, exact_var=None):
        assert (r.total, r.non_null, bool(r.has_value)) == (st.total, st.non_null, bool(st.has_value)), e
        if not st.has_value:
            return
        if st.is_float:
            assert orc.nan_equal(r.min_f, st.min_f) and orc.nan_equal(r.max_f, st.max_f), (e, r.min_f, st.min_f)
            if not math.isnan(st.min_f):
                assert math.copysign(1, r.min_f) == math.copysign(1, st.min_f), e
            if math.isnan(st.sum_hi) or math.isinf(st.sum_hi):
                assert orc.nan_equal(r.sum_f, st.sum_hi), (e, r.sum_f, st.sum_hi)
                return
            assert rel_err(r.sum_f, st.sum_hi) < TOL or abs(r.sum_f - st.sum_hi) < 1e-6 * st.non_null, (e, r.sum_f, st.sum_hi)
        else:
            assert (r.min_i, r.max_i, r.sum_i) == (st.min_i, st.max_i, st.sum_i_wrapping), (e, r.min_i, st.min_i)
        assert rel_err(r.mean, st.mean) < TOL or abs(r.mean - st.mean) < 1e-9, (e, r.mean, st.mean)
        if variance:
            assert bool(r.has_variance) == bool(st.has_variance), e
            if st.has_variance and not (math.isnan(st.var_samp) or math.isinf(st.var_samp)):
                # The oracle restates DataFusion's online update, which loses digits on offset data (values near 6e11
                # with a spread of 40: 143.50026 for a true 143.5); the device's pivot-shifted sums do not.  So: within
                # 1e-6 of the reference's value, give or take the reference's own distance from the exact one -- and
                # never further from the exact value than the reference is, beyond 1e-7 relative.
                # States and partitions are merged with Chan's update in doubles -- here as in DataFusion's
                # VarianceAccumulator::merge_batch -- whose `delta` of two means carries the means' rounding: an absolute
                # eps * |mean| * sqrt(var) or so, whatever the batching (8 rows near 1e12: 2e-5 on a variance of 6).
                slack = 0.0 if exact_var is None else 4 * abs(st.var_samp - exact_var)
                merge_noise = 32 * 2.2e-16 * abs(st.mean) * math.sqrt(abs(st.var_samp))
                assert abs(r.var_samp - st.var_samp) <= 1e-6 * abs(st.var_samp) + slack + merge_noise + 1e-12, (
                    e, r.var_samp, st.var_samp, exact_var)
                if exact_var is not None:
                    assert abs(r.var_samp - exact_var) <= abs(st.var_samp - exact_var) + 1e-7 * abs(exact_var) + \
                        merge_noise + 1e-12, (e, r.var_samp, st.var_samp, exact_var)


def run_seed(seed, max_rows=2_600_000, host_only=False):
    case = Case(seed, max_rows, host_only)
    try:
        case.check(case.run_device())
        if case.has_two_phases():  # the count phases: the same table through the same machinery, on a fresh plan
            case.enter_pass_two()
            case.check(case.run_device())
    except AssertionError as err:
        raise AssertionError("%s\n%s" % (case.describe(), err)) from None
    except T.TgxError as err:
        raise AssertionError("%s\n%s" % (case.describe(), err)) from None
    return case
