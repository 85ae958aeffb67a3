"""Seeded cases for the pattern kernels (kernels/regex.hip) against RE2, route by route.

One integer seed fixes a case through random.Random(seed) -- no numpy generator, no clock: one string column (Utf8,
LargeUtf8, Utf8View or Dictionary), one to six REGEX_MATCH specs drawn from the grammar and the templates of
tools/fuzz_regex_diff.py with TRIM / NULL_IS_VALID / CASE_INSENSITIVE drawn per spec, zero to two LENGTH specs, for
dictionary columns sometimes a DISTINCT spec (so that the per-row gathers fuse into its pass), value lengths chosen to
force each way a 128-row wave step is fed, and a batching.  Three things are derived from a case WITHOUT a device:

  * the expectation: counts from RE2 (pyarrow.compute.match_substring_regex) and Python's len() over the Python values
    -- nothing of the library in it.  What the oracle VM (orc.Regex) and the host automaton (tgx_regex_is_match) say
    per value is recorded beside it, so that a disagreement names its culprit;
  * the route of every spec: table class (tgx_regex_table_info + launch_regex's thresholds, restated ONCE below), single
    walk or product automaton (regex_plan_finish's grouping replayed through tgx_regex_match_group), counted or not,
    layout, fused gather or not, and the set of feeds its wave steps take (regex.hip's fetch .. walk section replayed
    over the column's offsets / views);
  * the census: which cells of table x layout x {single, product} x feed the committed seeds cover.

How a seed decides its case (Case.__init__, _general, _tiny, _large):

    seed                      kind      what is fixed by arithmetic, the rest is drawn from random.Random(seed)
    1 000 000 + k, k = 0..2   large     table class direct / LDS / global, ~1.2 M rows of values <= 8 bytes, one DEVICE batch
    seed % 8 == 0             tiny      rows = TINY_ROWS[(seed / 8) % 10], layout = utf8 / large / view by (seed / 8) % 3, one
                                        batch (the launch has exactly these rows); three single walks, one per table class
    seed % 40 == 39           fuse      a dictionary column, a DISTINCT spec and six pattern specs (four gathers fuse)
    any other                 general   g = the seed's index among the seeds that are no multiple of 8
                                            = (seed / 8) * 7 + seed % 8 - 1;  stratum = g % 24,  lap = g / 24
                                        layout      = utf8, large, view, dict        by stratum % 4
                                        table class = direct, lds, global            by (stratum / 4) % 3
                                        product automaton asked for                  when stratum >= 12
                                        value profile by lap % 8 (a list per layout), coalesced batches when lap % 4 == 2,
                                        view data buffers 1, 3, 1, 2 by lap % 4, dictionary pool 400, 400, 60 by lap % 3

A targeted draw (_draw) asks tgx_regex_table_info until a pattern of the stratum's table class comes up: the EXPECTATION
never depends on the library, but which patterns a seed draws does.  After a change to the pattern compiler (or to the
grammar) the committed cases are other cases: run --select again, replace SEEDS, and update the counts in
tests/test_regex_cases.py.

tests/test_regex_cases.py tests all this without a device, tests/test_gpu_regex_cases.py runs the seeds on the GPU,
tools/fuzz_regex_device.py any other range of seeds.

    python tests/regex_cases.py --census                 # the census of the committed seeds
    python tests/regex_cases.py --select FIRST COUNT     # which seeds of a range can be committed, and what they add"""
import collections
import contextlib
import ctypes as C
import hashlib
import os
import random
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(_HERE, ".."), _HERE, os.path.join(_HERE, "..", "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle_binding as orc  # noqa: E402
import term_amd as T  # noqa: E402
from _lib_spec import spec  # noqa: E402
from fuzz_regex_diff import pattern, subject, template  # noqa: E402

# ---- the kernel's and the launch's thresholds, restated in ONE place ------------------------------------------------
# tests/test_regex_cases.py::test_thresholds_are_the_sources reads the same numbers out of the sources: when one moves,
# that test fails and names the line to follow here.
DIRECT_MAX_ENTRIES = 4096     # regex_device.cpp upload_dfa: byte-indexed while n_states * 256 <= 4096
LDS_MAX_ENTRIES = 32767       # regex.hip launch_regex: kLdsEntries (and entries * 2 <= 65535)
PRODUCT_MAX_ENTRIES = 16384   # regex_types.h kRegexLdsEntries: what dfa_product may build (regex_plan_finish)
MAX_GROUP = 4                 # regex_types.h kMaxRegexGroup
STEP_ROWS = 128               # regex.hip: a wave step, two rows per lane
STAGE_BYTES = 4096            # regex.hip kStageBytes
INLINE_AREA = 2048            # regex.hip: the inline slots of a view step, 16 bytes a row
INLINE_MAX = 12               # Arrow: a view holds up to 12 bytes itself
DICT_MAX_FUSED = 4            # dict.hip kDictMaxFused (small dictionaries: dict_fuse_capacity answers this)
COALESCE_MAX_ROWS = 1 << 16   # api_internal.h kCoalesceMaxRows: smaller batches are gathered into one before any kernel
# The largest grid launch_regex can choose is 512 rows x 256 CUs x 7 resident workgroups.  The 256 (CUs of an MI355X)
# and the 7 (launch_regex caps the occupancy answer at 7) are READ FROM THE CODE AND THE DATA SHEET, not measured: a
# column with more rows than that makes the persistent grid's loop run a second sweep whatever the occupancy turns out.
GRID_ROWS = 512
N_CU = 256
MAX_RESIDENT = 7
SECOND_SWEEP_ROWS = GRID_ROWS * N_CU * MAX_RESIDENT

TABLES = ["direct", "lds", "global"]
LAYOUTS = ["utf8", "large", "view", "dict"]
PLAIN_FEEDS = ["whole", "half", "lane"]  # whole step staged / one or both halves staged / per-lane global reads
VIEW_FEEDS = ["v-inline+long", "v-long", "v-inline", "v-2buf", "v-span"]
TINY_ROWS = [1, 63, 64, 65, 127, 128, 129, 511, 512, 513]
CUTS = ["one", "cuts", "stream", "merge"]
MEMS = ["device", "host", "mixed"]
FLAG_NAMES = [("TRIM", T.FLAG_TRIM), ("NIV", T.FLAG_NULL_IS_VALID), ("CI", T.FLAG_CASE_INSENSITIVE)]
LARGE_SEEDS = [1_000_000, 1_000_001, 1_000_002]  # the three fixed second-sweep cases: direct, LDS, global table

# Cells no case can reach, by name, with the reason (test_regex_cases.py asserts the reason itself).
UNREACHABLE = {
    "global/*/product/*": "dfa_product is capped at kRegexLdsEntries = %d entries, below launch_regex's %d: a product "
                          "automaton's table always fits LDS, so the MULTI instances with a global table never launch"
                          % (PRODUCT_MAX_ENTRIES, LDS_MAX_ENTRIES),
}


def table_class(n_states, n_classes):
    if n_states * 256 <= DIRECT_MAX_ENTRIES:
        return "direct"
    entries = n_states * n_classes
    return "lds" if entries <= LDS_MAX_ENTRIES and entries * 2 <= 65535 else "global"


# ---- the library's host-side answers ----------------------------------------------------------------------------------
def table_info(pat, flags=0):
    """(n_states, n_classes, len_min, len_max) or None when the engine refuses the pattern"""
    pb = pat.encode()
    ns, nc, lo, hi, err = C.c_uint32(), C.c_uint32(), C.c_int64(), C.c_int64(), T._lib._Error()
    rc = T.lib().tgx_regex_table_info(pb, len(pb), flags, C.byref(ns), C.byref(nc), C.byref(lo), C.byref(hi), C.byref(err))
    return (ns.value, nc.value, lo.value, hi.value) if rc == 0 else None


def validates(pat, flags=0):
    pb, err = pat.encode(), T._lib._Error()
    return T.lib().tgx_regex_validate(pb, len(pb), flags, C.byref(err)) == 0


def host_is_match(pat, flags, value):
    pb, vb, m, err = pat.encode(), value.encode(), C.c_int32(-1), T._lib._Error()
    rc = T.lib().tgx_regex_is_match(pb, len(pb), flags, vb, len(vb), C.byref(m), C.byref(err))
    return bool(m.value) if rc == 0 else None


def would_group(members):
    """members: [(pattern, flags)] of one TRIM flag -> does their product automaton fit (tgx_regex_match_group)"""
    L = T.lib()
    k = len(members)
    enc = [p.encode() for p, _ in members]
    arr, lens = (C.c_char_p * k)(*enc), (C.c_size_t * k)(*[len(e) for e in enc])
    fl = (C.c_uint32 * k)(*[f for _, f in members])
    mask, grouped, err = C.c_uint32(), C.c_int32(), T._lib._Error()
    rc = L.tgx_regex_match_group(arr, lens, fl, k, b"", 0, C.byref(mask), C.byref(grouped), C.byref(err))
    return rc == 0 and bool(grouped.value)


def re2_matches(pat, values):
    """RE2's verdict per value, or None when RE2 refuses the pattern"""
    import pyarrow as pa
    import pyarrow.compute as pc

    try:
        return pc.match_substring_regex(pa.array(values, pa.large_string()), pat).to_pylist()
    except Exception:
        return None


# ---- what the column helpers ask of a numpy Generator, answered from random.Random -----------------------------------
class _Rng:
    def __init__(self, seed):
        self.r = random.Random(seed)

    def integers(self, lo, hi=None, size=None, dtype=None):
        if hi is None:
            lo, hi = 0, lo
        if size is None:
            return self.r.randrange(lo, hi)
        return np.array([self.r.randrange(lo, hi) for _ in range(size)], dtype=dtype or np.int64)

    def permutation(self, n):
        p = list(range(n))
        self.r.shuffle(p)
        return np.array(p, dtype=np.int64)


# ---- values ------------------------------------------------------------------------------------------------------------
PROFILES = ["short", "mid", "w31", "w33", "w65", "spikes", "padded", "bands"]


def _clip(s, nbytes):
    while len(s.encode()) > nbytes:
        s = s[:-1]
    return s


def _value(rng, ascii_only, profile):
    if profile == "short":  # <= 12 bytes: a view holds them itself
        return _clip(subject(rng, ascii_only), INLINE_MAX)
    if profile == "mid":    # 0 .. 40 bytes: inline and long values side by side
        return _clip("".join(subject(rng, ascii_only) for _ in range(rng.randint(0, 5))), 40)
    if profile in ("w31", "w33", "w65"):
        # exactly 31 / 33 / 65 bytes: 128 rows span just under 4096 bytes (whole step staged), just over (two halves), more
        # than 8192 (neither half fits)
        want = int(profile[1:])
        s = ""
        while len(s.encode()) < want:
            s += subject(rng, ascii_only) or "a"
        s = _clip(s, want)
        return s + "a" * (want - len(s.encode()))
    if profile == "padded":  # runs of U+0020 at both ends (and tabs, which TRIM must leave alone)
        core = _clip("".join(subject(rng, ascii_only) for _ in range(rng.randint(0, 3))), 30)
        lead, trail = rng.choice([0, 0, 1, 2, 9, 17]), rng.choice([0, 0, 1, 3, 8, 16])
        return " " * lead + rng.choice(["", "", "\t"]) + core + " " * trail
    raise ValueError(profile)


def _values(rng, n, ascii_only, profile, null_rate, pool):
    """n values; `pool` > 0: drawn from that many distinct ones (dictionary columns, the large cases)"""
    def one(i):
        if profile == "spikes":  # a few values longer than the stage among short ones
            if rng.random() < 0.015:
                return "".join(subject(rng, ascii_only) or "b" for _ in range(rng.randint(900, 1400)))
            return _value(rng, ascii_only, "short")
        if profile == "bands":   # stretches of ~150 rows of one width each: every feed in one column
            band = ["short", "w31", "w33", "w65", "mid", "padded"][(i // 150) % 6]
            return _value(rng, ascii_only, band)
        v = _value(rng, ascii_only, profile)
        return "" if profile in ("short", "mid", "padded") and rng.random() < 0.04 else v

    if pool:
        base = [one(i * 150 if profile == "bands" else i) for i in range(pool)]  # (bands: entry i is of width i % 6)
        vals = rng.choices(base, k=n)
    else:
        vals = [one(i) for i in range(n)]
    if null_rate >= 1.0:
        return [None] * n
    if null_rate > 0:
        vals = [None if rng.random() < null_rate else v for v in vals]
    return vals


# ---- one case ----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, seed):
        self.seed = seed
        rng = random.Random(seed)
        self.kind = "large" if seed in LARGE_SEEDS else "tiny" if seed % 8 == 0 else "fuse" if seed % 40 == 39 else "general"
        self.n_buffers, self.repeat_entries, self.extra_entries, self.pool = 1, False, 0, 0
        self.distinct = False
        self.coalesce = False
        self._memo = {}  # (a case never changes once built: expectation and routes are computed once)
        if self.kind == "large":
            self._large(rng, LARGE_SEEDS.index(seed))
        elif self.kind == "tiny":
            self._tiny(rng, seed // 8)
        else:
            self._general(rng)
        counts = collections.Counter(self.values)
        self.nulls = counts.pop(None, 0)
        self.counts = counts  # distinct non-NULL value -> rows

    # -- draws
    def _flags(self, rng, pat, trim=None):
        f = 0
        if (rng.random() < 0.35) if trim is None else trim:
            f |= T.FLAG_TRIM
        if rng.random() < 0.35:
            f |= T.FLAG_NULL_IS_VALID
        # the case flag only where tools/fuzz_regex_diff.py compares (?i): the pattern does not open with a flag group
        if not pat.startswith("(?") and rng.random() < 0.3:
            f |= T.FLAG_CASE_INSENSITIVE
        return f

    def _draw(self, rng, want=None, kinds=None, trim=None, small=False):
        """one (pattern, flags); `want`: drawn again until its table is of that class (refusals never are)"""
        for _ in range(400):
            if kinds and rng.random() < 0.7:
                pat = template(rng, self.ascii_only, rng.choice(kinds))
            else:
                pat = pattern(rng, self.ascii_only)
            flags = self._flags(rng, pat, trim)
            if want is None:
                return pat, flags
            if len(pat) > 40:
                continue  # (a long draw is a big automaton and a slow compile: not worth asking for its class)
            info = table_info(pat, flags)
            if info is not None and table_class(info[0], info[1]) == want and (not small or info[0] * info[1] <= 2000):
                return pat, flags
        raise RuntimeError("seed %d: no %s pattern in 400 draws" % (self.seed, want))

    KINDS = {"direct": ["tiny"], "lds": ["counted_ascii", "stacked", "counted"], "global": ["word"]}

    def _add_regex(self, pf):
        if pf not in [(s[1], s[2]) for s in self.specs if s[0] == "regex"]:  # (equal specs would share one task)
            self.specs.append(("regex", pf[0], pf[1]))

    def _add_lengths(self, rng, k):
        for _ in range(k):
            lo = rng.choice([0, 0, 1, 3, 12, 31])
            hi = None if rng.random() < 0.3 else lo + rng.choice([0, 1, 9, 20, 34, 60])
            if ("length", lo, hi) not in self.specs:
                self.specs.append(("length", lo, hi))

    def _general(self, rng):
        # the seed's place among the general seeds fixes the stratum -- layout x table class x {single, product} -- and,
        # lap after lap, the value profile: the rest is drawn
        g = (self.seed // 8) * 7 + self.seed % 8 - 1
        stratum, lap = g % 24, g // 24
        self.layout = LAYOUTS[stratum % 4]
        target = TABLES[(stratum // 4) % 3]
        product = stratum >= 12
        if self.kind == "fuse":
            self.layout = "dict"
        self.profile = {"view": ["bands", "mid", "w31", "bands", "w33", "spikes", "padded", "short"],
                        "dict": ["w65", "bands", "w33", "mid", "padded", "w65", "short", "spikes"]}.get(
                            self.layout, ["bands", "w65", "w33", "spikes", "padded", "mid", "short", "bands"])[lap % 8]
        self.ascii_only = rng.random() < 0.5 or target == "global"
        self.coalesce = lap % 4 == 2
        self.cut = rng.choice(CUTS if self.profile in ("short", "mid", "padded") else ["one", "cuts", "merge"])
        self.mem = rng.choice(MEMS)
        if self.cut == "stream":
            self.n = rng.randint(8193, 20000)
        elif self.profile == "bands":
            self.n = rng.randint(1000, 6000)  # (every band at least once)
        else:
            self.n = rng.choice(TINY_ROWS) if rng.random() < 0.1 else rng.randint(130, 6000)
        self.null_rate = rng.choice([0.0, 0.0, 0.03, 0.03, 0.03, 0.03, 1.0] if self.kind == "general" and not product else [0.0, 0.03])
        self.specs = []
        if self.kind == "fuse":
            # more than four pattern specs beside a DISTINCT spec: the first four gathers ride on its pass, the rest run
            # on their own
            self.layout, self.distinct = "dict", True
            for k in range(6):
                self._add_regex(self._draw(rng, rng.choice([None, "direct", "lds"]), self.KINDS["direct"] + self.KINDS["lds"]))
        elif self.null_rate >= 1.0:
            self._add_regex(self._draw(rng, target, self.KINDS[target]))  # (no product: both verdicts cannot occur)
        elif product:
            trim = rng.random() < 0.35
            if target == "global":  # unreachable as a product: a global single first, which nothing can join, then a pair
                self._add_regex(self._draw(rng, "global", self.KINDS["global"], trim))
                target = rng.choice(["direct", "lds"])
            self._add_regex(self._draw(rng, target, ["tiny"] if target == "direct" else ["counted_ascii"], trim, small=True))  # (room for the others)
            if target == "direct":
                # the product's own size is not exported: only a PAIR whose state counts multiply to 16 or fewer is
                # certain to stay byte-indexed (routes()), so the direct stratum draws pairs
                first = table_info(self.specs[-1][1], self.specs[-1][2])[0]
                for _ in range(400):
                    pf = self._draw(rng, "direct", ["tiny"], trim)
                    if first * table_info(*pf)[0] * 256 <= DIRECT_MAX_ENTRIES and pf != self.specs[-1][1:]:
                        break
                self._add_regex(pf)
            else:
                for _ in range(rng.randint(1, 3)):
                    self._add_regex(self._draw(rng, "direct", ["tiny"], trim))
        else:
            self._add_regex(self._draw(rng, target, self.KINDS[target]))
            for _ in range(rng.randint(0, 3)):
                self._add_regex(self._draw(rng, None, ["tiny", "counted_ascii", "stacked", "counted", "word"]))
        self._add_lengths(rng, rng.choice([0, 0, 1, 2]))
        if self.layout == "dict":
            self.distinct = self.distinct or rng.random() < 0.4
            self.pool = [400, 400, 60][lap % 3]
            self.repeat_entries, self.extra_entries = rng.random() < 0.5, rng.choice([0, 0, 3])
        if self.layout == "view":
            self.n_buffers = [1, 3, 1, 2][lap % 4]  # several: some steps find their long values in two buffers
        if self.distinct:
            self.specs.append(("distinct",))
        self.values = _values(rng, self.n, self.ascii_only, self.profile, self.null_rate, self.pool)

    def _tiny(self, rng, k):
        """the tiny row counts, each with one single walk per table class (the TRIM flags differ, so nothing groups)"""
        self.layout = ["utf8", "large", "view"][k % 3]  # (a dictionary column's launch has its ENTRIES' length)
        self.n = TINY_ROWS[k % len(TINY_ROWS)]
        self.ascii_only = True
        self.cut, self.mem = "one", rng.choice(["device", "host"])  # one batch: the launch has exactly these rows
        self.profile = rng.choice(["short", "mid", "w33", "padded"])
        self.null_rate = rng.choice([0.0, 0.03, 0.03])
        self.specs = []
        self._add_regex(self._draw(rng, "global", self.KINDS["global"], trim=False))
        self._add_regex(self._draw(rng, "lds", self.KINDS["lds"], trim=True))
        self._add_regex(self._draw(rng, "direct", self.KINDS["direct"], trim=False))
        self._add_lengths(rng, 1)
        if self.layout == "view":
            self.n_buffers = rng.choice([1, 2])
        self.values = _values(rng, self.n, True, self.profile, self.null_rate, self.pool)

    def _large(self, rng, k):
        """values <= 8 bytes, about 1.2 M rows -- more than SECOND_SWEEP_ROWS: the persistent grid's loop goes round"""
        self.layout = ["utf8", "large", "utf8"][k]
        self.n = 1_200_000 + 4097 * k + 1
        assert self.n > SECOND_SWEEP_ROWS
        self.ascii_only = True
        self.cut, self.mem = "one", "device"
        self.profile, self.null_rate, self.pool = "short8", 0.03, 2048
        pat = [r"[0-9]$", r"^[a-z0-9._-]{3,30}$", r"\bab\b"][k]
        self.specs = [("regex", pat, [T.FLAG_NULL_IS_VALID, T.FLAG_TRIM, 0][k]), ("length", 2, 6)]
        base = [_clip(subject(rng, True), 8) for _ in range(self.pool)]
        vals = rng.choices(base, k=self.n)
        for i in rng.sample(range(self.n), int(self.n * self.null_rate)):
            vals[i] = None
        self.values = vals

    # -- the plan
    def plan_specs(self):
        out = []
        for s in self.specs:
            if s[0] == "regex":
                out.append(spec(T.REGEX_MATCH, 0, flags=s[2], pattern=s[1]))
            elif s[0] == "length":
                out.append(spec(T.LENGTH, 0, length_min=s[1], length_max=s[2]))
            else:
                out.append(spec(T.DISTINCT, 0))
        return out

    # -- the column: built the same way for the host and for the device (the helpers' draws do not depend on where)
    def column(self, device):
        from test_gpu_dictionary import encode
        from test_gpu_regex import utf8_column
        from test_gpu_utf8view import view_column

        rng = _Rng(self.seed * 7919 + 1)
        if self.layout == "view":
            return view_column(self.values, rng, device, n_buffers=self.n_buffers)
        if self.layout == "dict":
            return encode(self.values, rng, extra_entries=["unused-%d" % i for i in range(self.extra_entries)],
                          repeat_entries=self.repeat_entries, large=self.seed % 3 == 0, device=device)
        offs, data, validity = orc.utf8_from_list(self.values)
        return utf8_column(offs, data, validity, device, large=self.layout == "large")

    def bounds(self):
        """[(lo, hi)] of the batches.  Ragged cuts are fed as Arrow slices whose offsets are no multiples of 8 (1, 7 and 9
        among them)"""
        n = self.n
        if self.cut == "one":
            return [(0, n)]
        if self.cut == "merge":
            return [(0, n // 2), (n // 2, n)]
        if self.cut == "stream":
            return [(lo, min(lo + 8192, n)) for lo in range(0, n, 8192)]
        rng = random.Random(self.seed * 31 + 5)
        pts = {1, 7, 9}
        for _ in range(rng.randint(1, 5)):
            p = rng.randrange(0, n + 1)
            pts.add(p if p % 8 else p + 3)
        pts = [0] + sorted(p for p in pts if 0 < p < n) + [n]
        return list(zip(pts[:-1], pts[1:]))

    def on_device(self, batch):
        return {"device": True, "host": False, "mixed": batch % 2 == 0}[self.mem]

    # -- expectation: RE2 and len() over the Python values
    def matched(self, s):
        """what the pattern sees of a value under the spec's flags"""
        return s[1], [v.strip(" ") if s[2] & T.FLAG_TRIM else v for v in self._distinct()]

    def _distinct(self):
        return list(self.counts)

    def expect(self):
        """per spec: (total, matches) -- for DISTINCT (total, distinct); None where RE2 refuses the pattern"""
        if "expect" not in self._memo:
            self._memo["expect"] = self._expect()
        return list(self._memo["expect"])

    def _expect(self):
        out = []
        for s in self.specs:
            if s[0] == "regex":
                pat, subjects = self.matched(s)
                if s[2] & T.FLAG_CASE_INSENSITIVE:
                    pat = "(?i)" + pat
                verdicts = re2_matches(pat, subjects) if subjects else []
                if verdicts is None:
                    out.append(None)
                    continue
                m = sum(self.counts[v] for v, hit in zip(self._distinct(), verdicts) if hit)
                out.append((self.n, m + (self.nulls if s[2] & T.FLAG_NULL_IS_VALID else 0)))
            elif s[0] == "length":
                m = sum(c for v, c in self.counts.items() if len(v) >= s[1] and (s[2] is None or len(v) <= s[2]))
                out.append((self.n, m + self.nulls))  # (NULL rows always count: LENGTH(col) BETWEEN .. OR col IS NULL)
            else:
                out.append((self.n, len(self.counts)))
        return out

    def verdict_counts(self, s):
        """(values that match, values that do not) among the non-NULL rows, by RE2"""
        if ("verdicts", s) not in self._memo:
            self._memo["verdicts", s] = self._verdict_counts(s)
        return self._memo["verdicts", s]

    def _verdict_counts(self, s):
        pat, subjects = self.matched(s)
        verdicts = re2_matches(("(?i)" if s[2] & T.FLAG_CASE_INSENSITIVE else "") + pat, subjects) if subjects else []
        hit = sum(self.counts[v] for v, h in zip(self._distinct(), verdicts or []) if h)
        return hit, self.n - self.nulls - hit

    def reference_disagreements(self):
        """RE2 against the oracle VM and the host automaton on every (pattern, flags, value): a list of what differs"""
        bad = []
        for s in self.specs:
            if s[0] != "regex":
                continue
            pat, subjects = self.matched(s)
            ci = bool(s[2] & T.FLAG_CASE_INSENSITIVE)
            want = re2_matches(("(?i)" if ci else "") + pat, subjects) if subjects else []
            if want is None:
                bad.append("RE2 refuses %r" % pat)
                continue
            rx = orc.Regex(pat, case_insensitive=ci)
            for raw, v, w in zip(self._distinct(), subjects, want):
                got_o, got_h = rx.is_match(v), host_is_match(pat, s[2], raw)
                if got_o != w or got_h != w:
                    bad.append("pattern %r flags %d value %r: RE2 %s oracle VM %s host automaton %s" % (pat, s[2], raw, w, got_o, got_h))
        return bad

    def refused(self):
        """the patterns RE2 or tgx_regex_validate refuse, with and without their flags: must be empty for a committed seed"""
        out = []
        for s in self.specs:
            if s[0] != "regex":
                continue
            for f in {0, s[2]}:
                if not validates(s[1], f):
                    out.append("tgx_regex_validate refuses %r (flags %d)" % (s[1], f))
            for p in {s[1], ("(?i)" if s[2] & T.FLAG_CASE_INSENSITIVE else "") + s[1]}:
                if re2_matches(p, ["a"]) is None:
                    out.append("RE2 refuses %r" % p)
        return out

    # -- routes
    def groups(self):
        """regex_plan_finish replayed: spec index -> ('single' | 'product', members).  Same column (there is one), same
        TRIM flag, greedy in spec order, at most four members; a counted automaton is walked alone (dfa_product refuses it)"""
        idx = [i for i, s in enumerate(self.specs) if s[0] == "regex"]
        group_of = {}
        for a, i in enumerate(idx):
            if i in group_of:
                continue
            members = [i]
            for j in idx[a + 1:]:
                if len(members) >= MAX_GROUP:
                    break
                if j in group_of or (self.specs[i][2] ^ self.specs[j][2]) & T.FLAG_TRIM:
                    continue
                if would_group([(self.specs[m][1], self.specs[m][2]) for m in members + [j]]):
                    members.append(j)
            if len(members) >= 2:
                for m in members:
                    group_of[m] = members
        return {i: ("product", group_of[i]) if i in group_of else ("single", [i]) for i in idx}

    def segments(self):
        """[(feed, the values walked that way)]: regex.hip's fetch .. walk section replayed over what each launch sees --
        the rows of every batch, or, for a dictionary column, the ENTRIES (every batch walks them all); None where the
        library coalesces the batches first (the kernel then sees its gathered copy, not these buffers)"""
        if "segments" not in self._memo:
            self._memo["segments"] = self._segments()
        return self._memo["segments"]

    def _segments(self):
        if self.coalesce and self.n <= COALESCE_MAX_ROWS:
            return None
        keep = self.column(False)._keep
        out = []
        if self.layout == "view":
            views = np.asarray(keep[0]).view(np.int32).reshape(-1, 4)
            valid = orc.unpack_validity(keep[1], len(views)) if keep[1] is not None else np.ones(len(views), bool)
            for lo, hi in self.bounds():
                out += [(f, self.values[lo + a:lo + b]) for a, b, f in view_steps(views[lo:hi], valid[lo:hi])]
        elif self.layout == "dict":
            entries = self.entries()
            out += [(f, entries[a:b]) for a, b, f in plain_steps(np.asarray(keep[4]._keep[2]), 0, len(entries))]
        else:
            for lo, hi in self.bounds():
                out += [(f, self.values[a:b]) for a, b, f in plain_steps(np.asarray(keep[2]), lo, hi)]
        return out

    def entries(self):
        """the dictionary's entries, decoded from the column that is fed"""
        d = self.column(False)._keep[4]._keep
        offs, data = np.asarray(d[2]), np.asarray(d[3]).tobytes()
        return [data[int(offs[i]):int(offs[i + 1])].decode() for i in range(len(offs) - 1)]

    def launch_lengths(self):
        """d.length of every regex_match_kernel launch: the batches' rows, or a dictionary's entries; none derivable
        when the library coalesces"""
        if self.coalesce and self.n <= COALESCE_MAX_ROWS:
            return []
        if self.layout == "dict":
            return [len(self.entries())]
        return [hi - lo for lo, hi in self.bounds() if hi > lo]

    def feeds(self):
        """the feeds the wave steps of this case's launches take (the same for every pattern spec: one column)"""
        seg = self.segments()
        return {"coalesced"} if seg is None else {f for f, _ in seg}

    def feed_verdicts(self, s):
        """feed -> (some value walked that way matches, some does not), by RE2 under the spec's flags"""
        if ("feed_verdicts", s) not in self._memo:
            seg = self.segments() or []
            distinct = sorted({v for _, vals in seg for v in vals if v is not None})
            pat = ("(?i)" if s[2] & T.FLAG_CASE_INSENSITIVE else "") + s[1]
            verdict = dict(zip(distinct, re2_matches(pat, [v.strip(" ") if s[2] & T.FLAG_TRIM else v for v in distinct]) or []))
            out = {}
            for f, vals in seg:
                got = {verdict.get(v) for v in vals if v is not None}
                h, m = out.get(f, (False, False))
                out[f] = (h or True in got, m or False in got)
            self._memo["feed_verdicts", s] = out
        return self._memo["feed_verdicts", s]

    def routes(self):
        """per spec: a dict of route marks (None for DISTINCT)"""
        if "routes" not in self._memo:
            self._memo["routes"] = self._routes()
        return self._memo["routes"]

    def _routes(self):
        groups, feeds = self.groups(), self.feeds()
        tasks = [i for i, s in enumerate(self.specs) if s[0] in ("regex", "length")]
        out = []
        for i, s in enumerate(self.specs):
            if s[0] == "distinct":
                out.append(None)
                continue
            r = {"kind": s[0], "layout": self.layout, "rows": self.n, "cut": self.cut, "mem": self.mem,
                 "second_sweep": self.n > SECOND_SWEEP_ROWS}
            if self.layout == "dict":  # regex_update: the first gathers (in task order) ride on the DISTINCT usage pass
                r["gather"] = "fused" if self.distinct and (self.counts or self.extra_entries) and tasks.index(i) < DICT_MAX_FUSED else "unfused"
            if s[0] == "regex":
                info = table_info(s[1], s[2])
                how, members = groups[i]
                r.update(group=how, members=members, counted=info[3] >= 0, flags=[n for n, f in FLAG_NAMES if s[2] & f],
                         feeds=sorted(feeds), pattern=s[1])
                if how == "single":
                    r["table"] = table_class(info[0], info[1])
                else:
                    # the product's own size is not exported; bounded by its parts: it has every undecided state of every
                    # part (> max states) and at most the product of their state counts
                    sizes = [table_info(self.specs[m][1], self.specs[m][2])[0] for m in members]
                    prod = 1
                    for k in sizes:
                        prod *= k
                    r["table"] = "direct" if prod * 256 <= DIRECT_MAX_ENTRIES else "lds" if (max(sizes) + 2) * 256 > DIRECT_MAX_ENTRIES else "?"
            out.append(r)
        return out

    def describe(self):
        """everything a seed fixes, as one comparable value (the buffers by digest)"""
        col = self.column(False)
        h = hashlib.sha1()

        def eat(keep):
            for b in keep:
                if isinstance(b, np.ndarray):
                    h.update(b.tobytes())
                elif isinstance(b, list):
                    eat(b)
                elif isinstance(b, T.Column):
                    eat(b._keep)
        eat(col._keep)
        return {"seed": self.seed, "kind": self.kind, "layout": self.layout, "rows": self.n, "profile": self.profile,
                "nulls": self.nulls, "ascii": self.ascii_only, "specs": list(self.specs), "cut": self.cut, "mem": self.mem,
                "coalesce": self.coalesce, "bounds": self.bounds(), "values": hashlib.sha1(repr(self.values).encode()).hexdigest(),
                "buffers": h.hexdigest()}

    # -- on the device
    def run(self):
        """feeds the case through the C ABI the way its batching says -> [(total, matches)] per spec"""
        T.init()
        plan = T.Plan(self.plan_specs())
        cols = {}

        def batch(k, lo, hi):
            dev = self.on_device(k)
            if dev not in cols:
                cols[dev] = self.column(dev)
            return cols[dev].sliced(lo, hi - lo)

        with _env("TGX_COALESCE", None if self.coalesce else "0"):  # (read when a state is created)
            bounds = self.bounds()
            if self.cut == "merge":  # two states fed half each, united through serialize -> deserialize -> merge
                st, other = T.State(plan), T.State(plan)
                st.update([batch(0, *bounds[0])])
                other.update([batch(1, *bounds[1])])
                st.merge([T.State.deserialize(plan, other.serialize())])
            else:
                st = T.State(plan)
                for k, (lo, hi) in enumerate(bounds):
                    st.update([batch(k, lo, hi)])
            res = st.finalize()
        return [(r.total, r.distinct) if s[0] == "distinct" else (r.total, r.matches) for s, r in zip(self.specs, res)]


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


# ---- feeds: regex.hip's fetch .. walk section over a column's offsets / views -----------------------------------------
def _fits(begin, end, slack):
    """does [begin, end) fit the stage when the copy starts `slack` bytes early (16-byte blocks by absolute address)"""
    return end - (begin - slack) <= STAGE_BYTES


def _robust(decide):
    """a decision that depends on where a buffer's allocation starts (0 .. 15 bytes of slack in front of the span) is
    only counted when every alignment decides alike; decisions are monotone in the slack"""
    a, b = decide(0), decide(15)
    return a if a == b else None


def plain_steps(offsets, lo, hi):
    """rows [lo, hi) of an offsets column, 128 at a time -> [(first row, end row, feed)], a step or a 64-row half each.
    'whole': the step's values fit the stage; otherwise each half is staged when it fits ('half') or read lane by lane
    from global memory ('lane').  'edge': within 16 bytes of a threshold, where the allocation's alignment decides"""
    out = []
    for g in range(lo, hi, STEP_ROWS):
        mid, end = min(g + 64, hi), min(g + STEP_ROWS, hi)
        b_first, b_half, e_last = int(offsets[g]), int(offsets[mid]), int(offsets[end])
        whole = _robust(lambda s: _fits(b_first, e_last, s))
        if whole is None or whole:
            out.append((g, end, "whole" if whole else "edge"))
            continue
        for r0, r1, b, e in [(g, mid, b_first, b_half)] + ([(mid, end, b_half, e_last)] if end > mid else []):
            fit = _robust(lambda s: _fits(b, e, s))
            out.append((r0, r1, "edge" if fit is None else "half" if fit else "lane"))
    return out


def plain_feeds(offsets, lo, hi):
    return {f for _, _, f in plain_steps(offsets, lo, hi)}


def view_steps(views, valid):
    """rows of a view column (int32 [n, 4]: length, prefix, buffer, offset; `valid` per row), 128 at a time ->
    [(first row, end row, feed)]"""
    out = []
    for g in range(0, len(views), STEP_ROWS):
        v, ok = views[g:g + STEP_ROWS], valid[g:g + STEP_ROWS]
        lens = np.where(ok, v[:, 0], 0)
        long_ = lens > INLINE_MAX
        area = INLINE_AREA if (ok & ~long_).any() else 0
        if not long_.any():
            feed = "v-inline" if area else "v-empty"
        elif len(set(v[long_, 2].tolist())) > 1:
            feed = "v-2buf"  # the step's long values lie in two buffers: not staged
        else:
            first = int(v[long_, 3].min())
            last = int((v[long_, 3].astype(np.int64) + lens[long_]).max())
            staged = _robust(lambda s: last - (first - s) <= STAGE_BYTES - area)
            feed = "edge" if staged is None else ("v-inline+long" if area else "v-long") if staged else "v-span"
        out.append((g, g + len(v), feed))
    return out


def view_feeds(views, valid):
    return {f for _, _, f in view_steps(views, valid)}


# ---- the census --------------------------------------------------------------------------------------------------------
def feeds_of(layout):
    return VIEW_FEEDS if layout == "view" else PLAIN_FEEDS


def requirements():
    """name -> how many (case, spec) pairs (cases, for the batchings) must cover it"""
    req = {}
    for table in TABLES:
        for layout in LAYOUTS:
            for group in ("single", "product"):
                if table == "global" and group == "product":
                    continue  # UNREACHABLE
                for feed in feeds_of(layout):
                    cell = "%s/%s/%s/%s" % (table, layout, group, feed)
                    # ... and both verdicts occur among the values that are walked that way: a walk that always ended
                    # dead (or matched) on one route would not pass
                    req["cell:" + cell] = req["hit:" + cell] = req["miss:" + cell] = 1
        for feed in PLAIN_FEEDS + VIEW_FEEDS:
            for flag, _ in FLAG_NAMES:
                req["flag:%s/%s/%s" % (table, feed, flag)] = 1
        for rows in TINY_ROWS:
            req["tiny:%s/%d" % (table, rows)] = 1
        req["sweep2:%s" % table] = 1
    for where in ("plain", "view", "dict"):
        req["counted:%s" % where] = 1
    for layout in LAYOUTS:
        req["length:%s" % layout] = 1
    req["gather:fused"] = req["gather:unfused"] = 1
    for b in CUTS + MEMS + ["coalesced", "immediate"]:
        req["batching:%s" % b] = 3
    # properties of the generator a later choice of seeds must not lose (all on launches as they arrive)
    for name in ("nulls:all", "value:longer-than-stage", "dict:repeated-entries", "dict:unused-entries"):
        req[name] = 1
    return req


def coverage(case):
    """Counter: requirement name -> (case, spec) pairs of this case that cover it"""
    cov = collections.Counter()
    immediate = not (case.coalesce and case.n <= COALESCE_MAX_ROWS)
    # (DEVICE and HOST buffers can only mix in a case of two batches or more)
    mem = case.mem if case.mem != "mixed" or len(case.bounds()) >= 2 else "device"
    for b in (case.cut, mem, "immediate" if immediate else "coalesced"):
        cov["batching:%s" % b] += 1
    if immediate:
        cov["nulls:all"] += case.null_rate >= 1.0
        cov["value:longer-than-stage"] += any(len(v.encode()) > STAGE_BYTES for v in case.counts)
        if case.layout == "dict":
            entries = case.entries()
            cov["dict:repeated-entries"] += len(set(entries)) < len(entries)
            cov["dict:unused-entries"] += bool(set(entries) - set(case.counts))
    for s, r in zip(case.specs, case.routes()):
        if r is None:
            continue
        if "gather" in r:
            cov["gather:%s" % r["gather"]] += 1
        if r["kind"] == "length":
            cov["length:%s" % r["layout"]] += 1
            continue
        if r["counted"]:
            cov["counted:%s" % {"utf8": "plain", "large": "plain"}.get(r["layout"], r["layout"])] += 1
        if r["table"] == "?":
            continue
        verdicts = case.feed_verdicts(s)
        for feed in r["feeds"]:
            cell = "%s/%s/%s/%s" % (r["table"], r["layout"], r["group"], feed)
            cov["cell:" + cell] += 1
            for flag in r["flags"]:
                cov["flag:%s/%s/%s" % (r["table"], feed, flag)] += 1
            hit, miss = verdicts.get(feed, (False, False))
            cov["hit:" + cell] += hit
            cov["miss:" + cell] += miss
        for rows in set(case.launch_lengths()) & set(TINY_ROWS):  # (the lengths the kernel is LAUNCHED at)
            cov["tiny:%s/%d" % (r["table"], rows)] += 1
        if r["second_sweep"]:
            cov["sweep2:%s" % r["table"]] += 1
    return +cov  # (without the zeros)


def census(coverages):
    total = collections.Counter()
    for c in coverages:
        total.update(c)
    return total


def missing(coverages):
    """the requirements the cases do not meet, by name"""
    total = census(coverages)
    return sorted(k for k, need in requirements().items() if total[k] < need)


def product_verdict_gaps(case):
    """members of a product automaton that match every row or none: a walk that lost one pattern's bit would pass"""
    out = []
    for i, r in enumerate(case.routes()):
        if r and r["kind"] == "regex" and r["group"] == "product":
            hit, miss = case.verdict_counts(case.specs[i])
            if not (hit and miss):
                out.append("seed %d spec %d %r: %d rows match, %d do not" % (case.seed, i, case.specs[i][1], hit, miss))
    return out


# ---- the comparison ----------------------------------------------------------------------------------------------------
def disagreements(case, got):
    """got: [(total, matches)] per spec -> what differs from the expectation, each with its route"""
    want = case.expect()
    bad = []
    if len(got) != len(want):
        return ["%d results for %d specs" % (len(got), len(want))]
    routes = None
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            bad.append("spec %d %r: RE2 refuses the pattern -- nothing to compare with" % (i, case.specs[i]))
        elif tuple(g) != tuple(w):
            routes = routes or case.routes()
            bad.append("seed %d spec %d %r: device (total, matches) %r, RE2 %r; route %r"
                       % (case.seed, i, case.specs[i], tuple(g), tuple(w), routes[i]))
    return bad


def check(case, got):
    bad = disagreements(case, got)
    assert not bad, "\n".join(bad)


def run_seed(seed):
    case = Case(seed)
    check(case, case.run())
    return case


# The committed seeds (tests/test_gpu_regex_cases.py runs them, tests/test_regex_cases.py holds them to the census).  Chosen
# with --select: a seed whose draw either engine refuses, or whose product automaton has a member that matches every row
# or none, is not in the list.
SEEDS = [0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 13, 16, 17, 18, 19, 20, 21, 23, 24, 25, 29, 31, 32, 35, 36, 37, 38, 40, 44, 48, 52, 53,
         54, 55, 56, 57, 58, 64, 72, 79, 84, 85, 87, 88, 90, 97, 105, 108, 113, 126, 129, 136, 146, 149, 160, 164, 170, 192, 193,
         199, 204, 259, 273, 328, 337, 400]


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--census", action="store_true")
    ap.add_argument("--select", nargs=2, type=int, metavar=("FIRST", "COUNT"))
    args = ap.parse_args()
    if args.select:
        req = requirements()
        have = census(coverage(Case(s)) for s in LARGE_SEEDS)
        kept = []
        for seed in range(args.select[0], args.select[0] + args.select[1]):
            try:
                case = Case(seed)
            except RuntimeError as e:
                print("# %s" % e)
                continue
            why = case.refused() or product_verdict_gaps(case)
            if why:
                print("# seed %d left out: %s" % (seed, why[0]), flush=True)
                continue
            for finding in case.reference_disagreements()[:3]:
                print("# FINDING seed %d: %s" % (seed, finding))
            cov = coverage(case)
            new = sorted(k for k in cov if k in req and have[k] < req[k])
            if new:
                kept.append(seed)
                have.update(cov)
            print("%d  %s %s %d rows %s %s/%s%s  +%d: %s" % (seed, case.kind, case.layout, case.n, case.profile, case.cut, case.mem,
                                                        " coalesced" if case.coalesce else "", len(new), " ".join(new[:6])))
        print("# seeds that each added a cell: %r" % kept)
        print("# still missing: %s" % " ".join(k for k in sorted(req) if have[k] < req[k]))
        return 0
    covs = [coverage(Case(s)) for s in SEEDS + LARGE_SEEDS]
    total = census(covs)
    print("%d seeds + %d large cases; cell -> (case, spec) pairs" % (len(SEEDS), len(LARGE_SEEDS)))
    for k in sorted(set(total) | set(requirements())):
        print("%-40s %d" % (k, total[k]))
    for k, why in UNREACHABLE.items():
        print("%-40s unreachable: %s" % (k, why))
    gaps = missing(covs)
    print("missing: %s" % (" ".join(gaps) or "none"))
    return 1 if gaps else 0


if __name__ == "__main__":
    sys.exit(main())
