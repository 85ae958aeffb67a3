"""CPU: tests/regex_cases.py tested without a device -- the committed seeds build the same case twice, no drawn pattern
is refused by RE2 or by the engine (so every spec of every case is compared: the share that may be skipped is zero), the
three references agree on every (pattern, flags, value), the seeds together cover every reachable cell of table class x
layout x {single, product} x feed (and the flags, tiny row counts, second sweeps, counted routes, gathers and batchings
asked of them), the unreachable cell is named with a reason that is asserted, and both the comparison and the census
fail when they should."""
import collections
import os
import re

import numpy as np
import pyarrow  # noqa: F401  (RE2 is the expectation: not a skip)
import pytest

import regex_cases as R
import term_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SEEDS = 67
N_COMPARED_SPECS = 244  # every spec of the 67 + 3 cases: pattern, LENGTH and DISTINCT specs alike


@pytest.fixture(scope="module")
def cases():
    return [R.Case(s) for s in R.SEEDS + R.LARGE_SEEDS]


@pytest.fixture(scope="module")
def coverages(cases):
    return [R.coverage(c) for c in cases]


def source(*path):
    with open(os.path.join(ROOT, "term_amd", "csrc", *path)) as f:
        return f.read()


def test_thresholds_are_the_sources():
    """the numbers regex_cases.py restates, read out of the sources: a moved threshold fails here, by name"""
    hip, types, dev = source("kernels", "regex.hip"), source("kernels", "regex_types.h"), source("regex_device.cpp")
    def num(text, rx):
        m = re.search(rx, text)
        assert m, "not found any more: %s" % rx
        return int(m.group(1))
    assert num(hip, r"constexpr uint32_t kStageBytes = (\d+);") == R.STAGE_BYTES
    assert num(hip, r"constexpr uint64_t kLdsEntries = (\d+);") == R.LDS_MAX_ENTRIES
    assert "entries <= kLdsEntries && entries * 2 <= 65535" in hip
    assert num(hip, r"dfa\.direct && entries <= (\d+);") == R.DIRECT_MAX_ENTRIES
    assert num(dev, r"\*direct = \(uint64_t\)n_states \* 256 <= (\d+);") == R.DIRECT_MAX_ENTRIES
    assert num(hip, r"ballot_w64\(inl0 \|\| inl1\) \? (\d+)u : 0u") == R.INLINE_AREA
    assert "e_last - base <= (int64_t)kStageBytes" in hip and "e_half - base <= (int64_t)kStageBytes" in hip
    assert "(int64_t)hi - sbase <= (int64_t)(kStageBytes - area)" in hip
    assert "(d.length + 127) / 128" in hip and R.STEP_ROWS == 128
    assert num(hip, r"if \(occ > (\d+)\) occ = \d+;") == R.MAX_RESIDENT
    assert "(d.length + 511) / 512" in hip and R.GRID_ROWS == 512
    assert num(types, r"constexpr uint32_t kRegexLdsEntries = (\d+);") == R.PRODUCT_MAX_ENTRIES
    assert num(types, r"constexpr int kMaxRegexGroup = (\d+);") == R.MAX_GROUP
    assert "rx::dfa_product(parts, kRegexLdsEntries, &prod)" in dev
    # regex_plan_finish's grouping, which Case.groups() replays through tgx_regex_match_group: greedy in task order, at
    # most kMaxRegexGroup members, same column, same TRIM flag, a candidate stays when the product still fits -- and the
    # host-side function decides by the same product and the same TRIM test.  A change to either fails here.
    assert "for (size_t j = i + 1; j < rp->tasks.size() && g.members.size() < (size_t)kMaxRegexGroup; j++) {" in dev
    assert ("if (b.is_length || rp->group_of[j] >= 0 || b.column != a.column ||\n"
            "          ((a.flags ^ b.flags) & TGX_FLAG_TRIM) != 0)\n        continue;") in dev
    assert "if (g.members.size() < 2) continue;" in dev
    assert "const bool ok = same_trim && rx::dfa_product(parts, kRegexLdsEntries, &prod);" in dev
    assert "same_trim &= ((f ^ (flags ? flags[0] : 0)) & TGX_FLAG_TRIM) == 0;" in dev
    assert "if (p->len_max >= 0) return false;" in source("regex", "regex_compile.cpp")  # (counted automata walk alone)
    assert num(source("kernels", "dict.hip"), r"constexpr int kDictMaxFused = (\d+);") == R.DICT_MAX_FUSED
    assert "kCoalesceMaxRows = 1 << 16" in source("api_internal.h") and R.COALESCE_MAX_ROWS == 1 << 16


def test_table_info_is_the_plans_compile():
    assert R.table_info("@") == (3, 2, -1, -1) and R.table_class(3, 2) == "direct"
    ns, nc, lo, hi = R.table_info(r"^\w{1,64}$")
    assert (lo, hi) == (1, 64) and R.table_class(ns, nc) == "lds"  # `^\w*$` and a character count
    assert R.table_info(r"^[^@]{2,5}$")[2:] == (-1, -1)  # (small enough to be expanded: no count)
    ns, nc, _, _ = R.table_info(r"\bab\b")
    assert R.table_class(ns, nc) == "global" and ns * nc > R.LDS_MAX_ENTRIES
    assert R.table_info("(") is None
    folded = R.table_info("^[a-z0-9._-]{3,12}$", T.FLAG_CASE_INSENSITIVE)
    assert folded[1] > R.table_info("^[a-z0-9._-]{3,12}$")[1]  # (the flag is part of the compile)


def test_feed_rules_at_their_thresholds():
    def offsets(widths):
        return np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    assert R.plain_feeds(offsets([31] * 128), 0, 128) == {"whole"}          # 3968 bytes
    assert R.plain_feeds(offsets([33] * 128), 0, 128) == {"half"}           # 4224: two halves of 2112
    assert R.plain_feeds(offsets([65] * 128), 0, 128) == {"lane"}           # 8320: neither half of 4160 fits
    assert R.plain_feeds(offsets([65] * 64 + [33] * 64), 0, 128) == {"lane", "half"}
    assert R.plain_feeds(offsets([65] * 70), 0, 70) == {"lane", "half"}     # (a short second half: 6 rows)
    assert R.plain_feeds(offsets([65] * 64), 0, 64) == {"lane"}             # (no second half at all)
    # the stage holds 4096 bytes from a 16-byte block border: up to 15 bytes in front of the span are copied too
    assert R.plain_feeds(offsets([4081] + [0] * 127), 0, 128) == {"whole"}
    assert R.plain_feeds(offsets([4082] + [0] * 127), 0, 128) == {"edge"}
    assert R.plain_feeds(offsets([4096] + [0] * 127), 0, 128) == {"edge"}
    assert R.plain_feeds(offsets([4097] + [0] * 127), 0, 128) == {"lane", "half"}  # (the empty half fits)
    # a slice: steps count from ITS first row
    assert R.plain_feeds(offsets([65] * 128 + [1] * 128), 0, 256) == {"lane", "whole"}
    assert R.plain_feeds(offsets([65] * 128 + [1] * 128), 64, 256) == {"lane", "half", "whole"}
    assert R.plain_feeds(offsets([65] * 128 + [1] * 128), 128, 256) == {"whole"}

    def views(rows):  # (length, buffer, offset)
        return np.array([[n, 0, b, o] for n, b, o in rows], dtype=np.int32)
    ok = np.ones(128, bool)
    assert R.view_feeds(views([(5, 0, 0)] * 128), ok) == {"v-inline"}
    assert R.view_feeds(views([(5, 0, 0)] * 128), ~ok) == {"v-empty"}  # (NULL rows: nothing to stage)
    assert R.view_feeds(views([(31, 0, 31 * i) for i in range(128)]), ok) == {"v-long"}
    assert R.view_feeds(views([(31, 0, 31 * i) for i in range(127)] + [(3, 0, 0)]), ok) == {"v-span"}  # 3937 > 4096 - 2048
    assert R.view_feeds(views([(31, 0, 31 * i) for i in range(60)] + [(3, 0, 0)] * 68), ok) == {"v-inline+long"}
    assert R.view_feeds(views([(31, i % 2, 31 * i) for i in range(128)]), ok) == {"v-2buf"}
    assert R.view_feeds(views([(2033, 0, 0), (3, 0, 0)]), ok[:2]) == {"v-inline+long"}
    assert R.view_feeds(views([(2034, 0, 0), (3, 0, 0)]), ok[:2]) == {"edge"}
    assert R.view_feeds(views([(2049, 0, 0), (3, 0, 0)]), ok[:2]) == {"v-span"}
    assert R.view_feeds(views([(5000, 0, 0)]), ok[:1]) == {"v-span"}


def test_seed_list_and_stability(cases):
    assert len(R.SEEDS) == len(set(R.SEEDS)) == N_SEEDS and len(R.LARGE_SEEDS) == 3
    for c in cases:
        assert R.Case(c.seed).describe() == c.describe(), c.seed


def test_nothing_is_left_out(cases):
    compared = 0
    for c in cases:
        assert c.refused() == [], c.seed  # RE2 and tgx_regex_validate take every drawn pattern, with and without flags
        want = c.expect()
        assert len(want) == len(c.specs) and None not in want, c.seed
        T.Plan(c.plan_specs())  # (the plan compiles without a device)
        compared += len(want)
    assert compared == N_COMPARED_SPECS


def test_trim_is_u0020_only(cases):
    """the expectation under TRIM is the value without its U+0020 runs -- tabs and line feeds stay"""
    seen_tab = False
    for c in cases:
        for s in c.specs:
            if s[0] == "regex" and s[2] & T.FLAG_TRIM:
                for raw, sub in zip(c._distinct(), c.matched(s)[1]):
                    assert sub == raw.strip(" ") and (sub == "" or (sub[0] != " " and sub[-1] != " "))
                    seen_tab |= sub != sub.strip(" \t\n")
    assert seen_tab  # (stripping more than blanks would change some subject of the list)


def test_references_agree(cases):
    """RE2, the oracle VM and the host automaton on every (pattern, flags, value) of every case"""
    for c in cases:
        assert c.reference_disagreements() == [], c.seed


def test_census(cases, coverages):
    assert R.missing(coverages) == []
    total = R.census(coverages)
    # the cells: every table class x layout x {single, product} x feed but the unreachable ones, each at least once
    cells = [k for k in R.requirements() if k.startswith("cell:")]
    assert len(cells) == (3 * 2 - 1) * (3 * len(R.PLAIN_FEEDS) + len(R.VIEW_FEEDS)) and all(total[k] >= 1 for k in cells)
    for b in R.CUTS + R.MEMS:
        assert total["batching:%s" % b] >= 3
    # the ragged cuts are Arrow slices at offsets that are no multiples of 8, 1, 7 and 9 among them
    for c in cases:
        if c.cut == "cuts":
            starts = [lo for lo, _ in c.bounds()[1:]]
            assert all(lo % 8 for lo in starts) and (c.n <= 9 or {1, 7, 9} <= set(starts)), c.seed
        assert c.bounds()[0][0] == 0 and c.bounds()[-1][1] == c.n and all(a[1] == b[0] for a, b in zip(c.bounds(), c.bounds()[1:]))
    # a tiny row count is credited where a launch really has that length: the tiny cases are one batch, no dictionary
    for c in cases:
        if c.kind == "tiny":
            assert c.launch_lengths() == [c.n] and c.n in R.TINY_ROWS and c.layout != "dict", c.seed
        if c.cut == "merge" and not c.coalesce and c.layout != "dict":
            assert c.launch_lengths() == [hi - lo for lo, hi in c.bounds() if hi > lo] and sum(c.launch_lengths()) == c.n
    # both verdicts per CELL, from the values its steps really carry
    assert all(total["hit:" + k[5:]] >= 1 and total["miss:" + k[5:]] >= 1 for k in cells)
    # the second sweep: more rows than the largest grid covers at once
    assert all(c.n > R.SECOND_SWEEP_ROWS == 512 * 256 * 7 for c in cases if c.kind == "large")


def test_the_unreachable_cell_and_its_reason(cases):
    """a product automaton never has a global table: dfa_product stops at kRegexLdsEntries, below launch_regex's limit"""
    assert list(R.UNREACHABLE) == ["global/*/product/*"]
    assert R.PRODUCT_MAX_ENTRIES <= R.LDS_MAX_ENTRIES and R.PRODUCT_MAX_ENTRIES * 2 <= 65535
    assert not any(k.startswith("cell:global/") and "/product/" in k for k in R.requirements())
    for c in cases:
        for r in c.routes():
            assert not (r and r["kind"] == "regex" and r["group"] == "product" and r["table"] == "global"), c.seed
    # ... and a pattern whose own table is global joins no group: the product would be larger still
    assert R.would_group([("a", 0), ("@", 0)]) and not R.would_group([(r"\bab\b", 0), ("@", 0)])


def test_both_verdicts_in_every_product(cases):
    n = 0
    for c in cases:
        assert R.product_verdict_gaps(c) == []
        n += sum(1 for r in c.routes() if r and r["kind"] == "regex" and r["group"] == "product")
    assert n >= 30


def test_grouping_replays_the_plan(cases):
    """greedy, in spec order, one TRIM flag, at most four members, counted automata alone"""
    for c in cases:
        for i, (how, members) in c.groups().items():
            assert len(members) <= R.MAX_GROUP and len({c.specs[m][2] & T.FLAG_TRIM for m in members}) == 1
            if R.table_info(c.specs[i][1], c.specs[i][2])[3] >= 0:
                assert how == "single", (c.seed, i)


def test_the_comparison_bites(cases):
    for c in cases[:12] + cases[-1:]:
        want = [tuple(w) for w in c.expect()]
        assert R.disagreements(c, want) == []
        R.check(c, want)
        for i in range(len(want)):
            for delta in ((0, 1), (0, -1), (1, 0)):  # a count off by one either way; `total` off by one
                got = list(want)
                got[i] = (want[i][0] + delta[0], want[i][1] + delta[1])
                bad = R.disagreements(c, got)
                assert len(bad) == 1 and "spec %d" % i in bad[0] and "route" in bad[0]
                with pytest.raises(AssertionError):
                    R.check(c, got)
        pairs = [(i, j) for i in range(len(want)) for j in range(i) if want[i] != want[j]]
        for i, j in pairs:  # two specs' counts swapped
            got = list(want)
            got[i], got[j] = want[j], want[i]
            assert len(R.disagreements(c, got)) == 2
        assert R.disagreements(c, want[:-1]) != []
    assert sum(1 for c in cases[:12] for _ in c.specs) > 30


def test_the_census_bites(cases, coverages):
    """every requirement taken out of the case list in turn: the census names it"""
    req = R.requirements()
    assert len(req) > 200
    for name in req:
        rest = [cov for cov in coverages if not cov[name]]
        assert len(rest) < len(coverages), name
        assert name in R.missing(rest), name
    # a batching needs three cases: with two it is missing
    for b in R.CUTS + R.MEMS:
        name = "batching:%s" % b
        two = [cov for cov in coverages if cov[name]][:2]
        assert name in R.missing([cov for cov in coverages if not cov[name]] + two)
    assert R.missing([]) == sorted(req)
    assert R.census(coverages) == sum(coverages, collections.Counter())
