"""The differential tester (tests/fuzz_plans.py) tested itself, without a device: Case(seed) only builds tables and
draws a plan.

- the cases of the first seed set are what they were before the JOINT_BINS / TEMPORAL / HISTOGRAM dimensions existed
  (tests/golden/fuzz_case_digests.json, written by tests/golden/make_fuzz_case_digests.py);
- the committed seeds meet every combination the new dimensions are there for (the census);
- the TIME_GAP dimension, drawn last and from a stream of its own, leaves those digests and that census as they are (it
  is not one of NEW_KINDS), and the three committed sets together meet a census of its own: every cell for the grouped
  and for the ungrouped route;
- the VALUE_RULE / VALUE_COUNTS / PAIR_COUNTS / GROUP_COUNTS / GROUP_SUMS dimension, drawn after it from a stream of its
  own, leaves all of that as it is too; the four committed sets together meet a census of its own, keep the share of
  tasks that references alone cannot pin (a table that may overflow, a float sum that may) to a quarter, and the
  dimension is drawn only where its rules allow;
- the KEY_PROBE dimension, drawn last of all from a stream of its own (what is random when a case runs from a second
  one: run_device_inner draws from the case's stream what it drew before), leaves all of that as it is again; the five
  committed sets together meet a census of its own for each of its plain, counted and strings modes and for rows specs,
  the share of tasks whose exact number of missing keys exceeds their bound stays within a quarter per mode, and the
  dimension is drawn only where its rules allow, for between a third and two thirds of the eligible cases;
- check_one passes on the references' own answers and fails on each of a list of single perturbations."""
import hashlib
import json
import os

import numpy as np

NEW_KINDS = ("histogram", "joint", "temporal")
FIRST_SEEDS = range(48)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_case_digests.json")


def _h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _plain(x):
    """an expectation / parameter as JSON gives it back: tuples as lists, numpy scalars as Python's"""
    if isinstance(x, (tuple, list)):
        return [_plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    return x


def case_digest(case):
    """everything a seed decided before the new kinds were drawn: the table (hashes of every buffer), the older
    expectations and their specs, the batching, the environment, the state sequence and the presentations"""
    cols = []
    for kind, vals, vb, mask, extra in case.cols:
        d = [kind, str(vals.dtype), len(vals), _h(vals), None if vb is None else _h(vb), _h(mask)]
        if extra is not None:
            d += [_h(extra[0]), bool(extra[1]), extra[2], _h(np.frombuffer("\0".join(extra[3]).encode() or b"\0", np.uint8)),
                  _h(extra[4])]
        cols.append(d)
    old = [k for k, e in enumerate(case.expect) if e[0] not in NEW_KINDS + ("time_gap", "key_probe") + case.RULES_AND_COUNTS]
    specs = []
    for k in old:
        s = case.specs[k]
        specs.append([s.kind, s.column, s.column2, s.flags, s.pattern.decode() if s.pattern else None, s.kll_k,
                      [s.columns[j] for j in range(s.n_columns)], s.length_min, s.length_max])
    return {"n": case.n, "cols": cols, "expect": [_plain(case.expect[k]) for k in old], "specs": specs, "mode": case.mode,
            "cuts": [len(case.cuts), _h(np.array(case.cuts, np.int64))], "device": case.device, "after": case.after,
            "seq": case.seq, "world": getattr(case, "world", None), "env": dict(sorted(case.env.items())),
            "retain": case.retain, "exact_keys": case.exact_keys,
            "present": [p if p is None or isinstance(p, str) else p.__name__ for p in case.present]}


def test_the_first_seed_set_keeps_its_cases():
    from fuzz_plans import Case

    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(str(s) for s in FIRST_SEEDS)
    for seed in FIRST_SEEDS:
        case = Case(seed)
        got, want = json.loads(json.dumps(case_digest(case))), golden[str(seed)]
        temporal = {ci for e in case.expect if e[0] == "temporal" for ci in case.columns_of_expect(e)}
        for ci in temporal:  # the one permitted difference: a column a TEMPORAL check reads arrives as Int64
            assert got["present"][ci] is None, (seed, ci)
            want["present"][ci] = None
        assert got == want, seed


# ---- the census: a condition on the committed seeds, not a measurement ----------------------------------------------
AFTERS, SEQS, DEVICES = ("finalize", "blob", "merge", "ranks"), ("resume", "sync", "reuse"), ("device", "host", "mixed")
PHASED = ("histogram/range", "histogram/count", "joint/range", "joint/count", "temporal")


def census_cells(case):
    """the cells of the census this case fills, as strings"""
    import exact_histogram as EH
    import term_amd as T

    cells = set()
    for e in case.expect:
        kind = e[0]
        if kind not in NEW_KINDS:
            continue
        cols = case.columns_of_expect(e)
        for phased in ([kind] if kind == "temporal" else [kind + "/range", kind + "/count"]):
            cells.add("%s after=%s" % (phased, case.after))
        if case.seq != "plain":
            cells.add("%s seq=%s" % (kind, case.seq))
        cells.add("%s buffers=%s" % (kind, case.device))
        if case.retain and case.device != "device":  # (HOST batches handed over as HOST_RETAINED)
            cells.add("%s retained" % kind)
        if case.n == 0 or any(not case.cols[ci][3].any() for ci in cols):
            cells.add("%s without rows" % kind)
        if kind == "histogram":
            cells.add("histogram on %s" % case.cols[e[1]][0])
            if case.present[e[1]] is not None:
                cells.add("histogram on a narrow presentation")
            if e[2] in (1, 1000):
                cells.add("histogram buckets=%d" % e[2])
            cells.add("histogram edges=%s" % e[3])
        elif kind == "joint":
            if case.cols[e[1]][0] != case.cols[e[2]][0]:
                cells.add("joint on a mixed pair")
            cells.add("joint moved=%s" % e[4])
        else:
            cells.add("temporal mode=%s" % e[3])
            for name, bit in (("KEEP_NULLS", T.TEMPORAL_KEEP_NULLS), ("WEEKDAYS_ONLY", T.TEMPORAL_WEEKDAYS_ONLY)):
                if e[4]["flags"] & bit:
                    cells.add("temporal %s" % name)
    ranged = [e for e in case.expect if e[0] == "histogram"]
    if ranged:
        rules = [rule for e in ranged for rule, _ in EH.sum_rules(case.reference(("histogram_range", e[1])))]
        cells.add("histogram sums by the overflow rule" if any(r != "bound" for r in rules) else "histogram sums by the bound")
    if cells:
        cells.add("a new kind")
    return cells


REQUIRED = (["%s after=%s" % (p, a) for p in PHASED for a in AFTERS]
            + ["%s seq=%s" % (k, s) for k in NEW_KINDS for s in SEQS]
            + ["%s buffers=%s" % (k, d) for k in NEW_KINDS for d in DEVICES]
            + ["%s retained" % k for k in NEW_KINDS] + ["%s without rows" % k for k in NEW_KINDS]
            + ["histogram on %s" % k for k in ("i", "f", "i32", "f32")]
            + ["histogram on a narrow presentation", "histogram buckets=1", "histogram buckets=1000",
               "histogram edges=exact", "histogram edges=shifted", "histogram edges=uneven",
               "joint on a mixed pair", "joint moved=True", "joint moved=False",
               "temporal mode=order", "temporal mode=time_of_day", "temporal mode=range",
               "temporal KEEP_NULLS", "temporal WEEKDAYS_ONLY"])


_CASES = {}


def committed_cases(third=False):
    """the cases of the first two committed sets (built once per session), of the third (True), of the fourth ("fourth")
    or of the fifth ("fifth")"""
    from fuzz_plans import Case
    from test_gpu_fuzz import SECOND_MAX_ROWS, SECOND_SEEDS, THIRD_SEEDS

    if third not in _CASES:
        if third in ("fourth", "fifth"):
            from test_gpu_fuzz import FIFTH_SEEDS, FOURTH_SEEDS

            _CASES[third] = [Case(seed, max_rows=SECOND_MAX_ROWS) for seed in (FOURTH_SEEDS if third == "fourth" else FIFTH_SEEDS)]
        elif third:
            _CASES[third] = [Case(seed, max_rows=SECOND_MAX_ROWS) for seed in THIRD_SEEDS]
        else:
            _CASES[third] = [Case(seed) for seed in FIRST_SEEDS] + [Case(seed, max_rows=SECOND_MAX_ROWS) for seed in SECOND_SEEDS]
    return _CASES[third]


def test_census_of_the_committed_seeds():
    counts, cases = {}, 0
    for case in committed_cases():
        cases += 1
        for cell in census_cells(case):
            counts[cell] = counts.get(cell, 0) + 1
    for cell in sorted(counts):
        print("%4d  %s" % (counts[cell], cell))
    missing = [cell for cell in REQUIRED if not counts.get(cell)]
    assert not missing, missing
    # about one committed case in two carries a new kind
    assert 0.4 <= counts["a new kind"] / cases <= 0.6, (counts["a new kind"], cases)
    # the overflow rule stands in for the sum bound in a quarter of the HISTOGRAM range cases at the most
    by_rule, by_bound = counts.get("histogram sums by the overflow rule", 0), counts["histogram sums by the bound"]
    assert 4 * by_rule <= by_rule + by_bound, (by_rule, by_bound)


# ---- the TIME_GAP census: the three committed sets together ---------------------------------------------------------
TG_ROUTES = ("ungrouped", "grouped")
TG_SEQS, TG_MODES = ("plain",) + SEQS, ("one", "cuts", "stream")
TG_SORT_ROUTES = ("shipped", "two_passes", "three_passes", "chunked_last_pass", "many_stretches")
TG_SHARED = {"a DISTINCT or tuple check": ("distinct", "tuple"), "NUMERIC_STATS": ("stats",),
             "HISTOGRAM, JOINT_BINS or TEMPORAL": NEW_KINDS}


def time_gap_tasks(case):
    """{(timestamp column, group column or -1): number of thresholds}"""
    tasks = {}
    for e in case.expect:
        if e[0] == "time_gap":
            tasks[(e[1], e[2])] = tasks.get((e[1], e[2]), 0) + 1
    return tasks


def sort_passes(rows, env):
    """the partition passes kernels/sortrank.hip's sr_shape gives a sort of `rows` keys under a forcing environment"""
    target, cap, ways = int(env["TGX_SORT_TARGET"]), int(env["TGX_SORT_CAP"]), int(env["TGX_SORT_SPLIT"]) + 1
    buckets = max(2, -(-rows // target))
    return 0 if rows <= cap else 1 if buckets <= ways else 2 if buckets <= ways * ways else 3


def forced_route_is_taken(route, env, rows):
    """does a sort of `rows` keys under `env` go the way the environment's name says?"""
    passes = sort_passes(rows, env)
    if route == "chunked_last_pass":  # buckets of about TARGET keys, beyond what the slow kernel sorts in one piece
        return passes >= 1 and int(env["TGX_SORT_TARGET"]) > int(env["TGX_SORT_SLOWCAP"])
    return passes == {"two_passes": 2, "three_passes": 3, "many_stretches": 3}[route]


def time_gap_cells(case):
    """the cells of the TIME_GAP census this case fills"""
    cells = set()
    tasks = time_gap_tasks(case)
    if not tasks:
        return cells
    assert case.after == "finalize" and case.n <= case.NEW_KINDS_MAX_ROWS
    for (ct, cg), thresholds in tasks.items():
        assert case.cols[ct][0] == "i" and case.present[ct] is None, (case.seed, ct)
        route = TG_ROUTES[cg >= 0]
        stamped = case.cols[ct][3]
        mine = set()
        mine.add("seq=%s" % case.seq)
        mine.add("buffers=%s" % case.device)
        if case.retain and case.device != "device":
            mine.add("retained")
        mine.add("batching=%s" % case.mode)
        if "TGX_COALESCE_FLUSH_ROWS" in case.env:
            mine.add("coalesce flush rows set")
        if case.n == 0 or not stamped.any():
            mine.add("without rows")
        if thresholds > 8:  # kTimeGapThresholds
            mine.add("more thresholds than one pass compares")
        if case.shapes[ct] == "wide":
            mine.add("timestamps wide")
        if case.shapes[ct] in ("constant", "few"):
            mine.add("timestamps constant or few")
        # the longest list the task sorts: all its rows, or those of them that have a group
        rows = int((stamped & case.cols[cg][3]).sum() if cg >= 0 else stamped.sum())
        if not case.sort_env:
            mine.add("sort=shipped")
        elif forced_route_is_taken(case.sort_route, case.sort_env, rows):
            mine.add("sort=%s" % case.sort_route)
        for name, kinds in TG_SHARED.items():
            if any(e[0] in kinds and {ct, cg} & set(case.columns_of_expect(e)) for e in case.expect):
                mine.add("a column shared with %s" % name)
        if cg >= 0:
            assert case.cols[cg][0] in ("i", "i32") and not (case.present[cg] == "bool" or case.present[cg] is np.uint64)
            if case.n > 0 and not case.cols[cg][3].any():
                mine.add("every group NULL")
            if case.cols[cg][0] == "i32":
                mine.add("group column of kind i32")
            if case.present[cg] is not None:
                mine.add("group column under a narrow presentation")
            if cg == ct:
                mine.add("grouped by the timestamp column")
        cells |= {"%s %s" % (route, cell) for cell in mine}
    stamps = [ct for ct, _ in tasks]
    if len(stamps) == 2:
        cells.add("two tasks on one timestamp column" if stamps[0] == stamps[1] else "two tasks on different timestamp columns")
    cells.add("a TIME_GAP check")
    return cells


TG_REQUIRED = (["%s %s" % (r, c) for r in TG_ROUTES for c in (
    ["seq=%s" % s for s in TG_SEQS] + ["buffers=%s" % d for d in DEVICES] + ["retained"]
    + ["batching=%s" % m for m in TG_MODES] + ["coalesce flush rows set", "without rows",
                                               "more thresholds than one pass compares", "timestamps wide",
                                               "timestamps constant or few"]
    + ["sort=%s" % r for r in TG_SORT_ROUTES]
    + ["a column shared with %s" % name for name in TG_SHARED])]
    + ["grouped %s" % c for c in ("every group NULL", "group column of kind i32", "group column under a narrow presentation",
                                  "grouped by the timestamp column")]
    + ["two tasks on one timestamp column", "two tasks on different timestamp columns"])


def test_time_gap_census_of_the_three_committed_sets():
    from fuzz_plans import Case
    from test_gpu_fuzz import SECOND_SEEDS, THIRD_SEEDS

    assert len(THIRD_SEEDS) <= 48 and len(set(THIRD_SEEDS)) == len(THIRD_SEEDS) and not set(THIRD_SEEDS) & set(SECOND_SEEDS)
    assert TG_SORT_ROUTES[1:] == Case.FORCED_SORT_ROUTES  # every route the tester can force is a cell
    counts = {}
    for third in (False, True):
        for case in committed_cases(third):
            cells = time_gap_cells(case)
            if third:  # every seed of the third set carries the check
                assert cells, case.seed
            for cell in cells:
                counts[cell] = counts.get(cell, 0) + 1
    for cell in sorted(counts):
        print("%4d  %s" % (counts[cell], cell))
    missing = [cell for cell in TG_REQUIRED if not counts.get(cell)]
    assert not missing, missing


def test_the_time_gap_dimension_is_drawn_where_it_can_be():
    """eligibility is a condition: only simply finalized cases of at most NEW_KINDS_MAX_ROWS rows with an Int64 column
    presented as Int64, and a large share of those"""
    eligible = drawn = 0
    for third in (False, True):
        for case in committed_cases(third):
            has = bool(time_gap_tasks(case))
            can = (case.after == "finalize" and case.n <= case.NEW_KINDS_MAX_ROWS
                   and any(c[0] == "i" and p is None for c, p in zip(case.cols, case.present)))
            assert can or not has, case.seed
            if not third:
                eligible += can
                drawn += has
            if not has:
                assert not case.sort_env, case.seed
            for (ct, cg), thresholds in time_gap_tasks(case).items():
                assert 1 <= thresholds <= 11, (case.seed, ct, cg, thresholds)
    print("TIME_GAP drawn for %d of the %d eligible cases of the first two sets" % (drawn, eligible))
    assert 0.5 <= drawn / eligible <= 0.9, (drawn, eligible)


# ---- the census of VALUE_RULE and the four counting kinds: the four committed sets together ---------------------------
RC_KINDS = ("rule", "value_counts", "pair_counts", "group_counts", "group_sums")
RC_COUNTING = RC_KINDS[1:]
RC_MODES = ("one", "cuts", "stream")
RC_SHARED = {"a DISTINCT or tuple check": ("distinct", "tuple"), "NUMERIC_STATS": ("stats",), "another of the five kinds": RC_KINDS}
RC_KEYS = ("i", "i32", "a narrow presentation", "s/plain", "s/LargeUtf8", "s/view", "s/dict")
RULE_MODES = {1: "GE_ZERO", 2: "GT_ZERO", 3: "BETWEEN", 4: "INTEGER"}


def rc_key_columns(case, e):
    """the columns whose values are a counting task's keys: the column, the group column, or both sides of a pair"""
    return {"value_counts": (e[1],), "pair_counts": (e[1], e[2])}.get(e[0], (e[2],))


def rc_keys_and_bound(case, e):
    """(the exact number of keys d of the whole table, the bound) of a counting task"""
    if e[0] == "value_counts":
        return case.reference(("value_counts", e[1], e[3]))["distinct"], e[2]
    if e[0] == "pair_counts":
        return case.reference(("pair_counts", e[1], e[2], e[4], case.pair_binning(e)))["distinct"], e[3]
    return case.reference(("value_counts", e[2], e[4]))["distinct"], e[3]


def rc_tasks(case):
    """per counting kind [may the task be left to invariants: d > bound], and for the float GROUP_SUMS tasks [is any
    group, class or total decided by the overflow rule]"""
    tasks = {k: [] for k in RC_COUNTING + ("float group_sums",)}
    for e in case.expect:
        if e[0] in RC_COUNTING:
            d, bound = rc_keys_and_bound(case, e)
            tasks[e[0]].append(d > bound)
        if e[0] == "group_sums" and case.cols[e[1]][0] in ("f", "f32"):
            tasks["float group_sums"].append(bool(case.reference(("group_sums", e[1], e[2], e[4]))["rules"]))
    return tasks


def rc_cells(case):
    """the cells of the census this case fills"""
    cells = set()
    rule_counts = {}
    for e in case.expect:
        kind = e[0]
        if kind not in RC_KINDS:
            continue
        cols = case.columns_of_expect(e)
        mine = {"after=%s" % case.after, "buffers=%s" % case.device, "batching=%s" % case.mode}
        if case.seq != "plain":
            mine.add("seq=%s" % case.seq)
        if case.retain and case.device != "device":
            mine.add("retained")
        if case.n == 0 or any(not case.cols[ci][3].any() for ci in cols):
            mine.add("without rows")
        for name, kinds in RC_SHARED.items():
            if any(o is not e and o[0] in kinds and set(cols) & set(case.columns_of_expect(o)) for o in case.expect):
                mine.add("a column shared with %s" % name)
        if kind == "rule":
            rule = e[2]
            mine.add("mode=%s" % RULE_MODES[rule["mode"]])
            is_float = case.cols[e[1]][0] in ("f", "f32")
            if rule["flags"] & 1:
                mine.add("BOUNDS_AS_DOUBLE")
            if rule["mode"] == 3:
                import exact_value_rule as EV

                as_double = is_float or rule["flags"] & 1
                lo, hi = ((EV.key(EV.bits_of(rule["lo_f"])), EV.key(EV.bits_of(rule["hi_f"]))) if as_double
                          else (rule["lo_i"], rule["hi_i"]))
                if lo > hi:
                    mine.add("lo > hi")
            if is_float:
                d = case.doubles_of(e[1])[case.cols[e[1]][3]]
                if np.isnan(d).any() and np.isinf(d).any() and (d == 0.0).any():
                    mine.add("a float column with specials")
            rule_counts[e[1]] = rule_counts.get(e[1], 0) + 1
            if rule_counts[e[1]] > 8:  # (the rules of one column go to the kernel eight at a time)
                mine.add("more than eight rules on a column")
        else:
            d, bound = rc_keys_and_bound(case, e)
            mvb = e[3] if kind == "value_counts" else e[4]
            for ck in rc_key_columns(case, e):
                k, _, _, mask, extra = case.cols[ck]
                if k == "s":
                    mine.add("key s/%s" % (extra[2] if extra[2] != "plain" else "LargeUtf8" if extra[1] else "plain"))
                    if case.reference(("value_counts", ck, mvb))["long_rows"]:
                        mine.add("long rows")
                elif k in ("i", "i32"):
                    mine.add("key %s" % ("a narrow presentation" if case.present[ck] is not None else k))
                    if (case.wide_of(ck)[mask] == -1).any():
                        mine.add("the -1 key")
                if case.n > 0 and not mask.any():
                    mine.add("every key NULL")
            if bound == d:
                mine.add("bound=d")
            if bound == d + 1:
                mine.add("bound=d+1")
            if d > bound:
                mine.add("a bound that overflows")
            if case.after == "merge" and len(case.cuts) == 2:  # (one batch: every state but the first stays empty)
                mine.add("a merged state that saw no batch")
        if kind == "group_counts":
            if sum(1 for o in case.expect if o[0] == kind and o[2:] == e[2:]) > 1:
                mine.add("more than one member on a walk")
            if e[1] == e[2]:
                mine.add("the value column is the key column")
        elif kind == "group_sums":
            floats = case.cols[e[1]][0] in ("f", "f32")
            mine.add("float values" if floats else "integer values")
            if floats and case.reference(("group_sums", e[1], e[2], e[4]))["rules"]:
                mine.add("float sums by the overflow rule")
        elif kind == "pair_counts":
            side = case.pair_numeric_side(e)
            mine.add("two string sides" if side is None else "a numeric %s" % "xy"[side])
            if side is not None:
                b = case.pair_binning(e)
                mine.add("range phase after=%s" % case.after)
                if b is not None and case.valid_binning(b):
                    mine.add("count phase after=%s" % case.after)
                    if e[6]:
                        mine.add("a moved origin")
        cells |= {"%s %s" % (kind, cell) for cell in mine}
    return cells


RC_REQUIRED = (["%s %s" % (k, c) for k in RC_KINDS for c in (
    ["after=%s" % a for a in AFTERS] + ["seq=%s" % q for q in SEQS] + ["buffers=%s" % d for d in DEVICES] + ["retained"]
    + ["batching=%s" % m for m in RC_MODES] + ["without rows"] + ["a column shared with %s" % name for name in RC_SHARED])]
    + ["%s %s" % (k, c) for k in RC_COUNTING for c in (
        ["key %s" % key for key in RC_KEYS] + ["bound=d", "bound=d+1", "a bound that overflows", "long rows", "the -1 key",
                                               "every key NULL", "a merged state that saw no batch"])]
    + ["rule mode=%s" % m for m in RULE_MODES.values()]
    + ["rule %s" % c for c in ("BOUNDS_AS_DOUBLE", "lo > hi", "a float column with specials", "more than eight rules on a column")]
    + ["group_counts more than one member on a walk", "group_counts the value column is the key column",
       "group_sums integer values", "group_sums float values", "group_sums float sums by the overflow rule",
       "pair_counts two string sides", "pair_counts a numeric x", "pair_counts a numeric y", "pair_counts a moved origin"]
    + ["pair_counts %s phase after=%s" % (p, a) for p in ("range", "count") for a in AFTERS])


def test_rules_and_counts_census_of_the_four_committed_sets():
    from test_gpu_fuzz import FOURTH_SEEDS, SECOND_SEEDS, THIRD_SEEDS

    assert len(FOURTH_SEEDS) <= 48 and len(set(FOURTH_SEEDS)) == len(FOURTH_SEEDS)
    assert not set(FOURTH_SEEDS) & (set(FIRST_SEEDS) | set(SECOND_SEEDS) | set(THIRD_SEEDS))
    counts, tasks = {}, {}
    for which in (False, True, "fourth"):
        for case in committed_cases(which):
            cells = rc_cells(case)
            if which == "fourth":  # every seed of the fourth set carries the dimension
                assert cells, case.seed
            for cell in cells:
                counts[cell] = counts.get(cell, 0) + 1
            for name, flags in rc_tasks(case).items():
                tasks.setdefault(name, []).extend(flags)
    for cell in sorted(counts):
        print("%4d  %s" % (counts[cell], cell))
    missing = [cell for cell in RC_REQUIRED if not counts.get(cell)]
    assert not missing, missing
    # a condition, not a measurement: the references alone pin three tasks in four of every counting kind (d <= bound:
    # full equality is required), and the sum bound three float GROUP_SUMS tasks in four
    for name, flags in sorted(tasks.items()):
        print("%s: %d tasks, %d %s" % (name, len(flags), sum(flags), "with a group, class or total by the overflow rule"
                                       if name == "float group_sums" else "with more keys than their bound"))
        assert flags and 4 * sum(flags) <= len(flags), (name, sum(flags), len(flags))


def test_the_rules_and_counts_dimension_is_drawn_where_it_can_be():
    """eligibility is a condition: only cases of at most NEW_KINDS_MAX_ROWS rows, no UInt64 / Boolean presentation in a key
    or rule role, the types each role takes -- and between a third and two thirds of the eligible cases"""
    eligible = drawn = 0
    for which in (False, True, "fourth"):
        for case in committed_cases(which):
            mine = [e for e in case.expect if e[0] in RC_KINDS]
            kinds = [c[0] for c in case.cols]
            ok = [not case.unsupported_as_key(ci) for ci in range(len(kinds))]
            numeric = [ci for ci, k in enumerate(kinds) if k in ("i", "i32", "f", "f32") and ok[ci]]
            keys = [ci for ci, k in enumerate(kinds) if k == "s" or (k in ("i", "i32") and ok[ci])]
            can = case.n <= case.NEW_KINDS_MAX_ROWS and bool(numeric or keys)
            assert can or not mine, case.seed
            if any(e[0] in ("spearman", "time_gap") for e in case.expect):  # (their restriction stands)
                assert case.after in ("finalize", "ranks") and (case.after == "finalize" or not time_gap_tasks(case)), case.seed
            for e in mine:
                if e[0] == "rule":
                    assert e[1] in numeric, (case.seed, e)
                elif e[0] == "value_counts":
                    assert e[1] in keys, (case.seed, e)
                elif e[0] == "group_counts":
                    assert e[2] in keys and 0 <= e[1] < len(kinds), (case.seed, e)
                elif e[0] == "group_sums":
                    assert e[2] in keys and e[1] in numeric, (case.seed, e)
                else:
                    sides = [kinds[e[1]] == "s", kinds[e[2]] == "s"]
                    assert any(sides) and all(s or c in numeric for s, c in zip(sides, e[1:3])), (case.seed, e)
                if e[0] in RC_COUNTING:
                    bound = e[2] if e[0] == "value_counts" else e[3]
                    assert 1 <= bound <= case.BOUND_LIMIT, (case.seed, e)
            rules = {}
            for e in mine:
                if e[0] == "rule":
                    rules[e[1]] = rules.get(e[1], 0) + 1
            assert all(1 <= c <= 3 or c == 9 for c in rules.values()), (case.seed, rules)
            if which is False:
                eligible += can
                drawn += bool(mine)
    print("the dimension is drawn for %d of the %d eligible cases of the first two sets" % (drawn, eligible))
    assert 1 / 3 <= drawn / eligible <= 2 / 3, (drawn, eligible)


# ---- the KEY_PROBE census: the five committed sets together ----------------------------------------------------------------
KP_PROBING = ("plain", "counted", "strings")
# (no NUMERIC_STATS check reads a string column: a strings spec shares its column with LENGTH or REGEX_MATCH instead)
KP_SHARED = {"a DISTINCT or tuple check": ("distinct", "tuple"), "NUMERIC_STATS": ("stats",),
             "LENGTH or REGEX_MATCH": ("length", "regex"),
             "one of the five counting kinds": RC_KINDS, "another KEY_PROBE spec": ("key_probe",)}
KP_NOT_SHARED = {"plain": "LENGTH or REGEX_MATCH", "counted": "LENGTH or REGEX_MATCH", "strings": "NUMERIC_STATS"}
KP_ROUTES = {"plain": (0, 1, 2), "counted": (0, 3, 4), "strings": (0, 5)}
KP_SOURCES = {"plain": "ab", "counted": "abc", "strings": "ab"}
KP_LIMIT = {"plain": 128, "counted": 4}  # exact_key_probe.route_of, exact_join_coverage.route_of


def kp_specs(case):
    return [e for e in case.expect if e[0] == "key_probe"]


def kp_want(case, e):
    """(the reference's state, the route it gives the set) of a probing spec"""
    want = case.reference(case.kp_reference_key(e))
    return want, want["route"] if e[2] != "strings" else 5 if want["parent_keys"] else 0


def kp_tasks(case):
    """per probing mode [may the task be left to invariants: d > bound]"""
    tasks = {m: [] for m in KP_PROBING}
    for e in kp_specs(case):
        if e[2] != "rows":
            tasks[e[2]].append(kp_want(case, e)[0]["missing_keys"] > e[4])
    return tasks


def kp_cells(case):
    """the cells of the census this case fills"""
    cells = set()
    specs = kp_specs(case)
    for e in specs:
        _, ci, mode, parent, bound, mvb = e
        kind, _, _, mask, extra = case.cols[ci]
        if mode == "rows":
            cells |= {"rows seq=%s" % case.seq, "rows batching=%s" % case.mode}
            if mask.any() and not mask.all():
                cells.add("rows a column with NULLs")
            continue
        want, route = kp_want(case, e)
        d = want["missing_keys"]
        mine = {"after=%s" % case.after, "buffers=%s" % case.device, "batching=%s" % case.mode,
                "source (%s)" % parent.source, "route %d" % route}
        if case.seq != "plain":
            mine.add("seq=%s" % case.seq)
        if case.retain and case.device != "device":
            mine.add("retained")
        if case.n == 0:
            mine.add("without rows")
        for name, kinds in KP_SHARED.items():
            if any(o is not e and o[0] in kinds and ci in case.columns_of_expect(o) for o in case.expect):
                mine.add("a column shared with %s" % name)
        if bound == d:
            mine.add("bound=d")
        if bound == d + 1:
            mine.add("bound=d+1")
        if d > bound:
            mine.add("a bound that overflows")
        if want["non_null"] and not want["missing_rows"]:
            mine.add("no key missing")
        if want["non_null"] and not want["matched"]:
            mine.add("every key missing")
        if case.n > 0 and not want["non_null"]:
            mine.add("every child row NULL")
        if case.kp_refusal_step():
            mine.add("a mid-table blob with the refusal step")
        if case.after == "merge" and len(case.cuts) == 2:  # (one batch: every state but the first stays empty)
            mine.add("a merged state that saw no batch")
        alike = [o for o in specs if o[1:3] == e[1:3]]
        if len(alike) >= 9 and len({kp_want(case, o)[1] for o in alike}) == 1:
            mine.add("nine specs on one column and route")
        if mode == "strings":
            mine.add("layout %s" % (extra[2] if extra[2] != "plain" else "LargeUtf8" if extra[1] else "plain"))
            if want["long_rows"]:
                mine.add("long rows")
            live = parent.values[parent.valid]
            if parent.source == "a" and len(np.unique(live)) < len(live):
                mine.add("duplicate records")
            if parent.near:
                mine.add("records that share one fingerprint word with a missing key")
        else:
            keys, counts = parent.records()
            if parent.on_threshold(KP_LIMIT[mode]):
                mine.add("a set on a route threshold")
            if (keys == -1).any():
                mine.add("the -1 key in the set")
            if (case.kp_child(ci)[0][mask] == -1).any():
                mine.add("the -1 key among the child's values")
            if parent.duplicates():
                mine.add("duplicate records")
            if mode == "counted" and len(counts) and int(counts.max()) >= 1 << 40:
                mine.add("a count of 2^40")
            mine.add("child %s" % ("a narrow presentation" if case.present[ci] is not None else kind))
            if parent.width != case.kp_width(ci):
                mine.add("a parent from a column of another width")
            if any(o[3] is parent and {o[2], mode} == {"plain", "counted"} for o in specs if o is not e):
                cells.add("a plain and a counted spec that agree")
        cells |= {"%s %s" % (mode, cell) for cell in mine}
    return cells


KP_REQUIRED = (["%s %s" % (m, c) for m in KP_PROBING for c in (
    ["after=%s" % a for a in AFTERS] + ["seq=%s" % q for q in SEQS] + ["buffers=%s" % d for d in DEVICES] + ["retained"]
    + ["batching=%s" % b for b in RC_MODES] + ["without rows"] + ["a column shared with %s" % name for name in KP_SHARED if name != KP_NOT_SHARED[m]]
    + ["source (%s)" % x for x in KP_SOURCES[m]] + ["route %d" % x for x in KP_ROUTES[m]]
    + ["bound=d", "bound=d+1", "a bound that overflows", "no key missing", "every key missing", "every child row NULL",
       "duplicate records", "a mid-table blob with the refusal step", "a merged state that saw no batch",
       "nine specs on one column and route"])]
    + ["%s %s" % (m, c) for m in ("plain", "counted") for c in (
        ["a set on a route threshold", "the -1 key in the set", "the -1 key among the child's values",
         "a parent from a column of another width"] + ["child %s" % k for k in ("i", "i32", "a narrow presentation")])]
    + ["counted a count of 2^40", "strings long rows", "strings records that share one fingerprint word with a missing key", "a plain and a counted spec that agree"]
    + ["strings layout %s" % x for x in ("plain", "LargeUtf8", "view", "dict")]
    + ["rows seq=%s" % q for q in ("plain",) + SEQS] + ["rows batching=%s" % b for b in RC_MODES] + ["rows a column with NULLs"])
ALL_SETS = (False, True, "fourth", "fifth")


def test_key_probe_census_of_the_five_committed_sets():
    from test_gpu_fuzz import FIFTH_SEEDS, FOURTH_SEEDS, SECOND_SEEDS, THIRD_SEEDS

    assert len(FIFTH_SEEDS) <= 48 and len(set(FIFTH_SEEDS)) == len(FIFTH_SEEDS)
    assert not set(FIFTH_SEEDS) & (set(FIRST_SEEDS) | set(SECOND_SEEDS) | set(THIRD_SEEDS) | set(FOURTH_SEEDS))
    counts, tasks = {}, {}
    for which in ALL_SETS:
        for case in committed_cases(which):
            cells = kp_cells(case)
            if which == "fifth":  # every seed of the fifth set carries the kind
                assert cells, case.seed
            for cell in cells:
                counts[cell] = counts.get(cell, 0) + 1
            for name, flags in kp_tasks(case).items():
                tasks.setdefault(name, []).extend(flags)
    for cell in sorted(counts):
        print("%4d  %s" % (counts[cell], cell))
    missing = [cell for cell in KP_REQUIRED if not counts.get(cell)]
    assert not missing, missing
    # a condition, not a measurement: the references alone pin three tasks in four of every probing mode (d <= bound: full
    # equality is required) -- from the exact number of missing keys d, on the CPU
    for name, flags in sorted(tasks.items()):
        print("%s: %d tasks, %d with more missing keys than their bound" % (name, len(flags), sum(flags)))
        assert flags and 4 * sum(flags) <= len(flags), (name, sum(flags), len(flags))


def test_the_key_probe_dimension_is_drawn_where_it_can_be():
    """eligibility is a condition: only cases of at most NEW_KINDS_MAX_ROWS rows; integer children Int64, Int32 or a narrow
    presentation, never UInt64 or Boolean; string children in a strings spec only; a rows spec only in a case that is
    simply finalized; the bounds the library takes -- and between a third and two thirds of the eligible cases"""
    import term_amd as T
    from fuzz_plans import ParentSet

    eligible = drawn = 0
    for which in ALL_SETS:
        for case in committed_cases(which):
            mine = kp_specs(case)
            kinds = [c[0] for c in case.cols]
            ints = [ci for ci, k in enumerate(kinds) if k in ("i", "i32") and not case.unsupported_as_key(ci)]
            can = case.n <= case.NEW_KINDS_MAX_ROWS and (bool(ints) or "s" in kinds)
            assert can or not mine, case.seed
            assert len(mine) in (0, 1, 2, 3, 9), (case.seed, len(mine))
            for _, ci, mode, parent, bound, mvb in mine:
                assert mode in case.KP_MODES and (ci in ints if mode != "strings" else kinds[ci] == "s"), (case.seed, ci, mode)
                if mode == "rows":
                    assert case.after == "finalize" and parent is None, case.seed
                    continue
                assert isinstance(parent, ParentSet) and parent.source in KP_SOURCES[mode], (case.seed, mode, parent)
                assert 1 <= bound <= T.KEY_PROBE_MAX_MISSING_KEYS == case.BOUND_LIMIT, (case.seed, bound)
                if mode == "strings":
                    assert 1 <= mvb <= T.KEY_PROBE_MAX_VALUE_BYTES, (case.seed, mvb)
                else:  # no draw lets rows x the largest multiplicity come near 2^64
                    assert case.n * max(1, parent.max_count()) < 1 << 62, case.seed
            if which is False:
                eligible += can
                drawn += bool(mine)
    print("KEY_PROBE is drawn for %d of the %d eligible cases of the first two sets" % (drawn, eligible))
    assert 1 / 3 <= drawn / eligible <= 2 / 3, (drawn, eligible)


# ---- the comparisons fail when they should ----------------------------------------------------------------------------
class FakeResult:
    def __init__(self, total=0, non_null=0, matches=0, distinct=0, sum_i=0, sum_f=0.0, has_value=0):
        self.total, self.non_null, self.matches, self.distinct = total, non_null, matches, distinct
        self.sum_i, self.sum_f, self.has_value = sum_i, sum_f, has_value


class FakeState:
    """the state reads check_one makes, answered from dicts keyed by spec index"""

    def __init__(self):
        self.hist_range, self.hist_counts, self.j_range, self.j_counts, self.temporal = {}, {}, {}, {}, {}
        self.time_gap = {}
        # VALUE_RULE: the four counters; the counting kinds: (summary, entries), as term_amd.State's readers give them
        self.rule, self.vc, self.pc, self.pr, self.gc, self.gs = {}, {}, {}, {}, {}, {}
        # KEY_PROBE: (summary, entries) of a plain, counted or strings spec (a rows spec: its three counters, no entry),
        # the pairs of a counted one, the {key, 1} records of a rows one as a host array
        self.kp, self.kp_pairs, self.kp_rows = {}, {}, {}

    def key_probe(self, si):
        return dict(self.kp[si][0]), dict(self.kp[si][1])

    key_probe_strings = key_probe

    def key_probe_pairs(self, si):
        return dict(self.kp_pairs[si])

    def key_probe_rows(self, si):
        return self.kp_rows[si].copy(), len(self.kp_rows[si])

    def value_rule_counts(self, si):
        return tuple(self.rule[si])

    def value_counts(self, si):
        return dict(self.vc[si][0]), dict(self.vc[si][1])

    def pair_counts(self, si):
        return dict(self.pc[si][0]), dict(self.pc[si][1])

    def pair_range(self, si):
        return dict(self.pr[si])

    def group_counts(self, si):
        return dict(self.gc[si][0]), dict(self.gc[si][1])

    def group_sums(self, si):
        return dict(self.gs[si][0]), dict(self.gs[si][1])

    def histogram_range(self, si):
        return dict(self.hist_range[si])

    def histogram_counts(self, si):
        counts, else_rows, non_finite = self.hist_counts[si]
        return list(counts), else_rows, non_finite

    def joint_range(self, si):
        return dict(self.j_range[si])

    def joint_counts(self, si):
        return list(self.j_counts[si][0]), self.j_counts[si][1]

    def temporal_counts(self, si):
        return tuple(self.temporal[si])

    def time_gap_counts(self, si):
        return tuple(self.time_gap[si])


X = [0.0, 0.5, 1.0, 2.5, 4.0, float("nan"), 3.0, None, 1.5, 4.0, 0.25, 3.75]
Y = [3, 1, 4, 1, 5, 9, 2, 6, None, 5, 8, 0]
# (as a group column: 5, 0 and 4 hold several rows each, and three rows with a timestamp have no group)
Z = [5, 0, 4, None, 5, 0, None, 4, 3, None, 0, 5]
# (a string column: NULL rows, the empty string, a word longer than SMALL_MAX_BYTES; "a" holds X's NaN, "bb" only finite values)
S = ["a", "bb", "a", None, "long word", "a", "bb", "", "a", None, "long word", "bb"]
S_WORDS = ["a", "bb", "", "long word"]
SMALL_MAX_BYTES, SMALL_BOUND, PAIR_BINS = 4, 10000, 2
HIST, JOINT, TEMPORAL, TIME_GAP = 0, 1, 2, 3  # spec indices
RULE, VALUE_COUNTS, PAIR_COUNTS, GROUP_COUNTS, GROUP_SUMS_F, GROUP_SUMS_I = 4, 5, 6, 7, 8, 9
KP_PLAIN, KP_COUNTED, KP_STRINGS, KP_ROWS = 10, 11, 12, 13
N_SPECS = 14
# KEY_PROBE on the small table.  Plain, Y against hand-made records with a duplicate and a far key (4 records over a range
# of 1000 > 128 * 4: the hash route): 1, 1, 5, 5 match; 0, 2, 3, 4, 6, 8, 9 are missing once each.  Counted, Z against
# multiplicities: 5 (three rows) twice and 0 (three rows) once are 9 pairs of 6 matched rows; 4 is missing twice, 3 once.
# Strings, S under a bound of KP_MAX_BYTES = 2 bytes: "a" matches; "bb" (exactly 2 bytes) and "" are kept, "long word"
# is two long rows.  Rows: Z's nine non-NULL keys.
KP_PLAIN_RECORDS = [1, 5, 5, 1000]
KP_COUNTED_RECORDS = [(5, 2), (0, 1), (7, 3)]
KP_STRING_PARENT = ["a", "zz", "a"]
KP_MAX_BYTES = 2
KP_KEY = bytes(range(1, 17))
TIME_GAP_MAX = 2  # Y grouped by Z has the gaps 3, 2 | 7, 1 | 2 | 1, 3 (the NULL group): three above, four not


def small_case(phase, edges="shifted", moved=True):
    """a four-column table with one spec of each new kind (GROUP_SUMS twice: float and integer values), built without
    the generator"""
    import exact_value_rule as EV
    import term_amd as T
    from fuzz_plans import Case, ParentSet

    c = Case.__new__(Case)
    c.host_only, c.kp_set_held, c.kp_key = False, True, KP_KEY
    c.seed, c.n, c.specs, c.present, c.phase, c.pass_two, c._cache = -1, len(X), [None] * N_SPECS, [None] * 4, 1, {}, {}
    c.tables = 1
    c.cols = []
    for kind, vals, dtype in (("f", X, np.float64), ("i", Y, np.int64), ("i", Z, np.int64)):
        mask = np.array([v is not None for v in vals])
        c.cols.append((kind, np.array([0 if v is None else v for v in vals], dtype), None, mask, None))
    s_mask = np.array([v is not None for v in S])
    picks = np.array([S_WORDS.index(v) if v is not None else 0 for v in S])
    c.cols.append(("s", None, None, s_mask, (None, False, "plain", S_WORDS, picks)))
    c.expect = [("histogram", 0, 4, edges, 7), ("joint", 0, 1, 2, moved),
                ("temporal", 1, 2, "order", dict(mode=T.TEMPORAL_ORDER, flags=0, delta=1)),
                ("time_gap", 1, 2, TIME_GAP_MAX),
                ("rule", 0, EV.rule(EV.INTEGER)), ("value_counts", 3, SMALL_BOUND, SMALL_MAX_BYTES),
                ("pair_counts", 3, 0, SMALL_BOUND, SMALL_MAX_BYTES, PAIR_BINS, moved),
                ("group_counts", 0, 3, SMALL_BOUND, SMALL_MAX_BYTES), ("group_sums", 0, 3, SMALL_BOUND, SMALL_MAX_BYTES),
                ("group_sums", 1, 3, SMALL_BOUND, SMALL_MAX_BYTES)]
    ones = np.ones(len(KP_PLAIN_RECORDS), bool)
    c.expect += [
        ("key_probe", 1, "plain", ParentSet("a", KP_PLAIN_RECORDS, ones, ones.astype(np.uint64), "by hand"), SMALL_BOUND, 0),
        ("key_probe", 2, "counted", ParentSet("a", [k for k, _ in KP_COUNTED_RECORDS], ones[:3],
                                              np.array([n for _, n in KP_COUNTED_RECORDS], np.uint64), "by hand"), SMALL_BOUND, 0),
        ("key_probe", 3, "strings", ParentSet("b", [0, 1, 0], ones[:3], None, "by hand", words=KP_STRING_PARENT[:2],
                                              layout=("plain", False)), SMALL_BOUND, KP_MAX_BYTES),
        ("key_probe", 2, "rows", None, 0, 0)]
    if phase == 2:
        c.enter_pass_two()
    return c


def reference_answer(case):
    """what a faultless device would say, from the plain walks of the exact modules"""
    import exact_histogram as EH
    import exact_joint as EJ
    import exact_temporal as ET

    import exact_time_gap as EG

    res, st = [FakeResult() for _ in range(N_SPECS)], FakeState()
    rules_and_counts_answer(case, res, st)
    key_probe_answer(res, st)
    r = EH.value_range(X)
    res[HIST] = FakeResult(r["total"], r["n"] + r["non_finite"])
    st.hist_range[HIST] = dict(total=r["total"], nulls=r["nulls"], non_finite=r["non_finite"], n=r["n"], min=r["min"],
                               max=r["max"], sum=float(r["sum"]), sum_squared=float(r["sum_squared"]))
    p = EJ.pair_range(X, Y)
    res[JOINT] = FakeResult(len(X), p["n"])
    st.j_range[JOINT] = dict(p, total=len(X))
    if case.phase == 2:
        st.hist_counts[HIST] = EH.counts_of(X, case.pass_two[HIST])
        st.hist_range[HIST].update(min=float("nan"), max=float("nan"), sum=float("nan"), sum_squared=float("nan"))
        cells, outside = EJ.joint_counts(X, Y, case.pass_two[JOINT])
        st.j_counts[JOINT] = (EJ.dense(cells, 2), outside)
    seen, considered, violations = ET.counts(ET.ORDER, dict(delta=1), Y, Z, [v is not None for v in Y], [v is not None for v in Z])
    res[TEMPORAL] = FakeResult(seen, considered, considered - violations)
    st.temporal[TEMPORAL] = (seen, considered, violations)
    want = EG.counts(TIME_GAP_MAX, *time_gap_columns())
    assert want == (12, 11, 7, 3, 7)  # (worked by hand above: the perturbations below have room on both sides)
    set_time_gap(res, st, want)
    return res, st


def s_cells():
    return [None if v is None else v.encode() for v in S]


def set_counted(res, st, si, store, summary, entries):
    """a device that holds `summary` and `entries` for a VALUE_COUNTS / PAIR_COUNTS / GROUP_COUNTS task, consistently
    through its getters and tgx_finalize"""
    getattr(st, store)[si] = (summary, entries)
    if store == "vc":
        res[si] = FakeResult(summary["seen"], summary["non_null"], summary["counted"], summary["distinct"])
    elif store == "pc":
        res[si] = FakeResult(summary["seen"], summary["both_non_null"], summary["counted"], summary["distinct"])
    else:
        res[si] = FakeResult(summary["seen"], sum(v is not None for v in X), summary["counted"], summary["groups"])


def set_group_sums(res, st, si, summary, entries, values):
    """the same for a GROUP_SUMS task over `values`; tgx_finalize carries the sum over all four classes"""
    import exact_group_sums as EGS

    st.gs[si] = (summary, entries)
    non_null = [v for v in values if v is not None]
    total = sum(summary[c][2] for c in ("counted", "null_group", "overflow", "long_rows"))
    res[si] = FakeResult(summary["seen"], len(non_null), summary["counted"][0], summary["groups"], has_value=int(bool(non_null)))
    if values is X:  # (float values)
        res[si].sum_f = total
    else:
        res[si].sum_i, res[si].sum_f = EGS.wrap(total), float(EGS.wrap(total))


def rules_and_counts_answer(case, res, st):
    """VALUE_RULE and the four counting kinds, from the plain walks (the tester compares with their numpy twins)"""
    import exact_group_counts as EGC
    import exact_group_sums as EGS
    import exact_pair_counts as EP
    import exact_value_counts as EVC
    import exact_value_rule as EV

    bits = [0 if v is None else EV.bits_of(v) for v in X]
    want = EV.counts(case.expect[RULE][2], bits, [v is not None for v in X], is_float=True)
    assert want == (12, 11, 5, 1)  # (0, 1, 4, 3 and 4 are whole; the NaN is a cast error)
    set_rule(res, st, want)
    w = EVC.walk(s_cells(), SMALL_MAX_BYTES)
    assert (w["distinct"], w["long_rows"], w["non_null"]) == (3, 2, 10)
    set_counted(res, st, VALUE_COUNTS, "vc", {k: v for k, v in w.items() if k != "counts"}, w["counts"])
    # PAIR_COUNTS (S, X): the range of X over the rows that have a word, then the counts under pass two's binning
    r = EP.side_range(X, S)
    st.pr[PAIR_COUNTS] = dict(r, min=float("nan") if r["min"] is None else r["min"], max=float("nan") if r["max"] is None else r["max"])
    blank = dict(seen=len(X), both_non_null=r["both_non_null"], distinct=0, counted=0, overflow_rows=0, long_rows=0,
                 non_finite=0, out_of_range=0)
    set_counted(res, st, PAIR_COUNTS, "pc", blank, {})
    if case.phase == 2:
        w = EP.walk(S, X, None, case.pass_two[PAIR_COUNTS], SMALL_MAX_BYTES)
        assert min(w["counted"], w["long_rows"], w["non_finite"]) > 0 and w["distinct"] >= 2
        set_counted(res, st, PAIR_COUNTS, "pc", {k: v for k, v in w.items() if k != "counts"}, w["counts"])
    w = EGC.walk(X, s_cells(), SMALL_MAX_BYTES)
    assert w["groups"] == 3 and min(w["null_group_rows"], w["long_rows"]) > 0
    set_counted(res, st, GROUP_COUNTS, "gc", {k: v for k, v in w.items() if k != "entries"}, w["entries"])
    for si, values, is_float in ((GROUP_SUMS_F, X, True), (GROUP_SUMS_I, Y, False)):
        w = EGS.walk(values, s_cells(), SMALL_MAX_BYTES, is_float)
        entries = {k: c[:3] for k, c in w["entries"].items()}
        counted = w["counted"][:2] + (sum(c[2] for c in entries.values()),)  # (the entries' sums in key order)
        summary = dict(seen=w["seen"], groups=w["groups"], is_float=w["is_float"], counted=counted,
                       null_group=w["null_group"][:3], overflow=w["overflow"][:3], long_rows=w["long_rows"][:3])
        set_group_sums(res, st, si, summary, entries, values)


def set_key_probe(res, st, si, summary, entries):
    """a device that holds `summary` and `entries` for a KEY_PROBE spec, consistently through its getter and tgx_finalize"""
    st.kp[si] = (summary, entries)
    res[si] = FakeResult(summary["seen"], summary["non_null"], summary["matched"], summary["missing_keys"])


def key_probe_answer(res, st):
    """KEY_PROBE in its four modes, from the plain walks (the tester compares with their numpy twins)"""
    import exact_join_coverage as EJC
    import exact_key_probe as EKP
    import exact_key_probe_strings as EKS

    def side(values):
        return [0 if v is None else v for v in values], [v is not None for v in values]

    w = EKP.walk(*side(Y), KP_PLAIN_RECORDS, None, SMALL_BOUND, n_records=len(KP_PLAIN_RECORDS))
    assert (w["matched"], w["missing_keys"], w["parent_keys"], w["route"]) == (4, 7, 3, EKP.ROUTE_HASH)
    assert EKP.route_of(KP_PLAIN_RECORDS[:3]) == EKP.ROUTE_BITMAP  # (the far key alone makes it a hash table)
    entries = w.pop("entries")
    del w["within_bound"]
    set_key_probe(res, st, KP_PLAIN, w, entries)
    w, pairs = EJC.walk(*side(Z), KP_COUNTED_RECORDS, SMALL_BOUND)
    assert (w["matched"], pairs["pairs"], pairs["max_count"], w["entries"]) == (6, 9, 3, {3: 1, 4: 2})
    entries = w.pop("entries")
    set_key_probe(res, st, KP_COUNTED, w, entries)
    st.kp_pairs[KP_COUNTED] = pairs
    w = EKS.walk(S, KP_STRING_PARENT, KP_MAX_BYTES, SMALL_BOUND)
    assert (w["matched"], w["long_rows"], w["entries"]) == (4, 2, {b"": 1, b"bb": 3})
    entries = w.pop("entries")
    del w["within_bound"]
    w.update(max_value_bytes=KP_MAX_BYTES, parent_digest=EKS.parent_digest(KP_KEY, KP_STRING_PARENT), route=5)
    set_key_probe(res, st, KP_STRINGS, w, entries)
    z, valid = side(Z)
    blank = dict.fromkeys(st.kp[KP_PLAIN][0], 0)
    set_key_probe(res, st, KP_ROWS, dict(blank, seen=len(Z), non_null=sum(valid), null_rows=len(Z) - sum(valid)), {})
    st.kp_rows[KP_ROWS] = np.array([[v, 1] for v, m in zip(z, valid) if m], np.int64).view(np.uint64)[::-1]


def set_rule(res, st, counts):
    """a device that says `counts`, consistently through tgx_value_rule_get and tgx_finalize"""
    seen, considered, valid, errors = counts
    st.rule[RULE] = tuple(counts)
    res[RULE] = FakeResult(seen, considered, valid, errors)


def time_gap_columns():
    """(t, valid_t, g, valid_g) of the TIME_GAP spec, as the plain reference takes them"""
    return ([0 if v is None else v for v in Y], [v is not None for v in Y],
            [0 if v is None else v for v in Z], [v is not None for v in Z])


def set_time_gap(res, st, counts):
    """a device that says `counts`, consistently through tgx_time_gap_get and tgx_finalize"""
    seen, _, gaps, violations, _ = counts
    st.time_gap[TIME_GAP] = tuple(counts)
    res[TIME_GAP] = FakeResult(seen, gaps, gaps - violations)


def test_check_one_passes_on_the_references_own_answers():
    for phase in (1, 2):
        for edges in ("exact", "shifted", "uneven"):
            for moved in (False, True):
                case = small_case(phase, edges, moved)
                case.check_one(*reference_answer(case))


def _bucket_to_neighbour(res, st):
    counts, else_rows, non_finite = st.hist_counts[HIST]
    assert counts[1] > 0
    counts = list(counts)
    counts[1] -= 1
    counts[2] += 1
    st.hist_counts[HIST] = (counts, else_rows, non_finite)


def _else_row_into_the_last_bucket(res, st):
    counts, else_rows, non_finite = st.hist_counts[HIST]
    assert else_rows > 0  # (the shifted edges leave rows below the first edge)
    st.hist_counts[HIST] = (counts, else_rows - 1, non_finite)


def _histogram_non_finite(res, st):
    st.hist_range[HIST]["non_finite"] += 1


def _histogram_counts_non_finite(res, st):
    counts, else_rows, non_finite = st.hist_counts[HIST]
    st.hist_counts[HIST] = (counts, else_rows, non_finite + 1)


def _joint_non_finite(res, st):
    st.j_range[JOINT]["non_finite"] += 1


def _histogram_min_next_double(res, st):
    import math

    st.hist_range[HIST]["min"] = math.nextafter(st.hist_range[HIST]["min"], math.inf)


def _joint_min_next_double(res, st):
    import math

    st.j_range[JOINT]["y_min"] = math.nextafter(st.j_range[JOINT]["y_min"], math.inf)


def _histogram_negative_zero(res, st):
    assert st.hist_range[HIST]["min"] == 0.0
    st.hist_range[HIST]["min"] = -0.0


def _joint_negative_zero(res, st):
    assert st.j_range[JOINT]["x_min"] == 0.0
    st.j_range[JOINT]["x_min"] = -0.0


def _sum_off_by_twice_its_bound(name):
    def perturb(res, st):
        import exact_histogram as EH

        r = EH.value_range(X)
        bound = EH.sum_bounds(r)[("sum", "sum_squared").index(name)]
        moved = float(r[name] + 2 * bound)
        assert moved != st.hist_range[HIST][name]
        st.hist_range[HIST][name] = moved
    return perturb


def _joint_cell_transposed(res, st):
    cells, outside = st.j_counts[JOINT]
    cells = list(cells)
    i, j = next((i, j) for i in range(3) for j in range(3) if i != j and cells[i * 3 + j] > 0)
    cells[i * 3 + j] -= 1
    cells[j * 3 + i] += 1
    st.j_counts[JOINT] = (cells, outside)


def _considered_and_violations_up(res, st):
    seen, considered, violations = st.temporal[TEMPORAL]
    st.temporal[TEMPORAL] = (seen, considered + 1, violations + 1)
    res[TEMPORAL].non_null += 1  # (matches = considered - violations stays)


def _null_row_considered(res, st):
    seen, considered, violations = st.temporal[TEMPORAL]
    st.temporal[TEMPORAL] = (seen, considered + 1, violations)
    res[TEMPORAL].non_null += 1
    res[TEMPORAL].matches += 1


def _time_gap(change):
    """a perturbation of the five counters; the finalize fields follow, so the counters' comparison has to see it"""
    def perturb(res, st):
        before = st.time_gap[TIME_GAP]
        after = tuple(change(*before))
        assert after != before, change.__name__
        set_time_gap(res, st, after)
    perturb.__qualname__ = "time_gap: " + change.__name__
    return perturb


def violations_up(seen, rows, gaps, violations, largest):
    return seen, rows, gaps, violations + 1, largest


def violations_down_matches_consistent(seen, rows, gaps, violations, largest):
    return seen, rows, gaps, violations - 1, largest


def largest_gap_up(seen, rows, gaps, violations, largest):
    return seen, rows, gaps, violations, largest + 1


def a_partition_split_in_two(seen, rows, gaps, violations, largest):
    return seen, rows, gaps - 1, violations, largest


def a_null_timestamp_retained(seen, rows, gaps, violations, largest):
    return seen, rows + 1, gaps, violations, largest


def a_row_not_seen(seen, rows, gaps, violations, largest):
    return seen - 1, rows, gaps, violations, largest


def null_group_split_row_by_row(*_):
    from test_exact_time_gap import perturbed

    return perturbed("null_group_per_row", TIME_GAP_MAX, *time_gap_columns())


def the_ungrouped_answer(*_):
    import exact_time_gap as EG

    t, vt, _, _ = time_gap_columns()
    return EG.counts(TIME_GAP_MAX, t, vt)


def _time_gap_finalize_alone(res, st):
    res[TIME_GAP].matches += 1  # (tgx_finalize disagreeing with tgx_time_gap_get)


# ---- VALUE_RULE and the counting kinds: one perturbation at a time ----------------------------------------------------------
def _rule(change):
    def perturb(res, st):
        before = st.rule[RULE]
        after = tuple(change(*before))
        assert after != before
        set_rule(res, st, after)
    perturb.__qualname__ = "rule: " + change.__name__
    return perturb


def valid_up(seen, considered, valid, errors):
    return seen, considered, valid + 1, errors


def a_cast_error_counted_as_valid(seen, considered, valid, errors):
    return seen, considered, valid + 1, errors - 1


def a_null_row_considered(seen, considered, valid, errors):
    return seen, considered + 1, valid, errors


def _rule_finalize_alone(res, st):
    res[RULE].matches += 1  # (tgx_finalize disagreeing with tgx_value_rule_get)


class Counted:
    """one counting task of the small case, read and written through the names its kind gives the same things: the
    summary's fields for the rows in entries, the rows left out as NULL, the overflow and the long rows; an entry's
    count is the entry itself or its first field"""

    def __init__(self, name, si, store, phase, counted, nulls, nulls_down):
        self.name, self.si, self.store, self.phase = name, si, store, phase
        self.counted, self.nulls, self.nulls_down = counted, nulls, nulls_down

    def read(self, st):
        summary, entries = getattr(st, self.store)[self.si]
        return dict(summary), dict(entries)

    def write(self, res, st, summary, entries, order=None):
        n_name = "distinct" if "distinct" in summary else "groups"
        summary[n_name] = len(entries)
        if order is not None:
            entries = {k: entries[k] for k in order}
        if self.store == "gs":
            values = X if self.si == GROUP_SUMS_F else Y
            set_group_sums(res, st, self.si, summary, entries, values)
        else:
            set_counted(res, st, self.si, self.store, summary, entries)

    @staticmethod
    def bump(entries, key, by):
        v = entries.get(key, 0 if not entries or not isinstance(next(iter(entries.values())), tuple)
                        else (0,) * len(next(iter(entries.values()))))
        entries[key] = v + by if not isinstance(v, tuple) else (v[0] + by,) + tuple(v[1:])

    def field(self, summary, name, by):
        """a row count of the summary up or down (GROUP_SUMS: the rows of the class)"""
        if self.store == "gs":
            cls = {"counted": "counted", "overflow_rows": "overflow", "long_rows": "long_rows",
                   "null_group_rows": "null_group"}[name]
            summary[cls] = (summary[cls][0] + by,) + tuple(summary[cls][1:])
        else:
            summary[name] += by

    def perturbations(self):
        def two_keys(entries):
            keys = list(entries)
            assert len(keys) >= 2
            return keys[0], keys[1]

        def a_row_from_one_entry_to_another(res, st):
            summary, entries = self.read(st)
            a = max(entries, key=lambda k: entries[k][0] if isinstance(entries[k], tuple) else entries[k])
            b = next(k for k in entries if k != a)
            self.bump(entries, a, -1)
            self.bump(entries, b, +1)
            assert all((v[0] if isinstance(v, tuple) else v) > 0 for v in entries.values())
            self.write(res, st, summary, entries)

        def an_entry_up_and_the_summary_follows(res, st):
            summary, entries = self.read(st)
            self.bump(entries, two_keys(entries)[0], +1)
            self.field(summary, self.counted, +1)
            self.write(res, st, summary, entries)

        def a_null_key_row_counted_in_an_entry(res, st):
            summary, entries = self.read(st)
            self.bump(entries, two_keys(entries)[0], +1)
            self.field(summary, self.counted, +1)
            self.field(summary, self.nulls, -1 if self.nulls_down else +1)
            self.write(res, st, summary, entries)

        def overflow_rows_under_the_bound(res, st):
            summary, entries = self.read(st)
            a = max(entries, key=lambda k: entries[k][0] if isinstance(entries[k], tuple) else entries[k])
            self.bump(entries, a, -1)
            self.field(summary, self.counted, -1)
            self.field(summary, "overflow_rows", +1)
            self.write(res, st, summary, entries)

        def a_long_row_counted(res, st):
            summary, entries = self.read(st)
            long_key = b"long word" if self.store != "pc" else (b"long word", next(iter(entries))[1])
            self.bump(entries, long_key, +1)
            self.field(summary, self.counted, +1)
            self.field(summary, "long_rows", -1)
            self.write(res, st, summary, entries, order=sorted(entries))

        def two_entries_swapped(res, st):
            summary, entries = self.read(st)
            a, b = two_keys(entries)
            self.write(res, st, summary, entries, order=[b, a] + list(entries)[2:])

        def finalize_alone(res, st):
            res[self.si].matches += 1  # (tgx_finalize disagreeing with the kind's getter)

        out = []
        for f in (a_row_from_one_entry_to_another, an_entry_up_and_the_summary_follows, a_null_key_row_counted_in_an_entry,
                  overflow_rows_under_the_bound, a_long_row_counted, two_entries_swapped, finalize_alone):
            f.__qualname__ = "%s: %s" % (self.name, f.__name__)
            out.append((self.phase, f))
        return out


COUNTED = [Counted("value_counts", VALUE_COUNTS, "vc", 1, "counted", "non_null", False),
           Counted("pair_counts", PAIR_COUNTS, "pc", 2, "counted", "both_non_null", False),
           Counted("group_counts", GROUP_COUNTS, "gc", 1, "counted", "null_group_rows", True),
           Counted("group_sums (floats)", GROUP_SUMS_F, "gs", 1, "counted", "null_group_rows", True),
           Counted("group_sums (integers)", GROUP_SUMS_I, "gs", 1, "counted", "null_group_rows", True)]


def _pair_cell_transposed(res, st):
    """a row of (word, bin i) counted under bin j of the same word"""
    summary, entries = st.pc[PAIR_COUNTS]
    entries = dict(entries)
    (word, i), _ = next(iter(entries.items()))
    j = 1 - i if i in (0, 1) else 0
    entries[(word, i)] -= 1
    entries[(word, j)] = entries.get((word, j), 0) + 1
    entries = {k: v for k, v in sorted(entries.items()) if v}
    set_counted(res, st, PAIR_COUNTS, "pc", dict(summary, distinct=len(entries)), entries)


def _pair_range_next_double(name):
    def perturb(res, st):
        import math

        st.pr[PAIR_COUNTS][name] = math.nextafter(st.pr[PAIR_COUNTS][name], math.inf)
    perturb.__qualname__ = "pair_counts: range %s moved to the next double" % name
    return perturb


def _pair_range_non_finite(res, st):
    st.pr[PAIR_COUNTS]["non_finite"] += 1
    st.pr[PAIR_COUNTS]["n"] -= 1


def _pair_entries_in_the_range_phase(res, st):
    summary, _ = st.pc[PAIR_COUNTS]
    st.pc[PAIR_COUNTS] = (summary, {(b"a", 0): 1})


def _group_sum(si, change, what):
    def perturb(res, st):
        summary, entries = st.gs[si]
        summary, entries = dict(summary), dict(entries)
        change(summary, entries)
        set_group_sums(res, st, si, summary, entries, X if si == GROUP_SUMS_F else Y)
    perturb.__qualname__ = "group_sums: " + what
    return perturb


def _integer_sum_off_by_one(summary, entries):
    rows, non_null, total = entries[b"bb"]
    entries[b"bb"] = (rows, non_null, total + 1)
    summary["counted"] = summary["counted"][:2] + (summary["counted"][2] + 1,)  # (the identities keep holding)
    summary["null_group"] = summary["null_group"][:2] + (summary["null_group"][2] - 1,)


def _float_sum_off_by_twice_its_bound(summary, entries):
    import exact_group_sums as EGS

    want = EGS.walk(X, s_cells(), SMALL_MAX_BYTES, True)["entries"][b"bb"]
    assert want[1] > 1 and want[2] == want[2]  # (0.5 + 3.0 + 3.75: a finite group, whose bound is not zero)
    bound = EGS.float_bound(want[1], want[2], want[3])
    assert bound > 0 and want[2] + 2 * bound != want[2]
    entries[b"bb"] = want[:2] + (want[2] + 2 * bound,)


def _is_float_flipped(summary, entries):
    summary["is_float"] = not summary["is_float"]


def _a_nan_group_that_is_finite(summary, entries):
    rows, non_null, total = entries[b"a"]
    assert total != total  # (the overflow rule: "a" holds X's NaN)
    entries[b"a"] = (rows, non_null, 2.5)


def _null_group_value_lost(summary, entries):
    rows, non_null, total = summary["null_group"]
    assert non_null > 0
    summary["null_group"] = (rows, non_null - 1, total)


# ---- KEY_PROBE: one perturbation at a time ---------------------------------------------------------------------------------
def _key_probe(si, what, change):
    """`change` edits (summary, entries) of spec si in place, may return the entries in a new order; tgx_finalize follows"""
    def perturb(res, st):
        summary, entries = dict(st.kp[si][0]), dict(st.kp[si][1])
        before = (dict(summary), list(entries.items()))
        entries = change(summary, entries) or entries
        assert (summary, list(entries.items())) != before, what
        set_key_probe(res, st, si, summary, entries)
    perturb.__qualname__ = "key_probe: " + what
    return perturb


def _shift(summary, **by):
    for k, v in by.items():
        summary[k] += v


def _kp_matched_row_missing(summary, entries):
    entries[3] += 1
    _shift(summary, matched=-1, missing_rows=+1, counted=+1)


def _kp_null_row_non_null(summary, entries):
    entries[3] += 1
    _shift(summary, null_rows=-1, non_null=+1, missing_rows=+1, counted=+1)


def _kp_count_to_the_neighbour(summary, entries):
    assert entries == {3: 1, 4: 2}
    entries.update({3: 2, 4: 1})


def _kp_out_of_order(summary, entries):
    keys = list(entries)
    return {k: entries[k] for k in [keys[1], keys[0]] + keys[2:]}


def _kp_entry_for_a_key_of_the_set(summary, entries):
    entries[5] = 1
    _shift(summary, matched=-1, missing_rows=+1, counted=+1, missing_keys=+1)
    return dict(sorted(entries.items()))


def _kp_field(name, by=None, to=None):
    def change(summary, entries):
        summary[name] = to if to is not None else summary[name] + by
    return change


def _kp_long_row_kept(summary, entries):
    entries[b"long word"] = 2
    _shift(summary, long_rows=-2, counted=+2, missing_keys=+1)
    return dict(sorted(entries.items()))


def _kp_exactly_max_value_bytes_is_long(summary, entries):
    assert len(b"bb") == KP_MAX_BYTES
    rows = entries.pop(b"bb")
    _shift(summary, long_rows=+rows, counted=-rows, missing_keys=-1)


def _kp_pairs(what, **fields):
    def perturb(res, st):
        assert all(st.kp_pairs[KP_COUNTED][k] != v for k, v in fields.items())
        st.kp_pairs[KP_COUNTED] = dict(st.kp_pairs[KP_COUNTED], **fields)
    perturb.__qualname__ = "key_probe: " + what
    return perturb


def _kp_rows_lost_a_record(res, st):
    st.kp_rows[KP_ROWS] = st.kp_rows[KP_ROWS][1:]


def _kp_rows_kept_a_null_row(res, st):
    st.kp_rows[KP_ROWS] = np.concatenate([st.kp_rows[KP_ROWS], np.array([[0, 1]], np.uint64)])


def _kp_finalize_alone(res, st):
    res[KP_PLAIN].matches += 1  # (tgx_finalize disagreeing with tgx_key_probe_get)


KP_PERTURBATIONS = [
    _key_probe(KP_PLAIN, "a matched row counted as missing, the identities kept", _kp_matched_row_missing),
    _key_probe(KP_PLAIN, "a NULL row counted as non-NULL", _kp_null_row_non_null),
    _key_probe(KP_COUNTED, "one entry's count moved to the neighbouring key", _kp_count_to_the_neighbour),
    _key_probe(KP_PLAIN, "two entries out of order", _kp_out_of_order),
    _key_probe(KP_STRINGS, "two entries out of order (bytes)", _kp_out_of_order),
    _key_probe(KP_PLAIN, "an entry for a key that is in the set", _kp_entry_for_a_key_of_the_set),
    _key_probe(KP_PLAIN, "parent_digest off by one", _kp_field("parent_digest", by=1)),
    _key_probe(KP_STRINGS, "parent_digest off by one (strings)", _kp_field("parent_digest", by=1)),
    _key_probe(KP_PLAIN, "parent_keys counting a duplicate record twice", _kp_field("parent_keys", to=len(KP_PLAIN_RECORDS))),
    _key_probe(KP_PLAIN, "route 1 where the rule gives 2", _kp_field("route", to=1)),
    _kp_pairs("pairs equal to matched where a multiplicity is 2", pairs=6, join_rows=6 + 3 + 3),
    _kp_pairs("max_count too small", max_count=2),
    _key_probe(KP_STRINGS, "a long row kept as an entry", _kp_long_row_kept),
    _key_probe(KP_STRINGS, "a missing key of exactly max_value_bytes bytes counted as a long row", _kp_exactly_max_value_bytes_is_long),
    _kp_rows_lost_a_record, _kp_rows_kept_a_null_row, _kp_finalize_alone]
for _f in KP_PERTURBATIONS[-3:]:
    _f.__qualname__ = "key_probe: " + _f.__name__[4:].replace("_", " ")


PERTURBATIONS = [(1, _time_gap(f)) for f in (
    violations_up, violations_down_matches_consistent, largest_gap_up, a_partition_split_in_two, a_null_timestamp_retained,
    a_row_not_seen, null_group_split_row_by_row, the_ungrouped_answer)] + [(1, _time_gap_finalize_alone)]
PERTURBATIONS += [(2, _bucket_to_neighbour), (2, _else_row_into_the_last_bucket), (1, _histogram_non_finite),
                 (2, _histogram_counts_non_finite), (1, _joint_non_finite), (1, _histogram_min_next_double),
                 (1, _joint_min_next_double), (1, _histogram_negative_zero), (1, _joint_negative_zero),
                 (1, _sum_off_by_twice_its_bound("sum")), (1, _sum_off_by_twice_its_bound("sum_squared")),
                 (2, _joint_cell_transposed), (1, _considered_and_violations_up), (1, _null_row_considered)]
PERTURBATIONS += [(1, _rule(f)) for f in (valid_up, a_cast_error_counted_as_valid, a_null_row_considered)] + [(1, _rule_finalize_alone)]
for _kind in COUNTED:
    PERTURBATIONS += _kind.perturbations()
PERTURBATIONS += [(2, _pair_cell_transposed), (1, _pair_range_next_double("min")), (1, _pair_range_next_double("max")),
                  (1, _pair_range_non_finite), (1, _pair_entries_in_the_range_phase),
                  (1, _group_sum(GROUP_SUMS_I, _integer_sum_off_by_one, "an integer sum off by one")),
                  (1, _group_sum(GROUP_SUMS_F, _float_sum_off_by_twice_its_bound, "a float sum off by twice its bound")),
                  (1, _group_sum(GROUP_SUMS_F, _is_float_flipped, "is_float flipped (floats)")),
                  (1, _group_sum(GROUP_SUMS_I, _is_float_flipped, "is_float flipped (integers)")),
                  (1, _group_sum(GROUP_SUMS_F, _a_nan_group_that_is_finite, "a finite sum for a group with a NaN")),
                  (1, _group_sum(GROUP_SUMS_F, _null_group_value_lost, "a value of the NULL group not counted"))]


PERTURBATIONS += [(1, f) for f in KP_PERTURBATIONS]


def test_check_one_fails_on_every_single_perturbation():
    import pytest

    for phase, perturb in PERTURBATIONS:
        case = small_case(phase)
        res, st = reference_answer(case)
        perturb(res, st)
        with pytest.raises(AssertionError):
            case.check_one(res, st)
        print("caught:", perturb.__qualname__)
