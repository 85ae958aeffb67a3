"""The differential tester (tests/fuzz_plans.py) tested itself, without a device: Case(seed) only builds tables and
draws a plan.

- the cases of the first seed set are what they were before the JOINT_BINS / TEMPORAL / HISTOGRAM dimensions existed
  (tests/golden/fuzz_case_digests.json, written by tests/golden/make_fuzz_case_digests.py);
- the committed seeds meet every combination the new dimensions are there for (the census);
- the TIME_GAP dimension, drawn last and from a stream of its own, leaves those digests and that census as they are (it
  is not one of NEW_KINDS), and the three committed sets together meet a census of its own: every cell for the grouped
  and for the ungrouped route;
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
    old = [k for k, e in enumerate(case.expect) if e[0] not in NEW_KINDS + ("time_gap",)]
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
    """the cases of the first two committed sets (built once per session), or of the third"""
    from fuzz_plans import Case
    from test_gpu_fuzz import SECOND_MAX_ROWS, SECOND_SEEDS, THIRD_SEEDS

    if third not in _CASES:
        if third:
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


# ---- the comparisons fail when they should ----------------------------------------------------------------------------
class FakeResult:
    def __init__(self, total=0, non_null=0, matches=0):
        self.total, self.non_null, self.matches = total, non_null, matches


class FakeState:
    """the state reads check_one makes, answered from dicts keyed by spec index"""

    def __init__(self):
        self.hist_range, self.hist_counts, self.j_range, self.j_counts, self.temporal = {}, {}, {}, {}, {}
        self.time_gap = {}

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
HIST, JOINT, TEMPORAL, TIME_GAP = 0, 1, 2, 3  # spec indices
TIME_GAP_MAX = 2  # Y grouped by Z has the gaps 3, 2 | 7, 1 | 2 | 1, 3 (the NULL group): three above, four not


def small_case(phase, edges="shifted", moved=True):
    """a three-column table with one spec of each new kind, built without the generator"""
    import term_amd as T
    from fuzz_plans import Case

    c = Case.__new__(Case)
    c.seed, c.n, c.specs, c.present, c.phase, c.pass_two, c._cache = -1, len(X), [None] * 4, [None] * 3, 1, {}, {}
    c.cols = []
    for kind, vals, dtype in (("f", X, np.float64), ("i", Y, np.int64), ("i", Z, np.int64)):
        mask = np.array([v is not None for v in vals])
        c.cols.append((kind, np.array([0 if v is None else v for v in vals], dtype), None, mask, None))
    c.expect = [("histogram", 0, 4, edges, 7), ("joint", 0, 1, 2, moved),
                ("temporal", 1, 2, "order", dict(mode=T.TEMPORAL_ORDER, flags=0, delta=1)),
                ("time_gap", 1, 2, TIME_GAP_MAX)]
    if phase == 2:
        c.enter_pass_two()
    return c


def reference_answer(case):
    """what a faultless device would say, from the plain walks of the exact modules"""
    import exact_histogram as EH
    import exact_joint as EJ
    import exact_temporal as ET

    import exact_time_gap as EG

    res, st = [FakeResult() for _ in range(4)], FakeState()
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


PERTURBATIONS = [(1, _time_gap(f)) for f in (
    violations_up, violations_down_matches_consistent, largest_gap_up, a_partition_split_in_two, a_null_timestamp_retained,
    a_row_not_seen, null_group_split_row_by_row, the_ungrouped_answer)] + [(1, _time_gap_finalize_alone)]
PERTURBATIONS += [(2, _bucket_to_neighbour), (2, _else_row_into_the_last_bucket), (1, _histogram_non_finite),
                 (2, _histogram_counts_non_finite), (1, _joint_non_finite), (1, _histogram_min_next_double),
                 (1, _joint_min_next_double), (1, _histogram_negative_zero), (1, _joint_negative_zero),
                 (1, _sum_off_by_twice_its_bound("sum")), (1, _sum_off_by_twice_its_bound("sum_squared")),
                 (2, _joint_cell_transposed), (1, _considered_and_violations_up), (1, _null_row_considered)]


def test_check_one_fails_on_every_single_perturbation():
    import pytest

    for phase, perturb in PERTURBATIONS:
        case = small_case(phase)
        res, st = reference_answer(case)
        perturb(res, st)
        with pytest.raises(AssertionError):
            case.check_one(res, st)
        print("caught:", perturb.__qualname__)
