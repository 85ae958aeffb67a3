#!/usr/bin/env python3
"""TGX_CHECK_ROW_PREDICATE beside its yardsticks, each pair over the same columns in one process:

    one CMP_LITERAL on an Int64 / a Float64 column      VALUE_RULE's BETWEEN on that column (the same bytes, the same class of walk)
    a <= b on two Int64 columns                         TEMPORAL's ORDER mode
    c IN ('F', 'O', 'P') on a Utf8 / Utf8View / Dictionary column      VALUE_COUNTS on that column
    a 4-column, 8-leaf numeric predicate                the roofline of its bytes at 8 TB/s

One DEVICE batch of --rows rows, no NULLs.  The predicates are compiled from their text by the library's compiler
(term_amd.suite.row_predicate).  Kernel times are HIP-event times on the state's stream (tgx_profile_get), the median of
--steps steps after one warm-up step of every shape.  There is no gate: every figure is reported beside its yardstick
from the same run, as a ratio, and goes into DESIGN.md.
    python tools/bench_row_predicate.py [--rows 1000000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes / s (MI355X, HBM3E)


def timed(T, plan, cols, kernel, steps):
    st = T.State(plan)
    st.profile_enable(True)
    times = []
    for it in range(steps + 1):
        st.reset()
        st.profile_reset()
        st.update(cols)
        st.finalize()
        if it:  # (step 0 warms the shape up)
            times.append(st.profile_get(kernel)["total_ms"])
    return st, statistics.median(times), min(times)


def predicate_plan(T, S, spec, expression, names):
    """a one-spec plan of `expression` over the table whose columns are `names`"""
    c = S.row_predicate(expression)
    plan = T.Plan([spec(T.ROW_PREDICATE, 0, columns=[names.index(n) for n in c["columns"]])])
    leaves = [dict((k, v) for k, v in leaf.items() if k != "lit_f_bits") for leaf in c["leaves"]]
    plan.set_row_predicate(0, leaves, [tuple(p) for p in c["program"]], bytes.fromhex(c["literals_hex"]))
    return plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import term_amd as T
    import term_amd.suite as S
    from term_amd._lib import spec

    n = args.rows // 64 * 64
    T.init(flags=T.OPT_NO_COALESCE)
    out = {"rows": n}
    lines = []

    def pair(name, ours, yard, yard_name):
        out[name] = {"row_predicate_ms": ours[1], "row_predicate_min_ms": ours[2], yard_name + "_ms": yard[1],
                     yard_name + "_min_ms": yard[2], "ratio": ours[1] / yard[1]}
        lines.append("%-28s row_predicate %8.3f ms | %-24s %8.3f ms | ratio %.2f" % (name, ours[1], yard_name, yard[1],
                                                                                    ours[1] / yard[1]))

    gen = torch.Generator(device="cuda").manual_seed(0x7E570020)
    a = torch.randint(-3000, 3000, (n,), dtype=torch.int64, device="cuda", generator=gen)
    b = torch.randint(-3000, 3000, (n,), dtype=torch.int64, device="cuda", generator=gen)
    x = a.to(torch.float64) * 0.5
    y = b.to(torch.float64) * 0.25
    ca, cb = T.Column.int64(a, None, length=n), T.Column.int64(b, None, length=n)
    cx, cy = T.Column.float64(x, None, length=n), T.Column.float64(y, None, length=n)

    # one CMP_LITERAL beside VALUE_RULE's BETWEEN
    for name, col, expression in (("cmp_literal_int64", ca, "a >= 0"), ("cmp_literal_float64", cx, "a >= 0.0")):
        ours = timed(T, predicate_plan(T, S, spec, expression, ["a"]), [col], "row_predicate", args.steps)
        plan = T.Plan([spec(T.VALUE_RULE, 0)])
        plan.set_value_rule(0, mode=T.RULE_BETWEEN, lo_i=-1000, hi_i=1000, lo_f=-1000.0, hi_f=1000.0)
        yard = timed(T, plan, [col], "value_rule", args.steps)
        seen, sat, unk, failed = ours[0].row_predicate_counts(0)
        assert seen == n and unk == 0 and 0 < sat < n
        pair(name, ours, yard, "value_rule_between")
        out[name]["hbm_fraction"] = n * 8 / (ours[1] * 1e-3) / HBM_PEAK

    # a <= b beside TEMPORAL's ORDER mode
    ours = timed(T, predicate_plan(T, S, spec, "a <= b", ["a", "b"]), [ca, cb], "row_predicate", args.steps)
    plan = T.Plan([spec(T.TEMPORAL, 0, column2=1)])
    plan.set_temporal(0, mode=T.TEMPORAL_ORDER, flags=0, delta=0)
    yard = timed(T, plan, [ca, cb], "temporal", args.steps)
    assert ours[0].row_predicate_counts(0)[0] == n
    pair("columns_le_int64", ours, yard, "temporal_order")
    out["columns_le_int64"]["hbm_fraction"] = n * 16 / (ours[1] * 1e-3) / HBM_PEAK

    # the 4-column, 8-leaf predicate beside the roofline of its bytes
    expression = "a BETWEEN -1000 AND 1000 AND b <> 7 AND (c >= 0.0 OR d < 100.5) AND a <= c AND NOT d = -0.0 AND b IS NOT NULL"
    compiled = S.row_predicate(expression)
    assert len(compiled["columns"]) == 4 and len(compiled["leaves"]) == 8
    ours = timed(T, predicate_plan(T, S, spec, expression, ["a", "b", "c", "d"]), [ca, cb, cx, cy], "row_predicate",
                 args.steps)
    roof_ms = n * 32 / HBM_PEAK * 1e3
    out["four_columns_eight_leaves"] = {"row_predicate_ms": ours[1], "row_predicate_min_ms": ours[2], "roofline_ms": roof_ms,
                                        "ratio": ours[1] / roof_ms, "counts": list(ours[0].row_predicate_counts(0))}
    lines.append("%-28s row_predicate %8.3f ms | %-24s %8.3f ms | ratio %.2f" % ("four_columns_eight_leaves", ours[1],
                                                                                "roofline at 8 TB/s", roof_ms, ours[1] / roof_ms))
    del a, b, x, y, ca, cb, cx, cy
    torch.cuda.empty_cache()

    # c IN ('F', 'O', 'P') on the string layouts beside VALUE_COUNTS: one-byte values out of four
    letters = torch.tensor(list(b"FOPX"), dtype=torch.uint8, device="cuda")
    pick = torch.randint(0, 4, (n,), dtype=torch.int32, device="cuda", generator=gen)
    data = letters[pick.long()]
    want = int((pick < 3).sum().item())
    offsets = torch.arange(n + 1, dtype=torch.int32, device="cuda")
    views = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    views[:, 0] = 1
    views[:, 1] = data.to(torch.int32)
    entries = T.Column(T.UTF8, 4, offsets=torch.arange(5, dtype=torch.int32, device="cuda"),
                       data=torch.cat([letters, torch.zeros(64, dtype=torch.uint8, device="cuda")]), mem=T.MEM_DEVICE)
    layouts = {
        "in_list_utf8": T.Column(T.UTF8, n, offsets=offsets, data=torch.cat([data, torch.zeros(64, dtype=torch.uint8, device="cuda")]),
                                 mem=T.MEM_DEVICE),
        "in_list_utf8_view": T.Column(T.UTF8_VIEW, n, values=views, mem=T.MEM_DEVICE, variadic=[]),
        "in_list_dictionary": T.Column(T.DICT32_UTF8, n, values=pick, dictionary=entries, mem=T.MEM_DEVICE),
    }
    for name, col in layouts.items():
        ours = timed(T, predicate_plan(T, S, spec, "c IN ('F', 'O', 'P')", ["c"]), [col], "row_predicate", args.steps)
        assert ours[0].row_predicate_counts(0) == (n, want, 0, n - want)
        plan = T.Plan([spec(T.VALUE_COUNTS, 0)])
        plan.set_value_counts(0, 16, 16)
        yard = timed(T, plan, [col], "value_counts", args.steps)
        pair(name, ours, yard, "value_counts")

    print("%d rows" % n)
    for line in lines:
        print(line, flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
