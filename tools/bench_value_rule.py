#!/usr/bin/env python3
"""The TGX_CHECK_VALUE_RULE modes, each alone and eight rules in one walk, beside two yardsticks over the same column in
one process: TGX_CHECK_TEMPORAL's RANGE mode (the same 8 B + 1 bit per row through the same row walker; Int64 columns
only) and the NUMERIC_STATS scan.  One column of --rows rows on DEVICE, one batch, no NULLs; Int64 and Float64 in turn.
Kernel times are HIP-event times on the state's stream (tgx_profile_get), the median of --steps steps after one warm-up
step of every shape.  There is no gate: the figures go into DESIGN.md.
    python tools/bench_value_rule.py [--rows 1000000000] [--steps 5] [--json out.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import term_amd as T
    from term_amd._lib import spec

    n = args.rows // 64 * 64
    T.init(flags=T.OPT_NO_COALESCE)
    out = {"rows": n}
    B = T.RULE_BOUNDS_AS_DOUBLE
    modes = {
        "ge_zero": dict(mode=T.RULE_GE_ZERO),
        "gt_zero": dict(mode=T.RULE_GT_ZERO),
        "between": dict(mode=T.RULE_BETWEEN, lo_i=-1000, hi_i=1000, lo_f=-1000.0, hi_f=1000.0),
        "between_as_double": dict(mode=T.RULE_BETWEEN, flags=B, lo_f=-999.5, hi_f=999.5),
        "integer": dict(mode=T.RULE_INTEGER),
    }
    eight = [modes["ge_zero"], modes["gt_zero"], modes["between"], modes["between_as_double"], modes["integer"],
             dict(mode=T.RULE_BETWEEN, lo_i=0, hi_i=10, lo_f=0.0, hi_f=10.0), dict(mode=T.RULE_BETWEEN, flags=B, lo_f=0.5, hi_f=1e6),
             dict(mode=T.RULE_BETWEEN, lo_i=-10**6, hi_i=-1, lo_f=-1e6, hi_f=-1.0)]
    for dtype in ("int64", "float64"):
        gen = torch.Generator(device="cuda").manual_seed(0x7E570014)
        # values around zero, a tenth of them beyond Int32; the Float64 column holds halves of them
        vals = torch.randint(-3000, 3000, (n,), dtype=torch.int64, device="cuda", generator=gen)
        vals = torch.where(vals % 10 == 0, vals * (1 << 30), vals)
        if dtype == "float64":
            vals = vals.to(torch.float64) * 0.5
        ctor = T.Column.int64 if dtype == "int64" else T.Column.float64
        cols = [ctor(vals, None, length=n)]
        res = out[dtype] = {}
        _, res["numeric_stats_ms"], res["numeric_stats_min_ms"] = timed(T, T.Plan([spec(T.NUMERIC_STATS, 0)]), cols, "scan", args.steps)
        if dtype == "int64":
            plan = T.Plan([spec(T.TEMPORAL, 0)])
            plan.set_temporal(0, mode=T.TEMPORAL_RANGE, lo=-1000, hi=1000)
            _, res["temporal_range_ms"], res["temporal_range_min_ms"] = timed(T, plan, cols, "temporal", args.steps)
        for name, params in modes.items():
            plan = T.Plan([spec(T.VALUE_RULE, 0)])
            plan.set_value_rule(0, **params)
            st, ms, mn = timed(T, plan, cols, "value_rule", args.steps)
            seen, considered, valid, errors = st.value_rule_counts(0)
            assert seen == considered == n and 0 < valid < n and (errors > 0) == (name == "integer")
            res[name + "_ms"], res[name + "_min_ms"] = ms, mn
            res[name + "_counts"] = [seen, considered, valid, errors]
            res[name + "_hbm_fraction"] = n * 8 / (ms * 1e-3) / HBM_PEAK
        plan = T.Plan([spec(T.VALUE_RULE, 0)] * len(eight))
        for i, params in enumerate(eight):
            plan.set_value_rule(i, **params)
        st, res["eight_rules_ms"], res["eight_rules_min_ms"] = timed(T, plan, cols, "value_rule", args.steps)
        assert [st.value_rule_counts(i) for i in range(5)] == [tuple(res[m + "_counts"]) for m in modes]
        res["eight_rules_hbm_fraction"] = n * 8 / (res["eight_rules_ms"] * 1e-3) / HBM_PEAK
        print("%d rows, %s: numeric_stats %.2f ms | temporal range %s ms | ge_zero %.2f | gt_zero %.2f | between %.2f | "
              "between as double %.2f | integer %.2f | eight rules in one walk %.2f ms  (HBM share of one rule on 8 B per row: %.2f)"
              % (n, dtype, res["numeric_stats_ms"], "%.2f" % res["temporal_range_ms"] if "temporal_range_ms" in res else "-",
                 res["ge_zero_ms"], res["gt_zero_ms"], res["between_ms"], res["between_as_double_ms"], res["integer_ms"],
                 res["eight_rules_ms"], res["ge_zero_hbm_fraction"]), flush=True)
        del cols, vals
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
