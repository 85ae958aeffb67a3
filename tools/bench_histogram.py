#!/usr/bin/env python3
"""The histogram check alone (TGX_CHECK_HISTOGRAM, both phases) beside its two comparators, in one process: one Float64
column, no NULLs, --rows rows (default: 100 M and 1 G), 10 and 1000 buckets, on shuffled, sorted and constant data.
Comparators: the stand-alone NUMERIC_STATS scan of the same column (the same bytes: 8 B per row -- the column has no
validity bitmap --, the figure the share of HBM bandwidth is taken on) and the JOINT_BINS count phase over (x, x) with
127 bins of width (max - min) / 127, which puts the maximum into bin 127 (twice the bytes, the same kind of LDS
atomics).  Kernel times are HIP-event times on the state's stream
(tgx_profile_get), the median of --steps steps after one warm-up step of every shape.
    python tools/bench_histogram.py [--rows 100000000 1000000000] [--steps 5] [--json out.json]"""
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


def reference_edges(mn, mx, buckets):
    """histogram.rs:253-275 in Python floats"""
    rng = mx - mn
    w = rng / float(buckets) if rng > 0.0 and buckets > 1 else 1.0
    return [mn + (float(i) * w) for i in range(buckets)] + [mx + w * 0.001]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000_000, 1_000_000_000])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import term_amd as T
    from term_amd._lib import spec

    T.init(flags=T.OPT_NO_COALESCE)
    gen = torch.Generator(device="cuda").manual_seed(0x7E570012)
    out = {}
    for rows in args.rows:
        n = rows // 64 * 64
        for order in ("shuffled", "sorted", "constant"):
            if order == "shuffled":
                x = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
            elif order == "sorted":
                x = torch.sort(torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)).values
            else:
                x = torch.full((n,), 42.0, dtype=torch.float64, device="cuda")
            col = T.Column.float64(x, None, length=n)
            row = {}
            _, row["stats_ms"], row["stats_min_ms"] = timed(T, T.Plan([spec(T.NUMERIC_STATS, 0)]), [col], "scan", args.steps)
            st, row["range_ms"], row["range_min_ms"] = timed(T, T.Plan([spec(T.HISTOGRAM, 0)]), [col], "hist_range", args.steps)
            r = st.histogram_range(0)
            assert r["n"] == n
            for buckets in (10, 1000):
                plan = T.Plan([spec(T.HISTOGRAM, 0)])
                plan.set_histogram_edges(0, reference_edges(r["min"], r["max"], buckets))
                st2, ms, mn = timed(T, plan, [col], "hist_counts", args.steps)
                counts, else_rows, _ = st2.histogram_counts(0)
                assert sum(counts) == n
                row["counts_%d_ms" % buckets], row["counts_%d_min_ms" % buckets] = ms, mn
                row["counts_%d_nonzero" % buckets], row["counts_%d_else_rows" % buckets] = sum(1 for c in counts if c), else_rows
            jplan = T.Plan([spec(T.JOINT_BINS, 0, column2=1)])
            width = (r["max"] - r["min"]) / 127 if r["max"] > r["min"] else 1.0
            jplan.set_joint_binning(0, r["min"], width, r["min"], width, 127)
            st3, row["joint_127_ms"], row["joint_127_min_ms"] = timed(T, jplan, [col, col], "joint_bins", args.steps)
            assert sum(st3.joint_counts(0)[0]) == n
            for k in ("stats_ms", "range_ms", "counts_10_ms", "counts_1000_ms"):
                row[k.replace("_ms", "_hbm_fraction")] = n * 8.0 / (row[k] * 1e-3) / HBM_PEAK
            row["counts_1000_over_joint_127"] = row["counts_1000_ms"] / row["joint_127_ms"]
            row["counts_1000_over_stats"] = row["counts_1000_ms"] / row["stats_ms"]
            row["range_over_stats"] = row["range_ms"] / row["stats_ms"]
            out["%d_%s" % (n, order)] = row
            print("%d rows, %s: stats %.3f ms | range %.3f ms | 10 buckets %.3f ms | 1000 buckets %.3f ms | joint 127 bins "
                  "%.3f ms  (1000 buckets / joint %.2f, / stats %.2f; range / stats %.2f)"
                  % (n, order, row["stats_ms"], row["range_ms"], row["counts_10_ms"], row["counts_1000_ms"],
                     row["joint_127_ms"], row["counts_1000_over_joint_127"], row["counts_1000_over_stats"],
                     row["range_over_stats"]), flush=True)
            del x, col
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
