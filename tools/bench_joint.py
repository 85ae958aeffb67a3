#!/usr/bin/env python3
"""Joint bin counts alone (TGX_CHECK_JOINT_BINS, both phases) beside the stand-alone COMOMENTS pass over the same two
columns, in one process: Int64 x Float64, no NULLs, --rows rows, 10 and 127 bins, on (a) independent shuffled input and
(b) sorted y = 2x.  Same bytes per row for all three kernels (16 B; 16.25 B with validity bitmaps, the figure the
share of HBM bandwidth is taken on): the co-moment kernel is the yardstick.  Kernel times are HIP-event times on the
state's stream (tgx_profile_get), the median of --steps steps after one warm-up step of every shape.
    python tools/bench_joint.py [--rows 1000000000] [--steps 5] [--json out.json]"""
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
    gen = torch.Generator(device="cuda").manual_seed(0x7E570010)
    out = {"rows": n}
    for shape in ("independent", "sorted_y_2x"):
        if shape == "independent":
            x = torch.randint(-10**9, 10**9, (n,), dtype=torch.int64, device="cuda", generator=gen)
            y = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        else:
            x = torch.arange(n, dtype=torch.int64, device="cuda")
            y = (2 * x).to(torch.float64)
        cols = [T.Column.int64(x, None, length=n), T.Column.float64(y, None, length=n)]
        row = {}
        # (a variance check on x keeps the pair off the fused scan: the stand-alone comoments_kernel runs, timed alone)
        como = T.Plan([spec(T.COMOMENTS, 0, column2=1), spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE)])
        _, row["comoments_ms"], row["comoments_min_ms"] = timed(T, como, cols, "comoments", args.steps)
        st, row["range_ms"], row["range_min_ms"] = timed(T, T.Plan([spec(T.JOINT_BINS, 0, column2=1)]), cols,
                                                         "joint_range", args.steps)
        r = st.joint_range(0)
        assert r["n"] == n
        for bins in (10, 127):
            plan = T.Plan([spec(T.JOINT_BINS, 0, column2=1)])
            xw, yw = (r["x_max"] - r["x_min"]) / bins, (r["y_max"] - r["y_min"]) / bins
            plan.set_joint_binning(0, r["x_min"], xw, r["y_min"], yw, bins)
            st2, ms, mn = timed(T, plan, cols, "joint_bins", args.steps)
            cells, outside = st2.joint_counts(0)
            assert sum(cells) == n and outside == 0
            row["bins_%d_ms" % bins], row["bins_%d_min_ms" % bins] = ms, mn
            row["bins_%d_nonzero_cells" % bins] = sum(1 for c in cells if c)
        for k in ("comoments_ms", "range_ms", "bins_10_ms", "bins_127_ms"):
            row[k.replace("_ms", "_hbm_fraction")] = n * 16.25 / (row[k] * 1e-3) / HBM_PEAK
        out[shape] = row
        print("%s, %d rows: comoments %.2f ms | range %.2f ms | 10 bins %.2f ms | 127 bins %.2f ms  (HBM share on "
              "16.25 B/row: %.2f | %.2f | %.2f | %.2f)"
              % (shape, n, row["comoments_ms"], row["range_ms"], row["bins_10_ms"], row["bins_127_ms"],
                 row["comoments_hbm_fraction"], row["range_hbm_fraction"], row["bins_10_hbm_fraction"],
                 row["bins_127_hbm_fraction"]), flush=True)
        del x, y, cols
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
