#!/usr/bin/env python3
"""The three TGX_CHECK_TEMPORAL modes alone beside the stand-alone COMOMENTS pass over the same two columns, in one
process: two Int64 columns of millisecond instants, no NULLs, --rows rows, on DEVICE, one batch.  Order mode reads what
the co-moment kernel reads (16 B per row) and does less arithmetic: that kernel is its yardstick.  The single-column
modes read 8 B per row.  Kernel times are HIP-event times on the state's stream (tgx_profile_get), the median of
--steps steps after one warm-up step of every shape.
    python tools/bench_temporal.py [--rows 1000000000] [--steps 5] [--json out.json]"""
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
    gen = torch.Generator(device="cuda").manual_seed(0x7E570011)
    day_ms = 86400 * 1000
    # created_at over +-30 years around the epoch; processed_at up to 30 s later, 10 % of the rows earlier
    before = torch.randint(-30 * 365 * day_ms, 30 * 365 * day_ms, (n,), dtype=torch.int64, device="cuda", generator=gen)
    after = before + torch.randint(-3000, 30000, (n,), dtype=torch.int64, device="cuda", generator=gen)
    cols = [T.Column.int64(before, None, length=n), T.Column.int64(after, None, length=n)]
    out = {"rows": n}
    # (a variance check on x keeps the pair off the fused scan: the stand-alone comoments_kernel runs, timed alone)
    como = T.Plan([spec(T.COMOMENTS, 0, column2=1), spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE)])
    _, out["comoments_ms"], out["comoments_min_ms"] = timed(T, como, cols, "comoments", args.steps)
    modes = {
        "order": (1, dict(mode=T.TEMPORAL_ORDER, delta=0), 16),
        "time_of_day": (-1, dict(mode=T.TEMPORAL_TIME_OF_DAY, flags=T.TEMPORAL_WEEKDAYS_ONLY, ticks_per_second=1000,
                                 tod_lo=9 * 3600 * 1000, tod_hi=17 * 3600 * 1000), 8),
        "range": (-1, dict(mode=T.TEMPORAL_RANGE, lo=-10 * 365 * day_ms, hi=10 * 365 * day_ms), 8),
    }
    for name, (column2, params, row_bytes) in modes.items():
        plan = T.Plan([spec(T.TEMPORAL, 0, column2=column2)])
        plan.set_temporal(0, **params)
        st, ms, mn = timed(T, plan, cols, "temporal", args.steps)
        seen, considered, violations = st.temporal_counts(0)
        assert seen == n and 0 < violations < considered <= n
        out[name + "_ms"], out[name + "_min_ms"] = ms, mn
        out[name + "_counts"] = [seen, considered, violations]
        out[name + "_hbm_fraction"] = n * row_bytes / (ms * 1e-3) / HBM_PEAK
    out["comoments_hbm_fraction"] = n * 16 / (out["comoments_ms"] * 1e-3) / HBM_PEAK
    print("%d rows: comoments %.2f ms | order %.2f ms | time of day (weekdays) %.2f ms | range %.2f ms  (HBM share on "
          "16 / 16 / 8 / 8 B per row: %.2f | %.2f | %.2f | %.2f)"
          % (n, out["comoments_ms"], out["order_ms"], out["time_of_day_ms"], out["range_ms"],
             out["comoments_hbm_fraction"], out["order_hbm_fraction"], out["time_of_day_hbm_fraction"],
             out["range_hbm_fraction"]), flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
