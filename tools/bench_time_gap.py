#!/usr/bin/env python3
"""TGX_CHECK_TIME_GAP alone, in one process: --rows timestamps (Int64 ticks, no NULLs) on DEVICE, one batch, whole table
and per group.  Timestamps shuffled, already sorted and constant; 1 k and 10 M groups (shuffled timestamps).  Per shape
the median of --steps steps after one warm-up step:
    append      the compaction kernel of tgx_update (HIP-event time on the state's stream, tgx_profile_get)
    sort        the sort jobs of the finalize -- whole table: ONE bare keys-only sort of the rows, the yardstick every
                other number here is read against; per group: the three sorts of the grouped route
    neighbours  the pass over the sorted rows
    finalize    wall time of the read (tgx_time_gap_get), host waits included
The steps of all shapes run in this one process, one after the other.
    python tools/bench_time_gap.py [--rows 1000000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes / s (MI355X, HBM3E)


def timed(T, plan, cols, steps):
    import torch

    st = T.State(plan)
    st.profile_enable(True)
    keys = ("time_gap_append", "time_gap_sort", "time_gap_neighbours")
    rows = {k: [] for k in keys + ("finalize",)}
    counts = None
    for it in range(steps + 1):
        st.reset()
        st.profile_reset()
        st.update(cols)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        counts = st.time_gap_counts(0)
        wall = (time.perf_counter() - t0) * 1e3
        if it:  # (step 0 warms the shape up: its work buffers are allocated there)
            for k in keys:
                rows[k].append(st.profile_get(k)["total_ms"])
            rows["finalize"].append(wall)
    st.close()
    return {k: statistics.median(v) for k, v in rows.items()}, counts


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
    gen = torch.Generator(device="cuda").manual_seed(0x7E570013)
    span = 30 * 365 * 86400 * 1000  # millisecond instants over +-30 years around the epoch
    shuffled = torch.randint(-span, span, (n,), dtype=torch.int64, device="cuda", generator=gen)
    out = {"rows": n, "shapes": {}}
    max_gap = 2 * span // n * 4  # four times the mean gap of the shuffled table
    shapes = [("whole_shuffled", shuffled, None), ("whole_sorted", None, None), ("whole_constant", None, None),
              ("groups_1k", shuffled, 1000), ("groups_10m", shuffled, 10_000_000)]
    for name, t, groups in shapes:
        if name == "whole_sorted":
            t = torch.arange(n, dtype=torch.int64, device="cuda") * 7 - span
        elif name == "whole_constant":
            t = torch.full((n,), 1_700_000_000_000, dtype=torch.int64, device="cuda")
        cols = [T.Column.int64(t, None, length=n)]
        if groups:
            g = torch.randint(0, groups, (n,), dtype=torch.int64, device="cuda", generator=gen)
            cols.append(T.Column.int64(g, None, length=n))
        plan = T.Plan([spec(T.TIME_GAP, 0, column2=1 if groups else -1)])
        plan.set_time_gap(0, max_gap * (groups or 1))
        ms, counts = timed(T, plan, cols, args.steps)
        seen, rows, gaps, violations, largest = counts
        assert seen == rows == n and (gaps == n - 1 if not groups else n - groups <= gaps < n)
        ms["counts"] = list(counts)
        out["shapes"][name] = ms
        print("%-15s %d rows: append %.2f ms | sort %.2f ms | neighbours %.2f ms | finalize (wall) %.2f ms   gaps %d, "
              "violations %d" % (name, n, ms["time_gap_append"], ms["time_gap_sort"], ms["time_gap_neighbours"],
                                 ms["finalize"], gaps, violations), flush=True)
        del cols, t
    w = out["shapes"]["whole_shuffled"]
    read_ms = n * 8 / HBM_PEAK * 1e3
    out["bare_sort_ms"] = w["time_gap_sort"]
    out["whole_finalize_over_sort_plus_read"] = w["finalize"] / (w["time_gap_sort"] + read_ms)
    out["groups_1k_finalize_over_bare_sort"] = out["shapes"]["groups_1k"]["finalize"] / w["time_gap_sort"]
    out["groups_10m_finalize_over_bare_sort"] = out["shapes"]["groups_10m"]["finalize"] / w["time_gap_sort"]
    print("bare keys-only sort %.2f ms; whole-table finalize / (sort + one 8 B/row read at HBM peak) = %.3f; per-group "
          "finalize / bare sort = %.2f (1 k groups), %.2f (10 M groups)"
          % (out["bare_sort_ms"], out["whole_finalize_over_sort_plus_read"], out["groups_1k_finalize_over_bare_sort"],
             out["groups_10m_finalize_over_bare_sort"]), flush=True)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
