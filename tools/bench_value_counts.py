#!/usr/bin/env python3
"""TGX_CHECK_VALUE_COUNTS beside its two neighbours, in one process: an Int64 column with 2 .. 60 000 distinct values,
uniform and Zipf-like (floor(K^u), u uniform: P(k) ~ 1/k), against HISTOGRAM's count phase on the same column (the
same 8 B + 1 bit per row, also one LDS atomic per row); and a Utf8, an all-inline Utf8View and a Dictionary<Int32, Utf8>
column of 8-byte strings against DISTINCT by fingerprint on the same strings.  One column on DEVICE, one batch, no
NULLs.  Kernel times are HIP-event times on the state's stream (tgx_profile_get), the median of --steps steps after one
warm-up step of every shape.  There is no gate: the figures go into DESIGN.md.
    python tools/bench_value_counts.py [--rows 100000000] [--string-rows 100000000] [--steps 5] [--json out.json]"""
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


def ids_of(torch, n, k, zipf, gen):
    u = torch.rand(n, device="cuda", generator=gen)
    if zipf:
        return (torch.pow(float(k), u).to(torch.int64) - 1).clamp_(0, k - 1)
    return (u * k).to(torch.int64).clamp_(0, k - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--string-rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import term_amd as T
    from term_amd._lib import spec

    T.init(flags=T.OPT_NO_COALESCE)
    n = args.rows // 64 * 64
    out = {"rows": n, "int64": {}, "strings": {}}
    gen = torch.Generator(device="cuda").manual_seed(0x7E570015)
    for k in (2, 16, 1000, 10_000, 60_000):
        for zipf in (False, True):
            name = "%d_%s" % (k, "zipf" if zipf else "uniform")
            vals = ids_of(torch, n, k, zipf, gen) * 7919 - 1000  # (spread values: the keys are not the ids themselves)
            torch.cuda.synchronize()  # (the library runs on a stream of its own: the column must be finished)
            cols = [T.Column.int64(vals, None, length=n)]
            plan = T.Plan([spec(T.VALUE_COUNTS, 0)])
            plan.set_value_counts(0, 65536, 256)
            st, ms, mn = timed(T, plan, cols, "value_counts", args.steps)
            summary, counts = st.value_counts(0)
            assert summary["counted"] == n and summary["overflow_rows"] == 0 and 0 < summary["distinct"] <= k, summary
            hplan = T.Plan([spec(T.HISTOGRAM, 0)])
            hplan.set_histogram_edges(0, [float(-1000 + 7919 * k * b / 16) for b in range(17)])
            _, hms, hmn = timed(T, hplan, cols, "hist_counts", args.steps)
            out["int64"][name] = {"value_counts_ms": ms, "value_counts_min_ms": mn, "histogram_counts_ms": hms,
                                  "histogram_counts_min_ms": hmn, "ratio": ms / hms, "distinct": summary["distinct"],
                                  "hbm_fraction": n * 8 / (ms * 1e-3) / HBM_PEAK}
            print("%d rows, Int64, %-14s value_counts %.2f ms | histogram count phase (16 buckets) %.2f ms | ratio %.2f | "
                  "HBM share on 8 B per row %.2f" % (n, name, ms, hms, ms / hms, out["int64"][name]["hbm_fraction"]), flush=True)
            del cols, vals
    torch.cuda.empty_cache()

    # 8-byte strings "aaaaaaaa" .. : letter j is 'a' + hex digit j of the id
    m = args.string_rows // 64 * 64
    out["string_rows"] = m
    for k in (16, 10_000) if m else ():
        ids = ids_of(torch, m, k, False, gen)
        shifts = torch.arange(8, device="cuda", dtype=torch.int64) * 4
        letters = (((ids[:, None] >> shifts[None, :]) & 15) + 97).to(torch.uint8)  # [m, 8]
        data = torch.cat([letters.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")])
        offsets = (torch.arange(m + 1, device="cuda", dtype=torch.int64) * 8).to(torch.int32)
        views = torch.zeros((m, 16), dtype=torch.uint8, device="cuda")
        views[:, 0] = 8
        views[:, 4:12] = letters
        entry_ids = np.arange(k, dtype=np.int64)
        entry_letters = (((entry_ids[:, None] >> (np.arange(8) * 4)[None, :]) & 15) + 97).astype(np.uint8)
        dictionary = T.Column.utf8(torch.from_numpy(np.arange(k + 1, dtype=np.int32) * 8).cuda(),
                                   torch.from_numpy(np.concatenate([entry_letters.reshape(-1), np.zeros(64, np.uint8)])).cuda())
        layouts = {"utf8": T.Column.utf8(offsets, data, None, length=m),
                   "utf8_view": T.Column.utf8_view(views.reshape(-1), [], None, length=m),
                   "dictionary": T.Column.dict32_utf8(ids.to(torch.int32), dictionary, None, length=m)}
        del letters
        torch.cuda.synchronize()
        for layout, col in layouts.items():
            plan = T.Plan([spec(T.VALUE_COUNTS, 0)])
            plan.set_value_counts(0, 65536, 256)
            st, ms, mn = timed(T, plan, [col], "value_counts", args.steps)
            summary, _ = st.value_counts(0)
            assert summary["counted"] == m and summary["overflow_rows"] == 0 and 0 < summary["distinct"] <= k
            dst, dms, dmn = timed(T, T.Plan([spec(T.DISTINCT, 0)]), [col], "distinct", args.steps)
            assert dst.finalize()[0].distinct == summary["distinct"]
            out["strings"]["%s_%d" % (layout, k)] = {"value_counts_ms": ms, "value_counts_min_ms": mn, "distinct_ms": dms,
                                                     "distinct_min_ms": dmn, "ratio": ms / dms, "distinct": summary["distinct"]}
            print("%d rows, %-10s %6d values: value_counts %.2f ms | DISTINCT by fingerprint %.2f ms | ratio %.2f"
                  % (m, layout, k, ms, dms, ms / dms), flush=True)
        del layouts, ids, data, offsets, views
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
