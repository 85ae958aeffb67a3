#!/usr/bin/env python3
"""TGX_CHECK_PAIR_COUNTS beside its neighbours, in one process: two columns of 8-byte strings -- x as Utf8, as an
all-inline Utf8View and as a Dictionary<Int32, Utf8>, y as Utf8 -- at 16 and 10 000 distinct pairs, against VALUE_COUNTS
on either side alone (the row does both sides' fingerprints and one chained one: expect no better than their sum) and
against DISTINCT by fingerprint on the pair as a 2-tuple; and one mixed pair, Int64 with 10 bins x Utf8, in both phases.
Columns on DEVICE, one batch, no NULLs.  Kernel times are HIP-event times on the state's stream (tgx_profile_get), the
median of --steps steps after one warm-up step of every shape.  There is no gate: the figures go into DESIGN.md.
    python tools/bench_pair_counts.py [--rows 100000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import term_amd as T
    from term_amd._lib import spec

    T.init(flags=T.OPT_NO_COALESCE)
    m = args.rows // 64 * 64
    out = {"rows": m, "strings": {}, "mixed": {}}
    gen = torch.Generator(device="cuda").manual_seed(0x7E570016)
    shifts = torch.arange(8, device="cuda", dtype=torch.int64) * 4
    offsets = (torch.arange(m + 1, device="cuda", dtype=torch.int64) * 8).to(torch.int32)

    def letters_of(ids, first):
        """8-byte strings: letter j is `first` + hex digit j of the id"""
        return (((ids[:, None] >> shifts[None, :]) & 15) + first).to(torch.uint8)  # [m, 8]

    def utf8_of(letters):
        return T.Column.utf8(offsets, torch.cat([letters.reshape(-1), torch.zeros(64, dtype=torch.uint8, device="cuda")]),
                             None, length=m)

    def value_counts_ms(col):
        plan = T.Plan([spec(T.VALUE_COUNTS, 0)])
        plan.set_value_counts(0, 65536, 256)
        st, ms, _ = timed(T, plan, [col], "value_counts", args.steps)
        assert st.value_counts(0)[0]["counted"] == m
        return ms

    for k, kx in ((16, 4), (10_000, 100)):
        pid = (torch.rand(m, device="cuda", generator=gen) * k).to(torch.int64).clamp_(0, k - 1)
        xid, yid = pid % kx, pid // kx
        xl = letters_of(xid, 97)
        ycol = utf8_of(letters_of(yid, 65))
        views = torch.zeros((m, 16), dtype=torch.uint8, device="cuda")
        views[:, 0] = 8
        views[:, 4:12] = xl
        entry_ids = np.arange(kx, dtype=np.int64)
        entry_letters = (((entry_ids[:, None] >> (np.arange(8) * 4)[None, :]) & 15) + 97).astype(np.uint8)
        dictionary = T.Column.utf8(torch.from_numpy(np.arange(kx + 1, dtype=np.int32) * 8).cuda(),
                                   torch.from_numpy(np.concatenate([entry_letters.reshape(-1), np.zeros(64, np.uint8)])).cuda())
        layouts = {"utf8": utf8_of(xl), "utf8_view": T.Column.utf8_view(views.reshape(-1), [], None, length=m),
                   "dictionary": T.Column.dict32_utf8(xid.to(torch.int32), dictionary, None, length=m)}
        del xl
        torch.cuda.synchronize()  # (the library runs on a stream of its own: the columns must be finished)
        y_ms = value_counts_ms(ycol)
        for layout, xcol in layouts.items():
            plan = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1)])
            plan.set_pair_counts(0, max_pairs=65536, max_value_bytes=256)
            st, ms, mn = timed(T, plan, [xcol, ycol], "pair_counts", args.steps)
            summary, _ = st.pair_counts(0)
            assert summary["counted"] == m and summary["overflow_rows"] == 0 and 0 < summary["distinct"] <= k, summary
            x_ms = value_counts_ms(xcol)
            dst, dms, _ = timed(T, T.Plan([spec(T.DISTINCT, 0, columns=[0, 1])]), [xcol, ycol], "distinct", args.steps)
            assert dst.finalize()[0].distinct == summary["distinct"]
            out["strings"]["%s_%d" % (layout, k)] = {
                "pair_counts_ms": ms, "pair_counts_min_ms": mn, "value_counts_x_ms": x_ms, "value_counts_y_ms": y_ms,
                "ratio_to_sum": ms / (x_ms + y_ms), "distinct_tuple_ms": dms, "ratio_to_tuple_distinct": ms / dms,
                "distinct": summary["distinct"]}
            print("%d rows, %-10s x utf8 %6d pairs: pair_counts %.2f ms | value_counts x %.2f + y %.2f ms (ratio to the sum "
                  "%.2f) | DISTINCT of the 2-tuple %.2f ms (ratio %.2f)"
                  % (m, layout, k, ms, x_ms, y_ms, ms / (x_ms + y_ms), dms, ms / dms), flush=True)
        if k == 16:  # the mixed pair: Int64 with 10 bins x Utf8, both phases
            nums = (torch.rand(m, device="cuda", generator=gen) * 1000).to(torch.int64)
            torch.cuda.synchronize()
            ncol = T.Column.int64(nums, None, length=m)
            first = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1)])
            first.set_pair_counts(0, x="range", max_pairs=65536)
            st, rms, _ = timed(T, first, [ncol, ycol], "pair_range", args.steps)
            r = st.pair_range(0)
            width = (r["max"] - r["min"]) / 10
            second = T.Plan([spec(T.PAIR_COUNTS, 0, column2=1)])
            second.set_pair_counts(0, x=(r["min"], width, 10), max_pairs=65536)
            st, cms, _ = timed(T, second, [ncol, ycol], "pair_counts", args.steps)
            summary, _ = st.pair_counts(0)
            assert summary["counted"] == m and summary["out_of_range"] == 0, summary
            out["mixed"]["int64_10bins_x_utf8_%d" % (k // kx)] = {"pair_range_ms": rms, "pair_counts_ms": cms,
                                                                  "value_counts_y_ms": y_ms, "distinct": summary["distinct"]}
            print("%d rows, Int64 in 10 bins x utf8 (%d values): range phase %.2f ms | count phase %.2f ms | value_counts y "
                  "%.2f ms" % (m, k // kx, rms, cms, y_ms), flush=True)
            del nums, ncol
        del layouts, views, pid, xid, yid, ycol
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
