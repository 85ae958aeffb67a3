#!/usr/bin/env python3
"""TGX_CHECK_GROUP_SUMS beside TGX_CHECK_GROUP_COUNTS (one value column) on the same group column, in one process and
interleaved step by step: an Int64 group column with 1 .. 60 000 distinct keys -- below, around and beyond the 4096 slots
of the workgroup's LDS table -- uniform and Zipf-like (floor(K^u), u uniform: P(k) ~ 1/k), and a Utf8, an all-inline
Utf8View and a Dictionary<Int32, Utf8> column of 8-byte strings; each with an Int64 and with a Float64 value column (one
validity bitmap, 10 % NULLs, at Arrow offset 1).  GROUP_COUNTS is the same walk minus the values and the sum.  Columns on
DEVICE, one batch, no NULL keys.  Kernel times are HIP-event times on the state's stream (tgx_profile_get), the median of
--steps steps after one warm-up step of every shape; the roofline share prices the kind's own bytes -- key, value and the
value's validity bit a row -- at 8 TB/s.  There is no gate: the figures go into DESIGN.md.
    python tools/bench_group_sums.py [--rows 100000000] [--string-rows 100000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12


def interleaved(T, runs, steps):
    """runs: [(plan, cols, kernel)]: every step runs each of them once, in turn -> [(median ms, min ms, state)]"""
    states = []
    for plan, _, _ in runs:
        st = T.State(plan)
        st.profile_enable(True)
        states.append(st)
    times = [[] for _ in runs]
    for it in range(steps + 1):
        for k, (st, (_, cols, kernel)) in enumerate(zip(states, runs)):
            st.reset()
            st.profile_reset()
            st.update(cols)
            st.finalize()
            if it:  # (step 0 warms the shape up)
                times[k].append(st.profile_get(kernel)["total_ms"])
    return [(statistics.median(t), min(t), st) for t, st in zip(times, states)]


def ids_of(torch, n, k, zipf, gen):
    u = torch.rand(n, device="cuda", generator=gen)
    if zipf:
        return (torch.pow(float(k), u).to(torch.int64) - 1).clamp_(0, k - 1)
    return (u * k).to(torch.int64).clamp_(0, k - 1)


def value_columns(T, torch, n, gen):
    """(the validity-only view GROUP_COUNTS reads, an Int64 column, a Float64 column) over one bitmap: 10 % NULLs,
    Arrow offset 1"""
    off = 1
    bits = torch.rand(n + off + 64, device="cuda", generator=gen) >= 0.1
    bits = bits[: (len(bits) // 8) * 8].reshape(-1, 8).to(torch.uint8)
    packed = (bits << torch.arange(8, device="cuda", dtype=torch.uint8)[None, :]).sum(dim=1).to(torch.uint8)
    iv = torch.randint(-2**40, 2**40, (n + off,), device="cuda", generator=gen, dtype=torch.int64)
    fv = torch.randn(n + off, device="cuda", generator=gen, dtype=torch.float64)
    return (T.Column(T.INT64, n, values=None, validity=packed, offset=off, mem=T.MEM_DEVICE),
            T.Column(T.INT64, n, values=iv, validity=packed, offset=off, mem=T.MEM_DEVICE),
            T.Column(T.FLOAT64, n, values=fv, validity=packed, offset=off, mem=T.MEM_DEVICE)), (packed, iv, fv)


def measure(T, spec, group_col, values, n, k, key_bytes, steps):
    """GROUP_COUNTS with one value column, GROUP_SUMS of Int64 and of Float64 values on one group column -> a dict"""
    flags, ints, floats = values
    cplan = T.Plan([spec(T.GROUP_COUNTS, 1, column2=0)])
    cplan.set_group_counts(0, 65536, 256)
    runs = [(cplan, [group_col, flags], "group_counts")]
    for col in (ints, floats):
        plan = T.Plan([spec(T.GROUP_SUMS, 1, column2=0)])
        plan.set_group_sums(0, 65536, 256)
        runs.append((plan, [group_col, col], "group_sums"))
    got = interleaved(T, runs, steps)
    (cms, cmn, cst) = got[0]
    counts, _ = cst.group_counts(0)
    assert counts["counted"] == n and counts["overflow_rows"] == 0 and 0 < counts["groups"] <= k, counts
    own_bytes = n * (key_bytes + 8) + n // 8
    row = {"group_counts_ms": cms, "group_counts_min_ms": cmn, "groups": counts["groups"], "own_bytes": own_bytes}
    for name, (ms, mn, st) in zip(("int64", "float64"), got[1:]):
        s, _ = st.group_sums(0)
        assert s["counted"][0] == n and s["overflow"][0] == 0 and s["groups"] == counts["groups"], s
        assert s["counted"][1] == counts["counted_non_null"] and st.profile_get("group_sums")["launches"] == 1
        assert s["is_float"] == (name == "float64")
        row["group_sums_%s_ms" % name] = ms
        row["group_sums_%s_min_ms" % name] = mn
        row["ratio_%s" % name] = ms / cms
        row["roofline_%s" % name] = own_bytes / (ms * 1e-3) / HBM_BYTES_PER_S
    return row


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
    m = args.string_rows // 64 * 64
    out = {"rows": n, "int64": {}, "strings": {}}
    gen = torch.Generator(device="cuda").manual_seed(0x7E570018)
    values, _keep = value_columns(T, torch, max(n, m), gen)

    def sized(cols, rows):
        return [c.sliced(0, rows) for c in cols]

    def report(what, name, rows, row):
        print("%d rows, %s, %-14s group_counts, 1 value column %.2f ms | group_sums Int64 %.2f ms (x %.2f, %.0f %% of "
              "8 TB/s) | Float64 %.2f ms (x %.2f, %.0f %%)" %
              (rows, what, name, row["group_counts_ms"], row["group_sums_int64_ms"], row["ratio_int64"],
               100 * row["roofline_int64"], row["group_sums_float64_ms"], row["ratio_float64"], 100 * row["roofline_float64"]),
              flush=True)

    shapes = [(1, False), (16, False), (1000, False), (1000, True), (3000, False), (10_000, False), (60_000, False),
              (60_000, True)]
    for k, zipf in shapes if n else ():
        name = "%d_%s" % (k, "zipf" if zipf else "uniform")
        keys = ids_of(torch, n, k, zipf, gen) * 7919 - 1000  # (spread keys: the keys are not the ids themselves)
        torch.cuda.synchronize()  # (the library runs on a stream of its own: the column must be finished)
        row = measure(T, spec, T.Column.int64(keys, None, length=n), sized(values, n), n, k, 8, args.steps)
        out["int64"][name] = row
        report("Int64", name, n, row)
        del keys
    torch.cuda.empty_cache()

    # 8-byte strings "aaaaaaaa" .. : letter j is 'a' + hex digit j of the id
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
        layouts = {"utf8": (T.Column.utf8(offsets, data, None, length=m), 12),  # (a 4-byte offset and 8 bytes a row)
                   "utf8_view": (T.Column.utf8_view(views.reshape(-1), [], None, length=m), 16),
                   "dictionary": (T.Column.dict32_utf8(ids.to(torch.int32), dictionary, None, length=m), 4)}
        del letters
        torch.cuda.synchronize()
        for layout, (col, key_bytes) in layouts.items():
            row = measure(T, spec, col, sized(values, m), m, k, key_bytes, args.steps)
            out["strings"]["%s_%d" % (layout, k)] = row
            report(layout, "%d values" % k, m, row)
        del layouts, ids, data, offsets, views
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
