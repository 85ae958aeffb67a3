#!/usr/bin/env python3
"""TGX_CHECK_GROUP_COUNTS beside TGX_CHECK_VALUE_COUNTS on the same group column, in one process and interleaved step by
step: an Int64 group column with 1 .. 60 000 distinct keys, uniform and Zipf-like (floor(K^u), u uniform: P(k) ~ 1/k),
and a Utf8, an all-inline Utf8View and a Dictionary<Int32, Utf8> column of 8-byte strings, each with 1 and with 8 value
columns riding the walk (every value column has a validity bitmap of its own, 10 % NULLs, at an Arrow offset of its
own).  VALUE_COUNTS is the same walk minus the validity bits and the wider slots.  Columns on DEVICE, one batch, no NULL
keys.  Kernel times are HIP-event times on the state's stream (tgx_profile_get), the median of --steps steps after one
warm-up step of every shape.  There is no gate: the figures go into DESIGN.md.
    python tools/bench_group_counts.py [--rows 100000000] [--string-rows 100000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MEMBERS = (1, 8)


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
    """eight validity-only value columns: a bitmap each, 10 % NULLs, Arrow offsets 1, 10, 19, .."""
    cols = []
    for m in range(max(MEMBERS)):
        off = 1 + 9 * m
        bits = torch.rand(n + off + 64, device="cuda", generator=gen) >= 0.1
        bits = bits[: (len(bits) // 8) * 8].reshape(-1, 8).to(torch.uint8)
        packed = (bits << torch.arange(8, device="cuda", dtype=torch.uint8)[None, :]).sum(dim=1).to(torch.uint8)
        cols.append(T.Column(T.INT64, n, values=None, validity=packed, offset=off, mem=T.MEM_DEVICE))
    return cols


def measure(T, spec, group_col, values, n, k, steps):
    """VALUE_COUNTS and GROUP_COUNTS with 1 and 8 members on one group column -> a dict of figures"""
    vplan = T.Plan([spec(T.VALUE_COUNTS, 0)])
    vplan.set_value_counts(0, 65536, 256)
    runs = [(vplan, [group_col], "value_counts")]
    for members in MEMBERS:
        plan = T.Plan([spec(T.GROUP_COUNTS, 1 + m, column2=0) for m in range(members)])
        for m in range(members):
            plan.set_group_counts(m, 65536, 256)
        runs.append((plan, [group_col] + values[:members], "group_counts"))
    got = interleaved(T, runs, steps)
    (vms, vmn, vst) = got[0]
    summary, _ = vst.value_counts(0)
    assert summary["counted"] == n and summary["overflow_rows"] == 0 and 0 < summary["distinct"] <= k, summary
    row = {"value_counts_ms": vms, "value_counts_min_ms": vmn, "distinct": summary["distinct"]}
    for members, (ms, mn, st) in zip(MEMBERS, got[1:]):
        s, _ = st.group_counts(members - 1)
        assert s["counted"] == n and s["overflow_rows"] == 0 and s["groups"] == summary["distinct"], s
        assert 0 < s["counted_non_null"] < n and st.profile_get("group_counts")["launches"] == 1
        row["group_counts_%d_ms" % members] = ms
        row["group_counts_%d_min_ms" % members] = mn
        row["ratio_%d" % members] = ms / vms
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
    out = {"rows": n, "int64": {}, "strings": {}}
    gen = torch.Generator(device="cuda").manual_seed(0x7E570017)
    values = value_columns(T, torch, max(n, args.string_rows // 64 * 64), gen)

    def sized(cols, rows):
        return [c.sliced(0, rows) for c in cols]

    def report(what, name, rows, row):
        print("%d rows, %s, %-14s value_counts %.2f ms | group_counts, 1 value column %.2f ms (x %.2f) | 8 value columns "
              "%.2f ms (x %.2f)" % (rows, what, name, row["value_counts_ms"], row["group_counts_1_ms"], row["ratio_1"],
                                    row["group_counts_8_ms"], row["ratio_8"]), flush=True)

    for k in (1, 16, 1000, 10_000, 60_000) if n else ():
        for zipf in (False, True):
            if k == 1 and zipf:
                continue
            name = "%d_%s" % (k, "zipf" if zipf else "uniform")
            vals = ids_of(torch, n, k, zipf, gen) * 7919 - 1000  # (spread keys: the keys are not the ids themselves)
            torch.cuda.synchronize()  # (the library runs on a stream of its own: the column must be finished)
            row = measure(T, spec, T.Column.int64(vals, None, length=n), sized(values, n), n, k, args.steps)
            out["int64"][name] = row
            report("Int64", name, n, row)
            del vals
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
            row = measure(T, spec, col, sized(values, m), m, k, args.steps)
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
