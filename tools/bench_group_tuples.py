#!/usr/bin/env python3
"""GROUP BY several columns on the device -- TGX_CHECK_GROUP_COUNTS / TGX_CHECK_GROUP_SUMS specs with a column list -- beside
what bounds them, in one process and interleaved step by step:

  tuple      the tuple walk: (Int64, Int64) with 16, 1 000 and 60 000 groups, (Utf8 of 12 bytes, Int64) and
             (Dictionary<Int32, Utf8>, Int64) with 1 000 groups
  single     single-column GROUP_COUNTS / GROUP_SUMS over an Int64 key AND over a Utf8 key of 12 bytes, each with the same
             number of groups as the tuple, beside every shape: what one key column of either kind costs
  distinct   the tuple DISTINCT of the same columns: the same reads and the same fingerprint without the counting -- the floor

GROUP_COUNTS counts the validity of one value column; GROUP_SUMS sums an Int64 and a Float64 value column.  Columns on
DEVICE, one batch of --rows rows, 1 % NULLs in every column's bitmap.  Kernel times are HIP-event times on the state's
stream (tgx_profile_get), the median of --steps steps after one warm-up step.  There is no gate: the figures go into
DESIGN.md.
    python tools/bench_group_tuples.py [--rows 100000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WIDTH = 12  # bytes of a string key


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import term_amd as T
    from term_amd._lib import spec

    T.init(flags=T.OPT_NO_COALESCE)
    n = args.rows // 64 * 64
    gen = torch.Generator(device="cuda").manual_seed(0x7E570023)
    out = {"rows": n, "cases": {}}
    shifts = (4 * torch.arange(WIDTH, device="cuda", dtype=torch.int64))[None, :]

    def bitmap():
        bits = (torch.rand(n + 64, device="cuda", generator=gen) >= 0.01).reshape(-1, 8).to(torch.uint8)
        return (bits << torch.arange(8, device="cuda", dtype=torch.uint8)[None, :]).sum(dim=1).to(torch.uint8)

    def render(ids):
        """ids -> (int32 offsets, bytes): 12 letters a .. p, a nibble each"""
        data = torch.empty((ids.numel(), WIDTH), device="cuda", dtype=torch.uint8)
        step = 1 << 24
        for lo in range(0, ids.numel(), step):
            data[lo:lo + step] = (((ids[lo:lo + step, None] >> shifts) & 15) + 97).to(torch.uint8)
        offsets = torch.arange(ids.numel() + 1, device="cuda", dtype=torch.int64).mul_(WIDTH).to(torch.int32)
        return offsets, torch.cat([data.reshape(-1), torch.zeros(64, device="cuda", dtype=torch.uint8)])

    validity = [bitmap() for _ in range(3)]
    ivalues = (torch.rand(n, device="cuda", generator=gen) * 2000).to(torch.int64) - 1000
    fvalues = ivalues.to(torch.float64) * 0.5
    value_cols = {"i64": T.Column.int64(ivalues, validity[2], length=n), "f64": T.Column.float64(fvalues, validity[2], length=n)}

    def median_ms(plans, cols):
        """{name: median kernel ms}; plans: {name: (plan, kernel name)}, run interleaved step by step"""
        states = {name: T.State(plan) for name, (plan, _) in plans.items()}
        times = {name: [] for name in plans}
        for st in states.values():
            st.profile_enable(True)
        for it in range(args.steps + 1):
            for name, st in states.items():
                st.reset()
                st.profile_reset()
                st.update(cols)
                st.finalize()
                if it:  # (step 0 warms the shape up)
                    times[name].append(st.profile_get(plans[name][1])["total_ms"])
        return {name: statistics.median(t) for name, t in times.items()}, states

    def counts_plan(value, group=None, columns=None):
        plan = T.Plan([spec(T.GROUP_COUNTS, value, column2=group) if columns is None else spec(T.GROUP_COUNTS, value, columns=columns)])
        plan.set_group_counts(0, 65536, 64)
        return plan

    def sums_plan(value, group=None, columns=None):
        plan = T.Plan([spec(T.GROUP_SUMS, value, column2=group) if columns is None else spec(T.GROUP_SUMS, value, columns=columns)])
        plan.set_group_sums(0, 65536, 64)
        return plan

    shapes = [("i64_i64", 16), ("i64_i64", 1000), ("i64_i64", 60000), ("utf8_i64", 1000), ("dict_i64", 1000)]
    for shape, groups in shapes:
        # the tuple's two components: `first` takes groups // second_card values, `second` second_card values
        second_card = 4 if groups == 16 else 10 if groups == 1000 else 240
        first_card = groups // second_card
        ids = (torch.rand(n, device="cuda", generator=gen) * groups).to(torch.int64).clamp_(0, groups - 1)
        first, second = ids // second_card, ids % second_card * 1_000_003
        keep = [ids, first, second]
        b = T.Column.int64(second, validity[1], length=n)
        single_i64 = T.Column.int64(ids * 7919 - 5, validity[0], length=n)
        offs, data = render(ids)  # the single string key: one of `groups` words
        single_utf8 = T.Column(T.UTF8, n, offsets=offs, data=data, validity=validity[0], mem=T.MEM_DEVICE)
        keep += [offs, data]
        if shape == "i64_i64":
            a = T.Column.int64(first * 7919 - 5, validity[0], length=n)
        else:
            if shape == "utf8_i64":
                foffs, fdata = render(first)
                a = T.Column(T.UTF8, n, offsets=foffs, data=fdata, validity=validity[0], mem=T.MEM_DEVICE)
                keep += [foffs, fdata]
            else:
                eoffs, edata = render(torch.arange(first_card, device="cuda", dtype=torch.int64))
                idx = first.to(torch.int32)
                a = T.Column(T.DICT32_UTF8, n, values=idx, validity=validity[0], mem=T.MEM_DEVICE,
                             dictionary=T.Column(T.UTF8, first_card, offsets=eoffs, data=edata, mem=T.MEM_DEVICE))
                keep += [eoffs, edata, idx]
        torch.cuda.synchronize()  # (the library runs on a stream of its own: the columns must be finished)
        name = "%s_%d" % (shape, groups)
        row = {}
        # columns: 0, 1 the tuple, 2 the single Int64 key, 3 the single Utf8 key, 4 the value column
        distinct = T.Plan([spec(T.DISTINCT, 0, columns=[0, 1])])
        for kind, value in (("counts", "i64"), ("sums_i64", "i64"), ("sums_f64", "f64")):
            cols = [a, b, single_i64, single_utf8, value_cols[value]]
            make = counts_plan if kind == "counts" else sums_plan
            kernel = "group_counts" if kind == "counts" else "group_sums"
            ms, states = median_ms({"tuple": (make(4, columns=[0, 1]), kernel + "_tuples"),
                                    "single_i64": (make(4, group=2), kernel), "single_utf8": (make(4, group=3), kernel),
                                    "distinct": (distinct, "distinct")}, cols)
            read = states["tuple"].group_counts(0) if kind == "counts" else states["tuple"].group_sums(0)
            summary = read[0]
            assert summary["seen"] == n and summary["groups"] >= groups, summary  # (+ the tuples with a NULL component)
            overflow = summary["overflow_rows"] if kind == "counts" else summary["overflow"][0]
            assert overflow == 0, summary
            row[kind] = {"tuple_ms": ms["tuple"], "single_i64_ms": ms["single_i64"], "single_utf8_ms": ms["single_utf8"],
                         "distinct_ms": ms["distinct"], "tuple_groups": summary["groups"],
                         "over_single_i64": ms["tuple"] / ms["single_i64"], "over_single_utf8": ms["tuple"] / ms["single_utf8"],
                         "over_distinct": ms["tuple"] / ms["distinct"]}
            print("%d rows, %-16s %-8s tuple %.2f ms | single Int64 key %.2f ms (x %.2f) | single Utf8 key %.2f ms (x %.2f) | "
                  "tuple DISTINCT %.2f ms (x %.2f) | %d groups held"
                  % (n, name, kind, ms["tuple"], ms["single_i64"], row[kind]["over_single_i64"], ms["single_utf8"],
                     row[kind]["over_single_utf8"], ms["distinct"], row[kind]["over_distinct"], summary["groups"]), flush=True)
            del states
        out["cases"][name] = row
        del a, b, single_i64, single_utf8, keep
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
