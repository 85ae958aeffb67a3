#!/usr/bin/env python3
"""TGX_CHECK_KEY_PROBE beside TGX_CHECK_VALUE_RULE's BETWEEN on the same child column, in one process and interleaved
step by step: an Int64 child column (one validity bitmap, 5 % NULLs) probed against a dense parent (keys 0 .. K-1: the
bitmap route) and a sparse one (keys 1009 * i: the hash route) of --parents keys each, with 0 %, 1 % and 50 % of the
non-NULL rows holding one of 300 keys that are not in the parent.  VALUE_RULE reads the same bytes through the same
walker and keeps no table: it is the yardstick.  The build of the set (tgx_key_probe_set_parent: reduce, clear, insert,
with its two waits) is timed by the wall clock around the call.  Columns on DEVICE, one batch.  Kernel times are
HIP-event times on the state's stream (tgx_profile_get), the median of --steps steps after one warm-up step; the
roofline share prices the kind's own bytes -- 8 B and one validity bit a row -- at 8 TB/s.  There is no gate: the
figures go into DESIGN.md.  The COUNTED mode (tgx_plan_set_key_probe_counted) runs beside the plain one on the same set
and the same column, its plan interleaved with the other two: the count array (route 3) beside the bitmap (route 1), the
table of {key, count} slots (route 4) beside the table of keys (route 2); every record's count is 1, so pairs must equal
the matched rows.
    python tools/bench_key_probe.py [--rows 100000000] [--parents 1000000,100000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12
STRIDE = 1009  # of the sparse parent's keys: a range of 1009 bits a key is no bitmap
N_MISSING = 300


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--parents", default="1000000,100000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import term_amd as T
    from term_amd._lib import spec

    T.init(flags=T.OPT_NO_COALESCE)
    n = args.rows // 64 * 64
    gen = torch.Generator(device="cuda").manual_seed(0x7E570019)
    out = {"rows": n, "cases": {}}
    own_bytes = n * 8 + n // 8

    bits = (torch.rand(n + 64, device="cuda", generator=gen) >= 0.05).reshape(-1, 8).to(torch.uint8)
    packed = (bits << torch.arange(8, device="cuda", dtype=torch.uint8)[None, :]).sum(dim=1).to(torch.uint8)
    non_null = int(bits.reshape(-1)[:n].sum())
    del bits

    for k in [int(p) for p in args.parents.split(",")]:
        ids = torch.arange(k, device="cuda", dtype=torch.int64)
        for sparse in (False, True):
            records = torch.ones((k, 2), device="cuda", dtype=torch.int64)
            records[:, 0] = ids * (STRIDE if sparse else 1)
            torch.cuda.synchronize()
            for share in (0.0, 0.01, 0.5):
                name = "%s_%d_missing_%g" % ("sparse" if sparse else "dense", k, share)
                keys = (torch.rand(n, device="cuda", generator=gen) * k).to(torch.int64).clamp_(0, k - 1)
                if sparse:
                    keys *= STRIDE
                if share:
                    miss = torch.rand(n, device="cuda", generator=gen) < share
                    keys = torch.where(miss, -2 - (keys % N_MISSING), keys)
                    del miss
                torch.cuda.synchronize()  # (the library runs on a stream of its own: the column must be finished)
                col = T.Column.int64(keys, packed, length=n)
                pplan = T.Plan([spec(T.KEY_PROBE, 0)])
                pplan.set_key_probe(0, 10000)
                rplan = T.Plan([spec(T.VALUE_RULE, 0)])
                rplan.set_value_rule(0, T.RULE_BETWEEN, lo_i=0, hi_i=k * STRIDE)
                cplan = T.Plan([spec(T.KEY_PROBE, 0)])
                cplan.set_key_probe_counted(0, 10000)
                pst, rst, cst = T.State(pplan), T.State(rplan), T.State(cplan)
                pst.profile_enable(True)
                rst.profile_enable(True)
                cst.profile_enable(True)
                builds = []
                for _ in range(3):  # (a state that has seen no batch takes a set again)
                    t0 = time.perf_counter()
                    pst.key_probe_set_parent(0, records.data_ptr(), k)
                    builds.append((time.perf_counter() - t0) * 1e3)
                cbuilds = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    cst.key_probe_set_parent(0, records.data_ptr(), k)
                    cbuilds.append((time.perf_counter() - t0) * 1e3)
                probe_ms, rule_ms, counted_ms = [], [], []
                for it in range(args.steps + 1):
                    for st, kernel, times in ((pst, "key_probe", probe_ms), (rst, "value_rule", rule_ms),
                                              (cst, "key_probe", counted_ms)):
                        st.reset()
                        st.profile_reset()
                        st.update([col])
                        st.finalize()
                        if it:  # (step 0 warms the shape up)
                            times.append(st.profile_get(kernel)["total_ms"])
                s, missing = pst.key_probe(0)
                assert s["seen"] == n and s["non_null"] == non_null and s["overflow_rows"] == 0, s
                assert s["parent_keys"] == k and s["route"] == (2 if sparse else 1), s
                assert s["missing_keys"] == (N_MISSING if share else 0) and s["matched"] + s["missing_rows"] == non_null, s
                assert abs(s["missing_rows"] - share * non_null) <= 0.01 * non_null + 1000, s
                cs, cmissing = cst.key_probe(0)
                cp = cst.key_probe_pairs(0)
                assert cs["route"] == s["route"] + 2 and cmissing == missing, cs
                assert {f: v for f, v in cs.items() if f != "route"} == {f: v for f, v in s.items() if f != "route"}, cs
                assert cp["pairs"] == s["matched"] and cp["parent_rows"] == k and cp["max_count"] == 1, cp
                assert cp["join_rows"] == n, cp
                pm, rm, cm = statistics.median(probe_ms), statistics.median(rule_ms), statistics.median(counted_ms)
                slots = 1 << max(1, (2 * k - 1).bit_length())
                row = {"counted_ms": cm, "counted_min_ms": min(counted_ms), "counted_max_ms": max(counted_ms),
                       "key_probe_max_ms": max(probe_ms), "counted_ratio": cm / pm,
                       "counted_build_ms": statistics.median(cbuilds), "counted_set_bytes": 16 * slots if sparse else 8 * k,
                       "key_probe_ms": pm, "key_probe_min_ms": min(probe_ms), "value_rule_ms": rm,
                       "value_rule_min_ms": min(rule_ms), "ratio": pm / rm,
                       "roofline": own_bytes / (pm * 1e-3) / HBM_BYTES_PER_S, "build_ms": statistics.median(builds),
                       "set_bytes": (k + 7) // 8 if not sparse else 8 * (1 << max(1, (2 * k - 1).bit_length())),
                       "missing_rows": s["missing_rows"]}
                out["cases"][name] = row
                print("%d rows, %-34s key_probe %.2f ms | value_rule BETWEEN %.2f ms (x %.2f) | %.0f %% of 8 TB/s | "
                      "set of %.1f MB built in %.2f ms" % (n, name, pm, rm, row["ratio"], 100 * row["roofline"],
                                                           row["set_bytes"] / 1e6, row["build_ms"]), flush=True)
                print("%d rows, %-34s counted   %.2f ms (%.2f .. %.2f) | plain %.2f ms (%.2f .. %.2f) (x %.2f) | "
                      "set of %.1f MB built in %.2f ms" % (n, name, cm, min(counted_ms), max(counted_ms), pm, min(probe_ms),
                                                           max(probe_ms), row["counted_ratio"],
                                                           row["counted_set_bytes"] / 1e6, row["counted_build_ms"]), flush=True)
                del pst, rst, cst, col, keys
            del records
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
