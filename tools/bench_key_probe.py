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
    python tools/bench_key_probe.py [--rows 100000000] [--parents 1000000,100000000] [--steps 5] [--json out.json]
    python tools/bench_key_probe.py --tuples ..   (composite keys: tuples_main)"""
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
    ap.add_argument("--strings", action="store_true", help="the string-key probe beside VALUE_COUNTS (strings_main)")
    ap.add_argument("--tuples", action="store_true", help="the tuple-key probe beside tuple DISTINCT (tuples_main)")
    args = ap.parse_args()
    if args.strings:
        return strings_main(args)
    if args.tuples:
        return tuples_main(args)
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


STRING_EXPECTATIONS = """expectations, written before the run:
 (1) a probe step costs what VALUE_COUNTS costs on the same column -- the same row-per-lane walk and the same fingerprint
     -- plus the lookup.  (The yardstick column has the child's shape and 5000 distinct values: on the child itself, a
     million distinct values, VALUE_COUNTS's 32 768-slot table overflows and every row walks a probe sequence to its end.)
 (2) 1 M keys, a 32 MiB table: out of an XCD's L2, inside the Infinity Cache; 100 M keys, a 4 GiB table: one 64-byte line
     from HBM a row, as on routes 2 and 4, so the step costs what route 4's costs (16-byte slots) plus the string walk.
 (3) the missing rate moves the time little: 300 missing keys combine in the wave and the LDS table; a miss probes on
     to a free slot (about 2.5 slots at load 0.5 against 1.5 for a hit).
 (4) the dictionary child costs its 4 bytes a row: the 10 000 lookups are nothing.
 (5) the COUNTED strings probe (route 6) reads 8 more bytes per matched row, from a count array beside the slot table:
     close to the plain probe where every row misses, somewhat above it where every row hits; its build adds an atomicAdd
     a record to route 5's claims.  The rows strings gather reads what the probe reads and writes 32 bytes a non-NULL
     row: it should cost about the plain probe against the small set plus 3 GB of stores.
"""


def tuples_main(args):
    """--tuples: a child of (Int64, Int64) and of (Int64, Utf8 of 12 bytes) tuples, 0.01 % NULLs a component's bitmap (every
    NULL-bearing tuple of such a child is distinct: a higher rate only measures the overflow counter), 1 % of
    the rows strangers (300 distinct), probed against sets of --parents tuple records (routes 5 and 6; the records are
    what a rows tuples spec gathers from the parent's columns): the plain probe, the counted probe and the gather of the
    child, beside the tuple DISTINCT of the same two columns and, for the (Int64, Utf8) shape, the counted STRINGS
    probe of its string column against a set of the same size -- all plans interleaved step by step in one process,
    one DEVICE batch, HIP-event kernel times (tgx_profile_get), medians of --steps steps after a warm-up step.  The
    roofline prices the all-numeric probe's own bytes -- 16 B and two validity bits a row, plus one 16-byte slot load a
    looked-up row -- at 8 TB/s.  There is no gate: the figures go into DESIGN.md."""
    import torch
    import term_amd as T
    from term_amd._lib import spec

    T.init(flags=T.OPT_NO_COALESCE)
    n = args.rows // 64 * 64
    width = 12
    gen = torch.Generator(device="cuda").manual_seed(0x7E570021)
    out = {"rows": n, "cases": {}}
    key = bytes(range(16))
    far = 1 << 44
    shifts = (4 * torch.arange(width, device="cuda", dtype=torch.int64))[None, :]

    def render(ids):
        data = torch.empty((ids.numel(), width), device="cuda", dtype=torch.uint8)
        step = 1 << 24
        for lo in range(0, ids.numel(), step):
            data[lo:lo + step] = (((ids[lo:lo + step, None] >> shifts) & 15) + 97).to(torch.uint8)
        offsets = torch.arange(ids.numel() + 1, device="cuda", dtype=torch.int64).mul_(width).to(torch.int32)
        return offsets, torch.cat([data.reshape(-1), torch.zeros(64, device="cuda", dtype=torch.uint8)])

    def bitmap():
        bits = (torch.rand(n + 64, device="cuda", generator=gen) >= 0.0001).reshape(-1, 8).to(torch.uint8)
        return (bits << torch.arange(8, device="cuda", dtype=torch.uint8)[None, :]).sum(dim=1).to(torch.uint8), bits.reshape(-1)[:n]

    va, ba = bitmap()
    vb, bb = bitmap()
    all_valid = int((ba & bb).sum())
    b_valid = int(bb.sum())
    del ba, bb

    def columns(ids, strings, validity=(None, None)):
        """the tuple (id, 3 * id + 1), or (id, the 12 letters of id)"""
        a = T.Column.int64(ids, validity[0], length=ids.numel())
        if not strings:
            second = ids * 3 + 1
            return [a, T.Column.int64(second, validity[1], length=ids.numel())], (ids, second)
        offs, data = render(ids)
        return [a, T.Column(T.UTF8, ids.numel(), offsets=offs, data=data, validity=validity[1], mem=T.MEM_DEVICE)], (ids, offs, data)

    def plan_of(mode, cols=(0, 1)):
        plan = T.Plan([spec(T.KEY_PROBE, 0, columns=list(cols))])
        plan.set_fingerprint_key(key)
        if mode == "rows":
            plan.set_key_probe_rows_tuples(0)
        else:
            getattr(plan, "set_key_probe_tuples" if mode == "plain" else "set_key_probe_tuples_counted")(0, 65536)
        return plan

    for strings in (False, True):
        shape = "int64_utf8" if strings else "int64_int64"
        for k in [int(p) for p in args.parents.split(",")]:
            name = "%s_%d" % (shape, k)
            pcols, pkeep = columns(torch.arange(k, device="cuda", dtype=torch.int64), strings)
            torch.cuda.synchronize()
            parent = T.State(plan_of("rows"))
            parent.update(pcols)
            ptr, n_records = parent.key_probe_rows(0)
            assert n_records == k, n_records
            ids = (torch.rand(n, device="cuda", generator=gen) * k).to(torch.int64).clamp_(0, k - 1)
            miss = torch.rand(n, device="cuda", generator=gen) < 0.01
            ids = torch.where(miss, far + (ids % N_MISSING), ids)
            del miss
            cols, keep = columns(ids, strings, (va, vb))
            torch.cuda.synchronize()
            states = {"plain": T.State(plan_of("plain")), "counted": T.State(plan_of("counted")), "rows": T.State(plan_of("rows"))}
            dplan = T.Plan([spec(T.DISTINCT, 0, columns=[0, 1])])
            dplan.set_fingerprint_key(key)
            states["distinct"] = T.State(dplan)
            builds = {}
            for mode in ("plain", "counted"):
                times = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    states[mode].key_probe_set_parent(0, ptr, n_records)
                    times.append((time.perf_counter() - t0) * 1e3)
                builds[mode] = statistics.median(times)
            if strings:  # the counted strings probe of the string column, against the parent's strings gathered
                gplan = T.Plan([spec(T.KEY_PROBE, 1)])
                gplan.set_fingerprint_key(key)
                gplan.set_key_probe_rows_strings(0)
                gathered = T.State(gplan)
                gathered.update(pcols)
                sptr, sn = gathered.key_probe_rows(0)
                splan = T.Plan([spec(T.KEY_PROBE, 1)])
                splan.set_fingerprint_key(key)
                splan.set_key_probe_strings_counted(0, 10000, 256)
                states["strings_counted"] = T.State(splan)
                states["strings_counted"].key_probe_set_parent(0, sptr, sn)
            kernels = {"plain": "key_probe", "counted": "key_probe", "rows": "key_probe_rows", "distinct": "distinct",
                       "strings_counted": "key_probe"}
            ms = {m: [] for m in states}
            for st in states.values():
                st.profile_enable(True)
            for it in range(args.steps + 1):
                for m, st in states.items():
                    st.reset()
                    st.profile_reset()
                    st.update(cols)
                    st.finalize()
                    if it:  # (step 0 warms the shape up)
                        ms[m].append(st.profile_get(kernels[m])["total_ms"])
            s, entries = states["plain"].key_probe_tuples(0)
            cs, _ = states["counted"].key_probe_tuples(0)
            cp = states["counted"].key_probe_pairs(0)
            assert s["seen"] == n and s["non_null"] == all_valid and s["overflow_rows"] == 0 and s["route"] == 5, s
            assert s["parent_keys"] == k and s["missing_keys"] == N_MISSING and s["null_overflow_rows"] == 0, s
            assert abs(s["missing_rows"] - 0.01 * all_valid) <= 0.002 * all_valid + 1000, s
            assert cs["route"] == 6 and cp["pairs"] == s["matched"] == cs["matched"] and cp["join_rows"] == n, (cs, cp)
            assert states["rows"].key_probe_rows(0)[1] == all_valid
            if strings:
                ss, _ = states["strings_counted"].key_probe_strings(0)
                assert ss["non_null"] == b_valid and ss["parent_keys"] == k, ss
            med = {m: statistics.median(v) for m, v in ms.items()}
            slots = 1 << max(1, (2 * k - 1).bit_length())
            own = n * 16 + 2 * (n // 8) + all_valid * 16  # (the all-numeric shape: its columns, bitmaps and slot loads)
            row = {"%s_ms" % m: med[m] for m in med}
            row.update({"%s_min_ms" % m: min(ms[m]) for m in ms})
            row.update({"%s_max_ms" % m: max(ms[m]) for m in ms})
            row.update(probe_over_distinct=med["plain"] / med["distinct"], counted_ratio=med["counted"] / med["plain"],
                       gather_ratio=med["rows"] / med["plain"], build_ms=builds["plain"], counted_build_ms=builds["counted"],
                       set_bytes=16 * slots, counted_set_bytes=24 * slots, matched=s["matched"], missing_rows=s["missing_rows"],
                       null_rows=s["null_rows"])
            if not strings:
                row["roofline"] = own / (med["plain"] * 1e-3) / HBM_BYTES_PER_S
            out["cases"][name] = row
            print("%d rows, %-24s plain %.2f ms (%.2f .. %.2f) | counted %.2f ms (x %.2f) | gather %.2f ms (x %.2f) | "
                  "tuple DISTINCT %.2f ms (probe x %.2f of it)%s%s | sets of %.1f / %.1f MB built in %.2f / %.2f ms"
                  % (n, name, med["plain"], min(ms["plain"]), max(ms["plain"]), med["counted"], row["counted_ratio"],
                     med["rows"], row["gather_ratio"], med["distinct"], row["probe_over_distinct"],
                     " | %.0f %% of 8 TB/s" % (100 * row["roofline"]) if not strings else "",
                     " | counted strings probe of the Utf8 column %.2f ms" % med["strings_counted"] if strings else "",
                     row["set_bytes"] / 1e6, row["counted_set_bytes"] / 1e6, builds["plain"], builds["counted"]), flush=True)
            del states, parent, cols, keep, pcols, pkeep, ids
            torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def strings_main(args):
    """--strings: a Utf8 child of 12-byte values (5 % NULLs, 300 distinct missing keys at 0 %, 1 % and 50 % of the
    non-NULL rows) probed against parents of --parents string keys (route 5: tables of 16-byte slots, 32 MiB and 4 GiB),
    beside VALUE_COUNTS in the same process, the plans interleaved step by step -- on a column of the same shape (rows,
    value length, validity) with 5000 distinct values, which its table holds: the same walker and fingerprint, no set;
    then a dictionary child of 10 000 entries.  The set is built from the parent column's DISTINCT export under the child plan's
    fingerprint key; its build is timed by the wall clock around tgx_key_probe_set_parent.  The roofline prices the
    kind's own bytes -- 12 B of data, a 4-byte offset and one validity bit a row -- at 8 TB/s.
    Beside each plain probe, interleaved with it step by step on the same column: the COUNTED strings probe
    (tgx_plan_set_key_probe_strings_counted, route 6) against the same records with every count 1 -- so pairs must equal
    the matched rows -- with its build, and the rows strings gather (tgx_plan_set_key_probe_rows_strings) of the column;
    each is stated as a ratio to the plain probe of the same case.  A child that misses on every row joins the cases."""
    import torch
    import term_amd as T
    from term_amd._lib import spec

    T.init(flags=T.OPT_NO_COALESCE)
    print(STRING_EXPECTATIONS, flush=True)
    n = args.rows // 64 * 64
    width = 12
    gen = torch.Generator(device="cuda").manual_seed(0x7E570020)
    out = {"rows": n, "cases": {}}
    own_bytes = n * (width + 4) + n // 8
    far = 1 << 44  # ids of the missing keys: beyond every parent
    shifts = (4 * torch.arange(width, device="cuda", dtype=torch.int64))[None, :]

    def render(ids):
        """ids -> (int32 offsets, bytes): 12 letters a .. p, a nibble each"""
        data = torch.empty((ids.numel(), width), device="cuda", dtype=torch.uint8)
        step = 1 << 24
        for lo in range(0, ids.numel(), step):  # (in pieces: the nibbles as int64 are 96 bytes a row)
            data[lo:lo + step] = (((ids[lo:lo + step, None] >> shifts) & 15) + 97).to(torch.uint8)
        offsets = torch.arange(ids.numel() + 1, device="cuda", dtype=torch.int64).mul_(width).to(torch.int32)
        return offsets, torch.cat([data.reshape(-1), torch.zeros(64, device="cuda", dtype=torch.uint8)])

    bits = (torch.rand(n + 64, device="cuda", generator=gen) >= 0.05).reshape(-1, 8).to(torch.uint8)
    packed = (bits << torch.arange(8, device="cuda", dtype=torch.uint8)[None, :]).sum(dim=1).to(torch.uint8)
    non_null = int(bits.reshape(-1)[:n].sum())
    del bits
    key = bytes(range(16))
    yoffs, ydata = render((torch.rand(n, device="cuda", generator=gen) * 5000).to(torch.int64).clamp_(0, 4999))
    ycol = T.Column(T.UTF8, n, offsets=yoffs, data=ydata, validity=packed, mem=T.MEM_DEVICE)

    def probe_plan():
        plan = T.Plan([spec(T.KEY_PROBE, 0)])
        plan.set_fingerprint_key(key)
        plan.set_key_probe_strings(0, 10000, 256)
        return plan

    for k in [int(p) for p in args.parents.split(",")]:
        poffs, pdata = render(torch.arange(k, device="cuda", dtype=torch.int64))
        dplan = T.Plan([spec(T.DISTINCT, 0)])
        dplan.set_fingerprint_key(key)
        parent = T.State(dplan)
        torch.cuda.synchronize()
        parent.update([T.Column(T.UTF8, k, offsets=poffs, data=pdata, mem=T.MEM_DEVICE)])
        ptr, counts = parent.distinct_export(0, 1)
        assert counts[0] == k, counts

        class Exported:  # (the export as a tensor: a copy of the records with every count 1, for the counted set)
            __cuda_array_interface__ = {"shape": (k, 4), "typestr": "<i8", "data": (ptr, False), "version": 2}

        ones = torch.as_tensor(Exported(), device="cuda").clone()
        ones[:, 2] = 1
        torch.cuda.synchronize()
        slots = 1 << max(1, (2 * k - 1).bit_length())
        cases = [("missing_%g" % share, share, False) for share in (0.0, 0.01, 0.5, 1.0)] + [("dictionary_10000", 0.01, True)]
        for label, share, as_dict in cases:
            name = "strings_%d_%s" % (k, label)
            if as_dict:
                entry_ids = torch.arange(10000, device="cuda", dtype=torch.int64)
                entry_ids = torch.where(entry_ids % 100 == 0, far + entry_ids // 100, entry_ids % k)
                eoffs, edata = render(entry_ids)
                idx = (torch.rand(n, device="cuda", generator=gen) * 10000).to(torch.int32).clamp_(0, 9999)
                torch.cuda.synchronize()
                col = T.Column(T.DICT32_UTF8, n, values=idx, validity=packed, mem=T.MEM_DEVICE,
                               dictionary=T.Column(T.UTF8, 10000, offsets=eoffs, data=edata, mem=T.MEM_DEVICE))
                case_bytes = n * 4 + n // 8
            else:
                ids = (torch.rand(n, device="cuda", generator=gen) * k).to(torch.int64).clamp_(0, k - 1)
                if share:
                    miss = torch.rand(n, device="cuda", generator=gen) < share
                    ids = torch.where(miss, far + (ids % N_MISSING), ids)
                    del miss
                offs, data = render(ids)
                del ids
                torch.cuda.synchronize()
                col = T.Column(T.UTF8, n, offsets=offs, data=data, validity=packed, mem=T.MEM_DEVICE)
                case_bytes = own_bytes
            pplan = probe_plan()
            vplan = T.Plan([spec(T.VALUE_COUNTS, 0)])
            vplan.set_fingerprint_key(key)
            vplan.set_value_counts(0, 10000, 256)
            cplan = T.Plan([spec(T.KEY_PROBE, 0)])
            cplan.set_fingerprint_key(key)
            cplan.set_key_probe_strings_counted(0, 10000, 256)
            gplan = T.Plan([spec(T.KEY_PROBE, 0)])
            gplan.set_fingerprint_key(key)
            gplan.set_key_probe_rows_strings(0)
            pst, vst, cst, gst = T.State(pplan), T.State(vplan), T.State(cplan), T.State(gplan)
            for st in (pst, vst, cst, gst):
                st.profile_enable(True)
            builds = []
            for _ in range(3):  # (a state that has seen no batch takes a set again)
                t0 = time.perf_counter()
                pst.key_probe_set_parent(0, ptr, k)
                builds.append((time.perf_counter() - t0) * 1e3)
            cbuilds = []
            for _ in range(3):
                t0 = time.perf_counter()
                cst.key_probe_set_parent(0, ones.data_ptr(), k)
                cbuilds.append((time.perf_counter() - t0) * 1e3)
            probe_ms, counts_ms, counted_ms, gather_ms = [], [], [], []
            for it in range(args.steps + 1):
                for st, kernel, times, batch in ((pst, "key_probe", probe_ms, col), (vst, "value_counts", counts_ms, ycol),
                                                 (cst, "key_probe", counted_ms, col), (gst, "key_probe_rows", gather_ms, col)):
                    st.reset()
                    st.profile_reset()
                    st.update([batch])
                    st.finalize()
                    if it:  # (step 0 warms the shape up)
                        times.append(st.profile_get(kernel)["total_ms"])
            s, missing = pst.key_probe_strings(0)
            assert s["seen"] == n and s["non_null"] == non_null and s["overflow_rows"] == 0 and s["long_rows"] == 0, s
            assert s["parent_keys"] == k and s["route"] == 5 and s["matched"] + s["missing_rows"] == non_null, s
            assert s["missing_keys"] == (100 if as_dict else N_MISSING if share else 0), s
            assert abs(s["missing_rows"] - share * non_null) <= 0.01 * non_null + 1000, s
            cs, cmissing = cst.key_probe_strings(0)
            cp = cst.key_probe_pairs(0)
            assert cs["route"] == 6 and cmissing == missing, cs
            assert {f: v for f, v in cs.items() if f != "route"} == {f: v for f, v in s.items() if f != "route"}, cs
            assert cp["pairs"] == s["matched"] and cp["parent_rows"] == k and cp["max_count"] == 1 and cp["join_rows"] == n, cp
            _, gathered = gst.key_probe_rows(0)
            assert gst.finalize()[0].non_null == non_null, gathered
            assert gathered == (non_null if not as_dict else 10000), gathered
            pm, vm = statistics.median(probe_ms), statistics.median(counts_ms)
            cm, gm = statistics.median(counted_ms), statistics.median(gather_ms)
            counted_row = {"counted_ms": cm, "counted_min_ms": min(counted_ms), "counted_max_ms": max(counted_ms),
                           "counted_ratio": cm / pm, "counted_build_ms": statistics.median(cbuilds),
                           "counted_set_bytes": 24 * slots, "gather_ms": gm, "gather_min_ms": min(gather_ms),
                           "gather_max_ms": max(gather_ms), "gather_ratio": gm / pm, "gathered_records": gathered}
            row = {"key_probe_ms": pm, "key_probe_min_ms": min(probe_ms), "key_probe_max_ms": max(probe_ms),
                   "value_counts_ms": vm, "value_counts_min_ms": min(counts_ms), "value_counts_max_ms": max(counts_ms),
                   "ratio": pm / vm, "roofline": case_bytes / (pm * 1e-3) / HBM_BYTES_PER_S,
                   "build_ms": statistics.median(builds), "set_bytes": 16 * slots, "missing_rows": s["missing_rows"]}
            row.update(counted_row)
            out["cases"][name] = row
            print("%d rows, %-36s key_probe %.2f ms (%.2f .. %.2f) | value_counts %.2f ms (%.2f .. %.2f) (x %.2f) | "
                  "%.0f %% of 8 TB/s | set of %.1f MB built in %.2f ms"
                  % (n, name, pm, min(probe_ms), max(probe_ms), vm, min(counts_ms), max(counts_ms), row["ratio"],
                     100 * row["roofline"], row["set_bytes"] / 1e6, row["build_ms"]), flush=True)
            print("%d rows, %-36s counted   %.2f ms (%.2f .. %.2f) (x %.2f of the plain probe) | set of %.1f MB built in "
                  "%.2f ms" % (n, name, cm, min(counted_ms), max(counted_ms), row["counted_ratio"],
                               row["counted_set_bytes"] / 1e6, row["counted_build_ms"]), flush=True)
            print("%d rows, %-36s gather    %.2f ms (%.2f .. %.2f) (x %.2f of the plain probe) | %d records of 32 B"
                  % (n, name, gm, min(gather_ms), max(gather_ms), row["gather_ratio"], gathered), flush=True)
            del pst, vst, cst, gst, col
            torch.cuda.empty_cache()
        del parent, poffs, pdata, ones
        torch.cuda.empty_cache()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
