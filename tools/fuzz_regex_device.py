#!/usr/bin/env python3
"""The pattern kernels on the GPU against RE2 (pyarrow.compute), seed by seed: the cases of tests/regex_cases.py -- one
string column (Utf8, LargeUtf8, Utf8View, dictionary) with value lengths that force each way a wave step is fed, one to
six patterns from tools/fuzz_regex_diff.py's grammar and templates with TRIM / NULL-is-valid / case flags, LENGTH checks,
fed as one batch, ragged Arrow slices, 8192-row batches, from DEVICE / HOST buffers or as two merged states -- over any
range of seeds.  Counts must be equal; a spec that disagrees is printed with its route (table class, single walk or
product automaton, layout, feeds), and its seed can go into tests/regex_cases.py's SEEDS.  Seeds whose draw RE2 or the
engine refuses are counted and passed over: nothing to compare.

    python tools/fuzz_regex_device.py [--first S] [--count K] [--seconds T] [--seed S]

A run covers the seeds --first .. --first + --count - 1 and says which it ran.  --seed is the earlier name of --first;
--seconds (default 0: no limit) stops starting new cases after that long, and the last line then says that the clock,
not the count, ended the run; --rows is accepted and ignored (a case draws its own row count)."""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0, help="stop starting new cases after this long (0: run them all)")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rows", type=int, default=6000)
    ap.add_argument("--first", type=int, default=None)
    ap.add_argument("--count", type=int, default=200)
    args = ap.parse_args()
    import pyarrow  # noqa: F401

    import regex_cases as R
    import term_amd as T

    T.init()
    first = args.seed if args.first is None else args.first
    t0 = time.time()
    cases = specs = bad = refused = 0
    routes = set()
    last, cut_short = None, False
    for seed in range(first, first + args.count):
        if args.seconds > 0 and time.time() - t0 > args.seconds:
            cut_short = True
            break
        last = seed
        try:
            case = R.Case(seed)
        except RuntimeError as e:  # (no pattern of the stratum's table class in the generator's draws)
            print("seed %d: %s" % (seed, e))
            refused += 1
            continue
        if case.refused():
            refused += 1
            continue
        got = case.run()
        cases += 1
        specs += len(got)
        for r in case.routes():
            if r and r["kind"] == "regex":
                routes.update((r["table"], r["layout"], r["group"], f) for f in r["feeds"])
        for line in R.disagreements(case, got):
            bad += 1
            print("DISAGREE", line, flush=True)
            for ref in case.reference_disagreements()[:5]:  # (a host walk that agrees with RE2 puts the fault in the kernel)
                print("         references:", ref, flush=True)
    print("seeds %d .. %s%s: %d cases, %d specs compared over %d routes, %d disagreements, %d seeds refused, %.0f s"
          % (first, last, " (ended by --seconds, %d asked for)" % args.count if cut_short else "", cases, specs, len(routes),
             bad, refused, time.time() - t0))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
