#!/usr/bin/env python3
"""Writes tests/golden/fuzz_case_digests.json: test_fuzz_cases.case_digest of Case(seed) for the seeds of
tests/test_gpu_fuzz.py's first set.  The committed file was written with tests/fuzz_plans.py as it stood BEFORE the
JOINT_BINS / TEMPORAL / HISTOGRAM dimensions were added (the digest leaves the new kinds' expectations out, so the file
pins that every older draw stayed what it was); run it again only when a change to the older cases is intended.

    python tests/golden/make_fuzz_case_digests.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

from fuzz_plans import Case  # noqa: E402
from test_fuzz_cases import FIRST_SEEDS, case_digest  # noqa: E402

if __name__ == "__main__":
    out = {str(seed): case_digest(Case(seed)) for seed in FIRST_SEEDS}
    with open(os.path.join(HERE, "fuzz_case_digests.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
