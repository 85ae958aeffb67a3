"""-m gpu: five fixed sets of seeds of the differential tester (tests/fuzz_plans.py): random plans x tables x batchings
through the C ABI against the oracle and the exact references.  The first set runs with the default table sizes (up to
2.6 M rows; the JOINT_BINS / TEMPORAL / HISTOGRAM checks are drawn up to 400 000 rows), the second with at most 400 000
rows, so that every case of it can carry them; tests/test_fuzz_cases.py holds the two sets together to a census of what
they must cover.  The third set, sized like the second, holds only cases that carry a TIME_GAP check (drawn for cases
that are simply finalized): chosen so that the three sets together meet the TIME_GAP census of tests/test_fuzz_cases.py
-- every batching, state sequence, sort route, column role and neighbouring check, grouped and ungrouped.  The fourth
set, sized like the second, holds only cases that carry VALUE_RULE or one of the four counting kinds (VALUE_COUNTS,
PAIR_COUNTS, GROUP_COUNTS, GROUP_SUMS; drawn for every way a state ends): chosen so that the four sets together meet the
census of those kinds in tests/test_fuzz_cases.py -- every key type and layout, bound, state sequence and neighbouring
check.  The fifth set, sized like the second, holds only cases that carry KEY_PROBE specs (plain, counted and strings for
every way a state ends, rows for states that are simply finalized): chosen so that it fills, on its own and twice where
the seeds allow, the KEY_PROBE census of tests/test_fuzz_cases.py -- every record source, route and route threshold, bound,
string layout, neighbouring check and state sequence, the refusal of a deserialized state included -- which the five sets
together must meet.  tools/fuzz_device.py runs any other range of seeds."""
import pytest

from fuzz_plans import run_seed

pytestmark = pytest.mark.gpu

SECOND_MAX_ROWS = 400_001
SECOND_SEEDS = [48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 68, 69, 70, 71, 72,
                73, 74, 75, 76, 77, 78, 79, 80, 81, 86, 89, 96, 100, 103, 104, 121, 126, 152, 167, 168, 206, 219, 266, 303]


THIRD_SEEDS = [95, 110, 122, 155, 157, 170, 183, 185, 193, 211, 220, 241, 244, 254, 256, 261, 271, 288, 304, 309, 326, 347, 360,
               378, 382, 387, 393, 397, 415, 427, 444, 479, 491, 503, 519, 583, 593, 603, 607, 613, 619, 633, 648, 650, 682, 696]


FOURTH_SEEDS = [700, 702, 703, 704, 705, 706, 707, 709, 713, 714, 715, 716, 717, 720, 721, 722, 724, 726, 727, 730, 732, 735, 737,
                738, 739, 742, 743, 776, 815, 872, 875, 895, 900, 901, 980, 991, 1024, 1036, 1062, 1102, 1104, 1113, 1121, 1344,
                1490, 1558, 1779, 2243]


FIFTH_SEEDS = [2380, 2385, 2409, 2436, 2588, 2973, 3015, 3302, 3399, 3513, 3521, 3541, 3552, 3561, 3585, 3619, 3620, 3766, 3770,
               3891, 4007, 4107, 4118, 4160, 4228, 4275, 6499, 7155, 8234, 11610, 14163, 18776, 19918, 29827, 58042]


@pytest.mark.parametrize("seed", range(48))
def test_seed(seed):
    run_seed(seed)


@pytest.mark.parametrize("seed", SECOND_SEEDS)
def test_seed_up_to_400_000_rows(seed):
    run_seed(seed, max_rows=SECOND_MAX_ROWS)


@pytest.mark.parametrize("seed", THIRD_SEEDS)
def test_seed_with_time_gap(seed):
    run_seed(seed, max_rows=SECOND_MAX_ROWS)


@pytest.mark.parametrize("seed", FOURTH_SEEDS)
def test_seed_with_rules_and_counts(seed):
    run_seed(seed, max_rows=SECOND_MAX_ROWS)


@pytest.mark.parametrize("seed", FIFTH_SEEDS)
def test_seed_with_key_probes(seed):
    run_seed(seed, max_rows=SECOND_MAX_ROWS)
