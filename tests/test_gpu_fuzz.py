"""-m gpu: three fixed sets of seeds of the differential tester (tests/fuzz_plans.py): random plans x tables x batchings
through the C ABI against the oracle and the exact references.  The first set runs with the default table sizes (up to
2.6 M rows; the JOINT_BINS / TEMPORAL / HISTOGRAM checks are drawn up to 400 000 rows), the second with at most 400 000
rows, so that every case of it can carry them; tests/test_fuzz_cases.py holds the two sets together to a census of what
they must cover.  The third set, sized like the second, holds only cases that carry a TIME_GAP check (drawn for cases
that are simply finalized): chosen so that the three sets together meet the TIME_GAP census of tests/test_fuzz_cases.py
-- every batching, state sequence, sort route, column role and neighbouring check, grouped and ungrouped.
tools/fuzz_device.py runs any other range of seeds."""
import pytest

from fuzz_plans import run_seed

pytestmark = pytest.mark.gpu

SECOND_MAX_ROWS = 400_001
SECOND_SEEDS = [48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 68, 69, 70, 71, 72,
                73, 74, 75, 76, 77, 78, 79, 80, 81, 86, 89, 96, 100, 103, 104, 121, 126, 152, 167, 168, 206, 219, 266, 303]


THIRD_SEEDS = [95, 110, 122, 155, 157, 170, 183, 185, 193, 211, 220, 241, 244, 254, 256, 261, 271, 288, 304, 309, 326, 347, 360,
               378, 382, 387, 393, 397, 415, 427, 444, 479, 491, 503, 519, 583, 593, 603, 607, 613, 619, 633, 648, 650, 682, 696]


@pytest.mark.parametrize("seed", range(48))
def test_seed(seed):
    run_seed(seed)


@pytest.mark.parametrize("seed", SECOND_SEEDS)
def test_seed_up_to_400_000_rows(seed):
    run_seed(seed, max_rows=SECOND_MAX_ROWS)


@pytest.mark.parametrize("seed", THIRD_SEEDS)
def test_seed_with_time_gap(seed):
    run_seed(seed, max_rows=SECOND_MAX_ROWS)
