"""-m gpu: the committed seeds of tests/regex_cases.py through the C ABI -- every pattern kernel route against RE2.
A case is built from its seed, fed the way its batching says (one batch, ragged Arrow slices, 8192-row batches, DEVICE /
HOST / mixed buffers, two states united by serialize -> deserialize -> merge; coalesced by the library or launched as
they arrive), and (total, matches) of every spec must EQUAL the expectation computed from RE2 and len() over the Python
values.  tests/test_regex_cases.py shows without a device which routes these seeds take and that none is left out;
tools/fuzz_regex_device.py runs any other range of seeds."""
import pyarrow  # noqa: F401  (RE2 is the expectation: a missing pyarrow is an error here, not a skip)
import pytest

from regex_cases import LARGE_SEEDS, SEEDS, run_seed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", SEEDS)
def test_seed(seed):
    run_seed(seed)


@pytest.mark.parametrize("seed", LARGE_SEEDS)
def test_second_sweep(seed):
    """about 1.2 M rows of short values: more rows than the largest persistent grid covers in one sweep"""
    run_seed(seed)
