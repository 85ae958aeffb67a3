"""TGX_CHECK_KEY_PROBE on TUPLE keys without a device: the column list at plan creation, the three plan calls and their
exclusions with the six single-column ones, the ABI's structs and symbols, and what a state that has seen nothing
answers."""
import ctypes as C

import pytest

import term_amd as T
from _lib_spec import spec

TUPLES = ("set_key_probe_tuples", "set_key_probe_tuples_counted", "set_key_probe_rows_tuples")
SINGLE = ("set_key_probe", "set_key_probe_counted", "set_key_probe_rows", "set_key_probe_strings",
          "set_key_probe_strings_counted", "set_key_probe_rows_strings")


def test_abi_symbols_and_structs():
    for name in ("tgx_plan_set_key_probe_tuples", "tgx_plan_set_key_probe_tuples_counted",
                 "tgx_plan_set_key_probe_rows_tuples", "tgx_key_probe_tuples_get", "tgx_key_probe_entries_tuples"):
        assert name in T.abi_symbols() and hasattr(T.lib(), name)
    assert C.sizeof(T._lib.KeyProbeTuples) == 32 and C.sizeof(T._lib.KeyProbeTupleEntry) == 32


def test_the_column_list_at_plan_creation():
    for arity in range(2, 9):
        T.Plan([spec(T.KEY_PROBE, 0, columns=list(range(arity)))]).set_key_probe_tuples(0)
    with pytest.raises(T.TgxError, match=r"TGX_UNSUPPORTED.*spec 0: KEY_PROBE over 9 columns \(2\.\.8 supported\)"):
        T.Plan([spec(T.KEY_PROBE, 0, columns=list(range(9)))])
    s = spec(T.KEY_PROBE, 0)
    s.n_columns = 3  # (and a NULL list)
    with pytest.raises(T.TgxError, match="TGX_UNSUPPORTED.*KEY_PROBE over 3 columns"):
        T.Plan([s])
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*negative column index"):
        T.Plan([spec(T.KEY_PROBE, 0, columns=[0, -1])])
    # every other kind keeps its refusal, word for word
    for kind in (T.COUNT, T.VALUE_COUNTS, T.NUMERIC_STATS):
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0: only DISTINCT takes a column list"):
            T.Plan([spec(kind, 0, columns=[0, 1])])
    # a state of such a plan needs the spec's parameters like any KEY_PROBE spec
    with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0.*needs its parameters"):
        T.State(T.Plan([spec(T.KEY_PROBE, 0, columns=[0, 1])]))


def test_the_three_calls_and_the_six_exclude_one_another():
    for first in TUPLES:
        for second in TUPLES:
            plan = T.Plan([spec(T.KEY_PROBE, 0, columns=[0, 1])])
            getattr(plan, first)(0)
            if first != second:
                with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0: the check has been set"):
                    getattr(plan, second)(0)
    plan = T.Plan([spec(T.KEY_PROBE, 0, columns=[2, 0]), spec(T.KEY_PROBE, 1), spec(T.COUNT, 0)])
    for call in SINGLE:
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 0: the spec has a column list"):
            getattr(plan, call)(0)
    for call in TUPLES:
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT.*spec 1: tgx_plan_set_key_probe.*needs a spec with a column list"):
            getattr(plan, call)(1)
        with pytest.raises(T.TgxError, match="TGX_INVALID_ARGUMENT"):
            getattr(plan, call)(2)  # (no KEY_PROBE spec)
    for bad in (0, 65537):
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_missing_keys must be 1 \.\. 65536"):
            plan.set_key_probe_tuples(0, bad)
        with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*max_missing_keys must be 1 \.\. 65536"):
            plan.set_key_probe_tuples_counted(0, bad)
    with pytest.raises(T.TgxError, match=r"TGX_INVALID_ARGUMENT.*reserved must be 0 \(3\)"):
        plan.set_key_probe_tuples(0, 10, reserved=3)
