"""-m gpu: a state blob with a section of every kind that writes one (term_amd/wire.py documents the layout) goes
through tgx_state_deserialize and back byte for byte -- up to the order of a key set's records, see records_sorted --
and every proper prefix of it is refused with TGX_INVALID_ARGUMENT, under the text of the module whose section the cut
falls into where that module has one."""
import math
import struct

import numpy as np
import pytest

import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity, to_device
from term_amd import wire
from term_amd._lib import Result

pytestmark = pytest.mark.gpu

KEY = bytes(range(0x40, 0x50))
ROWS = 300
KLL_K = 8
BINNING = (0.0, 20.0, -3.0, 3.0, 2)
INVALID_ARGUMENT = 1


def specs(kll_k=KLL_K):
    return [spec(T.COUNT, 4), spec(T.NUMERIC_STATS, 1, flags=T.FLAG_VARIANCE), spec(T.COMOMENTS, 0, column2=1),
            spec(T.DISTINCT, 0), spec(T.DISTINCT, 2, flags=T.FLAG_EXACT_KEYS), spec(T.APPROX_DISTINCT, 3),
            spec(T.KLL, 1, kll_k=kll_k), spec(T.REGEX_MATCH, 2, pattern=r"^user\d+@"), spec(T.LENGTH, 2, length_max=12),
            spec(T.JOINT_BINS, 0, column2=1)]


def make_plan(kll_k=KLL_K):
    plan = T.Plan(specs(kll_k), fingerprint_key=KEY)
    plan.set_joint_binning(9, *BINNING)
    return plan


def columns():
    """the one batch: an Int64, a Float64 and a Utf8 column of ROWS rows on the device, each with some NULLs; an Int64
    column without (APPROX_DISTINCT keeps registers for a column that no variance and no exact check reads); and the
    Float64 column once more, for COUNT alone (on a column that is scanned anyway COUNT rides on the scan)"""
    rng = np.random.default_rng(20261017)
    ints = rng.integers(0, 60, size=ROWS, dtype=np.int64)
    floats = rng.standard_normal(ROWS)
    words = [None if i % 17 == 3 else ("user%d@example.com" % (i % 90) if i % 4 else "Zoë%d" % (i % 11)) for i in range(ROWS)]
    offs, data, sval = orc.utf8_from_list(words)
    pad = np.zeros(64, np.uint8)
    ival, fval = (pad_validity(orc.pack_validity(rng.random(ROWS) >= 0.1)) for _ in range(2))
    floats_d, fval_d = to_device(floats), to_device(fval)
    return [T.Column.int64(to_device(ints), to_device(ival)), T.Column.float64(floats_d, fval_d),
            T.Column(T.UTF8, ROWS, offsets=to_device(offs), data=to_device(np.concatenate([data, pad])),
                     validity=to_device(np.concatenate([sval, pad]))),
            T.Column.int64(to_device(rng.integers(0, 1000, size=ROWS, dtype=np.int64))),
            T.Column.float64(floats_d, fval_d)]


def sections(blob, records=None):
    """name -> (first byte, end) of the blob's sections, walked by the layout of term_amd/wire.py; `records` (a list)
    receives (first byte, end, record size) of every DISTINCT task's key records"""
    u32 = lambda p: struct.unpack_from("<I", blob, p)[0]
    u64 = lambda p: struct.unpack_from("<Q", blob, p)[0]
    magic, version, n_scan, n_count, n_como, n_dist, n_kll, n_regex, n_hll = struct.unpack_from("<9I", blob, 0)
    assert (magic, version) == (wire.MAGIC, wire.VERSION)
    out, pos = {}, 0

    def close(name, end):
        nonlocal pos
        out[name] = (pos, end)
        pos = end

    close("head", 9 * 4 + 4 + 16)
    close("scan", pos + 96 * n_scan)
    close("count", pos + 16 * n_count)
    close("comoments", pos + 120 * n_como)
    p = pos
    for _ in range(n_dist):  # { u32 partitioned, wide; 5 u64 totals; u64 n_records; records }
        size = 32 if u32(p + 4) else 16
        if records is not None:
            records.append((p + 56, p + 56 + u64(p + 48) * size, size))
        p += 56 + u64(p + 48) * size
    close("distinct", p)
    for _ in range(n_kll):
        levels = u32(p + 4)
        p += 32
        for _ in range(levels):
            p += 4 + 8 * u32(p)
    close("kll", p)
    close("regex", pos + 16 * n_regex)
    p = pos
    for _ in range(n_hll):
        p += 8 + 16384 * u32(p + 4)
    close("hll", p)
    if p < len(blob):
        assert u32(p) == wire.JOINT_MAGIC
        tasks = u32(p + 4)
        p += 8
        for _ in range(tasks):
            p += 104 + 8 * u64(p + 96)
        close("joint", p)
    return out


def records_sorted(blob):
    """the blob with every DISTINCT task's key records in ascending order.  A key set travels as its records in the order
    of the hash table's slots, which the insert kernels' races decide: two states fed the same batch -- and a state and
    its own round trip -- hold the same records in another order, so blobs are compared in this form."""
    spans, out = [], bytearray(blob)
    sections(blob, spans)
    for lo, hi, size in spans:
        out[lo:hi] = b"".join(sorted(blob[k:k + size] for k in range(lo, hi, size)))
    return bytes(out)


@pytest.fixture(scope="module")
def fed():
    """(plan, state, blob) of the one batch"""
    T.init()
    plan = make_plan()
    st = T.State(plan)
    st.update(columns())
    return plan, st, st.serialize()


def refused(plan, blob):
    with pytest.raises(T.TgxError) as e:
        T.State.deserialize(plan, blob)
    assert e.value.code == INVALID_ARGUMENT, (len(blob), e.value.status, e.value.msg)
    return e.value.msg


def test_round_trip(fed):
    plan, st, blob = fed
    sec = sections(blob)
    assert list(sec) == ["head", "scan", "count", "comoments", "distinct", "kll", "regex", "hll", "joint"]
    assert all(hi > lo for lo, hi in sec.values()) and sec["joint"][1] == len(blob)
    back = T.State.deserialize(plan, blob)
    again = back.serialize()
    assert len(again) == len(blob) and records_sorted(again) == records_sorted(blob)
    for got, want in zip(back.finalize(), st.finalize()):
        for name, _ in Result._fields_:
            a, b = getattr(got, name), getattr(want, name)
            assert a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b)), name


def test_every_prefix_is_refused(fed):
    plan, _, blob = fed
    assert len(blob) > 512
    cuts = list(range(0, 256, 4)) + [len(blob) - 1]
    cuts += [256 + (len(blob) - 1 - 256) * i // 64 for i in range(64)]
    for cut in cuts:
        refused(plan, blob[:cut])


def test_each_module_reports_its_own_section(fed):
    plan, _, blob = fed
    sec = sections(blob)
    assert refused(plan, blob[:sec["scan"][0] + 40]) == "truncated state blob"
    kll = sec["kll"][0]
    assert refused(plan, blob[:kll + 4]) == "truncated state blob (kll)"           # inside the task's head
    assert refused(plan, blob[:sec["kll"][1] - 4]) == "truncated state blob (kll)"  # inside a level's items
    assert refused(plan, blob[:kll + 4] + struct.pack("<I", 65) + blob[kll + 8:]) == "corrupt state blob (kll levels)"
    assert refused(plan, blob[:sec["regex"][0] + 8]) == "truncated state blob (regex)"
    assert refused(plan, blob[:sec["regex"][1] - 8]) == "truncated state blob (regex)"
    joint = sec["joint"][0]
    assert refused(plan, blob[:joint + 4]) == "state blob was produced by a different plan (JOINT_BINS section)"
    assert refused(plan, blob[:len(blob) - 8]) == "malformed state blob (JOINT_BINS task 0)"  # inside the cells


def test_another_k_is_refused(fed):
    _, _, blob = fed
    assert "produced with k=%d, plan has k=16" % KLL_K in refused(make_plan(kll_k=16), blob)
