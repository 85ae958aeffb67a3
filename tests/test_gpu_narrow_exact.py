"""-m gpu: columns narrower than 8 bytes (Float32, Int32, the narrow integers, Boolean) against tests/exact_widening.py,
whose expected answers come from the ORIGINAL-width values by integer arithmetic -- never by the hardware conversion the
kernels use.

include/tgx.h promises that every check sees exactly the Int64 / Float64 column the values stand for.  For Float32 that
column is the bit-preserving widening: a signalling NaN stays apart from the quiet NaN of its payload for DISTINCT,
multiplicity and APPROX_DISTINCT, MIN / MAX order the widened bits, subnormals keep their values; Spearman ranks the
CAST AS DOUBLE values, where every NaN is quiet.

Value classes: every f32 NaN pattern, every f32 subnormal (16 777 214 rows each), the specials (+-0, +-inf, FLT_MAX,
FLT_MIN and their neighbours) among ordinary values sorted and shuffled, Int32 extremes, the whole domain of the 1- and
2-byte integers, UInt32 above 2^31, Boolean bits at every bit offset.  NULL slots hold a poison value no row holds.
Routes: one DEVICE batch with its values 16-byte aligned and not (the vector and the scalar path of widen32_kernel),
Arrow offsets that are no multiple of 64, HOST batches, coalesced 8192-row streams, the retained-column repair, merges
in two orders, a blob round trip and threaded ranks."""
import numpy as np
import pytest

import exact_quantiles as Q
import exact_widening as W
import oracle_binding as orc
import term_amd as T
from _lib_spec import spec
from gpu_util import pad_validity
from test_gpu_moments_exact import check_como, check_stats, var_tol
import exact_moments as M

pytestmark = pytest.mark.gpu

F_POISON = 0x4B3C614E   # 12345678.0f: no class below holds it
I_POISON = 1_234_567_891
FLT_EDGES = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7FFFFE, 0x00800000,
             0x80800000, 0x00800001, 0x007FFFFF, 0x807FFFFF, 0x00000001, 0x80000001, 0x3F800000, 0xBF800000]
NAN_SAMPLES = [0x7F800001, 0x7FC00001, 0xFF800001, 0xFFC00001, 0x7FBFFFFF, 0x7FFFFFFF, 0xFFBFFFFF, 0xFFFFFFFF,
               0x7FC00000, 0xFFC00000, 0x7F812345, 0x7FC12345]


def all_nan():
    return np.concatenate([np.arange(0x7F800001, 0x80000000, dtype=np.uint64),
                           np.arange(0xFF800001, 0x100000000, dtype=np.uint64)]).astype(np.uint32)


def all_sub():
    return np.concatenate([np.arange(1, 0x800000, dtype=np.uint64),
                           np.arange(0x80000001, 0x80800000, dtype=np.uint64)]).astype(np.uint32)


def f32_values(kind, n, rng):
    """uint32 patterns of a Float32 column"""
    if kind == "nan_all":
        return all_nan()[rng.permutation(2 * (2 ** 23 - 1))]
    if kind == "sub_all":
        return all_sub()[rng.permutation(2 * (2 ** 23 - 1))]
    x = (rng.standard_normal(n) * 1e3).astype(np.float32).view(np.uint32)
    pick = rng.random(n)
    x[pick < 0.05] = np.array(FLT_EDGES, np.uint32)[rng.integers(0, len(FLT_EDGES), int((pick < 0.05).sum()))]
    sub = (pick >= 0.05) & (pick < 0.08)
    x[sub] = all_sub()[rng.integers(0, 2 * (2 ** 23 - 1), int(sub.sum()))]
    if kind in ("mixed_nan", "sorted_nan"):
        nan = (pick >= 0.08) & (pick < 0.11)
        x[nan] = np.array(NAN_SAMPLES, np.uint32)[rng.integers(0, len(NAN_SAMPLES), int(nan.sum()))]
        x[(pick >= 0.11) & (pick < 0.12)] = all_nan()[rng.integers(0, 2 * (2 ** 23 - 1), int(((pick >= 0.11) & (pick < 0.12)).sum()))]
    x[:len(FLT_EDGES)] = FLT_EDGES  # every edge at least once
    x[x == F_POISON] = 0x3F800000
    if kind.startswith("sorted"):
        x = x[np.argsort(W.total_key(W.widen_f32_bits(x)), kind="stable")]
    return x


def i32_partner(n, rng):
    v = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    v[rng.random(n) < 0.3] = rng.integers(-40, 40)
    v[: 4] = [-2 ** 31, 2 ** 31 - 1, 0, -1]
    v[v == I_POISON] = 7
    return v.astype(np.int32)


def layout(name, n, rng):
    if name == "none":
        return None
    if name == "nulls_first":
        m = np.ones(n, bool)
        m[: (n * 3) // 10 + 1] = False
        return m
    if name == "sparse":
        return rng.random(n) >= 0.1
    return np.zeros(n, bool)  # all_null


def poisoned(vals, mask, poison):
    if mask is None:
        return vals
    out = vals.copy()
    out[~mask] = poison
    return out


class Table:
    """a Float32 column (uint32 patterns) and an Int32 partner with one validity mask, and their references"""

    def __init__(self, f_bits, i32, mask):
        self.n = len(f_bits)
        self.mask = mask
        self.f = poisoned(f_bits, mask, F_POISON)
        self.i = poisoned(i32, mask, I_POISON)
        self.vb = None if mask is None else orc.pack_validity(mask)
        self.wide_f = W.widen_f32_bits(self.f)

    def valid(self):
        return np.ones(self.n, bool) if self.mask is None else self.mask


def column(kind, vals, validity_mask, mem, lo, hi, lead=0, unaligned=False):
    """rows lo .. hi of the column as a column of its own, `lead` rows of poison ahead of them (an Arrow offset);
    unaligned: the values buffer starts 4 bytes past a 16-byte boundary"""
    v = vals[lo:hi]
    m = None if validity_mask is None else validity_mask[lo:hi]
    poison = np.uint32(F_POISON) if kind == "f" else np.int32(I_POISON)
    v = np.concatenate([np.full(lead, poison, v.dtype), v, np.full(64, poison, v.dtype)])
    b = None if m is None else pad_validity(orc.pack_validity(np.concatenate([np.zeros(lead, bool), m])))
    ctor = T.Column.float32 if kind == "f" else T.Column.int32
    if mem == "host":
        return ctor(v.view(np.float32) if kind == "f" else v, b, length=hi - lo, offset=lead)
    import torch

    raw = np.concatenate([np.zeros(1, v.dtype), v]) if unaligned else v
    t = torch.from_numpy(raw.view(np.int32).copy()).cuda()
    if unaligned:
        t = t[1:]
        assert t.data_ptr() % 16 == 4
    return ctor(t, None if b is None else torch.from_numpy(b).cuda(), length=hi - lo, offset=lead)


SPECS = [spec(T.COUNT, 0), spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE), spec(T.DISTINCT, 0),
         spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.KLL, 0, kll_k=200), spec(T.NUMERIC_STATS, 1, flags=T.FLAG_VARIANCE),
         spec(T.DISTINCT, 1, flags=T.FLAG_MULTIPLICITY), spec(T.COMOMENTS, 1, column2=0), spec(T.APPROX_DISTINCT, 0)]
RANK_SPECS = [spec(T.SPEARMAN, 0, column2=1)]
HLL_SPECS = [spec(T.APPROX_DISTINCT, 0)]  # (alone: next to a DISTINCT of its column the exact key set answers)


def registers_of(state):
    """the last task's HyperLogLog registers: the tail of the state blob (term_amd/wire.py)"""
    return np.frombuffer(state.serialize()[-16384:], dtype=np.uint8)


def check_hll(tab, res, st):
    """APPROX_DISTINCT: the registers of the injective widening, and the estimate they give"""
    want = W.hll_registers(tab.wide_f, tab.vb)
    assert res[0].distinct == orc.hll_estimate(want), ("hll", res[0].distinct, orc.hll_estimate(want), tab.n)
    assert np.array_equal(registers_of(st), want), ("hll registers", tab.n)


def check(tab, res, st, rows_per_merge=None, spearman=None):
    where = "n=%d" % tab.n
    valid = tab.valid()
    assert (res[0].total, res[0].non_null) == (tab.n, int(valid.sum())), where
    # NUMERIC_STATS of the Float32 column: MIN / MAX bit for bit under the total order, the moments exactly
    r = res[1]
    lo, hi = W.minmax_bits(tab.wide_f, tab.vb)
    if lo is not None:
        got = (int(np.float64(r.min_f).view(np.uint64)), int(np.float64(r.max_f).view(np.uint64)))
        assert got == (lo, hi), ("min/max", [hex(x) for x in got], hex(lo), hex(hi), where)
    ref = W.float_moments(tab.wide_f, tab.vb)
    check_stats(r, ref, var_tol(ref, rows_per_merge))
    # DISTINCT by the original bits, with and without multiplicity
    nn, d, once = W.distinct(tab.f, tab.vb)
    assert (res[2].non_null, res[2].distinct) == (nn, d), ("distinct", res[2].distinct, d, where)
    assert (res[3].non_null, res[3].distinct, res[3].groups_once) == (nn, d, once), \
        ("multiplicity", res[3].distinct, res[3].groups_once, d, once, where)
    # KLL of the widened values, NaN dropped
    Q.check_sketch(st, 4, W.kll_kept(tab.wide_f, tab.vb), 200, result=res[4])
    # the Int32 partner: sign-extended
    wide_i = W.widen_int(tab.i, "int32")
    ri = W.int_stats(wide_i, tab.vb)
    r = res[5]
    assert r.non_null == ri[0]
    if ri[0]:
        assert (r.min_i, r.max_i, r.sum_i) == ri[1:], ("int32", (r.min_i, r.max_i, r.sum_i), ri, where)
    nn, d, once = W.distinct(tab.i, tab.vb)
    assert (res[6].distinct, res[6].groups_once) == (d, once), where
    # COMOMENTS over the rows where both are valid; exact where the Float32 values are finite
    fin = (tab.wide_f & np.uint64(W.F64_EXP)) != np.uint64(W.F64_EXP)
    if (fin | ~valid).all():
        check_como(res[7], M.comoments(wide_i, tab.wide_f.view(np.float64), tab.vb, tab.vb))
    else:
        assert res[7].non_null == int(valid.sum())
    # APPROX_DISTINCT next to DISTINCT of the same column: the exact key set answers
    assert res[8].distinct == W.distinct(tab.f, tab.vb)[1], ("approx", res[8].distinct, where)
    if spearman is not None:
        kx = W.total_key(W.cast_f32_bits(tab.f[valid]))
        want = W.rank_sums(kx, wide_i[valid])
        s = spearman
        assert (s.non_null, s.sum_x, s.sum_y, s.sum_x2, s.sum_y2, s.sum_xy) == want, \
            ("spearman", (s.non_null, s.sum_x, s.sum_y, s.sum_x2, s.sum_y2, s.sum_xy), want, where)


def cuts_of(route, n):
    if route in ("stream_device", "stream_host"):
        return list(range(0, n, 8192)) + [n]
    if route in ("offsets_device", "host"):
        a = n // 3 + 5
        return sorted({0, min(a, n), min(a + 129, n), n})
    return [0, n]


def feed(tab, plan_specs, route):
    mem = "host" if route in ("host", "stream_host") else "device"
    lead = 37 if route in ("offsets_device", "host") else 0
    st = T.State(T.Plan(plan_specs))
    cuts = cuts_of(route, tab.n)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        st.update([column("f", tab.f, tab.mask, mem, lo, hi, lead, unaligned=route == "unaligned"),
                   column("i", tab.i, tab.mask, mem, lo, hi, lead)])
    return st


def run_route(tab, route):
    st = feed(tab, SPECS, route)
    res = st.finalize()
    rs = feed(tab, RANK_SPECS, route)
    per = 8192 if route.startswith("stream") else None
    check(tab, res, st, rows_per_merge=per, spearman=rs.finalize()[0])
    hs = feed(tab, HLL_SPECS, route)
    check_hll(tab, hs.finalize(), hs)


ROUTES = ["aligned", "unaligned", "offsets_device", "host", "stream_device", "stream_host"]


@pytest.fixture(autouse=True)
def _init():
    T.init()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("lay", ["none", "nulls_first", "sparse", "all_null"])
@pytest.mark.parametrize("kind", ["mixed", "mixed_nan", "sorted_nan"])
def test_float32_specials_on_every_route(kind, lay, route):
    import zlib

    rng = np.random.default_rng(zlib.crc32(("%s/%s/%s" % (kind, lay, route)).encode()))
    n = 70_001 if route.startswith("stream") else 300_003
    tab = Table(f32_values(kind, n, rng), i32_partner(n, rng), layout(lay, n, rng))
    run_route(tab, route)


@pytest.mark.parametrize("kind,route,lay", [("nan_all", "aligned", "none"), ("nan_all", "unaligned", "sparse"),
                                            ("nan_all", "host", "nulls_first"), ("sub_all", "aligned", "sparse"),
                                            ("sub_all", "unaligned", "none"), ("sub_all", "host", "none")])
def test_every_nan_and_every_subnormal_pattern(kind, route, lay):
    """16 777 214 rows: each pattern once (shuffled), so DISTINCT must count every one of them"""
    rng = np.random.default_rng(len(kind) * 7 + len(route) + len(lay))
    f = f32_values(kind, 0, rng)
    tab = Table(f, i32_partner(len(f), rng), layout(lay, len(f), rng))
    run_route(tab, route)


@pytest.mark.parametrize("kind", ["mixed_nan", "sub_dense"])
def test_merged_in_two_orders_and_a_blob(kind):
    rng = np.random.default_rng(11 if kind == "mixed_nan" else 12)
    n = 400_000
    f = f32_values("mixed_nan", n, rng) if kind == "mixed_nan" else all_sub()[rng.integers(0, 2 * (2 ** 23 - 1), n)]
    tab = Table(f, i32_partner(n, rng), layout("sparse", n, rng))
    cuts = [0, 1000, 150_001, n]
    for specs, chk in ((SPECS, lambda r, s: check(tab, r, s, rows_per_merge=n // 3)),
                       (HLL_SPECS, lambda r, s: check_hll(tab, r, s))):
        plan = T.Plan(specs)
        parts = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            s = T.State(plan)
            s.update([column("f", tab.f, tab.mask, "device", lo, hi), column("i", tab.i, tab.mask, "device", lo, hi)])
            parts.append(s)
        for order in ([0, 1, 2], [2, 0, 1]):
            m = T.State(plan)
            m.merge([parts[i] for i in order])
            chk(m.finalize(), m)
        back = T.State.deserialize(plan, m.serialize())
        chk(back.finalize(), back)


def test_threaded_ranks():
    from term_amd.distributed import shard_rows
    from test_gpu_distributed_sim import _run_ranks

    rng = np.random.default_rng(13)
    n = 600_003
    tab = Table(f32_values("mixed_nan", n, rng), i32_partner(n, rng), layout("sparse", n, rng))

    def shards_of(rank):
        lo, hi = shard_rows(n, 4, rank)
        return [column("f", tab.f, tab.mask, "device", lo, hi, 5), column("i", tab.i, tab.mask, "device", lo, hi, 5)]

    for res, st in _run_ranks(4, T.Plan(SPECS), shards_of):
        check(tab, res, st, rows_per_merge=n // 4)
    for res, st in _run_ranks(4, T.Plan(HLL_SPECS), shards_of):
        check_hll(tab, res, st)


def test_retained_float32_keys_repaired_after_a_sampled_range(monkeypatch):
    """DEVICE Float32 key columns are retained as the caller's 4-byte column and widened again for the repair
    (distinct_state.cpp, retained_numeric_view): keys outside the range the first batch's sample laid out, NaN payloads
    of both kinds among them, and one heavy key whose list overflows"""
    monkeypatch.setenv("TGX_FP_LISTS_MIN_ROWS", "1000")
    T.init()
    rng = np.random.default_rng(14)
    n = 100_000
    arrays = []
    for b in range(3):
        x = (rng.random(n) * (10.0 ** (b * 3)) + b * 1e6).astype(np.float32).view(np.uint32)
        x[rng.random(n) < 0.02] = np.array(NAN_SAMPLES, np.uint32)[rng.integers(0, len(NAN_SAMPLES), 1)]
        x[rng.random(n) < 0.01] = all_nan()[rng.integers(0, 2 * (2 ** 23 - 1), 1)]
        if b == 1:
            x[: n // 2] = 0x7F800001  # the heavy key is a signalling NaN
        x[rng.random(n) < 0.01] = all_sub()[rng.integers(0, 2 * (2 ** 23 - 1), 1)]
        arrays.append(x)
    st = T.State(T.Plan([spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.DISTINCT, 0)]))
    for a in arrays:
        st.update([column("f", a, None, "device", 0, n)])
    res = st.finalize()
    _, d, once = W.distinct(np.concatenate(arrays))
    assert (res[0].total, res[0].distinct, res[0].groups_once) == (3 * n, d, once)
    assert res[1].distinct == d


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("int32", [True, False])
def test_keys_of_a_batch_whose_sampled_rows_are_null(int32, device):
    """A first batch of 100 006 rows, the first 90 001 NULL: the key set's range sample (65 536 rows) sees no value,
    and the batch's keys must still be counted (distinct_state.cpp: an undecided key set reads every row first)."""
    rng = np.random.default_rng(15 + 2 * int32 + int(device))
    n, cut = 300_003, 100_006
    v = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64)
    v[rng.random(n) < 0.3] = 5
    mask = np.ones(n, bool)
    mask[:90_001] = False
    vals = v.astype(np.int32) if int32 else v
    st = T.State(T.Plan([spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.DISTINCT, 0)]))
    for lo, hi in ((0, cut), (cut, n)):
        b = pad_validity(orc.pack_validity(mask[lo:hi]))
        x = np.ascontiguousarray(vals[lo:hi])
        if device:
            import torch

            x, b = torch.from_numpy(x).cuda(), torch.from_numpy(b).cuda()
        st.update([(T.Column.int32 if int32 else T.Column.int64)(x, b, length=hi - lo)])
    res = st.finalize()
    nn, d, once = W.distinct(vals, orc.pack_validity(mask))
    assert (res[0].non_null, res[0].distinct, res[0].groups_once) == (nn, d, once)
    assert res[1].distinct == d


NARROW = [(T.INT8, np.int8, "int8"), (T.INT16, np.int16, "int16"), (T.UINT8, np.uint8, "uint8"),
          (T.UINT16, np.uint16, "uint16"), (T.UINT32, np.uint32, "uint32"), (T.INT32, np.int32, "int32")]


def narrow_values(dtype, rng):
    info = np.iinfo(dtype)
    if info.bits <= 16:  # the whole domain, every value three times, shuffled
        v = np.tile(np.arange(int(info.min), int(info.max) + 1, dtype=np.int64), 3)
    else:
        v = rng.integers(int(info.min), int(info.max) + 1, size=200_000, dtype=np.int64)
        v[rng.random(len(v)) < 0.2] = int(info.max)
        v[:6] = [info.min, info.min + 1, info.max, info.max - 1, 2 ** 31 - 1 if info.max > 2 ** 31 else 0,
                 2 ** 31 if info.max > 2 ** 31 else -1]
    return v[rng.permutation(len(v))].astype(dtype)


def narrow_column(type_id, vals, mask, mem, lo, hi, lead):
    v = vals[lo:hi]
    v = np.concatenate([np.full(lead, np.iinfo(vals.dtype).max // 3, vals.dtype), v, np.zeros(64, vals.dtype)])
    b = None if mask is None else pad_validity(orc.pack_validity(np.concatenate([np.zeros(lead, bool), mask[lo:hi]])))
    if mem == "device":
        import torch

        return T.Column(type_id, hi - lo, values=torch.from_numpy(v.view(np.uint8).copy()).cuda(),
                        validity=None if b is None else torch.from_numpy(b).cuda(), offset=lead)
    return T.Column(type_id, hi - lo, values=v, validity=b, offset=lead)


@pytest.mark.parametrize("route", ["device", "host", "stream_host", "stream_device"])
@pytest.mark.parametrize("lay", ["none", "nulls_first", "sparse"])
@pytest.mark.parametrize("type_id,dtype,name", NARROW)
def test_integers_sign_and_zero_extended(type_id, dtype, name, lay, route):
    rng = np.random.default_rng(type_id * 31 + len(lay) + len(route))
    vals = narrow_values(dtype, rng)
    n = len(vals)
    mask = layout(lay, n, rng)
    vb = None if mask is None else orc.pack_validity(mask)
    wide = W.widen_int(vals, name)
    specs = [spec(T.COUNT, 0), spec(T.NUMERIC_STATS, 0, flags=T.FLAG_VARIANCE), spec(T.DISTINCT, 0),
             spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY), spec(T.KLL, 0, kll_k=200), spec(T.APPROX_DISTINCT, 0)]
    st, hs = T.State(T.Plan(specs)), T.State(T.Plan([spec(T.APPROX_DISTINCT, 0)]))
    mem = "host" if "host" in route else "device"
    cuts = list(range(0, n, 8192)) + [n] if route.startswith("stream") else [0, n // 3 + 3, n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        for s in (st, hs):
            s.update([narrow_column(type_id, vals, mask, mem, lo, hi, 0 if route.startswith("stream") else 19)])
    res = st.finalize()
    assert (res[0].total, res[0].non_null) == W.count(n, vb)
    nn, lo_, hi_, s = W.int_stats(wide, vb)
    r = res[1]
    assert (r.non_null, r.min_i, r.max_i, r.sum_i) == (nn, lo_, hi_, s), (name, r.min_i, r.max_i, r.sum_i, lo_, hi_, s)
    check_stats(r, M.moments(wide, vb), var_tol(M.moments(wide, vb), 8192 if route.startswith("stream") else None))
    _, d, once = W.distinct(vals, vb)
    assert res[2].distinct == d and (res[3].distinct, res[3].groups_once) == (d, once)
    Q.check_sketch(st, 4, Q.kept(wide, vb), 200, result=res[4])
    assert res[5].distinct == d  # (next to DISTINCT of its column: the exact key set answers)
    want = W.hll_registers(wide.view(np.uint64), vb)
    assert hs.finalize()[0].distinct == orc.hll_estimate(want) and np.array_equal(registers_of(hs), want)


@pytest.mark.parametrize("device", [True, False])
@pytest.mark.parametrize("bit_offset", range(8))
def test_boolean_bits_at_every_offset(bit_offset, device):
    rng = np.random.default_rng(bit_offset * 2 + int(device))
    n = 5000 + bit_offset * 131
    bools = rng.random(n) < (0.0 if bit_offset == 3 else 1.0 if bit_offset == 5 else 0.3)
    mask = None if bit_offset % 2 else rng.random(n) >= 0.2
    buf = np.packbits(np.concatenate([rng.random(bit_offset) < 0.5, bools]), bitorder="little")
    buf = np.concatenate([buf, np.zeros(64, np.uint8)])
    vb = None if mask is None else pad_validity(orc.pack_validity(np.concatenate([np.zeros(bit_offset, bool), mask])))
    if device:
        import torch

        vals, valid = torch.from_numpy(buf).cuda(), None if vb is None else torch.from_numpy(vb).cuda()
    else:
        vals, valid = buf, vb
    st = T.State(T.Plan([spec(T.COUNT, 0), spec(T.DISTINCT, 0, flags=T.FLAG_MULTIPLICITY)]))
    st.update([T.Column(T.BOOL, n, values=vals, validity=valid, offset=bit_offset)])
    res = st.finalize()
    wide = W.widen_int(buf, "bool", n=n, bit_offset=bit_offset)
    assert np.array_equal(wide, bools.astype(np.int64))
    assert (res[0].total, res[0].non_null) == W.count(n, vb, bit_offset)
    _, d, once = W.distinct(wide, None if mask is None else orc.pack_validity(mask))
    assert (res[1].distinct, res[1].groups_once) == (d, once)
