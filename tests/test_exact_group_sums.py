"""tests/exact_group_sums.py is what the GPU tests of TGX_CHECK_GROUP_SUMS and of CrossTableSumConstraint trust, so it is
held to a second statement of the same thing: numpy's add.at for wrapping integer sums, pyarrow's group_by().aggregate
where it applies, and to tests/golden/cross_table_sum_vectors.json -- the tables and verdicts of the reference's own unit
tests plus hand-derived cases."""
import json
import math
import os

import numpy as np
import pyarrow as pa
import pytest

import exact_group_sums as ex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cross_table_sum_vectors.json")


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def golden_side(side, group_by):
    """(values, groups or None, is_float) of one side of a golden case"""
    cols = side["columns"]
    kind, values = cols[side["column"]]
    groups = None
    if group_by:
        gkind, groups = cols[group_by[0]]
        groups = [g.encode() if isinstance(g, str) else g for g in groups]
    return values, groups, kind.startswith("float")


def test_wrap_is_int64_arithmetic():
    assert ex.wrap(2**63) == -2**63 and ex.wrap(-2**63 - 1) == 2**63 - 1 and ex.wrap(2**64 + 5) == 5 and ex.wrap(-1) == -1
    a = np.array([2**63 - 1, 2**63 - 1, -2**63, 7], dtype=np.int64)
    with np.errstate(over="ignore"):
        assert ex.wrap(sum(int(x) for x in a)) == int(a.sum())  # (numpy's Int64 sum wraps as DataFusion's does)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_integer_walk_against_numpy_add_at(seed):
    rng = np.random.default_rng(seed)
    n = 5000
    keys = rng.integers(-5, 40, n)
    key_valid = rng.random(n) >= 0.1
    vals = rng.choice(np.array([2**63 - 1, -2**63, 2**62, -3, 11, 0], dtype=np.int64), n)
    valid = rng.random(n) >= 0.3
    got = ex.walk([int(v) if ok else None for v, ok in zip(vals, valid)],
                  [int(k) if ok else None for k, ok in zip(keys, key_valid)])
    uniq, inverse = np.unique(keys[key_valid], return_inverse=True)
    rows = np.zeros(len(uniq), np.int64)
    non_null = np.zeros(len(uniq), np.int64)
    sums = np.zeros(len(uniq), np.uint64)  # (unsigned: the wrap is defined)
    np.add.at(rows, inverse, 1)
    np.add.at(non_null, inverse, valid[key_valid].astype(np.int64))
    np.add.at(sums, inverse, np.where(valid, vals, 0)[key_valid].astype(np.uint64))
    want = {int(k): (int(r), int(nn), int(s.astype(np.int64))) for k, r, nn, s in zip(uniq, rows, non_null, sums)}
    assert got["entries"] == want and list(got["entries"]) == sorted(want)
    assert got["null_group"] == (int((~key_valid).sum()), int((valid & ~key_valid).sum()),
                                 ex.wrap(sum(int(v) for v in vals[valid & ~key_valid])))
    assert got["counted"] == (int(rows.sum()), int(non_null.sum()), ex.wrap(sum(int(s) for s in sums)))
    assert (got["seen"], got["groups"], got["is_float"], got["overflow"], got["long_rows"]) == \
        (n, len(uniq), False, (0, 0, 0), (0, 0, 0))


def test_walk_against_pyarrow_group_by():
    rng = np.random.default_rng(3)
    n = 4000
    keys = ["k%d" % k if k else None for k in rng.integers(0, 30, n)]
    ints = [int(v) if ok else None for v, ok in zip(rng.integers(-1000, 1000, n), rng.random(n) >= 0.3)]
    flts = [float(v) if ok else None for v, ok in zip(rng.integers(-2**20, 2**20, n), rng.random(n) >= 0.3)]
    table = pa.table({"g": pa.array(keys, pa.string()), "i": pa.array(ints, pa.int64()), "f": pa.array(flts, pa.float64())})
    agg = table.group_by("g").aggregate([("i", "count"), ("i", "sum"), ("f", "sum"), ([], "count_all")]).to_pydict()
    by_key = {g: (rows, nn, s_i, s_f) for g, nn, s_i, s_f, rows in
              zip(agg["g"], agg["i_count"], agg["i_sum"], agg["f_sum"], agg["count_all"])}
    got_i = ex.walk(ints, [None if k is None else k.encode() for k in keys])
    got_f = ex.walk(flts, [None if k is None else k.encode() for k in keys], is_float=True)
    for key, (rows, nn, s_i, s_f) in by_key.items():
        e_i = got_i["null_group"] if key is None else got_i["entries"][key.encode()]
        e_f = got_f["null_group"] if key is None else got_f["entries"][key.encode()]
        assert e_i == (rows, nn, s_i or 0)
        assert e_f[0] == rows and e_f[2] == (s_f or 0.0)  # small integers: exact in any order, pyarrow's included
    assert len(by_key) == got_i["groups"] + 1 and list(got_i["entries"]) == sorted(got_i["entries"])


def test_long_keys_and_the_float_classes():
    got = ex.walk([1.5, None, 2.5, 4.0], [b"abc", b"abcd", b"abcd", None], max_value_bytes=3, is_float=True)
    assert got["entries"] == {b"abc": (1, 1, 1.5, 1.5)} and got["long_rows"] == (2, 1, 2.5, 2.5)
    assert got["null_group"] == (1, 1, 4.0, 4.0) and got["counted"] == (1, 1) and got["is_float"] is True
    assert ex.walk([], [], is_float=True)["is_float"] is False
    nan = ex.float_class(3, [math.inf, -math.inf, 1.0])
    assert nan[2] != nan[2] and ex.float_class(2, [math.inf, 1.0])[2] == math.inf
    assert ex.float_class(2, [1.0, math.nan])[2] != ex.float_class(2, [1.0, math.nan])[2]


def test_the_float_bound_covers_orders_that_differ():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(2000) * np.exp(rng.uniform(-30, 30, 2000))).tolist()
    exact, mags = math.fsum(x), math.fsum(abs(v) for v in x)
    bound = ex.float_bound(len(x), exact, mags)
    orders = [x, x[::-1], sorted(x), sorted(x, key=abs), sorted(x, key=abs, reverse=True)]
    sums = []
    for o in orders:
        s = 0.0
        for v in o:
            s += v
        sums.append(s)
    pairwise = np.add.reduce(np.array(x))  # (numpy's pairwise tree)
    assert len(set(sums)) > 1  # the orders do differ
    assert all(abs(s - exact) <= bound for s in sums + [float(pairwise)])
    assert bound < 1e-12 * mags and ex.float_bound(1, 5.0, 5.0) == 2.0 ** -53 * 5.0 and ex.float_bound(0, 0.0, 0.0) == 0.0


def test_rust_number_formats():
    assert [ex.rust_f64(v) for v in (300.0, 14.5, 100.005, -0.0, 1e21, 1e-7, math.inf, -math.inf)] == \
        ["300", "14.5", "100.005", "-0", "1000000000000000000000", "0.0000001", "inf", "-inf"]
    assert ex.rust_f64(math.nan) == "NaN" and ex.rust_f64(-9223372036854775808.0) == "-9223372036854776000"
    assert [ex.fixed4(v) for v in (50.0, 0.003999999999990678, 0.00005, math.inf, math.nan)] == \
        ["50.0000", "0.0040", "0.0001", "inf", "NaN"]


def test_qualified_names():
    assert ex.parse_qualified("orders.total") == ("orders", "total")
    for bad in ("orders", "a.b.c", ""):
        with pytest.raises(ValueError, match=r"Column must be qualified \(table.column\): '%s'" % bad):
            ex.parse_qualified(bad)


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_the_golden_vectors(case):
    sides = []
    for side in (case["left"], case["right"]):
        values, groups, is_float = golden_side(side, case["group_by"])
        sides.append(ex.side_sums(values, groups, is_float))
    got = ex.cross_table_sum(sides[0], sides[1], case["tolerance"], case["group_by"],
                             "%s.%s" % (case["left"]["table"], case["left"]["column"]),
                             "%s.%s" % (case["right"]["table"], case["right"]["column"]),
                             case.get("max_violations_reported", 100))
    want = case["expect"]
    assert {k: got[k] for k in want} == want
    assert got["metric"] == want["max_difference"]


def test_nan_and_the_order_of_the_totals():
    nan = math.nan
    got = ex.cross_table_sum({1: nan, 2: 5.0}, {1: 1.0, 2: 1.0}, group_by_columns=["g"])
    assert got["violating_groups"] == 1 and got["max_difference"] != got["max_difference"]  # NaN > 0 is false; NaN shows
    assert ex.cross_table_sum({1: nan}, {1: 1.0}, group_by_columns=["g"])["status"] == "success"
    # ascending by key, the NULL groups last, the left one first: 1e16 + 1 + 1 is not 1 + 1 + 1e16
    got = ex.cross_table_sum({None: 1.0, 2: 1.0, 1: 1e16}, {1: 1e16, 2: 1.0, None: 1.0}, group_by_columns=["g"])
    assert got["total_left_sum"] == (1e16 + 1.0) + 1.0 + 0.0 and got["total_right_sum"] == (1e16 + 1.0) + 0.0 + 1.0
    assert got["total_groups"] == 4 and got["violating_groups"] == 2


# ---- the numpy twin against the plain walk; the overflow rule --------------------------------------------------------------
def test_the_numpy_twin_agrees_with_the_walk():
    import numpy as np

    rng = np.random.default_rng(20261)
    words = [b"", b"a", b"ab", b"b", "ÿ".encode(), b"long word!", b"x" * 40] + [b"w%d" % k for k in range(9)]
    pool = np.array([np.nan, np.inf, -np.inf, -0.0, 1e308, -1e308, 5e-324])
    met = set()  # (the decisions of the overflow rule that the tables reach)
    for n, null_rate, max_bytes in ((0, 0.0, 256), (1, 0.0, 256), (400, 0.2, 256), (400, 0.2, 4), (400, 1.0, 4),
                                    (3000, 0.05, 1), (3000, 0.3, 9)):
        for is_float in (False, True):
            if is_float:
                vals = np.round(rng.standard_normal(n) * 4, 1)
                hit = rng.random(n) < 0.1
                vals[hit] = pool[rng.integers(0, len(pool), size=int(hit.sum()))]
            else:
                vals = rng.integers(-(2**63), 2**63 - 1, size=n, dtype=np.int64)  # (the sums wrap)
            valid = rng.random(n) >= null_rate
            listed = [(float(v) if is_float else int(v)) if m else None for v, m in zip(vals, valid)]
            key_valid = rng.random(n) >= null_rate
            int_keys = rng.integers(-3, 40, size=n)
            codes = rng.integers(0, len(words), size=n)
            for keys, table in ((int_keys, None), (codes, words)):
                groups = [(int(k) if table is None else table[k]) if m else None for k, m in zip(keys, key_valid)]
                want = ex.walk(listed, groups, max_value_bytes=max_bytes, is_float=is_float)
                got = ex.walk_np(vals, valid, keys, key_valid, words=table, max_value_bytes=max_bytes)
                assert list(got["entries"]) == list(want["entries"]), (n, is_float, max_bytes)
                assert repr(sorted(got.items())) == repr(sorted(want.items())), (n, is_float, max_bytes)  # (repr: a NaN sum is a NaN sum)
                if n == 3000 and max_bytes == 9 and table is not None:
                    assert want["long_rows"][0] > 0 and want["null_group"][0] > 0 and want["groups"] > 10
                # rules=True: the two classes it adds and every overflow-rule decision, from the plain lists
                full = ex.walk_np(vals, valid, keys, key_valid, words=table, max_value_bytes=max_bytes, rules=True)
                assert repr(sorted((k, v) for k, v in full.items() if k in want)) == repr(sorted(want.items()))
                if not is_float:
                    assert "rules" not in full and "all" not in full
                    continue
                by_key, nulls, longs = ex.group_by(listed, groups), [], []
                for key, (_rows, values_of) in by_key.items():
                    if key is None:
                        nulls += values_of
                    elif isinstance(key, bytes) and len(key) > max_bytes:
                        longs += values_of
                in_entries = [v for key in want["entries"] for v in by_key[key][1]]
                lists = dict({key: by_key[key][1] for key in want["entries"]}, null_group=nulls, long_rows=longs,
                             counted_class=in_entries, all=[v for v in listed if v is not None])
                assert repr(full["all"]) == repr(ex.float_class(n, lists["all"])), (n, max_bytes)
                assert repr(full["counted_class"]) == repr(ex.float_class(want["counted"][0], in_entries)), (n, max_bytes)
                expected = {}
                for name, values_of in lists.items():
                    if not math.isfinite(ex.magnitudes_of(values_of)):
                        expected[name] = ex.float_rule(values_of)
                assert repr(sorted(full["rules"].items(), key=repr)) == repr(sorted(expected.items(), key=repr)), (n, max_bytes)
                if n == 3000:  # the rule decides entries and classes here, and every kind of decision is met
                    assert {"all", "counted_class"} <= set(expected) and len(expected) > 4
                met |= {how for how, _ in expected.values()}
    assert met == {"is", "unpinned"}


def test_the_overflow_rule():
    nan, inf, big = math.nan, math.inf, 1e308
    assert ex.float_rule([1.0, -2.5]) == ("bound", None) and ex.float_rule([]) == ("bound", None)
    assert ex.float_rule([big]) == ("bound", None)
    how, value = ex.float_rule([1.0, nan, inf])
    assert how == "is" and math.isnan(value)
    assert ex.float_rule([inf, 1.0, inf]) == ("is", inf) and ex.float_rule([-inf, big]) == ("is", -inf)
    how, value = ex.float_rule([inf, -inf])
    assert how == "is" and math.isnan(value)
    assert ex.float_rule([big, big]) == ("unpinned", None)  # 2e308: inf in every order, yet
    assert ex.float_rule([big, big, -big]) == ("unpinned", None)  # 1e308 in one order and inf in another
    assert ex.float_rule([inf, big, big]) == ("unpinned", None)  # (-inf from the finite ones would meet +inf as NaN)
    # the failure texts: a sum within the bound, one off by twice the bound, the rules
    c = ex.float_class(3, [0.1, 0.2, 0.3])
    bound = ex.float_bound(c[1], c[2], c[3])
    assert ex.float_failure(0.1 + 0.2 + 0.3, ("bound", None), *c[1:]) is None
    assert ex.float_failure(c[2] + 2 * bound, ("bound", None), *c[1:]) is not None
    assert ex.float_failure(nan, ("bound", None), *c[1:]) is not None
    assert ex.float_failure(inf, ("is", inf), 1, inf, inf) is None and ex.float_failure(nan, ("is", inf), 1, inf, inf)
    assert ex.float_failure(nan, ("is", nan), 1, nan, nan) is None and ex.float_failure(0.0, ("is", nan), 1, nan, nan)
    assert ex.float_failure(-inf, ("unpinned", None), 2, nan, inf) is None
