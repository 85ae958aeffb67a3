"""The reference of the TYPE_CLASSES tests is itself held to account (no device, no library): the byte-level classifier
and its `re` / `datetime` twin agree on the hand-listed edge table -- whose expected classes are written out -- and on
20 000 seeded strings, and the golden column of the reference's own test gets the contract's answer."""
import json
import os

import exact_type_classes as ex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_type_vectors.json")
with open(GOLDEN) as _f:
    G = json.load(_f)

SEEDED = ex.seeded_strings(20000)


def test_the_edge_table_has_the_classes_written_beside_it():
    assert len(ex.EDGES) == len({v for v, _ in ex.EDGES})  # no value twice
    wrong = [(v[:40], ex.NAMES[want], ex.NAMES[ex.classify(v)]) for v, want in ex.EDGES if ex.classify(v) != want]
    assert not wrong, wrong
    assert {want for _, want in ex.EDGES} == set(range(7))  # every class is met


def test_the_twin_agrees_on_the_edge_table():
    wrong = [(v[:40], ex.NAMES[ex.classify(v)], ex.NAMES[ex.classify_re(v)]) for v, _ in ex.EDGES
             if ex.classify(v) != ex.classify_re(v)]
    assert not wrong, wrong


def test_the_twin_agrees_on_seeded_strings():
    assert len(SEEDED) >= 20000
    wrong = [(v, ex.NAMES[ex.classify(v)], ex.NAMES[ex.classify_re(v)]) for v in SEEDED if ex.classify(v) != ex.classify_re(v)]
    assert not wrong, wrong[:10]
    met = {ex.classify(v) for v in SEEDED}
    assert met == set(range(7)), met  # the alphabet reaches every class


def test_the_issue_minimum_edge_list_is_in_the_table():
    listed = {v for v, _ in ex.EDGES}
    for text in ("0 1 2 -1 -0 +5 007 2147483647 2147483648 -2147483648 -2147483649 true TRUE tRuE yes t "
                 "1. .5 . 1e 1e5 1E+5 e5 +.5e-3 nan -NaN +inf Infinity infinit 1_0 0x10 "
                 "2023-01-01 2023-1-5 2023-02-29 2024-02-29 1900-02-29 2000-02-29 0000-02-29 2023-13-01 2023-00-10 2023-1- "
                 "2023-01-01T00:00:00 2023-01-01T24:00:00 2023-01-01T10:00 2023-01-01T10:00:00+05:30 "
                 "2023-01-01T10:00:00+0530 2023-01-01X +10999-12-31 5551-234 1234 12-34").split():
        assert text.encode() in listed, text
    for v in (b"truE ", "falſe".encode(), b"2023-01-01 23:59:59.123456789Z", b"", b"7" * 4096):
        assert v in listed, v


def test_counts_hold_the_identities():
    values = [v for v, _ in ex.EDGES] + [None] * 7
    c = ex.counts(values)
    assert c["seen"] == len(values) and c["seen"] == c["non_null"] + 7
    assert c["non_null"] == sum(c[n + "_rows"] for n in ex.NAMES)
    assert ex.add(c, c)["undecided_rows"] == 2 * c["undecided_rows"] > 0


def test_the_golden_column():
    g = G["mixed_type"]
    got = [ex.NAMES[ex.classify(v.encode())] for v in g["values"]]
    assert got == g["classes"]
    tally = {}
    for name in got:
        tally[name] = tally.get(name, 0) + 1
    assert tally == g["contract"]["type_counts"] and len(got) == g["contract"]["total_count"] == g["reference_asserts"]["total_count"]
    assert set(g["reference_asserts"]["keys_present"]) <= set(tally)
