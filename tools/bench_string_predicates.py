#!/usr/bin/env python3
"""The string leaves of TGX_CHECK_ROW_PREDICATE (STR_LENGTH, STR_LIKE, STR_BLANK, STR_CMP) beside their yardsticks, each
over the same column in one process:

    OCTET_LENGTH(s) <= n, LENGTH(s) >= n                       the LENGTH check kind on that column
    s LIKE 'ab%' / '%ab' / '%ab%' / '%a_b%c'                   a one-pattern REGEX_MATCH of the same meaning, and STR_EQ
    TRIM(s) <> '', s <= '1998-09-01'                           STR_EQ (the leaf that reads the same bytes)

on short ids (8 bytes, Utf8) and 40-byte emails (LargeUtf8: 100 M of them pass 2^31 bytes), and the short ids again as a
Utf8View and as a dictionary column.  One DEVICE batch of --rows rows, no NULLs.  The predicates are compiled from their text by the
library's compiler under the dialect string_functions.  Kernel times are HIP-event times on the state's stream
(tgx_profile_get), the median of --steps steps after one warm-up step of every shape.  There is no gate: every figure is
reported beside its yardstick from the same run, as a ratio, and goes into DESIGN.md.
    python tools/bench_string_predicates.py [--rows 100000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(T, plan, cols, kernel, steps):
    st = T.State(plan)
    st.profile_enable(True)
    times = []
    for it in range(steps + 1):
        st.reset()
        st.profile_reset()
        st.update(cols)
        st.finalize()
        if it:  # (step 0 warms the shape up)
            times.append(st.profile_get(kernel)["total_ms"])
    return st, statistics.median(times), min(times)


def predicate_plan(T, S, spec, expression):
    """a one-spec plan of `expression` over a table of the one column it names"""
    c = S.row_predicate(expression, string_functions=True)
    plan = T.Plan([spec(T.ROW_PREDICATE, 0, columns=[0])])
    leaves = [dict((k, v) for k, v in leaf.items() if k != "lit_f_bits") for leaf in c["leaves"]]
    plan.set_row_predicate(0, leaves, [tuple(p) for p in c["program"]], bytes.fromhex(c["literals_hex"]))
    return plan


PREDICATES = [  # (name, expression, the regex of the same meaning or None)
    ("octet_length_le", "OCTET_LENGTH(s) <= 20", None),
    ("length_ge", "LENGTH(s) >= 5", None),
    ("like_prefix", "s LIKE 'ab%'", "^ab"),
    ("like_suffix", "s LIKE '%ab'", "ab$"),
    ("like_infix", "s LIKE '%ab%'", "ab"),
    ("like_a_b_c", "s LIKE '%a_b%c'", "a.b.*c$"),  # (no line feed in the data: `.` and `_` agree)
    ("trim_not_blank", "TRIM(s) <> ''", None),
    ("order_le_date", "s <= '1998-09-01'", None),
    ("str_eq", "s = 'abababab'", None),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import term_amd as T
    import term_amd.suite as S
    from term_amd._lib import spec

    n = args.rows // 64 * 64
    T.init(flags=T.OPT_NO_COALESCE)
    out = {"rows": n}
    lines = []
    gen = torch.Generator(device="cuda").manual_seed(0x57210021)
    pad = torch.zeros(64, dtype=torch.uint8, device="cuda")
    alphabet = torch.tensor(list(b"abc 19-@."), dtype=torch.uint8, device="cuda")

    def fixed_width(width, offset_type=torch.int32):
        """n values of `width` bytes over a small alphabet, as a Utf8 / LargeUtf8 column's two buffers"""
        data = torch.empty(n * width, dtype=torch.uint8, device="cuda")
        chunk = 1 << 26  # (the index tensor is int64: drawn a chunk at a time)
        for lo in range(0, n * width, chunk):
            m = min(chunk, n * width - lo)
            data[lo:lo + m] = alphabet[torch.randint(0, len(alphabet), (m,), dtype=torch.int64, device="cuda", generator=gen)]
        offsets = torch.arange(n + 1, dtype=offset_type, device="cuda") * width
        return offsets, data

    def run(column_name, col, n_bytes):
        torch.cuda.synchronize()  # (the column was written on torch's stream; the library reads it on its own)
        yard_len = None
        for name, expression, regex in PREDICATES:
            ours = timed(T, predicate_plan(T, S, spec, expression), [col], "row_predicate", args.steps)
            seen, sat, unk, failed = ours[0].row_predicate_counts(0)
            assert seen == n and unk == 0
            if name in ("octet_length_le", "length_ge"):  # (every value has n_bytes ASCII bytes)
                assert sat == (n if (n_bytes <= 20 if name == "octet_length_le" else n_bytes >= 5) else 0), (name, sat)
            entry = {"expression": expression, "row_predicate_ms": ours[1], "row_predicate_min_ms": ours[2], "satisfied": sat,
                     "rows_per_s": n / (ours[1] * 1e-3)}
            line = "%-17s %-16s row_predicate %8.3f ms (%5.1f G rows/s, %d satisfied)" % (column_name, name, ours[1],
                                                                                         n / ours[1] * 1e-6, sat)
            if name in ("octet_length_le", "length_ge"):
                if yard_len is None:
                    # (the LENGTH kind counts characters, like LENGTH(s) >= 5; it runs under the pattern kernels' name)
                    try:
                        yard_len = timed(T, T.Plan([spec(T.LENGTH, 0, length_min=5)]), [col], "regex", args.steps)
                    except T.TgxError as e:
                        yard_len = e
                if isinstance(yard_len, Exception):
                    entry.update(length_error=str(yard_len))
                    line += " | LENGTH not measured: %s" % yard_len
                else:
                    entry.update(length_ms=yard_len[1], ratio_to_length=ours[1] / yard_len[1])
                    line += " | LENGTH %8.3f ms | ratio %.2f" % (yard_len[1], ours[1] / yard_len[1])
            if regex is not None:
                try:
                    yard = timed(T, T.Plan([spec(T.REGEX_MATCH, 0, pattern=regex)]), [col], "regex", args.steps)
                except T.TgxError as e:  # (a layout the pattern kernels do not take: said, not hidden)
                    entry.update(regex=regex, regex_error=str(e))
                    line += " | REGEX_MATCH not measured: %s" % e
                else:
                    matches = yard[0].finalize()[0].matches
                    assert matches == sat, (name, matches, sat)
                    entry.update(regex=regex, regex_ms=yard[1], ratio_to_regex=ours[1] / yard[1])
                    line += " | REGEX_MATCH %8.3f ms | ratio %.2f" % (yard[1], ours[1] / yard[1])
            out.setdefault(column_name, {"value_bytes": n_bytes})[name] = entry
            lines.append(line)
        eq = out[column_name]["str_eq"]["row_predicate_ms"]
        for name, _, _ in PREDICATES:
            out[column_name][name]["ratio_to_str_eq"] = out[column_name][name]["row_predicate_ms"] / eq

    # short ids: 8 bytes a value; the same values as Utf8, Utf8View (inline) and a dictionary column
    offsets, data = fixed_width(8)
    run("utf8_ids", T.Column(T.UTF8, n, offsets=offsets, data=torch.cat([data, pad]), mem=T.MEM_DEVICE), 8)
    views = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    views[:, 0] = 8
    views[:, 1:3] = data.view(torch.int32).view(n, 2)
    run("utf8_view_ids", T.Column(T.UTF8_VIEW, n, values=views, mem=T.MEM_DEVICE, variadic=[]), 8)
    del views
    n_entries = 1 << 16
    entries = T.Column(T.UTF8, n_entries, offsets=offsets[:n_entries + 1].clone(), data=torch.cat([data[:n_entries * 8].clone(), pad]),
                       mem=T.MEM_DEVICE)
    indices = torch.randint(0, n_entries, (n,), dtype=torch.int32, device="cuda", generator=gen)
    del offsets, data
    torch.cuda.empty_cache()
    run("dictionary_ids", T.Column(T.DICT32_UTF8, n, values=indices, dictionary=entries, mem=T.MEM_DEVICE), 8)
    del indices, entries
    torch.cuda.empty_cache()
    # emails: 40 bytes a value (beyond 2^31 bytes at 100 M rows: 64-bit offsets, a LargeUtf8 column)
    offsets, data = fixed_width(40, torch.int64)
    run("large_utf8_emails", T.Column(T.LARGE_UTF8, n, offsets=offsets, data=torch.cat([data, pad]), mem=T.MEM_DEVICE), 40)

    print("%d rows" % n)
    for line in lines:
        print(line)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
