#!/usr/bin/env python3
"""TGX_CHECK_TYPE_CLASSES beside its yardsticks on the same column, each in a plan of its own in one process:

    LENGTH (1 .. 64 characters), a one-pattern REGEX_MATCH (^[0-9]+$) and VALUE_COUNTS (10000 values of up to 256 bytes)

over --rows rows in one DEVICE batch, no NULLs, on six columns:

    short integer text (6 digits, Utf8)      the reference's golden mix, cycled (Utf8)      18-digit doubles (Utf8)
    40 bytes of free text (LargeUtf8)        6-digit text as a Utf8View (inline values)     a dictionary of 1000 entries

The random columns draw their rows from pools of 4096 values, so that VALUE_COUNTS, the yardstick, stays within its
bounds; the classifier does not care.  Kernel times are HIP-event times on the state's stream (tgx_profile_get), the median of --steps steps after one warm-up
step of every shape.  No time is fixed in advance: every figure is reported with its ratio to each yardstick from the
same run, and goes into DESIGN.md.
    python tools/bench_type_classes.py [--rows 100000000] [--steps 5] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GOLDEN = ["123", "456.78", "true", "2023-01-01", "hello", "789", "false", "3.14", "world", "0"]
GOLDEN_COUNTS = {"integer_rows": 2, "double_rows": 2, "boolean_rows": 3, "date_rows": 1, "string_rows": 2}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import term_amd as T
    from term_amd._lib import spec

    n = args.rows // 1000 * 1000
    T.init(flags=T.OPT_NO_COALESCE)
    out = {"rows": n}
    lines = []
    gen = torch.Generator(device="cuda").manual_seed(0x7E570021)
    pad = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def drawn(pool):
        """n rows drawn from the pool's 4096 values (VALUE_COUNTS, the yardstick, stays within its bounds)"""
        pick = torch.randint(0, pool.shape[0], (n,), dtype=torch.int64, device="cuda", generator=gen)
        return pool[pick]

    def digits_text(width):
        """(n, width) ASCII digits, the first one 1 .. 9"""
        d = torch.randint(48, 58, (4096, width), dtype=torch.uint8, device="cuda", generator=gen)
        d[:, 0] = torch.randint(49, 58, (4096,), dtype=torch.uint8, device="cuda", generator=gen)
        return drawn(d)

    def fixed_width(data2d, large=False):
        width = data2d.shape[1]
        offsets = torch.arange(n + 1, dtype=torch.int64 if large else torch.int32, device="cuda") * width
        return T.Column(T.LARGE_UTF8 if large else T.UTF8, n, offsets=offsets, data=torch.cat([data2d.reshape(-1), pad]),
                        mem=T.MEM_DEVICE)

    def run(name, col, expect):
        plan = T.Plan([spec(T.TYPE_CLASSES, 0)])
        ours = timed(T, plan, [col], "type_classes", args.steps)
        got = ours[0].type_classes(0)
        assert got["seen"] == got["non_null"] == n, got
        for k, v in expect.items():
            assert got[k] == v, (name, k, got)
        row = {"type_classes_ms": ours[1], "type_classes_min_ms": ours[2], "counts": got}
        line = "%-22s type_classes %8.3f ms" % (name, ours[1])
        yards = (("length", [spec(T.LENGTH, 0, length_min=1, length_max=64)], "regex"),
                 ("regex_match", [spec(T.REGEX_MATCH, 0, pattern=r"^[0-9]+$")], "regex"),
                 ("value_counts", [spec(T.VALUE_COUNTS, 0)], "value_counts"))
        for yard_name, specs, kernel in yards:
            yplan = T.Plan(specs)
            if yard_name == "value_counts":
                yplan.set_value_counts(0, 10000, 256)
            yard = timed(T, yplan, [col], kernel, args.steps)
            row[yard_name + "_ms"], row["ratio_to_" + yard_name] = yard[1], ours[1] / yard[1]
            line += " | %s %8.3f ms (ratio %.2f)" % (yard_name, yard[1], ours[1] / yard[1])
            del yard, yplan
        out[name] = row
        lines.append(line)
        print(line, flush=True)

    # short integer text; the same as inline views
    six = digits_text(6)
    run("integer_text_utf8", fixed_width(six), {"integer_rows": n})
    views = torch.zeros((n, 16), dtype=torch.uint8, device="cuda")
    views[:, 0] = 6
    views[:, 4:10] = six
    run("integer_text_utf8_view", T.Column(T.UTF8_VIEW, n, values=views, mem=T.MEM_DEVICE, variadic=[]), {"integer_rows": n})
    del views, six
    torch.cuda.empty_cache()

    # the golden mix, cycled
    cycle = "".join(GOLDEN).encode()
    lens = torch.tensor([len(g) for g in GOLDEN], dtype=torch.int32, device="cuda").repeat(n // 10)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    offsets[1:] = torch.cumsum(lens, 0, dtype=torch.int32)
    data = torch.tensor(list(cycle), dtype=torch.uint8, device="cuda").repeat(n // 10)
    run("golden_mix_utf8", T.Column(T.UTF8, n, offsets=offsets, data=torch.cat([data, pad]), mem=T.MEM_DEVICE),
        {k: v * (n // 10) for k, v in GOLDEN_COUNTS.items()})
    del lens, offsets, data
    torch.cuda.empty_cache()

    # 18-digit doubles (beyond Int32: every value is read to its end)
    run("double_18_digits_utf8", fixed_width(digits_text(18)), {"double_rows": n})
    torch.cuda.empty_cache()

    # 40 bytes of free text: decided from the first byte
    text = torch.randint(97, 123, (4096, 40), dtype=torch.uint8, device="cuda", generator=gen)  # a .. z
    text[:, 0] = torch.randint(111, 115, (4096,), dtype=torch.uint8, device="cuda", generator=gen)  # o .. r: no grammar's start
    text = drawn(text)
    run("free_text_40_large_utf8", fixed_width(text, large=True), {"string_rows": n})
    del text
    torch.cuda.empty_cache()

    # a dictionary of 1000 entries: the golden mix, a hundred times
    entries = GOLDEN * 100
    ebytes = "".join(entries).encode()
    eoffs = [0]
    for e in entries:
        eoffs.append(eoffs[-1] + len(e))
    dictionary = T.Column(T.UTF8, len(entries), offsets=torch.tensor(eoffs, dtype=torch.int32, device="cuda"),
                          data=torch.cat([torch.tensor(list(ebytes), dtype=torch.uint8, device="cuda"), pad]), mem=T.MEM_DEVICE)
    idx = (torch.arange(n, dtype=torch.int32, device="cuda") * 7) % len(entries)  # every entry equally often
    run("golden_mix_dictionary", T.Column(T.DICT32_UTF8, n, values=idx, dictionary=dictionary, mem=T.MEM_DEVICE),
        {k: v * (n // 10) for k, v in GOLDEN_COUNTS.items()})

    print("%d rows" % n)
    for line in lines:
        print(line)
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
