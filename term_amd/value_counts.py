"""What HistogramConstraint and EntropyAnalyzer derive from a column's value counts (TG/constraints/histogram.rs:37-127,
TG/analyzers/advanced/entropy.rs:95-190), over what State.value_counts reads from a TGX_CHECK_VALUE_COUNTS spec.

    summary, counts = state.value_counts(spec_index)
    hist = Histogram.from_counts(summary, counts, max_distinct)      # raises OutOfBound beyond the bounds
    hist.most_common_ratio(), hist.bucket_count(), hist.entropy(), ...
    es = EntropyState.from_counts(summary, counts, max_unique_values)
    es.metrics()

Value text is the string itself, or the decimal text of an integer.  Buckets are ordered by count descending, then by
the value's TEXT ascending (the reference's SQL orders CAST(col AS VARCHAR)); ratio = count / (total - nulls).  Sums are
taken with math.fsum: a left-to-right sum of a Gini figure loses the small terms behind a dominant one (1000 values,
one of them 10^9 times the others: 9.5e-16 off, twice the tolerance the tests hold these figures to).

Beyond the bounds nothing is approximated: distinct > max_distinct, overflow_rows > 0 or long_rows > 0 raise OutOfBound
with the numbers in it.  The reference's truncated top-N sampling is not reproduced."""
import json
import math


class OutOfBound(ValueError):
    pass


def value_text(v):
    if not isinstance(v, (bytes, bytearray)):
        return str(int(v))
    try:
        return v.decode("utf-8")
    except UnicodeDecodeError:
        raise OutOfBound("a value is not UTF-8 (%r): a binary column has no value text, not on the GPU path" % bytes(v[:16]))


def _check_bounds(what, summary, max_distinct):
    if summary["distinct"] > max_distinct or summary["overflow_rows"] or summary["long_rows"]:
        raise OutOfBound("%s: the column is beyond the bounds of its value counts: %d distinct values (max_distinct %d), "
                         "%d overflow rows, %d rows longer than max_value_bytes"
                         % (what, summary["distinct"], max_distinct, summary["overflow_rows"], summary["long_rows"]))


class HistogramBucket:
    def __init__(self, value, count, ratio):
        self.value, self.count, self.ratio = value, count, ratio

    def __repr__(self):
        return "HistogramBucket(%r, %d, %r)" % (self.value, self.count, self.ratio)


class Histogram:
    """histogram.rs:24-127"""

    def __init__(self, buckets, total_count, null_count):
        self.buckets, self.total_count, self.null_count = list(buckets), total_count, null_count
        self.distinct_count = len(self.buckets)

    @staticmethod
    def from_counts(summary, counts, max_distinct=10000):
        _check_bounds("histogram", summary, max_distinct)
        denominator = summary["non_null"]  # total - nulls
        rows = sorted(((value_text(v), c) for v, c in counts.items()), key=lambda tc: (-tc[1], tc[0]))
        return Histogram([HistogramBucket(t, c, c / denominator) for t, c in rows], summary["seen"],
                         summary["seen"] - summary["non_null"])

    def most_common_ratio(self): return self.buckets[0].ratio if self.buckets else 0.0
    def least_common_ratio(self): return self.buckets[-1].ratio if self.buckets else 0.0
    def bucket_count(self): return len(self.buckets)
    def top_n(self, n): return [(b.value, b.ratio) for b in self.buckets[:n]]
    def top_n_ratio(self, n): return math.fsum(b.ratio for b in self.buckets[:n])
    def follows_power_law(self, top_n, threshold): return self.top_n_ratio(top_n) >= threshold
    def null_ratio(self): return 0.0 if self.total_count == 0 else self.null_count / self.total_count

    def is_roughly_uniform(self, threshold=1.5):
        if not self.buckets:
            return True
        lo = self.least_common_ratio()
        return False if lo == 0.0 else self.most_common_ratio() / lo <= threshold

    def get_value_ratio(self, value):
        for b in self.buckets:
            if b.value == value:
                return b.ratio
        return None

    def entropy(self):
        """in nats (histogram.rs:103-109)"""
        return math.fsum(-b.ratio * math.log(b.ratio) for b in self.buckets if b.ratio > 0.0)

    def failure_message(self, column, assertion_description="custom assertion"):
        """histogram.rs:372-383"""
        return ("Histogram assertion '%s' failed for column '%s'. Distribution: %d distinct values, most common ratio: "
                "%.2f%%, null ratio: %.2f%%" % (assertion_description, column, self.distinct_count,
                                              self.most_common_ratio() * 100.0, self.null_ratio() * 100.0))


class EntropyState:
    """entropy.rs:84-190: {value_counts, total_count, truncated}; truncated is always False here (beyond the bound the
    state is not built at all)"""

    def __init__(self, value_counts, total_count, truncated=False):
        self.value_counts, self.total_count, self.truncated = dict(value_counts), int(total_count), bool(truncated)

    @staticmethod
    def from_counts(summary, counts, max_unique_values=10000):
        _check_bounds("entropy", summary, max_unique_values)
        return EntropyState({value_text(v): c for v, c in counts.items()}, summary["counted"])

    def entropy(self):
        """Shannon entropy in bits"""
        if self.total_count == 0:
            return 0.0
        t = float(self.total_count)
        return math.fsum(-(c / t) * math.log2(c / t) for c in self.value_counts.values() if c / t > 0.0)

    def normalized_entropy(self):
        n = len(self.value_counts)
        return 0.0 if n <= 1 else self.entropy() / math.log2(float(n))

    def gini_impurity(self):
        if self.total_count == 0:
            return 0.0
        t = float(self.total_count)
        return math.fsum([1.0] + [-(c / t) * (c / t) for c in self.value_counts.values()])

    def effective_values(self): return 2.0 ** self.entropy()
    def is_empty(self): return self.total_count == 0

    def probability_distribution(self):
        return {v: c / float(self.total_count) for v, c in self.value_counts.items()}

    @staticmethod
    def merge(states):
        counts, total, truncated = {}, 0, False
        for s in states:
            total += s.total_count
            truncated |= s.truncated
            for v, c in s.value_counts.items():
                counts[v] = counts.get(v, 0) + c
        return EntropyState(counts, total, truncated)

    def metrics(self):
        """the metric map of entropy.rs:337-395 (top_values: at most 100 values, the 10 most frequent; ties by text)"""
        m = {"entropy": self.entropy(), "normalized_entropy": self.normalized_entropy(),
             "gini_impurity": self.gini_impurity(), "effective_values": self.effective_values(),
             "unique_values": len(self.value_counts), "total_count": self.total_count, "truncated": self.truncated}
        if len(self.value_counts) <= 100:
            top = sorted(self.value_counts.items(), key=lambda vc: (-vc[1], vc[0]))[:10]
            m["top_values"] = {v: {"count": c, "probability": c / float(self.total_count)} for v, c in top}
        return m

    def to_json(self):
        """serde's form of EntropyState: integers as integer tokens"""
        return json.dumps({"value_counts": self.value_counts, "total_count": self.total_count, "truncated": self.truncated},
                          sort_keys=True, ensure_ascii=False)

    @staticmethod
    def from_json(text):
        d = json.loads(text)
        if not all(isinstance(c, int) and not isinstance(c, bool) and c >= 0 for c in d["value_counts"].values()) \
                or not isinstance(d["total_count"], int) or not isinstance(d["truncated"], bool):
            raise ValueError("EntropyState: value_counts and total_count are integers, truncated is a boolean")
        return EntropyState(d["value_counts"], d["total_count"], d["truncated"])
