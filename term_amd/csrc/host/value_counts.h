// value_counts.h -- HistogramConstraint (TG/constraints/histogram.rs) and what EntropyAnalyzer
// (TG/analyzers/advanced/entropy.rs; the analyzer itself is in analyzers.cpp) share with it, over
// TGX_CHECK_VALUE_COUNTS: the `GROUP BY col` count of one column, read from the device.
//
// Value text is the string itself, or the decimal text of an integer column.  A column whose declared Arrow type is a
// date, time, timestamp, duration, float, decimal or boolean is the constraint's / analyzer's own error ("... not on the
// GPU path": its CAST(col AS VARCHAR) text is not reproduced).  Beyond the bounds nothing is approximated:
// distinct > max_distinct, overflow_rows > 0 or long_rows > 0 is an error with the numbers in it; the reference's
// truncated top-N sampling (entropy.rs:229-262) is not reproduced.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "json.h"
#include "term_guard.h"

namespace term_guard {

// one spec's state as tgx_value_counts_get / tgx_value_counts_entries answer it, the values as text, ascending by value
struct ValueCounts {
  tgx_value_counts_summary summary = {};
  std::vector<std::pair<std::string, uint64_t>> entries;
};
ValueCounts read_value_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index);  // throws TermError (Internal)
SpecRequest value_counts_request(const std::string &column, uint64_t max_distinct);
// "" when a column of this declared Arrow type has a value text the device reproduces, else what is wrong with it
std::string value_text_refusal(const std::string &column, const std::string &arrow_type);
// "" within the bounds, else the error's text
std::string value_counts_out_of_bound(const ValueCounts &vc, uint64_t max_distinct);
// sums as the verdict layer takes them: compensated (Neumaier), so that a dominant term does not swallow the others
double compensated_sum(const std::vector<double> &terms);

// ---- histogram.rs:11-127
struct ValueBucket {  // HistogramBucket there (analyzers.h has the numeric analyzer's bucket of that name)
  std::string value;
  int64_t count = 0;
  double ratio = 0;
};
class Histogram {
 public:
  std::vector<ValueBucket> buckets;  // by count descending, then by the value's text ascending (the SQL's ORDER BY)
  int64_t total_count = 0;
  size_t distinct_count = 0;
  int64_t null_count = 0;
  Histogram(std::vector<ValueBucket> b, int64_t total, int64_t nulls)
      : buckets(std::move(b)), total_count(total), distinct_count(buckets.size()), null_count(nulls) {}
  // ratio = count / (total - nulls), as the SQL's `vc.count * 1.0 / (t.total_cnt - t.null_cnt)`
  static Histogram from_counts(const ValueCounts &vc);
  double most_common_ratio() const { return buckets.empty() ? 0.0 : buckets.front().ratio; }
  double least_common_ratio() const { return buckets.empty() ? 0.0 : buckets.back().ratio; }
  size_t bucket_count() const { return buckets.size(); }
  std::vector<std::pair<std::string, double>> top_n(size_t n) const;
  double top_n_ratio(size_t n) const;
  bool is_roughly_uniform(double threshold = 1.5) const;
  std::optional<double> get_value_ratio(const std::string &value) const;
  double entropy() const;  // nats
  bool follows_power_law(size_t top_n, double threshold) const { return top_n_ratio(top_n) >= threshold; }
  double null_ratio() const { return total_count == 0 ? 0.0 : (double)null_count / (double)total_count; }
};
typedef std::function<bool(const Histogram &)> HistogramAssertion;

// The JSON / Python form cannot carry a function: a conjunction of named measures, each held to an Assertion.
//   most_common_ratio, least_common_ratio, bucket_count, entropy, null_ratio, top_n_ratio {n}, value_ratio {value}
// (value_ratio of a value the histogram does not hold is 0.0, as `get_value_ratio(v).unwrap_or(0.0)`)
struct HistogramMeasure {
  std::string measure;
  Assertion assertion = Assertion::equals(0);
  size_t n = 0;       // top_n_ratio
  std::string value;  // value_ratio
};
double histogram_measure(const Histogram &h, const HistogramMeasure &m);  // throws TermError for an unknown measure
std::string histogram_measures_description(const std::vector<HistogramMeasure> &measures);

class HistogramConstraint : public Constraint {  // histogram.rs:154-410
 public:
  static constexpr uint64_t kDefaultMaxDistinct = 10000;
  HistogramConstraint(std::string column, HistogramAssertion assertion, std::string description = "custom assertion",
                      uint64_t max_distinct = kDefaultMaxDistinct)
      : column_(std::move(column)), assertion_(std::move(assertion)), description_(std::move(description)),
        max_distinct_(max_distinct) {}
  // the JSON form: every measure must hold
  HistogramConstraint(std::string column, std::vector<HistogramMeasure> measures, std::optional<std::string> description,
                      uint64_t max_distinct = kDefaultMaxDistinct);
  std::string name() const override { return "histogram"; }
  std::optional<std::string> column() const override { return column_; }
  std::string description() const;  // metadata().description (:401-406)
  std::vector<SpecRequest> plan() const override;
  ConstraintResult evaluate(const Inputs &in) const override;

 private:
  std::string column_;
  HistogramAssertion assertion_;
  std::string description_;
  uint64_t max_distinct_;
};

// ---- entropy.rs:84-190, on the state's serde form {"value_counts": {text: count}, "total_count", "truncated"}
json::Value entropy_state(const ValueCounts &vc);
json::Value entropy_merge(const std::vector<json::Value> &states);
double entropy_bits(const json::Value &state);
double entropy_gini(const json::Value &state);

}  // namespace term_guard
