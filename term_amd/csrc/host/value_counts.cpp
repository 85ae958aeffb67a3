// value_counts.cpp -- see value_counts.h.  Reference: TG/constraints/histogram.rs, TG/analyzers/advanced/entropy.rs.
#include "value_counts.h"

#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>

namespace term_guard {

ValueCounts read_value_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index) {
  ValueCounts out;
  tgx_error err;
  memset(&err, 0, sizeof(err));
  auto check = [&](tgx_status s) {
    if (s != TGX_OK) throw TermError{TermError::Internal, std::string(tgx_status_name(s)) + ": " + err.msg};
  };
  check(tgx_value_counts_get(plan, state, spec_index, &out.summary, &err));
  uint64_t n = 0, nb = 0;
  int32_t is_bytes = 0;
  check(tgx_value_counts_entries(plan, state, spec_index, nullptr, 0, &n, nullptr, 0, &nb, &is_bytes, &err));
  std::vector<tgx_value_count_entry> entries((size_t)n + 1);
  std::vector<uint8_t> bytes((size_t)nb + 1);
  check(tgx_value_counts_entries(plan, state, spec_index, entries.data(), n, &n, bytes.data(), nb, &nb, &is_bytes, &err));
  for (uint64_t i = 0; i < n; i++) {
    const tgx_value_count_entry &e = entries[i];
    out.entries.emplace_back(is_bytes ? std::string((const char *)bytes.data() + e.offset, (size_t)e.length)
                                      : std::to_string((long long)e.value),
                             e.count);
  }
  return out;
}

SpecRequest value_counts_request(const std::string &column, uint64_t max_distinct) {
  SpecRequest r;
  r.kind = TGX_CHECK_VALUE_COUNTS;
  r.column = column;
  tgx_value_counts_params p;
  // (a bound outside the device's range is the device's refusal, with its text)
  p.max_distinct = (uint32_t)std::min<uint64_t>(max_distinct, UINT32_MAX);
  p.max_value_bytes = TGX_VALUE_COUNTS_MAX_VALUE_BYTES;
  r.value_counts = p;
  return r;
}

std::string value_text_refusal(const std::string &column, const std::string &arrow_type) {
  // (by prefix, in either letter case: "Timestamp(Nanosecond, None)", "time32[s]", "decimal128(10, 2)", "LargeBinary")
  static const char *const kinds[] = {"date", "time", "duration", "float", "decimal", "bool", "interval",
                                      "binary", "largebinary", "fixedsizebinary"};
  std::string lower;
  for (char ch : arrow_type) lower += (char)tolower((unsigned char)ch);
  for (const char *k : kinds)  // ("time" covers Time32 / Time64 / Timestamp)
    if (lower.compare(0, strlen(k), k) == 0)
      return "the value text of column '" + column + "' (" + arrow_type +
             ") is CAST(col AS VARCHAR) of a date, time, timestamp, duration, float, decimal, boolean or binary value: "
             "not on the GPU path";
  return std::string();
}

std::string value_counts_out_of_bound(const ValueCounts &vc, uint64_t max_distinct) {
  const tgx_value_counts_summary &s = vc.summary;
  if (s.distinct <= max_distinct && s.overflow_rows == 0 && s.long_rows == 0) return std::string();
  char buf[256];
  snprintf(buf, sizeof(buf),
           "the column is beyond the bounds of its value counts: %llu distinct values (max_distinct %llu), %llu overflow "
           "rows, %llu rows longer than %d bytes",
           (unsigned long long)s.distinct, (unsigned long long)max_distinct, (unsigned long long)s.overflow_rows,
           (unsigned long long)s.long_rows, (int)TGX_VALUE_COUNTS_MAX_VALUE_BYTES);
  return buf;
}

double compensated_sum(const std::vector<double> &terms) {
  double sum = 0.0, comp = 0.0;
  for (double x : terms) {
    const double t = sum + x;
    comp += fabs(sum) >= fabs(x) ? (sum - t) + x : (x - t) + sum;
    sum = t;
  }
  return sum + comp;
}

// ---- Histogram
Histogram Histogram::from_counts(const ValueCounts &vc) {
  std::vector<ValueBucket> b;
  const double denominator = (double)vc.summary.non_null;  // total - nulls
  for (const auto &e : vc.entries) b.push_back({e.first, (int64_t)e.second, (double)e.second * 1.0 / denominator});
  std::sort(b.begin(), b.end(), [](const ValueBucket &x, const ValueBucket &y) {
    return x.count != y.count ? x.count > y.count : x.value < y.value;  // (bytewise: UTF-8 order is code point order)
  });
  return Histogram(std::move(b), (int64_t)vc.summary.seen, (int64_t)(vc.summary.seen - vc.summary.non_null));
}

std::vector<std::pair<std::string, double>> Histogram::top_n(size_t n) const {
  std::vector<std::pair<std::string, double>> out;
  for (size_t i = 0; i < buckets.size() && i < n; i++) out.emplace_back(buckets[i].value, buckets[i].ratio);
  return out;
}

double Histogram::top_n_ratio(size_t n) const {
  std::vector<double> r;
  for (size_t i = 0; i < buckets.size() && i < n; i++) r.push_back(buckets[i].ratio);
  return compensated_sum(r);
}

bool Histogram::is_roughly_uniform(double threshold) const {
  if (buckets.empty()) return true;
  const double lo = least_common_ratio();
  return lo == 0.0 ? false : most_common_ratio() / lo <= threshold;
}

std::optional<double> Histogram::get_value_ratio(const std::string &value) const {
  for (const ValueBucket &b : buckets)
    if (b.value == value) return b.ratio;
  return std::nullopt;
}

double Histogram::entropy() const {
  std::vector<double> terms;
  for (const ValueBucket &b : buckets)
    if (b.ratio > 0.0) terms.push_back(-b.ratio * log(b.ratio));
  return compensated_sum(terms);
}

// ---- the named measures
double histogram_measure(const Histogram &h, const HistogramMeasure &m) {
  if (m.measure == "most_common_ratio") return h.most_common_ratio();
  if (m.measure == "least_common_ratio") return h.least_common_ratio();
  if (m.measure == "bucket_count") return (double)h.bucket_count();
  if (m.measure == "entropy") return h.entropy();
  if (m.measure == "null_ratio") return h.null_ratio();
  if (m.measure == "top_n_ratio") return h.top_n_ratio(m.n);
  if (m.measure == "value_ratio") return h.get_value_ratio(m.value).value_or(0.0);
  throw TermError{TermError::Configuration, "unknown histogram measure '" + m.measure + "'"};
}

static std::string measure_text(const HistogramMeasure &m) {
  if (m.measure == "top_n_ratio") return "top_n_ratio(" + std::to_string(m.n) + ")";
  if (m.measure == "value_ratio") return "value_ratio('" + m.value + "')";
  return m.measure;
}

std::string histogram_measures_description(const std::vector<HistogramMeasure> &measures) {
  std::string o;
  for (size_t i = 0; i < measures.size(); i++)
    o += (i ? " and " : "") + measure_text(measures[i]) + " " + measures[i].assertion.description();
  return o;
}

// ---- HistogramConstraint
HistogramConstraint::HistogramConstraint(std::string column, std::vector<HistogramMeasure> measures,
                                         std::optional<std::string> description, uint64_t max_distinct)
    : column_(std::move(column)), max_distinct_(max_distinct) {
  if (measures.empty()) throw TermError{TermError::Configuration, "a histogram constraint needs at least one measure"};
  for (const HistogramMeasure &m : measures) (void)histogram_measure(Histogram({}, 0, 0), m);  // (an unknown name throws)
  description_ = description ? *description : histogram_measures_description(measures);
  assertion_ = [measures](const Histogram &h) {
    for (const HistogramMeasure &m : measures)
      if (!m.assertion.evaluate(histogram_measure(h, m))) return false;
    return true;
  };
}

std::string HistogramConstraint::description() const {
  return "Analyzes value distribution in column '" + column_ + "' and applies assertion: " + description_;
}

std::vector<SpecRequest> HistogramConstraint::plan() const {
  if (auto e = validate_identifier(column_)) throw *e;
  return {value_counts_request(column_, max_distinct_)};
}

ConstraintResult HistogramConstraint::evaluate(const Inputs &in) const {
  const std::string refusal = value_text_refusal(column_, in.arrow_types.empty() ? std::string() : in.arrow_types[0]);
  if (!refusal.empty()) throw TermError{TermError::ConstraintEvaluation, "'histogram': " + refusal};
  if (!in.value_counts) throw TermError{TermError::Internal, "histogram: no value counts in this run"};
  ValueCounts vc;
  in.value_counts(in.ctx, 0, &vc);
  const std::string beyond = value_counts_out_of_bound(vc, max_distinct_);
  if (!beyond.empty()) throw TermError{TermError::ConstraintEvaluation, "'histogram': " + beyond};
  if (vc.entries.empty()) return ConstraintResult::skipped("No data to analyze");  // (the query returns no row)
  const Histogram h = Histogram::from_counts(vc);
  const double entropy = h.entropy();
  if (assertion_(h)) return ConstraintResult::success_with_metric(entropy);
  char pct[96];
  snprintf(pct, sizeof(pct), "most common ratio: %.2f%%, null ratio: %.2f%%", h.most_common_ratio() * 100.0,
           h.null_ratio() * 100.0);
  return ConstraintResult::failure_with_metric(
      entropy, "Histogram assertion '" + description_ + "' failed for column '" + column_ + "'. Distribution: " +
                   std::to_string(h.distinct_count) + " distinct values, " + pct);
}

Check::Builder &Check::Builder::has_histogram(std::string column, HistogramAssertion assertion) {
  return constraint(std::make_shared<HistogramConstraint>(std::move(column), std::move(assertion)));
}
Check::Builder &Check::Builder::has_histogram_with_description(std::string column, HistogramAssertion assertion,
                                                               std::string description) {
  return constraint(std::make_shared<HistogramConstraint>(std::move(column), std::move(assertion), std::move(description)));
}

// ---- EntropyState
json::Value entropy_state(const ValueCounts &vc) {
  json::Value counts;
  counts.type = json::Value::Object;
  uint64_t total = 0;
  for (const auto &e : vc.entries) {
    counts.obj.emplace_back(e.first, json::Value::of_u64(e.second));
    total += e.second;
  }
  std::sort(counts.obj.begin(), counts.obj.end(),
            [](const std::pair<std::string, json::Value> &a, const std::pair<std::string, json::Value> &b) { return a.first < b.first; });
  json::Value truncated;
  truncated.type = json::Value::Bool;
  truncated.b = false;
  json::Value st;
  st.type = json::Value::Object;
  st.obj = {{"value_counts", counts}, {"total_count", json::Value::of_u64(total)}, {"truncated", truncated}};
  return st;
}

json::Value entropy_merge(const std::vector<json::Value> &states) {  // entropy.rs:165-185
  std::map<std::string, uint64_t> merged;
  uint64_t total = 0;
  bool truncated = false;
  for (const json::Value &s : states) {
    total += s.get_u64("total_count", 0);
    truncated |= s.get_bool("truncated", false);
    if (const json::Value *vc = s.get("value_counts"))
      if (vc->is(json::Value::Object))
        for (const auto &kv : vc->obj) merged[kv.first] += kv.second.as_u64();
  }
  ValueCounts all;
  for (const auto &kv : merged) all.entries.emplace_back(kv.first, kv.second);
  json::Value st = entropy_state(all);
  for (auto &kv : st.obj) {
    if (kv.first == "total_count") kv.second = json::Value::of_u64(total);
    if (kv.first == "truncated") kv.second.b = truncated;
  }
  return st;
}

static std::vector<double> probabilities(const json::Value &state) {
  std::vector<double> p;
  const double total = (double)state.get_u64("total_count", 0);
  if (const json::Value *vc = state.get("value_counts"))
    if (vc->is(json::Value::Object))
      for (const auto &kv : vc->obj) p.push_back((double)kv.second.as_u64() / total);
  return p;
}

double entropy_bits(const json::Value &state) {  // :97-114
  if (state.get_u64("total_count", 0) == 0) return 0.0;
  std::vector<double> terms;
  for (double p : probabilities(state))
    if (p > 0.0) terms.push_back(-p * log2(p));
  return compensated_sum(terms);
}

double entropy_gini(const json::Value &state) {  // :132-148
  if (state.get_u64("total_count", 0) == 0) return 0.0;
  std::vector<double> terms = {1.0};
  for (double p : probabilities(state)) terms.push_back(-(p * p));
  return compensated_sum(terms);
}

}  // namespace term_guard
