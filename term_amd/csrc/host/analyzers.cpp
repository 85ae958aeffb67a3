// analyzers.cpp -- see analyzers.h.  Reference: TG/analyzers/{traits,runner,context,types,errors}.rs,
// TG/analyzers/basic/{size,completeness,distinctness,mean,min_max,sum}.rs,
// TG/analyzers/advanced/{standard_deviation,correlation,mutual_information,histogram,entropy}.rs.
#include "analyzers.h"
#include "../group_key.h"
#include "custom_sql.h"
#include "tgx_handles.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <map>
#include <set>

namespace term_guard {
using tgx::GroupKeyCell;
using tgx::group_key_decode;
using tgx::kGroupKeyInt;
using tgx::kGroupKeyMaxArity;
using tgx::kGroupKeyNull;
using tgx::kGroupKeyString;

// ---------------------------------------------------------------- JSON helpers
static json::Value jnum(double v) {
  json::Value x;
  x.type = json::Value::Number;
  x.num = v;
  return x;
}
static json::Value jbool(bool v) {
  json::Value x;
  x.type = json::Value::Bool;
  x.b = v;
  return x;
}
static json::Value jnull() { return json::Value(); }
static json::Value jstr(const std::string &s) {
  json::Value x;
  x.type = json::Value::String;
  x.str = s;
  return x;
}
static json::Value jobj(std::vector<std::pair<std::string, json::Value>> kv) {
  json::Value x;
  x.type = json::Value::Object;
  x.obj = std::move(kv);
  return x;
}
static json::Value jcount(uint64_t v) { return json::Value::of_u64(v); }  // a `u64` field of a reference state struct
// An f64 field: the shortest text that reads back to the same double, and always with a fraction or an exponent so the
// token is a float to every reader (serde_json prints 30.0, 1e16, 0.1 the same way).
static std::string num_text(double v) {
  if (isnan(v) || isinf(v)) return "null";  // serde_json writes non-finite f64 as null
  char buf[40];
  if (v == floor(v) && fabs(v) < 9.0e15) {
    snprintf(buf, sizeof(buf), "%.1f", v);
    return buf;
  }
  for (int prec = 15; prec <= 17; prec++) {
    snprintf(buf, sizeof(buf), "%.*g", prec, v);
    if (strtod(buf, nullptr) == v) break;
  }
  if (!strpbrk(buf, ".eE")) strcat(buf, ".0");
  return buf;
}
static std::string value_text(const json::Value &v) {
  if (v.int_kind == json::Value::Unsigned) return std::to_string((unsigned long long)v.u);
  if (v.int_kind == json::Value::Signed) return std::to_string((long long)v.i);
  return num_text(v.num);
}
std::string json_dump(const json::Value &v) {
  switch (v.type) {
    case json::Value::Null: return "null";
    case json::Value::Bool: return v.b ? "true" : "false";
    case json::Value::Number: return value_text(v);
    case json::Value::String: return json::quote(v.str);
    case json::Value::Array: {
      std::string o = "[";
      for (size_t i = 0; i < v.arr.size(); i++) o += (i ? ", " : "") + json_dump(v.arr[i]);
      return o + "]";
    }
    case json::Value::Object: {
      std::string o = "{";
      for (size_t i = 0; i < v.obj.size(); i++)
        o += (i ? ", " : "") + json::quote(v.obj[i].first) + ": " + json_dump(v.obj[i].second);
      return o + "}";
    }
  }
  return "null";
}
static double f(const json::Value &s, const char *k) { return s.get_num(k, 0.0); }
static uint64_t u(const json::Value &s, const char *k) { return s.get_u64(k, 0); }
static std::optional<double> opt(const json::Value &s, const char *k) {
  const json::Value *v = s.get(k);
  if (!v || v->type != json::Value::Number) return std::nullopt;
  return v->num;
}

std::string MetricValue::to_json() const {
  switch (kind) {
    case Double: return "{\"type\": \"Double\", \"value\": " + num_text(d) + "}";
    case Long: return "{\"type\": \"Long\", \"value\": " + std::to_string(l) + "}";
    case Boolean: return std::string("{\"type\": \"Boolean\", \"value\": ") + (b ? "true" : "false") + "}";
    case String: return "{\"type\": \"String\", \"value\": " + json::quote(s) + "}";
    case Map: {
      std::string o = "{\"type\": \"Map\", \"value\": {";
      for (size_t i = 0; i < map.size(); i++) o += (i ? ", " : "") + json::quote(map[i].first) + ": " + map[i].second.to_json();
      return o + "}}";
    }
    case Histogram: {  // MetricDistribution's serde form (types.rs:95-169)
      auto optional = [](const std::optional<double> &v) { return v ? num_text(*v) : std::string("null"); };
      std::string o = "{\"type\": \"Histogram\", \"value\": {\"buckets\": [";
      for (size_t i = 0; i < histogram.buckets.size(); i++) {
        const HistogramBucket &b = histogram.buckets[i];
        o += std::string(i ? ", " : "") + "{\"lower_bound\": " + num_text(b.lower_bound) + ", \"upper_bound\": " +
             num_text(b.upper_bound) + ", \"count\": " + std::to_string((unsigned long long)b.count) + "}";
      }
      return o + "], \"total_count\": " + std::to_string((unsigned long long)histogram.total_count) + ", \"min\": " +
             optional(histogram.min) + ", \"max\": " + optional(histogram.max) + ", \"mean\": " +
             optional(histogram.mean) + ", \"std_dev\": " + optional(histogram.std_dev) + "}}";
    }
  }
  return "null";
}

std::string AnalyzerContext::to_json() const {
  std::string o = "{\"metrics\": {";
  for (size_t i = 0; i < metrics.size(); i++)
    o += (i ? ", " : "") + json::quote(metrics[i].first) + ": " + metrics[i].second.to_json();
  o += "}, \"states\": {";
  for (size_t i = 0; i < states.size(); i++)
    o += (i ? ", " : "") + json::quote(states[i].first) + ": " + json_dump(states[i].second);
  o += "}, \"errors\": [";
  for (size_t i = 0; i < errors.size(); i++)
    o += std::string(i ? ", " : "") + "{\"analyzer_name\": " + json::quote(errors[i].first) + ", \"error\": " +
         json::quote(errors[i].second) + "}";
  return o + "]}";
}

// ---------------------------------------------------------------- analyzers
namespace {

SpecRequest req(int kind, const std::string &col, uint32_t flags = 0) {
  SpecRequest r;
  r.kind = kind;
  r.column = col;
  r.flags = flags;
  return r;
}

class SizeAnalyzer : public Analyzer {  // basic/size.rs
 public:
  std::string name() const override { return "size"; }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_COUNT, "")}; }  // COUNT(*): any column
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    return jobj({{"count", jcount(r[0]->total)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // size.rs:60-63
    uint64_t c = 0;
    for (auto &s : states) c += u(s, "count");
    return jobj({{"count", jcount(c)}});
  }
  MetricValue metric_from_state(const json::Value &s) const override { return MetricValue::of_long((int64_t)u(s, "count")); }
};

// advanced/compliance.rs: the fraction of rows on which a predicate is TRUE,
//   SELECT COUNT(CASE WHEN (<predicate>) THEN 1 END), COUNT(*) FROM t
// as one TGX_CHECK_ROW_PREDICATE request; the predicate is compiled by host/custom_sql.h's closed subset
class ComplianceAnalyzer : public Analyzer {
 public:
  // string_functions: the opt-in "string_functions_on_device" (host/custom_sql.h's dialect of that name)
  ComplianceAnalyzer(std::string name, std::string predicate, bool string_functions = false)
      : name_(std::move(name)), predicate_(std::move(predicate)) {
    dialect_.string_functions = string_functions;
  }
  std::string name() const override { return "compliance"; }  // (metric_key: the trait's default, the name)
  const std::string &check_name() const { return name_; }
  const std::string &predicate() const { return predicate_; }
  std::vector<std::string> columns() const override {
    try {
      return compile_row_predicate(predicate_, dialect_).columns;
    } catch (const PredicateRefusal &) {
      return {};
    }
  }
  std::vector<SpecRequest> plan() const override {
    // validate_predicate (:88-108): a substring test on the lower-cased text, in the list's order
    if (auto word = compliance_forbidden_keyword(predicate_))
      throw AnalyzerError::custom("Invalid configuration: Predicate contains forbidden keyword: " + *word);
    try {
      return {row_predicate_request(compile_row_predicate(predicate_, dialect_))};
    } catch (const PredicateRefusal &r) {
      throw AnalyzerError::custom("Invalid configuration: Invalid predicate '" + predicate_ +
                                  "': not on the GPU path: " + r.what);
    }
  }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    return jobj({{"compliant_count", jcount(r[0]->matches)}, {"total_count", jcount(r[0]->total)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :66-75
    uint64_t c = 0, t = 0;
    for (auto &s : states) {
      c += u(s, "compliant_count");
      t += u(s, "total_count");
    }
    return jobj({{"compliant_count", jcount(c)}, {"total_count", jcount(t)}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :52-58: an empty dataset is compliant
    const uint64_t t = u(s, "total_count");
    return MetricValue::of_double(t == 0 ? 1.0 : (double)u(s, "compliant_count") / (double)t);
  }

 private:
  std::string name_, predicate_;
  PredicateDialect dialect_;
};

class ColumnAnalyzer : public Analyzer {
 public:
  explicit ColumnAnalyzer(std::string c) : column_(std::move(c)) {}
  std::string metric_key() const override { return name() + "." + column_; }
  std::vector<std::string> columns() const override { return {column_}; }

 protected:
  std::string column_;
};

class CompletenessAnalyzer : public ColumnAnalyzer {  // basic/completeness.rs
 public:
  using ColumnAnalyzer::ColumnAnalyzer;
  std::string name() const override { return "completeness"; }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_COUNT, column_)}; }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    return jobj({{"total_count", jcount(r[0]->total)}, {"non_null_count", jcount(r[0]->non_null)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :76-84
    uint64_t t = 0, n = 0;
    for (auto &s : states) {
      t += u(s, "total_count");
      n += u(s, "non_null_count");
    }
    return jobj({{"total_count", jcount(t)}, {"non_null_count", jcount(n)}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :62-68: empty dataset is complete
    const uint64_t t = u(s, "total_count");
    return MetricValue::of_double(t == 0 ? 1.0 : (double)u(s, "non_null_count") / (double)t);
  }
};

class DistinctnessAnalyzer : public ColumnAnalyzer {  // basic/distinctness.rs
 public:
  using ColumnAnalyzer::ColumnAnalyzer;
  std::string name() const override { return "distinctness"; }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_DISTINCT, column_)}; }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    // COUNT(col) is the denominator, not COUNT(*) (:113-116)
    return jobj({{"total_count", jcount(r[0]->non_null)}, {"distinct_count", jcount(r[0]->distinct)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :77-92: clamped sum, an upper bound
    uint64_t t = 0, d = 0;
    for (auto &s : states) {
      t += u(s, "total_count");
      d += u(s, "distinct_count");
    }
    return jobj({{"total_count", jcount(t)}, {"distinct_count", jcount(std::min(d, t))}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :35-41
    const uint64_t t = u(s, "total_count");
    return MetricValue::of_double(t == 0 ? 1.0 : (double)u(s, "distinct_count") / (double)t);
  }
};

// advanced/approx_count_distinct.rs: APPROX_DISTINCT(col) (DataFusion's HyperLogLog, a third-party estimate whose
// value is unpinned by the reference's tests) and COUNT(col).  The device path keeps a HyperLogLog of the same shape on
// the column's scan (TGX_CHECK_APPROX_DISTINCT; the exact count on string columns); state fields, the max-merge and the
// metric type are the reference's.
class ApproxCountDistinctAnalyzer : public ColumnAnalyzer {
 public:
  using ColumnAnalyzer::ColumnAnalyzer;
  std::string name() const override { return "approx_count_distinct"; }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_APPROX_DISTINCT, column_)}; }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    return jobj({{"approx_distinct_count", jcount(r[0]->distinct)}, {"total_count", jcount(r[0]->non_null)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :45-61: max of the counts
    uint64_t d = 0, t = 0;
    for (auto &s : states) {
      d = std::max(d, u(s, "approx_distinct_count"));
      t += u(s, "total_count");
    }
    return jobj({{"approx_distinct_count", jcount(d)}, {"total_count", jcount(t)}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :126-128
    return MetricValue::of_long((int64_t)u(s, "approx_distinct_count"));
  }
};

// SUM(col) comes back as Float64 for Float64 columns and Int64 (wrapping) for Int64 columns
double sql_sum(const tgx_result *r) { return r->is_float ? r->sum_f : (double)r->sum_i; }

class MeanAnalyzer : public ColumnAnalyzer {  // basic/mean.rs
 public:
  using ColumnAnalyzer::ColumnAnalyzer;
  std::string name() const override { return "mean"; }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_NUMERIC_STATS, column_)}; }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    // the sum is read as Float64Array only (:117-126): an Int64 column's SUM is Int64 -> InvalidData, unless the
    // sum is NULL (no non-null value), which reads as 0.0
    if (r[0]->non_null > 0 && !r[0]->is_float) throw AnalyzerError::invalid_data("Expected Float64 array for sum");
    return jobj({{"sum", jnum(r[0]->non_null > 0 ? r[0]->sum_f : 0.0)}, {"count", jcount(r[0]->non_null)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {
    double sum = 0;
    uint64_t c = 0;
    for (auto &s : states) {
      sum += f(s, "sum");
      c += u(s, "count");
    }
    return jobj({{"sum", jnum(sum)}, {"count", jcount(c)}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :147-152
    const uint64_t c = u(s, "count");
    if (c == 0) throw AnalyzerError::no_data();
    return MetricValue::of_double(f(s, "sum") / (double)c);
  }
};

class MinMaxAnalyzer : public ColumnAnalyzer {  // basic/min_max.rs (MinAnalyzer / MaxAnalyzer share MinMaxState)
 public:
  MinMaxAnalyzer(std::string c, bool is_max) : ColumnAnalyzer(std::move(c)), is_max_(is_max) {}
  std::string name() const override { return is_max_ ? "max" : "min"; }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_NUMERIC_STATS, column_)}; }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    if (!r[0]->has_value) return jobj({{"min", jnull()}, {"max", jnull()}});
    const double mn = r[0]->is_float ? r[0]->min_f : (double)r[0]->min_i;  // Int64 -> `as f64` (:118-123)
    const double mx = r[0]->is_float ? r[0]->max_f : (double)r[0]->max_i;
    return jobj({{"min", jnum(mn)}, {"max", jnum(mx)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :13-29
    std::optional<double> mn, mx;
    for (auto &s : states) {
      if (auto v = opt(s, "min")) mn = mn ? std::min(*mn, *v) : *v;
      if (auto v = opt(s, "max")) mx = mx ? std::max(*mx, *v) : *v;
    }
    return jobj({{"min", mn ? jnum(*mn) : jnull()}, {"max", mx ? jnum(*mx) : jnull()}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :167-172 / :316-321
    auto v = opt(s, is_max_ ? "max" : "min");
    if (!v) throw AnalyzerError::no_data();
    return MetricValue::of_double(*v);
  }

 private:
  bool is_max_;
};

class SumAnalyzer : public ColumnAnalyzer {  // basic/sum.rs
 public:
  using ColumnAnalyzer::ColumnAnalyzer;
  std::string name() const override { return "sum"; }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_NUMERIC_STATS, column_)}; }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    return jobj({{"sum", jnum(r[0]->non_null > 0 ? sql_sum(r[0]) : 0.0)}, {"has_values", jbool(r[0]->non_null > 0)}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :35-40
    double sum = 0;
    bool any = false;
    for (auto &s : states) {
      sum += f(s, "sum");
      any = any || s.get_bool("has_values");
    }
    return jobj({{"sum", jnum(sum)}, {"has_values", jbool(any)}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :145-151
    if (!s.get_bool("has_values")) throw AnalyzerError::no_data();
    return MetricValue::of_double(f(s, "sum"));
  }
};

class StandardDeviationAnalyzer : public ColumnAnalyzer {  // advanced/standard_deviation.rs
 public:
  using ColumnAnalyzer::ColumnAnalyzer;
  std::string name() const override { return "standard_deviation"; }
  std::string metric_key() const override { return name(); }  // the reference does not add the column (:281-291)
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_NUMERIC_STATS, column_, TGX_FLAG_VARIANCE)}; }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    const double n = (double)r[0]->non_null;
    if (r[0]->non_null == 0) return state(0, 0.0, 0.0, 0.0);  // :192-193
    // COUNT, AVG, SUM, SUM(x*x) WHERE x IS NOT NULL (:171-180); SUM of an Int64 column is Int64: "Expected Float64"
    if (!r[0]->is_float) throw AnalyzerError::invalid_data("Expected Float64 for sum");
    const double sum = r[0]->sum_f;
    // SUM(x*x) from the shifted moments the scan keeps: M2 + sum^2 / n  (M2 = var_samp * (n - 1))
    const double m2 = r[0]->has_variance ? r[0]->var_samp * (n - 1.0) : 0.0;
    return state(r[0]->non_null, sum, m2 + sum * sum / n, r[0]->mean);
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :133-150
    if (states.empty()) throw AnalyzerError::state_merge("No states to merge");
    uint64_t c = 0;
    double sum = 0, sq = 0;
    for (auto &s : states) {
      c += u(s, "count");
      sum += f(s, "sum");
      sq += f(s, "sum_squared");
    }
    return state(c, sum, sq, c > 0 ? sum / (double)c : 0.0);
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :239-279
    const uint64_t c = u(s, "count");
    const double sum = f(s, "sum"), sq = f(s, "sum_squared"), mean = f(s, "mean");
    MetricValue m;
    m.kind = MetricValue::Map;
    m.map.push_back({"count", MetricValue::of_long((int64_t)c)});
    m.map.push_back({"mean", MetricValue::of_double(mean)});
    std::optional<double> pop_var, samp_var;
    if (c > 0) pop_var = std::max(sq / (double)c - mean * mean, 0.0);                          // :78-88
    if (c > 1) samp_var = std::max((sq - sum * sum / (double)c) / (double)(c - 1), 0.0);       // :96-106
    if (pop_var) m.map.push_back({"std_dev", MetricValue::of_double(sqrt(*pop_var))});
    if (samp_var) m.map.push_back({"sample_std_dev", MetricValue::of_double(sqrt(*samp_var))});
    if (pop_var) m.map.push_back({"variance", MetricValue::of_double(*pop_var)});
    if (samp_var) m.map.push_back({"sample_variance", MetricValue::of_double(*samp_var)});
    if (pop_var && fabs(mean) >= 2.220446049250313e-16)                                         // :122-129
      m.map.push_back({"coefficient_of_variation", MetricValue::of_double(sqrt(*pop_var) / fabs(mean))});
    return m;
  }

 private:
  static json::Value state(uint64_t c, double sum, double sq, double mean) {
    return jobj({{"count", jcount(c)}, {"sum", jnum(sum)}, {"sum_squared", jnum(sq)}, {"mean", jnum(mean)}});
  }
};

class CorrelationAnalyzer : public Analyzer {  // advanced/correlation.rs
 public:
  enum Type { Pearson, Spearman, Covariance };
  CorrelationAnalyzer(std::string a, std::string b, Type t) : a_(std::move(a)), b_(std::move(b)), t_(t) {}
  std::string name() const override { return "correlation"; }
  std::string metric_key() const override {  // :445-452
    return std::string("correlation_") + (t_ == Pearson ? "pearson" : t_ == Spearman ? "spearman" : "covariance") + "_" +
           a_ + "_" + b_;
  }
  std::vector<std::string> columns() const override { return {a_, b_}; }
  std::vector<SpecRequest> plan() const override {
    SpecRequest r = req(t_ == Spearman ? TGX_CHECK_SPEARMAN : TGX_CHECK_COMOMENTS, a_);
    r.column2 = b_;
    return {r};
  }
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    return state((uint64_t)r[0]->non_null, r[0]->sum_x, r[0]->sum_y, r[0]->sum_x2, r[0]->sum_y2, r[0]->sum_xy);
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :65-110
    if (states.empty()) throw AnalyzerError::state_merge("Cannot merge empty states");
    if (t_ == Spearman) throw AnalyzerError::state_merge("Cannot merge rank-based correlation states");
    uint64_t n = 0;
    double v[5] = {0, 0, 0, 0, 0};
    static const char *k[5] = {"sum_x", "sum_y", "sum_x2", "sum_y2", "sum_xy"};
    for (auto &s : states) {
      n += u(s, "n");
      for (int i = 0; i < 5; i++) v[i] += f(s, k[i]);
    }
    return state(n, v[0], v[1], v[2], v[3], v[4]);
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :407-435
    const uint64_t nn = u(s, "n");
    if (nn < 2) return MetricValue::of_double(NAN);
    const double n = (double)nn, sx = f(s, "sum_x"), sy = f(s, "sum_y"), sx2 = f(s, "sum_x2"), sy2 = f(s, "sum_y2"),
                 sxy = f(s, "sum_xy");
    if (t_ == Covariance) return MetricValue::of_double((sxy - (sx * sy) / n) / (n - 1.0));
    const double num = n * sxy - sx * sy;
    const double den = sqrt((n * sx2 - sx * sx) * (n * sy2 - sy * sy));
    return MetricValue::of_double(den == 0.0 ? 0.0 : num / den);
  }

 private:
  json::Value state(uint64_t n, double sx, double sy, double sx2, double sy2, double sxy) const {
    return jobj({{"n", jcount(n)}, {"sum_x", jnum(sx)}, {"sum_y", jnum(sy)}, {"sum_x2", jnum(sx2)},
                 {"sum_y2", jnum(sy2)}, {"sum_xy", jnum(sxy)}, {"x_ranks", jnull()}, {"y_ranks", jnull()},
                 {"correlation_type", jstr(t_ == Pearson ? "Pearson" : t_ == Spearman ? "Spearman" : "Covariance")}});
  }
  std::string a_, b_;
  Type t_;
};

// advanced/mutual_information.rs, numeric x numeric branch (:143-248): two passes -- MIN / MAX of both columns over the
// rows with both sides non-NULL, then COUNT(*) GROUP BY FLOOR((x - x_min) / x_width), FLOOR((y - y_min) / y_width) --
// both on the device (TGX_CHECK_JOINT_BINS).  Categorical columns (the reference's other three branches group by the
// string value) are outside the path: the library answers TGX_UNSUPPORTED and that is this analyzer's error.
//
// State: the reference's struct is {n, joint_counts: HashMap<(String, String), u64>, x_counts, y_counts, bins} -- and
// serde_json cannot write a map with tuple keys at all ("key must be a string"), so there is no reference format to
// match for `joint_counts`: here it is a list of [x_label, y_label, count], non-empty cells only, in row-major order.
// `n` and `bins` are integer tokens, x_counts / y_counts maps keyed by the bin label.  A label is the Float64 bin
// index as Arrow casts it to text ("0.0", "1.0", ...: CAST(FLOOR(..) AS VARCHAR)).
//
// The other three branches (:249-293: a string column on either side or both) are an OPT-IN, "max_pairs": N (with an
// optional "max_value_bytes"): the reference's constructor has no bounds, the device's table needs them.  With it, a
// pair with at least one string column plans ONE TGX_CHECK_PAIR_COUNTS request: string x string is one pass; a mixed
// pair is two -- the numeric side's range over the rows with both sides non-NULL, then origin = MIN and
// width = range > 0 ? range / bins : 1.0 (:219-233) and the count.  The state has the same shape: a string side's label
// is its value, a binned side's the bin label; entries follow the library's order (ascending by x cell, then y cell).
// Beyond the bounds (overflow rows, long rows, rows outside the bins, more pairs than max_pairs) the analyzer fails
// with the numbers.  One fidelity guard: the reference takes a column for categorical only when no value of it parses
// as a double (MIN(TRY_CAST(col AS DOUBLE)) IS NULL); a string column with a value that MAY parse (may_parse_as_number:
// a deliberately generous superset of any float grammar) is this analyzer's error, not a guess.
class MutualInformationAnalyzer : public Analyzer {
 public:
  MutualInformationAnalyzer(std::string a, std::string b, uint64_t bins, std::optional<uint64_t> max_pairs = std::nullopt,
                            uint64_t max_value_bytes = TGX_PAIR_COUNTS_MAX_VALUE_BYTES,
                            std::vector<std::string> arrow_types = {})
      : a_(std::move(a)), b_(std::move(b)), bins_(std::max<uint64_t>(bins, 2)),  // :96-104
        max_pairs_(max_pairs), max_value_bytes_(max_value_bytes), arrow_types_(std::move(arrow_types)) {}
  std::string name() const override { return "mutual_information"; }
  std::string metric_key() const override { return "mutual_information_" + a_ + "_" + b_; }  // :413-415
  std::vector<std::string> columns() const override { return {a_, b_}; }
  std::vector<SpecRequest> plan() const override {
    SpecRequest r = req(TGX_CHECK_JOINT_BINS, a_);
    r.column2 = b_;
    return {r};
  }
  static bool is_text(int type) {
    return type == TGX_UTF8 || type == TGX_LARGE_UTF8 || type == TGX_UTF8_VIEW || type == TGX_DICT32_UTF8;
  }
  std::vector<SpecRequest> plan_for(const std::vector<int> &types, const std::vector<std::string> &declared) const override {
    if (!max_pairs_ || types.size() != 2 || (!is_text(types[0]) && !is_text(types[1]))) return plan();
    for (int side = 0; side < 2; side++) {
      const std::string &given = arrow_types_.size() == 2 && !arrow_types_[side].empty() ? arrow_types_[side]
                                 : declared.size() == 2                                  ? declared[side]
                                                                                         : std::string();
      std::string lower;
      for (char ch : given) lower += (char)tolower((unsigned char)ch);
      if (lower.find("binary") != std::string::npos)
        throw AnalyzerError::invalid_data("column '" + (side ? b_ : a_) + "' is declared " + given +
                                          ": its values are not text (not on the GPU path)");
    }
    if (*max_pairs_ < 1 || *max_pairs_ > TGX_PAIR_COUNTS_MAX_PAIRS || max_value_bytes_ < 1 ||
        max_value_bytes_ > TGX_PAIR_COUNTS_MAX_VALUE_BYTES)
      throw AnalyzerError::invalid_data("max_pairs must be 1 .. " + std::to_string(TGX_PAIR_COUNTS_MAX_PAIRS) + " (" +
                                        std::to_string(*max_pairs_) + ") and max_value_bytes 1 .. " +
                                        std::to_string(TGX_PAIR_COUNTS_MAX_VALUE_BYTES) + " (" +
                                        std::to_string(max_value_bytes_) + ")");
    SpecRequest r = req(TGX_CHECK_PAIR_COUNTS, a_);
    r.column2 = b_;
    tgx_pair_counts_params p;
    memset(&p, 0, sizeof(p));
    p.max_pairs = (uint32_t)*max_pairs_;
    p.max_value_bytes = (uint32_t)max_value_bytes_;
    p.x.mode = is_text(types[0]) ? TGX_PAIR_SIDE_VALUE : TGX_PAIR_SIDE_RANGE;
    p.y.mode = is_text(types[1]) ? TGX_PAIR_SIDE_VALUE : TGX_PAIR_SIDE_RANGE;
    r.pair_counts = p;
    return {r};
  }
  bool two_pass() const override { return true; }
  std::optional<FollowUp> follow_up(const FirstPass &first) const override {
    if (first.kind == TGX_CHECK_PAIR_COUNTS) {  // a mixed pair: the numeric side's range is in, the count follows
      const tgx_pair_range &range = first.pair;
      if (range.n == 0) return std::nullopt;
      if (bins_ > TGX_JOINT_MAX_BINS)
        throw AnalyzerError::query("TGX_UNSUPPORTED: " + std::to_string(bins_) + " bins: at most " +
                                   std::to_string(TGX_JOINT_MAX_BINS) + " are supported");
      const bool x_numeric = !is_text(first.column_types.at(0));
      const double span = range.max - range.min;
      if (!std::isfinite(span))
        throw AnalyzerError::invalid_data("the range of " + (x_numeric ? a_ : b_) + " overflows a double: no bin width");
      FollowUp out;
      tgx_pair_counts_params &p = out.pair;
      p.max_pairs = (uint32_t)max_pairs_.value_or(1);
      p.max_value_bytes = (uint32_t)max_value_bytes_;
      tgx_pair_side &num = x_numeric ? p.x : p.y, &text = x_numeric ? p.y : p.x;
      text.mode = TGX_PAIR_SIDE_VALUE;
      num.mode = TGX_PAIR_SIDE_BINNED;
      num.bins = (uint32_t)bins_;
      num.origin = range.min;
      num.width = span > 0.0 ? span / (double)bins_ : 1.0;  // :219-233, in the same double arithmetic
      return out;
    }
    const tgx_joint_range &range = first.joint;
    if (range.n == 0) return std::nullopt;
    if (bins_ > TGX_JOINT_MAX_BINS)
      throw AnalyzerError::query("TGX_UNSUPPORTED: " + std::to_string(bins_) + " bins: at most " +
                                 std::to_string(TGX_JOINT_MAX_BINS) + " are supported");
    FollowUp out;
    tgx_joint_binning &b = out.binning;
    // :219-233, in the same double arithmetic
    const double x_range = range.x_max - range.x_min, y_range = range.y_max - range.y_min;
    if (!std::isfinite(x_range) || !std::isfinite(y_range))
      throw AnalyzerError::invalid_data("the range of " + (std::isfinite(x_range) ? b_ : a_) +
                                        " overflows a double: no bin width");
    b.x_origin = range.x_min;
    b.x_width = x_range > 0.0 ? x_range / (double)bins_ : 1.0;
    b.y_origin = range.y_min;
    b.y_width = y_range > 0.0 ? y_range / (double)bins_ : 1.0;
    b.bins = (uint32_t)bins_;
    return out;
  }
  json::Value state_from_results(const std::vector<const tgx_result *> &, const std::vector<int> &) const override {
    return state_from_follow_up(FirstPass(), nullptr);
  }
  // is `v` inside a superset of what a cast of text to a double may take?  Conservative, and unverified against
  // arrow-cast: after stripping ASCII whitespace, a non-empty text of the characters 0-9 + - . e E _ with a digit in it,
  // or -- after an optional sign -- nan / inf / infinity in either letter case
  static bool may_parse_as_number(const std::string &v) {
    size_t lo = 0, hi = v.size();
    auto space = [](char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); };
    while (lo < hi && space(v[lo])) lo++;
    while (hi > lo && space(v[hi - 1])) hi--;
    if (lo == hi) return false;
    bool only = true, digit = false;
    for (size_t i = lo; i < hi; i++) {
      const char ch = v[i];
      digit |= ch >= '0' && ch <= '9';
      only &= (ch >= '0' && ch <= '9') || ch == '+' || ch == '-' || ch == '.' || ch == 'e' || ch == 'E' || ch == '_';
    }
    if (only && digit) return true;
    if (v[lo] == '+' || v[lo] == '-') lo++;
    std::string word;
    for (size_t i = lo; i < hi; i++) word += (char)tolower((unsigned char)v[i]);
    return word == "nan" || word == "inf" || word == "infinity";
  }
  static bool valid_utf8(const std::string &s) {
    const unsigned char *p = (const unsigned char *)s.data();
    size_t i = 0, n = s.size();
    while (i < n) {
      const unsigned c = p[i];
      size_t more;
      unsigned cp, least;
      if (c < 0x80) { i++; continue; }
      else if ((c & 0xE0) == 0xC0) { more = 1; cp = c & 0x1F; least = 0x80; }
      else if ((c & 0xF0) == 0xE0) { more = 2; cp = c & 0x0F; least = 0x800; }
      else if ((c & 0xF8) == 0xF0) { more = 3; cp = c & 0x07; least = 0x10000; }
      else return false;
      if (i + more >= n) return false;  // (cut short)
      for (size_t k = 1; k <= more; k++) {
        if ((p[i + k] & 0xC0) != 0x80) return false;
        cp = (cp << 6) | (p[i + k] & 0x3F);
      }
      if (cp < least || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;
      i += more + 1;
    }
    return true;
  }
  json::Value state_from_pair_counts(const PairCounts &pc) const override {
    const tgx_pair_counts_summary &s = pc.summary;
    const uint64_t max_pairs = max_pairs_.value_or(0);
    if (s.overflow_rows || s.long_rows || s.out_of_range || s.distinct > max_pairs) {
      char buf[320];
      snprintf(buf, sizeof(buf),
               "the pair is beyond the bounds of its pair counts: %llu distinct pairs (max_pairs %llu), %llu overflow "
               "rows, %llu rows with a value longer than %llu bytes, %llu rows outside the bins (the table changed "
               "between the two passes)",
               (unsigned long long)s.distinct, (unsigned long long)max_pairs, (unsigned long long)s.overflow_rows,
               (unsigned long long)s.long_rows, (unsigned long long)max_value_bytes_, (unsigned long long)s.out_of_range);
      throw AnalyzerError::invalid_data(buf);
    }
    std::vector<Cell> cells;
    uint64_t n = 0;
    for (const PairCounts::Entry &e : pc.entries) {
      std::string labels[2];
      for (int side = 0; side < 2; side++) {
        const PairCell &c = side ? e.y : e.x;
        const std::string &col = side ? b_ : a_;
        if (c.binned) {
          labels[side] = label((uint32_t)c.bin);
          continue;
        }
        if (!valid_utf8(c.bytes))
          throw AnalyzerError::invalid_data("a value of " + col + " is not valid UTF-8: it has no text (not on the GPU path)");
        if (may_parse_as_number(c.bytes))
          throw AnalyzerError::invalid_data("a value of " + col + " may parse as a number: the reference would bin this "
                                            "column (not on the GPU path)");
        labels[side] = c.bytes;
      }
      cells.push_back({labels[0], labels[1], e.count});
      n += e.count;
    }
    return state(n, cells, bins_);
  }
  json::Value state_from_follow_up(const FirstPass &first, const SecondPass *second) const override {
    if (first.kind == TGX_CHECK_PAIR_COUNTS)
      return second ? state_from_pair_counts(second->pairs) : state(0, std::vector<Cell>(), bins_);
    const JointCounts *counts = second ? &second->joint : nullptr;
    std::vector<Cell> cells;
    uint64_t n = 0;
    if (counts) {
      if (counts->out_of_range)
        throw AnalyzerError::query("the table changed between the two passes: " + std::to_string(counts->out_of_range) +
                                   " rows fell outside the bins");
      const uint32_t side = counts->bins + 1;
      for (uint32_t i = 0; i < side; i++)
        for (uint32_t j = 0; j < side; j++)
          if (const uint64_t c = counts->cells[(size_t)i * side + j]) {
            cells.push_back({label(i), label(j), c});
            n += c;
          }
    }
    return state(n, cells, bins_);
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :31-75
    if (states.empty()) throw AnalyzerError::state_merge("Cannot merge empty states");
    const uint64_t bins = u(states[0], "bins");
    uint64_t n = 0;
    std::vector<Cell> cells;
    for (const json::Value &s : states) {
      if (u(s, "bins") != bins) throw AnalyzerError::state_merge("Cannot merge states with different bin counts");
      n += u(s, "n");
      for (const Cell &c : cells_of(s)) {
        bool found = false;
        for (Cell &m : cells)
          if (m.x == c.x && m.y == c.y) {
            m.count += c.count;
            found = true;
          }
        if (!found) cells.push_back(c);
      }
    }
    // (the marginals of the reference's states are the sums of their cells, and stay so under addition)
    return state(n, cells, bins);
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :378-407
    const uint64_t nn = u(s, "n");
    if (nn == 0) return MetricValue::of_double(0.0);
    const double n = (double)nn;
    const json::Value *xc = s.get("x_counts"), *yc = s.get("y_counts");
    double mi = 0.0;
    for (const Cell &c : cells_of(s)) {  // in the state's order: row-major
      const double p_xy = (double)c.count / n;
      const uint64_t x_count = xc ? xc->get_u64(c.x, 0) : 0, y_count = yc ? yc->get_u64(c.y, 0) : 0;
      if (x_count > 0 && y_count > 0) {
        const double p_x = (double)x_count / n, p_y = (double)y_count / n;
        if (p_xy > 0.0) mi += p_xy * log(p_xy / (p_x * p_y));
      }
    }
    return MetricValue::of_double(mi / 0.6931471805599453);  // std::f64::consts::LN_2
  }

 private:
  struct Cell {
    std::string x, y;
    uint64_t count;
  };
  static std::string label(uint32_t i) { return std::to_string(i) + ".0"; }
  static std::vector<Cell> cells_of(const json::Value &s) {
    std::vector<Cell> out;
    const json::Value *j = s.get("joint_counts");
    if (!j || j->type != json::Value::Array) return out;
    for (const json::Value &e : j->arr) {
      if (e.type != json::Value::Array || e.arr.size() != 3 || e.arr[0].type != json::Value::String ||
          e.arr[1].type != json::Value::String)
        throw AnalyzerError::invalid_data("joint_counts entries are [x_label, y_label, count]");
      out.push_back({e.arr[0].str, e.arr[1].str, e.arr[2].as_u64()});
    }
    return out;
  }
  static json::Value state(uint64_t n, const std::vector<Cell> &cells, uint64_t bins) {
    json::Value joint;
    joint.type = json::Value::Array;
    std::vector<std::pair<std::string, uint64_t>> xs, ys;
    auto add = [](std::vector<std::pair<std::string, uint64_t>> &m, const std::string &k, uint64_t c) {
      for (auto &kv : m)
        if (kv.first == k) {
          kv.second += c;
          return;
        }
      m.push_back({k, c});
    };
    for (const Cell &c : cells) {
      json::Value e;
      e.type = json::Value::Array;
      e.arr = {jstr(c.x), jstr(c.y), jcount(c.count)};
      joint.arr.push_back(e);
      add(xs, c.x, c.count);
      add(ys, c.y, c.count);
    }
    std::vector<std::pair<std::string, json::Value>> xo, yo;
    for (auto &kv : xs) xo.push_back({kv.first, jcount(kv.second)});
    for (auto &kv : ys) yo.push_back({kv.first, jcount(kv.second)});
    return jobj({{"n", jcount(n)}, {"joint_counts", joint}, {"x_counts", jobj(xo)}, {"y_counts", jobj(yo)},
                 {"bins", jcount(bins)}});
  }
  std::string a_, b_;
  uint64_t bins_;
  std::optional<uint64_t> max_pairs_;  // the opt-in for string columns (TGX_CHECK_PAIR_COUNTS)
  uint64_t max_value_bytes_;
  std::vector<std::string> arrow_types_;  // the two columns' Arrow DataType names where the table does not say
};

// The reference's arithmetic on the first query's results, in IEEE doubles exactly as written: every product rounds
// before the sum that takes it.  (The library's build does not contract; the pragma keeps it so under any flags.)
struct HistogramArithmetic {
  // histogram.rs:253-275: width = range > 0 && B > 1 ? range / B : 1.0; lower_i = min + (i as f64 * width);
  // the last upper edge = max + width * 0.001
  static std::vector<double> edges(double min, double max, uint64_t buckets) {
#pragma clang fp contract(off)
    const double range = max - min;
    const double width = range > 0.0 && buckets > 1 ? range / (double)buckets : 1.0;
    std::vector<double> e(buckets + 1);
    for (uint64_t i = 0; i < buckets; i++) {
      const double step = (double)i * width;
      e[i] = min + step;
    }
    const double tail = width * 0.001;
    e[buckets] = max + tail;
    return e;
  }
  // histogram.rs:107-115: sqrt(sum_squared / n - mean * mean), NaN when the difference is negative
  static double std_dev(double sum_squared, double n, double mean) {
#pragma clang fp contract(off)
    const double mean_squared = mean * mean;
    const double variance = sum_squared / n - mean_squared;
    return sqrt(variance);
  }
};

// advanced/histogram.rs: two passes -- MIN, MAX, COUNT, SUM, SUM(c * c) WHERE c IS NOT NULL, then COUNT(*) GROUP BY a
// CASE chain over `num_buckets` equal-width buckets whose edges come from the first -- both on the device
// (TGX_CHECK_HISTOGRAM).  The reference downcasts MIN to Float64Array, so a column of another type is
// "Expected Float64 for min" there; with "strict_reference_types": false on the analyzer such a column runs CAST AS
// DOUBLE instead.  Rows holding a NaN or an infinity are left out of everything, as MutualInformationAnalyzer does.
class HistogramAnalyzer : public ColumnAnalyzer {
 public:
  HistogramAnalyzer(std::string c, uint64_t num_buckets, bool strict_types)
      : ColumnAnalyzer(std::move(c)), buckets_(std::min<uint64_t>(std::max<uint64_t>(num_buckets, 1), 1000)),  // :61-66
        strict_types_(strict_types) {}
  std::string name() const override { return "histogram"; }
  std::string metric_key() const override { return name(); }  // the reference does not add the column (traits.rs:133-135)
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_HISTOGRAM, column_)}; }
  bool two_pass() const override { return true; }
  std::optional<FollowUp> follow_up(const FirstPass &first) const override {
    const tgx_histogram_range &r = first.histogram;
    if (r.n == 0) return std::nullopt;  // :237-246: the empty state, no second query
    if (strict_types_ && !first.column_types.empty() && first.column_types[0] != TGX_FLOAT64)
      throw AnalyzerError::invalid_data("Expected Float64 for min");  // :205-210
    if (!std::isfinite(r.max - r.min))
      throw AnalyzerError::invalid_data("the range of " + column_ + " overflows a double: no bucket width");
    FollowUp out;
    out.edges = HistogramArithmetic::edges(r.min, r.max, buckets_);
    for (double e : out.edges)
      if (!std::isfinite(e))
        throw AnalyzerError::invalid_data("the bucket edges of " + column_ + " overflow a double");
    return out;
  }
  json::Value state_from_results(const std::vector<const tgx_result *> &, const std::vector<int> &) const override {
    return state_from_follow_up(FirstPass(), nullptr);
  }
  json::Value state_from_follow_up(const FirstPass &first, const SecondPass *second) const override {
    State s;
    if (!second) return dump(s);  // no rows
    const tgx_histogram_range &r = first.histogram;
    const std::vector<double> e = HistogramArithmetic::edges(r.min, r.max, buckets_);
    for (size_t i = 0; i < second->buckets.size() && i + 1 < e.size(); i++)
      s.buckets.push_back({e[i], e[i + 1], second->buckets[i]});
    s.min = r.min;
    s.max = r.max;
    s.total = r.n;
    s.sum = r.sum;
    s.sum_squared = r.sum_squared;
    return dump(s);
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :120-171
    if (states.empty()) throw AnalyzerError::state_merge("No states to merge");
    State m = parse(states[0]);  // the first state's bucket structure
    for (size_t k = 1; k < states.size(); k++) {
      const State s = parse(states[k]);
      if (s.buckets.size() == m.buckets.size())
        for (size_t i = 0; i < s.buckets.size(); i++) m.buckets[i].count += s.buckets[i].count;
      // min_by / max_by over partial_cmp, Equal when unordered: a later value replaces only when it compares below / not below
      if (s.min < m.min) m.min = s.min;
      if (!(s.max < m.max)) m.max = s.max;
      m.total += s.total;
      m.sum += s.sum;
      m.sum_squared += s.sum_squared;
    }
    return dump(m);
  }
  MetricValue metric_from_state(const json::Value &state) const override {  // :333-342
    const State s = parse(state);
    MetricValue m;
    m.kind = MetricValue::Histogram;
    m.histogram.buckets = s.buckets;
    for (const HistogramBucket &b : s.buckets) m.histogram.total_count += b.count;  // from_buckets (types.rs:130-140)
    const double n = (double)s.total;
    const std::optional<double> mean = s.total > 0 ? std::optional<double>(s.sum / n) : std::nullopt;  // :96-103
    const std::optional<double> sd =
        s.total > 1 ? std::optional<double>(HistogramArithmetic::std_dev(s.sum_squared, n, *mean)) : std::nullopt;
    m.histogram.min = s.min;
    m.histogram.max = s.max;
    m.histogram.mean = mean.value_or(0.0);
    m.histogram.std_dev = sd.value_or(0.0);
    return m;
  }

 private:
  struct State {  // HistogramState (:79-93)
    std::vector<HistogramBucket> buckets;
    double min = 0, max = 0, sum = 0, sum_squared = 0;
    uint64_t total = 0;
  };
  static State parse(const json::Value &v) {
    State s;
    if (const json::Value *b = v.get("buckets"))
      if (b->type == json::Value::Array)
        for (const json::Value &e : b->arr) s.buckets.push_back({f(e, "lower_bound"), f(e, "upper_bound"), u(e, "count")});
    s.min = f(v, "min_value");
    s.max = f(v, "max_value");
    s.total = u(v, "total_count");
    s.sum = f(v, "sum");
    s.sum_squared = f(v, "sum_squared");
    return s;
  }
  static json::Value dump(const State &s) {
    json::Value buckets;
    buckets.type = json::Value::Array;
    for (const HistogramBucket &b : s.buckets)
      buckets.arr.push_back(jobj({{"lower_bound", jnum(b.lower_bound)}, {"upper_bound", jnum(b.upper_bound)},
                                  {"count", jcount(b.count)}}));
    return jobj({{"buckets", buckets}, {"min_value", jnum(s.min)}, {"max_value", jnum(s.max)},
                 {"total_count", jcount(s.total)}, {"sum", jnum(s.sum)}, {"sum_squared", jnum(s.sum_squared)}});
  }
  uint64_t buckets_;
  bool strict_types_;
};

// advanced/entropy.rs: SELECT CAST(col AS VARCHAR), COUNT(*) .. WHERE col IS NOT NULL GROUP BY .. as one
// TGX_CHECK_VALUE_COUNTS request bounded by max_unique_values.  The state is EntropyState's serde form; beyond the bound
// the analyzer fails with the numbers (the reference's truncated top-N sampling is not reproduced: `truncated` is only
// ever true in a state that was handed in).  Its JSON tag is "value_entropy"; name() is the reference's "entropy".
class EntropyAnalyzer : public ColumnAnalyzer {
 public:
  EntropyAnalyzer(std::string c, uint64_t max_unique_values, std::string arrow_type)
      : ColumnAnalyzer(std::move(c)), max_unique_(std::max<uint64_t>(max_unique_values, 10)),  // entropy.rs:66-71
        arrow_type_(std::move(arrow_type)) {}
  std::string name() const override { return "entropy"; }
  std::vector<SpecRequest> plan() const override { return {value_counts_request(column_, max_unique_)}; }
  bool reads_value_counts() const override { return true; }
  std::string value_text_refusal(int type) const override {
    const std::string t = !arrow_type_.empty()      ? arrow_type_
                          : type == TGX_FLOAT64     ? "Float64"
                          : type == TGX_FLOAT32     ? "Float32"
                          : type == TGX_BOOL        ? "Boolean"
                                                    : "";
    return term_guard::value_text_refusal(column_, t);
  }
  json::Value state_from_results(const std::vector<const tgx_result *> &, const std::vector<int> &) const override {
    throw AnalyzerError::invalid_data("the entropy state is built from value counts");
  }
  json::Value state_from_value_counts(const ValueCounts &vc) const override {
    const std::string beyond = value_counts_out_of_bound(vc, max_unique_);
    if (!beyond.empty()) throw AnalyzerError::invalid_data(beyond);
    return entropy_state(vc);
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override { return entropy_merge(states); }
  MetricValue metric_from_state(const json::Value &s) const override {  // :337-395
    const json::Value *vc = s.get("value_counts");
    const size_t unique = vc && vc->is(json::Value::Object) ? vc->obj.size() : 0;
    const uint64_t total = u(s, "total_count");
    const double h = entropy_bits(s);
    MetricValue m;
    m.kind = MetricValue::Map;
    m.map.push_back({"entropy", MetricValue::of_double(h)});
    m.map.push_back({"normalized_entropy", MetricValue::of_double(unique <= 1 ? 0.0 : h / log2((double)unique))});
    m.map.push_back({"gini_impurity", MetricValue::of_double(entropy_gini(s))});
    m.map.push_back({"effective_values", MetricValue::of_double(pow(2.0, h))});
    m.map.push_back({"unique_values", MetricValue::of_long((int64_t)unique)});
    m.map.push_back({"total_count", MetricValue::of_long((int64_t)total)});
    m.map.push_back({"truncated", MetricValue::of_bool(s.get_bool("truncated", false))});
    if (unique <= 100) {  // the ten most frequent values (ties by text: the reference's HashMap order is arbitrary)
      std::vector<std::pair<std::string, uint64_t>> top;
      if (unique)
        for (const auto &kv : vc->obj) top.emplace_back(kv.first, kv.second.as_u64());
      std::sort(top.begin(), top.end(), [](const std::pair<std::string, uint64_t> &a, const std::pair<std::string, uint64_t> &b) {
        return a.second != b.second ? a.second > b.second : a.first < b.first;
      });
      if (top.size() > 10) top.resize(10);
      MetricValue tv;
      tv.kind = MetricValue::Map;
      for (const auto &e : top) {
        MetricValue one;
        one.kind = MetricValue::Map;
        one.map.push_back({"count", MetricValue::of_long((int64_t)e.second)});
        one.map.push_back({"probability", MetricValue::of_double((double)e.second / (double)total)});
        tv.map.push_back({e.first, one});
      }
      m.map.push_back({"top_values", tv});
    }
    return m;
  }

 private:
  uint64_t max_unique_;
  std::string arrow_type_;
};

// advanced/data_type.rs: the CASE over TRY_CASTs, counted per inferred type (:129-150).  What is planned depends on the
// column (plan_for):
//   a string column          one TGX_CHECK_TYPE_CLASSES request; the device's syntactic classes become the reference's
//                            labels in state_from_type_classes
//   a declared integer type  (Int8 .. Int64, UInt8 .. UInt32) two VALUE_RULE BETWEEN requests that share one walk:
//                            [0, 1] and the Int32 range.  CAST(c AS VARCHAR) of an integer is its canonical text, so
//                            boolean = valid[0, 1], integer = valid[Int32] - boolean, double = non_null - valid[Int32]
//                            (TRY_CAST AS DOUBLE of an Int64 never fails)
//   Float32 / Float64        a COUNT: every non-NULL row is 'double' (CAST(1.0 AS VARCHAR) is "1.0", never an integer's
//                            text, and a float is no boolean's text)
//   declared temporal, decimal, boolean, binary, UInt64: the analyzer's own error
// State {"type_counts": {label: u64}, "total_count": u64}; a class without rows is absent, as the GROUP BY has no row
// for it.
constexpr const char *kDatetimeLabel = "date";  // UNVERIFIED: arrow-cast's Date32 parser is believed to
                                                // take a text longer than 10 bytes through the timestamp parser and keep
                                                // the date, so the CASE stops at 'date' and 'timestamp' is unreachable
                                                // from a string column
class DataTypeAnalyzer : public ColumnAnalyzer {
 public:
  DataTypeAnalyzer(std::string c, std::string arrow_type) : ColumnAnalyzer(std::move(c)), arrow_type_(std::move(arrow_type)) {}
  std::string name() const override { return "data_type"; }
  enum Route { kStrings, kIntegers, kFloats };
  Route route_for(int type, const std::string &declared) const {
    const std::string &given = !arrow_type_.empty() ? arrow_type_ : declared;
    std::string t;
    for (char ch : given) t += (char)tolower((unsigned char)ch);
    auto starts = [&](const char *p) { return t.compare(0, strlen(p), p) == 0; };
    if (!t.empty()) {
      if (starts("utf8") || starts("largeutf8") || starts("dictionary") || starts("string") || starts("large_string"))
        return kStrings;
      if ((starts("int") && !starts("interval")) || (starts("uint") && !starts("uint64"))) return kIntegers;
      if (starts("float32") || starts("float64")) return kFloats;
      throw AnalyzerError::invalid_data("column '" + column_ + "' (" + given +
                                        ") is not on the GPU path: data_type takes string, integer (other than UInt64) "
                                        "and Float32 / Float64 columns");
    }
    switch (type) {
      case TGX_FLOAT64: case TGX_FLOAT32: return kFloats;
      case TGX_UINT64: case TGX_BOOL:
        throw AnalyzerError::invalid_data("column '" + column_ + "' (" + (type == TGX_BOOL ? "Boolean" : "UInt64") +
                                          ") is not on the GPU path: data_type takes string, integer (other than UInt64) "
                                          "and Float32 / Float64 columns");
      case 0: case TGX_UTF8: case TGX_LARGE_UTF8: case TGX_UTF8_VIEW: case TGX_DICT32_UTF8: return kStrings;
      default: return kIntegers;
    }
  }
  std::vector<SpecRequest> plan() const override { return {req(TGX_CHECK_TYPE_CLASSES, column_)}; }
  std::vector<SpecRequest> plan_for(const std::vector<int> &types, const std::vector<std::string> &declared) const override {
    const Route route = route_for(types.empty() ? 0 : types[0], declared.empty() ? std::string() : declared[0]);
    if (route == kStrings) return plan();
    if (route == kFloats) return {req(TGX_CHECK_COUNT, column_)};
    std::vector<SpecRequest> out;
    for (int k = 0; k < 2; k++) {
      SpecRequest r = req(TGX_CHECK_VALUE_RULE, column_);
      tgx_value_rule_params p;
      memset(&p, 0, sizeof(p));
      p.mode = TGX_RULE_BETWEEN;
      p.lo_i = k == 0 ? 0 : INT32_MIN;
      p.hi_i = k == 0 ? 1 : INT32_MAX;
      p.lo_f = (double)p.lo_i;
      p.hi_f = (double)p.hi_i;
      r.value_rule = p;
      out.push_back(r);
    }
    return out;
  }
  static json::Value state_of(const std::vector<std::pair<const char *, uint64_t>> &counts) {
    std::vector<std::pair<std::string, json::Value>> types;
    uint64_t total = 0;
    for (const auto &c : counts) {
      total += c.second;
      if (c.second == 0) continue;
      bool merged = false;
      for (auto &t : types)
        if (t.first == c.first) {
          t.second = jcount(t.second.as_u64() + c.second);
          merged = true;
        }
      if (!merged) types.push_back({c.first, jcount(c.second)});
    }
    return jobj({{"type_counts", jobj(types)}, {"total_count", jcount(total)}});
  }
  // the integer route (two VALUE_RULE results) and the float route (one COUNT)
  json::Value state_from_results(const std::vector<const tgx_result *> &r, const std::vector<int> &) const override {
    if (r.size() == 2) {
      const uint64_t non_null = (uint64_t)r[1]->non_null, small = (uint64_t)r[0]->matches, fits = (uint64_t)r[1]->matches;
      return state_of({{"boolean", small}, {"integer", fits - small}, {"double", non_null - fits}});
    }
    return state_of({{"double", (uint64_t)r[0]->non_null}});
  }
  json::Value state_from_type_classes(const tgx_type_classes_counts &c) const override {
    if (c.undecided_rows > 0)
      throw AnalyzerError::invalid_data("column '" + column_ + "' is not on the GPU path: " +
                                        std::to_string((unsigned long long)c.undecided_rows) +
                                        " values look like dates in a form this path does not decide");
    return state_of({{"boolean", c.boolean_rows}, {"integer", c.integer_rows}, {"double", c.double_rows},
                     {"date", c.date_rows}, {kDatetimeLabel, c.datetime_rows}, {"string", c.string_rows}});
  }
  json::Value merge_states(const std::vector<json::Value> &states) const override {  // :94-109
    std::vector<std::pair<std::string, json::Value>> types;
    uint64_t total = 0;
    for (const json::Value &s : states) {
      total += u(s, "total_count");
      const json::Value *tc = s.get("type_counts");
      if (!tc || !tc->is(json::Value::Object)) continue;
      for (const auto &kv : tc->obj) {
        bool merged = false;
        for (auto &t : types)
          if (t.first == kv.first) {
            t.second = jcount(t.second.as_u64() + kv.second.as_u64());
            merged = true;
          }
        if (!merged) types.push_back({kv.first, jcount(kv.second.as_u64())});
      }
    }
    return jobj({{"type_counts", jobj(types)}, {"total_count", jcount(total)}});
  }
  MetricValue metric_from_state(const json::Value &s) const override {  // :193-202: a Map of Long
    MetricValue m;
    m.kind = MetricValue::Map;
    if (const json::Value *tc = s.get("type_counts"))
      if (tc->is(json::Value::Object))
        for (const auto &kv : tc->obj) m.map.push_back({kv.first, MetricValue::of_long((int64_t)kv.second.as_u64())});
    return m;
  }

 private:
  std::string arrow_type_;  // the column's Arrow DataType name where the table does not say
};

// basic/grouped_completeness.rs + grouped.rs: CompletenessAnalyzer::with_grouping, "completeness per segment",
//   SELECT g, COUNT(*) AS total_count, COUNT(col) AS non_null_count FROM t GROUP BY g
//   ORDER BY COUNT(col) * 1.0 / COUNT(*) DESC LIMIT max_groups + 1                    (grouped_completeness.rs:119-150)
// as one TGX_CHECK_GROUP_COUNTS request.  name() stays "completeness"; metric_key() is
// "completeness.<col>_grouped_by_<g>" (grouped.rs:288-294); the JSON tag is "grouped_completeness".
// The reference's rules, restated:
//   - rows come ordered by completeness descending; the first max_groups are kept; total_groups counts the rows the
//     LIMIT let through, min(actual, max_groups + 1); `overall` sums the kept rows only (:160-200).  The order among
//     rows of equal completeness is unspecified there: here by key ascending, the NULL group last.
//   - a NULL key reads as "" (StringArray::value, :258-262).  When a "" group exists as well, the later of the two rows
//     overwrites the earlier in the map, yet both count in total_groups and `overall`, so `truncated` comes out true.
//   - included_groups is the map's size, truncated = total_groups > included_groups (grouped.rs:179-188).
//   - a group column that is no StringArray makes the reference push the {:?} of the WHOLE key array for every row
//     (:263-268): with strict_reference_types (the default) such a column is this analyzer's error; without, strings
//     of every layout group by value and integers print as decimal text.
// More than one group column, or none, is the analyzer's error: TGX_CHECK_GROUP_COUNTS groups by one column.
// The state is ours -- the reference's BTreeMap<Vec<String>, _> does not pass through serde_json, whose map keys must
// be strings: {"groups": [{"key": [..], "total_count", "non_null_count"}, ..ascending by key], "null_group": {..}|null,
// "overall": {..}|null, "metadata": GroupedMetadata}.  Beyond the device's bounds the analyzer fails with the numbers.
class GroupedCompletenessAnalyzer : public ColumnAnalyzer {
 public:
  GroupedCompletenessAnalyzer(std::string c, GroupingConfig config, bool strict, std::string group_arrow_type,
                              std::vector<std::string> group_arrow_types = {})
      : ColumnAnalyzer(std::move(c)), config_(std::move(config)), strict_(strict),
        group_arrow_type_(std::move(group_arrow_type)), group_arrow_types_(std::move(group_arrow_types)) {}
  std::string name() const override { return "completeness"; }
  std::string metric_key() const override {
    std::string joined;
    for (size_t i = 0; i < config_.columns.size(); i++) joined += (i ? "_" : "") + config_.columns[i];
    return "completeness." + column_ + "_grouped_by_" + joined;
  }
  std::vector<std::string> columns() const override {
    std::vector<std::string> cols = {column_};
    cols.insert(cols.end(), config_.columns.begin(), config_.columns.end());
    return cols;
  }
  // the table bound on the device: max_groups, capped at what the kind takes
  uint32_t device_bound() const {
    const uint64_t most = TGX_GROUP_COUNTS_MAX_GROUPS;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(config_.max_groups.value_or(most), 1), most);
  }
  // 2 .. 8 group columns with the opt-in: one request on the tuple of the columns
  bool tuples() const {
    return config_.composite_on_device && config_.columns.size() >= 2 && config_.columns.size() <= (size_t)kGroupKeyMaxArity;
  }
  std::vector<SpecRequest> plan() const override {
    if (tuples()) {
      SpecRequest r = req(TGX_CHECK_GROUP_COUNTS, column_);
      r.columns = config_.columns;
      r.group_counts = tgx_group_counts_params{device_bound(), TGX_GROUP_COUNTS_MAX_VALUE_BYTES};
      return {r};
    }
    if (config_.columns.size() != 1)
      throw AnalyzerError::invalid_data("grouped completeness groups by exactly one column on the GPU path (" +
                                        std::to_string(config_.columns.size()) + " given)");
    SpecRequest r = req(TGX_CHECK_GROUP_COUNTS, column_);
    r.column2 = config_.columns[0];
    r.group_counts = tgx_group_counts_params{device_bound(), TGX_GROUP_COUNTS_MAX_VALUE_BYTES};
    return {r};
  }
  std::vector<SpecRequest> plan_for(const std::vector<int> &types, const std::vector<std::string> &declared) const override {
    std::vector<SpecRequest> reqs = plan();
    if (!strict_) return reqs;
    // every group column must be declared Utf8: the error names the first that is not
    for (size_t g = 0; g < config_.columns.size(); g++) {
      const int type = types.size() > 1 + g ? types[1 + g] : 0;
      std::string t = g == 0 && !group_arrow_type_.empty() ? group_arrow_type_
                      : g < group_arrow_types_.size() && !group_arrow_types_[g].empty() ? group_arrow_types_[g]
                      : declared.size() > 1 + g ? declared[1 + g] : std::string();
      if (t.empty())
        t = type == TGX_UTF8 ? "Utf8" : type == TGX_LARGE_UTF8 ? "LargeUtf8" : type == TGX_UTF8_VIEW ? "Utf8View"
            : type == TGX_DICT32_UTF8 ? "Dictionary(Int32, Utf8)" : type == 0 ? "" : "tgx type " + std::to_string(type);
      if (!t.empty() && t != "Utf8")
        throw AnalyzerError::invalid_data(
            "group column '" + config_.columns[g] + "' is " + t + ": the reference reads only a Utf8 group column by value "
            "and pushes the {:?} of the whole key array for every row of any other (grouped_completeness.rs:263-268); "
            "strict_reference_types=false groups strings of every layout by value and prints integers as decimal text");
    }
    return reqs;
  }
  bool reads_group_counts() const override { return true; }
  json::Value state_from_results(const std::vector<const tgx_result *> &, const std::vector<int> &) const override {
    throw AnalyzerError::invalid_data("the grouped completeness state is built from group counts");
  }

  struct Row {
    bool null_key = false;
    int64_t value = 0;
    std::string bytes, text;
    uint64_t total = 0, non_null = 0;
  };
  static double completeness(uint64_t total, uint64_t non_null) {  // CompletenessState::completeness, completeness.rs:67-73
    return total == 0 ? 1.0 : (double)non_null / (double)total;
  }
  static json::Value counts(uint64_t total, uint64_t non_null) {
    return jobj({{"total_count", jcount(total)}, {"non_null_count", jcount(non_null)}});
  }
  json::Value metadata(uint64_t total_groups, uint64_t included) const {
    json::Value cols;
    cols.type = json::Value::Array;
    for (const std::string &c : config_.columns) cols.arr.push_back(jstr(c));
    return jobj({{"group_columns", cols}, {"total_groups", jcount(total_groups)}, {"included_groups", jcount(included)},
                 {"truncated", jbool(total_groups > included)}, {"overflow_strategy", jnull()}});
  }
  // the state's parts -> the state; `groups`: text key -> counts, any order
  json::Value state_of(std::vector<std::pair<std::string, std::pair<uint64_t, uint64_t>>> groups, const json::Value &null_group,
                       const json::Value &overall, const json::Value &meta) const {
    std::sort(groups.begin(), groups.end());
    json::Value arr;
    arr.type = json::Value::Array;
    for (const auto &g : groups) {
      json::Value key;
      key.type = json::Value::Array;
      key.arr.push_back(jstr(g.first));
      arr.arr.push_back(jobj({{"key", key}, {"total_count", jcount(g.second.first)}, {"non_null_count", jcount(g.second.second)}}));
    }
    return jobj({{"groups", arr}, {"null_group", null_group}, {"overall", overall}, {"metadata", meta}});
  }

  // ---- several group columns: the entries' keys are encoded tuples (group_key.h) ----
  // a key as the state holds it: per group column NULL, or the cell's text (an integer as decimal text)
  typedef std::vector<std::pair<bool, std::string>> KeyVec;  // (is NULL, text)
  // key ascending, a NULL cell after any value; values by their text's bytes
  static bool key_less(const KeyVec &a, const KeyVec &b) {
    for (size_t i = 0; i < a.size() && i < b.size(); i++) {
      if (a[i].first != b[i].first) return b[i].first;
      if (a[i].second != b[i].second) return a[i].second < b[i].second;
    }
    return a.size() < b.size();
  }
  static std::vector<std::string> texts_of(const KeyVec &k) {  // (a NULL reads as "")
    std::vector<std::string> t;
    for (const auto &c : k) t.push_back(c.first ? std::string() : c.second);
    return t;
  }
  struct TupleRow {
    std::vector<GroupKeyCell> cells;
    KeyVec key;
    uint64_t total = 0, non_null = 0;
  };
  // ... as the query orders it: integers numerically, strings bytewise, a NULL cell after any value
  static bool cells_less(const std::vector<GroupKeyCell> &a, const std::vector<GroupKeyCell> &b) {
    for (size_t i = 0; i < a.size() && i < b.size(); i++) {
      const bool an = a[i].tag == kGroupKeyNull, bn = b[i].tag == kGroupKeyNull;
      if (an != bn) return bn;
      if (a[i].tag != b[i].tag) return a[i].tag < b[i].tag;
      if (a[i].tag == kGroupKeyInt && a[i].value != b[i].value) return a[i].value < b[i].value;
      if (a[i].tag == kGroupKeyString && a[i].bytes != b[i].bytes) return a[i].bytes < b[i].bytes;
    }
    return a.size() < b.size();
  }
  json::Value tuple_state_of(std::vector<std::pair<KeyVec, std::pair<uint64_t, uint64_t>>> groups, const json::Value &overall,
                             const json::Value &meta) const {
    std::sort(groups.begin(), groups.end(), [](const auto &a, const auto &b) { return key_less(a.first, b.first); });
    json::Value arr;
    arr.type = json::Value::Array;
    for (const auto &g : groups) {
      json::Value key;
      key.type = json::Value::Array;
      for (const auto &c : g.first) key.arr.push_back(c.first ? jnull() : jstr(c.second));
      arr.arr.push_back(jobj({{"key", key}, {"total_count", jcount(g.second.first)}, {"non_null_count", jcount(g.second.second)}}));
    }
    return jobj({{"groups", arr}, {"null_group", jnull()}, {"overall", overall}, {"metadata", meta}});
  }
  static uint64_t distinct_texts(const std::vector<std::pair<KeyVec, std::pair<uint64_t, uint64_t>>> &groups) {
    std::set<std::vector<std::string>> seen;
    for (const auto &g : groups) seen.insert(texts_of(g.first));
    return seen.size();
  }
  std::string joined_columns() const {
    std::string joined;
    for (size_t i = 0; i < config_.columns.size(); i++) joined += (i ? ", " : "") + config_.columns[i];
    return joined;
  }
  json::Value tuple_state_from_group_counts(const GroupCounts &gc) const {
    std::vector<TupleRow> rows;
    for (const GroupCounts::Entry &e : gc.entries) {
      TupleRow r;
      if (!gc.is_bytes || !group_key_decode((const uint8_t *)e.bytes.data(), e.bytes.size(), &r.cells) ||
          r.cells.size() != config_.columns.size())
        throw AnalyzerError::invalid_data("a group key of columns [" + joined_columns() + "] is not the encoded form of a "
                                          "tuple of " + std::to_string(config_.columns.size()) + " columns");
      for (const GroupKeyCell &c : r.cells)
        r.key.push_back({c.tag == kGroupKeyNull, c.tag == kGroupKeyInt ? std::to_string((long long)c.value) : c.bytes});
      r.total = e.total;
      r.non_null = e.non_null;
      rows.push_back(std::move(r));
    }
    // ORDER BY completeness DESC; ties by key ascending, a NULL cell after any value
    std::stable_sort(rows.begin(), rows.end(), [](const TupleRow &a, const TupleRow &b) {
      const double ca = completeness(a.total, a.non_null), cb = completeness(b.total, b.non_null);
      if (ca != cb) return ca > cb;
      return cells_less(a.cells, b.cells);
    });
    const uint64_t limit = config_.max_groups ? *config_.max_groups : UINT64_MAX;
    const uint64_t total_groups = std::min<uint64_t>(rows.size(), limit == UINT64_MAX ? limit : limit + 1);  // LIMIT max_groups + 1
    const size_t kept = (size_t)std::min<uint64_t>(rows.size(), limit);
    std::vector<std::pair<KeyVec, std::pair<uint64_t, uint64_t>>> groups;
    uint64_t all = 0, all_non_null = 0;
    for (size_t i = 0; i < kept; i++) {
      all += rows[i].total;
      all_non_null += rows[i].non_null;
      groups.push_back({rows[i].key, {rows[i].total, rows[i].non_null}});
    }
    // (NULL reads as "": two kept rows with equal text vectors are one key of the reference's map)
    const uint64_t included = distinct_texts(groups);
    return tuple_state_of(std::move(groups), config_.include_overall ? counts(all, all_non_null) : jnull(),
                          metadata(total_groups, included));
  }
  static KeyVec key_of_json(const json::Value *key) {
    KeyVec k;
    if (key && key->type == json::Value::Array)
      for (const json::Value &c : key->arr) k.push_back({c.type != json::Value::String, c.type == json::Value::String ? c.str : std::string()});
    return k;
  }
  // merge_states over the whole key vector (a NULL cell is a cell of its own, apart from "")
  json::Value tuple_merge_states(const std::vector<json::Value> &states) const {
    std::map<KeyVec, std::pair<uint64_t, uint64_t>> by_key;
    bool has_overall = false;
    uint64_t all_t = 0, all_n = 0, total_groups = 0;
    for (const json::Value &st : states) {
      if (const json::Value *gs = st.get("groups"))
        if (gs->type == json::Value::Array)
          for (const json::Value &g : gs->arr) {
            std::pair<uint64_t, uint64_t> &c = by_key[key_of_json(g.get("key"))];
            c.first += u(g, "total_count");
            c.second += u(g, "non_null_count");
          }
      if (const json::Value *ov = st.get("overall"))
        if (ov->type == json::Value::Object) {
          has_overall = true;
          all_t += u(*ov, "total_count");
          all_n += u(*ov, "non_null_count");
        }
      if (const json::Value *md = st.get("metadata")) total_groups = std::max(total_groups, u(*md, "total_groups"));
    }
    std::vector<std::pair<KeyVec, std::pair<uint64_t, uint64_t>>> groups(by_key.begin(), by_key.end());
    json::Value meta = metadata(0, 0);
    if (const json::Value *md = states[0].get("metadata"))
      if (const json::Value *gc = md->get("group_columns")) meta.obj[0].second = *gc;
    const uint64_t included = distinct_texts(groups);
    meta.obj[1].second = jcount(total_groups);
    meta.obj[2].second = jcount(included);
    meta.obj[3].second = jbool(total_groups > included);
    return tuple_state_of(std::move(groups), has_overall ? counts(all_t, all_n) : jnull(), meta);
  }

  json::Value state_from_group_counts(const GroupCounts &gc) const override {
    const tgx_group_counts_summary &s = gc.summary;
    if (tuples() && (s.overflow_rows || s.long_rows))
      throw AnalyzerError::invalid_data(
          "columns [" + joined_columns() + "] have more groups than the table for max_groups " +
          std::to_string(device_bound()) + " holds, or encoded keys longer than " +
          std::to_string((int)TGX_GROUP_COUNTS_MAX_VALUE_BYTES) + " bytes: " + std::to_string(s.groups) + " groups held, " +
          std::to_string(s.overflow_rows) + " overflow rows, " + std::to_string(s.long_rows) + " long rows");
    if (tuples()) return tuple_state_from_group_counts(gc);
    if (s.overflow_rows || s.long_rows)
      throw AnalyzerError::invalid_data(
          "column '" + config_.columns[0] + "' has more groups than the table for max_groups " +
          std::to_string(device_bound()) + " holds, or keys longer than " +
          std::to_string((int)TGX_GROUP_COUNTS_MAX_VALUE_BYTES) + " bytes: " + std::to_string(s.groups) + " groups held, " +
          std::to_string(s.overflow_rows) + " overflow rows, " + std::to_string(s.long_rows) + " long rows");
    std::vector<Row> rows;
    for (const GroupCounts::Entry &e : gc.entries) {
      Row r;
      r.value = e.value;
      r.bytes = e.bytes;
      r.text = gc.is_bytes ? e.bytes : std::to_string((long long)e.value);
      r.total = e.total;
      r.non_null = e.non_null;
      rows.push_back(std::move(r));
    }
    if (s.null_group_rows) {
      Row r;
      r.null_key = true;
      r.total = s.null_group_rows;
      r.non_null = s.null_group_non_null;
      rows.push_back(std::move(r));
    }
    // ORDER BY completeness DESC; ties by key ascending (the library's order), the NULL group last
    std::stable_sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) {
      const double ca = completeness(a.total, a.non_null), cb = completeness(b.total, b.non_null);
      if (ca != cb) return ca > cb;
      return !a.null_key && b.null_key;
    });
    const uint64_t limit = config_.max_groups ? *config_.max_groups : UINT64_MAX;
    const uint64_t total_groups = std::min<uint64_t>(rows.size(), limit == UINT64_MAX ? limit : limit + 1);  // LIMIT max_groups + 1
    const size_t kept = (size_t)std::min<uint64_t>(rows.size(), limit);
    std::vector<std::pair<std::string, std::pair<uint64_t, uint64_t>>> groups;
    json::Value null_group = jnull();
    uint64_t all = 0, all_non_null = 0;
    bool empty_text = false, null_kept = false;
    for (size_t i = 0; i < kept; i++) {
      const Row &r = rows[i];
      all += r.total;
      all_non_null += r.non_null;
      if (r.null_key) {
        null_group = counts(r.total, r.non_null);
        null_kept = true;
      } else {
        groups.push_back({r.text, {r.total, r.non_null}});
        empty_text |= r.text.empty();
      }
    }
    const uint64_t included = groups.size() + (null_kept && !empty_text ? 1 : 0);  // (NULL reads as "": one key with "")
    return state_of(std::move(groups), null_group, config_.include_overall ? counts(all, all_non_null) : jnull(),
                    metadata(total_groups, included));
  }

  // grouped_completeness.rs:37-84: groups by key, their states summed; the overalls summed; the first state's
  // metadata with total_groups the maximum, included_groups the merged map's size, truncated = total > included
  json::Value merge_states(const std::vector<json::Value> &states) const override {
    if (states.empty()) throw AnalyzerError::custom("Invalid configuration: Cannot merge empty states");
    if (tuples()) return tuple_merge_states(states);
    std::vector<std::pair<std::string, std::pair<uint64_t, uint64_t>>> groups;
    bool has_null = false, has_overall = false, empty_text = false;
    uint64_t null_t = 0, null_n = 0, all_t = 0, all_n = 0, total_groups = 0;
    for (const json::Value &st : states) {
      if (const json::Value *gs = st.get("groups"))
        if (gs->type == json::Value::Array)
          for (const json::Value &g : gs->arr) {
            const json::Value *key = g.get("key");
            const std::string text = key && key->type == json::Value::Array && !key->arr.empty() ? key->arr[0].str : std::string();
            auto it = std::find_if(groups.begin(), groups.end(), [&](const auto &e) { return e.first == text; });
            if (it == groups.end()) it = groups.insert(groups.end(), {text, {0, 0}});
            it->second.first += u(g, "total_count");
            it->second.second += u(g, "non_null_count");
            empty_text |= text.empty();
          }
      if (const json::Value *ng = st.get("null_group"))
        if (ng->type == json::Value::Object) {
          has_null = true;
          null_t += u(*ng, "total_count");
          null_n += u(*ng, "non_null_count");
        }
      if (const json::Value *ov = st.get("overall"))
        if (ov->type == json::Value::Object) {
          has_overall = true;
          all_t += u(*ov, "total_count");
          all_n += u(*ov, "non_null_count");
        }
      if (const json::Value *md = st.get("metadata")) total_groups = std::max(total_groups, u(*md, "total_groups"));
    }
    json::Value meta = metadata(0, 0);
    if (const json::Value *md = states[0].get("metadata"))
      if (const json::Value *gc = md->get("group_columns")) meta.obj[0].second = *gc;
    const uint64_t included = groups.size() + (has_null && !empty_text ? 1 : 0);
    meta.obj[1].second = jcount(total_groups);
    meta.obj[2].second = jcount(included);
    meta.obj[3].second = jbool(total_groups > included);
    return state_of(std::move(groups), has_null ? counts(null_t, null_n) : jnull(),
                    has_overall ? counts(all_t, all_n) : jnull(), meta);
  }

  // GroupedMetrics::to_metric_value (grouped.rs:135-156): one Double per group under key.join("_"), then "__overall__",
  // then "__metadata__", a String holding the serde JSON of GroupedMetadata; a later insert of a key replaces the
  // earlier, as in the reference's HashMap
  MetricValue metric_from_state(const json::Value &st) const override {
    MetricValue m;
    m.kind = MetricValue::Map;
    auto put = [&](const std::string &key, MetricValue v) {
      for (auto &kv : m.map)
        if (kv.first == key) {
          kv.second = std::move(v);
          return;
        }
      m.map.push_back({key, std::move(v)});
    };
    const json::Value *ng = st.get("null_group");
    const bool has_null = ng && ng->type == json::Value::Object;
    const double null_c = has_null ? completeness(u(*ng, "total_count"), u(*ng, "non_null_count")) : 0.0;
    bool null_done = false;
    std::map<std::string, double> group_keys;  // (the keys that groups have put so far, with what they put)
    if (const json::Value *gs = st.get("groups"))
      if (gs->type == json::Value::Array)
        for (const json::Value &g : gs->arr) {
          std::string joined;
          if (const json::Value *key = g.get("key"))
            for (size_t i = 0; key->type == json::Value::Array && i < key->arr.size(); i++)
              joined += (i ? "_" : "") + (key->arr[i].type == json::Value::String ? key->arr[i].str : std::string());
          double c = completeness(u(g, "total_count"), u(g, "non_null_count"));
          // two groups under one joined key (a NULL cell reads as ""): the later in the query's order stays, which is
          // the less complete of the two
          const auto earlier = group_keys.find(joined);
          if (earlier != group_keys.end() && earlier->second < c) c = earlier->second;
          if (joined.empty() && has_null) {  // the "" row and the NULL row: the later in the query's order stays
            if (null_c <= c) c = null_c;
            null_done = true;
          }
          group_keys[joined] = c;
          put(joined, MetricValue::of_double(c));
        }
    if (has_null && !null_done) put("", MetricValue::of_double(null_c));
    if (const json::Value *ov = st.get("overall"))
      if (ov->type == json::Value::Object)
        put("__overall__", MetricValue::of_double(completeness(u(*ov, "total_count"), u(*ov, "non_null_count"))));
    std::string meta = "{\"group_columns\":[";
    const json::Value *md = st.get("metadata");
    if (md)
      if (const json::Value *gc = md->get("group_columns"))
        for (size_t i = 0; gc->type == json::Value::Array && i < gc->arr.size(); i++)
          meta += (i ? "," : "") + json::quote(gc->arr[i].str);
    meta += "],\"total_groups\":" + std::to_string((unsigned long long)(md ? u(*md, "total_groups") : 0)) +
            ",\"included_groups\":" + std::to_string((unsigned long long)(md ? u(*md, "included_groups") : 0)) +
            ",\"truncated\":" + (md && md->get_bool("truncated", false) ? "true" : "false") + ",\"overflow_strategy\":null}";
    put("__metadata__", MetricValue::of_string(meta));
    return m;
  }

 private:
  GroupingConfig config_;
  bool strict_;
  std::string group_arrow_type_;
  std::vector<std::string> group_arrow_types_;  // several group columns: their Arrow DataType names where the table does not say
};

}  // namespace

PairCounts read_pair_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index, const tgx_pair_counts_params &params) {
  PairCounts out;
  tgx_error err;
  memset(&err, 0, sizeof(err));
  auto check = [&](tgx_status s) {
    if (s != TGX_OK) throw AnalyzerError::query(std::string(tgx_status_name(s)) + ": " + err.msg);
  };
  check(tgx_pair_counts_get(plan, state, spec_index, &out.summary, &err));
  uint64_t n = 0, nb = 0;
  check(tgx_pair_counts_entries(plan, state, spec_index, nullptr, 0, &n, nullptr, 0, &nb, &err));
  std::vector<tgx_pair_count_entry> entries((size_t)n + 1);
  std::vector<uint8_t> bytes((size_t)nb + 1);
  check(tgx_pair_counts_entries(plan, state, spec_index, entries.data(), n, &n, bytes.data(), nb, &nb, &err));
  for (uint64_t i = 0; i < n; i++) {
    const tgx_pair_count_entry &e = entries[i];
    PairCounts::Entry o;
    o.x.binned = params.x.mode != TGX_PAIR_SIDE_VALUE;
    o.x.bin = e.x_bin;
    if (!o.x.binned) o.x.bytes.assign((const char *)bytes.data() + e.x_offset, (size_t)e.x_length);
    o.y.binned = params.y.mode != TGX_PAIR_SIDE_VALUE;
    o.y.bin = e.y_bin;
    if (!o.y.binned) o.y.bytes.assign((const char *)bytes.data() + e.y_offset, (size_t)e.y_length);
    o.count = e.count;
    out.entries.push_back(std::move(o));
  }
  return out;
}

GroupCounts read_group_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index) {
  GroupCounts out;
  tgx_error err;
  memset(&err, 0, sizeof(err));
  auto check = [&](tgx_status s) {
    if (s != TGX_OK) throw AnalyzerError::query(std::string(tgx_status_name(s)) + ": " + err.msg);
  };
  check(tgx_group_counts_get(plan, state, spec_index, &out.summary, &err));
  uint64_t n = 0, nb = 0;
  int32_t is_bytes = 0;
  check(tgx_group_counts_entries(plan, state, spec_index, nullptr, 0, &n, nullptr, 0, &nb, &is_bytes, &err));
  std::vector<tgx_group_count_entry> entries((size_t)n + 1);
  std::vector<uint8_t> bytes((size_t)nb + 1);
  check(tgx_group_counts_entries(plan, state, spec_index, entries.data(), n, &n, bytes.data(), nb, &nb, &is_bytes, &err));
  out.is_bytes = is_bytes != 0;
  for (uint64_t i = 0; i < n; i++) {
    const tgx_group_count_entry &e = entries[i];
    GroupCounts::Entry o;
    o.value = e.value;
    if (out.is_bytes) o.bytes.assign((const char *)bytes.data() + e.offset, (size_t)e.length);
    o.total = e.total;
    o.non_null = e.non_null;
    out.entries.push_back(std::move(o));
  }
  return out;
}

std::shared_ptr<Analyzer> completeness_with_grouping(const std::string &column, const GroupingConfig &config,
                                                     bool strict_reference_types, const std::string &group_arrow_type,
                                                     const std::vector<std::string> &group_arrow_types) {
  return std::make_shared<GroupedCompletenessAnalyzer>(column, config, strict_reference_types, group_arrow_type,
                                                       group_arrow_types);
}

std::shared_ptr<Analyzer> analyzer_from_json(const json::Value &v) {
  const std::string t = v.get_str("type");
  auto col = [&]() {
    const std::string c = v.get_str("column");
    if (c.empty()) throw TermError{TermError::Internal, "analyzer '" + t + "' needs a column"};
    return c;
  };
  if (t == "size") return std::make_shared<SizeAnalyzer>();
  if (t == "completeness") return std::make_shared<CompletenessAnalyzer>(col());
  if (t == "distinctness") return std::make_shared<DistinctnessAnalyzer>(col());
  if (t == "approx_count_distinct") return std::make_shared<ApproxCountDistinctAnalyzer>(col());
  if (t == "mean") return std::make_shared<MeanAnalyzer>(col());
  if (t == "min") return std::make_shared<MinMaxAnalyzer>(col(), false);
  if (t == "max") return std::make_shared<MinMaxAnalyzer>(col(), true);
  if (t == "sum") return std::make_shared<SumAnalyzer>(col());
  if (t == "standard_deviation") return std::make_shared<StandardDeviationAnalyzer>(col());
  if (t == "correlation") {
    const std::string m = v.get_str("method", "pearson");
    CorrelationAnalyzer::Type ct = m == "pearson"      ? CorrelationAnalyzer::Pearson
                                   : m == "spearman"   ? CorrelationAnalyzer::Spearman
                                   : m == "covariance" ? CorrelationAnalyzer::Covariance
                                                       : throw TermError{TermError::Internal, "unknown correlation method '" + m + "'"};
    if (v.get_str("column1").empty() || v.get_str("column2").empty())
      throw TermError{TermError::Internal, "correlation needs column1 and column2"};
    return std::make_shared<CorrelationAnalyzer>(v.get_str("column1"), v.get_str("column2"), ct);
  }
  if (t == "mutual_information") {
    if (v.get_str("column1").empty() || v.get_str("column2").empty())
      throw TermError{TermError::Internal, "mutual_information needs column1 and column2"};
    std::optional<uint64_t> max_pairs;
    if (const json::Value *mp = v.get("max_pairs"))
      if (mp->type != json::Value::Null) max_pairs = mp->as_u64();
    std::vector<std::string> arrow_types;
    if (const json::Value *at = v.get("arrow_types"))
      if (at->type == json::Value::Array)
        for (const json::Value &e : at->arr) arrow_types.push_back(e.type == json::Value::String ? e.str : std::string());
    return std::make_shared<MutualInformationAnalyzer>(v.get_str("column1"), v.get_str("column2"), v.get_u64("bins", 10),
                                                       max_pairs, v.get_u64("max_value_bytes", TGX_PAIR_COUNTS_MAX_VALUE_BYTES),
                                                       arrow_types);
  }
  if (t == "histogram")
    return std::make_shared<HistogramAnalyzer>(col(), v.get_u64("num_buckets", 10), v.get_bool("strict_reference_types", true));
  if (t == "grouped_completeness") {
    GroupingConfig cfg;
    if (const json::Value *g = v.get("group_by"))
      if (g->type == json::Value::Array)
        for (const json::Value &e : g->arr) cfg.columns.push_back(e.type == json::Value::String ? e.str : std::string());
    if (const json::Value *mg = v.get("max_groups")) {
      if (mg->type == json::Value::Null) cfg.max_groups.reset();
      else cfg.max_groups = mg->as_u64();
    }
    cfg.include_overall = v.get_bool("include_overall", true);
    cfg.composite_on_device = v.get_bool("composite_groups_on_device", false);
    std::vector<std::string> group_arrow_types;
    if (const json::Value *at = v.get("group_arrow_types"))
      if (at->type == json::Value::Array)
        for (const json::Value &e : at->arr) group_arrow_types.push_back(e.type == json::Value::String ? e.str : std::string());
    return completeness_with_grouping(col(), cfg, v.get_bool("strict_reference_types", true), v.get_str("group_arrow_type"),
                                      group_arrow_types);
  }
  if (t == "compliance")
    return std::make_shared<ComplianceAnalyzer>(v.get_str("name"), v.get_str("predicate"),
                                                v.get("string_functions_on_device") && v.get_bool("string_functions_on_device"));
  if (t == "data_type") return std::make_shared<DataTypeAnalyzer>(col(), v.get_str("arrow_type"));
  // ("entropy" stays an unknown type: the tag of EntropyAnalyzer is "value_entropy")
  if (t == "value_entropy")
    return std::make_shared<EntropyAnalyzer>(col(), v.get_u64("max_unique_values", 10000), v.get_str("arrow_type"));
  throw TermError{TermError::Internal, "unknown analyzer type '" + t + "'"};
}

// ---------------------------------------------------------------- runner
AnalyzerContext AnalysisRunner::run(const Context &ctx) const {
  AnalyzerContext out;
  const Table *table = ctx.table(table_name_);
  auto column_index = [&](const std::string &name) -> int {
    if (!table) return -1;
    for (size_t i = 0; i < table->column_names.size(); i++)
      if (table->column_names[i] == name) return (int)i;
    return -1;
  };
  struct Planned {
    std::vector<SpecRequest> reqs;
    std::vector<size_t> spec_index;
    std::vector<int> column_types;
    std::optional<std::string> error;
  };
  std::vector<Planned> planned(analyzers_.size());
  std::vector<SpecRequest> requests;
  for (size_t a = 0; a < analyzers_.size(); a++) {
    Planned &p = planned[a];
    if (!table) {
      p.error = AnalyzerError::query("Error during planning: table 'datafusion.public." + table_name_ + "' not found").text;
      continue;
    }
    std::vector<std::string> declared;
    for (const std::string &c : analyzers_[a]->columns()) {
      int ci = column_index(c);
      int type = 0;
      if (ci >= 0)
        for (const Batch &b : table->batches)
          if (type == 0) type = b.columns[ci].type;
      p.column_types.push_back(type);
      declared.push_back(ci >= 0 && (size_t)ci < table->arrow_types.size() ? table->arrow_types[ci] : std::string());
    }
    std::vector<SpecRequest> wanted;
    try {
      wanted = analyzers_[a]->plan_for(p.column_types, declared);
    } catch (const AnalyzerError &e) {
      p.error = e.text;
      continue;
    }
    for (SpecRequest r : wanted) {
      if (r.column.empty() && !table->column_names.empty()) r.column = table->column_names[0];  // COUNT(*)
      for (const std::string *c : {&r.column, &r.column2}) {
        if (c == &r.column2 && r.column2.empty()) continue;
        if (column_index(*c) < 0 && !p.error)
          p.error = AnalyzerError::query("Schema error: No field named " + *c + ".").text;
      }
      for (const std::string &c : r.columns)
        if (column_index(c) < 0 && !p.error) p.error = AnalyzerError::query("Schema error: No field named " + c + ".").text;
      if (p.error) break;
      p.reqs.push_back(r);
    }
    if (!p.error && analyzers_[a]->reads_value_counts()) {
      const std::string refusal = analyzers_[a]->value_text_refusal(p.column_types.empty() ? 0 : p.column_types[0]);
      if (!refusal.empty()) p.error = AnalyzerError::invalid_data(refusal).text;
    }
  }
  // one pass over the table for every analyzer that is still in the run: their requests fused and de-duplicated
  std::vector<tgx_check_spec> specs;
  std::deque<std::vector<int32_t>> list_columns;  // owns the column lists of the specs that have one
  auto fuse = [&]() {
    requests.clear();
    specs.clear();
    list_columns.clear();
    for (Planned &p : planned) {
      p.spec_index.clear();
      if (p.error) continue;
      for (const SpecRequest &r : p.reqs) {
        size_t found = requests.size();
        for (size_t i = 0; i < requests.size(); i++)
          if (requests[i].kind == r.kind && requests[i].column == r.column && requests[i].column2 == r.column2 &&
              requests[i].columns == r.columns && requests[i].flags == r.flags && requests[i].same_parameters(r))
            found = i;
        if (found == requests.size()) requests.push_back(r);
        p.spec_index.push_back(found);
      }
    }
    for (const SpecRequest &r : requests) {
      tgx_check_spec s;
      memset(&s, 0, sizeof(s));
      s.kind = r.kind;
      s.column = column_index(r.column);
      s.column2 = r.column2.empty() ? -1 : column_index(r.column2);
      s.flags = r.flags;
      if (r.kind == TGX_CHECK_DISTINCT) s.flags |= TGX_FLAG_EXACT_KEYS;  // DistinctnessAnalyzer counts by value
      // (the kinds of this runner that name columns through a list: a predicate's, and a GROUP BY over several)
      if (r.kind == TGX_CHECK_ROW_PREDICATE || (r.kind == TGX_CHECK_GROUP_COUNTS && !r.columns.empty())) {
        list_columns.emplace_back();
        for (const std::string &c : r.columns) list_columns.back().push_back(column_index(c));
        s.columns = list_columns.back().data();
        s.n_columns = (uint32_t)list_columns.back().size();
      }
      specs.push_back(s);
    }
  };
  Handles h;
  std::vector<tgx_result> results;
  std::optional<std::string> run_error;
  // `follow_ups`: the follow-up pass -- spec i is a two-phase check that these parameters put into its count phase
  auto pass = [&](Handles &hh, size_t max_rows, tgx_status *status,
                  const std::vector<FollowUp> *follow_ups = nullptr) -> std::optional<std::string> {
    tgx_error err;
    memset(&err, 0, sizeof(err));
    tgx_status s = tgx_init(nullptr, &err);
    if (s == TGX_OK) s = tgx_plan_create(specs.data(), specs.size(), &hh.plan, &err);
    for (size_t i = 0; s == TGX_OK && follow_ups && i < follow_ups->size(); i++) {
      const FollowUp &fu = (*follow_ups)[i];
      s = specs[i].kind == TGX_CHECK_HISTOGRAM
              ? tgx_plan_set_histogram_edges(hh.plan, i, fu.edges.data(), (uint32_t)(fu.edges.size() - 1), &err)
          : specs[i].kind == TGX_CHECK_PAIR_COUNTS ? tgx_plan_set_pair_counts(hh.plan, i, &fu.pair, &err)
                                                   : tgx_plan_set_joint_binning(hh.plan, i, &fu.binning, &err);
    }
    for (size_t i = 0; s == TGX_OK && !follow_ups && i < requests.size(); i++) {
      if (requests[i].value_rule) s = tgx_plan_set_value_rule(hh.plan, i, &*requests[i].value_rule, &err);
      if (s == TGX_OK && requests[i].value_counts)
        s = tgx_plan_set_value_counts(hh.plan, i, &*requests[i].value_counts, &err);
      if (requests[i].pair_counts) s = tgx_plan_set_pair_counts(hh.plan, i, &*requests[i].pair_counts, &err);
      if (s == TGX_OK && requests[i].group_counts)
        s = tgx_plan_set_group_counts(hh.plan, i, &*requests[i].group_counts, &err);
      if (s == TGX_OK && requests[i].row_predicate)
        s = tgx_plan_set_row_predicate(hh.plan, i, &*requests[i].row_predicate, &err);
    }
    if (s == TGX_OK) s = tgx_state_create(hh.plan, nullptr, &hh.state, &err);
    std::vector<tgx_column> cut;
    for (size_t b = 0; s == TGX_OK && b < table->batches.size(); b++) {
      const std::vector<tgx_column> &cols = table->batches[b].columns;
      if (max_rows == SIZE_MAX) {
        s = tgx_update(hh.plan, hh.state, cols.data(), cols.size(), &err);
      } else {  // (a probe: the first rows of the first batch)
        int64_t rows = 0;
        for (const tgx_column &c : cols) rows = std::max(rows, c.length);
        if (rows == 0 && b + 1 < table->batches.size()) continue;  // (an empty record batch says nothing)
        cut = cols;
        for (tgx_column &c : cut) c.length = std::min<int64_t>(c.length, (int64_t)max_rows);
        s = tgx_update(hh.plan, hh.state, cut.data(), cut.size(), &err);
        break;
      }
    }
    if (s == TGX_OK) {
      results.assign(specs.size(), tgx_result());
      s = tgx_finalize(hh.plan, hh.state, results.data(), results.size(), &err);
    }
    *status = s;
    if (s != TGX_OK) return AnalyzerError::query(std::string(tgx_status_name(s)) + ": " + err.msg).text;
    return std::nullopt;
  };
  fuse();
  if (!specs.empty()) {
    tgx_status status = TGX_OK;
    run_error = pass(h, SIZE_MAX, &status);
    if (run_error && (status == TGX_UNSUPPORTED || status == TGX_INVALID_ARGUMENT)) {
      // one analyzer the library refuses (a column type outside the path) keeps the refusal as ITS error -- the
      // reference runs every analyzer as a query of its own (runner.rs:141-201) -- and the others run again as one pass:
      // every analyzer's requests are tried alone on the table's first row (term_guard.cpp, ValidationSuite::run)
      std::vector<std::optional<std::string>> saved;
      for (const Planned &p : planned) saved.push_back(p.error);
      size_t refused = 0;
      for (size_t k = 0; k < planned.size(); k++) {
        if (saved[k]) continue;
        for (size_t j = 0; j < planned.size(); j++)
          if (j != k && !planned[j].error) planned[j].error = std::string();  // (not part of this probe)
        fuse();
        Handles probe;
        tgx_status ps = TGX_OK;
        const std::optional<std::string> pe = specs.empty() ? std::nullopt : pass(probe, 1, &ps);
        for (size_t j = 0; j < planned.size(); j++) planned[j].error = saved[j];
        if (pe && (ps == TGX_UNSUPPORTED || ps == TGX_INVALID_ARGUMENT)) {
          planned[k].error = saved[k] = pe;
          refused++;
        }
      }
      fuse();
      if (refused) {
        h.reset();
        run_error.reset();
        if (!specs.empty()) run_error = pass(h, SIZE_MAX, &status);
      }
    }
  }
  // The second pass (analyzers.h, Analyzer::follow_up): the analyzers whose first-pass results are in say what their
  // follow-up request is; all of those run as ONE more pass over the table.  A run without such an analyzer makes one pass.
  struct Followed {
    FirstPass first;
    bool counted = false;
    SecondPass second;
  };
  std::vector<Followed> followed(analyzers_.size());
  if (!run_error && h.state) {
    std::vector<size_t> owners;
    std::vector<FollowUp> follow_ups;
    std::vector<tgx_check_spec> first_specs = specs;
    for (size_t a = 0; a < analyzers_.size(); a++) {
      if (!analyzers_[a]->two_pass() || planned[a].error || planned[a].spec_index.empty()) continue;
      tgx_error err;
      memset(&err, 0, sizeof(err));
      FirstPass &first = followed[a].first;
      first.kind = specs[planned[a].spec_index[0]].kind;
      first.column_types = planned[a].column_types;
      if (first.kind == TGX_CHECK_PAIR_COUNTS) {
        // string x string: the first pass counted the pairs, there is no follow-up
        const tgx_pair_counts_params &pp = *requests[planned[a].spec_index[0]].pair_counts;
        if (pp.x.mode != TGX_PAIR_SIDE_RANGE && pp.y.mode != TGX_PAIR_SIDE_RANGE) {
          try {
            followed[a].second.pairs = read_pair_counts(h.plan, h.state, planned[a].spec_index[0], pp);
            followed[a].counted = true;
          } catch (const AnalyzerError &e) {
            planned[a].error = e.text;
          }
          continue;
        }
      }
      const tgx_status s = first.kind == TGX_CHECK_HISTOGRAM
                               ? tgx_histogram_range_get(h.plan, h.state, planned[a].spec_index[0], &first.histogram, &err)
                           : first.kind == TGX_CHECK_PAIR_COUNTS
                               ? tgx_pair_range_get(h.plan, h.state, planned[a].spec_index[0], &first.pair, &err)
                               : tgx_joint_range_get(h.plan, h.state, planned[a].spec_index[0], &first.joint, &err);
      if (s != TGX_OK) {
        planned[a].error = AnalyzerError::query(std::string(tgx_status_name(s)) + ": " + err.msg).text;
        continue;
      }
      try {
        if (std::optional<FollowUp> fu = analyzers_[a]->follow_up(first)) {
          owners.push_back(a);
          follow_ups.push_back(std::move(*fu));
        }
      } catch (const AnalyzerError &e) {
        planned[a].error = e.text;
      }
    }
    if (!owners.empty()) {
      specs.clear();
      for (size_t a : owners) specs.push_back(first_specs[planned[a].spec_index[0]]);
      Handles second;
      tgx_status status = TGX_OK;
      const std::vector<tgx_result> first_results = results;
      std::optional<std::string> second_error = pass(second, SIZE_MAX, &status, &follow_ups);
      results = first_results;
      for (size_t k = 0; k < owners.size(); k++) {
        Followed &fo = followed[owners[k]];
        tgx_error err;
        memset(&err, 0, sizeof(err));
        if (!second_error) {
          tgx_status s = TGX_OK;
          if (fo.first.kind == TGX_CHECK_PAIR_COUNTS) {
            try {
              fo.second.pairs = read_pair_counts(second.plan, second.state, k, follow_ups[k].pair);
            } catch (const AnalyzerError &e) {
              second_error = e.text;
            }
          } else if (fo.first.kind == TGX_CHECK_HISTOGRAM) {
            fo.second.buckets.assign(follow_ups[k].edges.size() - 1, 0);
            s = tgx_histogram_counts(second.plan, second.state, k, fo.second.buckets.data(), fo.second.buckets.size(),
                                     nullptr, nullptr, &err);
          } else {
            JointCounts &jc = fo.second.joint;
            uint64_t n_cells = 0;
            jc.bins = follow_ups[k].binning.bins;
            jc.cells.assign((size_t)(jc.bins + 1) * (jc.bins + 1), 0);
            s = tgx_joint_counts(second.plan, second.state, k, jc.cells.data(), jc.cells.size(), &n_cells,
                                 &jc.out_of_range, &err);
          }
          if (s != TGX_OK) second_error = AnalyzerError::query(std::string(tgx_status_name(s)) + ": " + err.msg).text;
        }
        if (second_error)
          planned[owners[k]].error = second_error;
        else
          fo.counted = true;
      }
      specs = first_specs;
    }
  }
  for (size_t a = 0; a < analyzers_.size(); a++) {
    const Analyzer &an = *analyzers_[a];
    std::optional<std::string> error = planned[a].error ? planned[a].error : run_error;
    if (!error) {
      try {
        std::vector<const tgx_result *> r;
        for (size_t si : planned[a].spec_index) r.push_back(&results[si]);
        json::Value st;
        if (an.reads_value_counts()) {
          try {
            st = an.state_from_value_counts(read_value_counts(h.plan, h.state, planned[a].spec_index[0]));
          } catch (const TermError &e) {
            throw AnalyzerError::query(e.display());
          }
        } else if (an.reads_group_counts()) {
          st = an.state_from_group_counts(read_group_counts(h.plan, h.state, planned[a].spec_index[0]));
        } else if (!planned[a].reqs.empty() && planned[a].reqs[0].kind == TGX_CHECK_TYPE_CLASSES) {
          tgx_type_classes_counts counts;
          tgx_error err;
          memset(&err, 0, sizeof(err));
          const tgx_status s = tgx_type_classes_get(h.plan, h.state, planned[a].spec_index[0], &counts, &err);
          if (s != TGX_OK) throw AnalyzerError::query(std::string(tgx_status_name(s)) + ": " + err.msg);
          st = an.state_from_type_classes(counts);
        } else {
          st = an.two_pass()
                   ? an.state_from_follow_up(followed[a].first, followed[a].counted ? &followed[a].second : nullptr)
                   : an.state_from_results(r, planned[a].column_types);
        }
        MetricValue m = an.metric_from_state(st);
        out.states.push_back({an.metric_key(), st});
        // context.rs:71-73: a later analyzer with the same key replaces the earlier metric
        bool replaced = false;
        for (auto &kv : out.metrics)
          if (kv.first == an.metric_key()) {
            kv.second = m;
            replaced = true;
          }
        if (!replaced) out.metrics.push_back({an.metric_key(), m});
      } catch (const AnalyzerError &e) {
        error = e.text;
      }
    }
    if (error) {
      out.errors.push_back({an.name(), *error});  // runner.rs:172-175
      if (!continue_on_error_) throw AnalyzerError::custom("Analyzer " + an.name() + " failed");  // :177-181
    }
  }
  return out;
}

}  // namespace term_guard
