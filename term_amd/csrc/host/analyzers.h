// analyzers.h -- host-side mirror of term-guard's Analyzer / AnalyzerState / AnalysisRunner surface
// (TG/analyzers/traits.rs:65-179, TG/analyzers/runner.rs:64-202, TG/analyzers/context.rs:35-128).
//
// The reference runs every analyzer as its own SQL scan (runner.rs:141-165, "TODO: group compatible analyzers");
// here AnalysisRunner::run plans ALL analyzers into one tgx_plan, feeds the table once and lets each analyzer
// turn the shared aggregates into its state and metric.  States keep the reference's serde field names, so a
// state JSON produced here can be merged / turned into a metric exactly as AnalyzerState::merge and
// Analyzer::compute_metric_from_state do -- those two halves need no device.
#pragma once
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "json.h"
#include "term_guard.h"
#include "value_counts.h"

namespace term_guard {

// TG/analyzers/types.rs:13-35 (serde: {"type": "Double", "value": 0.8})
struct HistogramBucket {  // types.rs:158-169
  double lower_bound = 0, upper_bound = 0;
  uint64_t count = 0;
};
struct MetricDistribution {  // types.rs:95-157; the statistics are Options there (null when absent)
  std::vector<HistogramBucket> buckets;
  uint64_t total_count = 0;
  std::optional<double> min, max, mean, std_dev;
};
struct MetricValue {
  enum Kind { Double, Long, Map, Histogram, Boolean, String } kind = Double;
  double d = 0;
  std::string s;  // String
  int64_t l = 0;
  bool b = false;
  std::vector<std::pair<std::string, MetricValue>> map;  // insertion ordered (the reference's HashMap is unordered)
  MetricDistribution histogram;
  static MetricValue of_double(double v) {
    MetricValue m;
    m.kind = Double;
    m.d = v;
    return m;
  }
  static MetricValue of_bool(bool v) {
    MetricValue m;
    m.kind = Boolean;
    m.b = v;
    return m;
  }
  static MetricValue of_string(std::string v) {
    MetricValue m;
    m.kind = String;
    m.s = std::move(v);
    return m;
  }
  static MetricValue of_long(int64_t v) {
    MetricValue m;
    m.kind = Long;
    m.l = v;
    return m;
  }
  std::string to_json() const;
};

// TG/analyzers/errors.rs:10-50 -- what(): the reference's Display text
struct AnalyzerError {
  std::string text;
  static AnalyzerError no_data() { return {"No data available for analysis"}; }
  static AnalyzerError invalid_data(const std::string &m) { return {"Invalid data: " + m}; }
  static AnalyzerError state_merge(const std::string &m) { return {"Failed to merge states: " + m}; }
  static AnalyzerError query(const std::string &m) { return {"Query execution failed: " + m}; }
  static AnalyzerError custom(const std::string &m) { return {m}; }
};

// The two passes of a two-pass analyzer (AnalysisRunner::run).  Its plan()[0] is ONE request of a two-phase check kind
// -- TGX_CHECK_JOINT_BINS or TGX_CHECK_HISTOGRAM -- and the members that belong to that kind are the ones in use.
struct JointCounts {
  uint32_t bins = 0;
  std::vector<uint64_t> cells;  // (bins + 1)^2, row-major (tgx_joint_counts)
  uint64_t out_of_range = 0;
};
// one spec's state as tgx_pair_counts_get / tgx_pair_counts_entries answer it, in the library's order
struct PairCell {
  bool binned = false;  // a binned side: `bin`; a string side: `bytes`
  int64_t bin = 0;
  std::string bytes;
};
struct PairCounts {
  tgx_pair_counts_summary summary = {};
  struct Entry {
    PairCell x, y;
    uint64_t count = 0;
  };
  std::vector<Entry> entries;
};
PairCounts read_pair_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                            const tgx_pair_counts_params &params);  // throws AnalyzerError (query)
// one spec's state as tgx_group_counts_get / tgx_group_counts_entries answer it, in the library's order (ascending by
// key); the NULL group is in the summary
struct GroupCounts {
  tgx_group_counts_summary summary = {};
  bool is_bytes = false;  // string keys: `bytes`; integer keys: `value`
  struct Entry {
    int64_t value = 0;
    std::string bytes;
    uint64_t total = 0, non_null = 0;
  };
  std::vector<Entry> entries;
};
GroupCounts read_group_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index);  // throws AnalyzerError (query)

// TG/analyzers/grouped.rs:14-95: how an analyzer's metric is computed per group.  Defaults: GroupingConfig::new
// (grouped.rs:32-39).  The overflow strategy is carried, not acted on: the reference's query orders by the metric
// descending and keeps the first max_groups whatever it says (grouped_completeness.rs:130-150).
enum class OverflowStrategy { TopK, BottomK, Sample, Fail };
struct GroupingConfig {
  std::vector<std::string> columns;
  std::optional<uint64_t> max_groups = 10000;
  bool include_overall = true;
  OverflowStrategy overflow_strategy = OverflowStrategy::TopK;
  // an opt-in: 2 .. 8 group columns are one TGX_CHECK_GROUP_COUNTS request on the tuple of the columns (off: more than
  // one group column is the analyzer's error, as it always was)
  bool composite_on_device = false;
  GroupingConfig &composite_groups_on_device(bool on) {
    composite_on_device = on;
    return *this;
  }
};
class Analyzer;
// CompletenessAnalyzer::with_grouping (grouped.rs:200-210, basic/grouped_completeness.rs): the one grouped analyzer.
// strict_reference_types: only a group column declared Utf8 is taken (see the class in analyzers.cpp)
std::shared_ptr<Analyzer> completeness_with_grouping(const std::string &column, const GroupingConfig &config,
                                                     bool strict_reference_types = true,
                                                     const std::string &group_arrow_type = std::string(),
                                                     const std::vector<std::string> &group_arrow_types = {});

struct FirstPass {  // what the request's range phase found
  int kind = 0;                   // the kind of plan()[0]
  std::vector<int> column_types;  // tgx_type of columns() in order
  tgx_joint_range joint = {};
  tgx_histogram_range histogram = {};
  tgx_pair_range pair = {};       // PAIR_COUNTS with a side in its range phase
};
struct FollowUp {  // the parameters that put the request into its count phase
  tgx_joint_binning binning = {};  // JOINT_BINS (tgx_plan_set_joint_binning)
  std::vector<double> edges;       // HISTOGRAM (tgx_plan_set_histogram_edges): buckets + 1
  tgx_pair_counts_params pair = {};  // PAIR_COUNTS (tgx_plan_set_pair_counts): the range side now binned
};
struct SecondPass {  // what the request's count phase found
  JointCounts joint;
  std::vector<uint64_t> buckets;  // HISTOGRAM (tgx_histogram_counts)
  PairCounts pairs;               // PAIR_COUNTS; a string x string request is counted by the FIRST pass and lands here too
};

class Analyzer {
 public:
  virtual ~Analyzer() {}
  virtual std::string name() const = 0;
  virtual std::string metric_key() const { return name(); }  // traits.rs:133-135
  virtual std::vector<std::string> columns() const { return {}; }
  // aggregates this analyzer needs (its half of the fused plan)
  virtual std::vector<SpecRequest> plan() const = 0;
  // ... where the plan depends on what the columns hold (column_types: tgx_type of columns() in order; 0 = unknown).
  // MutualInformationAnalyzer with "max_pairs" plans TGX_CHECK_PAIR_COUNTS when a column is a string one.  Throws
  // AnalyzerError for a column the analyzer refuses before the device sees it.
  // `declared`: the columns' Arrow DataType names where the caller holds them (Table::arrow_types), else empty strings.
  virtual std::vector<SpecRequest> plan_for(const std::vector<int> & /*column_types*/,
                                            const std::vector<std::string> & /*declared*/) const {
    return plan();
  }
  // the state of an analyzer whose request is a TGX_CHECK_PAIR_COUNTS one, from the pairs the device counted
  virtual json::Value state_from_pair_counts(const PairCounts &) const { return json::Value(); }
  // compute_state_from_data's second half: aggregates (answering plan() in order) -> state (serde field names).
  // column_types: tgx_type of columns() in order (the reference's downcasts depend on the SQL result type).
  virtual json::Value state_from_results(const std::vector<const tgx_result *> &r,
                                         const std::vector<int> &column_types) const = 0;
  // A SECOND PASS over the table, for aggregates whose parameters depend on the first pass's results (bin edges from
  // the table's MIN / MAX: the reference's MutualInformationAnalyzer and HistogramAnalyzer run two queries,
  // mutual_information.rs:143-248, histogram.rs:184-330).  An analyzer that overrides follow_up() has ONE request of a
  // two-phase kind as plan()[0]; once the first pass is in, the runner hands it that request's range and gets the
  // parameters of the follow-up request back (nullopt: no rows, no second pass; throws AnalyzerError when the range
  // has none), runs ALL follow-up requests of the run as one more fused pass and builds the state with
  // state_from_follow_up (the SecondPass is nullptr when there was no second pass).
  // An analyzer whose plan()[0] is a TGX_CHECK_VALUE_COUNTS request (EntropyAnalyzer) builds its state from the entries
  // the device counted, not from a tgx_result (host/value_counts.h).  value_text_refusal(): what is wrong with reading
  // the column's values as text, asked before the device sees the column ("" when nothing is)
  virtual bool reads_value_counts() const { return false; }
  virtual std::string value_text_refusal(int /*tgx_type of the column*/) const { return std::string(); }
  virtual json::Value state_from_value_counts(const ValueCounts &) const { return json::Value(); }
  // An analyzer whose plan()[0] is a TGX_CHECK_GROUP_COUNTS request (the grouped CompletenessAnalyzer) builds its state
  // from the groups the device counted
  virtual bool reads_group_counts() const { return false; }
  virtual json::Value state_from_group_counts(const GroupCounts &) const { return json::Value(); }
  // An analyzer whose planned request is a TGX_CHECK_TYPE_CLASSES one (DataTypeAnalyzer on a string column) builds its
  // state from the nine counters of tgx_type_classes_get
  virtual json::Value state_from_type_classes(const tgx_type_classes_counts &) const { return json::Value(); }
  virtual bool two_pass() const { return false; }
  virtual std::optional<FollowUp> follow_up(const FirstPass &) const { return std::nullopt; }
  virtual json::Value state_from_follow_up(const FirstPass &, const SecondPass *) const { return json::Value(); }
  virtual json::Value merge_states(const std::vector<json::Value> &states) const = 0;      // AnalyzerState::merge
  virtual MetricValue metric_from_state(const json::Value &state) const = 0;              // throws AnalyzerError
};

std::shared_ptr<Analyzer> analyzer_from_json(const json::Value &v);  // throws TermError on malformed input
std::string json_dump(const json::Value &v);

struct AnalyzerContext {  // context.rs:35-44
  std::vector<std::pair<std::string, MetricValue>> metrics;  // key -> value, in execution order
  std::vector<std::pair<std::string, json::Value>> states;   // key -> state (not in the reference's context; for merges)
  std::vector<std::pair<std::string, std::string>> errors;   // (analyzer_name, error text)
  std::string to_json() const;
};

class AnalysisRunner {  // runner.rs:64-202
 public:
  AnalysisRunner &add(std::shared_ptr<Analyzer> a) {
    analyzers_.push_back(std::move(a));
    return *this;
  }
  AnalysisRunner &continue_on_error(bool c) {
    continue_on_error_ = c;
    return *this;
  }
  AnalysisRunner &table_name(std::string t) {
    table_name_ = std::move(t);
    return *this;
  }
  size_t analyzer_count() const { return analyzers_.size(); }
  // throws AnalyzerError ("Analyzer {name} failed") when an analyzer fails and continue_on_error is off
  AnalyzerContext run(const Context &ctx) const;

 private:
  std::vector<std::shared_ptr<Analyzer>> analyzers_;
  bool continue_on_error_ = true;   // runner.rs:71
  std::string table_name_ = "data";  // core/validation_context.rs default
};

}  // namespace term_guard
