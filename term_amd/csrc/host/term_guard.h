// term_guard.h -- host-side mirror of term-guard's ValidationSuite / Check / Constraint surface, driving
// libtgx instead of DataFusion.
//
// Same names, argument meaning, verdict rules and messages as the reference (cited per item, paths
// relative to /root/reference/term-guard/src):
//   ValidationSuite::builder(..).table_name(..).check(..).build().run(..)   core/suite.rs:351-600
//   Check::builder(..).level(..).completeness(..).has_min(..) ...           core/check.rs:172-2310
//   Constraint / ConstraintResult / ConstraintStatus                        core/constraint.rs:13-225
//   Assertion                                                               constraints/assertion.rs:27-76
//   LogicalOperator / ConstraintOptions                                     core/logical.rs:32-100, core/unified.rs
//   ValidationResult / Report / Metrics / Issue, Level                      core/result.rs, core/level.rs
// What differs by design: where the reference runs one SQL scan per constraint (core/suite.rs:67-100),
// run() plans every constraint's aggregates into ONE tgx_plan, feeds each batch once and then lets each
// constraint apply its own verdict to the shared results.  The DataFusion SessionContext is replaced by
// `Context`, a registry of named tables whose batches are Arrow-layout column views (host or device).
#pragma once
#include <string.h>

#include <functional>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../../../include/tgx.h"

namespace term_guard {

// ---- core/level.rs:76-117
enum class Level { Info, Warning, Error };
const char *level_str(Level l);

// ---- core/constraint.rs:13-99
enum class ConstraintStatus { Success, Failure, Skipped };
struct ConstraintResult {
  ConstraintStatus status = ConstraintStatus::Success;
  std::optional<double> metric;
  std::optional<std::string> message;
  static ConstraintResult success() { return {ConstraintStatus::Success, {}, {}}; }
  static ConstraintResult success_with_metric(double m) { return {ConstraintStatus::Success, m, {}}; }
  static ConstraintResult failure(std::string msg) { return {ConstraintStatus::Failure, {}, std::move(msg)}; }
  static ConstraintResult failure_with_metric(double m, std::string msg) {
    return {ConstraintStatus::Failure, m, std::move(msg)};
  }
  static ConstraintResult skipped(std::string msg) { return {ConstraintStatus::Skipped, {}, std::move(msg)}; }
};

// TermError (error.rs:14-145): only the variants this path produces
struct TermError {
  // ConstraintEvaluation: `message` starts with the quoted constraint name ("'temporal_ordering': ..", error.rs:28)
  enum Kind { Internal, SecurityError, DataFusion, NotSupported, Configuration, TypeMismatch, ConstraintEvaluation,
              ValidationFailed } kind = Internal;
  std::string message;
  std::string display() const;  // thiserror Display strings, e.g. "Security error: ..."
};

// ---- constraints/assertion.rs:27-76
struct Assertion {
  enum Kind { Equals, NotEquals, GreaterThan, GreaterThanOrEqual, LessThan, LessThanOrEqual, Between, NotBetween };
  Kind kind;
  double a = 0, b = 0;
  static Assertion equals(double v) { return {Equals, v, 0}; }
  static Assertion not_equals(double v) { return {NotEquals, v, 0}; }
  static Assertion greater_than(double v) { return {GreaterThan, v, 0}; }
  static Assertion greater_than_or_equal(double v) { return {GreaterThanOrEqual, v, 0}; }
  static Assertion less_than(double v) { return {LessThan, v, 0}; }
  static Assertion less_than_or_equal(double v) { return {LessThanOrEqual, v, 0}; }
  static Assertion between(double lo, double hi) { return {Between, lo, hi}; }
  static Assertion not_between(double lo, double hi) { return {NotBetween, lo, hi}; }
  bool evaluate(double value) const;
  std::string description() const;
};

// Rust's `{}` for f64 (shortest round-trip digits, never scientific notation)
std::string rust_f64(double v);

// ---- core/logical.rs:32-100
struct LogicalOperator {
  enum Kind { All, Any, Exactly, AtLeast, AtMost } kind = All;
  size_t n = 0;
  bool evaluate(const std::vector<bool> &results) const;
  std::string description() const;
};

// ---- security.rs:89-255
std::optional<TermError> validate_identifier(const std::string &identifier);

// ---- constraints/format.rs:160-390
struct FormatType {
  enum Kind { Regex, Email, Url, CreditCard, Phone, PostalCode, UUID, IPv4, IPv6, Json, Iso8601DateTime,
              SocialSecurityNumber } kind = Regex;
  std::string pattern;        // Regex
  bool allow_localhost = false;
  bool detect_only = false;
  std::optional<std::string> country;  // Phone (optional) / PostalCode (required)
  std::string get_pattern() const;     // format.rs:217-307
  std::string name() const;            // :310-325
  std::string description() const;     // :328-360
};
struct FormatOptions {
  bool case_sensitive = true, trim_before_check = false, null_is_valid = true;  // format.rs:376-384
};

// ---- constraints/uniqueness.rs:56-140
enum class NullHandling { Exclude, Include, Distinct };
struct UniquenessType {
  enum Kind { FullUniqueness, Distinctness, UniqueValueRatio, PrimaryKey, UniqueWithNulls } kind = FullUniqueness;
  double threshold = 1.0;
  std::optional<Assertion> assertion;
  NullHandling null_handling = NullHandling::Exclude;
  std::string name() const;
};

// ---- constraints/statistics.rs:24-108
struct StatisticType {
  enum Kind { Min, Max, Mean, Sum, StandardDeviation, Variance, Median, Percentile } kind = Min;
  double p = 0.5;
  std::string name() const;             // "minimum", ...
  std::string constraint_name() const;  // "min", ...
};

// ---- constraints/quantile.rs:36-112
struct QuantileCheck {
  double quantile = 0.5;
  Assertion assertion = Assertion::equals(0);
};
struct QuantileValidation {
  enum Kind { Single, Multiple, Distribution, Monotonic, Custom } kind = Single;
  std::vector<QuantileCheck> checks;  // Single: one entry; Multiple: one per quantile
  std::vector<double> quantiles;      // Monotonic
  bool strict = false;                // Monotonic
};

// ---- constraints/correlation.rs:19-117
struct CorrelationType {
  enum Kind { Pearson, Spearman, KendallTau, MutualInformation, Covariance, Custom } kind = Pearson;
  std::string sql_expression;        // Custom
  std::string name() const;             // "Pearson correlation", ...  (:39-48)
  std::string constraint_name() const;  // "correlation", ...          (:51-60)
};
struct CorrelationValidation {
  enum Kind { Pairwise, Range, MultiColumn, Independence, Stability } kind = Pairwise;
  std::string column1, column2;
  CorrelationType type;                       // Pairwise / Range
  Assertion assertion = Assertion::equals(0);  // Pairwise
  double min = 0, max = 0;                    // Range
  double max_correlation = 0;                 // Independence
  std::vector<std::string> columns;           // MultiColumn (needs >= 2)
};

// The unit-free parameters of a TGX_CHECK_TEMPORAL request (host/temporal.h turns them, with the columns' Arrow types,
// into tgx_temporal_params): seconds, "HH:MM", TIMESTAMP literal texts.  A TGX_CHECK_TIME_GAP request (MaxTimeGap with
// window_on_device) carries kTemporalTimeGapMode and max_gap_seconds; host/temporal.h turns them into tgx_time_gap_params
constexpr int kTemporalTimeGapMode = 4;  // (host side only: not a mode of tgx_temporal_params)
struct TemporalRequest {
  int mode = 0;  // TGX_TEMPORAL_ORDER / _TIME_OF_DAY / _RANGE, or kTemporalTimeGapMode
  bool allow_equal = false, allow_nulls = false, weekdays_only = false;
  int64_t tolerance_seconds = 0;
  int64_t max_gap_seconds = 0;               // kTemporalTimeGapMode
  std::string start_time, end_time;          // "HH:MM"
  std::optional<std::string> min_date, max_date;
  bool operator==(const TemporalRequest &o) const {
    return mode == o.mode && allow_equal == o.allow_equal && allow_nulls == o.allow_nulls &&
           weekdays_only == o.weekdays_only && tolerance_seconds == o.tolerance_seconds && start_time == o.start_time &&
           end_time == o.end_time && min_date == o.min_date && max_date == o.max_date &&
           max_gap_seconds == o.max_gap_seconds;
  }
};

// One aggregate a constraint needs; the suite runner resolves column names and fuses all requests.
struct SpecRequest {
  int kind = 0;  // tgx_check_kind
  std::string column, column2;
  std::vector<std::string> columns;  // DISTINCT over a tuple of columns (then `column` is columns[0]); GROUP_COUNTS by
                                     // the tuple of these columns (`column` stays the value column, `column2` is empty)
  uint32_t flags = 0;
  std::string pattern;
  uint32_t kll_k = 0;
  uint64_t length_min = 0, length_max = ~0ull;  // LENGTH: inclusive character-count bounds
  std::optional<TemporalRequest> temporal;      // TEMPORAL (`column2`: the after column in order mode) and TIME_GAP
                                                // (`column2`: the group column, or empty)
  std::optional<tgx_value_rule_params> value_rule;  // VALUE_RULE: the rule as the device takes it (host/datatype.h)
  std::optional<tgx_value_counts_params> value_counts;  // VALUE_COUNTS: the bounds (host/value_counts.h)
  std::optional<tgx_pair_counts_params> pair_counts;    // PAIR_COUNTS: the bounds and the sides (host/analyzers.cpp)
  std::optional<tgx_group_counts_params> group_counts;  // GROUP_COUNTS (`column2`: the group column): the bounds
  // ROW_PREDICATE (`columns`: the spec's column list, of any length from 1): the predicate as the device takes it
  // (host/custom_sql.h); what a leaf does not read is zero, so equal predicates are equal bytes
  std::optional<tgx_row_predicate_params> row_predicate;
  // do two requests ask the device for the same thing (what the runners' fusing compares beside kind and columns)?
  bool same_parameters(const SpecRequest &o) const {
    return value_rule.has_value() == o.value_rule.has_value() &&
           (!value_rule || memcmp(&*value_rule, &*o.value_rule, sizeof(tgx_value_rule_params)) == 0) &&
           value_counts.has_value() == o.value_counts.has_value() &&
           (!value_counts || (value_counts->max_distinct == o.value_counts->max_distinct &&
                              value_counts->max_value_bytes == o.value_counts->max_value_bytes)) &&
           pair_counts.has_value() == o.pair_counts.has_value() &&
           (!pair_counts || memcmp(&*pair_counts, &*o.pair_counts, sizeof(tgx_pair_counts_params)) == 0) &&
           group_counts.has_value() == o.group_counts.has_value() &&
           (!group_counts || (group_counts->max_groups == o.group_counts->max_groups &&
                              group_counts->max_value_bytes == o.group_counts->max_value_bytes)) &&
           row_predicate.has_value() == o.row_predicate.has_value() &&
           (!row_predicate || memcmp(&*row_predicate, &*o.row_predicate, sizeof(tgx_row_predicate_params)) == 0);
  }
};
struct ValueCounts;  // host/value_counts.h
class Histogram;
class Context;       // below: the SessionContext stand-in
struct Table;        // below: a registered table's batches

// ---- core/constraint.rs:187-225.  `evaluate(&SessionContext)` is split in two so scans can be fused:
// plan() says which aggregates are needed, evaluate() turns them into the verdict.
class Constraint {
 public:
  virtual ~Constraint() {}
  virtual std::string name() const = 0;
  virtual std::optional<std::string> column() const { return {}; }
  // throws TermError for what the reference reports as Err(...) from evaluate()
  virtual std::vector<SpecRequest> plan() const = 0;
  // results[i] answers plan()[i]; `quantile` evaluates a KLL request (index into plan()) at phi
  struct Inputs {
    std::vector<const tgx_result *> results;
    const void *ctx = nullptr;
    double (*quantile)(const void *ctx, size_t request_index, double phi) = nullptr;
    // reads a VALUE_COUNTS request (index into plan()): the counters and the entries, values as text; throws TermError
    void (*value_counts)(const void *ctx, size_t request_index, ValueCounts *out) = nullptr;
    // the Arrow DataType of the column request i reads, as the caller holds it ("Int64", "Int32", "Date32",
    // "Timestamp", "Float32", "UInt16", ...; empty = unknown, taken for Int64 / Float64), and whether the verdict
    // follows the reference's own extraction rule for it (reference_extracts below)
    std::vector<std::string> arrow_types;
    // ... and of the columns of request i's column list, in the list's order (empty for a request without a list)
    std::vector<std::vector<std::string>> list_arrow_types;
    bool strict_reference_types = true;
  };
  virtual ConstraintResult evaluate(const Inputs &in) const = 0;
  // A constraint whose reference turns a query's error into a verdict (CustomSqlConstraint: a Failure that carries the
  // error's text) says so here: `error` is what the run would otherwise report as this constraint's error -- a column
  // the table lacks, a batch the device refuses.  nullopt: the error stands
  virtual std::optional<ConstraintResult> failure_from_error(const std::string & /*error*/) const { return std::nullopt; }
  // A constraint that reads tables of its own (CrossTableSumConstraint) is no part of the suite's fused plan: plan() is
  // empty and ValidationSuite::run evaluates it beside the plan, against the Context.  Throws TermError as plan() does.
  virtual bool reads_context() const { return false; }
  virtual ConstraintResult evaluate_context(const Context &ctx) const;
};

// What DataFusion 50's aggregate hands back for a column of Arrow type `arrow_type`, and whether the reference can
// read it: StatisticalConstraint::evaluate downcasts the result column to Int64Array, then Float64Array, else
// Err("Failed to extract statistic value") (constraints/statistics.rs:277-308; MultiStatisticalConstraint pushes
// "Failed to compute {name}", :466-483).  MIN / MAX / APPROX_PERCENTILE_CONT keep the input type, SUM widens signed
// integers to Int64 and floats to Float64 (unsigned: UInt64), AVG / STDDEV / VARIANCE are Float64.  So on an Int32,
// Date32, Float32, Timestamp or UInt column the reference's has_min is an ERROR, not a verdict -- and with
// `strict_reference_types` (the default) so is this library's, although the kernels could answer (the widening
// behaviour is opt-in and listed as a deviation in INTEGRATION.md).
enum class StatisticResultKind { Min, Max, Mean, Sum, StandardDeviation, Variance, Quantile };
bool reference_extracts(StatisticResultKind stat, const std::string &arrow_type);
// QuantileConstraint reads Float64, Int64 or Int32 (constraints/quantile.rs:308-324), else TypeMismatch
bool reference_extracts_quantile(const std::string &arrow_type);

// ---- constraints/cross_table_sum.rs: SUM(left) against SUM(right), over the whole tables or per group of ONE group
// column.  Each side is one walk of its table on the device -- a TGX_CHECK_GROUP_SUMS spec (grouped) or a
// TGX_CHECK_NUMERIC_STATS spec (ungrouped) -- and the FULL OUTER JOIN of at most 65 536 groups a side runs on the host.
// One side's groups as the join takes them: COALESCE(SUM(col), 0.0) as a double per key, ascending by key
struct SideSums {
  bool is_bytes = false;                             // string keys (`bytes`), else integer keys (`value`)
  int arity = 0;                                     // 2 .. 8: GROUP BY a tuple of columns, `bytes` an encoded tuple key
                                                     // (group_key.h); 0: one group column.  The tuple join refuses a
                                                     // side whose arity is not the constraint's
  struct Group {
    int64_t value = 0;
    std::string bytes;
    double sum = 0;
  };
  std::vector<Group> groups;                         // ascending by key, as tgx_group_sums_entries gives them
  std::optional<double> null_group;                  // the rows with a NULL key, when there are any
  uint64_t overflow_rows = 0, long_rows = 0;         // rows beyond the bounds: no verdict on partial sums
};
struct CrossTableSumRow {                            // the reference's result row (:273-279)
  int64_t total_groups = 0, violating_groups = 0;
  double total_left_sum = 0, total_right_sum = 0, max_difference = 0;
};
class CrossTableSumConstraint : public Constraint {
 public:
  static constexpr uint32_t kDefaultMaxGroups = 65536;
  CrossTableSumConstraint(std::string left_column, std::string right_column)  // "table.column" each (:87-95)
      : left_(std::move(left_column)), right_(std::move(right_column)) {}
  CrossTableSumConstraint &group_by(std::vector<std::string> columns) { group_by_ = std::move(columns); return *this; }
  CrossTableSumConstraint &tolerance(double t) { tolerance_ = t < 0 ? -t : t; return *this; }  // (:129-132: abs)
  CrossTableSumConstraint &max_violations_reported(size_t n) { max_violations_ = n; return *this; }
  // this layer's own: the groups a side's table on the device is sized for (1 .. 65 536).  A side with rows beyond it
  // (overflow) or with keys longer than 256 bytes makes the constraint an error that names the bound
  CrossTableSumConstraint &max_groups(uint32_t n) { max_groups_ = n; return *this; }
  // an opt-in: 2 .. 8 group_by columns are one TGX_CHECK_GROUP_SUMS walk a side on the tuple of the columns, and the
  // outer join merges the two sides' entries by their encoded key bytes (off: several columns are an error, as ever)
  CrossTableSumConstraint &composite_groups_on_device(bool on) { composite_ = on; return *this; }
  bool composite_groups() const { return composite_; }
  // the opt-in given and 2 .. 8 group_by columns: the sides are tuple walks and join() merges encoded tuple keys
  bool groups_by_tuple() const { return composite_ && group_by_.size() >= 2 && group_by_.size() <= 8; }

  const std::string &left_column() const { return left_; }
  const std::string &right_column() const { return right_; }
  const std::vector<std::string> &group_by_columns() const { return group_by_; }
  double tolerance_value() const { return tolerance_; }
  size_t violations_reported() const { return max_violations_; }
  uint32_t groups_bound() const { return max_groups_; }

  std::string name() const override { return "cross_table_sum"; }
  std::vector<SpecRequest> plan() const override { return {}; }
  ConstraintResult evaluate(const Inputs &in) const override;  // throws: the constraint reads the Context
  bool reads_context() const override { return true; }
  ConstraintResult evaluate_context(const Context &ctx) const override;

  // (table, column) of a qualified name; throws the reference's errors (:158-175)
  static std::pair<std::string, std::string> parse_qualified_column(const std::string &qualified);
  // the join and the result row; throws TermError where a side is beyond its bounds or the key kinds differ
  CrossTableSumRow join(const SideSums &left, const SideSums &right) const;
  CrossTableSumRow totals(double left_total, double right_total) const;  // the ungrouped form
  // the verdict and the message (:572-630); left_total / right_total feed the ungrouped form's example
  ConstraintResult verdict(const CrossTableSumRow &row) const;

 private:
  std::string left_, right_;
  std::vector<std::string> group_by_;
  double tolerance_ = 0.0;
  size_t max_violations_ = 100;
  uint32_t max_groups_ = kDefaultMaxGroups;
  bool composite_ = false;
  CrossTableSumRow join_tuples(const SideSums &left, const SideSums &right) const;  // (2 .. 8 group columns)
};

// ---- constraints/foreign_key.rs: every non-NULL value of child.c is a value of parent.p.  The parent's column is walked
// once under a TGX_CHECK_DISTINCT spec, its key set handed to a TGX_CHECK_KEY_PROBE spec over the child's column, and the
// child walked once: integer keys, or string keys when both columns are string layouts (the parent's values then travel
// as keyed fingerprints and the child's plan takes the parent plan's fingerprint key).  What the verdict is made from,
// as tgx_key_probe_get / _entries (_strings_get / _entries_bytes) give it
struct ForeignKeyCounts {
  uint64_t null_rows = 0, missing_rows = 0, overflow_rows = 0, missing_keys = 0;
  uint64_t long_rows = 0;             // string keys: missing rows whose value is longer than max_value_bytes
  std::vector<int64_t> keys;          // the missing keys held, ascending
  std::vector<std::string> str_keys;  // ... of string keys, ascending bytewise
  bool strings = false;
  bool examples = true;       // the child column is of a type the reference's collector downcasts (:265-291)
};
class ForeignKeyConstraint : public Constraint {
 public:
  static constexpr uint32_t kDefaultMaxMissingKeys = 10000;
  static constexpr uint32_t kDefaultMaxValueBytes = 256;
  ForeignKeyConstraint(std::string child_column, std::string parent_column)  // "table.column" each (:78-91)
      : child_(std::move(child_column)), parent_(std::move(parent_column)) {}
  ForeignKeyConstraint &allow_nulls(bool allow) { allow_nulls_ = allow; return *this; }
  ForeignKeyConstraint &use_left_join(bool on) { use_left_join_ = on; return *this; }  // (accepted; one strategy here)
  ForeignKeyConstraint &max_violations_reported(size_t n) { max_violations_ = n; return *this; }
  // this layer's own: the missing keys the child's table on the device is sized for (1 .. 65 536).  Rows beyond it are
  // counted (overflow): the verdict and the metric stand, `unique` reads "at least n"
  ForeignKeyConstraint &max_missing_keys(uint32_t n) { max_missing_keys_ = n; return *this; }
  // this layer's own, string keys only: the bytes a missing key may have to be kept (1 .. 256).  Missing rows with a
  // longer value are counted (long rows): the verdict and the metric stand, `unique` reads "at least n"
  ForeignKeyConstraint &max_value_bytes(uint32_t n) { max_value_bytes_ = n; value_bytes_given_ = true; return *this; }

  const std::string &child_column() const { return child_; }
  const std::string &parent_column() const { return parent_; }
  bool nulls_allowed() const { return allow_nulls_; }
  bool left_join() const { return use_left_join_; }
  size_t violations_reported() const { return max_violations_; }
  uint32_t missing_keys_bound() const { return max_missing_keys_; }
  uint32_t value_bytes_bound() const { return max_value_bytes_; }
  bool value_bytes_given() const { return value_bytes_given_; }  // (the JSON form names the option only then)

  std::string name() const override { return "foreign_key"; }
  std::vector<SpecRequest> plan() const override { return {}; }
  ConstraintResult evaluate(const Inputs &in) const override;  // throws: the constraint reads the Context
  bool reads_context() const override { return true; }
  ConstraintResult evaluate_context(const Context &ctx) const override;

  // (table, column) of a qualified name; throws the reference's errors (:130-149)
  static std::pair<std::string, std::string> parse_qualified_column(const std::string &qualified);
  // the verdict and the message (:334-410)
  ConstraintResult verdict(const ForeignKeyCounts &counts) const;

 private:
  ConstraintResult evaluate_strings(const Table &child_table, int ci, const Table &parent_table, int pi) const;
  std::string child_, parent_;
  bool allow_nulls_ = false, use_left_join_ = true;
  size_t max_violations_ = 100;
  uint32_t max_missing_keys_ = kDefaultMaxMissingKeys;
  uint32_t max_value_bytes_ = kDefaultMaxValueBytes;
  bool value_bytes_given_ = false;
};

// ---- constraints/join_coverage.rs: the match rate of L LEFT / RIGHT JOIN R ON L.l = R.r, SUM(CASE WHEN the far side's key
// IS NOT NULL ..) / COUNT(*).  COUNT(*) over a join counts matched PAIRS: the far side's non-NULL keys are gathered as
// {key, 1} records (tgx_plan_set_key_probe_rows) and go into a COUNTED TGX_CHECK_KEY_PROBE spec over the near side's
// column (tgx_plan_set_key_probe_counted), so matched = pairs and total = join_rows.  One key pair only: integer keys,
// or string keys when both columns are string layouts (ForeignKeyConstraint's rule) -- the far side is then gathered as
// fingerprint records (tgx_plan_set_key_probe_rows_strings), the near side probed under a counted strings spec
// (tgx_plan_set_key_probe_strings_counted), and every plan of the evaluation carries one fingerprint key.
enum class CoverageType { LeftCoverage, RightCoverage, BidirectionalCoverage };
// what the verdict is made from.  left: L probed against R's set, right: R against L's; a side the coverage type does not
// ask for stays !known
struct JoinCoverageCounts {
  struct Side {
    bool known = false;
    uint64_t pairs = 0, join_rows = 0;
  } left, right;
  uint64_t left_distinct = 0;  // COUNT(DISTINCT L.l): read with distinct_only and LeftCoverage
  // the examples, always of the left side (:289-324): L's missing keys against R's set, its NULL rows, and the rows
  // whose key found no slot; read when the check fails and max_examples_reported > 0
  bool examples_known = false;
  uint64_t missing_keys = 0, null_rows = 0, overflow_rows = 0;
  uint64_t long_rows = 0;  // string keys: L's missing rows whose value is longer than max_value_bytes (not kept)
  // composite keys: L's distinct tuples with a NULL component (each a distinct value of the examples query) and the
  // rows of such tuples that found no slot; where they are not known the NULL rows count as ONE distinct value
  bool null_keys_known = false;
  uint64_t null_keys = 0, null_overflow_rows = 0;
};
class JoinCoverageConstraint : public Constraint {
 public:
  static constexpr uint32_t kDefaultMaxMissingKeys = 10000;
  static constexpr uint32_t kDefaultMaxValueBytes = ForeignKeyConstraint::kDefaultMaxValueBytes;
  JoinCoverageConstraint(std::string left_table, std::string right_table)  // (:94-105)
      : left_(std::move(left_table)), right_(std::move(right_table)) {}
  JoinCoverageConstraint &on(std::string l, std::string r) {
    keys_.assign(1, {std::move(l), std::move(r)});
    return *this;
  }
  JoinCoverageConstraint &on_multiple(std::vector<std::pair<std::string, std::string>> keys) {
    keys_ = std::move(keys);
    return *this;
  }
  JoinCoverageConstraint &expect_match_rate(double r) {  // rate.clamp(0.0, 1.0) (:139-142); a NaN stays one
    expected_ = r < 0.0 ? 0.0 : r > 1.0 ? 1.0 : r;
    return *this;
  }
  JoinCoverageConstraint &coverage_type(CoverageType t) { type_ = t; return *this; }
  JoinCoverageConstraint &distinct_only(bool d) { distinct_only_ = d; return *this; }
  JoinCoverageConstraint &max_examples_reported(size_t n) { max_examples_ = n; return *this; }
  // this layer's own, as ForeignKeyConstraint's: the missing keys the probe's table on the device is sized for
  JoinCoverageConstraint &max_missing_keys(uint32_t n) { max_missing_keys_ = n; return *this; }
  // this layer's own, string keys only, as ForeignKeyConstraint's: the bytes a missing key may have to be kept (1 .. 256).
  // Missing rows with a longer value are counted (long rows): the rate stands, the examples read "at least n"
  JoinCoverageConstraint &max_value_bytes(uint32_t n) { max_value_bytes_ = n; value_bytes_given_ = true; return *this; }
  // this layer's own, an opt-in: a join on 2 .. 8 key pairs (on_multiple) runs on the device, each pair two integer or
  // two string columns, under TGX_CHECK_KEY_PROBE's tuple modes (tgx_plan_set_key_probe_tuples*).  A row with a NULL in
  // any key column joins nothing, and the examples are counted over fingerprints.  Off (the default), and with one key
  // pair, everything is what it was
  JoinCoverageConstraint &composite_keys_on_device(bool on) { composite_ = on; return *this; }
  bool composite_keys() const { return composite_; }
  static constexpr size_t kMaxKeyPairs = 8;

  const std::string &left_table() const { return left_; }
  const std::string &right_table() const { return right_; }
  const std::vector<std::pair<std::string, std::string>> &join_keys() const { return keys_; }
  double expected_match_rate() const { return expected_; }
  CoverageType coverage() const { return type_; }
  bool distinct() const { return distinct_only_; }
  size_t examples_reported() const { return max_examples_; }
  uint32_t missing_keys_bound() const { return max_missing_keys_; }
  uint32_t value_bytes_bound() const { return max_value_bytes_; }
  bool value_bytes_given() const { return value_bytes_given_; }  // (the JSON form names the option only then)

  std::string name() const override { return "join_coverage"; }
  std::vector<SpecRequest> plan() const override { return {}; }
  ConstraintResult evaluate(const Inputs &in) const override;  // throws: the constraint reads the Context
  bool reads_context() const override { return true; }
  ConstraintResult evaluate_context(const Context &ctx) const override;

  // what evaluation refuses before it looks at a table: no keys, composite keys, identifiers, RightCoverage with
  // distinct_only, the bound.  Throws
  void validate() const;
  // does a failing verdict read the examples' counts?
  bool wants_examples() const { return max_examples_ > 0; }
  // the rate, the verdict and the message (:327-421); throws when the join has no rows
  ConstraintResult verdict(const JoinCoverageCounts &counts) const;

 private:
  std::string left_, right_;
  std::vector<std::pair<std::string, std::string>> keys_;
  double expected_ = 1.0;
  CoverageType type_ = CoverageType::LeftCoverage;
  bool distinct_only_ = false;
  size_t max_examples_ = 100;
  uint32_t max_missing_keys_ = kDefaultMaxMissingKeys;
  uint32_t max_value_bytes_ = kDefaultMaxValueBytes;
  bool value_bytes_given_ = false;
  bool composite_ = false;
  ConstraintResult evaluate_composite(const Context &ctx) const;  // (2 .. 8 key pairs, the opt-in given)
};

// ---- core/check.rs
class Check {
 public:
  const std::string &name() const { return name_; }
  Level level() const { return level_; }
  const std::optional<std::string> &description() const { return description_; }
  const std::vector<std::shared_ptr<Constraint>> &constraints() const { return constraints_; }
  class Builder;
  static Builder builder(std::string name);

 private:
  friend class Builder;
  std::string name_;
  Level level_ = Level::Warning;  // Level::default() (core/level.rs:80-81)
  std::optional<std::string> description_;
  std::vector<std::shared_ptr<Constraint>> constraints_;
};

struct CompletenessOptions {  // core/builder_extensions.rs:14-80 (as ConstraintOptions)
  LogicalOperator op;
  double threshold = 1.0;
  static CompletenessOptions full() { return {}; }
  static CompletenessOptions with_threshold(double t) {
    CompletenessOptions o;
    o.threshold = t;
    return o;
  }
  static CompletenessOptions at_least(size_t n) {
    CompletenessOptions o;
    o.op = {LogicalOperator::AtLeast, n};
    return o;
  }
  static CompletenessOptions any() {
    CompletenessOptions o;
    o.op = {LogicalOperator::Any, 0};
    return o;
  }
};

class Check::Builder {
 public:
  explicit Builder(std::string name) { check_.name_ = std::move(name); }
  Builder &level(Level l) { check_.level_ = l; return *this; }
  Builder &description(std::string d) { check_.description_ = std::move(d); return *this; }
  Builder &constraint(std::shared_ptr<Constraint> c) { check_.constraints_.push_back(std::move(c)); return *this; }
  // check.rs:321 / :1743 / :2233-2300
  Builder &has_size(Assertion a);
  Builder &has_approx_count_distinct(std::string column, Assertion a);  // core/check.rs:379-390 (metric: exact count)
  Builder &completeness(std::vector<std::string> columns, CompletenessOptions options);
  Builder &completeness(std::string column, CompletenessOptions options) {
    return completeness(std::vector<std::string>{std::move(column)}, options);
  }
  Builder &any_complete(std::vector<std::string> columns);
  Builder &at_least_complete(size_t n, std::vector<std::string> columns, double threshold);
  Builder &exactly_complete(size_t n, std::vector<std::string> columns, double threshold);
  // check.rs:1812-1960
  Builder &statistic(std::string column, StatisticType stat, Assertion a);
  Builder &has_min(std::string c, Assertion a) { return statistic(std::move(c), {StatisticType::Min}, a); }
  Builder &has_max(std::string c, Assertion a) { return statistic(std::move(c), {StatisticType::Max}, a); }
  Builder &has_mean(std::string c, Assertion a) { return statistic(std::move(c), {StatisticType::Mean}, a); }
  Builder &has_sum(std::string c, Assertion a) { return statistic(std::move(c), {StatisticType::Sum}, a); }
  Builder &has_standard_deviation(std::string c, Assertion a) {
    return statistic(std::move(c), {StatisticType::StandardDeviation}, a);
  }
  Builder &has_variance(std::string c, Assertion a) { return statistic(std::move(c), {StatisticType::Variance}, a); }
  // check.rs:1480-1740
  Builder &uniqueness(std::vector<std::string> columns, UniquenessType type);
  Builder &validates_uniqueness(std::vector<std::string> columns, double threshold);
  Builder &validates_distinctness(std::vector<std::string> columns, Assertion a);
  Builder &validates_unique_value_ratio(std::vector<std::string> columns, Assertion a);
  Builder &validates_primary_key(std::vector<std::string> columns);
  Builder &validates_uniqueness_with_nulls(std::vector<std::string> columns, double threshold, NullHandling h);
  Builder &primary_key(std::vector<std::string> columns);  // builder_extensions.rs:276-295
  // check.rs:829-1260, builder_extensions.rs:309-420
  // check.rs:518-623, 1777-1785 + constraints/length.rs (kind: min | max | between | exactly | not_empty)
  Builder &is_contained_in(std::string column, std::vector<std::string> allowed_values);  // constraints/values.rs:200-218
  Builder &length(std::string column, std::string kind, uint64_t a, uint64_t b);
  Builder &has_min_length(std::string column, uint64_t n) { return length(std::move(column), "min", n, 0); }
  Builder &has_max_length(std::string column, uint64_t n) { return length(std::move(column), "max", n, 0); }
  Builder &has_length_between(std::string column, uint64_t lo, uint64_t hi) { return length(std::move(column), "between", lo, hi); }
  Builder &has_exact_length(std::string column, uint64_t n) { return length(std::move(column), "exactly", n, 0); }
  Builder &is_not_empty(std::string column) { return length(std::move(column), "not_empty", 0, 0); }
  Builder &has_format(std::string column, FormatType format, double threshold, FormatOptions options);
  Builder &validates_regex(std::string column, std::string pattern, double threshold);
  Builder &validates_email(std::string column, double threshold);
  Builder &validates_url(std::string column, double threshold, bool allow_localhost);
  Builder &validates_credit_card(std::string column, double threshold, bool detect_only);
  Builder &validates_phone(std::string column, double threshold, std::optional<std::string> country);
  Builder &validates_postal_code(std::string column, double threshold, std::string country);
  Builder &validates_uuid(std::string column, double threshold);
  Builder &validates_ipv4(std::string column, double threshold);
  Builder &validates_ipv6(std::string column, double threshold);
  Builder &validates_json(std::string column, double threshold);
  Builder &validates_iso8601_datetime(std::string column, double threshold);
  Builder &email(std::string column, double threshold);
  Builder &contains_ssn(std::string column, double threshold);
  // check.rs:414 / :478
  Builder &has_approx_quantile(std::string column, double quantile, Assertion a);
  Builder &has_correlation(std::string column1, std::string column2, Assertion a);
  // the unified constraints handed to CheckBuilder::constraint(..) in the reference (core/check.rs:263):
  // MultiStatisticalConstraint::new (constraints/statistics.rs:377-417), QuantileConstraint::new / ::multiple
  // (constraints/quantile.rs:159-216), CorrelationConstraint::new / ::independence (constraints/correlation.rs:156-263)
  Builder &multi_statistic(std::string column, std::vector<std::pair<StatisticType, Assertion>> statistics);
  Builder &quantile_validation(std::string column, QuantileValidation validation);
  Builder &correlation(CorrelationValidation validation);
  // core/check.rs:2125-2179: pushes TemporalOrderingConstraint::new(table) -- empty column names, so evaluating it
  // fails identifier validation, as in the reference; configured objects come through constraint(..) (host/temporal.h)
  Builder &temporal_ordering(std::string table);
  // core/check.rs:651-657: pushes DataTypeConstraint::type_consistency(column, threshold); throws TermError where the
  // reference's constructor returns Err and the builder panics on it (a threshold outside [0, 1]: Configuration).  The other validations come
  // as configured objects through constraint(..) (host/datatype.h)
  Builder &has_consistent_data_type(std::string column, double threshold);
  // core/check.rs:685-694: pushes CustomSqlConstraint::new(expression, hint); throws TermError (ValidationFailed) where
  // the reference's builder panics on the constructor's Err (host/custom_sql.h)
  // string_functions_on_device: the constraint's opt-in of that name
  Builder &satisfies(std::string sql_expression, std::optional<std::string> hint = std::nullopt,
                     bool string_functions_on_device = false);
  // core/check.rs has_histogram / has_histogram_with_description: pushes HistogramConstraint::new[_with_description]
  // (host/value_counts.h; max_distinct bounds the values the device counts, default 10000)
  Builder &has_histogram(std::string column, std::function<bool(const Histogram &)> assertion);
  Builder &has_histogram_with_description(std::string column, std::function<bool(const Histogram &)> assertion,
                                          std::string description);
  // core/check.rs:2054-2065: pushes CrossTableSumConstraint::new(left, right); a configured object comes through
  // constraint(..)
  Builder &cross_table_sum(std::string left_column, std::string right_column);
  // pushes ForeignKeyConstraint::new(child, parent); a configured object comes through constraint(..)
  Builder &foreign_key(std::string child_column, std::string parent_column);
  // Check::join_coverage (core/check.rs:2112): JoinCoverageConstraint::new(left, right) -- without join keys, which is
  // an evaluation error; a configured constraint goes through constraint()
  Builder &join_coverage(std::string left_table, std::string right_table);
  Check build() { return check_; }

 private:
  Check check_;
};

// ---- the SessionContext stand-in: named tables = named columns x batches
struct Batch {
  std::vector<tgx_column> columns;  // parallel to Table::column_names
};
struct Table {
  std::vector<std::string> column_names;
  std::vector<Batch> batches;
  // Arrow DataType names parallel to column_names (optional: a column without one is what its tgx_type says --
  // TGX_INT64 "Int64", TGX_INT32 "Int32", TGX_FLOAT32 "Float32", ...; a Timestamp / Date32 column handed over as
  // TGX_INT64 / TGX_INT32 needs its name here for the reference's result-type rule to apply)
  std::vector<std::string> arrow_types;
};
// what the constraints that join two tables' key columns ask of a column (foreign_key, join_coverage): both take the
// strings route when both columns are string layouts in every batch that has them, and a side without a batch goes the
// way of the other side
inline bool string_layout(int type) {
  return type == TGX_UTF8 || type == TGX_LARGE_UTF8 || type == TGX_UTF8_VIEW || type == TGX_DICT32_UTF8;
}
// 1: the column is a string layout in every batch that has it; 0: no batch has it (an empty table); -1: another type
inline int string_side(const Table &table, int index) {
  int side = 0;
  for (const Batch &b : table.batches)
    if ((size_t)index < b.columns.size()) {
      if (!string_layout(b.columns[index].type)) return -1;
      side = 1;
    }
  return side;
}
class Context {
 public:
  void register_table(const std::string &name, Table t) { tables_[name] = std::move(t); }
  const Table *table(const std::string &name) const {
    auto it = tables_.find(name);
    return it == tables_.end() ? nullptr : &it->second;
  }

 private:
  std::map<std::string, Table> tables_;
};

// ---- core/result.rs
struct ValidationMetrics {
  size_t total_checks = 0, passed_checks = 0, failed_checks = 0, skipped_checks = 0;
  uint64_t execution_time_ms = 0;
  std::map<std::string, double> custom_metrics;
  double success_rate() const { return total_checks == 0 ? 100.0 : 100.0 * passed_checks / total_checks; }
};
struct ValidationIssue {
  std::string check_name, constraint_name;
  Level level;
  std::string message;
  std::optional<double> metric;
};
struct ValidationReport {
  std::string suite_name, timestamp;
  ValidationMetrics metrics;
  std::vector<ValidationIssue> issues;
  bool has_errors() const;
  bool has_warnings() const;
};
struct ValidationResult {
  bool success = true;  // ValidationResult::Success{metrics, report} / Failure{report}
  ValidationReport report;
  bool is_success() const { return success; }
  bool is_failure() const { return !success; }
  std::string to_json() const;  // serde_json::to_string_pretty of the tagged enum (formatters.rs:222-245)
};

// ---- core/suite.rs:351-600
class ValidationSuite {
 public:
  class Builder;
  static Builder builder(std::string name);
  const std::string &name() const { return name_; }
  const std::string &table_name() const { return table_name_; }
  const std::vector<Check> &checks() const { return checks_; }
  // throws TermError only for library-level failures (no device, ...); constraint errors become issues
  ValidationResult run(const Context &ctx) const;

 private:
  friend class Builder;
  std::string name_;
  std::optional<std::string> description_;
  std::string table_name_ = "data";  // suite.rs:549
  std::vector<Check> checks_;
  bool strict_types_ = true;
  bool exact_keys_ = true;
  std::map<std::string, std::string> declared_types_;
};
class ValidationSuite::Builder {
 public:
  explicit Builder(std::string name) { suite_.name_ = std::move(name); }
  Builder &description(std::string d) { suite_.description_ = std::move(d); return *this; }
  Builder &table_name(std::string t) { suite_.table_name_ = std::move(t); return *this; }
  Builder &check(Check c) { suite_.checks_.push_back(std::move(c)); return *this; }
  Builder &with_optimizer(bool) { return *this; }  // suite.rs:457-469: the reference ignores it too
  // true (default): MIN / MAX / SUM / quantiles on columns whose aggregate the reference cannot read are errors, as
  // there (reference_extracts); false: the widened value answers (a deviation)
  Builder &strict_reference_types(bool on) { suite_.strict_types_ = on; return *this; }
  // true (default): uniqueness checks over string / binary / tuple keys count by VALUE -- equal fingerprints are
  // confirmed byte by byte (TGX_FLAG_EXACT_KEYS), `COUNT(DISTINCT c)` as the reference's DataFusion computes it
  // (constraints/uniqueness.rs:612-617); false: by keyed 128-bit fingerprint alone (faster on big batches; two distinct
  // values count once only if all 128 bits agree under a key the data's producer does not know: INTEGRATION.md)
  Builder &exact_string_keys(bool on) { suite_.exact_keys_ = on; return *this; }
  // the Arrow DataType (its Debug form: "Int32", "Date32", "Timestamp(Nanosecond, None)", "UInt8", ...) of a column of
  // the table the suite will run on; takes precedence over Table::arrow_types
  Builder &column_type(std::string column, std::string arrow_type) {
    suite_.declared_types_[std::move(column)] = std::move(arrow_type);
    return *this;
  }
  ValidationSuite build() { return suite_; }

 private:
  ValidationSuite suite_;
};

// JSON description of a suite (the bridge the Python binding uses) -> suite
ValidationSuite suite_from_json(const std::string &json);  // throws TermError on malformed input

}  // namespace term_guard
