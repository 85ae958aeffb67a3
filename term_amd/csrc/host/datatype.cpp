// datatype.cpp -- DataTypeConstraint (TG/constraints/datatype.rs), placeholders included.
#include "datatype.h"

#include "custom_sql.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

namespace term_guard {

namespace {

[[noreturn]] void evaluation_error(const std::string &msg) {
  throw TermError{TermError::ConstraintEvaluation, "'datatype': " + msg};
}

// Rust's {:.1} of a percentage
std::string pct1(double v) {
  if (isnan(v)) return "NaN";
  if (isinf(v)) return v > 0 ? "inf" : "-inf";
  char buf[64];
  snprintf(buf, sizeof(buf), "%.1f", v);
  return buf;
}

// how DataFusion reads the bound the reference has printed with `{}`
enum class Literal { Int64, Float64 };
Literal classify_bound(double b, const char *which) {
  if (!isfinite(b))
    evaluation_error(std::string("a range bound that is not finite is not a SQL literal, the reference's query fails to "
                                 "parse (not on the GPU path): the ") + which + " is " + rust_f64(b));
  if (b != floor(b)) return Literal::Float64;
  if (fabs(b) > 9007199254740992.0)
    evaluation_error(std::string("an integral range bound beyond 2^53 is an integer literal whose SQL type is not pinned "
                                 "(not on the GPU path): the ") + which + " is " + rust_f64(b));
  return Literal::Int64;
}

const char *const kNumericNames[] = {"non_negative", "positive", "integer", "range", "finite"};
const char *const kStringNames[] = {"not_empty", "valid_utf8", "not_blank", "max_bytes"};
const char *const kTemporalNames[] = {"past_date", "future_date", "date_range", "valid_timezone"};

template <size_t N>
int index_of(const char *const (&names)[N], const std::string &s, const char *what) {
  for (size_t i = 0; i < N; i++)
    if (s == names[i]) return (int)i;
  throw TermError{TermError::Internal, std::string("unknown ") + what + " validation '" + s + "'"};
}

// a bound of the JSON form: a number, or "inf" / "-inf" / "NaN" (JSON has no such numbers)
double bound_from(const json::Value &c, const char *key) {
  const json::Value *v = c.get(key);
  if (!v) throw TermError{TermError::Internal, std::string("constraint JSON is missing '") + key + "'"};
  if (v->is(json::Value::Number)) return v->num;
  if (v->is(json::Value::String)) {
    if (v->str == "inf") return INFINITY;
    if (v->str == "-inf") return -INFINITY;
    if (v->str == "NaN") return NAN;
  }
  throw TermError{TermError::Internal, std::string("'") + key + "' must be a number, \"inf\", \"-inf\" or \"NaN\""};
}

}  // namespace

// ---- datatype.rs:95-128
std::string DataTypeValidation::description() const {
  switch (kind) {
    case SpecificType: return "type is " + type_name;
    case Consistency: return "type consistency >= " + pct1(threshold * 100.0) + "%";
    case Numeric:
      switch (numeric.kind) {
        case NumericValidation::NonNegative: return "non-negative values";
        case NumericValidation::Positive: return "positive values";
        case NumericValidation::Integer: return "integer values";
        case NumericValidation::Range:
          return "values between " + rust_f64(numeric.min) + " and " + rust_f64(numeric.max);
        case NumericValidation::Finite: return "finite values";
      }
      break;
    case String:
      switch (string.kind) {
        case StringTypeValidation::NotEmpty: return "non-empty strings";
        case StringTypeValidation::ValidUtf8: return "valid UTF-8 strings";
        case StringTypeValidation::NotBlank: return "non-blank strings";
        case StringTypeValidation::MaxBytes: return "strings with max " + std::to_string(string.max_bytes) + " bytes";
      }
      break;
    case Temporal:
      switch (temporal.kind) {
        case TemporalValidation::PastDate: return "past dates";
        case TemporalValidation::FutureDate: return "future dates";
        case TemporalValidation::DateRange: return "dates between " + temporal.start + " and " + temporal.end;
        case TemporalValidation::ValidTimezone: return "valid timezone";
      }
      break;
    case Custom: return "custom validation: " + sql_predicate;
  }
  return std::string();
}

// ---- datatype.rs:252-287
DataTypeConstraint::DataTypeConstraint(std::string column, DataTypeValidation validation)
    : column_(std::move(column)), validation_(std::move(validation)) {
  if (auto e = validate_identifier(column_)) throw *e;
  if (validation_.kind == DataTypeValidation::Consistency && !(validation_.threshold >= 0.0 && validation_.threshold <= 1.0))
    throw TermError{TermError::Configuration, "Threshold must be between 0.0 and 1.0"};
}
DataTypeConstraint DataTypeConstraint::non_negative(std::string column) {
  return DataTypeConstraint(std::move(column), DataTypeValidation::of(NumericValidation{NumericValidation::NonNegative}));
}
DataTypeConstraint DataTypeConstraint::type_consistency(std::string column, double threshold) {
  return DataTypeConstraint(std::move(column), DataTypeValidation::consistency(threshold));
}
DataTypeConstraint DataTypeConstraint::specific_type(std::string column, std::string data_type) {
  return DataTypeConstraint(std::move(column), DataTypeValidation::specific_type(std::move(data_type)));
}

std::string DataTypeConstraint::description() const {
  return "Validates " + validation_.description() + " for column '" + column_ + "'";
}

// ---- datatype.rs:161-175
std::string DataTypeConstraint::string_predicate() const {
  std::string col = "\"";
  for (char ch : column_) col += ch == '"' ? std::string("\"\"") : std::string(1, ch);
  col += "\"";
  switch (validation_.string.kind) {
    case StringTypeValidation::NotEmpty: return "LENGTH(" + col + ") > 0";
    case StringTypeValidation::ValidUtf8: return col + " IS NOT NULL";
    case StringTypeValidation::NotBlank: return "TRIM(" + col + ") != ''";
    case StringTypeValidation::MaxBytes: return "OCTET_LENGTH(" + col + ") <= " + std::to_string(validation_.string.max_bytes);
  }
  return std::string();
}

namespace {

// the verdict of the validations that count (:406-438): `valid` of `considered` rows
ConstraintResult rate_verdict(double valid, double considered, const std::string &description) {
  const double rate = valid / considered;  // (0 / 0: NaN, a Failure)
  const std::string msg = pct1(rate * 100.0) + "% of values satisfy " + description;
  if (rate >= 1.0) return {ConstraintStatus::Success, rate, msg};
  return ConstraintResult::failure_with_metric(rate, msg);
}

}  // namespace

tgx_value_rule_params value_rule_params(const NumericValidation &v) {
  tgx_value_rule_params p;
  memset(&p, 0, sizeof(p));
  switch (v.kind) {
    case NumericValidation::NonNegative: p.mode = TGX_RULE_GE_ZERO; break;
    case NumericValidation::Positive: p.mode = TGX_RULE_GT_ZERO; break;
    case NumericValidation::Integer: p.mode = TGX_RULE_INTEGER; break;
    case NumericValidation::Range: {
      const Literal lo = classify_bound(v.min, "minimum"), hi = classify_bound(v.max, "maximum");
      p.mode = TGX_RULE_BETWEEN;
      // (-0.0 prints "-0", the Int64 literal 0: + 0.0 makes it +0.0 where it is read as a double)
      p.lo_f = lo == Literal::Int64 ? v.min + 0.0 : v.min;
      p.hi_f = hi == Literal::Int64 ? v.max + 0.0 : v.max;
      if (lo == Literal::Float64 || hi == Literal::Float64) {
        p.flags = TGX_RULE_BOUNDS_AS_DOUBLE;
      } else {
        p.lo_i = (int64_t)v.min;
        p.hi_i = (int64_t)v.max;
      }
      break;
    }
    case NumericValidation::Finite:
      evaluation_error("finite values validation is ISFINITE(col), which DataFusion 50 is not known to have "
                       "(not on the GPU path)");
  }
  return p;
}

// evaluate() up to its query (:296-396): what the device is asked
std::vector<SpecRequest> DataTypeConstraint::plan() const {
  SpecRequest r;
  r.column = column_;
  switch (validation_.kind) {
    case DataTypeValidation::SpecificType:  // the schema alone (:302-334); the request says that the column exists
    case DataTypeValidation::Consistency:   // SELECT COUNT(*) .. WHERE col IS NOT NULL, its answer unread (:341-359)
      r.kind = TGX_CHECK_COUNT;
      break;
    case DataTypeValidation::Numeric:
      r.kind = TGX_CHECK_VALUE_RULE;
      r.value_rule = value_rule_params(validation_.numeric);
      break;
    case DataTypeValidation::String:
      if (!string_functions_)
        evaluation_error(validation_.description() + " validation reads a string column (not on the GPU path)");
      if (validation_.string.max_bytes > (uint64_t)INT64_MAX)
        evaluation_error("a byte limit beyond int64 is no SQL integer literal (not on the GPU path)");
      try {
        PredicateDialect dialect;
        dialect.string_functions = true;
        return {row_predicate_request(compile_row_predicate(string_predicate(), dialect))};
      } catch (const PredicateRefusal &refusal) {
        evaluation_error(validation_.description() + " validation is not on the GPU path: " + refusal.what);
      }
    case DataTypeValidation::Temporal:
      evaluation_error(validation_.description() + " validation compares with CURRENT_DATE or date texts "
                       "(not on the GPU path)");
    case DataTypeValidation::Custom:
      evaluation_error("custom validation is an arbitrary SQL predicate (not on the GPU path)");
  }
  return {r};
}

ConstraintResult DataTypeConstraint::evaluate(const Inputs &in) const {
  switch (validation_.kind) {
    case DataTypeValidation::SpecificType: {  // :302-334
      const std::string actual = in.arrow_types.empty() ? std::string() : in.arrow_types[0];
      if (actual.empty())
        evaluation_error("the Arrow type of column '" + column_ + "' is not known: declare it with column_type(..)");
      if (actual == validation_.type_name)
        return {ConstraintStatus::Success, 1.0, "Column '" + column_ + "' has expected type " + validation_.type_name};
      return ConstraintResult::failure_with_metric(
          0.0, "Column '" + column_ + "' has type " + actual + ", expected " + validation_.type_name);
    }
    case DataTypeValidation::Consistency: {  // :357-381: the reference's placeholder
      const double consistency = 0.95, t = validation_.threshold;
      if (consistency >= t)
        return {ConstraintStatus::Success, consistency,
                "Type consistency " + pct1(consistency * 100.0) + "% meets threshold " + pct1(t * 100.0) + "%"};
      return ConstraintResult::failure_with_metric(
          consistency, "Type consistency " + pct1(consistency * 100.0) + "% below threshold " + pct1(t * 100.0) + "%");
    }
    case DataTypeValidation::Numeric: {  // :406-438.  total = rows seen, non_null = COUNT(*), matches = valid,
      const tgx_result &r = *in.results.at(0);  // distinct = rows CAST(col AS INT) fails on
      if (r.distinct > 0)
        evaluation_error(std::to_string(r.distinct) + " rows do not fit Int32: the reference's query fails on "
                         "CAST(" + column_ + " AS INT), which is not TRY_CAST");
      return rate_verdict((double)r.matches, (double)r.non_null, validation_.description());
    }
    case DataTypeValidation::String: {  // :383-439: COUNT(*) and the valid rows, WHERE col IS NOT NULL
      if (!string_functions_) return plan(), ConstraintResult::success();  // (plan() throws the validation's error)
      if (!in.list_arrow_types.empty() && !in.list_arrow_types[0].empty() && !in.list_arrow_types[0][0].empty()) {
        const std::string &t = in.list_arrow_types[0][0];
        const bool dict_of_strings = t.compare(0, 10, "Dictionary") == 0 && t.find("Utf8") != std::string::npos;
        if (t != "Utf8" && t != "LargeUtf8" && t != "Utf8View" && !dict_of_strings)
          evaluation_error(validation_.description() + " validation reads a string column: column '" + column_ +
                           "' is declared " + t);
      }
      // total = rows seen, matches = satisfied, non_null = rows on which the predicate is not UNKNOWN -- the non-NULL
      // rows, but for `col IS NOT NULL`, which is never UNKNOWN and TRUE on exactly the non-NULL rows
      const tgx_result &r = *in.results.at(0);
      const int64_t considered = validation_.string.kind == StringTypeValidation::ValidUtf8 ? r.matches : r.non_null;
      return rate_verdict((double)r.matches, (double)considered, validation_.description());
    }
    default:
      return plan(), ConstraintResult::success();  // (plan() throws the validation's error)
  }
}

// {"type": "datatype", "column": c, "validation": "specific_type" ("data_type") | "consistency" ("threshold") |
//  "numeric" ("numeric": non_negative | positive | integer | range ("min", "max": numbers, or "inf" / "-inf" / "NaN") |
//  finite) | "string" ("string": not_empty | valid_utf8 | not_blank | max_bytes ("max_bytes")) | "temporal"
//  ("temporal": past_date | future_date | date_range ("start", "end") | valid_timezone) | "custom" ("sql_predicate"),
//  "string_functions_on_device"? (an opt-in: the String validations on the device)}
std::shared_ptr<Constraint> datatype_from_json(const json::Value &c) {
  const std::string v = c.get_str("validation");
  DataTypeValidation d;
  if (v == "specific_type") {
    d = DataTypeValidation::specific_type(c.get_str("data_type"));
  } else if (v == "consistency") {
    d = DataTypeValidation::consistency(c.get_num("threshold", 0.0));
  } else if (v == "numeric") {
    NumericValidation n;
    n.kind = (NumericValidation::Kind)index_of(kNumericNames, c.get_str("numeric"), "numeric");
    if (n.kind == NumericValidation::Range) {
      n.min = bound_from(c, "min");
      n.max = bound_from(c, "max");
    }
    d = DataTypeValidation::of(n);
  } else if (v == "string") {
    StringTypeValidation s;
    s.kind = (StringTypeValidation::Kind)index_of(kStringNames, c.get_str("string"), "string");
    s.max_bytes = c.get_u64("max_bytes");
    d = DataTypeValidation::of(s);
  } else if (v == "temporal") {
    TemporalValidation t;
    t.kind = (TemporalValidation::Kind)index_of(kTemporalNames, c.get_str("temporal"), "temporal");
    t.start = c.get_str("start");
    t.end = c.get_str("end");
    d = DataTypeValidation::of(t);
  } else if (v == "custom") {
    d = DataTypeValidation::custom(c.get_str("sql_predicate"));
  } else {
    throw TermError{TermError::Internal, "unknown datatype validation '" + v + "'"};
  }
  auto out = std::make_shared<DataTypeConstraint>(c.get_str("column"), std::move(d));
  if (c.get("string_functions_on_device")) out->string_functions_on_device(c.get_bool("string_functions_on_device"));
  return out;
}

Check::Builder &Check::Builder::has_consistent_data_type(std::string column, double threshold) {
  return constraint(std::make_shared<DataTypeConstraint>(DataTypeConstraint::type_consistency(std::move(column), threshold)));
}

}  // namespace term_guard
