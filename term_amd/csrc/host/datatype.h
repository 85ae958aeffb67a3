// datatype.h -- DataTypeConstraint (TG/constraints/datatype.rs) over TGX_CHECK_VALUE_RULE: the numeric NonNegative,
// Positive, Integer and Range validations are one scan on the device; SpecificType and Consistency need no scan beyond
// the one that says the column exists; Finite and every String, Temporal and Custom validation are the constraint's own
// error (the caller hands such a constraint to the stock path).  The four String validations run on the device after
// string_functions_on_device(true), an opt-in: one TGX_CHECK_ROW_PREDICATE request on [column], built from the SQL of
// datatype.rs:161-175 by host/custom_sql.h's compiler under its dialect string_functions.  Included by term_guard.h's
// users through term_guard.cpp and host_abi.cpp.
#pragma once
#include "json.h"
#include "term_guard.h"

namespace term_guard {

// ---- datatype.rs:42-91
struct NumericValidation {
  enum Kind { NonNegative, Positive, Integer, Range, Finite } kind = NonNegative;
  double min = 0, max = 0;  // Range
  static NumericValidation range(double min, double max) { return {Range, min, max}; }
};
struct StringTypeValidation {
  enum Kind { NotEmpty, ValidUtf8, NotBlank, MaxBytes } kind = NotEmpty;
  uint64_t max_bytes = 0;  // MaxBytes
};
struct TemporalValidation {
  enum Kind { PastDate, FutureDate, DateRange, ValidTimezone } kind = PastDate;
  std::string start, end;  // DateRange
};
// ---- datatype.rs:21-40, 93-128
struct DataTypeValidation {
  enum Kind { SpecificType, Consistency, Numeric, String, Temporal, Custom } kind = SpecificType;
  std::string type_name;  // SpecificType: the Arrow DataType's Debug form ("Int64", "Timestamp(Nanosecond, None)")
  double threshold = 0;   // Consistency
  NumericValidation numeric;
  StringTypeValidation string;
  TemporalValidation temporal;
  std::string sql_predicate;  // Custom
  static DataTypeValidation specific_type(std::string t) {
    DataTypeValidation v;
    v.kind = SpecificType;
    v.type_name = std::move(t);
    return v;
  }
  static DataTypeValidation consistency(double threshold) {
    DataTypeValidation v;
    v.kind = Consistency;
    v.threshold = threshold;
    return v;
  }
  static DataTypeValidation of(NumericValidation n) {
    DataTypeValidation v;
    v.kind = Numeric;
    v.numeric = n;
    return v;
  }
  static DataTypeValidation of(StringTypeValidation s) {
    DataTypeValidation v;
    v.kind = String;
    v.string = s;
    return v;
  }
  static DataTypeValidation of(TemporalValidation t) {
    DataTypeValidation v;
    v.kind = Temporal;
    v.temporal = std::move(t);
    return v;
  }
  static DataTypeValidation custom(std::string sql_predicate) {
    DataTypeValidation v;
    v.kind = Custom;
    v.sql_predicate = std::move(sql_predicate);
    return v;
  }
  std::string description() const;  // :95-128
};

// ---- datatype.rs:233-454
class DataTypeConstraint : public Constraint {
 public:
  // throws TermError as DataTypeConstraint::new returns Err: a column name that is no identifier; a consistency
  // threshold outside [0, 1] (Configuration)
  DataTypeConstraint(std::string column, DataTypeValidation validation);
  static DataTypeConstraint non_negative(std::string column);
  static DataTypeConstraint type_consistency(std::string column, double threshold);
  static DataTypeConstraint specific_type(std::string column, std::string data_type);

  std::string name() const override { return "datatype"; }
  std::optional<std::string> column() const override { return column_; }
  std::vector<SpecRequest> plan() const override;
  ConstraintResult evaluate(const Inputs &in) const override;
  const DataTypeValidation &validation() const { return validation_; }
  // an opt-in: a String validation plans a ROW_PREDICATE request instead of being the constraint's error.  Every other
  // validation answers as without it
  DataTypeConstraint &string_functions_on_device(bool on) { string_functions_ = on; return *this; }
  bool string_functions() const { return string_functions_; }
  // the predicate of a String validation, as datatype.rs:161-175 writes it (the column quoted)
  std::string string_predicate() const;
  std::string description() const;  // metadata(): "Validates {description} for column '{column}'"

 private:
  std::string column_;
  DataTypeValidation validation_;
  bool string_functions_ = false;
};

// a numeric validation -> the device's rule.  Range {min, max}: the reference prints the bounds with Rust's `{}` and
// DataFusion parses the text -- a finite integral bound with |b| <= 2^53 is an Int64 literal (-0.0 prints "-0" and is
// 0), any other finite bound a Float64 literal that round-trips; one Float64 literal makes the comparison a double one
// (TGX_RULE_BOUNDS_AS_DOUBLE).  Throws TermError (constraint evaluation, 'datatype') for what stays off the device:
// Finite, a bound that is not finite ("inf" and "NaN" are no SQL literals), an integral bound beyond 2^53.
tgx_value_rule_params value_rule_params(const NumericValidation &v);
std::shared_ptr<Constraint> datatype_from_json(const json::Value &c);

}  // namespace term_guard
