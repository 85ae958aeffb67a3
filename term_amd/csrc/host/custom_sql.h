// custom_sql.h -- CustomSqlConstraint (TG/constraints/custom_sql.rs), the predicate compiler behind it and behind
// ComplianceAnalyzer (TG/analyzers/advanced/compliance.rs), and the device request both make: one TGX_CHECK_ROW_PREDICATE
// spec.  Host-only C++: nothing here needs HIP.
//
// The compiler takes a CLOSED subset, not SQL:
//     pred    := term (OR term)*
//     term    := factor (AND factor)*
//     factor  := NOT factor | '(' pred ')' | atom
//     atom    := operand cmp operand | col IS [NOT] NULL | col [NOT] BETWEEN lit AND lit
//              | col [NOT] IN '(' lit (',' lit)* ')'
//     operand := col | lit            cmp := = | <> | != | < | <= | > | >=
// An atom needs at least one column.  Identifiers are unquoted (lowercased before lookup, as DataFusion normalises
// them) or "quoted"; a `table.` qualifier is not accepted.  A literal is an integer token (it must fit int64), a float
// token (a point or an exponent; read by strtod) or a 'string' with '' for a quote; a leading `-` belongs to a numeric
// literal.  Keywords are case-insensitive.  `lit op col` is turned round; `<>`, BETWEEN and IN are lowered by SQL's own
// definitions (NOT(x = l); x >= a AND x <= b; an OR of equalities) onto the leaves and the postfix program of
// include/tgx.h.  Everything else -- arithmetic, function calls, LIKE, CASE, casts, TRUE / FALSE, string order
// comparisons, literal-against-literal comparisons, IN lists that mix strings and numbers, more than 8 columns, 32
// leaves, 64 ops or 256 literal bytes -- is refused with a message that names the first thing outside the subset.
//
// The dialect `string_functions` (an opt-in; without it the above is all there is, byte for byte) adds the atoms
//     col [NOT] LIKE 'pattern'                                 STR_LIKE, under NOT where written
//     lenfn '(' col ')' cmp int | lenfn '(' col ')' [NOT] BETWEEN int AND int
//                                                              STR_LENGTH; lenfn := LENGTH | CHAR_LENGTH |
//                                                              CHARACTER_LENGTH (characters) | OCTET_LENGTH (bytes)
//     TRIM '(' col ')' (= | <> | !=) ''                        STR_BLANK, under NOT for the two inequalities
//     col (< | <= | > | >=) 'lit' | col [NOT] BETWEEN 'a' AND 'b'     STR_CMP
// lowered as above (`lit op call` is turned round too).  It is a superset: what the base dialect accepts compiles to the
// identical leaves, program and pool.  Refused by name: ILIKE, SIMILAR TO, an ESCAPE clause, a pattern with a backslash;
// a length against a float literal, a string, a column or another call, a nested call, IN on a length; TRIM against
// any literal but '', LTRIM / RTRIM / BTRIM, TRIM(.. FROM ..); every other function.
#pragma once
#include <optional>
#include <string>
#include <vector>

#include "term_guard.h"

namespace term_guard {

// what compile_row_predicate throws: `what` names the first thing outside the subset
struct PredicateRefusal {
  std::string what;
};

struct RowPredicate {
  std::vector<std::string> columns;  // in order of first appearance: the spec's column list
  tgx_row_predicate_params params;   // what a leaf does not read is zero
  // per column: a CMP_LITERAL leaf reads it (what a declared temporal / decimal / boolean / binary type refuses)
  std::vector<char> literal_compared;
};
struct PredicateDialect {
  bool string_functions = false;
};
// throws PredicateRefusal
RowPredicate compile_row_predicate(const std::string &expression, const PredicateDialect &dialect = PredicateDialect());
std::string row_predicate_json(const RowPredicate &p);
// the request of a compiled predicate: kind TGX_CHECK_ROW_PREDICATE, `columns`, `row_predicate`
SpecRequest row_predicate_request(const RowPredicate &p);

// validate_sql_expression (custom_sql.rs:100-190): the reference's message, or nullopt for an expression it accepts.  Of
// several forbidden words the FIRST in the list's written order is named (the reference walks a HashSet)
std::optional<std::string> custom_sql_refusal(const std::string &sql);
// ComplianceAnalyzer::validate_predicate (compliance.rs:88-108): the forbidden keyword found, or nullopt
std::optional<std::string> compliance_forbidden_keyword(const std::string &predicate);

class CustomSqlConstraint : public Constraint {
 public:
  // throws TermError (ValidationFailed) where the reference's constructor returns Err
  CustomSqlConstraint(std::string expression, std::optional<std::string> hint);
  static CustomSqlConstraint try_new(std::string expression, std::optional<std::string> hint) {
    return CustomSqlConstraint(std::move(expression), std::move(hint));
  }
  const std::string &expression() const { return expression_; }
  const std::optional<std::string> &hint() const { return hint_; }
  // an opt-in: the expression is compiled under the dialect `string_functions` (LIKE, LENGTH, TRIM(c) = '', string
  // order).  Without it such an expression is what it was: "not on the GPU path"
  CustomSqlConstraint &string_functions_on_device(bool on) { string_functions_ = on; return *this; }
  bool string_functions() const { return string_functions_; }

  std::string name() const override { return "custom_sql"; }
  // throws TermError ("... not on the GPU path: <what>") for an expression outside the subset
  std::vector<SpecRequest> plan() const override;
  ConstraintResult evaluate(const Inputs &in) const override;
  std::optional<ConstraintResult> failure_from_error(const std::string &error) const override;
  // custom_sql.rs:288-302
  std::string description() const { return "Checks that all rows satisfy the SQL expression: " + expression_; }
  std::vector<std::pair<std::string, std::string>> metadata() const;

 private:
  std::string expression_;
  std::optional<std::string> hint_;
  bool string_functions_ = false;
  PredicateDialect dialect() const {
    PredicateDialect d;
    d.string_functions = string_functions_;
    return d;
  }
};

}  // namespace term_guard
