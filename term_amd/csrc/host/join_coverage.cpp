// join_coverage.cpp -- JoinCoverageConstraint (TG/constraints/join_coverage.rs).  The reference runs one or two outer
// joins whose rows nobody reads (:181-286):
//   SELECT COUNT(*) [or COUNT(DISTINCT L.l)] AS total, SUM(CASE WHEN R.r IS NOT NULL THEN 1 ELSE 0 END) AS matched
//   FROM L LEFT JOIN R ON L.l = R.r
// and match_rate = matched / total; RightCoverage is the same with the sides swapped, BidirectionalCoverage the LEAST of
// the two rates.  COUNT(*) over a join counts matched PAIRS: with m_R(k) the rows of R that hold key k,
//   matched = sum over rows of L of m_R(l) = pairs,   total = pairs + missing rows + NULL rows = join_rows
// Here the far side is walked once under a TGX_CHECK_KEY_PROBE spec that gathers its non-NULL keys as {key, 1} records
// (tgx_plan_set_key_probe_rows: a DISTINCT export knows a key as seen once or more than once, not how often), the
// records go into a COUNTED TGX_CHECK_KEY_PROBE spec over the near side's column, where records of one key add up, and
// the near side is walked once.  Only the walks the answer needs are run: Left walks R, then L; Right walks L, then R,
// and for the examples of a failing check R again and a plain probe of L; Bidirectional walks R, then L (the probe, and
// the gathering for the other direction, in one plan: the column crosses HBM once), then R.  distinct_only adds a
// DISTINCT spec on L.l to L's plan.
// String keys -- both columns string layouts in every batch that has them, ForeignKeyConstraint's rule -- take the same
// walks with the string calls: the far side is gathered as {hash_a, hash_b, n, 0} fingerprint records
// (tgx_plan_set_key_probe_rows_strings), the near side runs under a counted strings spec
// (tgx_plan_set_key_probe_strings_counted), RightCoverage's examples under a plain strings spec, and the DISTINCT spec
// counts by value (TGX_FLAG_EXACT_KEYS, the host layer's default for a string uniqueness count).  Every plan of one
// evaluation carries ONE fingerprint key, the first plan's: records made under another key would match nothing.  On the
// Bidirectional walk L's plan holds a counted strings spec and a rows strings spec on one column, which run as two
// launches: the known second pass.
// Composite keys are an opt-in (composite_keys_on_device): a join on 2 .. 8 key pairs takes the same three walk patterns
// with the tuple calls -- the far side gathered as tuple fingerprint records (tgx_plan_set_key_probe_rows_tuples), the
// near side under a counted tuples spec (tgx_plan_set_key_probe_tuples_counted), the examples under a plain one -- each
// pair two integer or two string columns, every plan under one fingerprint key.  A row with a NULL in any key column
// joins nothing; the examples are the missing tuples plus the distinct NULL-bearing tuples, as the reference's
// SELECT DISTINCT l0, l1 .. counts them.  distinct_only counts COUNT(DISTINCT L.k0), the first left key alone.
// Without the opt-in, one key pair only: composite keys, every other column type, a pair of an integer and a string column and columns
// declared Binary are the constraint's own error, so the caller can hand the constraint to the stock path.
#include <stdio.h>
#include <string.h>

#include "term_guard.h"
#include "tgx_handles.h"

namespace term_guard {

namespace {

[[noreturn]] void evaluation_error(const std::string &msg) {
  throw TermError{TermError::ConstraintEvaluation, "'join_coverage': " + msg};
}
[[noreturn]] void query_failed(const std::string &why) {  // (:340-345)
  evaluation_error("Join coverage query failed: " + why);
}

// one side of the join: its table and key column, with the reference's planning / schema errors
struct Side {
  const Table *table = nullptr;
  int column = -1;
  std::string qualified;  // "table.column"
};
Side side_of(const Context &ctx, const std::string &table_name, const std::string &column) {
  Side s;
  s.qualified = table_name + "." + column;
  s.table = ctx.table(table_name);
  if (!s.table) query_failed("Error during planning: table 'datafusion.public." + table_name + "' not found");
  for (size_t i = 0; i < s.table->column_names.size(); i++)
    if (s.table->column_names[i] == column) s.column = (int)i;
  if (s.column < 0) query_failed("Schema error: No field named " + table_name + "." + column + ".");
  // (a column declared Binary arrives in a string layout; it is no string key)
  if ((size_t)s.column < s.table->arrow_types.size() && s.table->arrow_types[s.column] == "Binary")
    evaluation_error("column '" + s.qualified + "' is a Binary column: join keys of that type are not on the GPU path "
                     "(TGX_CHECK_KEY_PROBE takes integer and string keys)");
  return s;
}
// a side of the integer route: every batch's column is of a type the integer probe takes
void integer_side(const Side &s) {
  for (const Batch &b : s.table->batches)
    if ((size_t)s.column < b.columns.size())
      if (const char *name = off_path_type(b.columns[s.column].type))
        evaluation_error("column '" + s.qualified + "' is a " + name +
                         " column: join keys of that type are not on the GPU path (TGX_CHECK_KEY_PROBE takes integer keys)");
}

std::string percent(double rate) {  // {:.2} of rate * 100.0
  char buf[64];
  snprintf(buf, sizeof(buf), "%.2f", rate * 100.0);
  return buf;
}

// the device side of one evaluation
struct Walks {
  Checker check{query_failed};
  // string keys: the calls are the string ones, a missing key keeps up to max_value_bytes bytes, and every plan carries
  // the fingerprint key of the evaluation's first plan
  bool strings = false;
  uint32_t max_value_bytes = 0;
  bool have_key = false;
  uint8_t key[16];

  // (before the plan's first state)
  bool tuples = false;  // composite keys: the tuple calls, which are keyed too
  void keyed(tgx_plan *plan) {
    if (!strings && !tuples) return;
    if (have_key) check(tgx_plan_set_fingerprint_key(plan, key, &check.err));
    else check(tgx_plan_get_fingerprint_key(plan, key));
    have_key = true;
  }

  // `side` gathered: one {key, 1} record a non-NULL row (string keys: {hash_a, hash_b, n, 0} records).  (The records
  // stay the state's until its next call: `h` lives as long as they are read)
  void key_set(const Side &side, Handles &h, const void **records, uint64_t *n_records) {
    tgx_check_spec spec;
    memset(&spec, 0, sizeof(spec));
    spec.kind = TGX_CHECK_KEY_PROBE;
    spec.column = side.column;
    spec.column2 = -1;
    check(tgx_plan_create(&spec, 1, &h.plan, &check.err));
    keyed(h.plan);
    check(strings ? tgx_plan_set_key_probe_rows_strings(h.plan, 0, &check.err)
                  : tgx_plan_set_key_probe_rows(h.plan, 0, &check.err));
    check(tgx_state_create(h.plan, nullptr, &h.state, &check.err));
    for (const Batch &b : side.table->batches) check(tgx_update(h.plan, h.state, b.columns.data(), b.columns.size(), &check.err));
    check(tgx_key_probe_rows_get(h.plan, h.state, 0, records, n_records, &check.err));
  }

  // `near` walked once against the set of `records`: a counted probe (or a plain one); in the same plan, with
  // `distinct` a DISTINCT spec on the column, whose count goes there, and with `own_records` a spec that gathers the
  // column for the other direction; string keys: *long_rows are the missing rows whose value was too long to keep
  void probe(const Side &near, const void *records, uint64_t n_records, bool counted, uint32_t max_missing_keys,
             Handles &h, tgx_key_probe_summary *summary, tgx_key_probe_pairs *pairs, uint64_t *distinct,
             const void **own_records, uint64_t *own_n, uint64_t *long_rows) {
    tgx_check_spec specs[3];
    memset(specs, 0, sizeof(specs));
    size_t n = 1, gathers = 0, counts_distinct = 0;
    specs[0].kind = TGX_CHECK_KEY_PROBE;
    if (own_records) specs[gathers = n++].kind = TGX_CHECK_KEY_PROBE;
    if (distinct) specs[counts_distinct = n++].kind = TGX_CHECK_DISTINCT;
    if (distinct && strings) specs[counts_distinct].flags = TGX_FLAG_EXACT_KEYS;  // COUNT(DISTINCT) by value
    for (size_t i = 0; i < n; i++) {
      specs[i].column = near.column;
      specs[i].column2 = -1;
    }
    check(tgx_plan_create(specs, n, &h.plan, &check.err));
    keyed(h.plan);
    const tgx_key_probe_params params = {max_missing_keys, 0};
    const tgx_key_probe_strings_params string_params = {max_missing_keys, max_value_bytes};
    if (strings)
      check(counted ? tgx_plan_set_key_probe_strings_counted(h.plan, 0, &string_params, &check.err)
                    : tgx_plan_set_key_probe_strings(h.plan, 0, &string_params, &check.err));
    else
      check(counted ? tgx_plan_set_key_probe_counted(h.plan, 0, &params, &check.err)
                    : tgx_plan_set_key_probe(h.plan, 0, &params, &check.err));
    if (own_records)
      check(strings ? tgx_plan_set_key_probe_rows_strings(h.plan, gathers, &check.err)
                    : tgx_plan_set_key_probe_rows(h.plan, gathers, &check.err));
    check(tgx_state_create(h.plan, nullptr, &h.state, &check.err));
    check(tgx_key_probe_set_parent(h.plan, h.state, 0, records, n_records, &check.err));
    for (const Batch &b : near.table->batches) check(tgx_update(h.plan, h.state, b.columns.data(), b.columns.size(), &check.err));
    check(tgx_key_probe_get(h.plan, h.state, 0, summary, &check.err));
    if (counted) check(tgx_key_probe_pairs_get(h.plan, h.state, 0, pairs, &check.err));
    *long_rows = 0;
    if (strings) {
      tgx_key_probe_strings more;
      check(tgx_key_probe_strings_get(h.plan, h.state, 0, &more, &check.err));
      *long_rows = more.long_rows;
    }
    if (distinct) {
      tgx_result results[3];
      memset(results, 0, sizeof(results));
      check(tgx_finalize(h.plan, h.state, results, n, &check.err));
      *distinct = (uint64_t)results[counts_distinct].distinct;
    }
    if (own_records) check(tgx_key_probe_rows_get(h.plan, h.state, gathers, own_records, own_n, &check.err));
  }

  // ---- composite keys: the same two walks over the key columns of a side as ONE tuple key ----
  static void tuple_spec(tgx_check_spec *spec, const std::vector<int32_t> &columns) {
    spec->kind = TGX_CHECK_KEY_PROBE;
    spec->column = columns[0];
    spec->column2 = -1;
    spec->columns = columns.data();
    spec->n_columns = (uint32_t)columns.size();
  }
  void tuple_set(const Table &table, const std::vector<int32_t> &columns, Handles &h, const void **records,
                 uint64_t *n_records) {
    tgx_check_spec spec;
    memset(&spec, 0, sizeof(spec));
    tuple_spec(&spec, columns);
    check(tgx_plan_create(&spec, 1, &h.plan, &check.err));
    keyed(h.plan);
    check(tgx_plan_set_key_probe_rows_tuples(h.plan, 0, &check.err));
    check(tgx_state_create(h.plan, nullptr, &h.state, &check.err));
    for (const Batch &b : table.batches) check(tgx_update(h.plan, h.state, b.columns.data(), b.columns.size(), &check.err));
    check(tgx_key_probe_rows_get(h.plan, h.state, 0, records, n_records, &check.err));
  }
  // `distinct`: COUNT(DISTINCT) of the FIRST key column alone, by value when it is a string column
  void tuple_probe(const Table &near, const std::vector<int32_t> &columns, const void *records, uint64_t n_records,
                   bool counted, uint32_t max_missing_keys, Handles &h, tgx_key_probe_summary *summary,
                   tgx_key_probe_pairs *pairs, tgx_key_probe_tuples *more, uint64_t *distinct, bool distinct_is_string,
                   const void **own_records, uint64_t *own_n) {
    tgx_check_spec specs[3];
    memset(specs, 0, sizeof(specs));
    size_t n = 1, gathers = 0, counts_distinct = 0;
    tuple_spec(&specs[0], columns);
    if (own_records) tuple_spec(&specs[gathers = n++], columns);
    if (distinct) {
      counts_distinct = n++;
      specs[counts_distinct].kind = TGX_CHECK_DISTINCT;
      specs[counts_distinct].column = columns[0];
      specs[counts_distinct].column2 = -1;
      if (distinct_is_string) specs[counts_distinct].flags = TGX_FLAG_EXACT_KEYS;
    }
    check(tgx_plan_create(specs, n, &h.plan, &check.err));
    keyed(h.plan);
    const tgx_key_probe_params params = {max_missing_keys, 0};
    check(counted ? tgx_plan_set_key_probe_tuples_counted(h.plan, 0, &params, &check.err)
                  : tgx_plan_set_key_probe_tuples(h.plan, 0, &params, &check.err));
    if (own_records) check(tgx_plan_set_key_probe_rows_tuples(h.plan, gathers, &check.err));
    check(tgx_state_create(h.plan, nullptr, &h.state, &check.err));
    check(tgx_key_probe_set_parent(h.plan, h.state, 0, records, n_records, &check.err));
    for (const Batch &b : near.batches) check(tgx_update(h.plan, h.state, b.columns.data(), b.columns.size(), &check.err));
    check(tgx_key_probe_get(h.plan, h.state, 0, summary, &check.err));
    check(tgx_key_probe_tuples_get(h.plan, h.state, 0, more, &check.err));
    if (counted) check(tgx_key_probe_pairs_get(h.plan, h.state, 0, pairs, &check.err));
    if (distinct) {
      tgx_result results[3];
      memset(results, 0, sizeof(results));
      check(tgx_finalize(h.plan, h.state, results, n, &check.err));
      *distinct = (uint64_t)results[counts_distinct].distinct;
    }
    if (own_records) check(tgx_key_probe_rows_get(h.plan, h.state, gathers, own_records, own_n, &check.err));
  }
};

}  // namespace

ConstraintResult JoinCoverageConstraint::evaluate(const Inputs &) const {
  throw TermError{TermError::Internal, "join_coverage reads the tables of the context, not the suite's fused plan"};
}

void JoinCoverageConstraint::validate() const {
  // :165-176, then :181-188
  if (auto e = validate_identifier(left_)) throw *e;
  if (auto e = validate_identifier(right_)) throw *e;
  for (const auto &k : keys_) {
    if (auto e = validate_identifier(k.first)) throw *e;
    if (auto e = validate_identifier(k.second)) throw *e;
  }
  if (keys_.empty()) evaluation_error("No join keys specified. Use .on() or .on_multiple() to set join keys");
  if (keys_.size() > 1 && composite_ && keys_.size() > kMaxKeyPairs)
    evaluation_error("a join on " + std::to_string(keys_.size()) + " key pairs: composite keys on the device take 2 .. " +
                     std::to_string(kMaxKeyPairs) + " pairs (TGX_CHECK_KEY_PROBE's tuple keys)");
  if (keys_.size() > 1 && !composite_)
    evaluation_error("a join on " + std::to_string(keys_.size()) + " key pairs (" + left_ + "." + keys_[0].first + ", " +
                     left_ + "." + keys_[1].first + ", ..) is not on the GPU path: TGX_CHECK_KEY_PROBE takes one integer "
                     "key column");
  if (type_ == CoverageType::RightCoverage && distinct_only_)
    evaluation_error("distinct_only with RightCoverage counts the keys common to both sides (COUNT(DISTINCT " + left_ + "." +
                     keys_[0].first + ") over the right join's rows): that is not on the GPU path");
  if (max_missing_keys_ < 1 || max_missing_keys_ > TGX_KEY_PROBE_MAX_MISSING_KEYS)
    evaluation_error("max_missing_keys must be 1 .. " + std::to_string((int)TGX_KEY_PROBE_MAX_MISSING_KEYS) + " (" +
                     std::to_string(max_missing_keys_) + ")");
  if (max_value_bytes_ < 1 || max_value_bytes_ > TGX_KEY_PROBE_MAX_VALUE_BYTES)
    evaluation_error("max_value_bytes must be 1 .. " + std::to_string((int)TGX_KEY_PROBE_MAX_VALUE_BYTES) + " (" +
                     std::to_string(max_value_bytes_) + ")");
}

// :327-421
ConstraintResult JoinCoverageConstraint::verdict(const JoinCoverageCounts &c) const {
  const bool left = type_ != CoverageType::RightCoverage, right = type_ != CoverageType::LeftCoverage;
  if ((left && !c.left.known) || (right && !c.right.known))
    throw TermError{TermError::Internal, "join_coverage: the counts of a side the coverage type reads are missing"};
  double rate = 0.0;
  bool first = true;
  auto take = [&](uint64_t matched, uint64_t total) {
    // (the reference divides NULL by zero here and then reads a NULL slot's value)
    if (total == 0) evaluation_error("the join of '" + left_ + "' and '" + right_ + "' has no rows: there is no match rate");
    const double r = (double)matched / (double)total;
    rate = first ? r : std::min(rate, r);  // LEAST
    first = false;
  };
  // distinct_only: COUNT(DISTINCT L.l) under the same numerator, so the rate can exceed 1; Bidirectional ignores it
  if (left) take(c.left.pairs, type_ == CoverageType::LeftCoverage && distinct_only_ ? c.left_distinct : c.left.join_rows);
  if (right) take(c.right.pairs, c.right.join_rows);
  if (rate >= expected_) return ConstraintResult::success_with_metric(rate);

  const char *arrow = type_ == CoverageType::LeftCoverage ? " -> " : type_ == CoverageType::RightCoverage ? " <- " : " <-> ";
  std::string message = "Join coverage constraint failed: " + left_ + arrow + right_ + " coverage is " + percent(rate) +
                        "% (expected: " + percent(expected_) + "%)";
  // the examples: SELECT DISTINCT L.l FROM L LEFT JOIN R .. WHERE R.r IS NULL LIMIT n, always from the left side; a NULL
  // is one distinct value (:289-324, :386-400).  (A long missing value is a distinct left value the table did not keep:
  // it makes the number a lower bound as an overflow row does)
  if (max_examples_ > 0) {
    if (!c.examples_known)
      throw TermError{TermError::Internal, "join_coverage: a failing check with examples needs the left side's missing keys"};
    // (composite keys: every distinct tuple with a NULL component is a value of its own)
    const uint64_t null_values = c.null_keys_known ? c.null_keys : (c.null_rows > 0 ? 1 : 0);
    const uint64_t found = c.missing_keys + null_values, n = std::min<uint64_t>(max_examples_, found);
    if (n > 0)
      message += std::string(" (") + ((c.overflow_rows > 0 || c.long_rows > 0 || c.null_overflow_rows > 0) && n < max_examples_ ? "at least " : "") + std::to_string(n) +
                 " unmatched examples found)";
  }
  return ConstraintResult::failure_with_metric(rate, message);
}

// 2 .. 8 key pairs under the opt-in: the three walk patterns with the tuple calls
ConstraintResult JoinCoverageConstraint::evaluate_composite(const Context &ctx) const {
  std::vector<int32_t> lcols, rcols;
  const Table *lt = nullptr, *rt = nullptr;
  bool first_is_string = false;
  for (size_t k = 0; k < keys_.size(); k++) {
    const Side L = side_of(ctx, left_, keys_[k].first), R = side_of(ctx, right_, keys_[k].second);
    lt = L.table;
    rt = R.table;
    // (a side without a batch has no type to object with: it goes the way of the other side)
    const int ls = string_side(*L.table, L.column), rs = string_side(*R.table, R.column);
    if (ls != 1) integer_side(L);  // (Float, UInt64 and Boolean columns: the wording of before)
    if (rs != 1) integer_side(R);
    if ((ls == 1 && rs == -1) || (ls == -1 && rs == 1))
      evaluation_error("key pair " + std::to_string(k) + ": columns '" + L.qualified + "' and '" + R.qualified + "' are " +
                       (ls == 1 ? "a string and an integer" : "an integer and a string") +
                       " column: the two columns of a key pair are two integer columns or two string columns");
    if (k == 0) first_is_string = ls == 1;
    lcols.push_back(L.column);
    rcols.push_back(R.column);
  }
  Walks w;
  w.tuples = true;
  w.check(tgx_init(nullptr, &w.check.err));

  JoinCoverageCounts counts;
  tgx_key_probe_summary s;
  tgx_key_probe_pairs p;
  tgx_key_probe_tuples more;
  memset(&p, 0, sizeof(p));
  auto note_examples = [&](const tgx_key_probe_summary &of_left, const tgx_key_probe_tuples &nulls) {
    counts.examples_known = true;
    counts.missing_keys = of_left.missing_keys;
    counts.null_rows = of_left.null_rows;
    counts.overflow_rows = of_left.overflow_rows;
    counts.null_keys_known = true;
    counts.null_keys = nulls.null_keys;
    counts.null_overflow_rows = nulls.null_overflow_rows;
  };
  const void *records = nullptr, *left_records = nullptr;
  uint64_t n_records = 0, n_left = 0;
  Handles r_set, l_walk, r_walk, l_set, l_plain;
  if (type_ != CoverageType::RightCoverage) {
    const bool both = type_ == CoverageType::BidirectionalCoverage;
    w.tuple_set(*rt, rcols, r_set, &records, &n_records);
    w.tuple_probe(*lt, lcols, records, n_records, true, max_missing_keys_, l_walk, &s, &p, &more,
                  !both && distinct_only_ ? &counts.left_distinct : nullptr, first_is_string,
                  both ? &left_records : nullptr, &n_left);
    counts.left.known = true;
    counts.left.pairs = p.pairs;
    counts.left.join_rows = p.join_rows;
    note_examples(s, more);
    if (both) {
      w.tuple_probe(*rt, rcols, left_records, n_left, true, max_missing_keys_, r_walk, &s, &p, &more, nullptr, false,
                    nullptr, nullptr);
      counts.right.known = true;
      counts.right.pairs = p.pairs;
      counts.right.join_rows = p.join_rows;
    }
    return verdict(counts);
  }
  w.tuple_set(*lt, lcols, l_set, &left_records, &n_left);
  w.tuple_probe(*rt, rcols, left_records, n_left, true, max_missing_keys_, r_walk, &s, &p, &more, nullptr, false, nullptr,
                nullptr);
  counts.right.known = true;
  counts.right.pairs = p.pairs;
  counts.right.join_rows = p.join_rows;
  const bool fails = p.join_rows != 0 && !((double)p.pairs / (double)p.join_rows >= expected_);
  if (fails && wants_examples()) {
    w.tuple_set(*rt, rcols, r_set, &records, &n_records);
    w.tuple_probe(*lt, lcols, records, n_records, false, max_missing_keys_, l_plain, &s, &p, &more, nullptr, false, nullptr,
                  nullptr);
    note_examples(s, more);
  }
  return verdict(counts);
}

ConstraintResult JoinCoverageConstraint::evaluate_context(const Context &ctx) const {
  validate();
  if (keys_.size() > 1) return evaluate_composite(ctx);
  const Side L = side_of(ctx, left_, keys_[0].first), R = side_of(ctx, right_, keys_[0].second);
  // (a side without a batch has no type to object with: it goes the way of the other side)
  const int ls = string_side(*L.table, L.column), rs = string_side(*R.table, R.column);
  Walks w;
  w.strings = ls >= 0 && rs >= 0 && ls + rs > 0;
  w.max_value_bytes = max_value_bytes_;
  if (!w.strings) {
    if (ls != 1) integer_side(L);
    if (rs != 1) integer_side(R);
    if (ls == 1 || rs == 1)
      evaluation_error("columns '" + L.qualified + "' and '" + R.qualified + "' are " +
                       (ls == 1 ? "a string and an integer" : "an integer and a string") +
                       " column: join keys of different kinds are not on the GPU path (TGX_CHECK_KEY_PROBE takes two "
                       "integer columns or two string columns)");
  }
  w.check(tgx_init(nullptr, &w.check.err));

  JoinCoverageCounts counts;
  tgx_key_probe_summary s;
  tgx_key_probe_pairs p;
  memset(&p, 0, sizeof(p));
  uint64_t long_rows = 0;
  auto note_examples = [&](const tgx_key_probe_summary &of_left) {
    counts.examples_known = true;
    counts.missing_keys = of_left.missing_keys;
    counts.null_rows = of_left.null_rows;
    counts.overflow_rows = of_left.overflow_rows;
    counts.long_rows = long_rows;
  };
  const void *records = nullptr, *left_records = nullptr;
  uint64_t n_records = 0, n_left = 0;
  Handles r_set, l_walk, r_walk, l_set, l_plain;
  if (type_ != CoverageType::RightCoverage) {
    // R's rows, then L once: the probe, L's DISTINCT where distinct_only reads it, L's rows for the other direction
    const bool both = type_ == CoverageType::BidirectionalCoverage;
    w.key_set(R, r_set, &records, &n_records);
    w.probe(L, records, n_records, true, max_missing_keys_, l_walk, &s, &p,
            !both && distinct_only_ ? &counts.left_distinct : nullptr, both ? &left_records : nullptr, &n_left, &long_rows);
    counts.left.known = true;
    counts.left.pairs = p.pairs;
    counts.left.join_rows = p.join_rows;
    note_examples(s);
    if (both) {
      uint64_t unread = 0;
      w.probe(R, left_records, n_left, true, max_missing_keys_, r_walk, &s, &p, nullptr, nullptr, nullptr, &unread);
      counts.right.known = true;
      counts.right.pairs = p.pairs;
      counts.right.join_rows = p.join_rows;
    }
    return verdict(counts);
  }
  w.key_set(L, l_set, &left_records, &n_left);
  w.probe(R, left_records, n_left, true, max_missing_keys_, r_walk, &s, &p, nullptr, nullptr, nullptr, &long_rows);
  counts.right.known = true;
  counts.right.pairs = p.pairs;
  counts.right.join_rows = p.join_rows;
  // a failing check with examples: one plain probe of L against R's set
  const bool fails = p.join_rows != 0 && !((double)p.pairs / (double)p.join_rows >= expected_);
  if (fails && wants_examples()) {
    w.key_set(R, r_set, &records, &n_records);
    w.probe(L, records, n_records, false, max_missing_keys_, l_plain, &s, &p, nullptr, nullptr, nullptr, &long_rows);
    note_examples(s);
  }
  return verdict(counts);
}

Check::Builder &Check::Builder::join_coverage(std::string left_table, std::string right_table) {
  return constraint(std::make_shared<JoinCoverageConstraint>(std::move(left_table), std::move(right_table)));
}

}  // namespace term_guard
