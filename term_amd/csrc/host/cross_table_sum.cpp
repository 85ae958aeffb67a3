// cross_table_sum.cpp -- CrossTableSumConstraint (TG/constraints/cross_table_sum.rs).  The reference runs one SQL
// statement over both tables; here each side is one walk of its table on the device and the join runs on the host:
//   ungrouped   COALESCE((SELECT SUM(col) FROM t), 0.0) per side (:209-213): a TGX_CHECK_NUMERIC_STATS spec
//   grouped     SELECT g, COALESCE(SUM(col), 0.0) FROM t GROUP BY g per side (:251-262): a TGX_CHECK_GROUP_SUMS spec,
//               then the FULL OUTER JOIN on l.g = r.g and the aggregate over it (:263-279) below
//   grouped by several columns (an opt-in, composite_groups_on_device): each side is one GROUP_SUMS walk on the TUPLE of
//               the group_by columns, whose entries are encoded tuple keys (group_key.h); the join merges the two entry
//               lists by those bytes, and a key with a NULL component never joins (join_tuples below)
// A sum is a double when it is compared: an integer column's SUM is DataFusion's wrapping Int64 sum, cast by the
// COALESCE with 0.0 -- after the sum (the reader downcasts the result to Float64Array, :536-570).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../group_key.h"
#include "term_guard.h"
#include "tgx_handles.h"

namespace term_guard {

namespace {

[[noreturn]] void evaluation_error(const std::string &msg) {
  throw TermError{TermError::ConstraintEvaluation, "'cross_table_sum': " + msg};
}
[[noreturn]] void query_failed(const std::string &why) {  // (:490-495)
  evaluation_error("Cross-table sum validation query failed: " + why);
}

// Rust's {:.4}
std::string fixed4(double v) {
  if (isnan(v)) return "NaN";
  if (isinf(v)) return v > 0 ? "inf" : "-inf";
  char buf[400];
  snprintf(buf, sizeof(buf), "%.4f", v);
  return buf;
}

int column_index(const Table &t, const std::string &name) {
  for (size_t i = 0; i < t.column_names.size(); i++)
    if (t.column_names[i] == name) return (int)i;
  return -1;
}

bool is_float_type(int type) { return type == TGX_FLOAT64 || type == TGX_FLOAT32; }

// one side of the comparison: its table walked once.  `group` empty: the ungrouped form, whose sum comes back in
// *total; otherwise the side's groups in *sums
// `more_groups`: the further group_by columns (then the side groups by the tuple (group, more_groups..))
void walk_side(const Context &ctx, const std::string &table_name, const std::string &column, const std::string &group,
               uint32_t max_groups, double *total, SideSums *sums, const std::vector<std::string> &more_groups = {}) {
  const Table *table = ctx.table(table_name);
  if (!table) query_failed("Error during planning: table 'datafusion.public." + table_name + "' not found");
  const int vi = column_index(*table, column), gi = group.empty() ? -1 : column_index(*table, group);
  if (vi < 0) query_failed("Schema error: No field named " + column + ".");
  if (!group.empty() && gi < 0) query_failed("Schema error: No field named " + group + ".");
  std::vector<int32_t> list;
  if (!more_groups.empty()) {
    list.push_back(gi);
    for (const std::string &g : more_groups) {
      list.push_back(column_index(*table, g));
      if (list.back() < 0) query_failed("Schema error: No field named " + g + ".");
    }
  }

  tgx_check_spec spec;
  memset(&spec, 0, sizeof(spec));
  spec.kind = group.empty() ? TGX_CHECK_NUMERIC_STATS : TGX_CHECK_GROUP_SUMS;
  spec.column = vi;
  spec.column2 = list.empty() ? gi : -1;
  if (!list.empty()) {
    spec.columns = list.data();
    spec.n_columns = (uint32_t)list.size();
  }
  Handles h;
  Checker check(query_failed);
  tgx_error &err = check.err;
  check(tgx_init(nullptr, &err));
  check(tgx_plan_create(&spec, 1, &h.plan, &err));
  if (!group.empty()) {
    const tgx_group_sums_params p = {max_groups, TGX_GROUP_SUMS_MAX_VALUE_BYTES};
    check(tgx_plan_set_group_sums(h.plan, 0, &p, &err));
  }
  check(tgx_state_create(h.plan, nullptr, &h.state, &err));
  bool is_float = false;
  for (const Batch &b : table->batches) {
    if ((size_t)vi < b.columns.size()) is_float = is_float || is_float_type(b.columns[vi].type);
    check(tgx_update(h.plan, h.state, b.columns.data(), b.columns.size(), &err));
  }
  if (group.empty()) {
    tgx_result r;
    memset(&r, 0, sizeof(r));
    check(tgx_finalize(h.plan, h.state, &r, 1, &err));
    *total = !r.has_value ? 0.0 : is_float ? r.sum_f : (double)r.sum_i;
    return;
  }
  tgx_group_sums_summary s;
  check(tgx_group_sums_get(h.plan, h.state, 0, &s, &err));
  uint64_t n = 0, nb = 0;
  int32_t is_bytes = 0;
  check(tgx_group_sums_entries(h.plan, h.state, 0, nullptr, 0, &n, nullptr, 0, &nb, &is_bytes, &err));
  std::vector<tgx_group_sum_entry> entries((size_t)n + 1);
  std::vector<uint8_t> bytes((size_t)nb + 1);
  check(tgx_group_sums_entries(h.plan, h.state, 0, entries.data(), n, &n, bytes.data(), nb, &nb, &is_bytes, &err));
  sums->is_bytes = is_bytes != 0;
  sums->arity = (int)list.size();
  sums->overflow_rows = s.overflow.rows;
  sums->long_rows = s.long_rows.rows;
  if (s.null_group.rows) sums->null_group = s.null_group.sum_f;  // (sum_f: the double, or the Int64 sum cast)
  for (uint64_t i = 0; i < n; i++) {
    SideSums::Group g;
    g.value = entries[i].value;
    if (sums->is_bytes) g.bytes.assign((const char *)bytes.data() + entries[i].offset, (size_t)entries[i].length);
    g.sum = entries[i].sum_f;
    sums->groups.push_back(std::move(g));
  }
}

}  // namespace

ConstraintResult Constraint::evaluate_context(const Context &) const {
  throw TermError{TermError::Internal, "constraint '" + name() + "' does not read the context"};
}

ConstraintResult CrossTableSumConstraint::evaluate(const Inputs &) const {
  throw TermError{TermError::Internal, "cross_table_sum reads the tables of the context, not the suite's fused plan"};
}

// :158-175
std::pair<std::string, std::string> CrossTableSumConstraint::parse_qualified_column(const std::string &qualified) {
  std::vector<std::string> parts(1);
  for (char ch : qualified) {
    if (ch == '.') parts.emplace_back();
    else parts.back().push_back(ch);
  }
  if (parts.size() != 2) evaluation_error("Column must be qualified (table.column): '" + qualified + "'");
  if (auto e = validate_identifier(parts[0])) throw *e;
  if (auto e = validate_identifier(parts[1])) throw *e;
  return {parts[0], parts[1]};
}

CrossTableSumRow CrossTableSumConstraint::totals(double l, double r) const {  // :203-213
  CrossTableSumRow row;
  row.total_groups = 1;
  row.max_difference = fabs(l - r);
  row.violating_groups = row.max_difference > tolerance_ ? 1 : 0;  // (NaN > tolerance is false, as in SQL)
  row.total_left_sum = l;
  row.total_right_sum = r;
  return row;
}

// The FULL OUTER JOIN on l.g = r.g (:263-272) and the aggregate over it (:273-279).  A key on one side only is a group
// against 0.0; NULL = NULL is not true, so NULL keys never join: each side's NULL group is a group of its own against
// 0.0.  The totals add the groups in ascending key order, the NULL groups last, the left one first (SQL leaves the order
// open).  A NaN difference is no violation and makes max_difference NaN.
CrossTableSumRow CrossTableSumConstraint::join(const SideSums &left, const SideSums &right) const {
  if (groups_by_tuple()) return join_tuples(left, right);  // (the opt-in and 2 .. 8 columns; else the join it always was)
  const std::string bound = "max_groups = " + std::to_string(max_groups_) + " (keys of at most " +
                            std::to_string((int)TGX_GROUP_SUMS_MAX_VALUE_BYTES) + " bytes)";
  const SideSums *sides[2] = {&left, &right};
  for (int i = 0; i < 2; i++)
    if (sides[i]->overflow_rows || sides[i]->long_rows)
      evaluation_error("the " + std::string(i ? "right" : "left") + " side has more groups than the bound " + bound +
                       " holds: " + std::to_string(sides[i]->overflow_rows) + " overflow rows, " +
                       std::to_string(sides[i]->long_rows) + " rows with a longer key; no verdict on partial sums");
  if (!left.groups.empty() && !right.groups.empty() && left.is_bytes != right.is_bytes)
    evaluation_error("the group columns of the two sides must both be integer or both be string columns (the left one "
                     "holds " + std::string(left.is_bytes ? "strings" : "integers") + ", the right one " +
                     (right.is_bytes ? "strings" : "integers") + ")");
  CrossTableSumRow row;
  bool nan_difference = false;
  auto group = [&](double l, double r) {
    const double diff = fabs(l - r);
    row.total_groups++;
    row.violating_groups += diff > tolerance_ ? 1 : 0;
    row.total_left_sum += l;
    row.total_right_sum += r;
    if (isnan(diff)) nan_difference = true;
    else if (diff > row.max_difference) row.max_difference = diff;
  };
  const bool strings = left.groups.empty() ? right.is_bytes : left.is_bytes;
  auto before = [&](const SideSums::Group &a, const SideSums::Group &b) {
    return strings ? a.bytes < b.bytes : a.value < b.value;  // (std::string compares as unsigned bytes)
  };
  size_t i = 0, j = 0;
  while (i < left.groups.size() || j < right.groups.size()) {
    if (j == right.groups.size() || (i < left.groups.size() && before(left.groups[i], right.groups[j]))) {
      group(left.groups[i++].sum, 0.0);
    } else if (i == left.groups.size() || before(right.groups[j], left.groups[i])) {
      group(0.0, right.groups[j++].sum);
    } else {
      group(left.groups[i++].sum, right.groups[j++].sum);
    }
  }
  if (left.null_group) group(*left.null_group, 0.0);
  if (right.null_group) group(0.0, *right.null_group);
  if (nan_difference) row.max_difference = NAN;
  return row;
}

// The join for 2 .. 8 group columns: the sides' entries are encoded tuple keys, ascending bytewise -- one order for both
// sides once every position holds one kind of value, so the outer join is a merge by bytes.  A key with a NULL component
// on either side never joins (NULL = NULL is not true): each is a group of its own against 0.0, added after the joined
// groups, the left side's first.  A position that holds integers on one side and strings on the other is this
// constraint's error (the reference's SQL would fail to plan the comparison): judged by the tags of the entries.
CrossTableSumRow CrossTableSumConstraint::join_tuples(const SideSums &left, const SideSums &right) const {
  const std::string bound = "max_groups = " + std::to_string(max_groups_) + " (encoded keys of at most " +
                            std::to_string((int)TGX_GROUP_SUMS_MAX_VALUE_BYTES) + " bytes)";
  const SideSums *sides[2] = {&left, &right};
  const size_t arity = group_by_.size();
  if (arity < 2 || arity > (size_t)tgx::kGroupKeyMaxArity)  // (join() routes here within the bound only)
    evaluation_error("a join on tuple keys takes 2 .. " + std::to_string(tgx::kGroupKeyMaxArity) + " group_by columns (" +
                     std::to_string(arity) + ")");
  // per side and position: does it hold integers, strings?  per group: has it a NULL component?
  bool holds[2][tgx::kGroupKeyMaxArity][3] = {};  // (arity is within it; a decoded cell's tag is 0 .. 2)
  static_assert(tgx::kGroupKeyMaxArity == 8, "groups_by_tuple() bounds the columns by 8");
  std::vector<char> with_null[2];
  for (int i = 0; i < 2; i++) {
    if ((size_t)sides[i]->arity != arity)
      evaluation_error("the " + std::string(i ? "right" : "left") + " side was grouped by " +
                       std::to_string(sides[i]->arity) + " columns, the constraint groups by " + std::to_string(arity));
    if (sides[i]->overflow_rows || sides[i]->long_rows)
      evaluation_error("the " + std::string(i ? "right" : "left") + " side has more groups than the bound " + bound +
                       " holds: " + std::to_string(sides[i]->overflow_rows) + " overflow rows, " +
                       std::to_string(sides[i]->long_rows) + " rows with a longer key; no verdict on partial sums");
    for (const SideSums::Group &g : sides[i]->groups) {
      std::vector<tgx::GroupKeyCell> cells;
      if (!sides[i]->is_bytes || !tgx::group_key_decode((const uint8_t *)g.bytes.data(), g.bytes.size(), &cells) ||
          cells.size() != arity)
        evaluation_error("a group key of the " + std::string(i ? "right" : "left") + " side is not the encoded form of a "
                         "tuple of " + std::to_string(arity) + " columns");
      bool any_null = false;
      for (size_t c = 0; c < arity; c++) {
        holds[i][c][cells[c].tag] = true;
        any_null |= cells[c].tag == tgx::kGroupKeyNull;
      }
      with_null[i].push_back(any_null ? 1 : 0);
    }
  }
  for (size_t c = 0; c < arity; c++)
    for (int i = 0; i < 2; i++)
      if (holds[i][c][tgx::kGroupKeyInt] && holds[1 - i][c][tgx::kGroupKeyString])
        evaluation_error("group column " + std::to_string(c) + " ('" + group_by_[c] + "') holds integers on the " +
                         (i ? "right" : "left") + " side and strings on the " + (i ? "left" : "right") +
                         " side: the two sides' group columns must be of one kind, position by position");
  CrossTableSumRow row;
  bool nan_difference = false;
  auto group = [&](double l, double r) {
    const double diff = fabs(l - r);
    row.total_groups++;
    row.violating_groups += diff > tolerance_ ? 1 : 0;
    row.total_left_sum += l;
    row.total_right_sum += r;
    if (isnan(diff)) nan_difference = true;
    else if (diff > row.max_difference) row.max_difference = diff;
  };
  size_t i = 0, j = 0;
  const size_t nl = left.groups.size(), nr = right.groups.size();
  while (true) {
    while (i < nl && with_null[0][i]) i++;
    while (j < nr && with_null[1][j]) j++;
    if (i == nl && j == nr) break;
    if (j == nr || (i < nl && left.groups[i].bytes < right.groups[j].bytes)) {  // (std::string compares as unsigned bytes)
      group(left.groups[i++].sum, 0.0);
    } else if (i == nl || right.groups[j].bytes < left.groups[i].bytes) {
      group(0.0, right.groups[j++].sum);
    } else {
      group(left.groups[i++].sum, right.groups[j++].sum);
    }
  }
  for (size_t k = 0; k < nl; k++)
    if (with_null[0][k]) group(left.groups[k].sum, 0.0);
  for (size_t k = 0; k < nr; k++)
    if (with_null[1][k]) group(0.0, right.groups[k].sum);
  if (nan_difference) row.max_difference = NAN;
  return row;
}

// :572-630
ConstraintResult CrossTableSumConstraint::verdict(const CrossTableSumRow &row) const {
  if (row.violating_groups == 0) return ConstraintResult::success_with_metric(row.max_difference);
  const std::string tolerance_text =
      tolerance_ > 0.0 ? " (tolerance: " + fixed4(tolerance_) + ")" : std::string(" (exact match required)");
  std::string grouping_text = "overall totals";
  if (!group_by_.empty()) {
    grouping_text = "groups by [";
    for (size_t i = 0; i < group_by_.size(); i++) grouping_text += (i ? ", " : "") + group_by_[i];
    grouping_text += "]";
  }
  const std::string head = "Cross-table sum mismatch: " + std::to_string(row.violating_groups) + "/" +
                           std::to_string(row.total_groups) + " " + grouping_text + " failed validation" + tolerance_text;
  std::string message;
  if (group_by_.empty() && max_violations_ > 0) {
    // examples are collected for the ungrouped form only (:409-413), where there is exactly one: 'ALL' (:303-314)
    message = head + ". Examples: [Group 'ALL': " + left_ + " = " + fixed4(row.total_left_sum) + ", " + right_ + " = " +
              fixed4(row.total_right_sum) + " (diff: " + fixed4(row.max_difference) + ")]";
  } else {
    message = head + ", total sums: " + rust_f64(row.total_left_sum) + " vs " + rust_f64(row.total_right_sum) +
              " (max diff: " + fixed4(row.max_difference) + ")";
  }
  return ConstraintResult::failure_with_metric(row.max_difference, message);
}

ConstraintResult CrossTableSumConstraint::evaluate_context(const Context &ctx) const {
  const auto left = parse_qualified_column(left_), right = parse_qualified_column(right_);
  for (const std::string &g : group_by_)  // :178-183
    if (auto e = validate_identifier(g)) throw *e;
  const bool tuples = groups_by_tuple();
  if (group_by_.size() > 1 && !tuples)
    evaluation_error("GROUP BY over " + std::to_string(group_by_.size()) +
                     " columns is not on the GPU path: TGX_CHECK_GROUP_SUMS groups by exactly one column");
  if (max_groups_ < 1 || max_groups_ > TGX_GROUP_SUMS_MAX_GROUPS)
    evaluation_error("max_groups must be 1 .. " + std::to_string((int)TGX_GROUP_SUMS_MAX_GROUPS) + " (" +
                     std::to_string(max_groups_) + ")");
  if (group_by_.empty()) {
    double l = 0, r = 0;
    walk_side(ctx, left.first, left.second, std::string(), 0, &l, nullptr);
    walk_side(ctx, right.first, right.second, std::string(), 0, &r, nullptr);
    return verdict(totals(l, r));
  }
  SideSums ls, rs;
  const std::vector<std::string> more(group_by_.begin() + 1, group_by_.end());
  walk_side(ctx, left.first, left.second, group_by_[0], max_groups_, nullptr, &ls, more);
  walk_side(ctx, right.first, right.second, group_by_[0], max_groups_, nullptr, &rs, more);
  // both tables empty: COUNT(*) = 0 and NULL aggregates whose slots the reference reads with .value(0) (:512-570);
  // arrow leaves the slot of a NULL zeroed, so it sees 0 violating groups and succeeds with metric 0.0 -- what join()
  // returns for no groups
  return verdict(join(ls, rs));
}

Check::Builder &Check::Builder::cross_table_sum(std::string left_column, std::string right_column) {
  return constraint(std::make_shared<CrossTableSumConstraint>(std::move(left_column), std::move(right_column)));
}

}  // namespace term_guard
