// foreign_key.cpp -- ForeignKeyConstraint (TG/constraints/foreign_key.rs).  The reference runs
//   SELECT COUNT(*), COUNT(DISTINCT child.c) FROM child LEFT JOIN parent ON child.c = parent.p
//   WHERE parent.p IS NULL [AND child.c IS NOT NULL]                                                      (:152-176)
// and a SELECT DISTINCT .. LIMIT n for the examples (:179-207).  Here the parent's column is walked once under a
// TGX_CHECK_DISTINCT spec, its key set is exported (world 1) into the TGX_CHECK_KEY_PROBE spec of the child's column,
// and the child is walked once: membership per row on the device, the verdict and the message on the host.  A NULL
// parent row is no key of the set (NULL = x is not true), a NULL child row matches nothing: it is a violation unless
// allow_nulls.  Integer keys, or string keys when BOTH columns are string layouts (Utf8, LargeUtf8, Utf8View,
// Dictionary<Int32, Utf8>): the parent's export is then the values' keyed fingerprints, the child's plan takes the
// parent plan's fingerprint key, and the probe is a strings spec (tgx_plan_set_key_probe_strings).  Every other column
// type, and a pair of an integer and a string column, is the constraint's own error, so the caller can hand the
// constraint to the stock path.
#include <string.h>

#include "term_guard.h"
#include "tgx_handles.h"

namespace term_guard {

namespace {

[[noreturn]] void evaluation_error(const std::string &msg) {
  throw TermError{TermError::ConstraintEvaluation, "'foreign_key': " + msg};
}
[[noreturn]] void query_failed(const std::string &why) {  // (:320-325)
  evaluation_error("Foreign key validation query failed: " + why);
}

// the table and the index of the column behind a qualified name, with the reference's planning / schema errors
const Table *side_of(const Context &ctx, const std::pair<std::string, std::string> &name, int *index) {
  const Table *table = ctx.table(name.first);
  if (!table) query_failed("Error during planning: table 'datafusion.public." + name.first + "' not found");
  *index = -1;
  for (size_t i = 0; i < table->column_names.size(); i++)
    if (table->column_names[i] == name.second) *index = (int)i;
  if (*index < 0) query_failed("Schema error: No field named " + name.second + ".");
  return table;
}

// the first batch's type of the column (0: no batch has it)
int first_type(const Table &table, int index) {
  for (const Batch &b : table.batches)
    if ((size_t)index < b.columns.size()) return b.columns[index].type;
  return 0;
}

// the column's type over the table's batches (0: no batch has the column); integer keys only
int key_type(const Table &table, int index, const std::string &qualified) {
  int type = 0;
  for (const Batch &b : table.batches)
    if ((size_t)index < b.columns.size()) {
      const int t = b.columns[index].type;
      if (const char *name = off_path_type(t))
        evaluation_error("column '" + qualified + "' is a " + name +
                         " column: foreign keys of that type are not on the GPU path (TGX_CHECK_KEY_PROBE takes integer "
                         "keys)");
      if (type == 0) type = t;
    }
  return type;
}

// The two walks of an evaluation, the same for integer and for string keys.
// the parent: its column walked under a DISTINCT spec, and the records of its distinct non-NULL keys (Int32 / narrow
// columns as their sign- or zero-extended int64 values, strings as fingerprints under the plan's key).  The records stay
// the parent state's until its next call: `p` lives to the end
void export_parent(Checker &check, const Table &table, int column, Handles &p, const void **records, uint64_t *n_records) {
  tgx_check_spec spec;
  memset(&spec, 0, sizeof(spec));
  spec.kind = TGX_CHECK_DISTINCT;
  spec.column = column;
  spec.column2 = -1;
  check(tgx_plan_create(&spec, 1, &p.plan, &check.err));
  check(tgx_state_create(p.plan, nullptr, &p.state, &check.err));
  for (const Batch &b : table.batches) check(tgx_update(p.plan, p.state, b.columns.data(), b.columns.size(), &check.err));
  check(tgx_distinct_export(p.plan, p.state, 0, 1, records, n_records, &check.err));
}

// the child: its column walked under a KEY_PROBE spec against that set; `set` makes the plan's tgx_plan_set_key_probe*
// call (and hands over what its mode needs beside it).  The summary; the entries are read by the caller
tgx_key_probe_summary probe_child(Checker &check, const Table &table, int column, const void *records, uint64_t n_records,
                                  Handles &c, const std::function<void(tgx_plan *)> &set) {
  tgx_check_spec spec;
  memset(&spec, 0, sizeof(spec));
  spec.kind = TGX_CHECK_KEY_PROBE;
  spec.column = column;
  spec.column2 = -1;
  check(tgx_plan_create(&spec, 1, &c.plan, &check.err));
  set(c.plan);
  check(tgx_state_create(c.plan, nullptr, &c.state, &check.err));
  check(tgx_key_probe_set_parent(c.plan, c.state, 0, records, n_records, &check.err));
  for (const Batch &b : table.batches) check(tgx_update(c.plan, c.state, b.columns.data(), b.columns.size(), &check.err));
  tgx_key_probe_summary s;
  check(tgx_key_probe_get(c.plan, c.state, 0, &s, &check.err));
  return s;
}

}  // namespace

ConstraintResult ForeignKeyConstraint::evaluate(const Inputs &) const {
  throw TermError{TermError::Internal, "foreign_key reads the tables of the context, not the suite's fused plan"};
}

// :130-149
std::pair<std::string, std::string> ForeignKeyConstraint::parse_qualified_column(const std::string &qualified) {
  std::vector<std::string> parts(1);
  for (char ch : qualified) {
    if (ch == '.') parts.emplace_back();
    else parts.back().push_back(ch);
  }
  if (parts.size() != 2) evaluation_error("Foreign key column must be qualified (table.column): '" + qualified + "'");
  if (auto e = validate_identifier(parts[0])) throw *e;
  if (auto e = validate_identifier(parts[1])) throw *e;
  return {parts[0], parts[1]};
}

// :334-410.  total_violations = COUNT(*) over the rows the join left without a parent: the missing rows, and the NULL
// rows unless allow_nulls filters them; unique_violations = COUNT(DISTINCT child.c), which counts no NULL
ConstraintResult ForeignKeyConstraint::verdict(const ForeignKeyCounts &c) const {
  const uint64_t total = c.missing_rows + (allow_nulls_ ? 0 : c.null_rows);
  if (total == 0) return ConstraintResult::success();
  const std::string unique = (c.overflow_rows || c.long_rows ? "at least " : "") + std::to_string(c.missing_keys);
  std::string message = "Foreign key constraint violation: " + std::to_string(total) + " values in '" + child_ +
                        "' do not exist in '" + parent_ + "' (total: " + std::to_string(total) + ", unique: " + unique + ")";
  // the examples: the max_violations_reported smallest missing keys (the reference's LIMIT has no order; a NULL takes
  // no slot here); up to 5 are listed (:387-395)
  // (string keys are printed raw, as the reference's join(", ") prints them)
  const size_t n = c.examples ? std::min(c.strings ? c.str_keys.size() : c.keys.size(), max_violations_) : 0;
  if (n > 0) {
    std::string list;
    for (size_t i = 0; i < std::min<size_t>(n, 5); i++)
      list += (i ? ", " : "") + (c.strings ? c.str_keys[i] : std::to_string(c.keys[i]));
    if (n > 5) list += ", ... (" + std::to_string(n - 5) + " more)";
    message += ". Examples: [" + list + "]";
  }
  return ConstraintResult::failure_with_metric((double)total, message);
}

ConstraintResult ForeignKeyConstraint::evaluate_context(const Context &ctx) const {
  const auto child = parse_qualified_column(child_), parent = parse_qualified_column(parent_);
  if (max_missing_keys_ < 1 || max_missing_keys_ > TGX_KEY_PROBE_MAX_MISSING_KEYS)
    evaluation_error("max_missing_keys must be 1 .. " + std::to_string((int)TGX_KEY_PROBE_MAX_MISSING_KEYS) + " (" +
                     std::to_string(max_missing_keys_) + ")");
  int ci = -1, pi = -1;
  const Table *child_table = side_of(ctx, child, &ci);
  const Table *parent_table = side_of(ctx, parent, &pi);
  // (a column declared Binary arrives in a string layout; the reference's examples would not print its bytes)
  for (const auto &side : {std::make_pair(child_table, ci), std::make_pair(parent_table, pi)})
    if ((size_t)side.second < side.first->arrow_types.size() && side.first->arrow_types[side.second] == "Binary")
      evaluation_error("column '" + (side.first == child_table && side.second == ci ? child_ : parent_) +
                       "' is a Binary column: foreign keys of that type are not on the GPU path (TGX_CHECK_KEY_PROBE "
                       "takes integer and string keys)");
  // (a side without a batch has no type to object with: it goes the way of the other side)
  const int cs = string_side(*child_table, ci), ps = string_side(*parent_table, pi);
  if (cs >= 0 && ps >= 0 && cs + ps > 0)
    return evaluate_strings(*child_table, ci, *parent_table, pi);
  const int child_type = key_type(*child_table, ci, child_);
  key_type(*parent_table, pi, parent_);

  Checker check(query_failed);
  check(tgx_init(nullptr, &check.err));
  Handles p, c;
  const void *records = nullptr;
  uint64_t n_records = 0;
  export_parent(check, *parent_table, pi, p, &records, &n_records);
  const tgx_key_probe_summary s = probe_child(check, *child_table, ci, records, n_records, c, [&](tgx_plan *plan) {
    const tgx_key_probe_params params = {max_missing_keys_, 0};
    check(tgx_plan_set_key_probe(plan, 0, &params, &check.err));
  });
  uint64_t n = 0;
  check(tgx_key_probe_entries(c.plan, c.state, 0, nullptr, 0, &n, &check.err));
  std::vector<tgx_key_probe_entry> entries((size_t)n + 1);
  check(tgx_key_probe_entries(c.plan, c.state, 0, entries.data(), n, &n, &check.err));

  ForeignKeyCounts counts;
  counts.null_rows = s.null_rows;
  counts.missing_rows = s.missing_rows;
  counts.overflow_rows = s.overflow_rows;
  counts.missing_keys = s.missing_keys;
  for (uint64_t i = 0; i < n; i++) counts.keys.push_back(entries[i].value);
  counts.examples = child_type == TGX_INT64 || child_type == TGX_INT32;  // (:265-291)
  return verdict(counts);
}

// both columns are string layouts: the same two walks over fingerprints
ConstraintResult ForeignKeyConstraint::evaluate_strings(const Table &child_table, int ci, const Table &parent_table,
                                                        int pi) const {
  if (max_value_bytes_ < 1 || max_value_bytes_ > TGX_KEY_PROBE_MAX_VALUE_BYTES)
    evaluation_error("max_value_bytes must be 1 .. " + std::to_string((int)TGX_KEY_PROBE_MAX_VALUE_BYTES) + " (" +
                     std::to_string(max_value_bytes_) + ")");
  Checker check(query_failed);
  check(tgx_init(nullptr, &check.err));
  Handles p, c;
  const void *records = nullptr;
  uint64_t n_records = 0;
  export_parent(check, parent_table, pi, p, &records, &n_records);
  // (the child's plan fingerprints under the parent plan's key)
  const tgx_key_probe_summary s = probe_child(check, child_table, ci, records, n_records, c, [&](tgx_plan *plan) {
    uint8_t key[16];
    check(tgx_plan_get_fingerprint_key(p.plan, key));
    check(tgx_plan_set_fingerprint_key(plan, key, &check.err));
    const tgx_key_probe_strings_params params = {max_missing_keys_, max_value_bytes_};
    check(tgx_plan_set_key_probe_strings(plan, 0, &params, &check.err));
  });
  tgx_key_probe_strings more;
  check(tgx_key_probe_strings_get(c.plan, c.state, 0, &more, &check.err));
  uint64_t n = 0, n_bytes = 0;
  check(tgx_key_probe_entries_bytes(c.plan, c.state, 0, nullptr, 0, &n, nullptr, 0, &n_bytes, &check.err));
  std::vector<tgx_value_count_entry> entries((size_t)n + 1);
  std::vector<uint8_t> bytes((size_t)n_bytes + 1);
  check(tgx_key_probe_entries_bytes(c.plan, c.state, 0, entries.data(), n, &n, bytes.data(), n_bytes, &n_bytes,
                                    &check.err));

  ForeignKeyCounts counts;
  counts.strings = true;
  counts.null_rows = s.null_rows;
  counts.missing_rows = s.missing_rows;
  counts.overflow_rows = s.overflow_rows;
  counts.long_rows = more.long_rows;
  counts.missing_keys = s.missing_keys;
  for (uint64_t i = 0; i < n; i++)
    counts.str_keys.emplace_back((const char *)bytes.data() + entries[i].offset, (size_t)entries[i].length);
  counts.examples = first_type(child_table, ci) == TGX_UTF8;  // (the collector downcasts to StringArray only: :265-291)
  return verdict(counts);
}

Check::Builder &Check::Builder::foreign_key(std::string child_column, std::string parent_column) {
  return constraint(std::make_shared<ForeignKeyConstraint>(std::move(child_column), std::move(parent_column)));
}

}  // namespace term_guard
