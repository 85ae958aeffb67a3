/*
 * tgx_host.h -- C entry points of the host-side mirror of term-guard's ValidationSuite / Check /
 * Constraint surface (term_amd/csrc/host/term_guard.h is the C++ API; this is the bridge other languages
 * bind).  Suites travel as JSON; results come back as the JSON term-guard's own JsonFormatter produces
 * (`serde_json::to_string_pretty(ValidationResult)`, TG/formatters.rs:222-245, TG/core/result.rs:123-136).
 *
 * Suite JSON:
 *   {"name": "...", "table_name": "data",
 *    "column_types": {"c": "Int32", "d": "Timestamp(Nanosecond, None)"},   (optional: Arrow DataTypes as the caller holds
 *                     them; a column without an entry is what its tgx_type says)
 *    "strict_reference_types": true,    (default.  StatisticalConstraint reads its aggregate as Int64Array or Float64Array
 *                     and fails with "Failed to extract statistic value" otherwise (TG/constraints/statistics.rs:277-308):
 *                     MIN / MAX / quantiles of an Int32, Date32, Float32, Timestamp or UInt column, SUM of a UInt column
 *                     are ERRORS there, and here.  false: the value of the widened column answers -- a deviation)
 *    "checks": [{"name": "...", "level": "error|warning|info",
 *     "constraints": [
 *       {"type": "size", "assertion": A},
 *       {"type": "approx_count_distinct", "column": "c", "assertion": A},   (metric: the exact distinct count)
 *       {"type": "completeness", "columns": ["c", ...], "operator": "all"|"any"|{"at_least": n}|{"exactly": n}|
 *                                 {"at_most": n}, "threshold": 1.0},
 *       {"type": "statistic", "column": "c", "statistic": "min|max|mean|sum|standard_deviation|variance|median|
 *                              percentile", "p": 0.5, "assertion": A},
 *       {"type": "uniqueness", "columns": ["c"], "kind": "full_uniqueness|distinctness|unique_value_ratio|primary_key|
 *                               unique_with_nulls", "threshold": 1.0, "assertion": A, "null_handling": "exclude|include|distinct"},
 *       {"type": "format", "column": "c", "format": "regex|email|url|credit_card|phone|postal_code|uuid|ipv4|ipv6|json|
 *                           iso8601_datetime|social_security_number", "pattern": "...", "allow_localhost": false,
 *                           "detect_only": false, "country": "US", "threshold": 1.0,
 *                           "options": {"case_sensitive": true, "trim_before_check": false, "null_is_valid": true}},
 *       {"type": "containment", "column": "c", "allowed_values": ["a", "b"]},
 *       {"type": "length", "column": "c", "kind": "min|max|between|exactly|not_empty", "a": n, "b": m},
 *       {"type": "quantile", "column": "c", "quantile": 0.5, "assertion": A},
 *       {"type": "correlation", "column1": "a", "column2": "b", "assertion": A}]}]}
 *   A = {"kind": "equals|not_equals|greater_than|greater_than_or_equal|less_than|less_than_or_equal|between|
 *                 not_between", "args": [x] or [lo, hi]}                          (TG/constraints/assertion.rs:27-46)
 *
 * Strings returned through `char **` are owned by the library: release them with tgx_host_free.
 */
#ifndef TGX_HOST_H
#define TGX_HOST_H

#include "tgx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ValidationSuite::run (TG/core/suite.rs:399): plans every constraint into one tgx_plan, feeds the table's
 * batches once, applies each constraint's verdict.  `columns` holds n_batches x n_columns views, batch-major;
 * column_names[i] names columns[b * n_columns + i].  The table is registered under the suite's table_name. */
tgx_status tgx_host_run_suite_json(const char *suite_json, const char *const *column_names, size_t n_columns,
                                   const tgx_column *columns, size_t n_batches, char **out_json, tgx_error *err);

/* The aggregates one constraint asks for (its half of the fused plan), as a JSON array. */
tgx_status tgx_host_constraint_plan_json(const char *constraint_json, char **out_json, tgx_error *err);

/* A "temporal_ordering" constraint ({"type": "temporal_ordering", "table": t, "validation": "before_after |
 * business_hours | date_range | max_time_gap | event_sequence", the builder calls' arguments by name, "allow_nulls",
 * "tolerance_seconds"}) + the Arrow DataType names of its columns ({"created_at": "Timestamp(Nanosecond, None)", ..})
 * -> the tgx_temporal_params the suite runner hands to tgx_plan_set_temporal, in the column's ticks:
 * {"column", "column2", "mode", "flags", "delta", "ticks_per_second", "tod_lo", "tod_hi", "lo", "hi"}.  What the GPU path
 * does not take (a unit it cannot know, a time zone other than UTC, MaxTimeGap, EventSequence, an unreadable literal) is
 * TGX_INVALID_ARGUMENT with the constraint's error text: hand such a constraint to the stock path.  Needs no device.
 * A max_time_gap constraint that carries "window_on_device": true plans a TGX_CHECK_TIME_GAP spec instead, and the
 * answer is the tgx_time_gap_params of that spec: {"column", "column2" (the group column or ""), "kind": 13, "max_gap"
 * (max_gap_seconds x the column's ticks per second), "flags"}.  Its timestamp column must be a Timestamp (any zone). */
tgx_status tgx_host_temporal_params_json(const char *constraint_json, const char *arrow_types_json, char **out_json,
                                         tgx_error *err);

/* A "datatype" constraint with a numeric validation ({"type": "datatype", "column": c, "validation": "numeric",
 * "numeric": "non_negative | positive | integer | range", "min", "max"}) -> the tgx_value_rule_params the suite runner
 * hands to tgx_plan_set_value_rule: {"column", "kind": 14, "mode", "flags", "lo_i", "hi_i", "lo_f", "hi_f"}.  A range's
 * bounds are read as DataFusion reads what the reference prints with `{}`: a finite integral bound with |b| <= 2^53 is an
 * Int64 literal, any other finite bound a Float64 literal, and one Float64 literal sets TGX_RULE_BOUNDS_AS_DOUBLE.  What
 * the GPU path does not take (finite, a bound that is not finite or an integer beyond 2^53, every string, temporal and
 * custom validation) is TGX_INVALID_ARGUMENT with the constraint's error text: hand such a constraint to the stock path.
 * Needs no device. */
tgx_status tgx_host_value_rule_params_json(const char *constraint_json, char **out_json, tgx_error *err);

/* What the predicate compiler of Check::satisfies / ComplianceAnalyzer makes of `expression` (host/custom_sql.h has the
 * grammar): {"columns": the columns in order of first appearance, "leaves": [{"kind", "op", "col", "col2", "flags",
 * "lit_offset", "lit_len", "lit_i", "lit_f", "lit_f_bits"}] (the fields of tgx_row_predicate_leaf; lit_f_bits: the
 * double's bits as an unsigned integer, which keeps the sign of -0.0), "program": [[code, arg], ..],
 * "literals_hex": the literal pool}.  An expression outside the subset is TGX_UNSUPPORTED with
 * "the expression is not on the GPU path: <the first thing outside the subset>".  Needs no device. */
tgx_status tgx_host_row_predicate_json(const char *expression, char **out_json, tgx_error *err);
/* The same under options: options_json is NULL or {"string_functions": true|false (default false)} -- the compiler's
 * dialect of that name (LIKE, LENGTH / CHAR_LENGTH / CHARACTER_LENGTH / OCTET_LENGTH, TRIM(c) = '', string order; the
 * leaves TGX_PRED_STR_CMP .. TGX_PRED_STR_BLANK).  Without the option the answer is tgx_host_row_predicate_json's. */
tgx_status tgx_host_row_predicate_json_ex(const char *expression, const char *options_json, char **out_json,
                                          tgx_error *err);

/* One string leaf of TGX_CHECK_ROW_PREDICATE (kind TGX_PRED_STR_CMP .. TGX_PRED_STR_BLANK; op, flags, lit_i as in
 * tgx_row_predicate_leaf; `pattern`: the literal of STR_CMP / the pattern of STR_LIKE) on ONE non-NULL value, through the
 * functions the kernel compiles (kernels/string_leaf.h): *out = 1 for TRUE, 0 for FALSE.  The value is read in aligned
 * words as the kernel reads it, `value`'s own address giving the alignment.  What tgx_plan_set_row_predicate refuses of
 * a leaf (another kind, a comparison outside the kind's ops, a flag, a 0x5C in a pattern) is TGX_INVALID_ARGUMENT.
 * Needs no device. */
tgx_status tgx_host_string_leaf(int32_t kind, int32_t op, uint32_t flags, int64_t lit_i, const uint8_t *pattern,
                                uint32_t pattern_len, const uint8_t *value, uint64_t value_len, int *out);

/* `Constraint::evaluate`'s verdict half on given aggregates: results_json is an array of objects with
 * tgx_result's field names (answering the plan in order; a KLL entry may carry {"quantiles": {"0.5": v}}, a
 * VALUE_COUNTS entry {"total", "non_null", "value_counts": {"entries": {value text: count}, "overflow_rows",
 * "long_rows"}}).
 * A "histogram" constraint is {"type": "histogram", "column": c, "measures": [{"measure": "most_common_ratio |
 * least_common_ratio | bucket_count | entropy | null_ratio | top_n_ratio | value_ratio", "assertion": {..}, "n"
 * (top_n_ratio), "value" (value_ratio)}, ..], "description" (optional), "max_distinct" (default 10000)}: every measure
 * must hold; it plans one TGX_CHECK_VALUE_COUNTS request ({"kind": 15, "value_counts": {"max_distinct",
 * "max_value_bytes"}}).
 * Returns {"status": "success|failure|skipped", "metric": x|null, "message": s|null}.  Needs no device.
 * The constraint JSON may carry "column_type" (the column's Arrow DataType) and "strict_reference_types" as above,
 * and "column_types" (an array: the Arrow DataTypes of a ROW_PREDICATE request's column list, in the list's order). */
tgx_status tgx_host_constraint_verdict_json(const char *constraint_json, const char *results_json, char **out_json,
                                            tgx_error *err);

/* SqlSecurity::validate_identifier (TG/security.rs:103-146) */
tgx_status tgx_host_validate_identifier(const char *identifier, tgx_error *err);

/* Assertion::evaluate + Display (TG/constraints/assertion.rs:48-76) */
tgx_status tgx_host_assertion_json(const char *assertion_json, double value, int32_t *holds, char **description,
                                   tgx_error *err);

/* ---- analyzers (TG/analyzers/traits.rs:65-179, runner.rs:64-202) --------------------------------------------
 * Analysis JSON: {"table_name": "data", "continue_on_error": true, "analyzers": [
 *     {"type": "size"}, {"type": "completeness|distinctness|approx_count_distinct|mean|min|max|sum|standard_deviation", "column": "c"},
 *     {"type": "correlation", "column1": "a", "column2": "b", "method": "pearson|spearman|covariance"},
 *     {"type": "mutual_information", "column1": "a", "column2": "b", "bins": 10, "max_pairs": N (optional),
 *      "max_value_bytes": 256 (optional), "arrow_types": ["Utf8", "Int64"] (optional)},
 *     {"type": "histogram", "column": "c", "num_buckets": 10, "strict_reference_types": true},
 *     {"type": "grouped_completeness", "column": "c", "group_by": ["g"], "max_groups": 10000 | null, "include_overall": true,
 *      "strict_reference_types": true, "group_arrow_type": "Utf8" (optional: the Arrow DataType of the ONE group column
 *      where the table does not say it), "composite_groups_on_device": true (optional, an opt-in: 2 .. 8 "group_by"
 *      columns are one TGX_CHECK_GROUP_COUNTS walk on the tuple of the columns), "group_arrow_types": ["Utf8", "Int64"]
 *      (optional, with several group columns: their Arrow DataTypes, parallel to "group_by"; "" = the table says)},
 *     {"type": "value_entropy", "column": "c", "max_unique_values": 10000, "arrow_type": "Int64" (optional)},
 *     {"type": "data_type", "column": "c", "arrow_type": "Int32" (optional)}]}
 * "value_entropy" is the tag of EntropyAnalyzer (TG/analyzers/advanced/entropy.rs; name() "entropy", metric key
 * "entropy.<column>"): the tag "entropy" is not taken, it stays an unknown analyzer type.
 * AnalysisRunner::run: every analyzer's aggregates planned into ONE tgx_plan, one pass over the table; the
 * mutual_information and histogram analyzers (bin edges depend on the whole table) add a second pass for their counts,
 * shared by all such analyzers of the run.  "max_pairs" is mutual_information's opt-in for string columns: with it, a
 * pair with at least one Utf8 / LargeUtf8 / Utf8View / Dictionary column plans ONE TGX_CHECK_PAIR_COUNTS request
 * (string x string: one pass; a mixed pair: the numeric side's range, then the count, in the shared second pass);
 * without it the analyzer does what it always did (JOINT_BINS; a string column is its TGX_UNSUPPORTED error).  A pair
 * beyond the bounds, a column declared binary and a string value that may parse as a number are the
 * analyzer's own errors.  Returns
 *   {"metrics": {metric_key: {"type": "Double|Long|Boolean|Map|Histogram", "value": ..}},   (MetricValue's serde form, types.rs:11-35)
 *    "states":  {metric_key: {..the AnalyzerState's serde fields..}},
 *    "errors":  [{"analyzer_name": "..", "error": ".."}]}                        (context.rs:118-123)
 * With continue_on_error false the first failing analyzer makes the call fail with "Analyzer {name} failed". */
tgx_status tgx_host_run_analysis_json(const char *analysis_json, const char *const *column_names, size_t n_columns,
                                      const tgx_column *columns, size_t n_batches, char **out_json, tgx_error *err);

/* AnalyzerState::merge of the analyzer's state type over a JSON array of states; needs no device. */
tgx_status tgx_host_merge_states_json(const char *analyzer_json, const char *states_json, char **out_state_json,
                                      tgx_error *err);

/* Analyzer::compute_metric_from_state; needs no device.  An AnalyzerError (e.g. NoData) is returned as
 * TGX_INVALID_ARGUMENT with the reference's Display text in err->msg. */
tgx_status tgx_host_metric_from_state_json(const char *analyzer_json, const char *state_json, char **out_metric_json,
                                           tgx_error *err);

/* What an analyzer plans for columns of the given tgx_types (column_types_json: an array of tgx_type numbers parallel to
 * the analyzer's columns; 0 = unknown): {"requests": [{"kind", "column", "column2", "pair_counts": {"max_pairs",
 * "max_value_bytes", "x_mode", "y_mode"} (TGX_CHECK_PAIR_COUNTS only), "group_counts": {"max_groups", "max_value_bytes"}
 * (TGX_CHECK_GROUP_COUNTS only; a request that groups by several columns -- a "grouped_completeness" analyzer with
 * "composite_groups_on_device": true and 2 .. 8 "group_by" columns -- has "column2": "" and "columns": [..]), "value_rule": {"mode", "flags", "lo_i", "hi_i", "lo_f", "hi_f"} (TGX_CHECK_VALUE_RULE
 * only)}]}.  Needs no device. */
tgx_status tgx_host_analyzer_plan_json(const char *analyzer_json, const char *column_types_json, char **out_json,
                                       tgx_error *err);

/* The state a mutual_information analyzer builds from given pair counts; needs no device.  pair_counts_json:
 * {"summary": {tgx_pair_counts_summary's fields; absent ones are 0}, "entries": [[x, y, count], ..]} in the library's
 * order, a cell being a string (a value), an array of byte values (a value that is no UTF-8) or an integer (a bin).  An
 * AnalyzerError is returned as TGX_INVALID_ARGUMENT with its text in err->msg. */
tgx_status tgx_host_pair_counts_state_json(const char *analyzer_json, const char *pair_counts_json, char **out_state_json,
                                           tgx_error *err);

/* The state a grouped_completeness analyzer builds from given group counts; needs no device.  group_counts_json:
 * {"summary": {tgx_group_counts_summary's fields; absent ones are 0}, "entries": [[key, total, non_null], ..]} in the
 * library's order, a key being a string, an array of byte values (a key that is no UTF-8) or an integer.  An
 * AnalyzerError is returned as TGX_INVALID_ARGUMENT with its text in err->msg. */
tgx_status tgx_host_group_counts_state_json(const char *analyzer_json, const char *group_counts_json,
                                            char **out_state_json, tgx_error *err);

/* The class (TGX_TYPE_CLASS_*, include/tgx.h) the lexer of TGX_CHECK_TYPE_CLASSES gives the value bytes[0 .. len): the
 * same function the kernels compile (kernels/typeclass_lex.h).  `bytes` may be NULL when len is 0.  Needs no device. */
int32_t tgx_host_type_class(const uint8_t *bytes, uint64_t len);

/* The state a "data_type" analyzer ({"type": "data_type", "column": "c", "arrow_type": "Int32" (optional: the column's
 * Arrow DataType where the table does not say it)}; TG/analyzers/advanced/data_type.rs) builds from given counts; needs
 * no device.  counts_json is either the nine counters of tgx_type_classes_counts by their field names (a string column;
 * absent ones are 0), or {"results": [{"total", "non_null", "matches"}, ..]}: the tgx_results that answer the requests
 * the analyzer plans for an integer column (two VALUE_RULE requests) or a float column (one COUNT).  Returns
 * {"type_counts": {label: n}, "total_count": n}; undecided_rows > 0 is TGX_INVALID_ARGUMENT with the analyzer's error. */
tgx_status tgx_host_data_type_state_json(const char *analyzer_json, const char *counts_json, char **out_state_json,
                                         tgx_error *err);

/* ValidationSuite::run over SEVERAL registered tables: what tgx_host_run_suite_json does, with every table of `tables`
 * registered under its own name (the suite's table among them, under the suite's table_name; a suite whose table is not
 * registered answers as the reference does for a missing table).  A "cross_table_sum" constraint
 *   {"type": "cross_table_sum", "left_column": "orders.total", "right_column": "payments.amount", "group_by": ["g"],
 *    "tolerance": 0.0, "max_violations_reported": 100, "max_groups": 65536}       (TG/constraints/cross_table_sum.rs)
 * (optional: "composite_groups_on_device": true, an opt-in -- 2 .. 8 "group_by" columns are one GROUP_SUMS walk a side on
 * the tuple of the columns; without it several columns are the constraint's error)
 * is evaluated beside the suite's fused plan, against the registered tables: each side is walked once, as a
 * TGX_CHECK_GROUP_SUMS spec (grouped) or a TGX_CHECK_NUMERIC_STATS spec (ungrouped); the outer join of the sides'
 * groups runs on the host.  The suite JSON may carry "table_column_types": {table: {column: DataType}}, the Arrow types the
 * caller holds for columns whose layout does not say them: a column declared "Binary" arrives in a string layout and is
 * refused as a foreign key.  The table registered under the suite's "table_name" takes the suite's "column_types". */
typedef struct tgx_host_table {
  const char *name;
  const char *const *column_names; /* n_columns names */
  size_t n_columns;
  const tgx_column *columns;       /* n_batches x n_columns views, batch-major */
  size_t n_batches;
} tgx_host_table;
tgx_status tgx_host_run_suite_tables_json(const char *suite_json, const tgx_host_table *tables, size_t n_tables,
                                          char **out_json, tgx_error *err);

/* The join and the verdict of a "cross_table_sum" constraint on given sums; needs no device.  sums_json:
 * {"left": S, "right": S} with S = a number (the ungrouped form: COALESCE(SUM(col), 0.0) of the side) or
 * {"groups": [[key, sum], ..] ascending by key (a key a string or an integer), "null_group": sum or null,
 *  "overflow_rows": n, "long_rows": n}; NaN / Infinity / -Infinity are read as Python's json writes them.  Returns
 * {"status", "metric", "message", "total_groups", "violating_groups", "total_left_sum", "total_right_sum",
 *  "max_difference", "config": {the constraint as the host layer read it}}; a number that is not finite comes back as
 * the string "NaN" / "inf" / "-inf".  A side beyond its bounds, sides of different key kinds and an unqualified column
 * are TGX_INVALID_ARGUMENT with the constraint's error text. */
tgx_status tgx_host_cross_table_sum_json(const char *constraint_json, const char *sums_json, char **out_json,
                                         tgx_error *err);

/* The verdict of a "foreign_key" constraint
 *   {"type": "foreign_key", "child_column": "orders.customer_id", "parent_column": "customers.id", "allow_nulls": false,
 *    "use_left_join": true, "max_violations_reported": 100, "max_missing_keys": 10000}   (TG/constraints/foreign_key.rs)
 * on given counts; needs no device.  (Within a suite run over several tables the constraint is evaluated beside the fused
 * plan: the parent's column under a TGX_CHECK_DISTINCT spec, its key set handed to a TGX_CHECK_KEY_PROBE spec over the
 * child's column.)  counts_json: {"null_rows": n, "missing_rows": n, "overflow_rows": n, "missing_keys": n,
 * "entries": [[key, count], ..] ascending by key, "examples": true} as tgx_key_probe_get / tgx_key_probe_entries give
 * them; "examples": false stands for a child column of a type the reference's example collector does not read.
 * String keys (both columns string layouts; the constraint's own "max_value_bytes": 1 .. 256, named in the config only
 * when it was given): the entries' keys are JSON strings, ascending bytewise, and "long_rows": n counts the missing rows
 * whose value was too long to keep (missing_rows == sum of the counts + overflow_rows + long_rows), as
 * tgx_key_probe_strings_get / tgx_key_probe_entries_bytes give them.
 * Returns {"status", "metric", "message", "config": {the constraint as the host layer read it}}.  An unqualified column
 * and counts that contradict each other are TGX_INVALID_ARGUMENT. */
tgx_status tgx_host_foreign_key_json(const char *constraint_json, const char *counts_json, char **out_json,
                                     tgx_error *err);

/* The verdict of a "join_coverage" constraint
 *   {"type": "join_coverage", "left_table": "orders", "right_table": "customers", "join_keys": [["customer_id", "id"]],
 *    "expected_match_rate": 1.0, "coverage_type": "left" | "right" | "bidirectional", "distinct_only": false,
 *    "max_examples_reported": 100, "max_missing_keys": 10000}                       (TG/constraints/join_coverage.rs)
 * on given counts; needs no device.  (Within a suite run over several tables the far side's column is gathered as
 * {key, 1} records and handed to a COUNTED TGX_CHECK_KEY_PROBE spec over the near side's column; string keys: as
 * fingerprint records, to a counted strings spec.)  "max_value_bytes": n (1 .. 256, string keys only, optional) is the
 * bytes a missing key may have to be kept.  "composite_keys_on_device": true (optional, an opt-in) lets "join_keys" hold
 * 2 .. 8 pairs: the join then runs under TGX_CHECK_KEY_PROBE's tuple modes, each pair two integer or two string
 * columns; a row with a NULL in any key column joins nothing.  Absent or false, more than one key pair is the error it
 * was.  "examples" then takes two more optional counts, "null_keys" (the left side's distinct tuples with a NULL
 * component: each a distinct value of the examples query) and "null_overflow_rows" (rows of such tuples that found no
 * slot: the number reads "at least"); where "null_keys" is absent the NULL rows count as ONE value, as for a single key.
 * counts_json: {"left": {"pairs": n, "join_rows": n}, "right": {..}, "left_distinct": n, "examples": {"missing_keys": n,
 * "null_rows": n, "overflow_rows": n, "long_rows": n}} ("long_rows": string keys, optional) -- "left": the left column probed against the right side's counted set as
 * tgx_key_probe_pairs_get gives it, "right": the other way round, "left_distinct": COUNT(DISTINCT left column),
 * "examples": the left column's missing keys, NULL rows and overflow rows against the right side's set.  A side the
 * coverage type reads must be there, and "examples" when the check fails with max_examples_reported > 0.
 * Returns {"status", "metric", "message", "config": {the constraint as the host layer read it}}.  A constraint without
 * join keys, with more than one key pair without the opt-in or more than 8 with it, RightCoverage with distinct_only and a join without rows are
 * TGX_INVALID_ARGUMENT with the constraint's error text. */
tgx_status tgx_host_join_coverage_json(const char *constraint_json, const char *counts_json, char **out_json,
                                       tgx_error *err);

void tgx_host_free(char *s);

#ifdef __cplusplus
}
#endif
#endif /* TGX_HOST_H */
