// host_abi.cpp -- the C bridge of include/tgx_host.h over host/term_guard.{h,cpp}.
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../../include/tgx_host.h"
#include "json.h"
#include "analyzers.h"
#include "custom_sql.h"
#include "datatype.h"
#include "../kernels/string_leaf.h"
#include "../kernels/typeclass_lex.h"
#include "value_counts.h"
#include "temporal.h"
#include "term_guard.h"

using namespace term_guard;

namespace term_guard {
void add_constraint_from_json(Check::Builder &b, const json::Value &c);
}

static tgx_status hfail(tgx_error *err, tgx_status code, const std::string &msg) {
  if (err) {
    err->code = code;
    snprintf(err->msg, sizeof(err->msg), "%s", msg.c_str());
  }
  return code;
}

static char *dup_string(const std::string &s) {
  char *p = (char *)malloc(s.size() + 1);
  if (p) memcpy(p, s.c_str(), s.size() + 1);
  return p;
}

extern "C" void tgx_host_free(char *s) { free(s); }

extern "C" tgx_status tgx_host_run_suite_json(const char *suite_json, const char *const *column_names,
                                              size_t n_columns, const tgx_column *columns, size_t n_batches,
                                              char **out_json, tgx_error *err) {
  if (!suite_json || !out_json || (n_columns && (!column_names || (n_batches && !columns))))
    return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    ValidationSuite suite = suite_from_json(suite_json);
    Table t;
    for (size_t i = 0; i < n_columns; i++) t.column_names.push_back(column_names[i]);
    for (size_t b = 0; b < n_batches; b++) {
      Batch batch;
      batch.columns.assign(columns + b * n_columns, columns + (b + 1) * n_columns);
      t.batches.push_back(std::move(batch));
    }
    Context ctx;
    if (n_columns > 0) ctx.register_table(suite.table_name(), std::move(t));
    ValidationResult r = suite.run(ctx);
    *out_json = dup_string(r.to_json());
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

static std::shared_ptr<Constraint> constraint_from_json_text(const char *text) {
  json::Value v;
  std::string perr;
  if (!json::parse(text, &v, &perr)) throw TermError{TermError::Internal, "constraint JSON: " + perr};
  Check::Builder b = Check::builder("c");
  add_constraint_from_json(b, v);
  Check c = b.build();
  return c.constraints().at(0);
}

// a double as JSON: 17 significant digits round-trip; a NaN or an infinity (a BETWEEN bound may be one at the C ABI,
// never from this layer) as a string
static std::string json_f64(double v) {
  if (std::isnan(v)) return "\"NaN\"";
  if (std::isinf(v)) return v > 0 ? "\"inf\"" : "\"-inf\"";
  char buf[64];
  snprintf(buf, sizeof(buf), "%.17g", v);
  return buf;
}

static std::string value_rule_json(const tgx_value_rule_params &p) {
  return "{\"mode\": " + std::to_string(p.mode) + ", \"flags\": " + std::to_string(p.flags) + ", \"lo_i\": " +
         std::to_string(p.lo_i) + ", \"hi_i\": " + std::to_string(p.hi_i) + ", \"lo_f\": " + json_f64(p.lo_f) +
         ", \"hi_f\": " + json_f64(p.hi_f) + "}";
}

extern "C" tgx_status tgx_host_constraint_plan_json(const char *constraint_json, char **out_json, tgx_error *err) {
  if (!constraint_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto c = constraint_from_json_text(constraint_json);
    std::string o = "{\"name\": " + json::quote(c->name()) + ", \"requests\": [";
    auto reqs = c->plan();
    for (size_t i = 0; i < reqs.size(); i++) {
      const SpecRequest &r = reqs[i];
      if (i) o += ", ";
      o += "{\"kind\": " + std::to_string(r.kind) + ", \"column\": " + json::quote(r.column) + ", \"column2\": " +
           json::quote(r.column2) + ", \"flags\": " + std::to_string(r.flags) + ", \"pattern\": " + json::quote(r.pattern) +
           ", \"kll_k\": " + std::to_string(r.kll_k);
      if (r.temporal) {
        const TemporalRequest &t = *r.temporal;
        auto text = [](const std::optional<std::string> &s) { return s ? json::quote(*s) : std::string("null"); };
        o += std::string(", \"temporal\": {\"mode\": ") + std::to_string(t.mode) + ", \"allow_equal\": " +
             (t.allow_equal ? "true" : "false") + ", \"allow_nulls\": " + (t.allow_nulls ? "true" : "false") +
             ", \"weekdays_only\": " + (t.weekdays_only ? "true" : "false") + ", \"tolerance_seconds\": " +
             std::to_string(t.tolerance_seconds) + ", \"start_time\": " + json::quote(t.start_time) +
             ", \"end_time\": " + json::quote(t.end_time) + ", \"min_date\": " + text(t.min_date) +
             ", \"max_date\": " + text(t.max_date) +
             (t.mode == kTemporalTimeGapMode ? ", \"max_gap_seconds\": " + std::to_string(t.max_gap_seconds) : std::string()) +
             "}";
      }
      if (r.value_rule) o += ", \"value_rule\": " + value_rule_json(*r.value_rule);
      if (r.value_counts)
        o += ", \"value_counts\": {\"max_distinct\": " + std::to_string(r.value_counts->max_distinct) +
             ", \"max_value_bytes\": " + std::to_string(r.value_counts->max_value_bytes) + "}";
      if (r.row_predicate) {
        RowPredicate p;
        p.columns = r.columns;
        p.params = *r.row_predicate;
        o += ", \"row_predicate\": " + row_predicate_json(p);
      }
      o += "}";
    }
    o += "]}";
    *out_json = dup_string(o);
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

namespace {
struct FakeQuantiles {
  std::vector<std::vector<std::pair<double, double>>> per_request;
  std::vector<std::optional<ValueCounts>> value_counts;  // per request: what a VALUE_COUNTS entry of results_json carries
};
void fake_value_counts(const void *ctx, size_t idx, ValueCounts *out) {
  const FakeQuantiles *f = (const FakeQuantiles *)ctx;
  if (!f->value_counts.at(idx)) throw TermError{TermError::Internal, "results_json has no value_counts for this request"};
  *out = *f->value_counts[idx];
}
double fake_quantile(const void *ctx, size_t idx, double phi) {
  const FakeQuantiles *f = (const FakeQuantiles *)ctx;
  for (auto &kv : f->per_request.at(idx))
    if (kv.first == phi) return kv.second;
  throw TermError{TermError::Internal, "results_json has no quantile for phi=" + rust_f64(phi)};
}
}  // namespace

extern "C" tgx_status tgx_host_constraint_verdict_json(const char *constraint_json, const char *results_json,
                                                       char **out_json, tgx_error *err) {
  if (!constraint_json || !results_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto c = constraint_from_json_text(constraint_json);
    json::Value rv;
    std::string perr;
    if (!json::parse(results_json, &rv, &perr) || !rv.is(json::Value::Array))
      return hfail(err, TGX_INVALID_ARGUMENT, "results JSON must be an array: " + perr);
    std::vector<tgx_result> results(rv.arr.size());
    FakeQuantiles fq;
    fq.per_request.resize(rv.arr.size());
    fq.value_counts.resize(rv.arr.size());
    for (size_t i = 0; i < rv.arr.size(); i++) {
      const json::Value &o = rv.arr[i];
      tgx_result &r = results[i];
      memset(&r, 0, sizeof(r));
      r.is_float = (int32_t)o.get_i64("is_float");
      r.total = o.get_i64("total");
      r.non_null = o.get_i64("non_null");
      r.has_value = (int32_t)o.get_i64("has_value");
      r.has_variance = (int32_t)o.get_i64("has_variance");
      r.min_i = o.get_i64("min_i");
      r.max_i = o.get_i64("max_i");
      r.min_f = o.get_num("min_f");
      r.max_f = o.get_num("max_f");
      r.sum_i = o.get_i64("sum_i");
      r.sum_f = o.get_num("sum_f");
      r.mean = o.get_num("mean");
      r.var_samp = o.get_num("var_samp");
      r.stddev_samp = o.get_num("stddev_samp");
      r.distinct = o.get_i64("distinct");
      r.groups_once = o.get_i64("groups_once");
      r.matches = o.get_i64("matches");
      r.sum_x = o.get_num("sum_x");
      r.sum_y = o.get_num("sum_y");
      r.sum_x2 = o.get_num("sum_x2");
      r.sum_y2 = o.get_num("sum_y2");
      r.sum_xy = o.get_num("sum_xy");
      if (o.get("co_m2_x")) {
        r.co_mean_x = o.get_num("co_mean_x");
        r.co_mean_y = o.get_num("co_mean_y");
        r.co_m2_x = o.get_num("co_m2_x");
        r.co_m2_y = o.get_num("co_m2_y");
        r.co_c_xy = o.get_num("co_c_xy");
      } else if (r.non_null > 0) {  // results that carry the raw sums only: centred from them
        const double n = (double)r.non_null;
        r.co_mean_x = r.sum_x / n;
        r.co_mean_y = r.sum_y / n;
        r.co_m2_x = std::max(0.0, r.sum_x2 - r.sum_x * r.sum_x / n);
        r.co_m2_y = std::max(0.0, r.sum_y2 - r.sum_y * r.sum_y / n);
        r.co_c_xy = r.sum_xy - r.sum_x * r.sum_y / n;
      }
      r.kll_n = o.get_u64("kll_n");
      if (const json::Value *q = o.get("quantiles"))
        for (auto &kv : q->obj) fq.per_request[i].emplace_back(atof(kv.first.c_str()), kv.second.num);
      if (const json::Value *vc = o.get("value_counts")) {  // {"entries": {text: count}, "overflow_rows", "long_rows"}
        ValueCounts v;
        v.summary.seen = (uint64_t)r.total;
        v.summary.non_null = (uint64_t)r.non_null;
        v.summary.overflow_rows = vc->get_u64("overflow_rows");
        v.summary.long_rows = vc->get_u64("long_rows");
        if (const json::Value *e = vc->get("entries"))
          for (auto &kv : e->obj) {
            v.entries.emplace_back(kv.first, kv.second.as_u64());
            v.summary.counted += kv.second.as_u64();
          }
        v.summary.distinct = vc->get("distinct") ? vc->get_u64("distinct") : v.entries.size();
        fq.value_counts[i] = std::move(v);
      }
    }
    const size_t want = c->plan().size();
    if (results.size() != want)
      return hfail(err, TGX_INVALID_ARGUMENT,
                   "constraint plans " + std::to_string(want) + " aggregates, got " + std::to_string(results.size()));
    Constraint::Inputs in;
    for (auto &r : results) in.results.push_back(&r);
    in.ctx = &fq;
    in.quantile = fake_quantile;
    in.value_counts = fake_value_counts;
    {  // the reference's result-type rule (term_guard.h reference_extracts): "column_type" = the column's Arrow DataType
      json::Value cv;
      std::string cerr;
      if (json::parse(constraint_json, &cv, &cerr) && cv.is(json::Value::Object)) {
        if (cv.get("column_type")) in.arrow_types.assign(results.size(), cv.get_str("column_type"));
        if (const json::Value *ct = cv.get("column_types"))  // ... of a request's column list, in the list's order
          if (ct->is(json::Value::Array)) {
            std::vector<std::string> types;
            for (const json::Value &e : ct->arr) types.push_back(e.is(json::Value::String) ? e.str : std::string());
            in.list_arrow_types.assign(results.size(), types);
          }
        in.strict_reference_types = cv.get_bool("strict_reference_types", true);
      }
    }
    ConstraintResult cr = c->evaluate(in);
    const char *st = cr.status == ConstraintStatus::Success ? "success" : cr.status == ConstraintStatus::Failure ? "failure" : "skipped";
    std::string o = std::string("{\"status\": \"") + st + "\", \"metric\": ";
    if (cr.metric && !std::isnan(*cr.metric) && !std::isinf(*cr.metric)) {
      char buf[64];
      snprintf(buf, sizeof(buf), "%.17g", *cr.metric);
      o += buf;
    } else {
      o += "null";
    }
    o += ", \"message\": " + (cr.message ? json::quote(*cr.message) : std::string("null")) + ", \"name\": " +
         json::quote(c->name()) + "}";
    *out_json = dup_string(o);
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_temporal_params_json(const char *constraint_json, const char *arrow_types_json,
                                                    char **out_json, tgx_error *err) {
  if (!constraint_json || !arrow_types_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto c = constraint_from_json_text(constraint_json);
    json::Value types;
    std::string perr;
    if (!json::parse(arrow_types_json, &types, &perr) || !types.is(json::Value::Object))
      return hfail(err, TGX_INVALID_ARGUMENT, "arrow types JSON must be an object {column: DataType}: " + perr);
    const std::vector<SpecRequest> reqs = c->plan();
    if (reqs.size() != 1 || !reqs[0].temporal)
      return hfail(err, TGX_INVALID_ARGUMENT, "not a temporal_ordering constraint");
    const SpecRequest &r = reqs[0];
    if (r.kind == TGX_CHECK_TIME_GAP) {  // MaxTimeGap with window_on_device: the tgx_time_gap_params of its spec
      const tgx_time_gap_params g = time_gap_params(*r.temporal, types.get_str(r.column), types.get_str(r.column2));
      *out_json = dup_string("{\"column\": " + json::quote(r.column) + ", \"column2\": " + json::quote(r.column2) +
                             ", \"kind\": " + std::to_string(r.kind) + ", \"max_gap\": " + std::to_string(g.max_gap) +
                             ", \"flags\": " + std::to_string(g.flags) + "}");
      return TGX_OK;
    }
    const tgx_temporal_params p = temporal_params(*r.temporal, types.get_str(r.column), types.get_str(r.column2));
    auto n = [](int64_t v) { return std::to_string(v); };
    *out_json = dup_string("{\"column\": " + json::quote(r.column) + ", \"column2\": " + json::quote(r.column2) +
                           ", \"mode\": " + n(p.mode) + ", \"flags\": " + n(p.flags) + ", \"delta\": " + n(p.delta) +
                           ", \"ticks_per_second\": " + n(p.ticks_per_second) + ", \"tod_lo\": " + n(p.tod_lo) +
                           ", \"tod_hi\": " + n(p.tod_hi) + ", \"lo\": " + n(p.lo) + ", \"hi\": " + n(p.hi) + "}");
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_value_rule_params_json(const char *constraint_json, char **out_json, tgx_error *err) {
  if (!constraint_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto c = constraint_from_json_text(constraint_json);
    const std::vector<SpecRequest> reqs = c->plan();
    if (reqs.size() != 1 || !reqs[0].value_rule)
      return hfail(err, TGX_INVALID_ARGUMENT, "not a numeric datatype constraint");
    const std::string rule = value_rule_json(*reqs[0].value_rule);
    *out_json = dup_string("{\"column\": " + json::quote(reqs[0].column) + ", \"kind\": " + std::to_string(reqs[0].kind) +
                           ", " + rule.substr(1));
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_row_predicate_json(const char *expression, char **out_json, tgx_error *err) {
  if (!expression || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    *out_json = dup_string(row_predicate_json(compile_row_predicate(expression)));
    return TGX_OK;
  } catch (const PredicateRefusal &r) {
    return hfail(err, TGX_UNSUPPORTED, "the expression is not on the GPU path: " + r.what);
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_row_predicate_json_ex(const char *expression, const char *options_json, char **out_json,
                                                     tgx_error *err) {
  if (!expression || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    PredicateDialect dialect;
    if (options_json) {
      json::Value o;
      std::string perr;
      if (!json::parse(options_json, &o, &perr)) return hfail(err, TGX_INVALID_ARGUMENT, "options JSON: " + perr);
      if (!o.is(json::Value::Object)) return hfail(err, TGX_INVALID_ARGUMENT, "options must be a JSON object");
      dialect.string_functions = o.get("string_functions") && o.get_bool("string_functions");
    }
    *out_json = dup_string(row_predicate_json(compile_row_predicate(expression, dialect)));
    return TGX_OK;
  } catch (const PredicateRefusal &r) {
    return hfail(err, TGX_UNSUPPORTED, "the expression is not on the GPU path: " + r.what);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_string_leaf(int32_t kind, int32_t op, uint32_t flags, int64_t lit_i, const uint8_t *pattern,
                                           uint32_t pattern_len, const uint8_t *value, uint64_t value_len, int *out) {
  if (!out || (!pattern && pattern_len) || (!value && value_len)) return TGX_INVALID_ARGUMENT;
  // (the value's words as the kernel would see them were its first byte where `value` points)
  tgx::SlHostFetch f{value, value_len, (uint32_t)((uintptr_t)value & 3)};
  const bool ordered = op >= TGX_PRED_LT && op <= TGX_PRED_GE;
  switch (kind) {
    case TGX_PRED_STR_CMP:
      if (!ordered || flags) return TGX_INVALID_ARGUMENT;
      *out = tgx::sl::order(f, value_len, (uint32_t)op, pattern, pattern_len);
      return TGX_OK;
    case TGX_PRED_STR_LENGTH:
      if (!(ordered || op == TGX_PRED_EQ) || (flags & ~(uint32_t)TGX_PRED_LENGTH_IN_BYTES)) return TGX_INVALID_ARGUMENT;
      *out = tgx::sl::length(f, value_len, (uint32_t)op, lit_i, (flags & TGX_PRED_LENGTH_IN_BYTES) != 0);
      return TGX_OK;
    case TGX_PRED_STR_LIKE:
      if (flags || (pattern_len && memchr(pattern, 0x5C, pattern_len))) return TGX_INVALID_ARGUMENT;
      *out = tgx::sl::like(f, value_len, pattern, pattern_len, tgx::sl::like_min_len(pattern, pattern_len));
      return TGX_OK;
    case TGX_PRED_STR_BLANK:
      if (flags) return TGX_INVALID_ARGUMENT;
      *out = tgx::sl::blank(f, value_len);
      return TGX_OK;
    default:
      return TGX_INVALID_ARGUMENT;
  }
}

extern "C" tgx_status tgx_host_validate_identifier(const char *identifier, tgx_error *err) try {
  if (!identifier) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  auto e = validate_identifier(identifier);
  if (e) return hfail(err, TGX_INVALID_ARGUMENT, e->display());
  return TGX_OK;
} catch (...) {
  return hfail(err, TGX_INTERNAL, "C++ exception while validating the identifier");
}

namespace term_guard {
ValidationSuite suite_from_json(const std::string &text);
}

extern "C" tgx_status tgx_host_assertion_json(const char *assertion_json, double value, int32_t *holds,
                                              char **description, tgx_error *err) {
  if (!assertion_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  try {
    // reuse the constraint parser: wrap the assertion into a size constraint
    std::string wrapped = std::string("{\"type\": \"size\", \"assertion\": ") + assertion_json + "}";
    auto c = constraint_from_json_text(wrapped.c_str());
    tgx_result r;
    memset(&r, 0, sizeof(r));
    // evaluate through Size: metric == total; only exact for integral values, so parse the assertion directly too
    json::Value v;
    std::string perr;
    json::parse(assertion_json, &v, &perr);
    Assertion a = Assertion::equals(0);
    const std::string k = v.get_str("kind");
    const json::Value *args = v.get("args");
    auto arg = [&](size_t i) { return args && args->arr.size() > i ? args->arr[i].num : 0.0; };
    if (k == "equals") a = Assertion::equals(arg(0));
    else if (k == "not_equals") a = Assertion::not_equals(arg(0));
    else if (k == "greater_than") a = Assertion::greater_than(arg(0));
    else if (k == "greater_than_or_equal") a = Assertion::greater_than_or_equal(arg(0));
    else if (k == "less_than") a = Assertion::less_than(arg(0));
    else if (k == "less_than_or_equal") a = Assertion::less_than_or_equal(arg(0));
    else if (k == "between") a = Assertion::between(arg(0), arg(1));
    else if (k == "not_between") a = Assertion::not_between(arg(0), arg(1));
    if (holds) *holds = a.evaluate(value) ? 1 : 0;
    if (description) *description = dup_string(a.description());
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

// ---- analyzers
static json::Value parse_json_text(const char *text, const char *what) {
  json::Value v;
  std::string perr;
  if (!json::parse(text, &v, &perr)) throw TermError{TermError::Internal, std::string(what) + " JSON: " + perr};
  return v;
}

extern "C" tgx_status tgx_host_run_analysis_json(const char *analysis_json, const char *const *column_names,
                                                 size_t n_columns, const tgx_column *columns, size_t n_batches,
                                                 char **out_json, tgx_error *err) {
  if (!analysis_json || !out_json || (n_columns && (!column_names || (n_batches && !columns))))
    return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    json::Value v = parse_json_text(analysis_json, "analysis");
    AnalysisRunner runner;
    runner.table_name(v.get_str("table_name", "data")).continue_on_error(v.get_bool("continue_on_error", true));
    if (const json::Value *as = v.get("analyzers"))
      for (const json::Value &a : as->arr) runner.add(analyzer_from_json(a));
    Table t;
    for (size_t i = 0; i < n_columns; i++) t.column_names.push_back(column_names[i]);
    for (size_t b = 0; b < n_batches; b++) {
      Batch batch;
      batch.columns.assign(columns + b * n_columns, columns + (b + 1) * n_columns);
      t.batches.push_back(std::move(batch));
    }
    Context ctx;
    if (n_columns > 0) ctx.register_table(v.get_str("table_name", "data"), std::move(t));
    *out_json = dup_string(runner.run(ctx).to_json());
    return TGX_OK;
  } catch (const AnalyzerError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.text);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_merge_states_json(const char *analyzer_json, const char *states_json,
                                                 char **out_state_json, tgx_error *err) {
  if (!analyzer_json || !states_json || !out_state_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_state_json = nullptr;
  try {
    auto a = analyzer_from_json(parse_json_text(analyzer_json, "analyzer"));
    json::Value states = parse_json_text(states_json, "states");
    if (states.type != json::Value::Array) return hfail(err, TGX_INVALID_ARGUMENT, "states must be a JSON array");
    *out_state_json = dup_string(json_dump(a->merge_states(states.arr)));
    return TGX_OK;
  } catch (const AnalyzerError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.text);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_metric_from_state_json(const char *analyzer_json, const char *state_json,
                                                      char **out_metric_json, tgx_error *err) {
  if (!analyzer_json || !state_json || !out_metric_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_metric_json = nullptr;
  try {
    auto a = analyzer_from_json(parse_json_text(analyzer_json, "analyzer"));
    *out_metric_json = dup_string(a->metric_from_state(parse_json_text(state_json, "state")).to_json());
    return TGX_OK;
  } catch (const AnalyzerError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.text);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_analyzer_plan_json(const char *analyzer_json, const char *column_types_json,
                                                  char **out_json, tgx_error *err) {
  if (!analyzer_json || !column_types_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto a = analyzer_from_json(parse_json_text(analyzer_json, "analyzer"));
    json::Value types = parse_json_text(column_types_json, "column types");
    if (types.type != json::Value::Array) return hfail(err, TGX_INVALID_ARGUMENT, "column types must be a JSON array");
    std::vector<int> column_types;
    for (const json::Value &t : types.arr) column_types.push_back((int)t.as_u64());
    std::string o = "{\"requests\": [";
    const std::vector<SpecRequest> reqs = a->plan_for(column_types, std::vector<std::string>());
    for (size_t i = 0; i < reqs.size(); i++) {
      const SpecRequest &r = reqs[i];
      o += std::string(i ? ", " : "") + "{\"kind\": " + std::to_string(r.kind) + ", \"column\": " + json::quote(r.column) +
           ", \"column2\": " + json::quote(r.column2);
      if (r.pair_counts)
        o += ", \"pair_counts\": {\"max_pairs\": " + std::to_string(r.pair_counts->max_pairs) + ", \"max_value_bytes\": " +
             std::to_string(r.pair_counts->max_value_bytes) + ", \"x_mode\": " + std::to_string(r.pair_counts->x.mode) +
             ", \"y_mode\": " + std::to_string(r.pair_counts->y.mode) + "}";
      if (r.kind == TGX_CHECK_GROUP_COUNTS && !r.columns.empty()) {  // (a tuple of group columns: the spec's list)
        o += ", \"columns\": [";
        for (size_t c = 0; c < r.columns.size(); c++) o += (c ? ", " : "") + json::quote(r.columns[c]);
        o += "]";
      }
      if (r.group_counts)
        o += ", \"group_counts\": {\"max_groups\": " + std::to_string(r.group_counts->max_groups) +
             ", \"max_value_bytes\": " + std::to_string(r.group_counts->max_value_bytes) + "}";
      if (r.value_rule) o += ", \"value_rule\": " + value_rule_json(*r.value_rule);
      o += "}";
    }
    o += "]}";
    *out_json = dup_string(o);
    return TGX_OK;
  } catch (const AnalyzerError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.text);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" int32_t tgx_host_type_class(const uint8_t *bytes, uint64_t len) {
  tgx::TcByteFetch f{bytes};
  return (int32_t)tgx::type_class_of(f, bytes ? len : 0);
}

extern "C" tgx_status tgx_host_data_type_state_json(const char *analyzer_json, const char *counts_json,
                                                    char **out_state_json, tgx_error *err) {
  if (!analyzer_json || !counts_json || !out_state_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_state_json = nullptr;
  try {
    auto a = analyzer_from_json(parse_json_text(analyzer_json, "analyzer"));
    json::Value v = parse_json_text(counts_json, "counts");
    if (!v.is(json::Value::Object)) return hfail(err, TGX_INVALID_ARGUMENT, "counts must be a JSON object");
    if (const json::Value *rs = v.get("results")) {
      if (!rs->is(json::Value::Array)) return hfail(err, TGX_INVALID_ARGUMENT, "results must be a JSON array");
      std::vector<tgx_result> results(rs->arr.size());
      std::vector<const tgx_result *> r;
      for (size_t i = 0; i < rs->arr.size(); i++) {
        memset(&results[i], 0, sizeof(tgx_result));
        results[i].total = (int64_t)rs->arr[i].get_u64("total", 0);
        results[i].non_null = (int64_t)rs->arr[i].get_u64("non_null", 0);
        results[i].matches = (int64_t)rs->arr[i].get_u64("matches", 0);
        r.push_back(&results[i]);
      }
      if (r.empty() || r.size() > 2) return hfail(err, TGX_INVALID_ARGUMENT, "results holds one or two tgx_results");
      *out_state_json = dup_string(json_dump(a->state_from_results(r, std::vector<int>())));
      return TGX_OK;
    }
    tgx_type_classes_counts c;
    c.seen = v.get_u64("seen", 0);
    c.non_null = v.get_u64("non_null", 0);
    c.boolean_rows = v.get_u64("boolean_rows", 0);
    c.integer_rows = v.get_u64("integer_rows", 0);
    c.double_rows = v.get_u64("double_rows", 0);
    c.date_rows = v.get_u64("date_rows", 0);
    c.datetime_rows = v.get_u64("datetime_rows", 0);
    c.string_rows = v.get_u64("string_rows", 0);
    c.undecided_rows = v.get_u64("undecided_rows", 0);
    *out_state_json = dup_string(json_dump(a->state_from_type_classes(c)));
    return TGX_OK;
  } catch (const AnalyzerError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.text);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_pair_counts_state_json(const char *analyzer_json, const char *pair_counts_json,
                                                      char **out_state_json, tgx_error *err) {
  if (!analyzer_json || !pair_counts_json || !out_state_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_state_json = nullptr;
  try {
    auto a = analyzer_from_json(parse_json_text(analyzer_json, "analyzer"));
    json::Value v = parse_json_text(pair_counts_json, "pair counts");
    PairCounts pc;
    if (const json::Value *s = v.get("summary")) {
      pc.summary.seen = s->get_u64("seen", 0);
      pc.summary.both_non_null = s->get_u64("both_non_null", 0);
      pc.summary.distinct = s->get_u64("distinct", 0);
      pc.summary.counted = s->get_u64("counted", 0);
      pc.summary.overflow_rows = s->get_u64("overflow_rows", 0);
      pc.summary.long_rows = s->get_u64("long_rows", 0);
      pc.summary.non_finite = s->get_u64("non_finite", 0);
      pc.summary.out_of_range = s->get_u64("out_of_range", 0);
    }
    if (const json::Value *es = v.get("entries")) {
      if (es->type != json::Value::Array) return hfail(err, TGX_INVALID_ARGUMENT, "entries must be a JSON array");
      for (const json::Value &e : es->arr) {
        if (e.type != json::Value::Array || e.arr.size() != 3)
          return hfail(err, TGX_INVALID_ARGUMENT, "an entry is [x, y, count]");
        PairCounts::Entry o;
        for (int side = 0; side < 2; side++) {
          PairCell &c = side ? o.y : o.x;
          const json::Value &j = e.arr[side];
          if (j.type == json::Value::String) {
            c.bytes = j.str;
          } else if (j.type == json::Value::Array) {
            for (const json::Value &b : j.arr) c.bytes += (char)(unsigned char)b.as_u64();
          } else if (j.type == json::Value::Number) {
            c.binned = true;
            c.bin = (int64_t)j.as_u64();
          } else {
            return hfail(err, TGX_INVALID_ARGUMENT, "a cell is a string, an array of bytes or a bin index");
          }
        }
        o.count = e.arr[2].as_u64();
        pc.entries.push_back(std::move(o));
      }
    }
    *out_state_json = dup_string(json_dump(a->state_from_pair_counts(pc)));
    return TGX_OK;
  } catch (const AnalyzerError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.text);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_group_counts_state_json(const char *analyzer_json, const char *group_counts_json,
                                                       char **out_state_json, tgx_error *err) {
  if (!analyzer_json || !group_counts_json || !out_state_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_state_json = nullptr;
  try {
    auto a = analyzer_from_json(parse_json_text(analyzer_json, "analyzer"));
    json::Value v = parse_json_text(group_counts_json, "group counts");
    GroupCounts gc;
    if (const json::Value *s = v.get("summary")) {
      gc.summary.seen = s->get_u64("seen", 0);
      gc.summary.groups = s->get_u64("groups", 0);
      gc.summary.counted = s->get_u64("counted", 0);
      gc.summary.counted_non_null = s->get_u64("counted_non_null", 0);
      gc.summary.null_group_rows = s->get_u64("null_group_rows", 0);
      gc.summary.null_group_non_null = s->get_u64("null_group_non_null", 0);
      gc.summary.overflow_rows = s->get_u64("overflow_rows", 0);
      gc.summary.overflow_non_null = s->get_u64("overflow_non_null", 0);
      gc.summary.long_rows = s->get_u64("long_rows", 0);
      gc.summary.long_non_null = s->get_u64("long_non_null", 0);
    }
    if (const json::Value *es = v.get("entries")) {
      if (es->type != json::Value::Array) return hfail(err, TGX_INVALID_ARGUMENT, "entries must be a JSON array");
      for (const json::Value &e : es->arr) {
        if (e.type != json::Value::Array || e.arr.size() != 3)
          return hfail(err, TGX_INVALID_ARGUMENT, "an entry is [key, total, non_null]");
        GroupCounts::Entry o;
        const json::Value &j = e.arr[0];
        if (j.type == json::Value::String) {
          gc.is_bytes = true;
          o.bytes = j.str;
        } else if (j.type == json::Value::Array) {
          gc.is_bytes = true;
          for (const json::Value &b : j.arr) o.bytes += (char)(unsigned char)b.as_u64();
        } else if (j.type == json::Value::Number) {
          o.value = j.as_i64();
        } else {
          return hfail(err, TGX_INVALID_ARGUMENT, "a key is a string, an array of bytes or an integer");
        }
        o.total = e.arr[1].as_u64();
        o.non_null = e.arr[2].as_u64();
        gc.entries.push_back(std::move(o));
      }
    }
    *out_state_json = dup_string(json_dump(a->state_from_group_counts(gc)));
    return TGX_OK;
  } catch (const AnalyzerError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.text);
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

// ---- cross-table constraints ---------------------------------------------------------------------------------------------
extern "C" tgx_status tgx_host_run_suite_tables_json(const char *suite_json, const tgx_host_table *tables, size_t n_tables,
                                                     char **out_json, tgx_error *err) {
  if (!suite_json || !out_json || (n_tables && !tables)) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    ValidationSuite suite = suite_from_json(suite_json);
    // {"table_column_types": {table: {column: DataType}}}: the Arrow types the caller holds for the further tables'
    // columns, where the layout they arrive in does not say (a Binary column arrives as a string layout)
    const json::Value doc = parse_json_text(suite_json, "suite");
    const json::Value *declared = doc.get("table_column_types");
    // (the suite's own table, registered under "table_name": the "column_types" the suite already carries)
    const json::Value *own = doc.get("column_types");
    const std::string own_name = suite.table_name();
    Context ctx;
    for (size_t k = 0; k < n_tables; k++) {
      const tgx_host_table &in = tables[k];
      if (!in.name || (in.n_columns && (!in.column_names || (in.n_batches && !in.columns))))
        return hfail(err, TGX_INVALID_ARGUMENT, "table " + std::to_string(k) + ": NULL argument");
      Table t;
      for (size_t i = 0; i < in.n_columns; i++) t.column_names.push_back(in.column_names[i]);
      for (size_t b = 0; b < in.n_batches; b++) {
        Batch batch;
        batch.columns.assign(in.columns + b * in.n_columns, in.columns + (b + 1) * in.n_columns);
        t.batches.push_back(std::move(batch));
      }
      const json::Value *types = declared ? declared->get(in.name) : nullptr;
      if (!types && own && own_name == in.name) types = own;
      if (types)
        for (const std::string &column : t.column_names) t.arrow_types.push_back(types->get_str(column));
      ctx.register_table(in.name, std::move(t));
    }
    ValidationResult r = suite.run(ctx);
    *out_json = dup_string(r.to_json());
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

static SideSums side_sums_from(const json::Value &v) {
  SideSums s;
  if (const json::Value *gs = v.get("groups")) {
    if (gs->type != json::Value::Array) throw TermError{TermError::Internal, "groups must be a JSON array"};
    for (const json::Value &e : gs->arr) {
      if (e.type != json::Value::Array || e.arr.size() != 2 || e.arr[1].type != json::Value::Number)
        throw TermError{TermError::Internal, "a group is [key, sum]"};
      SideSums::Group g;
      const json::Value &j = e.arr[0];
      if (j.type == json::Value::String) {
        s.is_bytes = true;
        g.bytes = j.str;
      } else if (j.type == json::Value::Array) {  // (bytes that are no text: an encoded tuple key)
        s.is_bytes = true;
        for (const json::Value &b : j.arr) g.bytes += (char)(unsigned char)b.as_u64();
      } else if (j.type == json::Value::Number) {
        g.value = j.as_i64();
      } else {
        throw TermError{TermError::Internal, "a key is a string, an array of bytes or an integer"};
      }
      g.sum = e.arr[1].num;
      s.groups.push_back(std::move(g));
    }
  }
  if (const json::Value *n = v.get("null_group"))
    if (n->type == json::Value::Number) s.null_group = n->num;
  s.overflow_rows = v.get_u64("overflow_rows", 0);
  s.long_rows = v.get_u64("long_rows", 0);
  s.arity = (int)v.get_u64("arity", 0);
  return s;
}

extern "C" tgx_status tgx_host_cross_table_sum_json(const char *constraint_json, const char *sums_json, char **out_json,
                                                    tgx_error *err) {
  if (!constraint_json || !sums_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto c = std::dynamic_pointer_cast<CrossTableSumConstraint>(constraint_from_json_text(constraint_json));
    if (!c) return hfail(err, TGX_INVALID_ARGUMENT, "not a cross_table_sum constraint");
    json::Value v;
    std::string perr;
    if (!json::parse(sums_json, &v, &perr)) return hfail(err, TGX_INVALID_ARGUMENT, "sums JSON: " + perr);
    const json::Value *l = v.get("left"), *r = v.get("right");
    if (!l || !r) return hfail(err, TGX_INVALID_ARGUMENT, "sums JSON needs 'left' and 'right'");
    (void)CrossTableSumConstraint::parse_qualified_column(c->left_column());
    (void)CrossTableSumConstraint::parse_qualified_column(c->right_column());
    const bool ungrouped = l->type == json::Value::Number && r->type == json::Value::Number;
    if (ungrouped != c->group_by_columns().empty())
      return hfail(err, TGX_INVALID_ARGUMENT, "a grouped constraint takes two sides of groups, an ungrouped one two numbers");
    const CrossTableSumRow row = ungrouped ? c->totals(l->num, r->num) : c->join(side_sums_from(*l), side_sums_from(*r));
    const ConstraintResult cr = c->verdict(row);
    std::string o = std::string("{\"status\": \"") +
                    (cr.status == ConstraintStatus::Success ? "success" : cr.status == ConstraintStatus::Failure ? "failure" : "skipped") +
                    "\", \"metric\": " + (cr.metric ? json_f64(*cr.metric) : "null") + ", \"message\": " +
                    (cr.message ? json::quote(*cr.message) : "null") + ", \"total_groups\": " +
                    std::to_string(row.total_groups) + ", \"violating_groups\": " + std::to_string(row.violating_groups) +
                    ", \"total_left_sum\": " + json_f64(row.total_left_sum) + ", \"total_right_sum\": " +
                    json_f64(row.total_right_sum) + ", \"max_difference\": " + json_f64(row.max_difference) +
                    ", \"config\": {\"name\": " + json::quote(c->name()) + ", \"left_column\": " +
                    json::quote(c->left_column()) + ", \"right_column\": " + json::quote(c->right_column()) + ", \"group_by\": [";
    for (size_t i = 0; i < c->group_by_columns().size(); i++) o += (i ? ", " : "") + json::quote(c->group_by_columns()[i]);
    o += "], \"tolerance\": " + json_f64(c->tolerance_value()) + ", \"max_violations_reported\": " +
         std::to_string(c->violations_reported()) + ", \"max_groups\": " + std::to_string(c->groups_bound()) +
         (c->composite_groups() ? ", \"composite_groups_on_device\": true" : "") + "}}";
    *out_json = dup_string(o);
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_join_coverage_json(const char *constraint_json, const char *counts_json, char **out_json,
                                                  tgx_error *err) {
  if (!constraint_json || !counts_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto c = std::dynamic_pointer_cast<JoinCoverageConstraint>(constraint_from_json_text(constraint_json));
    if (!c) return hfail(err, TGX_INVALID_ARGUMENT, "not a join_coverage constraint");
    json::Value v;
    std::string perr;
    if (!json::parse(counts_json, &v, &perr) || !v.is(json::Value::Object))
      return hfail(err, TGX_INVALID_ARGUMENT, "counts JSON: " + (perr.empty() ? std::string("not an object") : perr));
    c->validate();
    JoinCoverageCounts k;
    auto side = [&](const char *name, JoinCoverageCounts::Side *s) {
      const json::Value *o = v.get(name);
      if (!o) return;
      if (!o->is(json::Value::Object)) throw TermError{TermError::Internal, "counts JSON: a side is an object"};
      s->known = true;
      s->pairs = o->get_u64("pairs", 0);
      s->join_rows = o->get_u64("join_rows", 0);
      if (s->pairs > s->join_rows)
        throw TermError{TermError::Internal, "counts JSON: join_rows is pairs + missing_rows + null_rows"};
    };
    side("left", &k.left);
    side("right", &k.right);
    k.left_distinct = v.get_u64("left_distinct", 0);
    if (const json::Value *e = v.get("examples")) {
      if (!e->is(json::Value::Object)) throw TermError{TermError::Internal, "counts JSON: examples is an object"};
      k.examples_known = true;
      k.missing_keys = e->get_u64("missing_keys", 0);
      k.null_rows = e->get_u64("null_rows", 0);
      k.overflow_rows = e->get_u64("overflow_rows", 0);
      k.long_rows = e->get_u64("long_rows", 0);
      // (composite keys; absent: the NULL rows are one distinct value)
      k.null_keys_known = e->get("null_keys") != nullptr;
      k.null_keys = e->get_u64("null_keys", 0);
      k.null_overflow_rows = e->get_u64("null_overflow_rows", 0);
    }
    const ConstraintResult cr = c->verdict(k);
    std::string o =
        std::string("{\"status\": \"") +
        (cr.status == ConstraintStatus::Success ? "success" : cr.status == ConstraintStatus::Failure ? "failure" : "skipped") +
        "\", \"metric\": " + (cr.metric ? json_f64(*cr.metric) : "null") + ", \"message\": " +
        (cr.message ? json::quote(*cr.message) : "null") + ", \"config\": {\"name\": " + json::quote(c->name()) +
        ", \"left_table\": " + json::quote(c->left_table()) + ", \"right_table\": " + json::quote(c->right_table()) +
        ", \"join_keys\": [";
    for (size_t i = 0; i < c->join_keys().size(); i++)
      o += std::string(i ? ", " : "") + "[" + json::quote(c->join_keys()[i].first) + ", " +
           json::quote(c->join_keys()[i].second) + "]";
    o += std::string("], \"expected_match_rate\": ") + json_f64(c->expected_match_rate()) + ", \"coverage_type\": \"" +
         (c->coverage() == CoverageType::LeftCoverage ? "left" : c->coverage() == CoverageType::RightCoverage ? "right" : "bidirectional") +
         "\", \"distinct_only\": " + (c->distinct() ? "true" : "false") + ", \"max_examples_reported\": " +
         std::to_string(c->examples_reported()) + ", \"max_missing_keys\": " + std::to_string(c->missing_keys_bound()) +
         (c->value_bytes_given() ? ", \"max_value_bytes\": " + std::to_string(c->value_bytes_bound()) : std::string()) +
         (c->composite_keys() ? ", \"composite_keys_on_device\": true" : "") + "}}";
    *out_json = dup_string(o);
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}

extern "C" tgx_status tgx_host_foreign_key_json(const char *constraint_json, const char *counts_json, char **out_json,
                                                tgx_error *err) {
  if (!constraint_json || !counts_json || !out_json) return hfail(err, TGX_INVALID_ARGUMENT, "NULL argument");
  *out_json = nullptr;
  try {
    auto c = std::dynamic_pointer_cast<ForeignKeyConstraint>(constraint_from_json_text(constraint_json));
    if (!c) return hfail(err, TGX_INVALID_ARGUMENT, "not a foreign_key constraint");
    json::Value v;
    std::string perr;
    if (!json::parse(counts_json, &v, &perr) || !v.is(json::Value::Object))
      return hfail(err, TGX_INVALID_ARGUMENT, "counts JSON: " + (perr.empty() ? std::string("not an object") : perr));
    (void)ForeignKeyConstraint::parse_qualified_column(c->child_column());
    (void)ForeignKeyConstraint::parse_qualified_column(c->parent_column());
    ForeignKeyCounts k;
    k.null_rows = v.get_u64("null_rows", 0);
    k.missing_rows = v.get_u64("missing_rows", 0);
    k.overflow_rows = v.get_u64("overflow_rows", 0);
    k.long_rows = v.get_u64("long_rows", 0);
    if (v.get("examples")) k.examples = v.get_bool("examples");
    uint64_t counted = 0;
    if (const json::Value *es = v.get("entries")) {
      if (es->type != json::Value::Array) throw TermError{TermError::Internal, "entries must be a JSON array"};
      for (const json::Value &e : es->arr) {
        if (e.type != json::Value::Array || e.arr.size() != 2 ||
            (e.arr[0].type != json::Value::Number && e.arr[0].type != json::Value::String) ||
            e.arr[1].type != json::Value::Number)
          throw TermError{TermError::Internal, "an entry is [key, count]"};
        if (e.arr[0].type == json::Value::String) {  // string keys, ascending bytewise
          if (!k.keys.empty() || (!k.str_keys.empty() && !(k.str_keys.back() < e.arr[0].str)))
            throw TermError{TermError::Internal, "the entries must be ascending by key"};
          k.strings = true;
          k.str_keys.push_back(e.arr[0].str);
          counted += (uint64_t)e.arr[1].as_i64();
          continue;
        }
        if (k.strings) throw TermError{TermError::Internal, "the entries must be ascending by key"};
        const int64_t key = e.arr[0].as_i64();
        if (!k.keys.empty() && !(k.keys.back() < key))
          throw TermError{TermError::Internal, "the entries must be ascending by key"};
        k.keys.push_back(key);
        counted += (uint64_t)e.arr[1].as_i64();
      }
    }
    const uint64_t held = k.keys.size() + k.str_keys.size();
    k.missing_keys = v.get_u64("missing_keys", held);
    if (k.missing_keys != held || k.missing_rows != counted + k.overflow_rows + k.long_rows)
      throw TermError{TermError::Internal, "counts JSON: missing_keys is the number of entries and missing_rows the sum "
                                           "of their counts + overflow_rows + long_rows"};
    const ConstraintResult cr = c->verdict(k);
    const std::string o =
        std::string("{\"status\": \"") +
        (cr.status == ConstraintStatus::Success ? "success" : cr.status == ConstraintStatus::Failure ? "failure" : "skipped") +
        "\", \"metric\": " + (cr.metric ? json_f64(*cr.metric) : "null") + ", \"message\": " +
        (cr.message ? json::quote(*cr.message) : "null") + ", \"config\": {\"name\": " + json::quote(c->name()) +
        ", \"child_column\": " + json::quote(c->child_column()) + ", \"parent_column\": " +
        json::quote(c->parent_column()) + ", \"allow_nulls\": " + (c->nulls_allowed() ? "true" : "false") +
        ", \"use_left_join\": " + (c->left_join() ? "true" : "false") + ", \"max_violations_reported\": " +
        std::to_string(c->violations_reported()) + ", \"max_missing_keys\": " + std::to_string(c->missing_keys_bound()) +
        (c->value_bytes_given() ? ", \"max_value_bytes\": " + std::to_string(c->value_bytes_bound()) : std::string()) + "}}";
    *out_json = dup_string(o);
    return TGX_OK;
  } catch (const TermError &e) {
    return hfail(err, TGX_INVALID_ARGUMENT, e.display());
  } catch (const std::bad_alloc &) {
    return hfail(err, TGX_OUT_OF_MEMORY, "host allocation failed (std::bad_alloc)");
  } catch (const std::exception &e) {
    return hfail(err, TGX_INTERNAL, e.what());
  } catch (...) {
    return hfail(err, TGX_INTERNAL, "unknown C++ exception");
  }
}
