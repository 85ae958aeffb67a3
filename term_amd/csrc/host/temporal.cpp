// temporal.cpp -- TemporalOrderingConstraint (TG/constraints/temporal_ordering.rs), quirks included.
#include "temporal.h"

#include <stdio.h>
#include <string.h>

#include "json.h"

namespace term_guard {

namespace {

[[noreturn]] void evaluation_error(const std::string &msg) {
  throw TermError{TermError::ConstraintEvaluation, "'temporal_ordering': " + msg};
}

void require_identifier(const std::string &id) {
  if (auto e = validate_identifier(id)) throw *e;
}

struct ArrowTimestamp {
  bool is_timestamp = false;
  int64_t ticks_per_second = 0;
  std::string tz;  // "None", or what stands inside Some("..")
};

ArrowTimestamp parse_arrow_type(const std::string &t) {
  ArrowTimestamp a;
  if (t.rfind("Timestamp(", 0) != 0 || t.back() != ')') return a;
  const size_t comma = t.find(',');
  if (comma == std::string::npos) return a;
  const std::string unit = t.substr(10, comma - 10);
  if (unit == "Second") a.ticks_per_second = 1;
  else if (unit == "Millisecond") a.ticks_per_second = 1000;
  else if (unit == "Microsecond") a.ticks_per_second = 1000000;
  else if (unit == "Nanosecond") a.ticks_per_second = 1000000000;
  else return a;
  std::string tz = t.substr(comma + 1, t.size() - comma - 2);
  while (!tz.empty() && tz.front() == ' ') tz.erase(0, 1);
  if (tz.rfind("Some(\"", 0) == 0 && tz.size() >= 8) tz = tz.substr(6, tz.size() - 8);
  a.tz = tz;
  a.is_timestamp = true;
  return a;
}

std::string shown(const std::string &type) { return type.empty() ? "an unknown type" : type; }

ArrowTimestamp need_timestamp(const std::string &type, const char *what, bool utc_only) {
  const ArrowTimestamp a = parse_arrow_type(type);
  if (!a.is_timestamp)
    evaluation_error(std::string(what) + " needs a Timestamp(unit, tz) column to know its unit; the column is " +
                     shown(type) + " (not on the GPU path)");
  if (utc_only && a.tz != "None" && a.tz != "UTC" && a.tz != "+00:00")
    evaluation_error(std::string(what) + " needs a column without a time zone, or in UTC; the column is " + type +
                     " (not on the GPU path)");
  return a;
}

bool digits(const std::string &s, size_t at, size_t n, int *out) {
  if (at + n > s.size()) return false;
  int v = 0;
  for (size_t i = 0; i < n; i++) {
    if (s[at + i] < '0' || s[at + i] > '9') return false;
    v = v * 10 + (s[at + i] - '0');
  }
  *out = v;
  return true;
}

// "HH:MM" (+ ":00") as seconds into the day
int64_t hhmm_seconds(const std::string &text) {
  int h = 0, m = 0;
  if (text.size() != 5 || text[2] != ':' || !digits(text, 0, 2, &h) || !digits(text, 3, 2, &m) || h > 23 || m > 59)
    evaluation_error("Temporal validation query failed: cannot parse '" + text + ":00' as a TIME literal");
  return (int64_t)h * 3600 + m * 60;
}

int64_t days_from_civil(int64_t y, int m, int d) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}

// TIMESTAMP '<text>' as nanoseconds since the epoch: YYYY-MM-DD, YYYY-MM-DD HH:MM:SS[.f{1,9}], the T form; no offset,
// or Z
int64_t literal_ns(const std::string &text) {
  auto bad = [&]() {
    evaluation_error("Temporal validation query failed: cannot parse '" + text + "' as a TIMESTAMP literal");
  };
  int y = 0, mo = 0, d = 0, hh = 0, mi = 0, ss = 0;
  int64_t frac = 0;
  if (!digits(text, 0, 4, &y) || text.size() < 10 || text[4] != '-' || !digits(text, 5, 2, &mo) || text[7] != '-' ||
      !digits(text, 8, 2, &d))
    bad();
  size_t at = 10;
  if (at < text.size()) {
    if ((text[at] != ' ' && text[at] != 'T') || !digits(text, at + 1, 2, &hh) || text.size() < at + 9 ||
        text[at + 3] != ':' || !digits(text, at + 4, 2, &mi) || text[at + 6] != ':' || !digits(text, at + 7, 2, &ss))
      bad();
    at += 9;
    if (at < text.size() && text[at] == '.') {
      size_t n = 0;
      at++;
      while (at < text.size() && text[at] >= '0' && text[at] <= '9' && n < 9) {
        frac = frac * 10 + (text[at] - '0');
        at++;
        n++;
      }
      if (n == 0) bad();
      for (; n < 9; n++) frac *= 10;
    }
    if (at < text.size() && text[at] == 'Z') at++;
  }
  if (at != text.size()) bad();
  const bool leap = y % 4 == 0 && (y % 100 != 0 || y % 400 == 0);
  const int mdays[12] = {31, leap ? 29 : 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  if (mo < 1 || mo > 12 || d < 1 || d > mdays[mo - 1] || hh > 23 || mi > 59 || ss > 59) bad();
  const __int128 ns =
      ((__int128)days_from_civil(y, mo, d) * 86400 + hh * 3600 + mi * 60 + ss) * 1000000000 + frac;
  if (ns < (__int128)INT64_MIN || ns > (__int128)INT64_MAX) bad();  // (a nanosecond instant is an i64)
  return (int64_t)ns;
}

int64_t floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && (a < 0)) ? 1 : 0); }
int64_t ceil_div(int64_t a, int64_t b) { return a / b + ((a % b != 0 && (a > 0)) ? 1 : 0); }

}  // namespace

// ---- builder (temporal_ordering.rs:140-288) ---------------------------------------------------------------------------
TemporalOrderingConstraint &TemporalOrderingConstraint::before_after(std::string before, std::string after) {
  validation_ = Validation::BeforeAfter;
  column_ = std::move(before);
  column2_ = std::move(after);
  allow_equal_ = false;
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::before_or_equal(std::string before, std::string after) {
  before_after(std::move(before), std::move(after));
  allow_equal_ = true;
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::business_hours(std::string column, std::string start_time,
                                                                       std::string end_time) {
  validation_ = Validation::BusinessHours;
  column_ = std::move(column);
  start_time_ = std::move(start_time);
  end_time_ = std::move(end_time);
  weekdays_only_ = false;
  timezone_.reset();
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::weekdays_only(bool on) {
  if (validation_ == Validation::BusinessHours) weekdays_only_ = on;  // (:191-209: ignored on every other type)
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::with_timezone(std::string tz) {
  if (validation_ == Validation::BusinessHours) timezone_ = std::move(tz);
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::date_range(std::string column, std::optional<std::string> min_date,
                                                                   std::optional<std::string> max_date) {
  validation_ = Validation::DateRange;
  column_ = std::move(column);
  min_date_ = std::move(min_date);
  max_date_ = std::move(max_date);
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::max_time_gap(std::string column, int64_t max_gap_seconds) {
  validation_ = Validation::MaxTimeGap;
  column_ = std::move(column);
  group_by_.reset();
  window_on_device_ = false;
  max_gap_seconds_ = max_gap_seconds;
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::window_on_device(bool on) {
  if (validation_ == Validation::MaxTimeGap) window_on_device_ = on;  // (ignored on every other type, as weekdays_only)
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::group_by(std::string column) {
  if (validation_ == Validation::MaxTimeGap) group_by_ = std::move(column);
  return *this;
}
TemporalOrderingConstraint &TemporalOrderingConstraint::event_sequence(std::string event_column,
                                                                       std::string timestamp_column,
                                                                       std::vector<std::string> expected) {
  validation_ = Validation::EventSequence;
  column_ = std::move(timestamp_column);
  column2_ = std::move(event_column);
  expected_sequence_ = std::move(expected);
  return *this;
}

// generate_validation_query (:337-493): identifiers first, then the type's own errors
std::vector<SpecRequest> TemporalOrderingConstraint::plan() const {
  require_identifier(table_name_);
  SpecRequest r;
  r.kind = TGX_CHECK_TEMPORAL;
  r.column = column_;
  TemporalRequest t;
  t.allow_nulls = allow_nulls_;
  t.tolerance_seconds = tolerance_seconds_;  // (read in order mode only, as in the reference)
  switch (validation_) {
    case Validation::BeforeAfter:
      require_identifier(column_);
      require_identifier(column2_);
      r.column2 = column2_;
      t.mode = TGX_TEMPORAL_ORDER;
      t.allow_equal = allow_equal_;
      break;
    case Validation::BusinessHours:
      require_identifier(column_);
      t.mode = TGX_TEMPORAL_TIME_OF_DAY;
      t.start_time = start_time_;
      t.end_time = end_time_;
      t.weekdays_only = weekdays_only_;
      break;
    case Validation::DateRange:
      require_identifier(column_);
      if (!min_date_ && !max_date_)
        evaluation_error("DateRange validation requires at least min_date or max_date");  // :431-436
      t.mode = TGX_TEMPORAL_RANGE;
      t.min_date = min_date_;
      t.max_date = max_date_;
      break;
    case Validation::MaxTimeGap:
      require_identifier(column_);
      if (group_by_) require_identifier(*group_by_);
      if (!window_on_device_)
        evaluation_error("MaxTimeGap validation is a LAG() OVER (ORDER BY ..) window query and is not on the GPU path");
      r.kind = TGX_CHECK_TIME_GAP;  // (allow_nulls is not read: the query's WHERE ts IS NOT NULL stands either way)
      if (group_by_) r.column2 = *group_by_;
      t.mode = kTemporalTimeGapMode;
      t.max_gap_seconds = max_gap_seconds_;
      break;
    case Validation::EventSequence:
      require_identifier(column2_);
      require_identifier(column_);
      evaluation_error("Event sequence validation not yet implemented");  // :482-488
  }
  r.temporal = t;
  return {r};
}

// :521-602.  The result carries total = rows seen, non_null = the query's COUNT(*), matches = COUNT(*) - violations
// (MaxTimeGap, :551-601: COUNT(*) is the number of gaps; no gaps at all is a Success with metric 1.0)
ConstraintResult TemporalOrderingConstraint::evaluate(const Inputs &in) const {
  const tgx_result &r = *in.results.at(0);
  const int64_t total_rows = r.non_null, violations = r.non_null - r.matches;
  if (violations == 0) return ConstraintResult::success_with_metric(1.0);  // (no considered rows: SUM is NULL, read as 0)
  const double rate = total_rows > 0 ? (double)(total_rows - violations) / (double)total_rows : 1.0;
  char pct[64];
  snprintf(pct, sizeof(pct), "%.2f", rate * 100.0);
  const std::string v = std::to_string(violations);
  std::string msg;
  switch (validation_) {
    case Validation::BeforeAfter:
      msg = "Temporal ordering violation: " + v + " records where '" + column_ + "' is not before '" + column2_ + "' (" +
            pct + "% compliance)";
      break;
    case Validation::BusinessHours:
      msg = "Business hours violation: " + v + " records with '" + column_ + "' outside business hours (" + pct +
            "% compliance)";
      break;
    case Validation::DateRange:
      msg = "Date range violation: " + v + " records with '" + column_ + "' outside valid range (" + pct +
            "% compliance)";
      break;
    case Validation::MaxTimeGap:
      msg = "Time gap violation: " + v + " gaps exceed maximum allowed (" + pct + "% compliance)";
      break;
    default:
      msg = "Temporal validation failed: " + v + " violations (" + pct + "% compliance)";
  }
  return ConstraintResult::failure_with_metric(rate, msg);
}

tgx_temporal_params temporal_params(const TemporalRequest &req, const std::string &type, const std::string &type2) {
  tgx_temporal_params p;
  memset(&p, 0, sizeof(p));
  p.mode = req.mode;
  p.flags = req.allow_nulls ? TGX_TEMPORAL_KEEP_NULLS : 0;
  p.lo = INT64_MIN;
  p.hi = INT64_MAX;
  switch (req.mode) {
    case TGX_TEMPORAL_ORDER: {
      // :352-368: allow_equal picks '>' and the default '>=' (yes, inverted); the tolerance only when > 0
      int64_t tol = 0;
      if (req.tolerance_seconds > 0) {
        const ArrowTimestamp a = need_timestamp(type, "a tolerance in seconds", false);
        const ArrowTimestamp b = need_timestamp(type2, "a tolerance in seconds", false);
        if (a.ticks_per_second != b.ticks_per_second)
          evaluation_error("a tolerance in seconds needs both columns in the same unit; they are " + type + " and " +
                           type2 + " (not on the GPU path)");
        if (__builtin_mul_overflow(req.tolerance_seconds, a.ticks_per_second, &tol) || tol == INT64_MAX)
          evaluation_error("Temporal validation query failed: the tolerance overflows the column's unit");
      }
      p.delta = req.allow_equal ? tol + 1 : tol;
      break;
    }
    case TGX_TEMPORAL_TIME_OF_DAY: {
      const ArrowTimestamp a = need_timestamp(type, "business hours validation", true);
      p.ticks_per_second = a.ticks_per_second;
      p.tod_lo = hhmm_seconds(req.start_time) * a.ticks_per_second;
      p.tod_hi = hhmm_seconds(req.end_time) * a.ticks_per_second;
      if (req.weekdays_only) p.flags |= TGX_TEMPORAL_WEEKDAYS_ONLY;
      break;
    }
    case TGX_TEMPORAL_RANGE: {
      const ArrowTimestamp a = need_timestamp(type, "date range validation", true);
      const int64_t per = 1000000000 / a.ticks_per_second;  // a literal is a nanosecond instant
      if (req.min_date) p.lo = ceil_div(literal_ns(*req.min_date), per);
      if (req.max_date) p.hi = floor_div(literal_ns(*req.max_date), per);
      break;
    }
    default:
      evaluation_error("unknown temporal mode " + std::to_string(req.mode));
  }
  return p;
}

tgx_time_gap_params time_gap_params(const TemporalRequest &req, const std::string &type, const std::string &group_type) {
  if (req.mode != kTemporalTimeGapMode) evaluation_error("unknown temporal mode " + std::to_string(req.mode));
  const ArrowTimestamp a = need_timestamp(type, "max time gap validation on the device", false);
  static const char *const kGroupTypes[] = {"Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "Date32", "Date64"};
  bool group_ok = group_type.empty() || parse_arrow_type(group_type).is_timestamp;
  for (const char *g : kGroupTypes) group_ok = group_ok || group_type == g;
  if (!group_ok)
    evaluation_error("max time gap validation on the device needs a group column of Int8 .. Int64, UInt8 .. UInt32, a date "
                     "or a timestamp; the column is " + group_type + " (not on the GPU path)");
  tgx_time_gap_params p;
  memset(&p, 0, sizeof(p));
  if (__builtin_mul_overflow(req.max_gap_seconds, a.ticks_per_second, &p.max_gap))
    evaluation_error("Temporal validation query failed: the maximum gap overflows the column's unit");
  return p;
}

Check::Builder &Check::Builder::temporal_ordering(std::string table) {
  return constraint(std::make_shared<TemporalOrderingConstraint>(std::move(table)));
}

// {"type": "temporal_ordering", "table": t, "validation": "before_after|business_hours|date_range|max_time_gap|
//  event_sequence" (absent: the default object of TemporalOrderingConstraint::new), .. the builder calls' arguments ..;
//  "window_on_device": true with max_time_gap only}
std::shared_ptr<Constraint> temporal_ordering_from_json(const json::Value &c) {
  auto t = std::make_shared<TemporalOrderingConstraint>(c.get_str("table", "data"));
  const std::string v = c.get_str("validation");
  auto opt = [&](const char *key) -> std::optional<std::string> {
    const json::Value *x = c.get(key);
    return x && x->is(json::Value::String) ? std::optional<std::string>(x->str) : std::nullopt;
  };
  if (v == "before_after") {
    if (c.get_bool("allow_equal")) t->before_or_equal(c.get_str("before_column"), c.get_str("after_column"));
    else t->before_after(c.get_str("before_column"), c.get_str("after_column"));
  } else if (v == "business_hours") {
    t->business_hours(c.get_str("timestamp_column"), c.get_str("start_time"), c.get_str("end_time"));
    t->weekdays_only(c.get_bool("weekdays_only"));
    if (auto tz = opt("timezone")) t->with_timezone(*tz);
  } else if (v == "date_range") {
    t->date_range(c.get_str("timestamp_column"), opt("min_date"), opt("max_date"));
  } else if (v == "max_time_gap") {
    t->max_time_gap(c.get_str("timestamp_column"), c.get_i64("max_gap_seconds"));
    if (auto g = opt("group_by_column")) t->group_by(*g);
    t->window_on_device(c.get_bool("window_on_device"));
  } else if (v == "event_sequence") {
    std::vector<std::string> seq;
    if (const json::Value *s = c.get("expected_sequence"))
      for (const json::Value &e : s->arr) seq.push_back(e.str);
    t->event_sequence(c.get_str("event_column"), c.get_str("timestamp_column"), std::move(seq));
  } else if (!v.empty()) {
    throw TermError{TermError::Internal, "unknown temporal validation '" + v + "'"};
  }
  t->allow_nulls(c.get_bool("allow_nulls"));
  t->tolerance_seconds(c.get_i64("tolerance_seconds"));
  return t;
}

}  // namespace term_guard
