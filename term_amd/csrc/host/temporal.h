// temporal.h -- TemporalOrderingConstraint (TG/constraints/temporal_ordering.rs) over TGX_CHECK_TEMPORAL: the
// BeforeAfter, BusinessHours and DateRange modes are one scan on the device; MaxTimeGap (a window query) is an error
// unless window_on_device(true) asks for TGX_CHECK_TIME_GAP; EventSequence is an error.  Included by term_guard.h's users
// through term_guard.cpp and host_abi.cpp.
#pragma once
#include "json.h"
#include "term_guard.h"

namespace term_guard {

class TemporalOrderingConstraint : public Constraint {
 public:
  enum class Validation { BeforeAfter, BusinessHours, DateRange, MaxTimeGap, EventSequence };
  // temporal_ordering.rs:120-288, one method per builder call of the reference
  explicit TemporalOrderingConstraint(std::string table) : table_name_(std::move(table)) {}
  TemporalOrderingConstraint &before_after(std::string before, std::string after);
  TemporalOrderingConstraint &before_or_equal(std::string before, std::string after);
  TemporalOrderingConstraint &business_hours(std::string column, std::string start_time, std::string end_time);
  TemporalOrderingConstraint &weekdays_only(bool on);            // BusinessHours only, as in the reference
  TemporalOrderingConstraint &with_timezone(std::string tz);     // stored; never reaches the query (:385-391)
  TemporalOrderingConstraint &date_range(std::string column, std::optional<std::string> min_date,
                                         std::optional<std::string> max_date);
  TemporalOrderingConstraint &max_time_gap(std::string column, int64_t max_gap_seconds);
  TemporalOrderingConstraint &group_by(std::string column);      // MaxTimeGap only
  // MaxTimeGap only (this layer's own call; the reference has none): run the LAG() window on the device as a
  // TGX_CHECK_TIME_GAP.  Off by default: the check keeps 8 B per row (16 B with a group) on the device until the verdict
  // and its state cannot be merged, serialized or reduced across ranks -- no other check of a suite costs that.
  TemporalOrderingConstraint &window_on_device(bool on);
  TemporalOrderingConstraint &event_sequence(std::string event_column, std::string timestamp_column,
                                             std::vector<std::string> expected);
  TemporalOrderingConstraint &allow_nulls(bool allow) { allow_nulls_ = allow; return *this; }
  TemporalOrderingConstraint &tolerance_seconds(int64_t s) { tolerance_seconds_ = s; return *this; }

  std::string name() const override { return "temporal_ordering"; }
  std::vector<SpecRequest> plan() const override;
  ConstraintResult evaluate(const Inputs &in) const override;

  Validation validation() const { return validation_; }
  const std::string &table_name() const { return table_name_; }
  bool nulls_allowed() const { return allow_nulls_; }
  int64_t tolerance() const { return tolerance_seconds_; }
  bool weekdays() const { return weekdays_only_; }
  bool on_device_window() const { return window_on_device_; }

 private:
  std::string table_name_;
  Validation validation_ = Validation::BeforeAfter;
  std::string column_, column2_;  // before / after; timestamp column; (EventSequence: timestamp / event column)
  bool allow_equal_ = false, weekdays_only_ = false, allow_nulls_ = false, window_on_device_ = false;
  std::string start_time_, end_time_;
  std::optional<std::string> timezone_, min_date_, max_date_, group_by_;
  int64_t max_gap_seconds_ = 0, tolerance_seconds_ = 0;
  std::vector<std::string> expected_sequence_;
};

// request + the Arrow DataType names of its column(s) ("Timestamp(Nanosecond, None)"; `type2` only in order mode) ->
// the device's parameters, in the column's ticks.  Throws TermError (constraint evaluation, 'temporal_ordering')
// naming what is missing: the caller hands such a constraint back to the stock path.
tgx_temporal_params temporal_params(const TemporalRequest &req, const std::string &type, const std::string &type2);
// the same for a kTemporalTimeGapMode request: max_gap = max_gap_seconds x the timestamp column's ticks per second.  The
// timestamp column must be an Arrow Timestamp (any zone: a difference has none); `group_type` is the group column's type,
// or empty (no group column, or a type the caller does not know: the device decides)
tgx_time_gap_params time_gap_params(const TemporalRequest &req, const std::string &type, const std::string &group_type);
std::shared_ptr<Constraint> temporal_ordering_from_json(const json::Value &c);

}  // namespace term_guard
