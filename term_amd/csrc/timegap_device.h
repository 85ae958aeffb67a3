// timegap_device.h -- TIME_GAP tasks of a plan/state (kernels/timegap.hip); see timegap_device.cpp.
#pragma once
#include <vector>

#include "internal.h"

namespace tgx {
// one task per (timestamp column, group column): the specs on it differ in their thresholds only
struct TimeGapSpec {
  int spec_index;
  bool set;  // tgx_plan_set_time_gap was called
  int64_t max_gap;
};
struct TimeGapTask {
  int col_t, col_g;  // col_g: -1 without a group column
  std::vector<TimeGapSpec> specs;
};
tgx_status timegap_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err);
void timegap_plan_free(tgx_plan *plan);
size_t timegap_num_tasks(const tgx_plan *plan);
// a spec without its threshold refuses tgx_state_create
tgx_status timegap_plan_ready(const tgx_plan *plan, tgx_error *err);
// used / reads_values / needs_wide (group columns) / timegap_on of the plan's columns
void timegap_mark_used(tgx_plan *plan);
// the column types a task takes (include/tgx.h): TGX_UNSUPPORTED otherwise
tgx_status timegap_check_type(const tgx_plan *plan, int column, int type, tgx_error *err);
void timegap_state_init(tgx_state *st);
void timegap_state_free(tgx_state *st);
void timegap_state_reset(tgx_state *st);
tgx_status timegap_update(tgx_state *st, const tgx_column *dev_columns, int64_t nrows, tgx_error *err);
tgx_status timegap_fill_result(tgx_state *st, int spec_index, tgx_result *r, tgx_error *err);
// retained rows of one data set are not mergeable: TGX_UNSUPPORTED when a task holds rows
tgx_status timegap_check_mergeable(tgx_state *st, const char *what, tgx_error *err);
}  // namespace tgx
