// histogram_device.h -- TGX_CHECK_HISTOGRAM tasks of a state (range / count phase on the device, additive host part);
// see histogram_device.cpp.
#pragma once
#include "internal.h"
#include "wire_io.h"

namespace tgx {
tgx_status hist_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err);
void hist_state_init(tgx_state *st);
void hist_state_free(tgx_state *st);
tgx_status hist_state_reset(tgx_state *st, tgx_error *err);
// one batch (device views of the plan's columns) through the tasks' kernels
tgx_status hist_update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err);
tgx_status hist_fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err);
tgx_status hist_merge_states(tgx_state *dst, tgx_state *src, tgx_error *err);
// the blob's section: present only when the plan has such tasks (blobs of other plans keep their bytes)
TGX_HIDDEN tgx_status hist_serialize(tgx_state *st, Writer &w, tgx_error *err);
TGX_HIDDEN tgx_status hist_deserialize(tgx_state *st, Reader &r, tgx_error *err);
}  // namespace tgx
