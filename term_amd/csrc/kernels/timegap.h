// timegap.h -- descriptors shared by kernels/timegap.hip and timegap_device.cpp (TGX_CHECK_TIME_GAP).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgx {

constexpr int kTimeGapThresholds = 8;  // thresholds one neighbour pass compares with (more specs of a task: more passes)

struct TimeGapBatch {  // one batch's Int64 views: the timestamp column and, or nullptr, the group column
  const void *t, *g;
  const uint8_t *tv, *gv;
  int64_t toff, goff;
  int64_t length;
};

struct TimeGapThresholds {
  int32_t n;
  int64_t max_gap[kTimeGapThresholds];
};

void launch_timegap_compact(const TimeGapBatch &d, uint64_t *kt, uint64_t *kg, uint64_t cap, unsigned long long *count,
                            hipStream_t stream);
void launch_timegap_compose(uint64_t *ranks, uint64_t n, hipStream_t stream);
// out[0] += gaps, out[1] = max(out[1], largest gap), out[2 + k] += gaps above T.max_gap[k]; tags: the composed keys
// beside vals (grouped), or nullptr
void launch_timegap_neighbours(const uint64_t *vals, const uint64_t *tags, uint64_t n, const TimeGapThresholds &T,
                               unsigned long long *out, hipStream_t stream);

}  // namespace tgx
