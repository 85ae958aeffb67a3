// temporal.hip -- row predicates over timestamp columns for gfx950 (TGX_CHECK_TEMPORAL): the three pure-scan modes of
// the reference's TemporalOrderingConstraint (TG/constraints/temporal_ordering.rs:346-453), each a
//   SELECT COUNT(*), SUM(CASE WHEN <row predicate> THEN 0 ELSE 1 END) FROM t WHERE ...
//
//   ORDER        after - before >= delta, the difference taken in 128 bits (it cannot wrap)
//   TIME_OF_DAY  lo <= floormod(t, ticks per day) <= hi, optionally only over Monday .. Friday
//   RANGE        lo <= t <= hi
//
// One kernel, grid = (blocks, tasks).  The loads are those of jointbins.hip (row_walk.h); the single-column modes read
// one column: 8 B + 1 bit per row.  Per lane two 32-bit counters (rows considered, rows that pass), reduced within the
// wave by shuffles and added to the task's two 64-bit counters with one vector atomic per wave and counter: no LDS, no
// per-row atomic.
//
// The divisions are by compile-time constants: the mode and the column's unit are wave-uniform and dispatched OUTSIDE
// the row loop, so 86400 * 10^k and 7 reach the compiler as literals and become multiply-high sequences (a 64-bit
// division by a runtime value is an emulated routine of the order of a hundred instructions, against a streaming budget
// of a few tens per row).  The floor forms are written out: C++'s / and % truncate toward zero, and timestamps before
// 1970 are negative.
#include <hip/hip_runtime.h>

#include "bin_count.h"
#include "device_types.h"
#include "row_walk.h"

namespace tgx {

namespace {

template <int64_t kTicksPerDay>
__device__ __forceinline__ bool tp_time_of_day(int64_t t, int64_t lo, int64_t hi, bool weekdays_only, bool *weekday) {
  int64_t day = t / kTicksPerDay;
  int64_t tod = t - day * kTicksPerDay;
  if (tod < 0) {  // floor, not truncation
    tod += kTicksPerDay;
    day -= 1;
  }
  if (weekdays_only) {
    // 1970-01-01 is a Thursday; DOW 0 is Sunday.  |day| < 2^47, so day + 4 cannot wrap
    int64_t dow = (day + 4) % 7;
    if (dow < 0) dow += 7;
    *weekday = dow >= 1 && dow <= 5;
  }
  return lo <= tod && tod <= hi;
}

template <int64_t kTicksPerSecond>
__device__ __forceinline__ void tp_scan_time_of_day(const ComomentColDesc &d, const TemporalParams &P,
                                                    unsigned long long *__restrict__ out) {
  uint32_t considered = 0, passed = 0;  // (a workgroup sees fewer than 2^32 rows: temporal_update)
  const int64_t lo = P.lo, hi = P.hi;
  if (P.weekdays_only) {
    jb_for_rows_single(d, [&](int64_t t, bool ok) {
      bool weekday = true;
      const bool pass = tp_time_of_day<86400 * kTicksPerSecond>(t, lo, hi, true, &weekday);
      considered += ok && weekday ? 1u : 0u;
      passed += ok && weekday && pass ? 1u : 0u;
    });
  } else {
    jb_for_rows_single(d, [&](int64_t t, bool ok) {
      bool weekday = true;
      const bool pass = tp_time_of_day<86400 * kTicksPerSecond>(t, lo, hi, false, &weekday);
      considered += ok ? 1u : 0u;
      passed += ok && pass ? 1u : 0u;
    });
  }
  tail_flush(considered, passed, out);
}

}  // namespace

__global__ __launch_bounds__(kTemporalBlock) void temporal_kernel(const TemporalLaunch L) {
  const ComomentColDesc d = L.cols[blockIdx.y];
  const TemporalParams P = L.params[blockIdx.y];
  unsigned long long *__restrict__ out = L.counters[blockIdx.y];
  if (P.mode == kTemporalOrder) {
    uint32_t considered = 0, passed = 0;
    const __int128 delta = P.delta;
    jb_for_rows(d, [&](int64_t before, int64_t after, bool ok) {
      const bool pass = (__int128)after - (__int128)before >= delta;
      considered += ok ? 1u : 0u;
      passed += ok && pass ? 1u : 0u;
    });
    tail_flush(considered, passed, out);
  } else if (P.mode == kTemporalRange) {
    uint32_t considered = 0, passed = 0;
    const int64_t lo = P.lo, hi = P.hi;
    jb_for_rows_single(d, [&](int64_t t, bool ok) {
      considered += ok ? 1u : 0u;
      passed += ok && lo <= t && t <= hi ? 1u : 0u;
    });
    tail_flush(considered, passed, out);
  } else {
    switch (P.ticks_per_second) {  // (one of the four: tgx_plan_set_temporal)
      case 1: tp_scan_time_of_day<1>(d, P, out); break;
      case 1000: tp_scan_time_of_day<1000>(d, P, out); break;
      case 1000000: tp_scan_time_of_day<1000000>(d, P, out); break;
      default: tp_scan_time_of_day<1000000000>(d, P, out); break;
    }
  }
}

void launch_temporal(const TemporalLaunch &L, int n_tasks, int blocks_per_task, hipStream_t stream) {
  hipLaunchKernelGGL(temporal_kernel, dim3(blocks_per_task, n_tasks), dim3(kTemporalBlock), 0, stream, L);
}

}  // namespace tgx
