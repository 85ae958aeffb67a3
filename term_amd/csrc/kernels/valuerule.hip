// valuerule.hip -- numeric value rules for gfx950 (TGX_CHECK_VALUE_RULE): the fixed predicates of the reference's
// DataTypeConstraint (TG/constraints/datatype.rs:144-160), each a
//   SELECT COUNT(*), SUM(CASE WHEN <predicate> THEN 1 ELSE 0 END) FROM t WHERE col IS NOT NULL
//
//   GE_ZERO / GT_ZERO / BETWEEN   one inclusive range test lo <= k <= hi.  The host picks the key k per rule -- the
//                                 int64 value, or the IEEE totalOrder key of the value as a double -- and folds the
//                                 mode into the bounds (device_types.h), so the row loop holds no mode at all
//   INTEGER                       col = CAST(col AS INT): does the value fit Int32 (a cast error if not), and does the
//                                 cast give the value back
//
// One kernel, grid = (blocks, column groups).  A group is one column and up to 8 of its rules: the column is walked
// once (row_walk.h's single-column form: 8 B + 1 bit per row) and every rule is evaluated on the row in registers.
// What a group needs is wave-uniform and dispatched OUTSIDE the row loop, as template arguments: the number of rules
// (1, 2, 4 or 8, padded with rules that match nothing, so the per-rule counters are registers and not scratch), whether
// the column holds doubles, whether any rule reads the totalOrder key, whether any rule is INTEGER.  Per lane one
// 32-bit counter of non-NULL rows for the group and two per rule (valid, cast errors), reduced within the wave by
// shuffles and added to 64-bit counters with one vector atomic per wave and counter, non-zero values only (the group's
// non-NULL rows go to the slot of its first rule): no LDS, no per-row atomic.
//
// The Int32 range test for doubles is two compares against constants (a NaN fails both): truncation toward zero keeps
// everything in (-2^31 - 1, 2^31) in range, num-traits' rule.  There is no division anywhere.
#include <hip/hip_runtime.h>

#include "bin_count.h"
#include "device_types.h"
#include "row_walk.h"

namespace tgx {

namespace {

// kRules: rules evaluated per row (those from `n` on match nothing).  kFloat: the column's bits are doubles.  kKeys: a
// rule reads the totalOrder key (every range rule of a float column does).  kInteger: a rule is kRuleInteger.
template <int kRules, bool kFloat, bool kKeys, bool kInteger>
__device__ __forceinline__ void vr_scan(const ComomentColDesc &d, const ValueRule *__restrict__ R, int n,
                                        unsigned long long *__restrict__ counts) {
  int64_t lo[kRules], hi[kRules];
  bool on_key[kRules], integer[kRules];
#pragma unroll
  for (int r = 0; r < kRules; r++) {
    const bool live = r < n;
    lo[r] = live ? R[r].lo : 1;
    hi[r] = live ? R[r].hi : 0;
    on_key[r] = live && R[r].kind == kRuleRangeKey;
    integer[r] = live && R[r].kind == kRuleInteger;
  }
  uint32_t considered = 0, valid[kRules], cast_errors[kRules];  // (a workgroup sees fewer than 2^32 rows: side_rows_fit)
#pragma unroll
  for (int r = 0; r < kRules; r++) valid[r] = cast_errors[r] = 0;

  jb_for_rows_single(d, [&](int64_t v, bool ok) {
    considered += ok ? 1u : 0u;
    int64_t key = v;
    if (kKeys) key = f64_total_key(kFloat ? v : __double_as_longlong((double)v));  // (CAST AS DOUBLE: nearest-even)
    bool fits = true, whole = true;
    if (kInteger) {
      if (kFloat) {
        const double x = __longlong_as_double(v);
        fits = x > -2147483649.0 && x < 2147483648.0;
        const double back = (double)(int32_t)(fits ? x : 0.0);
        whole = __double_as_longlong(back) == v;  // (equal keys are equal bits: -0.0 comes back as +0.0)
      } else {
        fits = v >= -2147483648ll && v <= 2147483647ll;
      }
    }
#pragma unroll
    for (int r = 0; r < kRules; r++) {
      const int64_t k = (kFloat || on_key[r]) ? key : v;
      const bool pass = integer[r] ? (fits && whole) : (lo[r] <= k && k <= hi[r]);
      valid[r] += ok && pass ? 1u : 0u;
      if (kInteger) cast_errors[r] += ok && integer[r] && !fits ? 1u : 0u;
    }
  });

  const bool first = (threadIdx.x & 63) == 0;
  const uint32_t c = wave_sum(considered);
  if (first && c) atomicAdd(&counts[R[0].word + 2], (unsigned long long)c);  // (once per group: in its first rule's slot)
#pragma unroll
  for (int r = 0; r < kRules; r++) {
    const uint32_t a = wave_sum(valid[r]);
    const uint32_t e = kInteger ? wave_sum(cast_errors[r]) : 0u;
    if (first && r < n) {
      unsigned long long *out = counts + R[r].word;
      if (a) atomicAdd(&out[0], (unsigned long long)a);
      if (e) atomicAdd(&out[1], (unsigned long long)e);
    }
  }
}

template <int kRules>
__device__ __forceinline__ void vr_dispatch(const ComomentColDesc &d, const ValueRule *__restrict__ R, int n,
                                            unsigned long long *__restrict__ counts) {
  bool keys = false, integer = false;
  for (int r = 0; r < n; r++) {
    keys |= R[r].kind == kRuleRangeKey;
    integer |= R[r].kind == kRuleInteger;
  }
  if (d.x_is_float) {
    if (integer) vr_scan<kRules, true, true, true>(d, R, n, counts);
    else vr_scan<kRules, true, true, false>(d, R, n, counts);
  } else if (keys) {
    if (integer) vr_scan<kRules, false, true, true>(d, R, n, counts);
    else vr_scan<kRules, false, true, false>(d, R, n, counts);
  } else {
    if (integer) vr_scan<kRules, false, false, true>(d, R, n, counts);
    else vr_scan<kRules, false, false, false>(d, R, n, counts);
  }
}

}  // namespace

__global__ __launch_bounds__(kValueRuleBlock) void value_rule_kernel(const ValueRuleLaunch L) {
  const ComomentColDesc d = L.cols[blockIdx.y];
  const ValueRule *__restrict__ R = L.rules[blockIdx.y];
  const int n = L.n_rules[blockIdx.y];  // 1 .. kValueRulesPerGroup
  if (n <= 1) vr_dispatch<1>(d, R, n, L.counts);
  else if (n <= 2) vr_dispatch<2>(d, R, n, L.counts);
  else if (n <= 4) vr_dispatch<4>(d, R, n, L.counts);
  else vr_dispatch<8>(d, R, n, L.counts);
}

void launch_value_rule(const ValueRuleLaunch &L, int n_groups, int blocks_per_group, hipStream_t stream) {
  hipLaunchKernelGGL(value_rule_kernel, dim3(blocks_per_group, n_groups), dim3(kValueRuleBlock), 0, stream, L);
}

}  // namespace tgx
