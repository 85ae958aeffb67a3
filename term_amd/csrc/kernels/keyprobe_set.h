// keyprobe_set.h -- the lookup in a key probe's set of 128-bit fingerprints (routes 5 and 6), which the probe of string
// keys (keyprobe_strings.hip) and the probe of tuple keys (keyprobe_tuples.hip) share: one table layout, one way to find.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "keyset_device.h"

namespace tgx {

// the slot of (fa, fb) in the set's table, or -1: it is not in the set.  (Routes 5 and 6)
template <class Set>
__device__ __forceinline__ int64_t kps_find(const Set &s, unsigned long long fa, unsigned long long fb) {
  if (!s.slots) return -1;
  const ulonglong2 *slots = (const ulonglong2 *)s.slots;
  uint64_t h = fa & s.mask;
  for (uint64_t p = 0; p <= s.mask; p++) {
    const ulonglong2 e = slots[h];  // (one 16-byte load: both words)
    if (e.x == fa && e.y == fb) return (int64_t)h;
    if (e.x == kEmptyKey) return -1;
    h = (h + 1) & s.mask;
  }
  return -1;
}

// how often the value of slot `at` occurs in the parent: a plain set does not say
__device__ __forceinline__ unsigned long long kps_times(const KeyProbeStringSet &, int64_t) { return 1; }
__device__ __forceinline__ unsigned long long kps_times(const KeyProbeCountedStringSet &s, int64_t at) {
  return s.counts[at];
}
template <class Set>
struct KpsCounted {
  static constexpr bool value = false;
};
template <>
struct KpsCounted<KeyProbeCountedStringSet> {
  static constexpr bool value = true;
};

}  // namespace tgx
