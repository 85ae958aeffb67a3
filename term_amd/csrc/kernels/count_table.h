// count_table.h -- the open-addressing table primitive of the bounded GROUP BY kernels (valuecounts.hip, paircounts.hip):
// a slot is claimed by CAS on its key word; a 128-bit key (two fingerprint words) claims the first word by CAS and then
// settles the second by CAS: the slot is the key's when both come back free or equal, otherwise probing goes on.  Used in
// LDS per workgroup with 32-bit counts (a workgroup sees fewer than 2^32 rows: side_rows_fit) and in global memory per
// task with 64-bit counts.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "distinct_types.h"
#include "keyset_device.h"

namespace tgx {

__device__ __forceinline__ unsigned long long vc_peek(const unsigned long long *word) {
  return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// probes from slot `h` for `key`: the slot that holds it, claimed if need be, or -1 when `probes` slots held other keys
template <class Slot>
__device__ __forceinline__ int64_t vc_claim(unsigned long long *keys, Slot mask, Slot h, unsigned long long key,
                                            uint32_t probes) {
  for (uint32_t p = 0; p < probes; p++) {
    // (a key word never changes once it is set: a plain look spares the hot keys their CAS)
    unsigned long long old = vc_peek(&keys[h]);
    if (old == kEmptyKey) old = atomicCAS(&keys[h], (unsigned long long)kEmptyKey, key);
    if (old == kEmptyKey || old == key) return (int64_t)h;
    h = (h + 1) & mask;
  }
  return -1;
}

// the same for a 128-bit key (fa, fb) whose words lie in ka / kb, probing from slot `h`; *made: this lane made the entry
// (it owes the slot whatever lies behind the key: a row, the value's bytes)
template <class Slot>
__device__ __forceinline__ int64_t vc_claim128(unsigned long long *ka, unsigned long long *kb, Slot mask, Slot h,
                                               unsigned long long fa, unsigned long long fb, uint32_t probes,
                                               bool *made) {
  *made = false;
  for (uint32_t p = 0; p < probes; p++) {
    unsigned long long a = vc_peek(&ka[h]);
    if (a == kEmptyKey) a = atomicCAS(&ka[h], (unsigned long long)kEmptyKey, fa);
    if (a == kEmptyKey || a == fa) {
      unsigned long long b = vc_peek(&kb[h]);
      *made = b == kEmptyKey && (b = atomicCAS(&kb[h], (unsigned long long)kEmptyKey, fb)) == kEmptyKey;
      if (*made || b == fb) return (int64_t)h;
    }
    h = (h + 1) & mask;
  }
  return -1;
}

// Where a wave's lanes hold 64 consecutive rows (lane l: row `row`, `in`: the row exists), the validity of another
// column for the wave as one 64-bit window of its bitmap, whatever its Arrow offset: bit l is set when the row is
// non-NULL there.  A column without a bitmap: every row that exists.  (One byte load a lane, eight lanes a byte; what
// a key's lanes `same` count of the column is then popcount(same & window).)
__device__ __forceinline__ unsigned long long vc_valid_window(const uint8_t *validity, int64_t offset, int64_t row,
                                                              bool in) {
  typedef const uint8_t __attribute__((address_space(1))) *u8_ptr;
  u8_ptr v = (u8_ptr)(uintptr_t)validity;
  const int64_t bit = offset + row;
  return __ballot(in && (v == nullptr || ((v[bit >> 3] >> (bit & 7)) & 1) != 0));
}

// the workgroup's table of 128-bit keys: the two fingerprint words, a 32-bit count and a row that holds the key's value
struct VcLdsStrings {
  unsigned long long fa[kValueCountsStrLdsSlots], fb[kValueCountsStrLdsSlots], row[kValueCountsStrLdsSlots];
  unsigned int count[kValueCountsStrLdsSlots];
};
// false: the slots around the key's place hold other keys
__device__ __forceinline__ bool vc_insert_lds128(VcLdsStrings &l, unsigned long long fa, unsigned long long fb,
                                                 uint32_t weight, unsigned long long row) {
  uint32_t h = (uint32_t)fa & (kValueCountsStrLdsSlots - 1);
  for (uint32_t probe = 0; probe < kValueCountsLdsProbes; probe++) {
    unsigned long long a = vc_peek(&l.fa[h]);
    if (a == kEmptyKey) a = atomicCAS(&l.fa[h], (unsigned long long)kEmptyKey, fa);
    if (a == kEmptyKey || a == fa) {
      unsigned long long b = vc_peek(&l.fb[h]);
      const bool made = b == kEmptyKey && (b = atomicCAS(&l.fb[h], (unsigned long long)kEmptyKey, fb)) == kEmptyKey;
      if (made) l.row[h] = row;  // (read after the workgroup's barrier)
      if (made || b == fb) {
        atomicAdd(&l.count[h], weight);
        return true;
      }
    }
    h = (h + 1) & (kValueCountsStrLdsSlots - 1);
  }
  return false;
}

// where the value of slot `slot` of a string column lies (the three layouts: int32 offsets, int64 offsets, views)
__device__ __forceinline__ void utf8_value_of(const Utf8ColDesc &d, int64_t slot, uintptr_t *p, uint64_t *len) {
  if (d.views) {
    global_i32_ptr vw = (global_i32_ptr)((uintptr_t)d.views + (uintptr_t)slot * 16);
    const int32_t n = vw[0];
    *len = (uint64_t)(uint32_t)n;
    if (n <= 12) *p = (uintptr_t)d.views + (uintptr_t)slot * 16 + 4;
    else *p = (uintptr_t)d.buffers[vw[2]] + (uintptr_t)(uint32_t)vw[3];
  } else if (d.large_offsets) {
    global_i64_ptr off = (global_i64_ptr)(uintptr_t)d.offsets;
    const int64_t b = off[slot];
    *p = (uintptr_t)d.data + (uintptr_t)b;
    *len = (uint64_t)(off[slot + 1] - b);
  } else {
    global_i32_ptr off = (global_i32_ptr)(uintptr_t)d.offsets;
    const int32_t b = off[slot];
    *p = (uintptr_t)d.data + (uintptr_t)b;
    *len = (uint64_t)(off[slot + 1] - b);
  }
}

__device__ __forceinline__ unsigned long long vc_shfl64(unsigned long long v, int lane) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), lane, 64);
  return ((unsigned long long)hi << 32) | lo;
}

// ---- what the kinds that count string keys share (valuecounts.hip, keyprobe_strings.hip) ---------------------------------
// a string key (fa, fb) whose bytes are [p, p + len), with its weight, into a task's global table; a probe sequence
// that runs out adds the weight to *overflow
__device__ __forceinline__ void vc_insert_global128(const ValueCountsTable &t, unsigned long long fa,
                                                    unsigned long long fb, unsigned long long weight, uintptr_t p,
                                                    uint32_t len, unsigned long long *overflow) {
  uint64_t h = fa & t.mask;
  for (uint32_t probe = 0; probe < kValueCountsProbes; probe++) {
    unsigned long long a = vc_peek(&t.keys[h]);
    if (a == kEmptyKey) a = atomicCAS(&t.keys[h], (unsigned long long)kEmptyKey, fa);
    if (a == kEmptyKey || a == fa) {
      unsigned long long b = vc_peek(&t.keys2[h]);
      const bool made = b == kEmptyKey && (b = atomicCAS(&t.keys2[h], (unsigned long long)kEmptyKey, fb)) == kEmptyKey;
      if (made) {  // this lane made the entry: its bytes go to the slot's place in the store
        global_u8_ptr src = (global_u8_ptr)p;
        uint8_t *dst = t.store + h * (uint64_t)t.max_value_bytes;
        for (uint32_t i = 0; i < len; i++) dst[i] = src[i];
        t.lens[h] = len;
      }
      if (made || b == fb) {
        atomicAdd(&t.counts[h], weight);
        return;
      }
    }
    h = (h + 1) & t.mask;
  }
  atomicAdd(overflow, weight);
}

// Equal fingerprints combined within the wave, in up to four rounds: a round's leader (the first lane that is still
// pending) calls insert(weight) with the number of lanes that hold its key; whoever is pending after the rounds calls
// insert(1) for itself.  Every lane of the wave takes part (`live`: the lane has a key).
template <class Insert>
__device__ __forceinline__ void vc_wave_combine128(bool live, unsigned long long fa, unsigned long long fb, int lane,
                                                   Insert insert) {
  unsigned long long todo = __ballot(live);
  bool pending = live;
  for (int round = 0; round < 4 && todo != 0; round++) {
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned long long la = vc_shfl64(fa, leader), lb = vc_shfl64(fb, leader);
    const bool mine = pending && fa == la && fb == lb;
    const unsigned long long same = __ballot(mine);
    if (lane == leader) insert((uint32_t)__popcll(same));
    pending = pending && !mine;
    todo &= ~same;
  }
  if (pending) insert(1u);
}

}  // namespace tgx
