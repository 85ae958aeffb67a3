// keyset_device.h -- device helpers shared by the kernels of the exact key sets (distinct.hip, partition.hip,
// distinct128.hip): the key mixer, the table insert of 64-bit keys, the block reductions into the counters, the
// validity-bit test, the row stamp of the exact lists' records, and the grid of the grid-stride kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "distinct_types.h"

namespace tgx {

typedef const uint8_t __attribute__((address_space(1))) *global_u8_ptr;
typedef const uint64_t __attribute__((address_space(1))) *global_u64_ptr;
typedef const int32_t __attribute__((address_space(1))) *global_i32_ptr;
typedef const int64_t __attribute__((address_space(1))) *global_i64_ptr;

// workgroups of 256 threads of a grid-stride kernel over `items`
static inline int grid_for(uint64_t items) {
  uint64_t blocks = (items + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 256 * 8) blocks = 256 * 8;
  return (int)blocks;
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ULL;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebULL;
  x ^= x >> 31;
  return x;
}

// Bit `slot` of an Arrow validity bitmap (an int, 0 or 1).  A macro, not a function: behind a function the compiler
// settles on a 32-bit shift before it inlines and the callers lose the 16-bit one they compile to when the expression is
// written out in place.  `slot` is evaluated twice: pass an expression without side effects.
#define TGX_VALID_BIT(vbits, slot) (((vbits)[(slot) >> 3] >> ((slot) & 7)) & 1)

// Two per-thread counts summed over the workgroup and added to two counters: one atomicAdd per block and counter, and
// none for a sum of zero (a caller with one count passes 0 and &counters[kCntSpare], which is therefore never written).
// _any: workgroups of up to 16 waves (256 bytes of LDS, a loop over the waves there are);
// _4waves: workgroups of exactly 256 threads (64 bytes, no loop).
__device__ __forceinline__ void block_add2_any(unsigned long long a, unsigned long long b,
                                               unsigned long long *ga, unsigned long long *gb) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a += __shfl_down(a, d, 64);
    b += __shfl_down(b, d, 64);
  }
  __shared__ unsigned long long sa[16], sb[16];
  const int wave = threadIdx.x >> 6;
  const int n_waves = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) {
    sa[wave] = a;
    sb[wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long ta = 0, tb = 0;
    for (int w = 0; w < n_waves; w++) {
      ta += sa[w];
      tb += sb[w];
    }
    if (ta) atomicAdd(ga, ta);
    if (tb) atomicAdd(gb, tb);
  }
}

__device__ __forceinline__ void block_add2_4waves(unsigned long long a, unsigned long long b,
                                                  unsigned long long *ga, unsigned long long *gb) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    a += __shfl_down(a, d, 64);
    b += __shfl_down(b, d, 64);
  }
  __shared__ unsigned long long sa[4], sb[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sa[wave] = a;
    sb[wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long ta = sa[0] + sa[1] + sa[2] + sa[3], tb = sb[0] + sb[1] + sb[2] + sb[3];
    if (ta) atomicAdd(ga, ta);
    if (tb) atomicAdd(gb, tb);
  }
}

// returns 1 if the key was new; *became_dup = 1 if this insert is the key's second sighting
__device__ __forceinline__ int hash_insert(const HashSetView &t, uint64_t key, int want_mult,
                                           int weight_two, int *became_dup) {
  uint64_t h = mix64(key) & t.mask;
  for (;;) {
    unsigned long long old =
        atomicCAS((unsigned long long *)&t.keys[h], (unsigned long long)kEmptyKey,
                  (unsigned long long)key);
    if (old == kEmptyKey) {
      if (want_mult && weight_two) {
        // another thread that found this key may already have set the bit: count it once
        const uint32_t bit = 1u << (h & 31);
        uint32_t prev = atomicOr(&t.dup[h >> 5], bit);
        *became_dup = (prev & bit) ? 0 : 1;
      }
      return 1;
    }
    if (old == key) {
      if (want_mult) {
        const uint32_t bit = 1u << (h & 31);
        // plain read first: most duplicates of a hot key find the bit already set
        if (!(__hip_atomic_load(&t.dup[h >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) {
          uint32_t prev = atomicOr(&t.dup[h >> 5], bit);
          *became_dup = (prev & bit) ? 0 : 1;
        }
      }
      return 0;
    }
    h = (h + 1) & t.mask;
  }
}

// A record of an EXACT set's lists keeps the high half of its second fingerprint word and carries its ROW in the low
// half (equal fingerprints are settled on the rows' bytes); the low half waits in fb_lo[row], from where
// stamped_second_word() restores the fingerprint once the batch has been released (fp_demote_kernel).
__device__ __forceinline__ void stamp_row(ulonglong2 &r, uint32_t *fb_lo, int64_t row) {
  fb_lo[row] = (uint32_t)r.y;
  r.y = (r.y & 0xFFFFFFFF00000000ull) | (uint64_t)(uint32_t)row;
}
__device__ __forceinline__ uint64_t stamped_second_word(const ulonglong2 &r, const uint32_t *fb_lo) {
  return (r.y & 0xFFFFFFFF00000000ull) | (uint64_t)fb_lo[(uint32_t)r.y];
}

}  // namespace tgx
