// pivot_search.h -- the last resort of the pivot kernels (scan.hip scan_pivot_kernel, comoments.hip
// como_pivot_kernel): when neither look at a batch met a valid, finite value, the first such row of the batch.
//
// The search is spread over the launch's grid: grid = (blocks, columns), workgroup b of a column takes its own stretch
// of about kPivotSearchRows rows, walks it in order and offers the first row it finds to the column's PivotSearch slot
// (an atomic max of ~row: the smallest row wins, whatever the order the workgroups ran in).  A second, one-workgroup-
// per-column kernel then turns the winning row into the pivot and clears the slot.  Workgroups read the validity
// bitmap 64 rows a lane, so an all-NULL batch costs one parallel read of its bitmap.  A workgroup other than the first
// returns at once when the column's pivot is set, or when one of the rows the first look reads is valid and finite
// (the look then sets the pivot): a batch with data costs each of them a row or two, and no atomic.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_types.h"

namespace tgx {

// 64 validity bits from bit `b` on (bit k of the result = bit b + k of the bitmap); bytes at or past `end_byte` read
// as 0.  nullptr: no bitmap, every row valid.
__device__ __forceinline__ uint64_t validity_bits64(const uint8_t *v, int64_t b, int64_t end_byte) {
  if (!v) return ~0ull;
  const int64_t byte0 = b >> 3;
  uint64_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 8; k++)
    if (byte0 + k < end_byte) lo |= (uint64_t)v[byte0 + k] << (8 * k);
  if (byte0 + 8 < end_byte) hi = v[byte0 + 8];
  const int s = (int)(b & 7);
  return s ? (lo >> s) | (hi << (64 - s)) : lo;
}

// workgroups of a pivot launch: enough for kPivotSearchRows rows each of the longest column (or pair)
inline int pivot_search_blocks(int64_t max_length) {
  const int64_t b = (max_length + kPivotSearchRows - 1) / kPivotSearchRows;
  return (int)(b < 1 ? 1 : b > kPivotSearchBlocks ? kPivotSearchBlocks : b);
}

// this workgroup's stretch [*lo, *hi) of a column of n rows (multiples of 64 rows; empty past the end)
__device__ __forceinline__ void pivot_search_stretch(int64_t n, int64_t *lo, int64_t *hi) {
  const int64_t per = (((n + gridDim.x - 1) / gridDim.x) + 63) & ~(int64_t)63;
  *lo = (int64_t)blockIdx.x * per;
  *hi = *lo + per < n ? *lo + per : n;
}

// The first row i of [lo, hi) whose bit in valid64(r) (rows r .. r + 63) is set and for which finite(i) holds, or -1.
// Called by all 256 threads of the workgroup; rows are taken 256 x 64 a round, in order, and the first round that
// holds such a row ends the walk.  A lane tests the values of its set bits eight at a time (independent loads).
template <class Valid64, class Finite>
__device__ int64_t first_valid_finite_row(int64_t lo, int64_t hi, Valid64 valid64, Finite finite) {
  __shared__ unsigned long long s_first;
  for (int64_t base = lo; base < hi; base += 256 * 64) {
    if (threadIdx.x == 0) s_first = ~0ull;
    __syncthreads();
    const int64_t r = base + (int64_t)threadIdx.x * 64;
    if (r < hi) {
      uint64_t w = valid64(r);
      if (hi - r < 64) w &= (1ull << (hi - r)) - 1;
      int64_t found = -1;
      for (int j0 = 0; j0 < 64 && found < 0; j0 += 8) {
        const uint32_t byte = (uint32_t)(w >> j0) & 0xffu;
        if (!byte) continue;
        bool ok[8];
#pragma unroll
        for (int u = 0; u < 8; u++) ok[u] = ((byte >> u) & 1u) && finite(r + j0 + u);
#pragma unroll
        for (int u = 7; u >= 0; u--)
          if (ok[u]) found = r + j0 + u;
      }
      if (found >= 0) atomicMin(&s_first, (unsigned long long)found);
    }
    __syncthreads();
    const unsigned long long f = s_first;
    __syncthreads();  // (s_first is reset by the next round)
    if (f != ~0ull) return (int64_t)f;
  }
  return -1;
}

// Offers this workgroup's first row (none: row < 0) to the column's slot; the smallest row of the launch wins.
__device__ __forceinline__ void pivot_search_offer(PivotSearch *ps, int64_t row) {
  if (threadIdx.x == 0 && row >= 0) atomicMax(&ps->best, ~(unsigned long long)row);
}

}  // namespace tgx
