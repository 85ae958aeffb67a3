// row_walk.h -- the row walkers of the streaming check kernels (jointbins.hip, temporal.hip): every row of a window of
// 8-byte values once, one row per lane per load, row pairs as one 16-byte non-temporal load per column where the
// addresses allow, four loads in flight per column per lane, validity bits read per pair where the Arrow offset is even.
// (comoments.hip keeps its own walker: it carries the pivots and the block partials through the loop.)
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"

namespace tgx {

typedef const int64_t __attribute__((address_space(1))) *jb_i64_ptr;
typedef const uint8_t __attribute__((address_space(1))) *jb_u8_ptr;

__device__ __forceinline__ bool jb_valid(jb_u8_ptr v, int64_t bit) {
  return v == nullptr ? true : ((v[bit >> 3] >> (bit & 7)) & 1) != 0;
}

// every row of the window once: fold(x bits, y bits, row is in the window and non-NULL on every side that is read).
// kPair = false reads d.x / d.xv / d.xoff only (8 B + 1 bit per row); y bits are 0 there.
template <bool kPair, class Fold>
__device__ __forceinline__ void jb_walk_rows(const ComomentColDesc &d, Fold fold) {
  jb_i64_ptr x = (jb_i64_ptr)(uintptr_t)((const int64_t *)d.x + d.xoff);
  jb_i64_ptr y = (jb_i64_ptr)(uintptr_t)((const int64_t *)d.y + d.yoff);
  jb_u8_ptr xv = (jb_u8_ptr)(uintptr_t)d.xv;
  jb_u8_ptr yv = (jb_u8_ptr)(uintptr_t)d.yv;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool wide = ((((uintptr_t)((const int64_t *)d.x + d.xoff)) |
                      (kPair ? (uintptr_t)((const int64_t *)d.y + d.yoff) : (uintptr_t)0)) & 15) == 0;
  int64_t done = 0;  // rows [0, done) are handled by the wide path
  if (wide) {
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    typedef const i64x2 __attribute__((address_space(1))) *jb_i64x2_ptr;
    jb_i64x2_ptr x2 = (jb_i64x2_ptr)x, y2 = (jb_i64x2_ptr)y;
    const int64_t n_pairs = d.length >> 1;
    done = 2 * n_pairs;
    const bool x_even = (d.xoff & 1) == 0, y_even = (d.yoff & 1) == 0;
    for (int64_t p0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p0 < n_pairs; p0 += 4 * stride) {
      i64x2 xq[4], yq[4];
      bool ok[8];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int64_t p = p0 + u * stride;
        const bool in = p < n_pairs;
        const int64_t q = in ? p : 0;
        uint32_t xb2 = 3, yb2 = 3;  // both rows of a pair share a validity byte when the Arrow offset is even
        if (xv) {
          const int64_t b = d.xoff + 2 * q;
          xb2 = x_even ? ((uint32_t)xv[b >> 3] >> (b & 7)) & 3u
                       : (uint32_t)jb_valid(xv, b) | ((uint32_t)jb_valid(xv, b + 1) << 1);
        }
        if (kPair && yv) {
          const int64_t b = d.yoff + 2 * q;
          yb2 = y_even ? ((uint32_t)yv[b >> 3] >> (b & 7)) & 3u
                       : (uint32_t)jb_valid(yv, b) | ((uint32_t)jb_valid(yv, b + 1) << 1);
        }
        ok[2 * u] = in && (xb2 & yb2 & 1u);
        ok[2 * u + 1] = in && ((xb2 & yb2) >> 1);
        xq[u] = __builtin_nontemporal_load(x2 + q);
        if (kPair) yq[u] = __builtin_nontemporal_load(y2 + q);
        else yq[u] = i64x2{0, 0};
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        fold(xq[u].x, yq[u].x, ok[2 * u]);
        fold(xq[u].y, yq[u].y, ok[2 * u + 1]);
      }
    }
  }
  for (int64_t i0 = done + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < d.length; i0 += 4 * stride) {
    int64_t xb[4], yb[4];
    bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t i = i0 + u * stride;
      const bool in = i < d.length;
      xb[u] = in ? x[i] : 0;
      yb[u] = kPair && in ? y[i] : 0;
      ok[u] = in && jb_valid(xv, d.xoff + (in ? i : 0)) && (!kPair || jb_valid(yv, d.yoff + (in ? i : 0)));
    }
#pragma unroll
    for (int u = 0; u < 4; u++) fold(xb[u], yb[u], ok[u]);
  }
}

// the pair form: fold(x bits, y bits, both sides non-NULL)
template <class Fold>
__device__ __forceinline__ void jb_for_rows(const ComomentColDesc &d, Fold fold) {
  jb_walk_rows<true>(d, fold);
}

// the single-column form: fold(value bits, row is in the window and non-NULL)
template <class Fold>
__device__ __forceinline__ void jb_for_rows_single(const ComomentColDesc &d, Fold fold) {
  jb_walk_rows<false>(d, [&](int64_t xb, int64_t, bool ok) { fold(xb, ok); });
}

}  // namespace tgx
