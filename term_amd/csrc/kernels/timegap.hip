// timegap.hip -- TGX_CHECK_TIME_GAP on gfx950: the pieces around the sample sort (kernels/sortrank.hip) that answer
//   SELECT ts - LAG(ts) OVER ([PARTITION BY g] ORDER BY ts) ... WHERE ts IS NOT NULL
// of the reference's MaxTimeGap mode (TG/constraints/temporal_ordering.rs:454-481; include/tgx.h has the rules).
//
//   compact    per batch: the rows whose timestamp is non-NULL, as sort keys (v ^ 2^63: signed order -> unsigned order),
//              appended to the task's arrays.  Rows with a group go to the FRONT of the arrays (timestamp and group key
//              side by side), rows whose group is NULL to the BACK of the timestamp array (they are one partition of
//              their own and need no group key).
//   compose    grouped finalize: (RANK(g) - 1) << 32 | position in timestamp order -- sorted, these keys put every
//              partition's rows side by side and in timestamp order.
//   neighbours one pass over a sorted array: k[i] - k[i-1] (unsigned: it cannot wrap), compared with up to
//              kTimeGapThresholds thresholds, a running maximum; grouped, a gap is opened only where the high halves of
//              the neighbours' composed keys agree.  8 B (grouped: 16 B) read per row, per-lane 32-bit counters, reduced
//              within the wave by shuffles, one 64-bit vector atomic per wave and counter.
#include <hip/hip_runtime.h>

#include "timegap.h"

namespace tgx {

namespace {
typedef const int64_t __attribute__((address_space(1))) *global_i64_ptr;
typedef const uint8_t __attribute__((address_space(1))) *global_u8_ptr;

constexpr int kCompactRows = 8;

__device__ __forceinline__ uint32_t lanes_before(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
}  // namespace

// The placement is spearman_compact_kernel's: 2048 rows a trip, one global atomic per trip and list, the rows of a
// wave placed by ballot so that a store touches neighbouring slots.  count[0]: rows at the front, count[1]: at the back.
__global__ __launch_bounds__(256) void timegap_compact_kernel(TimeGapBatch d, uint64_t *kt, uint64_t *kg, uint64_t cap,
                                                               unsigned long long *count) {
  global_i64_ptr t = (global_i64_ptr)(uintptr_t)((const int64_t *)d.t + d.toff);
  global_i64_ptr g = (global_i64_ptr)(uintptr_t)(d.g ? (const int64_t *)d.g + d.goff : nullptr);
  global_u8_ptr tv = (global_u8_ptr)(uintptr_t)d.tv;
  global_u8_ptr gv = (global_u8_ptr)(uintptr_t)d.gv;
  __shared__ unsigned long long base_front, base_back;
  __shared__ uint32_t wave_front[4], wave_back[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int64_t kTrip = 256 * kCompactRows;
  const int64_t step = (int64_t)gridDim.x * kTrip;
  const int64_t rounded = (d.length + step - 1) / step * step;
  for (int64_t base = (int64_t)blockIdx.x * kTrip; base < rounded; base += step) {
    int64_t vt[kCompactRows], vg[kCompactRows];
    unsigned long long mf[kCompactRows], mb[kCompactRows];
    uint32_t front = 0, back = 0;
#pragma unroll
    for (int u = 0; u < kCompactRows; u++) {
      const int64_t i = base + u * 256 + threadIdx.x;
      const bool in = i < d.length;
      bool ok = in;
      if (ok && tv) ok = (tv[(d.toff + i) >> 3] >> ((d.toff + i) & 7)) & 1;
      bool grouped = true;  // (no group column: every row is of the one partition at the front)
      if (ok && gv) grouped = (gv[(d.goff + i) >> 3] >> ((d.goff + i) & 7)) & 1;
      vt[u] = in ? t[i] : 0;
      vg[u] = in && g ? g[i] : 0;
      mf[u] = __builtin_amdgcn_ballot_w64(ok && grouped);
      mb[u] = __builtin_amdgcn_ballot_w64(ok && !grouped);
      front += (uint32_t)__builtin_popcountll(mf[u]);
      back += (uint32_t)__builtin_popcountll(mb[u]);
    }
    if (lane == 0) {
      wave_front[wave] = front;
      wave_back[wave] = back;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t nf = wave_front[0] + wave_front[1] + wave_front[2] + wave_front[3];
      const uint32_t nb = wave_back[0] + wave_back[1] + wave_back[2] + wave_back[3];
      base_front = nf ? atomicAdd(&count[0], (unsigned long long)nf) : 0ull;
      base_back = nb ? atomicAdd(&count[1], (unsigned long long)nb) : 0ull;
    }
    __syncthreads();
    uint64_t off_f = base_front, off_b = base_back;
    for (uint32_t w = 0; w < wave; w++) {
      off_f += wave_front[w];
      off_b += wave_back[w];
    }
#pragma unroll
    for (int u = 0; u < kCompactRows; u++) {
      const uint64_t key = (uint64_t)vt[u] ^ 0x8000000000000000ULL;
      if ((mf[u] >> lane) & 1ull) {
        const uint64_t at = off_f + lanes_before(mf[u]);
        if (at < cap) {  // (the host sized the arrays for every row of the batch: never false)
          kt[at] = key;
          if (kg) kg[at] = (uint64_t)vg[u] ^ 0x8000000000000000ULL;
        }
      }
      if ((mb[u] >> lane) & 1ull) {
        const uint64_t at = off_b + lanes_before(mb[u]);
        if (at < cap) kt[cap - 1 - at] = key;
      }
      off_f += (uint32_t)__builtin_popcountll(mf[u]);
      off_b += (uint32_t)__builtin_popcountll(mb[u]);
    }
    __syncthreads();
  }
}

// ranks[i] = RANK() of the group key at position i of the timestamp order (1-based, below 2^32) -> the composed key,
// written where the rank stood
__global__ __launch_bounds__(256) void timegap_compose_kernel(uint64_t *ranks, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    ranks[i] = ((ranks[i] - 1ull) << 32) | i;
}

// out[0] += gaps, out[1] = max(out[1], largest gap), out[2 + k] += gaps above threshold k
template <bool GROUPED>
__global__ __launch_bounds__(256) void timegap_neighbours_kernel(const uint64_t *__restrict__ vals,
                                                                  const uint64_t *__restrict__ tags, uint64_t n,
                                                                  TimeGapThresholds T, unsigned long long *out) {
  uint32_t gaps = 0, over[kTimeGapThresholds];  // (fewer than 2^32 rows: timegap_device.cpp)
#pragma unroll
  for (int k = 0; k < kTimeGapThresholds; k++) over[k] = 0;
  unsigned long long largest = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t cur = __builtin_nontemporal_load(vals + i), prev = vals[i - 1];  // (the neighbour's line is in cache)
    bool open = true;
    if (GROUPED) open = (__builtin_nontemporal_load(tags + i) >> 32) == (tags[i - 1] >> 32);
    const uint64_t gap = cur - prev;  // sorted: cur >= prev as unsigned numbers
    gaps += open ? 1u : 0u;
    if (open && gap > largest) largest = gap;
#pragma unroll
    for (int k = 0; k < kTimeGapThresholds; k++) {
      const int64_t mg = T.max_gap[k];  // a negative threshold: every gap is above it
      over[k] += open && k < T.n && (mg < 0 || gap > (uint64_t)mg) ? 1u : 0u;
    }
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    gaps += __shfl_down(gaps, dlt, 64);
    const unsigned long long other = __shfl_down(largest, dlt, 64);
    largest = other > largest ? other : largest;
#pragma unroll
    for (int k = 0; k < kTimeGapThresholds; k++) over[k] += __shfl_down(over[k], dlt, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (gaps) atomicAdd(&out[0], (unsigned long long)gaps);
    if (largest) atomicMax(&out[1], largest);
#pragma unroll
    for (int k = 0; k < kTimeGapThresholds; k++)
      if (over[k]) atomicAdd(&out[2 + k], (unsigned long long)over[k]);
  }
}

static unsigned grid_for(uint64_t n, uint64_t per_block) {
  const uint64_t want = (n + per_block - 1) / per_block;
  const uint64_t most = (uint64_t)1024 * 8;
  return (unsigned)(want < 1 ? 1 : (want > most ? most : want));
}

void launch_timegap_compact(const TimeGapBatch &d, uint64_t *kt, uint64_t *kg, uint64_t cap, unsigned long long *count,
                            hipStream_t stream) {
  if (d.length <= 0) return;
  hipLaunchKernelGGL(timegap_compact_kernel, dim3(grid_for((uint64_t)d.length, 256 * kCompactRows)), dim3(256), 0, stream,
                     d, kt, kg, cap, count);
}

void launch_timegap_compose(uint64_t *ranks, uint64_t n, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(timegap_compose_kernel, dim3(grid_for(n, 256 * 8)), dim3(256), 0, stream, ranks, n);
}

void launch_timegap_neighbours(const uint64_t *vals, const uint64_t *tags, uint64_t n, const TimeGapThresholds &T,
                               unsigned long long *out, hipStream_t stream) {
  if (n < 2) return;
  if (tags)
    hipLaunchKernelGGL(timegap_neighbours_kernel<true>, dim3(grid_for(n, 256 * 8)), dim3(256), 0, stream, vals, tags, n, T,
                       out);
  else
    hipLaunchKernelGGL(timegap_neighbours_kernel<false>, dim3(grid_for(n, 256 * 8)), dim3(256), 0, stream, vals, tags, n,
                       T, out);
}

}  // namespace tgx
