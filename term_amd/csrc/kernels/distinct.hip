// distinct.hip -- exact COUNT(DISTINCT col) and GROUP BY col multiplicity for gfx950.
//
//   COUNT(DISTINCT c)                                   TG/constraints/uniqueness.rs:612-617
//   SUM(CASE WHEN cnt = 1 ...) over GROUP BY c          TG/constraints/uniqueness.rs:671-681
//
// Keys are 64-bit patterns (Int64 values; Float64 by bit pattern, as DataFusion hashes floats).
// Two device-resident set representations, chosen per column by the host from the running
// MIN/MAX of the column (tgx_api.cpp):
//   * range bitmap: 1 bit per value of [base, base + range) (+1 "seen twice" bit when multiplicity
//     is wanted).  global atomicOr per row; the bit's previous value says whether the key is new.
//     (Big batches populate it through the range-partition pass instead: partition.hip.)
//   * open-addressing hash set (linear probing, 64-bit atomicCAS claim), capacity 2^k >= 2 x keys;
//     the all-ones pattern doubles as EMPTY and is tracked by a side counter.
// Device-scope atomics execute at the memory side, so inserts from all 8 XCDs are coherent
// (MI355X_MICROARCH.md "Global float atomics" / SURVEY.md section 7 notes).  Counters are
// block-reduced first: one atomicAdd per block, not per row.
// Also here: the cross-rank export / rebase / adopt kernels and the key lists of big sparse batches (key_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdlib.h>

#include "device_types.h"
#include "distinct_types.h"
#include "keyset_device.h"
#include "lists.h"

namespace tgx {

// One row per lane, grid-stride.  counters: [0] distinct, [1] keys seen at least twice,
// [2] rows whose key is the all-ones pattern (EMPTY stand-in), [3] non-null rows.
__global__ __launch_bounds__(256) void distinct_hash_kernel(DistinctColDesc d, HashSetView t,
                                                             unsigned long long *counters) {
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)d.values + d.offset);
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  unsigned long long n_new = 0, n_dup = 0, n_empty = 0, n_valid = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.length; i += stride) {
    bool valid = true;
    if (vbits) {
      const int64_t b = d.offset + i;
      valid = TGX_VALID_BIT(vbits, b);
    }
    if (!valid) continue;
    n_valid++;
    uint64_t key = (uint64_t)vals[i];
    if (key == kEmptyKey) {
      n_empty++;
      continue;
    }
    int became_dup = 0;
    n_new += hash_insert(t, key, d.want_multiplicity, 0, &became_dup);
    n_dup += became_dup;
  }
  block_add2_any(n_new, n_dup, &counters[kCntDistinct], &counters[kCntTwice]);
  __syncthreads();
  block_add2_any(n_empty, n_valid, &counters[kCntEmptyRows], &counters[kCntValidRows]);
}

// Range bitmap: bit (key - base) of `seen`; `twice` marks keys seen again.
__global__ __launch_bounds__(256) void distinct_bitmap_kernel(DistinctColDesc d, BitmapView bm,
                                                               unsigned long long *counters) {
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)d.values + d.offset);
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  unsigned long long n_new = 0, n_dup = 0, n_out = 0, n_valid = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.length; i += stride) {
    bool valid = true;
    if (vbits) {
      const int64_t b = d.offset + i;
      valid = TGX_VALID_BIT(vbits, b);
    }
    if (!valid) continue;
    n_valid++;
    uint64_t rel = (uint64_t)vals[i] - (uint64_t)bm.base;  // wraps for keys below base
    if (rel >= bm.range) {
      n_out++;  // host guarantees this cannot happen; counted so a violation is detected
      continue;
    }
    const uint32_t bit = 1u << (rel & 31);
    uint32_t prev = atomicOr(&bm.seen[rel >> 5], bit);
    if (!(prev & bit)) {
      n_new++;
    } else if (d.want_multiplicity) {
      uint32_t p2 = atomicOr(&bm.twice[rel >> 5], bit);
      if (!(p2 & bit)) n_dup++;
    }
  }
  block_add2_any(n_new, n_dup, &counters[kCntDistinct], &counters[kCntTwice]);
  __syncthreads();
  block_add2_any(n_out, n_valid, &counters[kCntOutOfRange], &counters[kCntValidRows]);
}

// A strided sample of the column (at most 2^16 rows, evenly spread): where its keys lie, before anything has read
// it.  The DISTINCT pass lays its range bitmap out from this estimate (with slack) and takes the column's range
// aggregates along; keys that fall outside after all are counted and repaired later (tgx_api.cpp, distinct_resolve).
__global__ __launch_bounds__(256) void distinct_sample_kernel(DistinctColDesc d, DistinctSample *out) {
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)d.values + d.offset);
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  // d.pad != 0: every row (the exact MIN / MAX of a coalesced flush of DEVICE windows), not a sample
  const int64_t want = (d.pad || d.length < 65536) ? d.length : 65536;
  const int64_t step = d.length / want;
  int64_t mn = INT64_MAX, mx = INT64_MIN;
  unsigned long long cnt = 0;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < want; k += (int64_t)gridDim.x * 256) {
    const int64_t i = k * step + ((k * 40503) & 15 ? 0 : (step > 1 ? step / 2 : 0));  // (not a pure stride)
    bool valid = true;
    if (vbits) {
      const int64_t b = d.offset + i;
      valid = TGX_VALID_BIT(vbits, b);
    }
    if (!valid) continue;
    const int64_t v = vals[i];
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
    cnt++;
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    const int64_t omn = __shfl_down(mn, dlt, 64), omx = __shfl_down(mx, dlt, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    cnt += __shfl_down(cnt, dlt, 64);
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicMin((long long *)&out->min_v, (long long)mn);
    atomicMax((long long *)&out->max_v, (long long)mx);
    atomicAdd(&out->count, cnt);
  }
}

// The repair of a speculated range: the batch's keys OUTSIDE [base, base + range) -- never inserted into the bitmap
// -- go into the hash set (the bitmap's keys have been moved there first).  Row counters are not touched.
__global__ __launch_bounds__(256) void distinct_outlier_kernel(DistinctColDesc d, int64_t base, uint64_t range,
                                                                HashSetView t, unsigned long long *counters) {
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)d.values + d.offset);
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  unsigned long long n_new = 0, n_dup = 0, n_empty = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.length; i += stride) {
    bool valid = true;
    if (vbits) {
      const int64_t b = d.offset + i;
      valid = TGX_VALID_BIT(vbits, b);
    }
    if (!valid) continue;
    const uint64_t key = (uint64_t)vals[i];
    if (key - (uint64_t)base < range) continue;  // the bitmap had it
    if (key == kEmptyKey) {
      n_empty++;
      continue;
    }
    int became_dup = 0;
    n_new += hash_insert(t, key, d.want_multiplicity, 0, &became_dup);
    n_dup += became_dup;
  }
  block_add2_any(n_new, n_dup, &counters[kCntDistinct], &counters[kCntTwice]);
  __syncthreads();
  block_add2_any(n_empty, 0ull, &counters[kCntEmptyRows], &counters[kCntSpare]);
}

// Re-inserts every key of `src` into `dst` (growth, merge, bitmap -> hash conversion).
__global__ __launch_bounds__(256) void hash_rehash_kernel(HashSetView src, HashSetView dst,
                                                           int want_mult,
                                                           unsigned long long *counters) {
  unsigned long long n_new = 0, n_dup = 0;
  const uint64_t cap = src.mask + 1;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap;
       s += (uint64_t)gridDim.x * blockDim.x) {
    uint64_t key = src.keys[s];
    if (key == kEmptyKey) continue;
    int two = want_mult ? ((src.dup[s >> 5] >> (s & 31)) & 1) : 0;
    int became_dup = 0;
    // (a key present on both sides and already a duplicate on the source side: hash_insert has set the bit or found it
    //  set, and became_dup tells which)
    n_new += hash_insert(dst, key, want_mult, two, &became_dup);
    n_dup += became_dup;
  }
  block_add2_any(n_new, n_dup, &counters[kCntDistinct], &counters[kCntTwice]);
}

__global__ __launch_bounds__(256) void bitmap_to_hash_kernel(BitmapView bm, HashSetView dst,
                                                              int want_mult,
                                                              unsigned long long *counters) {
  unsigned long long n_new = 0, n_dup = 0, n_empty = 0;
  const uint64_t words = (bm.range + 31) >> 5;
  for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words;
       w += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t seen = bm.seen[w];
    uint32_t twice = want_mult ? bm.twice[w] : 0;
    while (seen) {
      int b = __builtin_ctz(seen);
      seen &= seen - 1;
      uint64_t key = (uint64_t)bm.base + (w << 5) + (uint64_t)b;
      if (key == kEmptyKey) {  // cannot live in the table: goes to the side counter
        n_empty += ((twice >> b) & 1) ? 2 : 1;
        continue;
      }
      int became_dup = 0;
      n_new += hash_insert(dst, key, want_mult, (twice >> b) & 1, &became_dup);
      n_dup += became_dup;
    }
  }
  block_add2_any(n_new, n_dup, &counters[kCntDistinct], &counters[kCntTwice]);
  __syncthreads();
  block_add2_any(n_empty, 0ull, &counters[kCntEmptyRows], &counters[kCntSpare]);
}

// Inserts 16-byte {key, count} records (count saturates at 2) -- merge / cross-rank import.
__global__ __launch_bounds__(256) void hash_import_kernel(const KeyRecord *recs, uint64_t n,
                                                           HashSetView dst, int want_mult,
                                                           unsigned long long *counters) {
  unsigned long long n_new = 0, n_dup = 0, n_empty = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    KeyRecord r = recs[i];
    if (r.key == kEmptyKey) {
      n_empty += r.count;
      continue;
    }
    int became_dup = 0;
    n_new += hash_insert(dst, r.key, want_mult, r.count >= 2, &became_dup);
    n_dup += became_dup;
  }
  block_add2_any(n_new, n_dup, &counters[kCntDistinct], &counters[kCntTwice]);
  __syncthreads();
  block_add2_any(n_empty, 0ull, &counters[kCntEmptyRows], &counters[kCntSpare]);
}

// Export: pass 1 counts records per owner, pass 2 scatters them (owner = mix(key) % world).  Both passes
// aggregate per workgroup in LDS first: one global atomic per (workgroup, owner) instead of one per key
// (all ranks' keys contend on only `world` counters otherwise).
constexpr uint32_t kMaxWorld = 256;

__device__ __forceinline__ uint32_t owner_of(uint64_t key, uint32_t world) {
  return (uint32_t)((mix64(key ^ 0x9e3779b97f4a7c15ULL) >> 32) % world);
}

struct HashSource {
  HashSetView v;
  int want_mult;
  __device__ uint64_t items() const { return v.mask + 1; }
  template <class F>
  __device__ void for_each(uint64_t s, F f) const {
    const uint64_t key = v.keys[s];
    if (key == kEmptyKey) return;
    f(key, (want_mult && ((v.dup[s >> 5] >> (s & 31)) & 1)) ? 2u : 1u);
  }
};

struct BitmapSource {
  BitmapView bm;
  int want_mult;
  __device__ uint64_t items() const { return (bm.range + 31) >> 5; }
  template <class F>
  __device__ void for_each(uint64_t w, F f) const {
    uint32_t seen = bm.seen[w];
    const uint32_t twice = want_mult ? bm.twice[w] : 0;
    while (seen) {
      const int b = __builtin_ctz(seen);
      seen &= seen - 1;
      f((uint64_t)bm.base + (w << 5) + (uint64_t)b, ((twice >> b) & 1) ? 2u : 1u);
    }
  }
};

template <class Src>
__global__ __launch_bounds__(256) void export_count_kernel(Src src, uint32_t world,
                                                            unsigned long long *owner_counts) {
  __shared__ unsigned int cnt[kMaxWorld];
  for (uint32_t t = threadIdx.x; t < world; t += 256) cnt[t] = 0;
  __syncthreads();
  const uint64_t n = src.items();
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
    src.for_each(i, [&](uint64_t key, uint32_t) { atomicAdd(&cnt[owner_of(key, world)], 1u); });
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < world; t += 256)
    if (cnt[t]) atomicAdd(&owner_counts[t], (unsigned long long)cnt[t]);
}

template <class Src>
__global__ __launch_bounds__(256) void export_scatter_kernel(Src src, uint32_t world,
                                                              unsigned long long *cursors, KeyRecord *out) {
  __shared__ unsigned int cnt[kMaxWorld];
  __shared__ unsigned long long pos[kMaxWorld];
  const uint64_t n = src.items();
  const uint64_t step = (uint64_t)gridDim.x * 256;
  const uint64_t rounded = (n + step - 1) / step * step;
  for (uint64_t base = (uint64_t)blockIdx.x * 256; base < rounded; base += step) {
    const uint64_t i = base + threadIdx.x;
    for (uint32_t t = threadIdx.x; t < world; t += 256) cnt[t] = 0;
    __syncthreads();
    if (i < n) src.for_each(i, [&](uint64_t key, uint32_t) { atomicAdd(&cnt[owner_of(key, world)], 1u); });
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < world; t += 256)
      pos[t] = cnt[t] ? atomicAdd(&cursors[t], (unsigned long long)cnt[t]) : 0ull;
    __syncthreads();
    if (i < n)
      src.for_each(i, [&](uint64_t key, uint32_t count) {
        const unsigned long long p = atomicAdd(&pos[owner_of(key, world)], 1ull);
        KeyRecord r;
        r.key = key;
        r.count = count;
        out[p] = r;
      });
    __syncthreads();
  }
}

// Cross-rank reduction of congruent range bitmaps: slice k of the result is the OR of slice k of every
// rank's bitmap; a key is "seen twice" if any rank saw it twice or two ranks saw it at all.
__global__ __launch_bounds__(256) void bitmap_adopt_kernel(const uint32_t *seen_slices,
                                                            const uint32_t *twice_slices, uint32_t n_slices,
                                                            uint64_t slice_words, uint64_t stride, uint32_t *out_seen,
                                                            uint32_t *out_twice,
                                                            unsigned long long *counters) {
  unsigned long long n_seen = 0, n_twice = 0;
  for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < slice_words;
       w += (uint64_t)gridDim.x * 256) {
    uint32_t acc_seen = 0, acc_twice = 0;
    for (uint32_t s = 0; s < n_slices; s++) {
      const uint32_t x = seen_slices[(uint64_t)s * stride + w];
      if (twice_slices) acc_twice |= (acc_seen & x) | twice_slices[(uint64_t)s * stride + w];
      acc_seen |= x;
    }
    out_seen[w] = acc_seen;
    if (out_twice) out_twice[w] = acc_twice;
    n_seen += __builtin_popcount(acc_seen);
    n_twice += __builtin_popcount(acc_twice);
  }
  block_add2_any(n_seen, n_twice, &counters[kCntDistinct], &counters[kCntTwice]);
}

// The send side of the cross-rank exchange (tgx_allreduce): cuts this rank's range bitmap, whose bit 0 stands for
// key `base` of its own choosing, into `world` slices of `slice_words` words on the grid all ranks agreed on -- bit 0
// of slice p stands for key global_lo + p * slice_words * 32.  delta_bits = global_lo - base, so word w of slice p is
// bits [l, l + 32) of the local bitmap with l = (p * slice_words + w) * 32 + delta_bits, zero outside it.  The
// local bitmaps therefore need not be congruent (no range hint, no second pass): re-basing rides on the copy into
// the all-to-all's send buffer.  Block p of the send buffer starts at p * row_words; this column's slice at col_words.
__global__ __launch_bounds__(256) void bitmap_rebase_kernel(const uint32_t *__restrict__ src, uint64_t src_words,
                                                             long long delta_bits, uint32_t world,
                                                             uint64_t slice_words, uint64_t row_words,
                                                             uint64_t col_words, uint32_t *__restrict__ send) {
  const uint64_t total = (uint64_t)world * slice_words;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t p = i / slice_words, w = i - p * slice_words;
    const long long l = (long long)(i * 32) + delta_bits;
    const long long wi = l >> 5;  // arithmetic shift: floor
    const uint32_t sh = (uint32_t)(l & 31);
    const uint32_t lo = (wi >= 0 && (uint64_t)wi < src_words) ? src[wi] : 0u;
    const uint32_t hi = (wi + 1 >= 0 && (uint64_t)(wi + 1) < src_words) ? src[wi + 1] : 0u;
    send[p * row_words + col_words + w] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
  }
}

// ---- big batches of keys that have no dense range (sparse Int64 ids, Float64): no global atomic per key -----------
// The hash set takes one 64-byte read-modify-write at the memory side per KEY (~27 G keys/s whatever the table's
// size).  A batch big enough to care goes the way of the big Utf8 batches instead (lists.h, distinct128.hip): every
// key is replaced by its splitmix64 mix -- a bijection, so equal records mean equal keys: the count is EXACT -- and
// the mixes are partitioned twice by 8 bits into kFpFan^2 lists that are deduplicated one by one in LDS.  The lists
// are the key set until something needs the table (key_insert_kernel un-mixes them into it); a list that overflows
// (heavily repeated keys) flags the batch for a redo through the table.
__device__ __forceinline__ uint64_t unmix64(uint64_t x) {  // inverse of mix64
  x ^= (x >> 31) ^ (x >> 62);
  x *= 0x319642b2d24d8ec3ULL;
  x ^= (x >> 27) ^ (x >> 54);
  x *= 0x96de1b173f119089ULL;
  x ^= (x >> 30) ^ (x >> 60);
  return x;
}

// level 1: a tile of the column's keys -> per-XCD lists by the top byte of their mix
__global__ __launch_bounds__(256) void key_partition_values_kernel(DistinctColDesc d, FpLists out,
                                                                    unsigned long long *counters) {
  constexpr int PER = kFpTile / 256;
  __shared__ FpTileLdsT<KeyRec> s;
  const uint32_t tid = threadIdx.x;
  fp_tile_begin(s);
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)d.values + d.offset);
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t first = (int64_t)blockIdx.x * kFpTile;
  KeyRec mine[PER];
  uint32_t present = 0, n_empty = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int64_t row = first + k * 256 + (int64_t)tid;
    mine[k] = 0;
    if (row < d.length) {
      bool valid = true;
      if (vbits) {
        const int64_t b = d.offset + row;
        valid = TGX_VALID_BIT(vbits, b);
      }
      if (valid) {
        const uint64_t key = (uint64_t)vals[row];
        if (key == kEmptyKey) {
          n_empty++;  // the table's free-slot marker: counted on the side, as everywhere
        } else {
          mine[k] = mix64(key);
          present |= 1u << k;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < PER; k++)
    if ((present >> k) & 1u) atomicAdd(&s.hist[mine[k] >> 56], 1u);
  if (n_empty) {  // (rare)
    atomicAdd(&counters[kCntEmptyRows], (unsigned long long)n_empty);
    atomicAdd(&counters[kCntValidRows], (unsigned long long)n_empty);
  }
  __syncthreads();
  fp_tile_scatter(s, mine, present, (blockIdx.x % kFpXcds) * kFpFan, out, 56, counters);
}

// the lists' records back to keys and into the global table (counted already: no counters)
__global__ __launch_bounds__(256) void key_insert_kernel(FpLists l, HashSetView t, int want_mult) {
  const uint32_t offered = l.offered[blockIdx.x];
  const uint32_t n = offered < l.cap ? offered : (uint32_t)l.cap;
  const KeyRec *recs = (const KeyRec *)l.recs + (uint64_t)blockIdx.x * l.cap;
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    int became_dup = 0;
    (void)hash_insert(t, unmix64(recs[i]), want_mult, 0, &became_dup);
  }
}

void launch_key_lists(const DistinctColDesc &d, const FpLists &level1, const FpLists &level2, int want_mult,
                      uint2 *per_list, unsigned long long *d_counters, hipStream_t stream) {
  const int64_t tiles = (d.length + kFpTile - 1) / kFpTile;
  hipLaunchKernelGGL(key_partition_values_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, d, level1, d_counters);
  const uint32_t tiles_per_list = (uint32_t)((level1.cap + kFpTile - 1) / kFpTile);
  hipLaunchKernelGGL(fp_partition_lists_kernel<KeyRec>, dim3(kFpXcds * kFpFan * tiles_per_list), dim3(256), 0, stream,
                     level1, tiles_per_list, level2, d_counters);
  launch_fp_count_lists<KeyRec>(level2, want_mult, per_list, level1.offered, d_counters, stream, PlainEq());
}

void launch_key_insert(const FpLists &level2, const HashSetView &t, int want_mult, hipStream_t stream) {
  hipLaunchKernelGGL(key_insert_kernel, dim3(kFpFan * kFpFan), dim3(256), 0, stream, level2, t, want_mult);
}

void launch_distinct_hash(const DistinctColDesc &d, const HashSetView &t,
                          unsigned long long *d_counters, hipStream_t stream) {
  hipLaunchKernelGGL(distinct_hash_kernel, dim3(grid_for((uint64_t)d.length)), dim3(256), 0, stream,
                     d, t, d_counters);
}

void launch_distinct_bitmap(const DistinctColDesc &d, const BitmapView &bm,
                            unsigned long long *d_counters, hipStream_t stream) {
  hipLaunchKernelGGL(distinct_bitmap_kernel, dim3(grid_for((uint64_t)d.length)), dim3(256), 0,
                     stream, d, bm, d_counters);
}

void launch_hash_rehash(const HashSetView &src, const HashSetView &dst, int want_mult,
                        unsigned long long *d_counters, hipStream_t stream) {
  hipLaunchKernelGGL(hash_rehash_kernel, dim3(grid_for(src.mask + 1)), dim3(256), 0, stream, src,
                     dst, want_mult, d_counters);
}

void launch_bitmap_to_hash(const BitmapView &bm, const HashSetView &dst, int want_mult,
                           unsigned long long *d_counters, hipStream_t stream) {
  hipLaunchKernelGGL(bitmap_to_hash_kernel, dim3(grid_for((bm.range + 31) >> 5)), dim3(256), 0,
                     stream, bm, dst, want_mult, d_counters);
}

void launch_hash_import(const KeyRecord *recs, uint64_t n, const HashSetView &dst, int want_mult,
                        unsigned long long *d_counters, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(hash_import_kernel, dim3(grid_for(n)), dim3(256), 0, stream, recs, n, dst,
                     want_mult, d_counters);
}

void launch_hash_export_count(const HashSetView &src, uint32_t world, unsigned long long *d_counts,
                              hipStream_t stream) {
  HashSource s{src, 0};
  hipLaunchKernelGGL(export_count_kernel<HashSource>, dim3(grid_for(src.mask + 1)), dim3(256), 0, stream, s,
                     world, d_counts);
}

void launch_hash_export_scatter(const HashSetView &src, uint32_t world, int want_mult,
                                unsigned long long *d_cursors, KeyRecord *out, hipStream_t stream) {
  HashSource s{src, want_mult};
  hipLaunchKernelGGL(export_scatter_kernel<HashSource>, dim3(grid_for(src.mask + 1)), dim3(256), 0, stream, s,
                     world, d_cursors, out);
}

void launch_bitmap_export_count(const BitmapView &bm, uint32_t world, unsigned long long *d_counts,
                                hipStream_t stream) {
  BitmapSource s{bm, 0};
  hipLaunchKernelGGL(export_count_kernel<BitmapSource>, dim3(grid_for((bm.range + 31) >> 5)), dim3(256), 0,
                     stream, s, world, d_counts);
}

void launch_bitmap_export_scatter(const BitmapView &bm, uint32_t world, int want_mult,
                                  unsigned long long *d_cursors, KeyRecord *out, hipStream_t stream) {
  BitmapSource s{bm, want_mult};
  hipLaunchKernelGGL(export_scatter_kernel<BitmapSource>, dim3(grid_for((bm.range + 31) >> 5)), dim3(256), 0,
                     stream, s, world, d_cursors, out);
}

void launch_bitmap_rebase(const uint32_t *src, uint64_t src_words, long long delta_bits, uint32_t world,
                          uint64_t slice_words, uint64_t row_words, uint64_t col_words, uint32_t *send,
                          hipStream_t stream) {
  hipLaunchKernelGGL(bitmap_rebase_kernel, dim3(grid_for((uint64_t)world * slice_words)), dim3(256), 0, stream, src,
                     src_words, delta_bits, world, slice_words, row_words, col_words, send);
}

void launch_bitmap_adopt(const uint32_t *seen_slices, const uint32_t *twice_slices, uint32_t n_slices,
                         uint64_t slice_words, uint64_t stride_words, uint32_t *out_seen, uint32_t *out_twice,
                         unsigned long long *d_counters, hipStream_t stream) {
  hipLaunchKernelGGL(bitmap_adopt_kernel, dim3(grid_for(slice_words)), dim3(256), 0, stream, seen_slices,
                     twice_slices, n_slices, slice_words, stride_words, out_seen, out_twice, d_counters);
}

// identities of the two small accumulators (a kernel, not two copies from pageable host memory: those stall the
// caller for a staging round trip each)
__global__ void distinct_init_kernel(DistinctSample *sample, OutlierStats *outliers) {
  if (threadIdx.x != 0) return;
  if (sample) {
    sample->min_v = INT64_MAX;
    sample->max_v = INT64_MIN;
    sample->count = 0;
    sample->pad = 0;
  }
  if (outliers) {
    outliers->mn = INT64_MAX;
    outliers->mx = INT64_MIN;
    outliers->lo32_sum = 0;
    outliers->hi32_sum = 0;
    outliers->count = 0;
  }
}

void launch_distinct_init(DistinctSample *sample, OutlierStats *outliers, hipStream_t stream) {
  hipLaunchKernelGGL(distinct_init_kernel, dim3(1), dim3(64), 0, stream, sample, outliers);
}

void launch_distinct_sample(const DistinctColDesc &d, DistinctSample *out, hipStream_t stream) {
  const int grid = d.pad ? (int)std::min<int64_t>(1024, (d.length + 4095) / 4096) : 64;
  hipLaunchKernelGGL(distinct_sample_kernel, dim3(grid < 1 ? 1 : grid), dim3(256), 0, stream, d, out);
}

void launch_distinct_outliers(const DistinctColDesc &d, int64_t base, uint64_t range, const HashSetView &t,
                              unsigned long long *d_counters, hipStream_t stream) {
  hipLaunchKernelGGL(distinct_outlier_kernel, dim3(grid_for((uint64_t)d.length)), dim3(256), 0, stream, d, base, range,
                     t, d_counters);
}

}  // namespace tgx
