// keyprobe.hip -- key probe for gfx950 (TGX_CHECK_KEY_PROBE): is each child key in the parent's key set?  The device side
// of the reference's ForeignKeyConstraint (TG/constraints/foreign_key.rs:152-176),
//   SELECT COUNT(*), COUNT(DISTINCT child.c) FROM child LEFT JOIN parent ON child.c = parent.p WHERE parent.p IS NULL
// for integer keys: one walk of the child column against a read-only set, plus a bounded table of the keys not in it.
//
//   the set     built once per parent (tgx_key_probe_set_parent) from 16-byte {key, count} records, counts ignored (a plain spec),
//               duplicates allowed.  key_probe_reduce_kernel takes MIN, MAX of the keys; the host picks the route:
//               a bitmap of 32-bit words over [MIN, MAX] when range <= 128 * records (no larger than the table would
//               be), else an open-addressing table of the smallest power of two >= 2 * records slots, filled by linear
//               probing from mix64(key) & mask with a CAS on kEmptyKey.  The key whose bits are kEmptyKey is a bit like
//               any other on the bitmap route and a flag on the hash route.  The lane whose atomicOr / CAS / exchange
//               made the entry counts it: parent_keys and parent_digest come out of the build itself.
//   the probe   key_probe_kernel<route>, grid = (blocks, tasks): row_walk.h's single-column walk (8 B + 1 bit a row).
//               Bitmap: an unsigned range test and one bit test.  Hash: probe until the key or a free slot, at most
//               mask + 1 probes (at load <= 0.5 a free slot always comes first; the bound keeps any table from making
//               the loop spin).  A miss goes into the workgroup's LDS count table and from there into the task's global
//               table, as valuecounts.hip's integer keys do: the wave's first missing key is counted once for its
//               lanes, a full LDS neighbourhood sends the key to the global table directly, a global probe sequence
//               that runs out adds the key's weight to the overflow counter.  So every non-NULL row is in exactly one
//               of: matched, an entry, the marker's counter, the overflow counter.
//   counted     a spec set with tgx_plan_set_key_probe_counted keeps the records' counts: the reference's
//               JoinCoverageConstraint (TG/constraints/join_coverage.rs) asks for COUNT(*) over the join, which counts
//               matched PAIRS.  key_probe_reduce_kernel<true> also takes, exactly, the records with a zero count, the
//               counts' sum (in three pieces that cannot wrap) and the count digest; the builds leave the largest count.  Route 3 is an
//               array of 64-bit counts over [MIN, MAX] when range <= 4 * records (no larger than route 4's table), route
//               4 a table of 16-byte {key, count} slots probed as route 2's is: a hit reads its count from the line it
//               has just fetched.  Duplicate records add up (atomicAdd); the lane that takes a count from 0 counts the
//               key.  The probe returns the key's multiplicity, 0 = not in the set; a lane sums the multiplicities of
//               its matched rows in 64 bits (the host refuses a batch that could carry the sum past 2^64 - 1) and a wave
//               adds its sum to kKpPairs once.  The miss path is the plain one.
#include <hip/hip_runtime.h>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "row_walk.h"

namespace tgx {

namespace {

__device__ __forceinline__ void kp_insert_global(const KeyProbeTable &t, unsigned long long key,
                                                 unsigned long long weight) {
  const int64_t s = vc_claim<uint64_t>(t.keys, t.mask, mix64(key ^ t.salt) & t.mask, key, kKeyProbeProbes);
  if (s >= 0) atomicAdd(&t.counts[s], weight);
  else atomicAdd(&t.words[kKpOverflow], weight);
}

// the wave's sums of a count and a digest term into the build's counters (non-zero counts only).  (Two wave_sums, with
// their shuffles taken step by step together as tail_flush takes its two: one after the other they come to the same
// sums, but the build kernels' tails are scheduled differently)
__device__ __forceinline__ void kp_build_flush(unsigned long long made, unsigned long long digest, KeyProbeBuild *b) {
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    made += __shfl_down(made, dlt, 64);
    digest += __shfl_down(digest, dlt, 64);
  }
  if ((threadIdx.x & 63) == 0 && made) {
    atomicAdd(&b->keys, made);
    atomicAdd(&b->digest, digest);
  }
}

// a counted build: the largest count a key has come to.  (Counts only grow and their sum is below 2^63: the largest
// value an atomicAdd has left behind is the largest count of the finished set)
__device__ __forceinline__ void kp_build_most(unsigned long long most, KeyProbeBuild *b) {
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    const unsigned long long o = __shfl_down(most, dlt, 64);
    most = o > most ? o : most;
  }
  if ((threadIdx.x & 63) == 0 && most) atomicMax(&b->max_count, most);
}

// how often `key` occurs in the set: 0 = it is not in it (a plain set: 0 or 1)
template <int kRoute>
__device__ __forceinline__ unsigned long long kp_lookup(const KeyProbeSet &s, unsigned long long key) {
  if (kRoute == kKpRouteBitmap) {
    const uint64_t off = key - s.base;  // (a key below the base wraps to something above every range)
    if (off >= s.range) return 0;
    return (s.bits[off >> 5] >> (off & 31)) & 1u;
  }
  if (kRoute == kKpRouteHash) {
    if (key == kEmptyKey) return s.has_marker != 0;
    uint64_t h = mix64(key) & s.mask;
    for (uint64_t p = 0; p <= s.mask; p++) {
      const unsigned long long k = s.keys[h];
      if (k == key) return 1;
      if (k == kEmptyKey) return 0;
      h = (h + 1) & s.mask;
    }
  }
  if (kRoute == kKpRouteCountArray) {
    const uint64_t off = key - s.base;
    if (off >= s.range) return 0;
    return s.counts[off];
  }
  if (kRoute == kKpRouteCountHash) {
    if (key == kEmptyKey) return s.marker_count;
    const ulonglong2 *slots = (const ulonglong2 *)s.counts;
    uint64_t h = mix64(key) & s.mask;
    for (uint64_t p = 0; p <= s.mask; p++) {
      const ulonglong2 e = slots[h];  // (one 16-byte load: the key and its count)
      if (e.x == key) return e.y;
      if (e.x == kEmptyKey) return 0;
      h = (h + 1) & s.mask;
    }
  }
  return 0;
}

}  // namespace

// ---- the build -----------------------------------------------------------------------------------------------------------
template <bool kCounted>
__global__ __launch_bounds__(256) void key_probe_reduce_kernel(const unsigned long long *__restrict__ recs, uint64_t n,
                                                               KeyProbeBuild *b) {
  long long lo = INT64_MAX, hi = INT64_MIN;
  unsigned long long zeros = 0, p0 = 0, p1 = 0, p2 = 0, cdigest = 0;
  constexpr unsigned long long kPiece = (1ull << kKpPieceBits) - 1;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long long k = (long long)recs[2 * i];
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
    if (kCounted) {
      const unsigned long long c = recs[2 * i + 1];
      zeros += c == 0 ? 1 : 0;
      p0 += c & kPiece;
      p1 += (c >> kKpPieceBits) & kPiece;
      p2 += c >> (2 * kKpPieceBits);
      cdigest += c * mix64((unsigned long long)k ^ kKeyProbeCountSalt);
    }
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    const long long ol = __shfl_down(lo, dlt, 64), oh = __shfl_down(hi, dlt, 64);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if (kCounted) {
    zeros = wave_sum(zeros);
    p0 = wave_sum(p0);
    p1 = wave_sum(p1);
    p2 = wave_sum(p2);
    cdigest = wave_sum(cdigest);
  }
  if ((threadIdx.x & 63) == 0 && lo <= hi) {
    atomicMin(&b->min, lo);
    atomicMax(&b->max, hi);
    if (kCounted) {
      if (zeros) atomicAdd(&b->zero_counts, zeros);
      if (p0) atomicAdd(&b->sum_piece[0], p0);
      if (p1) atomicAdd(&b->sum_piece[1], p1);
      if (p2) atomicAdd(&b->sum_piece[2], p2);
      atomicAdd(&b->count_digest, cdigest);
    }
  }
}

__global__ __launch_bounds__(256) void key_probe_build_bitmap_kernel(const unsigned long long *__restrict__ recs,
                                                                     uint64_t n, uint32_t *bits, uint64_t base,
                                                                     uint64_t range, KeyProbeBuild *b) {
  unsigned long long made = 0, digest = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long key = recs[2 * i];
    const uint64_t off = key - base;
    if (off >= range) continue;  // (cannot happen: base and range come from these records)
    const uint32_t bit = 1u << (off & 31);
    if ((atomicOr(&bits[off >> 5], bit) & bit) == 0) {
      made++;
      digest += mix64(key ^ kKeyProbeDigestSalt);
    }
  }
  kp_build_flush(made, digest, b);
}

__global__ __launch_bounds__(256) void key_probe_build_hash_kernel(const unsigned long long *__restrict__ recs,
                                                                   uint64_t n, unsigned long long *keys, uint64_t mask,
                                                                   KeyProbeBuild *b) {
  unsigned long long made = 0, digest = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long key = recs[2 * i];
    bool mine = false;
    if (key == kEmptyKey) {
      mine = atomicExch(&b->has_marker, 1u) == 0;
    } else {
      uint64_t h = mix64(key) & mask;
      for (uint64_t p = 0; p <= mask; p++) {
        unsigned long long old = vc_peek(&keys[h]);
        if (old == kEmptyKey) old = atomicCAS(&keys[h], (unsigned long long)kEmptyKey, key);
        mine = old == kEmptyKey;
        if (mine || old == key) break;
        h = (h + 1) & mask;
      }
    }
    if (mine) {
      made++;
      digest += mix64(key ^ kKeyProbeDigestSalt);
    }
  }
  kp_build_flush(made, digest, b);
}

// (every record's count is > 0: the host has looked at zero_counts before it builds)
__global__ __launch_bounds__(256) void key_probe_build_count_array_kernel(const unsigned long long *__restrict__ recs,
                                                                          uint64_t n, unsigned long long *counts,
                                                                          uint64_t base, uint64_t range, KeyProbeBuild *b) {
  unsigned long long made = 0, digest = 0, most = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long key = recs[2 * i], c = recs[2 * i + 1];
    const uint64_t off = key - base;
    if (off >= range || c == 0) continue;  // (cannot happen: base and range come from these records)
    const unsigned long long old = atomicAdd(&counts[off], c);
    most = old + c > most ? old + c : most;
    if (old == 0) {
      made++;
      digest += mix64(key ^ kKeyProbeDigestSalt);
    }
  }
  kp_build_flush(made, digest, b);
  kp_build_most(most, b);
}

// the slots of a counted table, free: {kEmptyKey, 0}
__global__ __launch_bounds__(256) void key_probe_clear_pairs_kernel(unsigned long long *slots, uint64_t n_slots) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
    slots[2 * i] = kEmptyKey;
    slots[2 * i + 1] = 0;
  }
}

__global__ __launch_bounds__(256) void key_probe_build_count_hash_kernel(const unsigned long long *__restrict__ recs,
                                                                         uint64_t n, unsigned long long *slots,
                                                                         uint64_t mask, KeyProbeBuild *b) {
  unsigned long long made = 0, digest = 0, most = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long key = recs[2 * i], c = recs[2 * i + 1];
    if (c == 0) continue;
    bool mine = false;
    unsigned long long old = 0;
    if (key == kEmptyKey) {
      old = atomicAdd(&b->marker_count, c);
      mine = old == 0;
    } else {
      uint64_t h = mix64(key) & mask;
      for (uint64_t p = 0; p <= mask; p++) {
        unsigned long long held = vc_peek(&slots[2 * h]);
        if (held == kEmptyKey) held = atomicCAS(&slots[2 * h], (unsigned long long)kEmptyKey, key);
        if (held == kEmptyKey || held == key) {
          old = atomicAdd(&slots[2 * h + 1], c);  // (the count is added after the claim)
          mine = old == 0;
          break;
        }
        h = (h + 1) & mask;
      }
    }
    most = old + c > most ? old + c : most;
    if (mine) {
      made++;
      digest += mix64(key ^ kKeyProbeDigestSalt);
    }
  }
  kp_build_flush(made, digest, b);
  kp_build_most(most, b);
}

// ---- the parent side from rows ---------------------------------------------------------------------------------------------
// A DISTINCT export knows a key as seen once or more than once, not how often.  A spec set with
// tgx_plan_set_key_probe_rows gathers its column instead: every non-NULL key of a batch becomes a {key, 1} record behind
// the records of the batches before it, which is what a counted set is built from (duplicate records add up).  *cursor
// is the task's kKpNonNull counter: the records so far.  The host has made room for every row of the batch; a position
// is still held against `cap` before it is written.
__global__ __launch_bounds__(256) void key_probe_rows_kernel(const ComomentColDesc d, unsigned long long *recs, uint64_t cap,
                                                             unsigned long long *cursor) {
  const int lane = threadIdx.x & 63;
  jb_for_rows_single(d, [&](int64_t v, bool ok) {
    const unsigned long long live = __ballot(ok);
    if (live == 0) return;
    const int leader = __ffsll((long long)live) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(live));
    base = vc_shfl64(base, leader);
    if (!ok) return;
    const uint64_t at = base + (uint64_t)__popcll(live & ((1ull << lane) - 1));
    if (at >= cap) return;  // (cannot happen: cap counts every row the state has seen)
    recs[2 * at] = (unsigned long long)v;
    recs[2 * at + 1] = 1;
  });
}

// ---- the probe -----------------------------------------------------------------------------------------------------------
template <int kRoute>
__global__ __launch_bounds__(kKeyProbeBlock) void key_probe_kernel(const KeyProbeLaunch L) {
  __shared__ unsigned long long lkeys[kKeyProbeLdsSlots];
  __shared__ unsigned int lcounts[kKeyProbeLdsSlots];
  for (uint32_t s = threadIdx.x; s < kKeyProbeLdsSlots; s += kKeyProbeBlock) {
    lkeys[s] = kEmptyKey;
    lcounts[s] = 0;
  }
  __syncthreads();

  const ComomentColDesc &d = L.cols[blockIdx.y];
  const KeyProbeSet &set = L.sets[blockIdx.y];
  const KeyProbeTable &t = L.tables[blockIdx.y];
  const int lane = threadIdx.x & 63;
  uint32_t non_null = 0, matched = 0, marker = 0;  // (a workgroup sees fewer than 2^32 rows: side_rows_fit)
  unsigned long long pairs = 0;                    // (a counted set: cannot wrap, the host has refused such a batch)
  jb_for_rows_single(d, [&](int64_t v, bool ok) {
    const unsigned long long key = (unsigned long long)v;
    non_null += ok ? 1u : 0u;
    const unsigned long long times = ok ? kp_lookup<kRoute>(set, key) : 0;
    const bool found = times != 0;
    matched += found ? 1u : 0u;
    if (kRoute >= kKpRouteCountArray) pairs += times;
    const bool miss = ok && !found;
    const bool is_marker = miss && key == kEmptyKey;  // (the missing key whose bits are the free-slot marker)
    marker += is_marker ? 1u : 0u;
    const bool live = miss && !is_marker;
    const unsigned long long todo = __ballot(live);
    if (todo == 0) return;
    // the wave's first missing key is counted once for all the lanes that hold it; the others add for themselves
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned long long first = vc_shfl64(key, leader);
    const unsigned long long same = __ballot(live && key == first);
    const bool adds = lane == leader || (live && key != first);
    if (!adds) return;
    const uint32_t weight = lane == leader ? (uint32_t)__popcll(same) : 1u;
    const int64_t s = vc_claim<uint32_t>(lkeys, kKeyProbeLdsSlots - 1,
                                         (uint32_t)mix64(key ^ t.salt) & (kKeyProbeLdsSlots - 1), key,
                                         kKeyProbeLdsProbes);
    if (s >= 0) atomicAdd(&lcounts[s], weight);
    else kp_insert_global(t, key, weight);  // (the workgroup's table is full around there)
  });
  tail_flush(non_null, matched, t.words);     // kKpNonNull, kKpMatched
  tail_flush(marker, 0u, t.words + kKpMarker);
  if (kRoute >= kKpRouteCountArray) {
    pairs = wave_sum(pairs);
    if (lane == 0 && pairs) atomicAdd(&t.words[kKpPairs], pairs);
  }
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kKeyProbeLdsSlots; s += kKeyProbeBlock) {
    const unsigned long long key = lkeys[s];
    if (key != kEmptyKey) kp_insert_global(t, key, lcounts[s]);
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
void launch_key_probe_reduce(const void *recs, uint64_t n, bool counted, KeyProbeBuild *b, hipStream_t stream) {
  if (counted)
    hipLaunchKernelGGL(key_probe_reduce_kernel<true>, dim3(grid_for(n)), dim3(256), 0, stream,
                       (const unsigned long long *)recs, n, b);
  else
    hipLaunchKernelGGL(key_probe_reduce_kernel<false>, dim3(grid_for(n)), dim3(256), 0, stream,
                       (const unsigned long long *)recs, n, b);
}

void launch_key_probe_build_bitmap(const void *recs, uint64_t n, uint32_t *bits, uint64_t base, uint64_t range,
                                   KeyProbeBuild *b, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_build_bitmap_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     (const unsigned long long *)recs, n, bits, base, range, b);
}

void launch_key_probe_build_hash(const void *recs, uint64_t n, unsigned long long *keys, uint64_t mask,
                                 KeyProbeBuild *b, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_build_hash_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     (const unsigned long long *)recs, n, keys, mask, b);
}

void launch_key_probe_build_count_array(const void *recs, uint64_t n, unsigned long long *counts, uint64_t base,
                                        uint64_t range, KeyProbeBuild *b, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_build_count_array_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     (const unsigned long long *)recs, n, counts, base, range, b);
}

void launch_key_probe_build_count_hash(const void *recs, uint64_t n, unsigned long long *slots, uint64_t mask,
                                       KeyProbeBuild *b, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_clear_pairs_kernel, dim3(grid_for(mask + 1)), dim3(256), 0, stream, slots, mask + 1);
  hipLaunchKernelGGL(key_probe_build_count_hash_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     (const unsigned long long *)recs, n, slots, mask, b);
}

void launch_key_probe_rows(const ComomentColDesc &d, unsigned long long *recs, uint64_t cap, unsigned long long *cursor,
                           int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_rows_kernel, dim3(blocks), dim3(256), 0, stream, d, recs, cap, cursor);
}

void launch_key_probe(const KeyProbeLaunch &L, int route, int n_tasks, int blocks, hipStream_t stream) {
  const dim3 grid(blocks, n_tasks), block(kKeyProbeBlock);
  if (route == kKpRouteBitmap) hipLaunchKernelGGL(key_probe_kernel<kKpRouteBitmap>, grid, block, 0, stream, L);
  else if (route == kKpRouteHash) hipLaunchKernelGGL(key_probe_kernel<kKpRouteHash>, grid, block, 0, stream, L);
  else if (route == kKpRouteCountArray) hipLaunchKernelGGL(key_probe_kernel<kKpRouteCountArray>, grid, block, 0, stream, L);
  else if (route == kKpRouteCountHash) hipLaunchKernelGGL(key_probe_kernel<kKpRouteCountHash>, grid, block, 0, stream, L);
  else hipLaunchKernelGGL(key_probe_kernel<kKpRouteEmpty>, grid, block, 0, stream, L);
}

}  // namespace tgx
