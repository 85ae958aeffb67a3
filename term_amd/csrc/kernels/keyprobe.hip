// keyprobe.hip -- key probe for gfx950 (TGX_CHECK_KEY_PROBE): is each child key in the parent's key set?  The device side
// of the reference's ForeignKeyConstraint (TG/constraints/foreign_key.rs:152-176),
//   SELECT COUNT(*), COUNT(DISTINCT child.c) FROM child LEFT JOIN parent ON child.c = parent.p WHERE parent.p IS NULL
// for integer keys: one walk of the child column against a read-only set, plus a bounded table of the keys not in it.
//
//   the set     built once per parent (tgx_key_probe_set_parent) from 16-byte {key, count} records, counts ignored,
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

// the wave's sums of a count and a digest term into the build's counters (non-zero counts only)
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

template <int kRoute>
__device__ __forceinline__ bool kp_contains(const KeyProbeSet &s, unsigned long long key) {
  if (kRoute == kKpRouteBitmap) {
    const uint64_t off = key - s.base;  // (a key below the base wraps to something above every range)
    if (off >= s.range) return false;
    return ((s.bits[off >> 5] >> (off & 31)) & 1u) != 0;
  }
  if (kRoute == kKpRouteHash) {
    if (key == kEmptyKey) return s.has_marker != 0;
    uint64_t h = mix64(key) & s.mask;
    for (uint64_t p = 0; p <= s.mask; p++) {
      const unsigned long long k = s.keys[h];
      if (k == key) return true;
      if (k == kEmptyKey) return false;
      h = (h + 1) & s.mask;
    }
  }
  return false;
}

}  // namespace

// ---- the build -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void key_probe_reduce_kernel(const unsigned long long *__restrict__ recs, uint64_t n,
                                                               KeyProbeBuild *b) {
  long long lo = INT64_MAX, hi = INT64_MIN;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const long long k = (long long)recs[2 * i];
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    const long long ol = __shfl_down(lo, dlt, 64), oh = __shfl_down(hi, dlt, 64);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if ((threadIdx.x & 63) == 0 && lo <= hi) {
    atomicMin(&b->min, lo);
    atomicMax(&b->max, hi);
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
  jb_for_rows_single(d, [&](int64_t v, bool ok) {
    const unsigned long long key = (unsigned long long)v;
    non_null += ok ? 1u : 0u;
    const bool found = ok && kp_contains<kRoute>(set, key);
    matched += found ? 1u : 0u;
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
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kKeyProbeLdsSlots; s += kKeyProbeBlock) {
    const unsigned long long key = lkeys[s];
    if (key != kEmptyKey) kp_insert_global(t, key, lcounts[s]);
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
void launch_key_probe_reduce(const void *recs, uint64_t n, KeyProbeBuild *b, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_reduce_kernel, dim3(grid_for(n)), dim3(256), 0, stream, (const unsigned long long *)recs,
                     n, b);
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

void launch_key_probe(const KeyProbeLaunch &L, int route, int n_tasks, int blocks, hipStream_t stream) {
  const dim3 grid(blocks, n_tasks), block(kKeyProbeBlock);
  if (route == kKpRouteBitmap) hipLaunchKernelGGL(key_probe_kernel<kKpRouteBitmap>, grid, block, 0, stream, L);
  else if (route == kKpRouteHash) hipLaunchKernelGGL(key_probe_kernel<kKpRouteHash>, grid, block, 0, stream, L);
  else hipLaunchKernelGGL(key_probe_kernel<kKpRouteEmpty>, grid, block, 0, stream, L);
}

}  // namespace tgx
