// keyprobe_strings.hip -- the key probe on STRING keys for gfx950 (a TGX_CHECK_KEY_PROBE spec set with
// tgx_plan_set_key_probe_strings): is each value of a child string column among the parent's values?  The device side of
// the reference's ForeignKeyConstraint (TG/constraints/foreign_key.rs:152-176) where both columns are strings.
//
//   the set     route 5, built once per parent (tgx_key_probe_set_parent) from 32-byte {hash_a, hash_b, count, 0} records
//               -- what a DISTINCT export hands out for a string column: the values' keyed 128-bit fingerprints
//               (fingerprint.h) -- counts ignored, duplicates allowed.  An open-addressing table of the smallest power of
//               two >= 2 * records slots of 16 bytes {fa, fb}, probed linearly from fa & mask; a slot is free while its fa
//               word is kEmptyKey.  The build claims fa by CAS and settles fb by CAS (count_table.h's order); the lane
//               that made the entry counts it and adds its digest term, so parent_keys and parent_digest come out of
//               the build itself.  A record with a marker word can be no fingerprint: it is counted, not inserted, and
//               the host refuses the set.
//   the probe   key_probe_utf8_kernel: a row per lane through utf8_value_of's three layouts, as valuecounts.hip's string
//               route.  The whole value is fingerprinted, whatever its length, and looked up: one 16-byte load a probe, a
//               hit when both words agree, a miss at a free slot, at most mask + 1 probes, every index masked before
//               use.  A missing value longer than max_value_bytes is a long row; the other missing values go the way
//               VALUE_COUNTS's strings go (vc_wave_combine128, the workgroup's VcLdsStrings table, vc_insert_global128
//               with the byte store; a probe sequence that runs out: the overflow counter).  So every non-NULL row is
//               in exactly one of: matched, an entry, the long rows, the overflow rows.
//   dictionary  dict_count.h counts the rows per entry; key_probe_dict_kernel then takes a lane per entry with a non-zero
//               count, fingerprints the entry and probes once: its count goes to matched, or the entry is inserted as
//               missing with that weight.  Rows of NULL entries and of indices outside the dictionary are counted
//               nowhere: they are NULL rows.
#include <hip/hip_runtime.h>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "dict_count.h"
#include "fingerprint.h"

namespace tgx {

namespace {

// is (fa, fb) in the set?
__device__ __forceinline__ bool kps_lookup(const KeyProbeStringSet &s, unsigned long long fa, unsigned long long fb) {
  if (!s.slots) return false;
  const ulonglong2 *slots = (const ulonglong2 *)s.slots;
  uint64_t h = fa & s.mask;
  for (uint64_t p = 0; p <= s.mask; p++) {
    const ulonglong2 e = slots[h];  // (one 16-byte load: both words)
    if (e.x == fa && e.y == fb) return true;
    if (e.x == kEmptyKey) return false;
    h = (h + 1) & s.mask;
  }
  return false;
}

}  // namespace

// ---- the build -----------------------------------------------------------------------------------------------------------
// (every slot word is kEmptyKey when the kernel starts)
__global__ __launch_bounds__(256) void key_probe_build_strings_kernel(const unsigned long long *__restrict__ recs,
                                                                      uint64_t n, unsigned long long *slots, uint64_t mask,
                                                                      KeyProbeStringsBuild *b) {
  unsigned long long made_n = 0, digest = 0, markers = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long fa = recs[4 * i], fb = recs[4 * i + 1];
    if (fa == kEmptyKey || fb == kEmptyKey) {
      markers++;
      continue;
    }
    uint64_t h = fa & mask;
    for (uint64_t p = 0; p <= mask; p++) {
      unsigned long long a = vc_peek(&slots[2 * h]);
      if (a == kEmptyKey) a = atomicCAS(&slots[2 * h], (unsigned long long)kEmptyKey, fa);
      if (a == kEmptyKey || a == fa) {
        unsigned long long o = vc_peek(&slots[2 * h + 1]);
        const bool made =
            o == kEmptyKey && (o = atomicCAS(&slots[2 * h + 1], (unsigned long long)kEmptyKey, fb)) == kEmptyKey;
        if (made) {
          made_n++;
          digest += mix64(mix64(fa ^ kKeyProbeDigestSalt) ^ fb);
        }
        if (made || o == fb) break;
      }
      h = (h + 1) & mask;
    }
  }
  made_n = wave_sum(made_n);
  digest = wave_sum(digest);
  markers = wave_sum(markers);
  if ((threadIdx.x & 63) == 0) {
    if (made_n) {
      atomicAdd(&b->keys, made_n);
      atomicAdd(&b->digest, digest);
    }
    if (markers) atomicAdd(&b->marker_records, markers);
  }
}

// ---- the probe -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void key_probe_utf8_kernel(const Utf8ColDesc d, const KeyProbeStringSet set,
                                                             const ValueCountsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t non_null = 0, matched = 0, too_long = 0;  // (a workgroup sees fewer than 2^32 rows: side_rows_fit)
  __shared__ VcLdsStrings lds;
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    lds.fa[s] = lds.fb[s] = kEmptyKey;
    lds.count[s] = 0;
  }
  __syncthreads();
  // (the loop is uniform within the wave: every lane takes part in the ballots of every round)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const int64_t slot = d.offset + i;
    const bool valid = i < d.length && (!vbits || TGX_VALID_BIT(vbits, slot));
    uintptr_t p = 0;
    uint64_t len = 0;
    unsigned long long fa = 0, fb = 0;
    bool live = false;
    if (valid) {
      non_null++;
      utf8_value_of(d, slot, &p, &len);
      uint64_t a, b;
      fingerprint(d.key, p, len, &a, &b);  // (of the whole value: only the table of missing keys is bounded in bytes)
      fa = a;
      fb = b;
      if (kps_lookup(set, fa, fb)) matched++;
      else if (len > t.max_value_bytes) too_long++;
      else live = true;
    }
    vc_wave_combine128(live, fa, fb, lane, [&](uint32_t weight) {
      if (!vc_insert_lds128(lds, fa, fb, weight, (unsigned long long)i))
        vc_insert_global128(t, fa, fb, (unsigned long long)weight, p, (uint32_t)len, &t.words[kKpOverflow]);
    });
  }
  __syncthreads();
  // every occupied LDS slot is one global insert with its count; its bytes are those of the row it remembers
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    const unsigned long long fa = lds.fa[s], fb = lds.fb[s];
    const unsigned int n = lds.count[s];
    if (fa == kEmptyKey || fb == kEmptyKey || n == 0) continue;
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, d.offset + (int64_t)lds.row[s], &p, &len);
    if (len > t.max_value_bytes) continue;  // (cannot happen: a remembered row was no long row)
    vc_insert_global128(t, fa, fb, (unsigned long long)n, p, (uint32_t)len, &t.words[kKpOverflow]);
  }
  // (tail_flush adds to out[0] and out[1], non-zero sums only: kKpLong's neighbour is never written from here)
  tail_flush(non_null, matched, t.words + kKpNonNull);
  tail_flush(too_long, 0u, t.words + kKpLong);
}

// `d`: the dictionary's values as a string column; a lane per entry with a non-zero count
__global__ __launch_bounds__(256) void key_probe_dict_kernel(const Utf8ColDesc d,
                                                             const unsigned long long *__restrict__ cells,
                                                             const KeyProbeStringSet set, const ValueCountsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long non_null = 0, matched = 0, too_long = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d.length; e += stride) {
    const unsigned long long n = cells[e];
    const int64_t slot = d.offset + e;
    if (n == 0 || (vbits && !TGX_VALID_BIT(vbits, slot))) continue;
    non_null += n;
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, slot, &p, &len);
    uint64_t fa, fb;
    fingerprint(d.key, p, len, &fa, &fb);
    if (kps_lookup(set, fa, fb)) matched += n;
    else if (len > t.max_value_bytes) too_long += n;
    else vc_insert_global128(t, fa, fb, n, p, (uint32_t)len, &t.words[kKpOverflow]);
  }
  non_null = wave_sum(non_null);
  matched = wave_sum(matched);
  too_long = wave_sum(too_long);
  if ((threadIdx.x & 63) == 0) {
    if (non_null) atomicAdd(&t.words[kKpNonNull], non_null);
    if (matched) atomicAdd(&t.words[kKpMatched], matched);
    if (too_long) atomicAdd(&t.words[kKpLong], too_long);
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
void launch_key_probe_build_strings(const void *recs, uint64_t n, unsigned long long *slots, uint64_t mask,
                                    KeyProbeStringsBuild *b, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_build_strings_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     (const unsigned long long *)recs, n, slots, mask, b);
}

void launch_key_probe_utf8(const Utf8ColDesc &d, const KeyProbeStringSet &set, const ValueCountsTable &t,
                           hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_utf8_kernel, dim3(grid_for((uint64_t)d.length)), dim3(256), 0, stream, d, set, t);
}

void launch_key_probe_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                           const Utf8ColDesc &dict, unsigned long long *cells, const KeyProbeStringSet &set,
                           const ValueCountsTable &t, hipStream_t stream) {
  launch_dict_count(indices, validity, offset, length, dict.length, cells, stream);
  hipLaunchKernelGGL(key_probe_dict_kernel, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0, stream, dict, cells,
                     set, t);
}

}  // namespace tgx
