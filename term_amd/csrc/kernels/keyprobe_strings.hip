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
//   counted     a spec set with tgx_plan_set_key_probe_strings_counted (the reference's JoinCoverageConstraint,
//               TG/constraints/join_coverage.rs, on string keys) keeps the records' counts: route 6 is route 5's slot
//               table -- the same claims, the same lookup, kps_claim and kps_find below -- with one 64-bit count a slot
//               in an array beside it.  The build adds a record's count to its slot's word after the claim (duplicate
//               records add up) and takes, in the same pass, keyprobe.hip's counted reduction: zero counts, the sum in
//               three pieces, the count digest, the largest count.  The probe kernels take the set as a template
//               parameter: on a hit the counted instantiation reads the slot's count (8 more bytes a matched row) and
//               sums it per lane, n * count on the dictionary walk; a wave adds its sum to kKpPairs once.  The miss path
//               is the plain one, and the plain instantiation is what it was.
//   gather      a spec set with tgx_plan_set_key_probe_rows_strings probes nothing: every non-NULL row becomes a 32-byte
//               {fa, fb, 1, 0} record -- a DISTINCT export's format -- behind the records of the batches before it, what
//               a counted set is built from.  A dictionary batch gives one {fa, fb, n, 0} record per entry that n > 0
//               of its rows refer to.  A wave counts the non-NULL rows of all its rounds from the validity bits and
//               bumps the cursor once (the dictionary walk, whose entries are few: once a round); a record is two
//               16-byte stores.
#include <hip/hip_runtime.h>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "dict_count.h"
#include "fingerprint.h"
#include "keyprobe_set.h"

namespace tgx {

namespace {

// (kps_find, kps_times and KpsCounted, the lookup in routes 5 and 6: keyprobe_set.h, shared with keyprobe_tuples.hip)
// the build's claim of (fa, fb), neither word the marker: fa by CAS, then fb by CAS (count_table.h's order).  The slot
// that holds the fingerprint, or -1 (a table without a free slot: cannot happen at load <= 0.5); *made: this call made
// the entry.  (Routes 5 and 6)
__device__ __forceinline__ int64_t kps_claim(unsigned long long *slots, uint64_t mask, unsigned long long fa,
                                             unsigned long long fb, bool *made) {
  *made = false;
  uint64_t h = fa & mask;
  for (uint64_t p = 0; p <= mask; p++) {
    unsigned long long a = vc_peek(&slots[2 * h]);
    if (a == kEmptyKey) a = atomicCAS(&slots[2 * h], (unsigned long long)kEmptyKey, fa);
    if (a == kEmptyKey || a == fa) {
      unsigned long long o = vc_peek(&slots[2 * h + 1]);
      *made = o == kEmptyKey && (o = atomicCAS(&slots[2 * h + 1], (unsigned long long)kEmptyKey, fb)) == kEmptyKey;
      if (*made || o == fb) return (int64_t)h;
    }
    h = (h + 1) & mask;
  }
  return -1;
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
    bool made;
    kps_claim(slots, mask, fa, fb, &made);
    if (made) {
      made_n++;
      digest += mix64(mix64(fa ^ kKeyProbeDigestSalt) ^ fb);
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

// route 6.  (every slot word is kEmptyKey and every count 0 when the kernel starts.)  A record with a marker word or
// a zero count is counted, not inserted: the host refuses the set.  The largest value an atomicAdd has left behind is
// the largest count of the finished set (counts only grow; the host refuses a sum of 2^63 or more)
__global__ __launch_bounds__(256) void key_probe_build_strings_counted_kernel(const unsigned long long *__restrict__ recs,
                                                                              uint64_t n, unsigned long long *slots,
                                                                              unsigned long long *counts, uint64_t mask,
                                                                              KeyProbeCountedStringsBuild *b) {
  unsigned long long made_n = 0, digest = 0, markers = 0, zeros = 0, p0 = 0, p1 = 0, p2 = 0, cdigest = 0, most = 0;
  constexpr unsigned long long kPiece = (1ull << kKpPieceBits) - 1;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned long long fa = recs[4 * i], fb = recs[4 * i + 1], c = recs[4 * i + 2];
    if (fa == kEmptyKey || fb == kEmptyKey) {
      markers++;
      continue;
    }
    if (c == 0) {
      zeros++;
      continue;
    }
    p0 += c & kPiece;
    p1 += (c >> kKpPieceBits) & kPiece;
    p2 += c >> (2 * kKpPieceBits);
    cdigest += c * mix64(mix64(fa ^ kKeyProbeCountSalt) ^ fb);
    bool made;
    const int64_t at = kps_claim(slots, mask, fa, fb, &made);
    if (at < 0) continue;  // (cannot happen)
    const unsigned long long old = atomicAdd(&counts[at], c);  // (the count is added after the claim)
    most = old + c > most ? old + c : most;
    if (made) {
      made_n++;
      digest += mix64(mix64(fa ^ kKeyProbeDigestSalt) ^ fb);
    }
  }
  made_n = wave_sum(made_n);
  digest = wave_sum(digest);
  markers = wave_sum(markers);
  zeros = wave_sum(zeros);
  p0 = wave_sum(p0);
  p1 = wave_sum(p1);
  p2 = wave_sum(p2);
  cdigest = wave_sum(cdigest);
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    const unsigned long long o = __shfl_down(most, dlt, 64);
    most = o > most ? o : most;
  }
  if ((threadIdx.x & 63) == 0) {
    if (made_n) {
      atomicAdd(&b->keys, made_n);
      atomicAdd(&b->digest, digest);
    }
    if (markers) atomicAdd(&b->marker_records, markers);
    if (zeros) atomicAdd(&b->zero_counts, zeros);
    if (p0) atomicAdd(&b->sum_piece[0], p0);
    if (p1) atomicAdd(&b->sum_piece[1], p1);
    if (p2) atomicAdd(&b->sum_piece[2], p2);
    if (cdigest) atomicAdd(&b->count_digest, cdigest);
    if (most) atomicMax(&b->max_count, most);
  }
}

// ---- the probe -----------------------------------------------------------------------------------------------------------
// `Set`: KeyProbeStringSet, or KeyProbeCountedStringSet for a counted task, whose hits also sum their slots' counts
template <class Set>
__global__ __launch_bounds__(256) void key_probe_utf8_kernel(const Utf8ColDesc d, const Set set, const ValueCountsTable t) {
  constexpr bool kCounted = KpsCounted<Set>::value;
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t non_null = 0, matched = 0, too_long = 0;  // (a workgroup sees fewer than 2^32 rows: side_rows_fit)
  unsigned long long pairs = 0;  // (a counted set: cannot wrap, the host has refused such a batch)
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
      const int64_t at = kps_find(set, fa, fb);
      if (at >= 0) {
        matched++;
        if (kCounted) pairs += kps_times(set, at);
      } else if (len > t.max_value_bytes) too_long++;
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
  if (kCounted) {
    pairs = wave_sum(pairs);
    if (lane == 0 && pairs) atomicAdd(&t.words[kKpPairs], pairs);
  }
}

// `d`: the dictionary's values as a string column; a lane per entry with a non-zero count
template <class Set>
__global__ __launch_bounds__(256) void key_probe_dict_kernel(const Utf8ColDesc d,
                                                             const unsigned long long *__restrict__ cells, const Set set,
                                                             const ValueCountsTable t) {
  constexpr bool kCounted = KpsCounted<Set>::value;
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long non_null = 0, matched = 0, too_long = 0, pairs = 0;
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
    const int64_t at = kps_find(set, fa, fb);
    if (at >= 0) {
      matched += n;
      if (kCounted) pairs += n * kps_times(set, at);
    } else if (len > t.max_value_bytes) too_long += n;
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
  if (kCounted) {
    pairs = wave_sum(pairs);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(&t.words[kKpPairs], pairs);
  }
}

// ---- the parent side from rows -------------------------------------------------------------------------------------------
// the wave's live lanes take consecutive records behind *cursor (one atomic a wave, as key_probe_rows_kernel does) and
// write {fa, fb, times, 0}: two 16-byte stores a record.  Every lane of the wave calls this.  The host has made room
// for every row of the batch; a position is still held against `cap` before it is written.
__device__ __forceinline__ void kps_emit(bool live, unsigned long long fa, unsigned long long fb, unsigned long long times,
                                         int lane, unsigned long long *recs, uint64_t cap, unsigned long long *cursor) {
  const unsigned long long todo = __ballot(live);
  if (todo == 0) return;
  const int leader = __ffsll((long long)todo) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(todo));
  base = vc_shfl64(base, leader);
  if (!live) return;
  const uint64_t at = base + (uint64_t)__popcll(todo & ((1ull << lane) - 1));
  if (at >= cap) return;  // (cannot happen: cap counts every row the state has seen)
  ulonglong2 *out = (ulonglong2 *)recs + 2 * at;
  out[0] = make_ulonglong2(fa, fb);
  out[1] = make_ulonglong2(times, 0);
}

// a row per lane; words: the task's counters (kKpNonNull: the non-NULL rows, kKpPairs: the cursor)
__global__ __launch_bounds__(256) void key_probe_rows_utf8_kernel(const Utf8ColDesc d, unsigned long long *recs,
                                                                  uint64_t cap, unsigned long long *words) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // (the loops are uniform within the wave: every lane takes part in the ballot of every round)
  // First the wave's room: the non-NULL rows of all its rounds, from the validity bits alone, and ONE bump of the cursor
  // for them -- a bump a round would put every wave of a hundred million rows on one word's atomic unit.
  unsigned long long mine = 0;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    mine += (unsigned long long)__popcll(__ballot(i < d.length && (!vbits || TGX_VALID_BIT(vbits, d.offset + i))));
  }
  if (mine == 0) return;  // (the wave as one)
  unsigned long long at = 0;
  if (lane == 0) {
    at = atomicAdd(&words[kKpPairs], mine);
    atomicAdd(&words[kKpNonNull], mine);
  }
  at = vc_shfl64(at, 0);
  // then the records, a round's behind the round's before
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const int64_t slot = d.offset + i;
    const bool valid = i < d.length && (!vbits || TGX_VALID_BIT(vbits, slot));
    const unsigned long long todo = __ballot(valid);
    const uint64_t to = at + (uint64_t)__popcll(todo & ((1ull << lane) - 1));
    at += (unsigned long long)__popcll(todo);
    if (!valid || to >= cap) continue;  // (past cap: cannot happen, cap counts every row the state has seen)
    uintptr_t p;
    uint64_t len, fa, fb;
    utf8_value_of(d, slot, &p, &len);
    fingerprint(d.key, p, len, &fa, &fb);
    ulonglong2 *out = (ulonglong2 *)recs + 2 * to;
    out[0] = make_ulonglong2(fa, fb);
    out[1] = make_ulonglong2(1, 0);
  }
}

// `d`: the dictionary's values as a string column; a lane per entry, a record per entry with a non-zero count
__global__ __launch_bounds__(256) void key_probe_rows_dict_kernel(const Utf8ColDesc d,
                                                                  const unsigned long long *__restrict__ cells,
                                                                  unsigned long long *recs, uint64_t cap,
                                                                  unsigned long long *words) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long non_null = 0;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < d.length; base += stride) {
    const int64_t e = base + threadIdx.x;
    const int64_t slot = d.offset + e;
    const unsigned long long n = e < d.length ? cells[e] : 0;
    const bool live = n != 0 && (!vbits || TGX_VALID_BIT(vbits, slot));
    uint64_t fa = 0, fb = 0;
    if (live) {
      non_null += n;
      uintptr_t p;
      uint64_t len;
      utf8_value_of(d, slot, &p, &len);
      fingerprint(d.key, p, len, &fa, &fb);
    }
    kps_emit(live, fa, fb, n, lane, recs, cap, words + kKpPairs);
  }
  non_null = wave_sum(non_null);
  if (lane == 0 && non_null) atomicAdd(&words[kKpNonNull], non_null);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
void launch_key_probe_build_strings(const void *recs, uint64_t n, unsigned long long *slots, uint64_t mask,
                                    KeyProbeStringsBuild *b, hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_build_strings_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     (const unsigned long long *)recs, n, slots, mask, b);
}

void launch_key_probe_utf8(const Utf8ColDesc &d, const KeyProbeStringSet &set, const ValueCountsTable &t,
                           hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_utf8_kernel<KeyProbeStringSet>, dim3(grid_for((uint64_t)d.length)), dim3(256), 0, stream,
                     d, set, t);
}

void launch_key_probe_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                           const Utf8ColDesc &dict, unsigned long long *cells, const KeyProbeStringSet &set,
                           const ValueCountsTable &t, hipStream_t stream) {
  launch_dict_count(indices, validity, offset, length, dict.length, cells, stream);
  hipLaunchKernelGGL(key_probe_dict_kernel<KeyProbeStringSet>, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0,
                     stream, dict, cells, set, t);
}

// (the counts are zeroed by the host, beside the slots)
void launch_key_probe_build_strings_counted(const void *recs, uint64_t n, unsigned long long *slots,
                                            unsigned long long *counts, uint64_t mask, KeyProbeCountedStringsBuild *b,
                                            hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_build_strings_counted_kernel, dim3(grid_for(n)), dim3(256), 0, stream,
                     (const unsigned long long *)recs, n, slots, counts, mask, b);
}

void launch_key_probe_utf8_counted(const Utf8ColDesc &d, const KeyProbeCountedStringSet &set, const ValueCountsTable &t,
                                   hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_utf8_kernel<KeyProbeCountedStringSet>, dim3(grid_for((uint64_t)d.length)), dim3(256), 0,
                     stream, d, set, t);
}

void launch_key_probe_dict_counted(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                                   const Utf8ColDesc &dict, unsigned long long *cells,
                                   const KeyProbeCountedStringSet &set, const ValueCountsTable &t, hipStream_t stream) {
  launch_dict_count(indices, validity, offset, length, dict.length, cells, stream);
  hipLaunchKernelGGL(key_probe_dict_kernel<KeyProbeCountedStringSet>, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0,
                     stream, dict, cells, set, t);
}

void launch_key_probe_rows_utf8(const Utf8ColDesc &d, unsigned long long *recs, uint64_t cap, unsigned long long *words,
                                hipStream_t stream) {
  hipLaunchKernelGGL(key_probe_rows_utf8_kernel, dim3(grid_for((uint64_t)d.length)), dim3(256), 0, stream, d, recs, cap,
                     words);
}

void launch_key_probe_rows_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                                const Utf8ColDesc &dict, unsigned long long *cells, unsigned long long *recs, uint64_t cap,
                                unsigned long long *words, hipStream_t stream) {
  launch_dict_count(indices, validity, offset, length, dict.length, cells, stream);
  hipLaunchKernelGGL(key_probe_rows_dict_kernel, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0, stream, dict, cells,
                     recs, cap, words);
}

}  // namespace tgx
