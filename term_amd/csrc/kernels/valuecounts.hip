// valuecounts.hip -- value counts for gfx950 (TGX_CHECK_VALUE_COUNTS): how often each value of one column occurs,
//   SELECT col, COUNT(*) FROM t WHERE col IS NOT NULL GROUP BY col
// for a BOUNDED number of distinct values (the GROUP BY behind the reference's HistogramConstraint and EntropyAnalyzer:
// TG/constraints/histogram.rs:205-391, TG/analyzers/advanced/entropy.rs:192-335).
//
// One open-addressing table primitive (vc_claim / vc_insert; count_table.h), used at two places: in LDS per workgroup with 32-bit counts
// (a workgroup sees fewer than 2^32 rows: side_rows_fit) and in global memory per task with 64-bit counts
// (ValueCountsTable, device_types.h).  A slot is claimed by CAS on its key word; a string key (two fingerprint words)
// claims the first word by CAS and then settles the second by CAS: the slot is the key's when both come back free or
// equal, otherwise probing goes on.  A probe sequence that runs out adds the key's weight to the overflow counter, so
// every non-NULL row ends up in exactly one of: an entry, the overflow counter, the long-rows counter.
//
//   numeric route     value_counts_i64_kernel walks the column once (row_walk.h's single-column form: 8 B + 1 bit per row).
//                     Equal keys are combined within the wave before the LDS atomic (the wave's first live key is
//                     broadcast, its lanes are counted with a ballot: a constant column is one LDS atomic per wave and
//                     64 rows).  The table has 8192 slots (96 KiB: one 1024-thread workgroup a CU; 4096 slots and two
//                     512-thread workgroups measured the same up to 16 values and 1.2 - 2.5 times slower from 1000
//                     values on).  A key that finds the workgroup's LDS table full goes to the global table directly; at the
//                     end every occupied LDS slot is one global insert with its count.
//   string route      value_counts_utf8_kernel: a row per lane (Utf8 / LargeUtf8 / Utf8View through utf8_value's three
//                     layouts).  Rows longer than max_value_bytes are counted as long rows; the others are reduced to
//                     their keyed fingerprint, equal fingerprints are combined within the wave (up to four rounds), and
//                     the leaders insert into the workgroup's LDS table, whose slots also remember a row that holds
//                     the value (a full table: straight into the global one).  At the end every occupied LDS slot is
//                     one global insert with its count.  The lane that claims a GLOBAL slot copies the value's bytes
//                     and length into the slot's place in the value store -- on the device, in the same stream.
//   dictionary route  value_counts_dict_count_kernel (dict_count.h) counts the INDICES into one 64-bit cell per dictionary entry (up to
//                     16384 entries through 32-bit cells in LDS, bin_count.h's idiom; above that with global atomics);
//                     value_counts_dict_insert_kernel then takes a lane per entry with a non-zero count, fingerprints the
//                     entry and inserts it with its count (rows of NULL entries are counted nowhere: they are NULLs).
//                     Entries that repeat a value, and the dictionaries of different batches, unite by value.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "dict_count.h"
#include "fingerprint.h"
#include "row_walk.h"

namespace tgx {

namespace {

// ---- the table primitive (vc_peek, vc_claim, the LDS table of 128-bit keys, the global insert of one and the wave's
// combining of equal ones: count_table.h) ---------------------------------------------------------------------------------
// a numeric key with its weight into the task's global table
__device__ __forceinline__ void vc_insert_global(const ValueCountsTable &t, unsigned long long key,
                                                 unsigned long long weight) {
  const int64_t s = vc_claim<uint64_t>(t.keys, t.mask, mix64(key ^ t.salt) & t.mask, key, kValueCountsProbes);
  if (s >= 0) atomicAdd(&t.counts[s], weight);
  else atomicAdd(&t.words[kVcOverflow], weight);
}

}  // namespace

// ---- numeric route ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kValueCountsBlock) void value_counts_i64_kernel(const ComomentColDesc d,
                                                                             const ValueCountsTable t) {
  __shared__ unsigned long long lkeys[kValueCountsLdsSlots];
  __shared__ unsigned int lcounts[kValueCountsLdsSlots];
  for (uint32_t s = threadIdx.x; s < kValueCountsLdsSlots; s += kValueCountsBlock) {
    lkeys[s] = kEmptyKey;
    lcounts[s] = 0;
  }
  __syncthreads();

  const int lane = threadIdx.x & 63;
  uint32_t non_null = 0, marker = 0;  // (a workgroup sees fewer than 2^32 rows: side_rows_fit)
  jb_for_rows_single(d, [&](int64_t v, bool ok) {
    const unsigned long long key = (unsigned long long)v;
    non_null += ok ? 1u : 0u;
    const bool is_marker = ok && key == kEmptyKey;  // (the value whose bits are the free-slot marker)
    marker += is_marker ? 1u : 0u;
    const bool live = ok && !is_marker;
    const unsigned long long todo = __ballot(live);
    if (todo == 0) return;
    // the wave's first live key is counted once for all the lanes that hold it; the others add for themselves
    const int leader = __ffsll((long long)todo) - 1;
    const unsigned long long first = vc_shfl64(key, leader);
    const unsigned long long same = __ballot(live && key == first);
    const bool adds = lane == leader || (live && key != first);
    if (!adds) return;
    const uint32_t weight = lane == leader ? (uint32_t)__popcll(same) : 1u;
    const int64_t s = vc_claim<uint32_t>(lkeys, kValueCountsLdsSlots - 1,
                                         (uint32_t)mix64(key ^ t.salt) & (kValueCountsLdsSlots - 1), key,
                                         kValueCountsLdsProbes);
    if (s >= 0) atomicAdd(&lcounts[s], weight);
    else vc_insert_global(t, key, weight);  // (the workgroup's table is full around there)
  });
  tail_flush(non_null, marker, t.words);  // kVcNonNull, kVcMarker
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kValueCountsLdsSlots; s += kValueCountsBlock) {
    const unsigned long long key = lkeys[s];
    if (key != kEmptyKey) vc_insert_global(t, key, lcounts[s]);
  }
}

// ---- string route -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void value_counts_utf8_kernel(const Utf8ColDesc d, const ValueCountsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t non_null = 0, too_long = 0;
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
      if (len > t.max_value_bytes) {
        too_long++;
      } else {
        uint64_t a, b;
        fingerprint(d.key, p, len, &a, &b);
        fa = a;
        fb = b;
        live = true;
      }
    }
    vc_wave_combine128(live, fa, fb, lane, [&](uint32_t weight) {
      if (!vc_insert_lds128(lds, fa, fb, weight, (unsigned long long)i))
        vc_insert_global128(t, fa, fb, (unsigned long long)weight, p, (uint32_t)len, &t.words[kVcOverflow]);
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
    vc_insert_global128(t, fa, fb, (unsigned long long)n, p, (uint32_t)len, &t.words[kVcOverflow]);
  }
  // (tail_flush adds to out[0] and out[1], non-zero sums only: both pairs lie within the task's four words)
  tail_flush(non_null, 0u, t.words + kVcNonNull);
  tail_flush(too_long, 0u, t.words + kVcLong);
}

// ---- dictionary route ---------------------------------------------------------------------------------------------------
// (the rows' indices into cells[dict_length]: dict_count.h)
// `d`: the dictionary's values as a string column; a lane per entry with a non-zero count
__global__ __launch_bounds__(256) void value_counts_dict_insert_kernel(const Utf8ColDesc d,
                                                                       const unsigned long long *__restrict__ cells,
                                                                       const ValueCountsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d.length; e += stride) {
    const unsigned long long n = cells[e];
    const int64_t slot = d.offset + e;
    if (n == 0 || (vbits && !TGX_VALID_BIT(vbits, slot))) continue;
    atomicAdd(&t.words[kVcNonNull], n);
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, slot, &p, &len);
    if (len > t.max_value_bytes) {
      atomicAdd(&t.words[kVcLong], n);
      continue;
    }
    uint64_t fa, fb;
    fingerprint(d.key, p, len, &fa, &fb);
    vc_insert_global128(t, fa, fb, n, p, (uint32_t)len, &t.words[kVcOverflow]);
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_value_counts_i64(const ComomentColDesc &d, const ValueCountsTable &t, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(value_counts_i64_kernel, dim3(blocks), dim3(kValueCountsBlock), 0, stream, d, t);
}

void launch_value_counts_utf8(const Utf8ColDesc &d, const ValueCountsTable &t, hipStream_t stream) {
  hipLaunchKernelGGL(value_counts_utf8_kernel, dim3(grid_for((uint64_t)d.length)), dim3(256), 0, stream, d, t);
}

void launch_value_counts_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, unsigned long long *cells, const ValueCountsTable &t,
                              hipStream_t stream) {
  launch_dict_count(indices, validity, offset, length, dict.length, cells, stream);
  hipLaunchKernelGGL(value_counts_dict_insert_kernel, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0, stream, dict,
                     cells, t);
}

}  // namespace tgx
