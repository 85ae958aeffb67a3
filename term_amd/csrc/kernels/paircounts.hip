// paircounts.hip -- pair counts for gfx950 (TGX_CHECK_PAIR_COUNTS): how often each pair of cells of two columns occurs,
//   SELECT cell(x), cell(y), COUNT(*) FROM t WHERE x IS NOT NULL AND y IS NOT NULL GROUP BY 1, 2
// for a BOUNDED number of distinct pairs (the GROUP BY behind the three categorical branches of the reference's
// MutualInformationAnalyzer: TG/analyzers/advanced/mutual_information.rs:249-293).  A side is a string column (Utf8 /
// LargeUtf8 / Utf8View / Dictionary<Int32, Utf8>: the cell is the value's bytes) or a numeric one (the cell is its bin
// index, bin_count.h's bin_index).
//
//   pair_counts_kernel  a row per lane, in the shape of value_counts_utf8_kernel.  Both validities are read; a
//                       dictionary side follows the row's index to its entry (a NULL entry or an index outside the
//                       dictionary makes the row a NULL row).  A row with a string longer than max_value_bytes on
//                       either side is a long row; else a row whose binned side is a NaN or an infinity is a non-finite
//                       row; else a row whose bin index lies outside [0, bins] is out of range.  Every other row is
//                       reduced to its PAIR KEY: each string side to its keyed fingerprint, a binned side to its
//                       index, and the two 128-bit cells chained into one fingerprint the way the components of a
//                       tuple key are (distinct128.hip's tuple_fingerprint: a block per component, the last one under
//                       K1) -- never a concatenation of the bytes.  Equal keys are combined within the wave (up to four
//                       rounds, leaders first), the leaders insert into the workgroup's LDS table (count_table.h:
//                       two key words, a 32-bit count and a row that holds the pair -- one row index locates both
//                       sides, so the slot is VALUE_COUNTS's 28 bytes); a full table: straight into the global one.
//                       At the end every occupied LDS slot is one global insert with its count.  The lane that claims
//                       a GLOBAL slot copies both sides' bytes and lengths (or the bin) into the slot's place -- on the
//                       device, in the same stream.
//   pair_side_range_kernel  the range phase: MIN / MAX / n / non-finite rows of the numeric side over the rows where both
//                       sides are non-NULL.  Per-lane accumulators, wave shuffles, one 64-bit vector atomic per wave
//                       and word (the extremes as totalOrder keys, so MIN / MAX are integer atomics).  It walks by
//                       row index, not through row_walk.h: whether the other side is NULL can depend on the row's
//                       dictionary entry, which needs the row.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "fingerprint.h"

namespace tgx {

namespace {

// one side of one row
struct PairCell {
  bool valid;       // the row is non-NULL on this side
  bool too_long, non_finite, outside;
  uint64_t ca, cb;  // the cell as a component block of the pair key
  uintptr_t p;      // string side: the bytes
  uint32_t word;    // string side: the length; binned side: the bin index
};

__device__ __forceinline__ Utf8ColDesc pair_strings(const PairSide &s) {
  Utf8ColDesc d;
  d.offsets = s.str_offsets;
  d.data = s.str_data;
  d.views = s.str_views;
  d.buffers = s.str_buffers;
  d.large_offsets = s.large_offsets;
  return d;
}

// is row i non-NULL on this side?  *slot: where its value lies (the row's slot, or its dictionary entry's)
__device__ __forceinline__ bool pair_side_valid(const PairSide &s, int64_t i, int64_t *slot) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)s.validity;
  const int64_t row = s.offset + i;
  *slot = row;
  if (vbits && !TGX_VALID_BIT(vbits, row)) return false;
  if (!s.indices) return true;
  const int64_t e = (int64_t)((global_i32_ptr)(uintptr_t)s.indices)[row];
  if (e < 0 || e >= s.dict_length) return false;  // (never read: an index outside the dictionary is a NULL row)
  *slot = s.dict_offset + e;
  global_u8_ptr dbits = (global_u8_ptr)(uintptr_t)s.dict_validity;
  return !dbits || TGX_VALID_BIT(dbits, *slot);
}

__device__ __forceinline__ double pair_side_number(const PairSide &s, int64_t slot) {
  const int64_t bits = ((global_i64_ptr)(uintptr_t)s.values)[slot];
  return s.is_float ? __longlong_as_double(bits) : (double)bits;
}

// the cell of a non-NULL row; `fingerprinted`: also reduce a string to its fingerprint (not needed to find its bytes again)
template <bool kFingerprint>
__device__ __forceinline__ void pair_cell(const PairSide &s, const FpKey &key, int64_t slot, uint32_t max_value_bytes,
                                          PairCell *c) {
  c->too_long = c->non_finite = c->outside = false;
  c->ca = c->cb = 0;
  c->p = 0;
  c->word = 0;
  if (s.mode == kPairSideValue) {
    uint64_t len;
    utf8_value_of(pair_strings(s), slot, &c->p, &len);
    c->too_long = len > max_value_bytes;
    c->word = c->too_long ? 0u : (uint32_t)len;
    if (kFingerprint && !c->too_long) {
      fingerprint(key, c->p, len, &c->ca, &c->cb);
      c->cb |= 2;  // (the tag space of tuple_fingerprint: 0 NULL, 1 numeric, >= 2 string)
    }
  } else {
    const double v = pair_side_number(s, slot);
    c->non_finite = !(v - v == 0.0);
    const double f = bin_index(v, s.origin, s.width);
    c->outside = !c->non_finite && !(f >= 0.0 && f <= (double)s.bins);
    c->word = c->non_finite || c->outside ? 0u : (uint32_t)f;  // <= bins
    c->ca = (uint64_t)c->word;
    c->cb = 1;
  }
}

// the pair (fa, fb) with its weight into the task's global table; cells x, y hold what a new entry keeps
__device__ __forceinline__ void pair_insert_global(const PairCountsTable &t, unsigned long long fa,
                                                   unsigned long long fb, unsigned long long weight,
                                                   const PairCell &x, const PairCell &y) {
  uint64_t h = fa & t.mask;
  for (uint32_t probe = 0; probe < kValueCountsProbes; probe++) {
    unsigned long long a = vc_peek(&t.keys[h]);
    if (a == kEmptyKey) a = atomicCAS(&t.keys[h], (unsigned long long)kEmptyKey, fa);
    if (a == kEmptyKey || a == fa) {
      unsigned long long b = vc_peek(&t.keys2[h]);
      const bool made = b == kEmptyKey && (b = atomicCAS(&t.keys2[h], (unsigned long long)kEmptyKey, fb)) == kEmptyKey;
      if (made) {  // this lane made the entry: both sides' bytes (or bins) go to the slot's place
#pragma unroll
        for (int side = 0; side < 2; side++) {
          const PairCell &c = side ? y : x;
          t.cell[side][h] = c.word;
          if (t.store[side]) {  // (a string side: word = its length <= max_value_bytes)
            global_u8_ptr src = (global_u8_ptr)c.p;
            uint8_t *dst = t.store[side] + h * (uint64_t)t.max_value_bytes;
            for (uint32_t i = 0; i < c.word; i++) dst[i] = src[i];
          }
        }
      }
      if (made || b == fb) {
        atomicAdd(&t.counts[h], weight);
        return;
      }
    }
    h = (h + 1) & t.mask;
  }
  atomicAdd(&t.words[kPcOverflow], weight);
}

}  // namespace

struct PairLaunch {
  PairSide x, y;
  PairCountsTable t;
  int64_t length;
  FpKey key;
};

__global__ __launch_bounds__(kPairCountsBlock) void pair_counts_kernel(const PairLaunch L) {
  const PairCountsTable &t = L.t;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t both = 0, too_long = 0, non_finite = 0, outside = 0;  // (a workgroup sees fewer than 2^32 rows)
  __shared__ VcLdsStrings lds;
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += kPairCountsBlock) {
    lds.fa[s] = lds.fb[s] = kEmptyKey;
    lds.count[s] = 0;
  }
  __syncthreads();
  // (the loop is uniform within the wave: every lane takes part in the ballots of every round)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < L.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    PairCell x, y;
    x.valid = y.valid = false;
    unsigned long long fa = 0, fb = 0;
    bool live = false;
    if (i < L.length) {
      int64_t xs, ys;
      x.valid = pair_side_valid(L.x, i, &xs);
      y.valid = pair_side_valid(L.y, i, &ys);
      if (x.valid && y.valid) {
        both++;
        pair_cell<true>(L.x, L.key, xs, t.max_value_bytes, &x);
        pair_cell<true>(L.y, L.key, ys, t.max_value_bytes, &y);
        if (x.too_long || y.too_long) {
          too_long++;
        } else if (x.non_finite || y.non_finite) {
          non_finite++;
        } else if (x.outside || y.outside) {
          outside++;
        } else {
          Fp s;
          fp_init(s, L.key);
          fp_block(s, x.ca, x.cb);
          fp_last_padded(s, y.ca, y.cb, true, L.key);
          uint64_t a, b;
          fp_out(s, &a, &b);
          fa = a;
          fb = b;
          live = true;
        }
      }
    }
    unsigned long long todo = __ballot(live);
    bool pending = live;
    for (int round = 0; round < 4 && todo != 0; round++) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long la = vc_shfl64(fa, leader), lb = vc_shfl64(fb, leader);
      const bool mine = pending && fa == la && fb == lb;
      const unsigned long long same = __ballot(mine);
      if (lane == leader && !vc_insert_lds128(lds, fa, fb, (uint32_t)__popcll(same), (unsigned long long)i))
        pair_insert_global(t, fa, fb, (unsigned long long)__popcll(same), x, y);
      pending = pending && !mine;
      todo &= ~same;
    }
    if (pending && !vc_insert_lds128(lds, fa, fb, 1u, (unsigned long long)i)) pair_insert_global(t, fa, fb, 1ull, x, y);
  }
  __syncthreads();
  // every occupied LDS slot is one global insert with its count; its cells are those of the row it remembers
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += kPairCountsBlock) {
    const unsigned long long fa = lds.fa[s], fb = lds.fb[s];
    const unsigned int n = lds.count[s];
    if (fa == kEmptyKey || fb == kEmptyKey || n == 0) continue;
    const int64_t i = (int64_t)lds.row[s];
    int64_t xs, ys;
    PairCell x, y;
    (void)pair_side_valid(L.x, i, &xs);  // (the row was counted: both sides are non-NULL)
    (void)pair_side_valid(L.y, i, &ys);
    pair_cell<false>(L.x, L.key, xs, t.max_value_bytes, &x);
    pair_cell<false>(L.y, L.key, ys, t.max_value_bytes, &y);
    pair_insert_global(t, fa, fb, (unsigned long long)n, x, y);
  }
  tail_flush(both, too_long, t.words + kPcBoth);            // kPcBoth, kPcLong
  tail_flush(non_finite, outside, t.words + kPcNonFinite);  // kPcNonFinite, kPcOutOfRange
}

// the range phase: `num` is the numeric side, `other` the string side
__global__ __launch_bounds__(kPairCountsBlock) void pair_side_range_kernel(const PairSide num, const PairSide other,
                                                                      int64_t length, PairRangeAcc *__restrict__ acc) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  long long both = 0, n = 0, non_finite = 0;
  long long lo = INT64_MAX, hi = INT64_MIN;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < length; i += stride) {
    int64_t ns, os;
    if (!pair_side_valid(num, i, &ns) || !pair_side_valid(other, i, &os)) continue;
    both++;
    const double v = pair_side_number(num, ns);
    if (v - v == 0.0) {
      const long long k = (long long)f64_total_key(__double_as_longlong(v));
      n++;
      lo = k < lo ? k : lo;
      hi = k > hi ? k : hi;
    } else {
      non_finite++;
    }
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    both += __shfl_down(both, dlt, 64);
    n += __shfl_down(n, dlt, 64);
    non_finite += __shfl_down(non_finite, dlt, 64);
    const long long olo = __shfl_down(lo, dlt, 64), ohi = __shfl_down(hi, dlt, 64);
    lo = olo < lo ? olo : lo;
    hi = ohi > hi ? ohi : hi;
  }
  if ((threadIdx.x & 63) == 0) {
    if (both) atomicAdd((unsigned long long *)&acc->both, (unsigned long long)both);
    if (non_finite) atomicAdd((unsigned long long *)&acc->non_finite, (unsigned long long)non_finite);
    if (n) {
      atomicAdd((unsigned long long *)&acc->n, (unsigned long long)n);
      atomicMin(&acc->min_key, lo);
      atomicMax(&acc->max_key, hi);
    }
  }
}

static int pair_blocks(int64_t length) {
  const int64_t per_block = (int64_t)kPairCountsBlock * kPairCountsRowsPerLane;
  return (int)std::min<int64_t>(std::max<int64_t>(1, (length + per_block - 1) / per_block), kPairCountsMaxBlocks);
}

void launch_pair_counts(const PairSide &x, const PairSide &y, const PairCountsTable &t, int64_t length,
                        const FpKey &key, hipStream_t stream) {
  PairLaunch L;
  L.x = x;
  L.y = y;
  L.t = t;
  L.length = length;
  L.key = key;
  hipLaunchKernelGGL(pair_counts_kernel, dim3(pair_blocks(length)), dim3(kPairCountsBlock), 0, stream, L);
}

void launch_pair_side_range(const PairSide &num, const PairSide &other, int64_t length, PairRangeAcc *acc,
                            hipStream_t stream) {
  hipLaunchKernelGGL(pair_side_range_kernel, dim3(pair_blocks(length)), dim3(kPairCountsBlock), 0, stream, num, other,
                     length, acc);
}

}  // namespace tgx
