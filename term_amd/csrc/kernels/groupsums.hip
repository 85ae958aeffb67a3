// groupsums.hip -- group sums for gfx950 (TGX_CHECK_GROUP_SUMS): one side of a cross-table sum check,
//   SELECT g, COUNT(*) AS rows, COUNT(col) AS non_null, SUM(col) AS sum FROM t GROUP BY g
// for a BOUNDED number of groups (each side of the reference's CrossTableSumConstraint:
// TG/constraints/cross_table_sum.rs:251-262).
//
// The tables are groupcounts.hip's (count_table.h) with one value column a walk, whose slots carry the group's rows,
// its rows with a non-NULL value and the sum of those values.  The sum is 64 bits: an integer that wraps (kFloat =
// false: Int64 values, narrower ones widened) or an IEEE double (kFloat = true) -- a template parameter of every
// kernel, never a per-row branch.  Integer sums are added with 64-bit integer atomics and are exact whatever the
// order; float sums are added with 64-bit floating atomic adds, in LDS and in global memory, in the order the device
// happens to add.  A NULL value contributes nothing (its lane carries 0, which is +0.0 as a double: a group of -0.0
// alone may come out as +0.0).
// Every row ends up in exactly one of: an entry, the NULL group, the overflow counters (a probe sequence ran out), the
// long-rows counters -- with its non-NULL bit and its value.
//
//   numeric route     group_sums_i64_kernel: a wave takes 64 consecutive rows at a time, eight such chunks in flight
//                     (key and value loads).  The wave's first live key is combined once for all the lanes `same`
//                     that hold it: rows and non_null by popcount, the sum by a masked wave reduction (lanes outside
//                     `same` contribute 0; a six-step butterfly of 64-bit adds) -- one LDS atomic per counter for the
//                     leading key, not one per row; the other lanes add for themselves.  The LDS slot is key + 32-bit
//                     rows + 32-bit non_null + 64-bit sum (kGroupSumsLdsSlots of them).  A key that finds the LDS
//                     table full around its place goes to the global table with all three counters; at the end every
//                     occupied LDS slot is one global insert.
//   string route      group_sums_utf8_kernel: a row per lane; group_counts_utf8_kernel's rounds, each with the masked
//                     reduction for its leader.
//   dictionary route  group_sums_dict_count_kernel sums per INDEX into cells of (rows, non_null, sum) -- in LDS while
//                     the dictionary has at most kGroupSumsDictLdsEntries entries, in global memory otherwise;
//                     group_sums_dict_insert_kernel takes a lane per used entry, fingerprints it and inserts it.
//   tuple route       group_sums_tuple_kernel<kFloat, ARITY, NUMERIC>: GROUP BY the tuple of 2 .. 8 columns; the string
//                     route's walk with tuple_key.h's fingerprint for the key and tuple_group.h's canonical bytes for the
//                     entry, as group_counts_tuple_kernel has them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "fingerprint.h"
#include "row_walk.h"
#include "tuple_group.h"

namespace tgx {

namespace {

// the sum's 64 bits: a + b
template <bool kFloat>
__device__ __forceinline__ unsigned long long gs_plus(unsigned long long a, unsigned long long b) {
  if (kFloat)
    return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) +
                                                    __longlong_as_double((long long)b));
  return a + b;
}
// *p += bits, in LDS or in global memory
template <bool kFloat>
__device__ __forceinline__ void gs_atomic_add(unsigned long long *p, unsigned long long bits) {
  if (kFloat) unsafeAtomicAdd((double *)p, __longlong_as_double((long long)bits));
  else atomicAdd(p, bits);
}
__device__ __forceinline__ unsigned long long gs_shfl_xor64(unsigned long long v, int mask) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
  return ((unsigned long long)hi << 32) | lo;
}
// the sum of the wave's 64 lanes, in every lane (a lane that is not meant brings 0); every lane takes part
template <bool kFloat>
__device__ __forceinline__ unsigned long long gs_wave_sum(unsigned long long v) {
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) v = gs_plus<kFloat>(v, gs_shfl_xor64(v, dlt));
  return v;
}

// `w` rows, `nn` of them with a non-NULL value, which add up to `sum`, into the counters of one class (kGs*)
template <bool kFloat>
__device__ __forceinline__ void gs_add_words(const GroupSumsTable &t, int word, unsigned long long w,
                                             unsigned long long nn, unsigned long long sum) {
  if (w == 0) return;
  atomicAdd(&t.words[word], w);
  if (nn == 0) return;
  atomicAdd(&t.words[word + 1], nn);
  gs_atomic_add<kFloat>(&t.words[word + 2], sum);
}

// ... into slot `s` of the global table
template <bool kFloat>
__device__ __forceinline__ void gs_add_slot(const GroupSumsTable &t, uint64_t s, unsigned long long w,
                                            unsigned long long nn, unsigned long long sum) {
  atomicAdd(&t.rows[s], w);
  if (nn == 0) return;
  atomicAdd(&t.non_null[s], nn);
  gs_atomic_add<kFloat>(&t.sums[s], sum);
}

// a numeric key with its counters into the global table
template <bool kFloat>
__device__ __forceinline__ void gs_insert_global(const GroupSumsTable &t, unsigned long long key, unsigned long long w,
                                                 unsigned long long nn, unsigned long long sum) {
  const int64_t s = vc_claim<uint64_t>(t.keys, t.mask, mix64(key ^ t.salt) & t.mask, key, kValueCountsProbes);
  if (s >= 0) gs_add_slot<kFloat>(t, (uint64_t)s, w, nn, sum);
  else gs_add_words<kFloat>(t, kGsOverflow, w, nn, sum);
}

// a string key (fa, fb) whose bytes are [p, p + len), with its counters
template <bool kFloat>
__device__ __forceinline__ void gs_insert_global128(const GroupSumsTable &t, unsigned long long fa,
                                                    unsigned long long fb, unsigned long long w, unsigned long long nn,
                                                    unsigned long long sum, uintptr_t p, uint32_t len) {
  bool made;
  const int64_t s = vc_claim128<uint64_t>(t.keys, t.keys2, t.mask, fa & t.mask, fa, fb, kValueCountsProbes, &made);
  if (s < 0) {
    gs_add_words<kFloat>(t, kGsOverflow, w, nn, sum);
    return;
  }
  if (made) {  // this lane made the entry: its bytes go to the slot's place in the store
    global_u8_ptr src = (global_u8_ptr)p;
    uint8_t *dst = t.store + (uint64_t)s * (uint64_t)t.max_value_bytes;
    for (uint32_t i = 0; i < len; i++) dst[i] = src[i];
    t.lens[s] = len;
  }
  gs_add_slot<kFloat>(t, (uint64_t)s, w, nn, sum);
}

// a wave's counters of one class: rows and nn are wave-uniform (ballots), the sum is each lane's own until the flush
struct GsWaveClass {
  uint32_t rows, nn;  // (a wave sees fewer than 2^32 rows: side_rows_fit)
  unsigned long long sum;
};
__device__ __forceinline__ void gs_class_clear(GsWaveClass &c) {
  c.rows = c.nn = 0;
  c.sum = 0;
}
// `lanes`: the wave's rows of the class, `mine`: this lane's is one; vm: the wave's non-NULL values; v: this lane's
// value, 0 where it is NULL
template <bool kFloat>
__device__ __forceinline__ void gs_class_count(GsWaveClass &c, unsigned long long lanes, bool mine,
                                               unsigned long long vm, unsigned long long v) {
  if (lanes == 0) return;
  c.rows += (uint32_t)__popcll(lanes);
  c.nn += (uint32_t)__popcll(lanes & vm);
  if (mine) c.sum = gs_plus<kFloat>(c.sum, v);
}
// (every lane of the wave calls it)
template <bool kFloat>
__device__ __forceinline__ void gs_class_flush(const GroupSumsTable &t, int word, const GsWaveClass &c) {
  const unsigned long long sum = gs_wave_sum<kFloat>(c.sum);
  if ((threadIdx.x & 63) == 0) gs_add_words<kFloat>(t, word, c.rows, c.nn, sum);
}

// what the lanes `same` of the wave's leading key add up to (every lane calls it; `mine`: this lane is one of them)
template <bool kFloat>
__device__ __forceinline__ unsigned long long gs_same_sum(unsigned long long same, bool mine, unsigned long long v) {
  if (__popcll(same) <= 1) return v;  // (wave-uniform: the leader alone, which brings its own value)
  return gs_wave_sum<kFloat>(mine ? v : 0ull);
}

// row `row`'s value: *vok whether it is non-NULL, the bits (0 for a NULL)
__device__ __forceinline__ unsigned long long gs_value(const GroupSumsValue &val, int64_t row, bool in, bool *vok) {
  jb_i64_ptr y = (jb_i64_ptr)(uintptr_t)((const int64_t *)val.values + val.offset);
  jb_u8_ptr yv = (jb_u8_ptr)(uintptr_t)val.validity;
  *vok = in && jb_valid(yv, val.offset + (in ? row : 0));
  return *vok ? (unsigned long long)y[row] : 0ull;
}

}  // namespace

// ---- numeric route ------------------------------------------------------------------------------------------------------
// d: x the group column, y the value column (each with its own validity and Arrow offset)
template <bool kFloat>
__global__ __launch_bounds__(kGroupSumsBlock) void group_sums_i64_kernel(const ComomentColDesc d,
                                                                         const GroupSumsTable t) {
  constexpr uint32_t kSlots = kGroupSumsLdsSlots;
  __shared__ unsigned long long lkeys[kSlots];
  __shared__ unsigned long long lsum[kSlots];
  __shared__ unsigned int lrows[kSlots];
  __shared__ unsigned int lnn[kSlots];
  for (uint32_t s = threadIdx.x; s < kSlots; s += kGroupSumsBlock) {
    lkeys[s] = kEmptyKey;
    lsum[s] = 0;
    lrows[s] = 0;
    lnn[s] = 0;
  }
  __syncthreads();

  jb_i64_ptr x = (jb_i64_ptr)(uintptr_t)((const int64_t *)d.x + d.xoff);
  jb_i64_ptr y = (jb_i64_ptr)(uintptr_t)((const int64_t *)d.y + d.yoff);
  jb_u8_ptr xv = (jb_u8_ptr)(uintptr_t)d.xv;
  jb_u8_ptr yv = (jb_u8_ptr)(uintptr_t)d.yv;
  const int lane = threadIdx.x & 63;
  constexpr int kWaves = kGroupSumsBlock / 64;
  const int64_t n_chunks = (d.length + 63) >> 6;  // 64 consecutive rows each
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * kWaves;
  GsWaveClass nulls, markers;
  gs_class_clear(nulls);
  gs_class_clear(markers);
  // (the loop is uniform within the wave: every lane takes part in the ballots and reductions of every chunk)
  constexpr int kChunks = 8;  // chunks a wave has in flight
  for (int64_t c0 = wave; c0 < n_chunks; c0 += kChunks * waves) {
    int64_t keys[kChunks], vals[kChunks];
    bool in[kChunks], ok[kChunks], vok[kChunks];
#pragma unroll
    for (int u = 0; u < kChunks; u++) {
      const int64_t i = (c0 + u * waves) * 64 + lane;
      in[u] = c0 + u * waves < n_chunks && i < d.length;
      keys[u] = in[u] ? x[i] : 0;
      vals[u] = in[u] ? y[i] : 0;
      ok[u] = in[u] && jb_valid(xv, d.xoff + (in[u] ? i : 0));
      vok[u] = in[u] && jb_valid(yv, d.yoff + (in[u] ? i : 0));
    }
#pragma unroll
    for (int u = 0; u < kChunks; u++) {
      if (c0 + u * waves >= n_chunks) break;
      const unsigned long long key = (unsigned long long)keys[u];
      const unsigned long long v = vok[u] ? (unsigned long long)vals[u] : 0ull;
      const unsigned long long vm = __ballot(vok[u]);
      const bool is_null = in[u] && !ok[u];
      gs_class_count<kFloat>(nulls, __ballot(is_null), is_null, vm, v);
      const bool is_marker = ok[u] && key == kEmptyKey;  // (the value whose bits are the free-slot marker)
      gs_class_count<kFloat>(markers, __ballot(is_marker), is_marker, vm, v);
      const bool live = ok[u] && !is_marker;
      const unsigned long long todo = __ballot(live);
      if (todo == 0) continue;
      // the wave's first live key is combined once for all the lanes that hold it; the others add for themselves
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long first = vc_shfl64(key, leader);
      const bool mine = live && key == first;
      const unsigned long long same = __ballot(mine);
      const unsigned long long led = gs_same_sum<kFloat>(same, mine, v);
      if (!(lane == leader || (live && key != first))) continue;
      const bool leads = lane == leader;
      const unsigned int w = leads ? (unsigned int)__popcll(same) : 1u;
      const unsigned int nn = leads ? (unsigned int)__popcll(same & vm) : (unsigned int)((vm >> lane) & 1ull);
      const unsigned long long sum = leads ? led : v;
      const int64_t s = vc_claim<uint32_t>(lkeys, kSlots - 1, (uint32_t)mix64(key ^ t.salt) & (kSlots - 1), key,
                                           kValueCountsLdsProbes);
      if (s >= 0) {
        atomicAdd(&lrows[s], w);
        if (nn) {
          atomicAdd(&lnn[s], nn);
          gs_atomic_add<kFloat>(&lsum[s], sum);
        }
      } else {
        gs_insert_global<kFloat>(t, key, w, nn, sum);  // (the workgroup's table is full around there)
      }
    }
  }
  gs_class_flush<kFloat>(t, kGsNull, nulls);
  gs_class_flush<kFloat>(t, kGsMarker, markers);
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kSlots; s += kGroupSumsBlock) {
    const unsigned long long key = lkeys[s];
    if (key == kEmptyKey) continue;
    gs_insert_global<kFloat>(t, key, lrows[s], lnn[s], lsum[s]);
  }
}

// ---- string route -------------------------------------------------------------------------------------------------------
namespace {
// the workgroup's table of 128-bit keys: the two fingerprint words, a row that holds the key's value, the counters
struct GsLdsStrings {
  unsigned long long fa[kGroupSumsStrLdsSlots], fb[kGroupSumsStrLdsSlots], row[kGroupSumsStrLdsSlots];
  unsigned long long sum[kGroupSumsStrLdsSlots];
  unsigned int rows[kGroupSumsStrLdsSlots], nn[kGroupSumsStrLdsSlots];
};
}  // namespace

template <bool kFloat>
__global__ __launch_bounds__(256) void group_sums_utf8_kernel(const Utf8ColDesc d, const GroupSumsValue val,
                                                              const GroupSumsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  __shared__ GsLdsStrings lds;
  for (uint32_t s = threadIdx.x; s < kGroupSumsStrLdsSlots; s += 256) {
    lds.fa[s] = lds.fb[s] = kEmptyKey;
    lds.sum[s] = 0;
    lds.rows[s] = lds.nn[s] = 0;
  }
  __syncthreads();
  GsWaveClass nulls, longs;
  gs_class_clear(nulls);
  gs_class_clear(longs);
  // the key (fa, fb) of row `row`, bytes [p, p + len), with its counters: the workgroup's table, or the global one
  // where that is full around the key's place
  auto insert = [&](unsigned long long fa, unsigned long long fb, unsigned int w, unsigned int nn,
                    unsigned long long sum, int64_t row, uintptr_t p, uint32_t len) {
    bool made;
    const int64_t s = vc_claim128<uint32_t>(lds.fa, lds.fb, kGroupSumsStrLdsSlots - 1,
                                            (uint32_t)fa & (kGroupSumsStrLdsSlots - 1), fa, fb, kValueCountsLdsProbes,
                                            &made);
    if (s < 0) {
      gs_insert_global128<kFloat>(t, fa, fb, w, nn, sum, p, len);
      return;
    }
    if (made) lds.row[s] = (unsigned long long)row;  // (read after the workgroup's barrier)
    atomicAdd(&lds.rows[s], w);
    if (nn) {
      atomicAdd(&lds.nn[s], nn);
      gs_atomic_add<kFloat>(&lds.sum[s], sum);
    }
  };
  // (the loop is uniform within the wave: a wave's lanes hold 64 consecutive rows and take part in every ballot)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const int64_t slot = d.offset + i;
    const bool in = i < d.length;
    const bool valid = in && (!vbits || TGX_VALID_BIT(vbits, slot));
    bool vok;
    const unsigned long long v = gs_value(val, i, in, &vok);
    const unsigned long long vm = __ballot(vok);
    uintptr_t p = 0;
    uint64_t len = 0;
    unsigned long long fa = 0, fb = 0;
    bool live = false, too_long = false;
    if (valid) {
      utf8_value_of(d, slot, &p, &len);
      if (len > t.max_value_bytes) {
        too_long = true;
      } else {
        uint64_t a, b;
        fingerprint(d.key, p, len, &a, &b);
        fa = a;
        fb = b;
        live = true;
      }
    }
    const bool is_null = in && !valid;
    gs_class_count<kFloat>(nulls, __ballot(is_null), is_null, vm, v);
    gs_class_count<kFloat>(longs, __ballot(too_long), too_long, vm, v);
    unsigned long long todo = __ballot(live);
    bool pending = live;
    for (int round = 0; round < 4 && todo != 0; round++) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long la = vc_shfl64(fa, leader), lb = vc_shfl64(fb, leader);
      const bool mine = pending && fa == la && fb == lb;
      const unsigned long long same = __ballot(mine);
      const unsigned long long led = gs_same_sum<kFloat>(same, mine, v);
      if (lane == leader)
        insert(fa, fb, (unsigned int)__popcll(same), (unsigned int)__popcll(same & vm), led, i, p, (uint32_t)len);
      pending = pending && !mine;
      todo &= ~same;
    }
    if (pending) insert(fa, fb, 1u, (unsigned int)((vm >> lane) & 1ull), v, i, p, (uint32_t)len);
  }
  gs_class_flush<kFloat>(t, kGsNull, nulls);
  gs_class_flush<kFloat>(t, kGsLong, longs);
  __syncthreads();
  // every occupied LDS slot is one global insert with its counters; its bytes are those of the row it remembers
  for (uint32_t s = threadIdx.x; s < kGroupSumsStrLdsSlots; s += 256) {
    const unsigned long long fa = lds.fa[s], fb = lds.fb[s];
    const unsigned int n = lds.rows[s];
    if (fa == kEmptyKey || fb == kEmptyKey || n == 0) continue;
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, d.offset + (int64_t)lds.row[s], &p, &len);
    gs_insert_global128<kFloat>(t, fa, fb, (unsigned long long)n, lds.nn[s], lds.sum[s], p, (uint32_t)len);
  }
}

// ---- tuple route --------------------------------------------------------------------------------------------------------
namespace {
// a tuple key (fa, fb) with its counters; `row` holds the key: the lane that makes the entry encodes it into the slot's
// place in the store
template <bool kFloat, int ARITY, bool NUMERIC>
__device__ __forceinline__ void gs_insert_global_tuple(const GroupSumsTable &t, const KeyProbeTupleDesc &L,
                                                       unsigned long long fa, unsigned long long fb,
                                                       unsigned long long w, unsigned long long nn,
                                                       unsigned long long sum, int64_t row) {
  bool made;
  const int64_t s = vc_claim128<uint64_t>(t.keys, t.keys2, t.mask, fa & t.mask, fa, fb, kValueCountsProbes, &made);
  if (s < 0) {
    gs_add_words<kFloat>(t, kGsOverflow, w, nn, sum);
    return;
  }
  if (made) {
    const uint32_t nulls = kpt_nulls<ARITY, NUMERIC>(L, row);
    const uint64_t len = tuple_encoded_length<ARITY, NUMERIC>(L, row, nulls);
    if (len <= t.max_value_bytes) {  // (always: a longer row is a long row and comes to no slot)
      tuple_encode<ARITY, NUMERIC>(L, row, nulls, t.store + (uint64_t)s * (uint64_t)t.max_value_bytes);
      t.lens[s] = (uint32_t)len;
    }
  }
  gs_add_slot<kFloat>(t, (uint64_t)s, w, nn, sum);
}
}  // namespace

// L: the group columns; val: the value column (with its own validity and Arrow offset).  NULL is a value of a
// component: there are no NULL-key rows
template <bool kFloat, int ARITY, bool NUMERIC>
__global__ __launch_bounds__(256) void group_sums_tuple_kernel(const KeyProbeTupleDesc L, const GroupSumsValue val,
                                                               const GroupSumsTable t) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  __shared__ GsLdsStrings lds;
  for (uint32_t s = threadIdx.x; s < kGroupSumsStrLdsSlots; s += 256) {
    lds.fa[s] = lds.fb[s] = kEmptyKey;
    lds.sum[s] = 0;
    lds.rows[s] = lds.nn[s] = 0;
  }
  __syncthreads();
  GsWaveClass longs;
  gs_class_clear(longs);
  auto insert = [&](unsigned long long fa, unsigned long long fb, unsigned int w, unsigned int nn,
                    unsigned long long sum, int64_t row) {
    bool made;
    const int64_t s = vc_claim128<uint32_t>(lds.fa, lds.fb, kGroupSumsStrLdsSlots - 1,
                                            (uint32_t)fa & (kGroupSumsStrLdsSlots - 1), fa, fb, kValueCountsLdsProbes,
                                            &made);
    if (s < 0) {
      gs_insert_global_tuple<kFloat, ARITY, NUMERIC>(t, L, fa, fb, w, nn, sum, row);
      return;
    }
    if (made) lds.row[s] = (unsigned long long)row;  // (read after the workgroup's barrier)
    atomicAdd(&lds.rows[s], w);
    if (nn) {
      atomicAdd(&lds.nn[s], nn);
      gs_atomic_add<kFloat>(&lds.sum[s], sum);
    }
  };
  // (the loop is uniform within the wave: a wave's lanes hold 64 consecutive rows and take part in every ballot)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < L.d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < L.d.length;
    bool vok;
    const unsigned long long v = gs_value(val, i, in, &vok);
    const unsigned long long vm = __ballot(vok);
    unsigned long long fa = 0, fb = 0;
    bool live = false, too_long = false;
    if (in) {
      const uint32_t nulls = kpt_nulls<ARITY, NUMERIC>(L, i);  // (before any value is read)
      if (tuple_encoded_length<ARITY, NUMERIC>(L, i, nulls) > (uint64_t)t.max_value_bytes) {
        too_long = true;
      } else {
        uint64_t a, b;
        kpt_fingerprint<ARITY, NUMERIC>(L, i, nulls, &a, &b);
        fa = a;
        fb = b;
        live = true;
      }
    }
    gs_class_count<kFloat>(longs, __ballot(too_long), too_long, vm, v);
    unsigned long long todo = __ballot(live);
    bool pending = live;
    for (int round = 0; round < 4 && todo != 0; round++) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long la = vc_shfl64(fa, leader), lb = vc_shfl64(fb, leader);
      const bool mine = pending && fa == la && fb == lb;
      const unsigned long long same = __ballot(mine);
      const unsigned long long led = gs_same_sum<kFloat>(same, mine, v);
      if (lane == leader)
        insert(fa, fb, (unsigned int)__popcll(same), (unsigned int)__popcll(same & vm), led, i);
      pending = pending && !mine;
      todo &= ~same;
    }
    if (pending) insert(fa, fb, 1u, (unsigned int)((vm >> lane) & 1ull), v, i);
  }
  gs_class_flush<kFloat>(t, kGsLong, longs);
  __syncthreads();
  // every occupied LDS slot is one global insert with its counters; its bytes are those of the row it remembers
  for (uint32_t s = threadIdx.x; s < kGroupSumsStrLdsSlots; s += 256) {
    const unsigned long long fa = lds.fa[s], fb = lds.fb[s];
    const unsigned int n = lds.rows[s];
    if (fa == kEmptyKey || fb == kEmptyKey || n == 0) continue;
    gs_insert_global_tuple<kFloat, ARITY, NUMERIC>(t, L, fa, fb, (unsigned long long)n, lds.nn[s], lds.sum[s],
                                                   (int64_t)lds.row[s]);
  }
}

// ---- dictionary route ---------------------------------------------------------------------------------------------------
// the rows' indices into cells[3 * dict_length]: entry e has its rows at cells[e], its non-NULL values at
// cells[dict_length + e], their sum at cells[2 * dict_length + e].  A NULL index, and an index outside the dictionary
// (never read), make the row a NULL-key row
template <bool kFloat, bool kLds>
__global__ __launch_bounds__(256) void group_sums_dict_count_kernel(const int32_t *__restrict__ indices,
                                                                    const uint8_t *__restrict__ validity,
                                                                    int64_t offset, int64_t length, int64_t dict_length,
                                                                    const GroupSumsValue val,
                                                                    unsigned long long *__restrict__ cells,
                                                                    const GroupSumsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  constexpr uint32_t kCells = kLds ? kGroupSumsDictLdsEntries : 1;  // (kLds: dict_length is at most that)
  __shared__ unsigned long long lsum[kCells];
  __shared__ unsigned int lrows[kCells], lnn[kCells];
  if (kLds) {
    for (uint32_t c = threadIdx.x; c < (uint32_t)dict_length; c += 256) {
      lsum[c] = 0;
      lrows[c] = lnn[c] = 0;
    }
    __syncthreads();
  }
  GsWaveClass nulls;
  gs_class_clear(nulls);
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const int64_t slot = offset + i;
    const bool in = i < length;
    bool live = in && (!vbits || TGX_VALID_BIT(vbits, slot));
    const int32_t idx = live ? indices[slot] : 0;
    live = live && idx >= 0 && (int64_t)idx < dict_length;
    bool vok;
    const unsigned long long v = gs_value(val, i, in, &vok);
    const unsigned long long vm = __ballot(vok);
    const bool is_null = in && !live;
    gs_class_count<kFloat>(nulls, __ballot(is_null), is_null, vm, v);
    const unsigned long long todo = __ballot(live);
    if (todo == 0) continue;
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t first = __shfl(idx, leader, 64);
    const bool mine = live && idx == first;
    const unsigned long long same = __ballot(mine);
    const unsigned long long led = gs_same_sum<kFloat>(same, mine, v);
    if (!(lane == leader || (live && idx != first))) continue;
    const bool leads = lane == leader;
    const unsigned int w = leads ? (unsigned int)__popcll(same) : 1u;
    const unsigned int nn = leads ? (unsigned int)__popcll(same & vm) : (unsigned int)((vm >> lane) & 1ull);
    const unsigned long long sum = leads ? led : v;
    if (kLds) {
      atomicAdd(&lrows[idx], w);
      if (nn) {
        atomicAdd(&lnn[idx], nn);
        gs_atomic_add<kFloat>(&lsum[idx], sum);
      }
    } else {
      atomicAdd(&cells[idx], (unsigned long long)w);
      if (nn) {
        atomicAdd(&cells[dict_length + idx], (unsigned long long)nn);
        gs_atomic_add<kFloat>(&cells[2 * dict_length + idx], sum);
      }
    }
  }
  gs_class_flush<kFloat>(t, kGsNull, nulls);
  if (kLds) {
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < (uint32_t)dict_length; c += 256) {
      const unsigned int w = lrows[c], nn = lnn[c];
      if (w == 0) continue;
      atomicAdd(&cells[c], (unsigned long long)w);
      if (nn) {
        atomicAdd(&cells[dict_length + c], (unsigned long long)nn);
        gs_atomic_add<kFloat>(&cells[2 * dict_length + c], lsum[c]);
      }
    }
  }
}

// `d`: the dictionary's values as a string column; a lane per entry that rows point at
template <bool kFloat>
__global__ __launch_bounds__(256) void group_sums_dict_insert_kernel(const Utf8ColDesc d,
                                                                     const unsigned long long *__restrict__ cells,
                                                                     const GroupSumsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d.length; e += stride) {
    const unsigned long long n = cells[e];
    if (n == 0) continue;
    const unsigned long long nn = cells[d.length + e], sum = cells[2 * d.length + e];
    const int64_t slot = d.offset + e;
    if (vbits && !TGX_VALID_BIT(vbits, slot)) {  // (rows of a NULL entry: NULL-key rows)
      gs_add_words<kFloat>(t, kGsNull, n, nn, sum);
      continue;
    }
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, slot, &p, &len);
    if (len > t.max_value_bytes) {
      gs_add_words<kFloat>(t, kGsLong, n, nn, sum);
      continue;
    }
    uint64_t fa, fb;
    fingerprint(d.key, p, len, &fa, &fb);
    gs_insert_global128<kFloat>(t, fa, fb, n, nn, sum, p, (uint32_t)len);
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_group_sums_i64(const ComomentColDesc &d, const GroupSumsTable &t, bool is_float, int blocks,
                           hipStream_t stream) {
  if (is_float)
    hipLaunchKernelGGL(group_sums_i64_kernel<true>, dim3(blocks), dim3(kGroupSumsBlock), 0, stream, d, t);
  else
    hipLaunchKernelGGL(group_sums_i64_kernel<false>, dim3(blocks), dim3(kGroupSumsBlock), 0, stream, d, t);
}

void launch_group_sums_utf8(const Utf8ColDesc &d, const GroupSumsValue &val, const GroupSumsTable &t, bool is_float,
                            hipStream_t stream) {
  const dim3 grid(grid_for((uint64_t)d.length));
  if (is_float) hipLaunchKernelGGL(group_sums_utf8_kernel<true>, grid, dim3(256), 0, stream, d, val, t);
  else hipLaunchKernelGGL(group_sums_utf8_kernel<false>, grid, dim3(256), 0, stream, d, val, t);
}

namespace {
template <bool kFloat>
void dict_launches(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                   const Utf8ColDesc &dict, const GroupSumsValue &val, unsigned long long *cells,
                   const GroupSumsTable &t, hipStream_t stream) {
  if (dict.length <= (int64_t)kGroupSumsDictLdsEntries)  // (fewer workgroups: each one flushes its cells once)
    hipLaunchKernelGGL((group_sums_dict_count_kernel<kFloat, true>), dim3(std::min(grid_for((uint64_t)length), 1024)),
                       dim3(256), 0, stream, indices, validity, offset, length, dict.length, val, cells, t);
  else
    hipLaunchKernelGGL((group_sums_dict_count_kernel<kFloat, false>), dim3(grid_for((uint64_t)length)), dim3(256), 0,
                       stream, indices, validity, offset, length, dict.length, val, cells, t);
  if (dict.length > 0)
    hipLaunchKernelGGL(group_sums_dict_insert_kernel<kFloat>, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0,
                       stream, dict, cells, t);
}
}  // namespace

// cells: 3 * dict.length 64-bit cells, zero
void launch_group_sums_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                            const Utf8ColDesc &dict, const GroupSumsValue &val, unsigned long long *cells,
                            const GroupSumsTable &t, bool is_float, hipStream_t stream) {
  if (is_float) dict_launches<true>(indices, validity, offset, length, dict, val, cells, t, stream);
  else dict_launches<false>(indices, validity, offset, length, dict, val, cells, t, stream);
}

namespace {
template <bool kFloat>
void tuple_launches(const KeyProbeTupleDesc &L, bool numeric, const GroupSumsValue &val, const GroupSumsTable &t,
                    hipStream_t stream) {
  const dim3 grid(grid_for((uint64_t)L.d.length)), block(256);
#define TGX_GST_CASE(N, NUMERIC) \
  hipLaunchKernelGGL((group_sums_tuple_kernel<kFloat, N, NUMERIC>), grid, block, 0, stream, L, val, t);
  TGX_TUPLE_GROUP_DISPATCH(L.d.n_cols, numeric, TGX_GST_CASE)
#undef TGX_GST_CASE
}
}  // namespace

// `numeric`: every component is an 8-byte integer column (TupleCol::kind 0)
void launch_group_sums_tuples(const KeyProbeTupleDesc &L, bool numeric, const GroupSumsValue &val,
                              const GroupSumsTable &t, bool is_float, hipStream_t stream) {
  if (is_float) tuple_launches<true>(L, numeric, val, t, stream);
  else tuple_launches<false>(L, numeric, val, t, stream);
}

}  // namespace tgx
