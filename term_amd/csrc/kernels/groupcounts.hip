// groupcounts.hip -- group counts for gfx950 (TGX_CHECK_GROUP_COUNTS): completeness per group,
//   SELECT g, COUNT(*) AS total_count, COUNT(col) AS non_null_count FROM t GROUP BY g
// for a BOUNDED number of groups (the GROUP BY behind the reference's CompletenessAnalyzer::with_grouping:
// TG/analyzers/basic/grouped_completeness.rs:160-200).
//
// The tables are valuecounts.hip's (count_table.h), with slots that carry several counters: the group's rows and, for
// each of the up to kGroupCountsMembers value columns ("members") that ride the walk, its rows whose value is non-NULL.
// The group column crosses HBM once however many members there are; a member adds one validity bit a row, and a
// member without a bitmap adds nothing.  A member's bitmap has its own Arrow offset.  Every route hands a wave 64
// consecutive rows, so a member's validity for the wave is one 64-bit window of its bitmap and what a key's lanes
// `same` count of the member is popcount(same & window).  The numeric route loads the windows as words (gc_window_of:
// one lane per (chunk, member), 64 windows a wave from two loads); the string and dictionary routes form them with a
// ballot of per-lane bits (vc_valid_window).
// Every row ends up in exactly one of: an entry, the NULL group (its key is NULL: SQL's NULL group, counted in two
// words, not in the table), the overflow counters (a probe sequence ran out), the long-rows counters -- and with it its
// non-NULL bit of every member.
//
//   numeric route     group_counts_i64_kernel<M>: a wave takes 64 consecutive rows at a time, eight such chunks in
//                     flight.  Equal keys are combined within the wave as value_counts_i64_kernel does (the first live
//                     key is broadcast; its leader adds popcount(same) to the total and popcount(same & window) to each
//                     member).  The LDS slot is key + 32-bit total + M 32-bit counts; the slot count follows M
//                     (group_counts_lds_slots).  The value whose bits are the free-slot marker and the NULL key are
//                     counted in words, per wave.  A key that finds the LDS table full goes to the global table with
//                     all its counters; at the end every occupied LDS slot is one global insert.
//   string route      group_counts_utf8_kernel: a row per lane; value_counts_utf8_kernel's rounds carry the members'
//                     windows; LDS slots remember a row; the lane that makes a global slot copies the bytes.
//   dictionary route  group_counts_dict_count_kernel counts per INDEX into cells of (1 + members) counters (in LDS while
//                     (1 + members) * entries fit kGroupCountsDictLdsCells, in global memory otherwise);
//                     group_counts_dict_insert_kernel takes a lane per used entry, fingerprints it and inserts it with
//                     all its counters.  Rows of NULL entries, and indices outside the dictionary, are NULL-key rows.
//   tuple route       group_counts_tuple_kernel<ARITY, NUMERIC>: GROUP BY the tuple of 2 .. 8 columns (a spec with a
//                     column list).  The string route's walk with tuple_key.h's fingerprint for the key -- the one
//                     DISTINCT and KEY_PROBE give the tuple -- and tuple_group.h's canonical bytes for the entry: the
//                     lane that makes a global slot encodes the row it holds, or the row the LDS slot remembers.  NULL
//                     is a value here: there are no NULL-key rows, (NULL, 'a') is a group like any other.
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

constexpr int kM = kGroupCountsMembers;

// `w` rows, nn[m] of them non-NULL in member m, into the counters of one class (kGc*Rows) of the walk
__device__ __forceinline__ void gc_add_words(const GroupCountsTable &t, const GroupMembers &mem, int word,
                                             unsigned long long w, const unsigned long long (&nn)[kM]) {
  if (w == 0) return;
  atomicAdd(&t.words[t.shared_word + word], w);
#pragma unroll
  for (int m = 0; m < kM; m++)
    if (m < mem.n && nn[m]) atomicAdd(&t.words[mem.word[m] + word + 1], nn[m]);
}

// ... into slot `s` of the walk's global table
__device__ __forceinline__ void gc_add_slot(const GroupCountsTable &t, const GroupMembers &mem, uint64_t s,
                                            unsigned long long w, const unsigned long long (&nn)[kM]) {
  atomicAdd(&t.totals[s], w);
#pragma unroll
  for (int m = 0; m < kM; m++)
    if (m < mem.n && nn[m]) atomicAdd(&t.non_null[(uint64_t)m * (t.mask + 1) + s], nn[m]);
}

// a numeric key with its counters into the walk's global table
__device__ __forceinline__ void gc_insert_global(const GroupCountsTable &t, const GroupMembers &mem,
                                                 unsigned long long key, unsigned long long w,
                                                 const unsigned long long (&nn)[kM]) {
  const int64_t s = vc_claim<uint64_t>(t.keys, t.mask, mix64(key ^ t.salt) & t.mask, key, kValueCountsProbes);
  if (s >= 0) gc_add_slot(t, mem, (uint64_t)s, w, nn);
  else gc_add_words(t, mem, kGcOverflowRows, w, nn);
}

// a string key (fa, fb) whose bytes are [p, p + len), with its counters
__device__ __forceinline__ void gc_insert_global128(const GroupCountsTable &t, const GroupMembers &mem,
                                                    unsigned long long fa, unsigned long long fb, unsigned long long w,
                                                    const unsigned long long (&nn)[kM], uintptr_t p, uint32_t len) {
  bool made;
  const int64_t s = vc_claim128<uint64_t>(t.keys, t.keys2, t.mask, fa & t.mask, fa, fb, kValueCountsProbes, &made);
  if (s < 0) {
    gc_add_words(t, mem, kGcOverflowRows, w, nn);
    return;
  }
  if (made) {  // this lane made the entry: its bytes go to the slot's place in the store
    global_u8_ptr src = (global_u8_ptr)p;
    uint8_t *dst = t.store + (uint64_t)s * (uint64_t)t.max_value_bytes;
    for (uint32_t i = 0; i < len; i++) dst[i] = src[i];
    t.lens[s] = len;
  }
  gc_add_slot(t, mem, (uint64_t)s, w, nn);
}

// a wave's counters of one class: `rows` lanes, of which the members' windows vm count theirs (wave-uniform)
struct GcWaveWords {
  uint32_t rows;  // (a wave sees fewer than 2^32 rows: side_rows_fit)
  uint32_t nn[kM];
};
__device__ __forceinline__ void gc_wave_clear(GcWaveWords &c) {
  c.rows = 0;
#pragma unroll
  for (int m = 0; m < kM; m++) c.nn[m] = 0;
}
__device__ __forceinline__ void gc_wave_count(GcWaveWords &c, unsigned long long lanes,
                                              const unsigned long long (&vm)[kM]) {
  if (lanes == 0) return;
  c.rows += (uint32_t)__popcll(lanes);
#pragma unroll
  for (int m = 0; m < kM; m++) c.nn[m] += (uint32_t)__popcll(lanes & vm[m]);
}
__device__ __forceinline__ void gc_wave_flush(const GroupCountsTable &t, const GroupMembers &mem, int word,
                                              const GcWaveWords &c) {
  if ((threadIdx.x & 63) != 0) return;
  unsigned long long nn[kM];
#pragma unroll
  for (int m = 0; m < kM; m++) nn[m] = c.nn[m];
  gc_add_words(t, mem, word, c.rows, nn);
}

// the members' windows for the wave whose lane holds row `row`
__device__ __forceinline__ void gc_windows(const GroupMembers &mem, int n, int64_t row, bool in,
                                           unsigned long long (&vm)[kM]) {
#pragma unroll
  for (int m = 0; m < kM; m++) vm[m] = m < n ? vc_valid_window(mem.validity[m], mem.offset[m], row, in) : 0ull;
}

// The numeric route's windows, read straight from the bitmaps: member `m`'s 64-bit window for the 64 rows of `chunk`,
// whatever the bitmap's Arrow offset -- the eight bytes that hold the window's first bits as one (unaligned) load and
// the ninth for the bits shifted out, byte by byte within the bitmap's last eight bytes; rows past `length` read 0
__device__ __forceinline__ unsigned long long gc_window_of(const GroupMembers &mem, int n, int m, int64_t chunk,
                                                           int64_t n_chunks, int64_t length) {
  if (m >= n || chunk >= n_chunks) return 0ull;
  const int64_t row0 = chunk * 64, rows = length - row0;
  const unsigned long long in_mask = rows >= 64 ? ~0ull : (1ull << rows) - 1;
  const uint8_t *vp = nullptr;
  int64_t off = 0;
#pragma unroll
  for (int mm = 0; mm < kM; mm++)
    if (mm == m) {
      vp = mem.validity[mm];
      off = mem.offset[mm];
    }
  if (vp == nullptr) return in_mask;
  struct __attribute__((packed)) Word {
    unsigned long long v;
  };
  typedef const Word __attribute__((address_space(1))) *word_ptr;
  global_u8_ptr v = (global_u8_ptr)(uintptr_t)vp;
  const int64_t bit = off + row0, b = bit >> 3, n_bytes = (off + length + 7) >> 3;
  const int sh = (int)(bit & 7);
  unsigned long long lo = 0, hi = 0;
  if (b + 9 <= n_bytes) {
    lo = ((word_ptr)(uintptr_t)(vp + b))->v;
    hi = v[b + 8];
  } else {
    for (int j = 0; j < 8; j++)
      if (b + j < n_bytes) lo |= (unsigned long long)v[b + j] << (8 * j);
  }
  return (sh ? (lo >> sh) | (hi << (64 - sh)) : lo) & in_mask;
}
__device__ __forceinline__ unsigned long long gc_readlane64(unsigned long long v, int lane) {  // `lane`: a constant
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((unsigned long long)hi << 32) | lo;
}

// what a lane adds: the leader of `same` for all its lanes, another lane for itself
__device__ __forceinline__ void gc_lane_counts(bool leader, unsigned long long same, int lane,
                                               const unsigned long long (&vm)[kM], unsigned long long *w,
                                               unsigned long long (&nn)[kM]) {
  *w = leader ? (unsigned long long)__popcll(same) : 1ull;
#pragma unroll
  for (int m = 0; m < kM; m++) nn[m] = leader ? (unsigned long long)__popcll(same & vm[m]) : (vm[m] >> lane) & 1ull;
}

}  // namespace

// ---- numeric route ------------------------------------------------------------------------------------------------------
template <int M>
__global__ __launch_bounds__(kGroupCountsBlock) void group_counts_i64_kernel(const ComomentColDesc d,
                                                                             const GroupMembers mem,
                                                                             const GroupCountsTable t) {
  constexpr uint32_t kSlots = group_counts_lds_slots(M);
  __shared__ unsigned long long lkeys[kSlots];
  __shared__ unsigned int ltotal[kSlots];
  __shared__ unsigned int lnn[M][kSlots];
  for (uint32_t s = threadIdx.x; s < kSlots; s += kGroupCountsBlock) {
    lkeys[s] = kEmptyKey;
    ltotal[s] = 0;
#pragma unroll
    for (int m = 0; m < M; m++) lnn[m][s] = 0;
  }
  __syncthreads();

  jb_i64_ptr x = (jb_i64_ptr)(uintptr_t)((const int64_t *)d.x + d.xoff);
  jb_u8_ptr xv = (jb_u8_ptr)(uintptr_t)d.xv;
  const int lane = threadIdx.x & 63;
  constexpr int kWaves = kGroupCountsBlock / 64;
  const int64_t n_chunks = (d.length + 63) >> 6;  // 64 consecutive rows each
  const int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * kWaves;
  GcWaveWords nulls, markers;
  gc_wave_clear(nulls);
  gc_wave_clear(markers);
  // (the loop is uniform within the wave: every lane takes part in the ballots of every chunk)
  constexpr int kChunks = 8;  // chunks a wave has in flight: lane u * 8 + m loads member m's window for chunk u
  static_assert(kChunks * kM == 64, "a (chunk, member) window a lane");
  for (int64_t c0 = wave; c0 < n_chunks; c0 += kChunks * waves) {
    int64_t keys[kChunks];
    bool in[kChunks], ok[kChunks];
    const unsigned long long window = gc_window_of(mem, M, lane & 7, c0 + (lane >> 3) * waves, n_chunks, d.length);
#pragma unroll
    for (int u = 0; u < kChunks; u++) {
      const int64_t i = (c0 + u * waves) * 64 + lane;
      in[u] = c0 + u * waves < n_chunks && i < d.length;
      keys[u] = in[u] ? x[i] : 0;
      ok[u] = in[u] && jb_valid(xv, d.xoff + (in[u] ? i : 0));
    }
#pragma unroll
    for (int u = 0; u < kChunks; u++) {
      if (c0 + u * waves >= n_chunks) break;
      const unsigned long long key = (unsigned long long)keys[u];
      unsigned long long vm[kM];
#pragma unroll
      for (int m = 0; m < kM; m++) vm[m] = m < M ? gc_readlane64(window, u * 8 + m) : 0ull;
      gc_wave_count(nulls, __ballot(in[u] && !ok[u]), vm);
      const bool is_marker = ok[u] && key == kEmptyKey;  // (the value whose bits are the free-slot marker)
      gc_wave_count(markers, __ballot(is_marker), vm);
      const bool live = ok[u] && !is_marker;
      const unsigned long long todo = __ballot(live);
      if (todo == 0) continue;
      // the wave's first live key is counted once for all the lanes that hold it; the others add for themselves
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long first = vc_shfl64(key, leader);
      const unsigned long long same = __ballot(live && key == first);
      if (!(lane == leader || (live && key != first))) continue;
      unsigned long long w, nn[kM];
      gc_lane_counts(lane == leader, same, lane, vm, &w, nn);
      const int64_t s = vc_claim<uint32_t>(lkeys, kSlots - 1, (uint32_t)mix64(key ^ t.salt) & (kSlots - 1), key,
                                           kValueCountsLdsProbes);
      if (s >= 0) {
        atomicAdd(&ltotal[s], (unsigned int)w);
#pragma unroll
        for (int m = 0; m < M; m++)
          if (nn[m]) atomicAdd(&lnn[m][s], (unsigned int)nn[m]);
      } else {
        gc_insert_global(t, mem, key, w, nn);  // (the workgroup's table is full around there)
      }
    }
  }
  gc_wave_flush(t, mem, kGcNullRows, nulls);
  gc_wave_flush(t, mem, kGcMarkerRows, markers);
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < kSlots; s += kGroupCountsBlock) {
    const unsigned long long key = lkeys[s];
    if (key == kEmptyKey) continue;
    unsigned long long nn[kM];
#pragma unroll
    for (int m = 0; m < kM; m++) nn[m] = m < M ? lnn[m < M ? m : 0][s] : 0ull;
    gc_insert_global(t, mem, key, ltotal[s], nn);
  }
}

// ---- string route -------------------------------------------------------------------------------------------------------
namespace {
// the workgroup's table of 128-bit keys: the two fingerprint words, a row that holds the key's value, the counters
struct GcLdsStrings {
  unsigned long long fa[kValueCountsStrLdsSlots], fb[kValueCountsStrLdsSlots], row[kValueCountsStrLdsSlots];
  unsigned int total[kValueCountsStrLdsSlots];
  unsigned int nn[kM][kValueCountsStrLdsSlots];
};
}  // namespace

__global__ __launch_bounds__(256) void group_counts_utf8_kernel(const Utf8ColDesc d, const GroupMembers mem,
                                                                const GroupCountsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  __shared__ GcLdsStrings lds;
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    lds.fa[s] = lds.fb[s] = kEmptyKey;
    lds.total[s] = 0;
#pragma unroll
    for (int m = 0; m < kM; m++) lds.nn[m][s] = 0;
  }
  __syncthreads();
  GcWaveWords nulls, longs;
  gc_wave_clear(nulls);
  gc_wave_clear(longs);
  // the key (fa, fb) of row `row`, bytes [p, p + len), with its counters: the workgroup's table, or the global one
  // where that is full around the key's place
  auto insert = [&](unsigned long long fa, unsigned long long fb, unsigned long long w,
                    const unsigned long long (&nn)[kM], int64_t row, uintptr_t p, uint32_t len) {
    bool made;
    const int64_t s = vc_claim128<uint32_t>(lds.fa, lds.fb, kValueCountsStrLdsSlots - 1,
                                            (uint32_t)fa & (kValueCountsStrLdsSlots - 1), fa, fb, kValueCountsLdsProbes,
                                            &made);
    if (s < 0) {
      gc_insert_global128(t, mem, fa, fb, w, nn, p, len);
      return;
    }
    if (made) lds.row[s] = (unsigned long long)row;  // (read after the workgroup's barrier)
    atomicAdd(&lds.total[s], (unsigned int)w);
#pragma unroll
    for (int m = 0; m < kM; m++)
      if (m < mem.n && nn[m]) atomicAdd(&lds.nn[m][s], (unsigned int)nn[m]);
  };
  // (the loop is uniform within the wave: a wave's lanes hold 64 consecutive rows and take part in every ballot)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const int64_t slot = d.offset + i;
    const bool in = i < d.length;
    const bool valid = in && (!vbits || TGX_VALID_BIT(vbits, slot));
    unsigned long long vm[kM];
    gc_windows(mem, mem.n, i, in, vm);
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
    gc_wave_count(nulls, __ballot(in && !valid), vm);
    gc_wave_count(longs, __ballot(too_long), vm);
    unsigned long long todo = __ballot(live);
    bool pending = live;
    for (int round = 0; round < 4 && todo != 0; round++) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long la = vc_shfl64(fa, leader), lb = vc_shfl64(fb, leader);
      const bool mine = pending && fa == la && fb == lb;
      const unsigned long long same = __ballot(mine);
      if (lane == leader) {
        unsigned long long w, nn[kM];
        gc_lane_counts(true, same, lane, vm, &w, nn);
        insert(fa, fb, w, nn, i, p, (uint32_t)len);
      }
      pending = pending && !mine;
      todo &= ~same;
    }
    if (pending) {
      unsigned long long w, nn[kM];
      gc_lane_counts(false, 0ull, lane, vm, &w, nn);
      insert(fa, fb, w, nn, i, p, (uint32_t)len);
    }
  }
  gc_wave_flush(t, mem, kGcNullRows, nulls);
  gc_wave_flush(t, mem, kGcLongRows, longs);
  __syncthreads();
  // every occupied LDS slot is one global insert with its counters; its bytes are those of the row it remembers
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    const unsigned long long fa = lds.fa[s], fb = lds.fb[s];
    const unsigned int n = lds.total[s];
    if (fa == kEmptyKey || fb == kEmptyKey || n == 0) continue;
    unsigned long long nn[kM];
#pragma unroll
    for (int m = 0; m < kM; m++) nn[m] = lds.nn[m][s];
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, d.offset + (int64_t)lds.row[s], &p, &len);
    gc_insert_global128(t, mem, fa, fb, (unsigned long long)n, nn, p, (uint32_t)len);
  }
}

// ---- tuple route --------------------------------------------------------------------------------------------------------
namespace {
// a tuple key (fa, fb) with its counters; `row` holds the key: the lane that makes the entry encodes it into the slot's
// place in the store
template <int ARITY, bool NUMERIC>
__device__ __forceinline__ void gc_insert_global_tuple(const GroupCountsTable &t, const GroupMembers &mem,
                                                       const KeyProbeTupleDesc &L, unsigned long long fa,
                                                       unsigned long long fb, unsigned long long w,
                                                       const unsigned long long (&nn)[kM], int64_t row) {
  bool made;
  const int64_t s = vc_claim128<uint64_t>(t.keys, t.keys2, t.mask, fa & t.mask, fa, fb, kValueCountsProbes, &made);
  if (s < 0) {
    gc_add_words(t, mem, kGcOverflowRows, w, nn);
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
  gc_add_slot(t, mem, (uint64_t)s, w, nn);
}
}  // namespace

template <int ARITY, bool NUMERIC>
__global__ __launch_bounds__(256) void group_counts_tuple_kernel(const KeyProbeTupleDesc L, const GroupMembers mem,
                                                                 const GroupCountsTable t) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  __shared__ GcLdsStrings lds;
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    lds.fa[s] = lds.fb[s] = kEmptyKey;
    lds.total[s] = 0;
#pragma unroll
    for (int m = 0; m < kM; m++) lds.nn[m][s] = 0;
  }
  __syncthreads();
  GcWaveWords longs;
  gc_wave_clear(longs);
  // the key (fa, fb) of row `row` with its counters: the workgroup's table, or the global one where that is full
  // around the key's place
  auto insert = [&](unsigned long long fa, unsigned long long fb, unsigned long long w,
                    const unsigned long long (&nn)[kM], int64_t row) {
    bool made;
    const int64_t s = vc_claim128<uint32_t>(lds.fa, lds.fb, kValueCountsStrLdsSlots - 1,
                                            (uint32_t)fa & (kValueCountsStrLdsSlots - 1), fa, fb, kValueCountsLdsProbes,
                                            &made);
    if (s < 0) {
      gc_insert_global_tuple<ARITY, NUMERIC>(t, mem, L, fa, fb, w, nn, row);
      return;
    }
    if (made) lds.row[s] = (unsigned long long)row;  // (read after the workgroup's barrier)
    atomicAdd(&lds.total[s], (unsigned int)w);
#pragma unroll
    for (int m = 0; m < kM; m++)
      if (m < mem.n && nn[m]) atomicAdd(&lds.nn[m][s], (unsigned int)nn[m]);
  };
  // (the loop is uniform within the wave: a wave's lanes hold 64 consecutive rows and take part in every ballot)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < L.d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < L.d.length;
    unsigned long long vm[kM];
    gc_windows(mem, mem.n, i, in, vm);
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
    gc_wave_count(longs, __ballot(too_long), vm);
    unsigned long long todo = __ballot(live);
    bool pending = live;
    for (int round = 0; round < 4 && todo != 0; round++) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned long long la = vc_shfl64(fa, leader), lb = vc_shfl64(fb, leader);
      const bool mine = pending && fa == la && fb == lb;
      const unsigned long long same = __ballot(mine);
      if (lane == leader) {
        unsigned long long w, nn[kM];
        gc_lane_counts(true, same, lane, vm, &w, nn);
        insert(fa, fb, w, nn, i);
      }
      pending = pending && !mine;
      todo &= ~same;
    }
    if (pending) {
      unsigned long long w, nn[kM];
      gc_lane_counts(false, 0ull, lane, vm, &w, nn);
      insert(fa, fb, w, nn, i);
    }
  }
  gc_wave_flush(t, mem, kGcLongRows, longs);
  __syncthreads();
  // every occupied LDS slot is one global insert with its counters; its bytes are those of the row it remembers
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    const unsigned long long fa = lds.fa[s], fb = lds.fb[s];
    const unsigned int n = lds.total[s];
    if (fa == kEmptyKey || fb == kEmptyKey || n == 0) continue;
    unsigned long long nn[kM];
#pragma unroll
    for (int m = 0; m < kM; m++) nn[m] = lds.nn[m][s];
    gc_insert_global_tuple<ARITY, NUMERIC>(t, mem, L, fa, fb, (unsigned long long)n, nn, (int64_t)lds.row[s]);
  }
}

// ---- dictionary route ---------------------------------------------------------------------------------------------------
// the rows' indices into cells[(1 + members) * dict_length]: cell c of entry e is cells[c * dict_length + e], c = 0 the
// rows, c = 1 + m member m's non-NULL rows.  A NULL index, and an index outside the dictionary (never read), make the
// row a NULL-key row
template <bool kLds>
__global__ __launch_bounds__(256) void group_counts_dict_count_kernel(const int32_t *__restrict__ indices,
                                                                      const uint8_t *__restrict__ validity,
                                                                      int64_t offset, int64_t length, int64_t dict_length,
                                                                      const GroupMembers mem,
                                                                      unsigned long long *__restrict__ cells,
                                                                      const GroupCountsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint32_t n_cells = (uint32_t)(1 + mem.n) * (uint32_t)dict_length;  // (kLds: at most kGroupCountsDictLdsCells)
  __shared__ unsigned int lcells[kLds ? kGroupCountsDictLdsCells : 1];
  if (kLds) {
    for (uint32_t c = threadIdx.x; c < n_cells; c += 256) lcells[c] = 0;
    __syncthreads();
  }
  GcWaveWords nulls;
  gc_wave_clear(nulls);
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const int64_t slot = offset + i;
    const bool in = i < length;
    bool live = in && (!vbits || TGX_VALID_BIT(vbits, slot));
    const int32_t idx = live ? indices[slot] : 0;
    live = live && idx >= 0 && (int64_t)idx < dict_length;
    unsigned long long vm[kM];
    gc_windows(mem, mem.n, i, in, vm);
    gc_wave_count(nulls, __ballot(in && !live), vm);
    const unsigned long long todo = __ballot(live);
    if (todo == 0) continue;
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t first = __shfl(idx, leader, 64);
    const unsigned long long same = __ballot(live && idx == first);
    if (!(lane == leader || (live && idx != first))) continue;
    unsigned long long w, nn[kM];
    gc_lane_counts(lane == leader, same, lane, vm, &w, nn);
    if (kLds) {
      atomicAdd(&lcells[idx], (unsigned int)w);
#pragma unroll
      for (int m = 0; m < kM; m++)
        if (m < mem.n && nn[m]) atomicAdd(&lcells[(uint32_t)(1 + m) * (uint32_t)dict_length + (uint32_t)idx], (unsigned int)nn[m]);
    } else {
      atomicAdd(&cells[idx], w);
#pragma unroll
      for (int m = 0; m < kM; m++)
        if (m < mem.n && nn[m]) atomicAdd(&cells[(int64_t)(1 + m) * dict_length + idx], nn[m]);
    }
  }
  gc_wave_flush(t, mem, kGcNullRows, nulls);
  if (kLds) {
    __syncthreads();
    bin_flush<256>(lcells, n_cells, cells);
  }
}

// `d`: the dictionary's values as a string column; a lane per entry that rows point at
__global__ __launch_bounds__(256) void group_counts_dict_insert_kernel(const Utf8ColDesc d, const GroupMembers mem,
                                                                       const unsigned long long *__restrict__ cells,
                                                                       const GroupCountsTable t) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d.length; e += stride) {
    const unsigned long long n = cells[e];
    if (n == 0) continue;
    unsigned long long nn[kM];
#pragma unroll
    for (int m = 0; m < kM; m++) nn[m] = m < mem.n ? cells[(int64_t)(1 + m) * d.length + e] : 0ull;
    const int64_t slot = d.offset + e;
    if (vbits && !TGX_VALID_BIT(vbits, slot)) {  // (rows of a NULL entry: NULL-key rows)
      gc_add_words(t, mem, kGcNullRows, n, nn);
      continue;
    }
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, slot, &p, &len);
    if (len > t.max_value_bytes) {
      gc_add_words(t, mem, kGcLongRows, n, nn);
      continue;
    }
    uint64_t fa, fb;
    fingerprint(d.key, p, len, &fa, &fb);
    gc_insert_global128(t, mem, fa, fb, n, nn, p, (uint32_t)len);
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_group_counts_i64(const ComomentColDesc &d, const GroupMembers &mem, const GroupCountsTable &t, int blocks,
                             hipStream_t stream) {
#define TGX_GC_CASE(M)                                                                                            \
  case M:                                                                                                         \
    hipLaunchKernelGGL(group_counts_i64_kernel<M>, dim3(blocks), dim3(kGroupCountsBlock), 0, stream, d, mem, t); \
    break;
  switch (mem.n) {
    TGX_GC_CASE(1)
    TGX_GC_CASE(2)
    TGX_GC_CASE(3)
    TGX_GC_CASE(4)
    TGX_GC_CASE(5)
    TGX_GC_CASE(6)
    TGX_GC_CASE(7)
    TGX_GC_CASE(8)
  }
#undef TGX_GC_CASE
}

void launch_group_counts_utf8(const Utf8ColDesc &d, const GroupMembers &mem, const GroupCountsTable &t,
                              hipStream_t stream) {
  hipLaunchKernelGGL(group_counts_utf8_kernel, dim3(grid_for((uint64_t)d.length)), dim3(256), 0, stream, d, mem, t);
}

// cells: (1 + mem.n) * dict.length 64-bit cells, zero
void launch_group_counts_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, const GroupMembers &mem, unsigned long long *cells,
                              const GroupCountsTable &t, hipStream_t stream) {
  if ((int64_t)(1 + mem.n) * dict.length <= (int64_t)kGroupCountsDictLdsCells)  // (fewer workgroups: each one flushes its cells once)
    hipLaunchKernelGGL(group_counts_dict_count_kernel<true>, dim3(std::min(grid_for((uint64_t)length), 1024)), dim3(256),
                       0, stream, indices, validity, offset, length, dict.length, mem, cells, t);
  else
    hipLaunchKernelGGL(group_counts_dict_count_kernel<false>, dim3(grid_for((uint64_t)length)), dim3(256), 0, stream,
                       indices, validity, offset, length, dict.length, mem, cells, t);
  if (dict.length > 0)
    hipLaunchKernelGGL(group_counts_dict_insert_kernel, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0, stream,
                       dict, mem, cells, t);
}

// `numeric`: every component is an 8-byte integer column (TupleCol::kind 0)
void launch_group_counts_tuples(const KeyProbeTupleDesc &L, bool numeric, const GroupMembers &mem,
                                const GroupCountsTable &t, hipStream_t stream) {
  const dim3 grid(grid_for((uint64_t)L.d.length)), block(256);
#define TGX_GCT_CASE(N, NUMERIC) \
  hipLaunchKernelGGL((group_counts_tuple_kernel<N, NUMERIC>), grid, block, 0, stream, L, mem, t);
  TGX_TUPLE_GROUP_DISPATCH(L.d.n_cols, numeric, TGX_GCT_CASE)
#undef TGX_GCT_CASE
}

}  // namespace tgx
