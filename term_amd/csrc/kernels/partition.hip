// partition.hip -- the range-partitioned population of a DISTINCT task's range bitmap on gfx950: the fast path for big
// batches of a dense-range Int64 column (the bitmap itself, the hash set and the key lists are in distinct.hip).
//   partition_init_kernel   clears the pass's cursors and totals and probes whether the keys arrive in order
//   partition_kernel        phase 1: buckets the keys' offsets into per-slice lists (plain / CLUSTERED form)
//   bucket_apply_kernel     phase 2: replays each list against its slice of the bitmap held in LDS
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_types.h"
#include "distinct_types.h"
#include "keyset_device.h"

namespace tgx {

// ---------------------------------------------------------------------------------------------
// Range-partitioned bitmap population: the fast path for big batches of a dense-range Int64 column.
// A global atomicOr per row runs at ~27 G rows/s on MI355X (memory-side atomics); replaying bucketed
// keys against an LDS-resident slice of the bitmap is bounded by HBM traffic instead:
//   phase 1 reads 8 B/row and writes 4 B/row, phase 2 reads 4 B/row (+ the bitmap once).
//
// Phase 1.  One 1024-thread workgroup takes tiles of 32768 rows.  Each key gets its bucket and an
// in-tile rank from an LDS histogram (ds_add_rtn); a block scan turns the histogram into offsets and
// the tile is counting-sorted by bucket inside LDS.  The workgroup then reserves room in every bucket
// list it touches with ONE global atomicAdd per (tile, bucket) and each wave streams whole runs out,
// padded to 16 slots so that every global store is a full, 64-byte aligned chunk (scattered 4-byte
// stores ran this kernel 7x slower: 11.9 ms vs 1.6 ms without them at 1 G rows).  A list that is full
// (skewed data) spills to the global atomicOr path, so the result is exact for any distribution and
// only the speed depends on the spread.
// loads one tile's keys + validity into registers.  Validity bytes are requested BEFORE the keys so that
// turning them into the `ok` mask only waits for those (vmcnt retires in order) and the 16-byte key loads
// stay in flight.
template <int THREADS, int KPT, bool VALIDITY>
__device__ __forceinline__ void partition_load_tile(const PartitionParams &p, int64_t tile, bool wide,
                                                    int64_t (&key)[KPT], uint32_t &ok) {
  constexpr int kPartitionThreads = THREADS;  // (shadows the namespace constant inside this function)
  constexpr int kTile = kPartitionThreads * KPT;
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)p.values + p.offset);
  // VALIDITY = false: the column has no validity bitmap (its own instance: no byte loads, fewer live registers)
  global_u8_ptr vbits = VALIDITY ? (global_u8_ptr)(uintptr_t)p.validity : (global_u8_ptr) nullptr;
  const uint32_t tid = threadIdx.x;
  const int64_t row0 = tile * kTile;
  const bool full = row0 + kTile <= p.length;
  ok = 0;
  if (full && wide) {
    // lane holds rows row0 + (j/2)*2*T + 2*tid + (j&1): one global_load_dwordx4 per pair
    typedef long long i64x2 __attribute__((ext_vector_type(2)));
    typedef const i64x2 __attribute__((address_space(1))) *global_i64x2_ptr;
    global_i64x2_ptr pv = (global_i64x2_ptr)(vals + row0) + tid;
    const bool pair_bytes = vbits && (p.offset & 1) == 0;  // both rows of a pair share a validity byte
    // The validity bytes are requested and folded into `ok` BEFORE the keys are requested: holding 16 byte
    // registers next to the 64 key registers in flight spilled 29 registers per thread (3.6 GB of scratch traffic
    // per 1 G-row column); the price is one short, byte-sized round trip per tile ahead of the key loads.
    ok = (uint32_t)((1ull << KPT) - 1ull);
    if (pair_bytes) {
      uint8_t vb[KPT / 2];
#pragma unroll
      for (int j = 0; j < KPT / 2; j++) {
        const int64_t bit = p.offset + row0 + (int64_t)j * 2 * kPartitionThreads + 2 * tid;
        vb[j] = vbits[bit >> 3];
      }
      ok = 0;
#pragma unroll
      for (int j = 0; j < KPT / 2; j++) {
        const int64_t bit = p.offset + row0 + (int64_t)j * 2 * kPartitionThreads + 2 * tid;
        ok |= (uint32_t)((vb[j] >> (bit & 7)) & 3) << (2 * j);
      }
    } else if (vbits) {
      ok = 0;
#pragma unroll
      for (int j = 0; j < KPT; j++) {
        const int64_t bit = p.offset + row0 + (int64_t)(j / 2) * 2 * kPartitionThreads + 2 * tid + (j & 1);
        ok |= (uint32_t)TGX_VALID_BIT(vbits, bit) << j;
      }
    }
    if (VALIDITY) asm volatile("" : "+v"(ok));  // (the fold stays ahead of the key loads)
#pragma unroll
    for (int j = 0; j < KPT / 2; j++) {
      i64x2 v = pv[(int64_t)j * kPartitionThreads];
      key[2 * j] = v.x;
      key[2 * j + 1] = v.y;
    }
  } else {
    // ragged last tile / 8-byte aligned buffers: lane holds rows row0 + j*T + tid
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      const int64_t i = row0 + (int64_t)j * kPartitionThreads + tid;
      const bool in = i < p.length;
      key[j] = vals[in ? i : p.length - 1];
      bool valid = in;
      if (in && vbits) {
        const int64_t bit = p.offset + i;
        valid = TGX_VALID_BIT(vbits, bit);
      }
      ok |= (uint32_t)valid << j;
    }
  }
}

// THREADS x KPT keys per tile, up to MAXP = 2 * THREADS buckets, runs padded to PAD slots.  <1024, 32>: one
// workgroup per CU (152 KiB of LDS); <512, 32>: two per CU, so one loads while the other sorts.
// ---- the per-tile body shared by both partition kernels -------------------------------------------------
// THREADS x KPT keys per tile (32768 either way), up to MAXP buckets, runs padded to PAD slots.
//   pass 1   LDS histogram of the tile's keys per bucket
//   scan     exclusive prefix of the counts + ONE global atomicAdd per touched bucket reserving the run
//   pass 2   counting sort of the 20-bit sub-keys into LDS      (hook `mid` runs just before it)
//   stores   each wave streams whole runs out, 16 bytes per lane (hook `before_stores` runs just before)
// (the hooks are where a software-pipelined caller would request the next tile; unused today)
template <int THREADS, int KPT, int MAXP, int PAD, bool KEY16, bool PACK20, bool CLUSTERED, class MidFn, class StoreFn>
__device__ __forceinline__ void partition_process_tile(const PartitionParams &p, uint32_t *sorted, uint32_t *hist,
                                                       uint32_t *toff, uint32_t *gbase, uint32_t *wave_sums,
                                                       uint32_t *long_runs, const uint32_t (&rel)[KPT], uint64_t ok,
                                                       MidFn &&mid,
                                                       StoreFn &&before_stores) {
  constexpr uint32_t NW = THREADS / 64;       // waves per workgroup
  constexpr int BPT = MAXP / THREADS;         // buckets per thread in the scan
  constexpr int NS = MAXP / (NW * 64);        // run-metadata sets per lane in the store phase
  static_assert(MAXP % THREADS == 0 && MAXP % (NW * 64) == 0 && PAD % 4 == 0, "shape");
  // KEY16: buckets of <= 2^16 keys, so a list entry is 2 bytes: half the list traffic.  Runs are padded to 32 slots
  // (64 bytes) by REPEATING their last key (a set union is idempotent; not used with multiplicity), since no
  // 16-bit value is left over as a filler.
  // PACK20 (round 5): 20-bit entries, three to an 8-byte word: a 64-byte line holds 24 of them (2.67 B per key instead
  // of 4); runs are padded to 24 entries, again by repeating their last key
  constexpr uint32_t RPAD = PACK20 ? 24u : KEY16 ? (uint32_t)kRunPad2 : (uint32_t)PAD;
  auto pad_up = [](uint32_t h) -> uint32_t { return PACK20 ? (h + 23u) / 24u * 24u : (h + (RPAD - 1u)) & ~(RPAD - 1u); };
  // six consecutive entries of a run as two words of three.  Past the run's end: its last key again -- or, with
  // multiplicity (a second sighting of a key counts), the filler 0xFFFFF, which no sub-key equals there (two bitmap
  // slices share the LDS: sub_bits <= 19).  Two copies of the loop, picked by a wave-uniform branch per run: the
  // selects of the filler form cost the plain form 8 % of the pass when both shared one body
  const bool fill = p.want_multiplicity != 0;
  auto pack6 = [&](uint32_t o, uint32_t h, uint32_t i) -> uint4 {
    uint64_t w[2];
    if (!fill) {
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const uint32_t i0 = i + 3u * q;
        const uint64_t a = sorted[o + (i0 < h ? i0 : h - 1)], b = sorted[o + (i0 + 1 < h ? i0 + 1 : h - 1)],
                       c = sorted[o + (i0 + 2 < h ? i0 + 2 : h - 1)];
        w[q] = a | (b << 20) | (c << 40);
      }
    } else {
#pragma unroll
      for (int q = 0; q < 2; q++) {
        uint64_t e[3];
#pragma unroll
        for (uint32_t j = 0; j < 3; j++) {
          const uint32_t at = i + 3u * q + j;
          e[j] = at < h ? (uint64_t)sorted[o + at] : 0xFFFFFull;
        }
        w[q] = e[0] | (e[1] << 20) | (e[2] << 40);
      }
    }
    return make_uint4((uint32_t)w[0], (uint32_t)(w[0] >> 32), (uint32_t)w[1], (uint32_t)(w[1] >> 32));
  };
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63, wave = tid >> 6;
  const uint32_t sub_mask = (uint32_t)((1ull << p.sub_bits) - 1);
  for (uint32_t b = tid; b < (uint32_t)MAXP; b += THREADS) hist[b] = 0;
  // CLUSTERED: runs of kLongRun keys and more (a tile of keys in order is one or two runs) are streamed out by the
  // whole workgroup, not by the one wave that owns the bucket: long_runs[0 .. n) are their buckets, [kMaxLongRuns] = n
  constexpr uint32_t kLongRun = 1024, kMaxLongRuns = THREADS * KPT / kLongRun;
  if (CLUSTERED && tid == 0) long_runs[kMaxLongRuns] = 0;
  __syncthreads();  // hist is zero
  // ---- pass 1: count keys per bucket ----
  // Keys that arrive in order (ids that grow with the row number, timestamps) put the 128 consecutive rows a wave
  // holds for one j into ONE bucket: 64 LDS atomics on one address take their turns (a tile of sorted keys cost
  // 180 us instead of 24).  CLUSTERED (the batch looked like that to partition_init_kernel's probe): a wave whose
  // valid lanes agree on the bucket for EVERY j of the tile (`whole`, a wave-uniform fact: one scalar branch picks a
  // straight-line loop) sends one add of the lane count per j, and in pass 2 lines its lanes up behind one cursor
  // bump.  A wave that straddles a bucket boundary takes the plain form for this tile.  (A template parameter and a
  // copy of the tile loop, not a question per tile: next to the plain passes in one loop the extra state spilled
  // ~200 bytes per lane and cost shuffled keys 0.5 - 1.3 ms per 1 G-row column.)
  bool whole = false;
  if (CLUSTERED) {
    uint32_t agreed = 0;
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      const bool okj = (ok >> j) & 1;
      const uint32_t b = rel[j] >> p.sub_bits;
      const uint64_t act = __ballot(okj);
      const uint32_t first = act ? (uint32_t)__builtin_ctzll(act) : 0u;
      const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)first);
      agreed |= (__ballot(okj && b != b0) == 0 ? 1u : 0u) << j;
    }
    whole = agreed == (uint32_t)((1ull << KPT) - 1ull);
  }
  if (CLUSTERED && whole) {
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      const uint64_t act = __ballot((ok >> j) & 1);
      const uint32_t first = act ? (uint32_t)__builtin_ctzll(act) : 64u;
      if (lane == first) atomicAdd(&hist[rel[j] >> p.sub_bits], (uint32_t)__builtin_popcountll(act));
    }
  } else {
#pragma unroll
    for (int j = 0; j < KPT; j++)
      if ((ok >> j) & 1) atomicAdd(&hist[rel[j] >> p.sub_bits], 1u);
  }
  __syncthreads();
  // ---- exclusive scan of the counts (BPT entries per thread) + one global reservation per touched bucket ----
  {
    uint32_t h[BPT], sum = 0;
#pragma unroll
    for (int k = 0; k < BPT; k++) {
      h[k] = hist[BPT * tid + k];
      sum += h[k];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      uint32_t up = __shfl_up(incl, d, 64);
      if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63) wave_sums[wave] = incl;
    __syncthreads();
    uint32_t excl = incl - sum;
    for (uint32_t w = 0; w < wave; w++) excl += wave_sums[w];
#pragma unroll
    for (int k = 0; k < BPT; k++) {
      const uint32_t b = BPT * tid + k;
      toff[b] = excl;
      hist[b] = excl;  // becomes the placement cursor of pass 2
      uint32_t g = 0;
      if (h[k] && b - p.bucket0 >= p.n_lists) {
        g = 0xFFFFFFFFu;  // no list for this bucket: the run goes straight to the bitmap
      } else if (h[k]) {
        const unsigned long long padded = pad_up(h[k]);
        const unsigned long long at = atomicAdd(&p.cursors[b], padded);
        // cap < 2^32 (checked on the host); a run that does not fit spills as a whole
        if (at + padded > p.cap) {
          // every later reservation fails too, so the list is valid exactly up to the first failure
          atomicMin(&p.cursors[p.n_buckets + b], at);
          g = 0xFFFFFFFFu;
        } else {
          g = (uint32_t)at;
          if (CLUSTERED && h[k] >= kLongRun) long_runs[atomicAdd(&long_runs[kMaxLongRuns], 1u)] = b;
        }
      }
      gbase[b] = g;
      excl += h[k];
    }
    if (tid == THREADS - 1) toff[MAXP] = excl;
  }
  __syncthreads();
  __builtin_amdgcn_sched_barrier(0);  // the hooks stay where they are written
  mid();
  __builtin_amdgcn_sched_barrier(0);
  // ---- pass 2: counting sort into LDS ----
  if (CLUSTERED && whole) {
    // one bucket per j for the whole wave: one cursor bump, the lanes line up behind it
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      const bool okj = (ok >> j) & 1;
      const uint64_t act = __ballot(okj);
      const uint32_t first = act ? (uint32_t)__builtin_ctzll(act) : 64u;
      uint32_t at = 0;
      if (lane == first) at = atomicAdd(&hist[rel[j] >> p.sub_bits], (uint32_t)__builtin_popcountll(act));
      at = (uint32_t)__builtin_amdgcn_readlane((int)at, (int)(first & 63u));
      const uint32_t before =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(act >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)act, 0u));
      if (okj) sorted[at + before] = rel[j] & sub_mask;
    }
  } else {
#pragma unroll
    for (int j = 0; j < KPT; j++) {
      if (!((ok >> j) & 1)) continue;
      const uint32_t pos = atomicAdd(&hist[rel[j] >> p.sub_bits], 1u);
      sorted[pos] = rel[j] & sub_mask;
    }
  }
  __syncthreads();
  __builtin_amdgcn_sched_barrier(0);
  before_stores();
  __builtin_amdgcn_sched_barrier(0);
  // ---- each wave streams whole runs out, 16 bytes per lane.  The wave owns buckets wave, wave + NW, ...;
  // lane m keeps the (offset, count, global start) of the (m + 64 s)-th of them in registers, so a step needs
  // no LDS round trip for the bookkeeping.  Four groups of 16 lanes take four buckets per step (a group covers
  // 64 slots per pass; runs average kTile/P keys).  The cost of this phase is per store instruction, not per
  // byte: 4-byte-per-lane stores of the same runs took 2.3 ms instead of 1.0 ms.
  {
    uint32_t m_o[NS], m_h[NS], m_g[NS];
#pragma unroll
    for (int s2 = 0; s2 < NS; s2++) {
      const uint32_t b = (lane + 64 * s2) * NW + wave;
      const bool in = b < p.n_buckets;
      const uint32_t o = in ? toff[b] : 0;
      m_o[s2] = o;
      m_h[s2] = in ? toff[b + 1] - o : 0;
      m_g[s2] = in ? gbase[b] : 0;
    }
    const uint32_t n_meta = (p.n_buckets > wave) ? (p.n_buckets - wave + NW - 1) / NW : 0;
    // lanes per bucket and buckets per step: 16 x 4 with 4-byte entries, 4 x 16 with 2-byte entries (a lane always
    // stores 16 bytes; runs average kTile / P keys)
    constexpr uint32_t LPB = (KEY16 || PACK20) ? 4u : 16u, BPS = 64u / LPB, KPL = PACK20 ? 6u : KEY16 ? 8u : 4u;
    const uint32_t grp = lane / LPB, sub = lane % LPB;
#pragma unroll
    for (int s2 = 0; s2 < NS; s2++) {
      const uint32_t m_end = n_meta > 64u * s2 ? (n_meta - 64u * s2 < 64u ? n_meta - 64u * s2 : 64u) : 0;
      for (uint32_t m0 = 0; m0 < m_end; m0 += BPS) {
        const uint32_t m = m0 + grp, src = m & 63;
        const uint32_t o = __shfl(m_o[s2], src, 64), g = __shfl(m_g[s2], src, 64);
        uint32_t h = __shfl(m_h[s2], src, 64);
        if (m >= m_end) h = 0;
        if (CLUSTERED && h >= kLongRun && g != 0xFFFFFFFFu) h = 0;  // (everybody's job, below)
        if (h == 0) continue;
        const uint32_t b = (m + 64 * s2) * NW + wave;
        if (g != 0xFFFFFFFFu) {
          const uint32_t padded = pad_up(h);
          if (PACK20) {
            // cap and g are multiples of 24 entries: the run starts on a 64-byte line
            uint8_t *dst = (uint8_t *)p.lists + ((uint64_t)(b - p.bucket0) * p.cap + g) / 3 * 8;
            for (uint32_t i = KPL * sub; i < padded; i += KPL * LPB) *(uint4 *)(dst + (uint64_t)(i / 3) * 8) = pack6(o, h, i);
          } else if (KEY16) {
            // 16-byte aligned: cap and g are multiples of 32 two-byte slots
            uint16_t *dst = (uint16_t *)p.lists + (uint64_t)(b - p.bucket0) * p.cap + g;
            for (uint32_t i = KPL * sub; i < padded; i += KPL * LPB) {
              uint32_t k8[8];
#pragma unroll
              for (uint32_t j = 0; j < 8; j++) k8[j] = sorted[o + (i + j < h ? i + j : h - 1)];
              uint4 v;
              v.x = k8[0] | (k8[1] << 16);
              v.y = k8[2] | (k8[3] << 16);
              v.z = k8[4] | (k8[5] << 16);
              v.w = k8[6] | (k8[7] << 16);
              *(uint4 *)&dst[i] = v;
            }
          } else {
            uint32_t *dst = p.lists + (uint64_t)(b - p.bucket0) * p.cap + g;  // 16-byte aligned: cap, g multiples of PAD
            for (uint32_t i = KPL * sub; i < padded; i += KPL * LPB) {
              uint4 v;
              v.x = i < h ? sorted[o + i] : kListPad;
              v.y = i + 1 < h ? sorted[o + i + 1] : kListPad;
              v.z = i + 2 < h ? sorted[o + i + 2] : kListPad;
              v.w = i + 3 < h ? sorted[o + i + 3] : kListPad;
              *(uint4 *)&dst[i] = v;
            }
          }
        } else {
          for (uint32_t i = sub; i < h; i += LPB) {
            // spill: straight into the global bitmap
            const uint64_t r = ((uint64_t)b << p.sub_bits) | sorted[o + i];
            const uint32_t bit = 1u << (r & 31);
            const uint32_t prev = atomicOr(&p.seen[r >> 5], bit);
            if ((prev & bit) && p.want_multiplicity) atomicOr(&p.twice[r >> 5], bit);
          }
        }
      }
    }
  }
  if (CLUSTERED) {
    const uint32_t n_long = long_runs[kMaxLongRuns];
    for (uint32_t q = 0; q < n_long; q++) {
      const uint32_t b = long_runs[q];
      const uint32_t o = toff[b], h = toff[b + 1] - o, g = gbase[b];
      const uint32_t padded = pad_up(h);
      if (PACK20) {
        uint8_t *dst = (uint8_t *)p.lists + ((uint64_t)(b - p.bucket0) * p.cap + g) / 3 * 8;
        for (uint32_t i = 6u * tid; i < padded; i += 6u * THREADS) *(uint4 *)(dst + (uint64_t)(i / 3) * 8) = pack6(o, h, i);
      } else if (KEY16) {
        uint16_t *dst = (uint16_t *)p.lists + (uint64_t)(b - p.bucket0) * p.cap + g;
        for (uint32_t i = 8u * tid; i < padded; i += 8u * THREADS) {
          uint32_t k8[8];
#pragma unroll
          for (uint32_t j = 0; j < 8; j++) k8[j] = sorted[o + (i + j < h ? i + j : h - 1)];
          uint4 v;
          v.x = k8[0] | (k8[1] << 16);
          v.y = k8[2] | (k8[3] << 16);
          v.z = k8[4] | (k8[5] << 16);
          v.w = k8[6] | (k8[7] << 16);
          *(uint4 *)&dst[i] = v;
        }
      } else {
        uint32_t *dst = p.lists + (uint64_t)(b - p.bucket0) * p.cap + g;
        for (uint32_t i = 4u * tid; i < padded; i += 4u * THREADS) {
          uint4 v;
          v.x = i < h ? sorted[o + i] : kListPad;
          v.y = i + 1 < h ? sorted[o + i + 1] : kListPad;
          v.z = i + 2 < h ? sorted[o + i + 2] : kListPad;
          v.w = i + 3 < h ? sorted[o + i + 3] : kListPad;
          *(uint4 *)&dst[i] = v;
        }
      }
    }
  }
  __syncthreads();
}

// Keys in order replayed against a slice: G neighbouring lanes hold the 32 keys of ONE bitmap word, and G atomics on one
// LDS address take their turns.  The lanes of such a group merge their bits (a butterfly over the group; merging only
// ever adds bits of the same word, so it is harmless when the group does not agree) and, when the whole group names
// the same word, only its first lane sends the OR.  Returns whether this lane still has to send its own.
template <int G>
__device__ __forceinline__ bool merge_word_group(uint32_t cw, uint32_t &cb) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < G; d <<= 1) {
    const uint32_t ow = __shfl_xor(cw, d, 64), ob = __shfl_xor(cb, d, 64);
    if (ow == cw) cb |= ob;
  }
  const uint32_t lead = lane & ~(uint32_t)(G - 1);
  const uint64_t agree = __ballot(cw == (uint32_t)__shfl(cw, (int)lead, 64));
  const bool whole = ((agree >> lead) & ((1ull << G) - 1)) == ((1ull << G) - 1);
  return !whole || lane == lead;
}

// key - base of one tile: in-range keys fit 31 bits (n_buckets << sub_bits <= 2^31).  "In range" is key - base < range,
// the test every other kernel of the key set applies (distinct_bitmap_kernel, distinct_outlier_kernel, the exports): NOT
// "inside the last slice" -- a key between the range's end and the slice's would be in the bitmap for this pass and
// an outlier for the repair, i.e. counted twice (groups_once came out short).  Keys outside the range (a
// sampled range that missed them, a later batch of keys that grow, a caller-supplied hint that does not hold) are never
// inserted but counted, so that the repair (distinct_resolve) or tgx_finalize knows; `outm` gets their positions.
template <int KPT>
__device__ __forceinline__ void partition_relative(const PartitionParams &p, const int64_t (&key)[KPT],
                                                   uint32_t (&rel)[KPT], uint32_t &outm) {
  outm = 0;
#pragma unroll
  for (int j = 0; j < KPT; j++) {
    const uint64_t r = (uint64_t)key[j] - (uint64_t)p.base;
    outm |= (r >= p.range ? 1u : 0u) << j;
    rel[j] = (uint32_t)r;  // the 64-bit keys die here
    asm volatile("" : "+v"(rel[j]));  // (keeps the compiler from re-deriving rel from the keys later)
  }
  __builtin_amdgcn_sched_barrier(0);
}

// The same for a batch of keys in no particular order (the plain passes): the few keys outside a sampled range add
// their share of the aggregates through global atomics where they are met.
template <int KPT, bool STATS>
__device__ __forceinline__ void partition_relative_plain(const PartitionParams &p, const int64_t (&key)[KPT],
                                                         uint32_t (&rel)[KPT], uint64_t &ok, unsigned long long &n_out) {
#pragma unroll
  for (int j = 0; j < KPT; j++) {
    const uint64_t r = (uint64_t)key[j] - (uint64_t)p.base;
    if (((ok >> j) & 1) && r >= p.range) {
      ok &= ~(1ull << j);
      n_out++;
      if (STATS) {
        const long long k = (long long)key[j];
        atomicMin(&p.outliers->mn, k);
        atomicMax(&p.outliers->mx, k);
        atomicAdd(&p.outliers->lo32_sum, (unsigned long long)((uint64_t)k & 0xFFFFFFFFull));
        atomicAdd((unsigned long long *)&p.outliers->hi32_sum, (unsigned long long)(k >> 32));
        atomicAdd(&p.outliers->count, 1ull);
      }
    }
    rel[j] = (uint32_t)r;  // the 64-bit keys die here
    asm volatile("" : "+v"(rel[j]));  // (keeps the compiler from re-deriving rel from the keys later)
  }
  __builtin_amdgcn_sched_barrier(0);
}

// The outliers' share of the column's aggregates (STATS), collected in LDS and handed on once by partition_kernel: a
// batch that lies outside the range altogether would otherwise queue five device-wide atomics per key on the same
// five addresses (3.9 ms per 4 Mi keys).  Their keys are read AGAIN here (from L2: the tile has just been loaded) --
// keeping the 64-bit keys until now, or reducing inside partition_relative, spills the tile's registers on every tile
// for the sake of a case that is rare.  MIN / MAX only bother the LDS when they would change it.
template <int THREADS, int KPT>
__device__ __forceinline__ void partition_outlier_stats(const PartitionParams &p, int64_t tile, bool wide, uint32_t outm,
                                                     OutlierStats *lds_out) {
  constexpr int kTile = THREADS * KPT;
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)p.values + p.offset);
  const int64_t row0 = tile * kTile;
  const bool paired = row0 + kTile <= p.length && wide;  // (the layout partition_load_tile chose)
  unsigned long long cnt = 0;
  for (int j = 0; j < KPT; j++) {
    if (!((outm >> j) & 1)) continue;
    const int64_t i = paired ? row0 + (int64_t)(j / 2) * 2 * THREADS + 2 * threadIdx.x + (j & 1)
                             : row0 + (int64_t)j * THREADS + threadIdx.x;
    const long long k = vals[i];
    if (k < *(volatile long long *)&lds_out->mn) atomicMin(&lds_out->mn, k);
    if (k > *(volatile long long *)&lds_out->mx) atomicMax(&lds_out->mx, k);
    atomicAdd(&lds_out->lo32_sum, (unsigned long long)((uint64_t)k & 0xFFFFFFFFull));
    atomicAdd((unsigned long long *)&lds_out->hi32_sum, (unsigned long long)(k >> 32));
    cnt++;
  }
  atomicAdd(&lds_out->count, cnt);
}

// 1024 threads x 32 keys, one workgroup per CU (152 KiB of LDS); any alignment, ragged last tile.
// FORM: the probe's verdict (partition_init_kernel) picks one of two copies of the tile loop for the whole launch; they
// are two KERNELS, launched one behind the other, the one whose form it is not leaving at once: in one kernel they
// shared a register allocation and the form for keys in order paid for it (78 scratch loads per tile and thread)
template <int THREADS, int KPT, int MAXP, int PAD, bool VALIDITY, bool KEY16, bool STATS, bool FORM_CLUSTERED, bool PACK20 = false>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void partition_kernel(
    PartitionParams p, unsigned long long *counters) {
  if ((p.force_form ? p.force_form == 2 : __builtin_amdgcn_readfirstlane((int)p.cursors[2 * p.n_buckets]) != 0) != FORM_CLUSTERED)
    return;
  constexpr int kTile = THREADS * KPT;
  __shared__ uint32_t sorted[kTile];     // the tile, grouped by bucket
  __shared__ uint32_t hist[MAXP];        // pass 1: keys per bucket; pass 2: placement cursors
  __shared__ uint32_t toff[MAXP + 1];    // exclusive prefix of the counts (toff[P] = tile total)
  __shared__ uint32_t gbase[MAXP];       // start of the run in the bucket's global list
  __shared__ uint32_t wave_sums[16];
  __shared__ uint32_t long_runs[kTile / 1024 + 1];
  __shared__ uint32_t t_lo, t_hi;  // (CLUSTERED) the span of the tile's keys
  const bool wide = (((uintptr_t)p.values + (uintptr_t)p.offset * 8) & 15) == 0;  // 16-byte loads legal
  unsigned long long n_valid = 0, n_out = 0;
  const int64_t n_tiles = (p.length + kTile - 1) / kTile;
  uint32_t rel[KPT];
  // STATS: the column's COUNT / MIN / MAX / SUM over the keys inside the range, taken from the 32-bit offsets (the
  // 64-bit keys are gone by then: no register is held across the tile for them) -- per tile a wave reduction and
  // four LDS atomics
  __shared__ uint32_t st_min, st_max;
  __shared__ unsigned long long st_sum, st_cnt;
  __shared__ OutlierStats st_out;  // (STATS) the keys outside the range: their aggregates go out once, at the end
  if (STATS && threadIdx.x == 0) {
    st_min = 0xFFFFFFFFu;
    st_max = 0;
    st_sum = 0;
    st_cnt = 0;
    st_out.mn = INT64_MAX;
    st_out.mx = INT64_MIN;
    st_out.lo32_sum = 0;
    st_out.hi32_sum = 0;
    st_out.count = 0;
  }
  if (STATS) __syncthreads();
  auto tile_loop = [&](auto clustered_tag) __attribute__((always_inline)) {
  constexpr bool CLUSTERED = decltype(clustered_tag)::value;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint64_t ok;
    {
      int64_t key[KPT];
      uint32_t ok32 = 0;
      partition_load_tile<THREADS, KPT, VALIDITY>(p, tile, wide, key, ok32);
      ok = ok32;
      n_valid += __builtin_popcountll(ok);  // every non-NULL row, whether its key lies inside the range or not
      if (CLUSTERED) {
        // (keys in order: a later batch of a column that grows lies outside the range as a whole)
        uint32_t outm;
        partition_relative<KPT>(p, key, rel, outm);
        outm &= ok32;
        ok = ok32 & ~outm;
        if (__ballot(outm != 0)) {
          n_out += __builtin_popcount(outm);
          if (STATS && outm) partition_outlier_stats<THREADS, KPT>(p, tile, wide, outm, &st_out);
        }
      } else {
        partition_relative_plain<KPT, STATS>(p, key, rel, ok, n_out);
      }
    }
    if (STATS) {
      uint32_t tmin = 0xFFFFFFFFu, tmax = 0;
      unsigned long long tsum = 0;
#pragma unroll
      for (int j = 0; j < KPT; j++) {
        const bool in = (ok >> j) & 1;
        tmin = (in && rel[j] < tmin) ? rel[j] : tmin;
        tmax = (in && rel[j] > tmax) ? rel[j] : tmax;
        tsum += in ? rel[j] : 0u;
      }
      unsigned long long tcnt = __builtin_popcountll(ok);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t omin = __shfl_down(tmin, d, 64), omax = __shfl_down(tmax, d, 64);
        tmin = omin < tmin ? omin : tmin;
        tmax = omax > tmax ? omax : tmax;
        tsum += __shfl_down(tsum, d, 64);
        tcnt += __shfl_down(tcnt, d, 64);
      }
      if ((threadIdx.x & 63) == 0 && tcnt) {
        atomicMin(&st_min, tmin);
        atomicMax(&st_max, tmax);
        atomicAdd(&st_sum, tsum);
        atomicAdd(&st_cnt, tcnt);
      }
    }
    if (CLUSTERED && !p.want_multiplicity) {
      // A tile of keys in order covers a short stretch of the range: when its keys span fewer bits than `sorted` has
      // (2^20: 32 768 consecutive ids span 2^15) the tile is OR-ed into a bitmap of that stretch in LDS and the
      // stretch's non-zero words into the global bitmap -- one device-wide atomic per 32 keys (ids in steps of one),
      // no list written, nothing to replay.  (Not with multiplicity: the second sighting of a key is not seen here.)
      if (threadIdx.x == 0) {
        t_lo = 0xFFFFFFFFu;
        t_hi = 0;
      }
      __syncthreads();
      uint32_t lo = 0xFFFFFFFFu, hi = 0;
#pragma unroll
      for (int j = 0; j < KPT; j++) {
        const bool in = (ok >> j) & 1;
        lo = (in && rel[j] < lo) ? rel[j] : lo;
        hi = (in && rel[j] > hi) ? rel[j] : hi;
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t olo = __shfl_xor(lo, d, 64), ohi = __shfl_xor(hi, d, 64);
        lo = olo < lo ? olo : lo;
        hi = ohi > hi ? ohi : hi;
      }
      if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&t_lo, lo);
        atomicMax(&t_hi, hi);
      }
      __syncthreads();
      const uint32_t tlo = t_lo, thi = t_hi;
      if (tlo > thi) continue;  // (no valid key inside the range in this tile)
      const uint32_t w0 = tlo >> 5, nw = (thi >> 5) - w0 + 1;
      if (nw <= (uint32_t)kTile) {
        for (uint32_t w = threadIdx.x; w < nw; w += THREADS) sorted[w] = 0;
        __syncthreads();
        // a lane's keys 2 j and 2 j + 1 are neighbouring rows; 16 lanes share a word when ids go in steps of one
#pragma unroll
        for (int j = 0; j < KPT; j += 2) {
          uint32_t cw = 0xFFFFFFFFu, cb = 0;
          if ((ok >> j) & 1) {
            cw = (rel[j] >> 5) - w0;
            cb = 1u << (rel[j] & 31);
          }
          if ((ok >> (j + 1)) & 1) {
            const uint32_t w1 = (rel[j + 1] >> 5) - w0, b1 = 1u << (rel[j + 1] & 31);
            if (w1 == cw) {
              cb |= b1;
            } else {
              if (cb) atomicOr(&sorted[cw], cb);
              cw = w1;
              cb = b1;
            }
          }
          const bool send = merge_word_group<16>(cw, cb);
          if (send && cb) atomicOr(&sorted[cw], cb);
        }
        __syncthreads();
        for (uint32_t w = threadIdx.x; w < nw; w += THREADS) {
          const uint32_t v = sorted[w];
          if (v) atomicOr(&p.seen[w0 + w], v);
        }
        __syncthreads();
        continue;
      }
    }
    partition_process_tile<THREADS, KPT, MAXP, PAD, KEY16, PACK20, CLUSTERED>(p, sorted, hist, toff, gbase, wave_sums, long_runs, rel, ok,
                                                                      [] {}, [] {});
  }
  };
  tile_loop(std::integral_constant<bool, FORM_CLUSTERED>{});
  if (STATS) {
    __syncthreads();
    if (threadIdx.x == 0) {
      ScanPartial out;
      out.min_k = INT64_MAX;
      out.max_k = INT64_MIN;
      out.sum_lo = 0;
      out.sum_hi = 0;
      out.non_null = (int64_t)st_cnt;
      out.sum = out.comp = out.s1 = out.s2 = 0.0;
      if (st_cnt) {
        out.min_k = (int64_t)((uint64_t)p.base + st_min);
        out.max_k = (int64_t)((uint64_t)p.base + st_max);
        const __int128 sum = (__int128)st_sum + (__int128)st_cnt * (__int128)p.base;
        out.sum_lo = (uint64_t)sum;
        out.sum_hi = (int64_t)(sum >> 64);
      }
      p.stats[blockIdx.x] = out;
      if (st_out.count) {
        atomicMin(&p.outliers->mn, st_out.mn);
        atomicMax(&p.outliers->mx, st_out.mx);
        atomicAdd(&p.outliers->lo32_sum, st_out.lo32_sum);
        atomicAdd((unsigned long long *)&p.outliers->hi32_sum, (unsigned long long)st_out.hi32_sum);
        atomicAdd(&p.outliers->count, st_out.count);
      }
    }
  }
  block_add2_any(n_valid, n_out, &counters[kCntValidRows], &counters[kCntOutOfRange]);
}

// (the outliers' share of the aggregates -- OutlierStats -- is folded by scan_reduce_kernel, kernels/scan.hip)

// Phase 2.  Workgroup b owns slice b of the bitmap: load it into LDS (it already holds the keys of
// earlier batches and this batch's spills), replay list b with LDS atomics, store it back, and add the
// slice's popcounts to the totals (counters[kCntDistinct] / [kCntTwice] are zeroed before the launch).
template <int LDS_WORDS, bool KEY16 = false, bool PACK20 = false>
__global__ __launch_bounds__(kPartitionThreads) void bucket_apply_kernel(PartitionParams p,
                                                                         unsigned long long *counters) {
  // static LDS: gfx950 lets one workgroup declare up to 160 KiB statically (dynamic LDS is capped lower)
  __shared__ __attribute__((aligned(16))) uint32_t lds[LDS_WORDS];
  const uint32_t tid = threadIdx.x;
  const uint32_t b = blockIdx.x;
  const uint32_t slice_words = (uint32_t)((1ull << p.sub_bits) >> 5);
  uint32_t *l_seen = lds;
  uint32_t *l_twice = lds + slice_words;  // only with multiplicity (host guarantees 2*slice_words fit)
  uint32_t *g_seen = p.seen + (uint64_t)b * slice_words;
  uint32_t *g_twice = p.want_multiplicity ? p.twice + (uint64_t)b * slice_words : nullptr;
  for (uint32_t w = tid * 4; w < slice_words; w += kPartitionThreads * 4) {
    *(uint4 *)&l_seen[w] = *(const uint4 *)&g_seen[w];
    if (g_twice) *(uint4 *)&l_twice[w] = *(const uint4 *)&g_twice[w];
  }
  __syncthreads();
  unsigned long long cnt = p.cursors[b];
  const unsigned long long limit = p.cursors[p.n_buckets + b];  // start of the first run that spilled
  if (cnt > limit) cnt = limit;
  const bool clustered = p.cursors[2 * p.n_buckets] != 0;  // (partition_init_kernel's probe)
  const uint32_t li = b - p.bucket0;  // (a bucket without a list has cnt == 0: its runs spilled)
  if (li >= p.n_lists) cnt = 0;
  if (PACK20) {
    // 20-bit entries, three to an 8-byte word, six per 16-byte load; cnt is a multiple of 24 and runs are padded with
    // repeats of real keys -- every entry counts -- or, with multiplicity, with a filler (the keys-in-order form of the pass takes this plain loop as well: a
    // column that reaches the lists in order has wide steps, and its tiles' words rarely repeat)
    const uint8_t *list = (const uint8_t *)p.lists + (uint64_t)li * p.cap / 3 * 8;
    constexpr uint64_t kStepP = (uint64_t)kPartitionThreads * 6;
    for (uint64_t w0 = (uint64_t)(tid & ~63u) * 6; w0 < cnt; w0 += 4 * kStepP) {
      const uint64_t i0 = w0 + (uint64_t)(tid & 63u) * 6;
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      u32x4 k4[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint64_t i = i0 + q * kStepP;
        k4[q] = u32x4{0, 0, 0, 0};
        if (i < cnt) k4[q] = __builtin_nontemporal_load((const u32x4 *)(list + i / 3 * 8));
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (i0 + q * kStepP >= cnt) continue;
        const uint64_t w[2] = {(uint64_t)k4[q].x | ((uint64_t)k4[q].y << 32), (uint64_t)k4[q].z | ((uint64_t)k4[q].w << 32)};
#pragma unroll
        for (int u = 0; u < 6; u++) {
          const uint32_t k = (uint32_t)(w[u / 3] >> (20 * (u % 3))) & 0xFFFFFu;
          const uint32_t bit = 1u << (k & 31);
          if (g_twice) {  // (multiplicity: runs are padded with the filler, never with a key)
            if (k == 0xFFFFFu) continue;
            const uint32_t prev = atomicOr(&l_seen[k >> 5], bit);
            if (prev & bit) atomicOr(&l_twice[k >> 5], bit);
          } else {
            atomicOr(&l_seen[k >> 5], bit);
          }
        }
      }
    }
  } else if (KEY16) {
    // 2-byte entries, eight per 16-byte load; runs are padded with repeats of real keys, so every entry counts
    const uint16_t *list16 = (const uint16_t *)p.lists + (uint64_t)li * p.cap;
    constexpr uint64_t kStep16 = (uint64_t)kPartitionThreads * 8;
    // (a wave's lanes leave the loop together -- the loop bound is the wave's first entry -- so that the merge of
    //  neighbouring lanes below always finds the whole wave)
    for (uint64_t w0 = (uint64_t)(tid & ~63u) * 8; w0 < cnt; w0 += 4 * kStep16) {
      const uint64_t i0 = w0 + (uint64_t)(tid & 63u) * 8;
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      u32x4 k4[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint64_t i = i0 + q * kStep16;
        k4[q] = u32x4{0, 0, 0, 0};
        if (i < cnt) k4[q] = __builtin_nontemporal_load((const u32x4 *)&list16[i]);
      }
      if (clustered) {
        // (the probe saw keys in order: a lane's eight keys mostly share a bitmap word, four lanes share it too)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const bool in = i0 + q * kStep16 < cnt;
          const uint32_t w4[4] = {k4[q].x, k4[q].y, k4[q].z, k4[q].w};
          uint32_t cw = 0xFFFFFFFFu, cb = 0;
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const uint32_t k = (u & 1) ? w4[u / 2] >> 16 : w4[u / 2] & 0xFFFFu;
            if (!in) continue;
            if ((k >> 5) != cw) {
              if (cb) atomicOr(&l_seen[cw], cb);
              cw = k >> 5;
              cb = 0;
            }
            cb |= 1u << (k & 31);
          }
          const bool send = merge_word_group<4>(cw, cb);
          if (send && cb) atomicOr(&l_seen[cw], cb);
        }
      } else {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        if (i0 + q * kStep16 >= cnt) continue;
        const uint32_t w4[4] = {k4[q].x, k4[q].y, k4[q].z, k4[q].w};
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const uint32_t ka = w4[u] & 0xFFFFu, kb = w4[u] >> 16;
          atomicOr(&l_seen[ka >> 5], 1u << (ka & 31));
          atomicOr(&l_seen[kb >> 5], 1u << (kb & 31));
        }
      }
      }
    }
  } else {
  const uint32_t *list = p.lists + (uint64_t)li * p.cap;
  // lists are made of 16-slot aligned runs, so cnt is a multiple of 4; kListPad slots are filler
  // four 16-byte loads in flight per lane before the first LDS atomic (requesting the NEXT four before the atomics
  // of the current ones -- the pipeline that pays in dict.hip / kll.hip -- measured 1.01 ms instead of 0.93 here)
  constexpr uint64_t kStep = (uint64_t)kPartitionThreads * 4;
  for (uint64_t w0 = (uint64_t)(tid & ~63u) * 4; w0 < cnt; w0 += 4 * kStep) {  // (whole waves, as above)
    const uint64_t i0 = w0 + (uint64_t)(tid & 63u) * 4;
    uint4 k4[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint64_t i = i0 + q * kStep;
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      u32x4 v = {kListPad, kListPad, kListPad, kListPad};
      if (i < cnt) v = __builtin_nontemporal_load((const u32x4 *)&list[i]);
      k4[q] = make_uint4(v.x, v.y, v.z, v.w);
    }
    if (clustered && !g_twice) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t ks[4] = {k4[q].x, k4[q].y, k4[q].z, k4[q].w};
        uint32_t cw = 0xFFFFFFFFu, cb = 0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
          if (ks[u] == kListPad) continue;
          if ((ks[u] >> 5) != cw) {
            if (cb) atomicOr(&l_seen[cw], cb);
            cw = ks[u] >> 5;
            cb = 0;
          }
          cb |= 1u << (ks[u] & 31);
        }
        const bool send = merge_word_group<8>(cw, cb);
        if (send && cb) atomicOr(&l_seen[cw], cb);
      }
      continue;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t ks[4] = {k4[q].x, k4[q].y, k4[q].z, k4[q].w};
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (ks[u] == kListPad) continue;
        const uint32_t bit = 1u << (ks[u] & 31);
        if (g_twice) {
          const uint32_t prev = atomicOr(&l_seen[ks[u] >> 5], bit);
          if (prev & bit) atomicOr(&l_twice[ks[u] >> 5], bit);
        } else {
          atomicOr(&l_seen[ks[u] >> 5], bit);
        }
      }
    }
  }
  }
  __syncthreads();
  unsigned long long n_seen = 0, n_twice = 0;
  for (uint32_t w = tid * 4; w < slice_words; w += kPartitionThreads * 4) {
    const uint4 s4 = *(const uint4 *)&l_seen[w];
    *(uint4 *)&g_seen[w] = s4;
    n_seen += __builtin_popcount(s4.x) + __builtin_popcount(s4.y) + __builtin_popcount(s4.z) +
              __builtin_popcount(s4.w);
    if (g_twice) {
      const uint4 t4 = *(const uint4 *)&l_twice[w];
      *(uint4 *)&g_twice[w] = t4;
      n_twice += __builtin_popcount(t4.x) + __builtin_popcount(t4.y) + __builtin_popcount(t4.z) +
                 __builtin_popcount(t4.w);
    }
  }
  block_add2_any(n_seen, n_twice, &counters[kCntDistinct], &counters[kCntTwice]);
}

// everything a partition pass wants cleared, in ONE launch (four small fills / kernels in a row were 20 us of a
// 100 M-row step per key column): the lists' cursors (zero) and valid-length limits (all-ones), the outliers'
// aggregates, and the two totals the replay recomputes
__global__ __launch_bounds__(1024) void partition_init_kernel(PartitionParams p, unsigned long long *totals) {
  unsigned long long *cursors = p.cursors;
  const uint32_t n_buckets = p.n_buckets;
  OutlierStats *outliers = p.outliers;
  for (uint32_t b = threadIdx.x; b < n_buckets; b += blockDim.x) {
    cursors[b] = 0;
    cursors[n_buckets + b] = ~0ull;
  }
  if (threadIdx.x == 0) {
    if (outliers) {
      outliers->mn = INT64_MAX;
      outliers->mx = INT64_MIN;
      outliers->lo32_sum = 0;
      outliers->hi32_sum = 0;
      outliers->count = 0;
    }
    totals[kCntDistinct] = 0;
    totals[kCntTwice] = 0;
  }
  // The probe: do keys that sit next to each other in the column fall into the same bucket?  64 groups of 128
  // consecutive rows, evenly spread (what a wave of partition_kernel holds for one j): a group agrees when every valid
  // key inside the range names one bucket.  Three quarters agreeing -> cursors[2 P] = 1 and partition_kernel runs its
  // CLUSTERED passes; shuffled keys never agree, keys in order always do (but for the groups that straddle a boundary).
  __shared__ uint32_t agree, asked;
  if (threadIdx.x == 0) agree = asked = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t n_groups = p.length / 128;
  global_i64_ptr vals = (global_i64_ptr)(uintptr_t)((const int64_t *)p.values + p.offset);
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)p.validity;
  // (one workgroup, all latency: a wave's four groups are requested together, then looked at)
  uint64_t rr[4][2];
  uint32_t vb[4][2];
  bool have[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const uint32_t g = wave + 16u * k;
    have[k] = (int64_t)g < n_groups;  // (g < 64: sixteen waves)
    const int64_t group = n_groups <= 64 ? (int64_t)g : (int64_t)g * (n_groups / 64);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int64_t i = group * 128 + h * 64 + lane;
      rr[k][h] = have[k] ? (uint64_t)vals[i] - (uint64_t)p.base : ~0ull;
      vb[k][h] = (have[k] && vbits) ? (uint32_t)TGX_VALID_BIT(vbits, p.offset + i) : 1u;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (!have[k]) continue;  // (wave-uniform)
    bool same = true;
    uint32_t b0 = 0xFFFFFFFFu;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint64_t r = rr[k][h];
      const bool okr = r < p.range && vb[k][h] != 0;
      const uint64_t act = __ballot(okr);
      if (act == 0) continue;  // (nothing inside the range: a group of outliers agrees -- CLUSTERED is their path too)
      const uint32_t b = (uint32_t)(r >> p.sub_bits);
      if (b0 == 0xFFFFFFFFu) b0 = (uint32_t)__builtin_amdgcn_readlane((int)b, (int)__builtin_ctzll(act));
      same = same && __ballot(okr && b != b0) == 0;
    }
    if (lane == 0) {
      atomicAdd(&asked, 1u);
      if (same) atomicAdd(&agree, 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long in_order = (asked >= 4 && 4 * agree >= 3 * asked) ? 1ull : 0ull;
    cursors[2 * n_buckets] = in_order;
    totals[kCntForm] = 1ull + in_order;  // (the host reads it with the counters: PartitionParams::force_form)
  }
}

// workgroups of launch_partition (= the ScanPartials it writes with stats)
int partition_grid(int64_t length, int n_cu) {
  int64_t n_tiles = (length + kPartitionTile - 1) / kPartitionTile;
  int grid = (int)(n_tiles < (int64_t)n_cu ? n_tiles : (int64_t)n_cu);
  return grid < 1 ? 1 : grid;
}

void launch_partition(const PartitionParams &p, unsigned long long *d_counters, int n_cu,
                      hipStream_t stream) {
  const int grid = partition_grid(p.length, n_cu);  // 152 KiB of LDS: one workgroup per CU
  // (software-pipelined variants -- next tile requested before this tile's stores -- were measured three times:
  //  with spills 3.3 ms, as 512 threads x 64 keys with 256 registers 6.0 ms, and spill-free 2.9 ms against
  //  2.7 ms without: the load and store phases already run at HBM rate and the other CUs fill the gaps)
  const bool plain = p.force_form != 2, in_order = p.force_form != 1;  // (force_form 0: both, the flag picks)
#define TGX_PART(VAL, K16, ST)                                                                                      \
  do {                                                                                                              \
    if (plain)                                                                                                      \
      hipLaunchKernelGGL((partition_kernel<kPartitionThreads, kPartitionKeysPerThread, (int)kMaxPartitions, kRunPad4, VAL, K16, ST, false>), \
                         dim3(grid), dim3(kPartitionThreads), 0, stream, p, d_counters);                            \
    if (in_order)                                                                                                   \
      hipLaunchKernelGGL((partition_kernel<kPartitionThreads, kPartitionKeysPerThread, (int)kMaxPartitions, kRunPad4, VAL, K16, ST, true>), \
                         dim3(grid), dim3(kPartitionThreads), 0, stream, p, d_counters);                            \
  } while (0)
#define TGX_PART20(VAL, ST)                                                                                         \
  do {                                                                                                              \
    if (plain)                                                                                                      \
      hipLaunchKernelGGL((partition_kernel<kPartitionThreads, kPartitionKeysPerThread, (int)kMaxPartitions, kRunPad4, VAL, false, ST, false, true>), \
                         dim3(grid), dim3(kPartitionThreads), 0, stream, p, d_counters);                            \
    if (in_order)                                                                                                   \
      hipLaunchKernelGGL((partition_kernel<kPartitionThreads, kPartitionKeysPerThread, (int)kMaxPartitions, kRunPad4, VAL, false, ST, true, true>), \
                         dim3(grid), dim3(kPartitionThreads), 0, stream, p, d_counters);                            \
  } while (0)
  if (p.key16 == 2) {  // 20-bit packed entries
    if (p.stats) {
      if (p.validity) TGX_PART20(true, true); else TGX_PART20(false, true);
    } else {
      if (p.validity) TGX_PART20(true, false); else TGX_PART20(false, false);
    }
    return;
  }
  if (p.stats) {
    if (p.key16) {
      if (p.validity) TGX_PART(true, true, true); else TGX_PART(false, true, true);
    } else {
      if (p.validity) TGX_PART(true, false, true); else TGX_PART(false, false, true);
    }
  } else if (p.key16) {
    if (p.validity) TGX_PART(true, true, false); else TGX_PART(false, true, false);
  } else {
    if (p.validity) TGX_PART(true, false, false); else TGX_PART(false, false, false);
  }
#undef TGX_PART
#undef TGX_PART20
}

hipError_t launch_bucket_apply(const PartitionParams &p, unsigned long long *d_counters,
                               hipStream_t stream) {
  const size_t words = ((size_t)1 << p.sub_bits) / 32 * (p.want_multiplicity ? 2 : 1);
  const dim3 grid(p.n_buckets), block(kPartitionThreads);
#define TGX_APPLY(W)                                                                                  \
  if (words <= W) {                                                                                   \
    if (p.key16 == 2)                                                                                 \
      hipLaunchKernelGGL((bucket_apply_kernel<W, false, true>), grid, block, 0, stream, p, d_counters); \
    else if (p.key16)                                                                                 \
      hipLaunchKernelGGL((bucket_apply_kernel<W, true>), grid, block, 0, stream, p, d_counters);      \
    else                                                                                              \
      hipLaunchKernelGGL((bucket_apply_kernel<W, false>), grid, block, 0, stream, p, d_counters);     \
    return hipGetLastError();                                                                         \
  }
  TGX_APPLY(1024)
  TGX_APPLY(2048)
  TGX_APPLY(4096)
  TGX_APPLY(8192)
  TGX_APPLY(16384)
  TGX_APPLY(32768)
#undef TGX_APPLY
  return hipErrorInvalidValue;
}

void launch_partition_init(const PartitionParams &p, unsigned long long *totals, hipStream_t stream) {
  hipLaunchKernelGGL(partition_init_kernel, dim3(1), dim3(1024), 0, stream, p, totals);
}

}  // namespace tgx
