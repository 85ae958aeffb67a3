// keyprobe_tuples.hip -- the key probe on TUPLE keys for gfx950 (a TGX_CHECK_KEY_PROBE spec with a column list, set with
// tgx_plan_set_key_probe_tuples*): is each row's tuple (c0, c1, ..) of 2 .. 8 child columns among the parent's tuples?
// The device side of the reference's JoinCoverageConstraint::on_multiple (TG/constraints/join_coverage.rs:127-138, the
// join condition at :192-197).
//
//   the key     a tuple is its keyed 128-bit fingerprint, tuple_key.h's tuple_fingerprint bit for bit: a 16-byte block a
//               component -- (the sign- or zero-extended int64, 1), (the string's fingerprint with tag 2), or the NULL
//               marker -- the last one under K1.  So a narrow column joins a wide one and any string layout any other.
//   the set     routes 5 and 6 of keyprobe_strings.hip, built by its kernels from 32-byte {hash_a, hash_b, count, 0}
//               records of tuple fingerprints; kps_find (keyprobe_set.h) is the lookup, every index masked before use.
//   NULLs       SQL's join: a row with at least one NULL component matches nothing, a parent tuple with a NULL in the
//               same place included, although the two fingerprint alike.  A row per lane reads the validity of ALL its
//               components first (a dictionary component: its index against the dictionary's length, then the entry's
//               validity; each component under its own Arrow offset); an any-NULL row is never looked up.  It is still
//               a distinct value of its own (the reference's examples query is SELECT DISTINCT l0, l1 ..): it is
//               counted under its fingerprint in the task's table with a value length of 1, where the missing tuples
//               have 0, in the table's upper half, which is this class's own -- the length is the flag; the byte behind it is of no account (it is copied from the first
//               component's buffer, which nobody writes while the kernel runs).  Such rows are rare: they are
//               combined within the wave and go straight to the global table, their overflow to kKpLong's word (a
//               tuple has no long rows: the table keeps fingerprints and no bytes).
//   the probe   key_probe_tuple_kernel<Set, ARITY, NUMERIC>: an all-valid row is fingerprinted and looked up; a hit adds
//               to matched, and under the counted set the slot's count to the lane's pairs; sums per lane, a wave
//               reduction, one 64-bit vector atomic a wave and counter.  A miss goes the way VALUE_COUNTS's 128-bit keys
//               go: vc_wave_combine128, the workgroup's VcLdsStrings table, vc_insert_global128 with a zero-length
//               value; a probe sequence that runs out: the overflow counter.
//   gather      key_probe_rows_tuple_kernel<ARITY, NUMERIC>: every all-valid row becomes a 32-byte {fa, fb, 1, 0} record
//               behind the records of the batches before it.  A wave counts the all-valid rows of all its rounds and
//               bumps the cursor once; a record is two 16-byte stores, every position held against `cap`.
//   instances   the arity and "every component is an 8-byte integer" are template parameters, dispatched by the
//               launchers: the component loop is unrolled, a component's descriptor is read from the kernel's arguments
//               with a constant index (nothing goes to scratch), and the all-numeric instances ((order_id, line_no), the
//               common case) carry none of the string paths.
#include <hip/hip_runtime.h>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "fingerprint.h"
#include "keyprobe_set.h"
#include "tuple_key.h"

namespace tgx {

// (kpt_valid, kpt_nulls and kpt_fingerprint: tuple_key.h, shared with the tuple GROUP BY of tuple_group.h)

// ---- the probe -----------------------------------------------------------------------------------------------------------
// `Set`: KeyProbeStringSet, or KeyProbeCountedStringSet for a counted task, whose hits also sum their slots' counts.
// t: the task's table in the strings layout with one byte of value a slot; t.words: its kKeyProbeWords counters
template <class Set, int ARITY, bool NUMERIC>
__global__ __launch_bounds__(256) void key_probe_tuple_kernel(const KeyProbeTupleDesc L, const Set set,
                                                              const ValueCountsTable t) {
  constexpr bool kCounted = KpsCounted<Set>::value;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t non_null = 0, matched = 0;  // (a workgroup sees fewer than 2^32 rows: side_rows_fit)
  unsigned long long pairs = 0;        // (a counted set: cannot wrap, the host has refused such a batch)
  // a readable byte that stays as it is: the one byte of value a NULL-bearing tuple's slot copies
  const uintptr_t any_byte = (uintptr_t)(L.d.cols[0].values ? L.d.cols[0].values : L.d.cols[0].offsets);
  // the table's lower half is the missing tuples', its upper half the NULL-bearing tuples': each class has its own
  // slots (a power of two of at least 2 * max_missing_keys), so neither can crowd the other out
  const uint64_t half = (t.mask + 1) >> 1;
  ValueCountsTable tm = t, tn = t;
  tm.mask = tn.mask = half - 1;
  tn.keys += half;
  tn.keys2 += half;
  tn.counts += half;
  tn.lens += half;
  tn.store += half * (uint64_t)t.max_value_bytes;
  __shared__ VcLdsStrings lds;
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    lds.fa[s] = lds.fb[s] = kEmptyKey;
    lds.count[s] = 0;
  }
  __syncthreads();
  // (the loop is uniform within the wave: every lane takes part in the ballots of every round)
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < L.d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < L.d.length;
    unsigned long long fa = 0, fb = 0;
    bool missing = false, with_null = false;
    if (in) {
      const uint32_t nulls = kpt_nulls<ARITY, NUMERIC>(L, i);  // (before any value is read)
      uint64_t a, b;
      kpt_fingerprint<ARITY, NUMERIC>(L, i, nulls, &a, &b);
      fa = a;
      fb = b;
      if (nulls != 0) {
        with_null = true;  // (never looked up: it matches nothing)
      } else {
        non_null++;
        const int64_t at = kps_find(set, fa, fb);
        if (at >= 0) {
          matched++;
          if (kCounted) pairs += kps_times(set, at);
        } else {
          missing = true;
        }
      }
    }
    vc_wave_combine128(missing, fa, fb, lane, [&](uint32_t weight) {
      if (!vc_insert_lds128(lds, fa, fb, weight, 0ull))
        vc_insert_global128(tm, fa, fb, (unsigned long long)weight, (uintptr_t)0, 0u, &t.words[kKpOverflow]);
    });
    if (__ballot(with_null) != 0)
      vc_wave_combine128(with_null, fa, fb, lane, [&](uint32_t weight) {
        vc_insert_global128(tn, fa, fb, (unsigned long long)weight, any_byte, 1u, &t.words[kKpLong]);
      });
  }
  __syncthreads();
  // every occupied LDS slot is one global insert with its count
  for (uint32_t s = threadIdx.x; s < kValueCountsStrLdsSlots; s += 256) {
    const unsigned long long fa = lds.fa[s], fb = lds.fb[s];
    const unsigned int n = lds.count[s];
    if (fa == kEmptyKey || fb == kEmptyKey || n == 0) continue;
    vc_insert_global128(tm, fa, fb, (unsigned long long)n, (uintptr_t)0, 0u, &t.words[kKpOverflow]);
  }
  tail_flush(non_null, matched, t.words + kKpNonNull);
  if (kCounted) {
    pairs = wave_sum(pairs);
    if (lane == 0 && pairs) atomicAdd(&t.words[kKpPairs], pairs);
  }
}

// ---- the parent side from rows -------------------------------------------------------------------------------------------
// a row per lane; words: the task's counters (kKpNonNull: the all-valid rows, kKpPairs: the cursor)
template <int ARITY, bool NUMERIC>
__global__ __launch_bounds__(256) void key_probe_rows_tuple_kernel(const KeyProbeTupleDesc L, unsigned long long *recs,
                                                                   uint64_t cap, unsigned long long *words) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // (the loops are uniform within the wave.)  First the wave's room: the all-valid rows of all its rounds, and ONE bump
  // of the cursor for them
  unsigned long long mine = 0;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < L.d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    mine += (unsigned long long)__popcll(__ballot(i < L.d.length && kpt_nulls<ARITY, NUMERIC>(L, i) == 0));
  }
  if (mine == 0) return;  // (the wave as one)
  unsigned long long at = 0;
  if (lane == 0) {
    at = atomicAdd(&words[kKpPairs], mine);
    atomicAdd(&words[kKpNonNull], mine);
  }
  at = vc_shfl64(at, 0);
  // then the records, a round's behind the round's before
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < L.d.length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool valid = i < L.d.length && kpt_nulls<ARITY, NUMERIC>(L, i) == 0;
    const unsigned long long todo = __ballot(valid);
    const uint64_t to = at + (uint64_t)__popcll(todo & ((1ull << lane) - 1));
    at += (unsigned long long)__popcll(todo);
    if (!valid || to >= cap) continue;  // (past cap: cannot happen, cap counts every row the state has seen)
    uint64_t fa, fb;
    kpt_fingerprint<ARITY, NUMERIC>(L, i, 0u, &fa, &fb);
    ulonglong2 *out = (ulonglong2 *)recs + 2 * to;
    out[0] = make_ulonglong2(fa, fb);
    out[1] = make_ulonglong2(1, 0);
  }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
namespace {

template <class Set, bool NUMERIC>
void launch_probe(const KeyProbeTupleDesc &L, const Set &set, const ValueCountsTable &t, hipStream_t stream) {
  const dim3 grid(grid_for((uint64_t)L.d.length)), block(256);
  switch (L.d.n_cols) {
#define TGX_KPT_CASE(N)                                                                                       \
  case N:                                                                                                     \
    hipLaunchKernelGGL((key_probe_tuple_kernel<Set, N, NUMERIC>), grid, block, 0, stream, L, set, t);        \
    break;
    TGX_KPT_CASE(2)
    TGX_KPT_CASE(3)
    TGX_KPT_CASE(4)
    TGX_KPT_CASE(5)
    TGX_KPT_CASE(6)
    TGX_KPT_CASE(7)
    TGX_KPT_CASE(8)
#undef TGX_KPT_CASE
    default:
      break;  // (the plan holds 2 .. kMaxTupleCols columns)
  }
}

template <bool NUMERIC>
void launch_rows(const KeyProbeTupleDesc &L, unsigned long long *recs, uint64_t cap, unsigned long long *words,
                 hipStream_t stream) {
  const dim3 grid(grid_for((uint64_t)L.d.length)), block(256);
  switch (L.d.n_cols) {
#define TGX_KPT_CASE(N)                                                                                           \
  case N:                                                                                                         \
    hipLaunchKernelGGL((key_probe_rows_tuple_kernel<N, NUMERIC>), grid, block, 0, stream, L, recs, cap, words);  \
    break;
    TGX_KPT_CASE(2)
    TGX_KPT_CASE(3)
    TGX_KPT_CASE(4)
    TGX_KPT_CASE(5)
    TGX_KPT_CASE(6)
    TGX_KPT_CASE(7)
    TGX_KPT_CASE(8)
#undef TGX_KPT_CASE
    default:
      break;
  }
}

static_assert(kMaxTupleCols == 8, "the launchers dispatch arities 2 .. 8");

}  // namespace

// `numeric`: every component is an 8-byte integer column (TupleCol::kind 0)
void launch_key_probe_tuples(const KeyProbeTupleDesc &L, bool numeric, const KeyProbeStringSet &set,
                             const ValueCountsTable &t, hipStream_t stream) {
  if (numeric) launch_probe<KeyProbeStringSet, true>(L, set, t, stream);
  else launch_probe<KeyProbeStringSet, false>(L, set, t, stream);
}

void launch_key_probe_tuples_counted(const KeyProbeTupleDesc &L, bool numeric, const KeyProbeCountedStringSet &set,
                                     const ValueCountsTable &t, hipStream_t stream) {
  if (numeric) launch_probe<KeyProbeCountedStringSet, true>(L, set, t, stream);
  else launch_probe<KeyProbeCountedStringSet, false>(L, set, t, stream);
}

void launch_key_probe_rows_tuples(const KeyProbeTupleDesc &L, bool numeric, unsigned long long *recs, uint64_t cap,
                                  unsigned long long *words, hipStream_t stream) {
  if (numeric) launch_rows<true>(L, recs, cap, words, stream);
  else launch_rows<false>(L, recs, cap, words, stream);
}

}  // namespace tgx
