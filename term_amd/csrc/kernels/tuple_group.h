// tuple_group.h -- GROUP BY a tuple of 2 .. 8 columns: what the tuple kernels of GROUP_COUNTS (groupcounts.hip) and
// GROUP_SUMS (groupsums.hip) share.  A row's NULL mask and its fingerprint are tuple_key.h's (kpt_nulls,
// kpt_fingerprint: the key DISTINCT and KEY_PROBE give the tuple, bit for bit); here is the key's canonical byte form,
// which an entry keeps and by which states, blobs and ranks unite (include/tgx.h; ../group_key.h is the host's twin):
//   NULL      0x00
//   integer   0x01, the 8 big-endian bytes of value ^ 2^63
//   string    0x02, the length as 2 big-endian bytes, the bytes
// the components one behind the other.  A NULL component is never read.
#pragma once
#include "tuple_key.h"

namespace tgx {

// the bytes row i's key takes, in 64 bits (a string of 65 536 bytes or more is past every max_value_bytes, which is at
// most 256: its row is a long row and is never encoded)
template <int ARITY, bool NUMERIC>
__device__ __forceinline__ uint64_t tuple_encoded_length(const KeyProbeTupleDesc &L, int64_t i, uint32_t nulls) {
  uint64_t n = 0;
#pragma unroll
  for (int c = 0; c < ARITY; c++) {
    if ((nulls >> c) & 1) n += 1;
    else if (NUMERIC || L.d.cols[c].kind == 0) n += 9;
    else n += 3 + tuple_component(L.d, c, i).len;
  }
  return n;
}

// row i's key into dst[0, tuple_encoded_length): the caller has found the length within its bound
template <int ARITY, bool NUMERIC>
__device__ __forceinline__ void tuple_encode(const KeyProbeTupleDesc &L, int64_t i, uint32_t nulls, uint8_t *dst) {
  uint32_t at = 0;
#pragma unroll
  for (int c = 0; c < ARITY; c++) {
    const TupleCol &col = L.d.cols[c];
    if ((nulls >> c) & 1) {
      dst[at++] = 0;
    } else if (NUMERIC || col.kind == 0) {
      const uint64_t v = (uint64_t)((global_i64_ptr)(uintptr_t)col.values)[col.offset + i] ^ 0x8000000000000000ULL;
      dst[at++] = 1;
      for (int b = 0; b < 8; b++) dst[at++] = (uint8_t)(v >> (56 - 8 * b));
    } else {
      const TupleComp comp = tuple_component(L.d, c, i);
      const uint32_t len = (uint32_t)comp.len;
      global_u8_ptr src = (global_u8_ptr)comp.p;
      dst[at++] = 2;
      dst[at++] = (uint8_t)(len >> 8);
      dst[at++] = (uint8_t)len;
      for (uint32_t b = 0; b < len; b++) dst[at++] = src[b];
    }
  }
}

// the launchers' dispatch on (arity, every component an 8-byte integer): CASE(N, NUMERIC) launches one instance
#define TGX_TUPLE_GROUP_DISPATCH(n_cols, numeric, CASE) \
  switch (n_cols) {                                     \
    case 2: if (numeric) { CASE(2, true) } else { CASE(2, false) } break; \
    case 3: if (numeric) { CASE(3, true) } else { CASE(3, false) } break; \
    case 4: if (numeric) { CASE(4, true) } else { CASE(4, false) } break; \
    case 5: if (numeric) { CASE(5, true) } else { CASE(5, false) } break; \
    case 6: if (numeric) { CASE(6, true) } else { CASE(6, false) } break; \
    case 7: if (numeric) { CASE(7, true) } else { CASE(7, false) } break; \
    case 8: if (numeric) { CASE(8, true) } else { CASE(8, false) } break; \
    default: break; /* (the plan holds 2 .. kMaxTupleCols columns) */     \
  }
static_assert(kMaxTupleCols == 8, "the launchers dispatch arities 2 .. 8");

}  // namespace tgx
