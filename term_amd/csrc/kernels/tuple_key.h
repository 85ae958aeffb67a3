// tuple_key.h -- a tuple of 2 .. 8 columns as ONE 128-bit key: what the tuple kernels of DISTINCT (distinct128.hip) and of
// the key probe (keyprobe_tuples.hip) share, so that a tuple has one fingerprint whichever kind reads it.
#pragma once
#include <hip/hip_runtime.h>

#include "distinct_types.h"
#include "fingerprint.h"
#include "keyset_device.h"

namespace tgx {

// ---- tuples of columns: COUNT(DISTINCT (a, b, ...)) / GROUP BY a, b, ... ------------------------------------
// Every component is reduced to 128 bits (numeric: its bit pattern; string: the fingerprint above; NULL: a
// marker no value maps to) and the components are the blocks of the tuple's own keyed fingerprint, in order.
// component c of row i: kind 0 NULL, 1 numeric (`value` = its 64 bits), 2 string (bytes [p, p + len))
struct TupleComp {
  uint32_t kind;
  uint64_t value;
  uintptr_t p;
  uint64_t len;
};
__device__ __forceinline__ TupleComp tuple_component(const TupleDesc &d, int c, int64_t i) {
  const TupleCol &col = d.cols[c];
  const int64_t slot = col.offset + i;
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)col.validity;
  TupleComp out;
  out.kind = 0;
  out.value = 0;
  out.p = 0;
  out.len = 0;
  if (vbits && !TGX_VALID_BIT(vbits, slot)) return out;
  if (col.kind == 0) {  // Int64 / Float64: the 64 bits themselves
    out.kind = 1;
    out.value = (uint64_t)((global_i64_ptr)(uintptr_t)col.values)[slot];
    return out;
  }
  int64_t b = 0, e = 0;
  uintptr_t base = (uintptr_t)col.data;
  if (col.kind == 4) {  // the row's dictionary entry: the component is the entry's string (or NULL), not the index
    const int64_t ds = col.dict_offset + (int64_t)((global_i32_ptr)(uintptr_t)col.values)[slot];
    global_u8_ptr dbits = (global_u8_ptr)(uintptr_t)col.dict_validity;
    if (dbits && !TGX_VALID_BIT(dbits, ds)) return out;  // a NULL entry makes the component NULL
    if (col.dict_large) {
      global_i64_ptr off = (global_i64_ptr)(uintptr_t)col.offsets;
      b = off[ds];
      e = off[ds + 1];
    } else {
      global_i32_ptr off = (global_i32_ptr)(uintptr_t)col.offsets;
      b = off[ds];
      e = off[ds + 1];
    }
  } else if (col.kind == 3) {
    global_i32_ptr vw = (global_i32_ptr)((uintptr_t)col.values + (uintptr_t)slot * 16);
    const int32_t len = vw[0];
    b = 0;
    e = len;
    if (len <= 12) {
      base = (uintptr_t)col.values + (uintptr_t)slot * 16 + 4;
    } else {
      const int32_t bi = vw[2], bo = vw[3];
      base = (uintptr_t)col.buffers[bi] + (uintptr_t)(uint32_t)bo;
    }
  } else if (col.kind == 2) {
    global_i64_ptr off = (global_i64_ptr)(uintptr_t)col.offsets;
    b = off[slot];
    e = off[slot + 1];
  } else {
    global_i32_ptr off = (global_i32_ptr)(uintptr_t)col.offsets;
    b = off[slot];
    e = off[slot + 1];
  }
  out.kind = 2;
  out.p = base + (uintptr_t)b;
  out.len = (uint64_t)(e - b);
  return out;
}

__device__ __forceinline__ void tuple_fingerprint(const TupleDesc &d, int64_t i, uint64_t *out_a, uint64_t *out_b,
                                                  bool *all_valid_out) {
  // the tuple's message: one 16-byte block per component (ca, cb) -- 16 x arity bytes, so the last component's block is
  // the message's last block and a full one (K1): tuples of another arity are messages of another length, which the
  // MAC tells apart as it does strings of different lengths (rounds 1-6a spent a third permutation on an arity block)
  Fp s;
  fp_init(s, d.key);
  bool all_valid = true;
  for (int c = 0; c < d.n_cols; c++) {
    const TupleComp comp = tuple_component(d, c, i);
    uint64_t ca, cb;
    if (comp.kind == 0) {
      all_valid = false;
      ca = 0x4e554c4c4e554c4cULL;  // "NULLNULL": tagged below so that no value of any type collides with it
      cb = 0;
    } else if (comp.kind == 1) {
      ca = comp.value;
      cb = 1;
    } else {
      fingerprint(d.key, comp.p, comp.len, &ca, &cb);
      cb |= 2;  // (tag space: 0 NULL, 1 numeric, >= 2 string)
    }
    if (c + 1 < d.n_cols)
      fp_block(s, ca, cb);
    else
      fp_last_padded(s, ca, cb, true, d.key);
  }
  fp_out(s, out_a, out_b);
  *all_valid_out = all_valid;
}

// ---- a tuple a row per lane, its NULLs known before any value is read: what the key probe (keyprobe_tuples.hip) and
// the tuple GROUP BY (tuple_group.h) share.  ARITY and NUMERIC ("every component is kind 0") are template parameters:
// the component loop is unrolled and a component's descriptor is read with a constant index ----
// is component c of row i a value?  (NUMERIC: every component is kind 0)
template <bool NUMERIC>
__device__ __forceinline__ bool kpt_valid(const KeyProbeTupleDesc &L, int c, int64_t i) {
  const TupleCol &col = L.d.cols[c];
  const int64_t slot = col.offset + i;
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)col.validity;
  if (vbits && !TGX_VALID_BIT(vbits, slot)) return false;
  if (!NUMERIC && col.kind == 4) {
    const int64_t idx = (int64_t)((global_i32_ptr)(uintptr_t)col.values)[slot];
    if ((uint64_t)idx >= (uint64_t)L.dict_length[c]) return false;  // (a negative index too)
    global_u8_ptr dbits = (global_u8_ptr)(uintptr_t)col.dict_validity;
    if (dbits && !TGX_VALID_BIT(dbits, col.dict_offset + idx)) return false;
  }
  return true;
}

// bit c: component c of row i is NULL
template <int ARITY, bool NUMERIC>
__device__ __forceinline__ uint32_t kpt_nulls(const KeyProbeTupleDesc &L, int64_t i) {
  uint32_t nulls = 0;
#pragma unroll
  for (int c = 0; c < ARITY; c++) nulls |= kpt_valid<NUMERIC>(L, c, i) ? 0u : 1u << c;
  return nulls;
}

// tuple_fingerprint's message for row i, whose NULL components are `nulls`: a component that is NULL is not read (an
// index outside its dictionary leads nowhere)
template <int ARITY, bool NUMERIC>
__device__ __forceinline__ void kpt_fingerprint(const KeyProbeTupleDesc &L, int64_t i, uint32_t nulls, uint64_t *out_a,
                                                uint64_t *out_b) {
  Fp s;
  fp_init(s, L.d.key);
#pragma unroll
  for (int c = 0; c < ARITY; c++) {
    const TupleCol &col = L.d.cols[c];
    uint64_t ca = 0x4e554c4c4e554c4cULL, cb = 0;  // the NULL marker
    if (!((nulls >> c) & 1)) {
      if (NUMERIC || col.kind == 0) {
        ca = (uint64_t)((global_i64_ptr)(uintptr_t)col.values)[col.offset + i];
        cb = 1;
      } else {
        const TupleComp comp = tuple_component(L.d, c, i);
        if (comp.kind == 2) {  // (nothing else: the component is a value and no number)
          fingerprint(L.d.key, comp.p, comp.len, &ca, &cb);
          cb |= 2;
        }
      }
    }
    if (c + 1 < ARITY)
      fp_block(s, ca, cb);
    else
      fp_last_padded(s, ca, cb, true, L.d.key);
  }
  fp_out(s, out_a, out_b);
}

}  // namespace tgx
