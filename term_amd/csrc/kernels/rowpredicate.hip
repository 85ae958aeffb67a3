// rowpredicate.hip -- row predicates for gfx950 (TGX_CHECK_ROW_PREDICATE): the reference's Check::satisfies and
// ComplianceAnalyzer, each a
//   SELECT COUNT(CASE WHEN <expr> THEN 1 END), COUNT(*) FROM t
// over a closed predicate subset (include/tgx.h has the leaves, the program and their exact semantics).
//
// A task is one spec; grid = (blocks, tasks), a task's descriptor is read from device memory with scalar loads.
//
//   per row     every leaf is evaluated into two 32-bit masks T and F: bit j set means leaf j is TRUE / FALSE, neither
//               means UNKNOWN.  The postfix program then runs on two 32-bit bit-stacks per row (bit 0 is the top): PUSH
//               shifts a leaf's two bits in, AND is t = t1 & t2, f = f1 | f2, OR the dual, NOT swaps -- Kleene's logic
//               with no branch on a row's values.  Leaves and ops are wave-uniform: the loops over them branch on
//               scalars, and each is run over ALL the rows a lane has in flight, so a leaf's descriptor is fetched once
//               per trip and not once per row.
//   counters    two 32-bit counters per lane (satisfied, unknown; side_rows_fit guards the width), reduced within the
//               wave by shuffles, one 64-bit vector atomic per wave and counter, non-zero values only.  The failed rows
//               follow on the host.
//   numeric     row_predicate_numeric_kernel: every column the task reads is an 8-byte numeric.  rp_walk_pairs is the
//               sibling of row_walk.h's walker for 1 .. 8 columns: a lane takes row PAIRS, per column one 16-byte
//               non-temporal load where that column's address allows and two 8-byte loads where it does not, each
//               column under its own validity bitmap and Arrow offset (the pair's two bits from one byte where the
//               offset is even), 8 / kCols pairs in flight per lane.  The column count class (1, 2, 4, 8) and whether
//               any leaf compares totalOrder keys are template arguments, dispatched outside the row loop; a leaf picks
//               its column's value from registers by a chain of selects on a scalar, so nothing goes to scratch.
//   general     row_predicate_general_kernel: any column is a string layout.  A row per lane; a row's components are
//               read once through tuple_key.h's tuple_component (shared, not copied; a dictionary column is followed to
//               its entry, an index outside the dictionary is a NULL row).  STR_EQ compares the length first, then the
//               bytes against the literal pool of the descriptor.  STR_CMP, STR_LENGTH, STR_LIKE and STR_BLANK are the
//               functions of string_leaf.h over word_fetch.h's TcWordFetch (aligned 32-bit words, nothing outside the
//               words that hold a byte of the value); a workgroup copies the task's literal pool into LDS once, and
//               STR_CMP and STR_LIKE read their literal from there -- a LIKE pattern is indexed per lane.  IS_NULL,
//               STR_LENGTH in bytes and LIKE's length test read no byte of a value.
#include <hip/hip_runtime.h>

#include "bin_count.h"
#include "device_types.h"
#include "rowpredicate_types.h"
#include "string_leaf.h"
#include "tuple_key.h"
#include "word_fetch.h"

namespace tgx {

namespace {

typedef long long rp_i64x2 __attribute__((ext_vector_type(2)));
typedef const rp_i64x2 __attribute__((address_space(1))) *rp_i64x2_ptr;

__device__ __forceinline__ bool rp_compare(uint32_t op, int64_t a, int64_t b) {
  const bool lt = a < b, eq = a == b;
  return op == kRpEq ? eq : op == kRpLt ? lt : op == kRpLe ? (lt || eq) : op == kRpGt ? !(lt || eq) : !lt;
}

// the value as the leaf compares it (CAST AS DOUBLE: nearest-even)
__device__ __forceinline__ int64_t rp_key(int64_t bits, bool is_float) {
  return f64_total_key(is_float ? bits : __double_as_longlong((double)bits));
}

// the program on the rows' leaf masks; afterwards bit 0 of t[r] / f[r] is the row's verdict
template <int R>
__device__ __forceinline__ void rp_run(const RowPredTask &task, const uint32_t (&T)[R], const uint32_t (&F)[R],
                                       uint32_t (&t)[R], uint32_t (&f)[R]) {
#pragma unroll
  for (int r = 0; r < R; r++) t[r] = f[r] = 0;
  const int n_ops = (int)task.n_ops;
  for (int k = 0; k < n_ops; k++) {
    const uint32_t word = task.program[k], code = word & 255u, arg = word >> 8;
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (code == kRpPush) {
        t[r] = (t[r] << 1) | ((T[r] >> arg) & 1u);
        f[r] = (f[r] << 1) | ((F[r] >> arg) & 1u);
      } else if (code == kRpNot) {
        const uint32_t x = (t[r] ^ f[r]) & 1u;
        t[r] ^= x;
        f[r] ^= x;
      } else {
        const uint32_t both = t[r] & (t[r] >> 1) & 1u, any = (t[r] | (t[r] >> 1)) & 1u;
        const uint32_t fboth = f[r] & (f[r] >> 1) & 1u, fany = (f[r] | (f[r] >> 1)) & 1u;
        t[r] = ((t[r] >> 2) << 1) | (code == kRpAnd ? both : any);
        f[r] = ((f[r] >> 2) << 1) | (code == kRpAnd ? fany : fboth);
      }
    }
  }
}

__device__ __forceinline__ void rp_flush(const RowPredTask &task, unsigned long long *__restrict__ counts,
                                         uint32_t satisfied, uint32_t unknown) {
  const uint32_t s = wave_sum(satisfied), u = wave_sum(unknown);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *out = counts + task.word;
    if (s) atomicAdd(&out[0], (unsigned long long)s);
    if (u) atomicAdd(&out[1], (unsigned long long)u);
  }
}

// ---- the numeric route ---------------------------------------------------------------------------------------------
// R rows of kCols columns in registers: v[c][r] the bits, nulls[r] bit c: column c is NULL in row r
template <int kCols, int R, bool kKeys>
__device__ __forceinline__ void rp_eval_numeric(const RowPredTask &task, const int64_t (&v)[kCols][R],
                                                const uint32_t (&nulls)[R], const bool (&in)[R], uint32_t &satisfied,
                                                uint32_t &unknown) {
  uint32_t T[R], F[R];
#pragma unroll
  for (int r = 0; r < R; r++) T[r] = F[r] = 0;
  const int n_leaves = (int)task.n_leaves;
  for (int j = 0; j < n_leaves; j++) {
    const RowPredLeaf &L = task.leaves[j];
    const uint32_t kind = L.kind, op = L.op, ca = L.col, cb = L.col2;
    const bool keyed = kKeys && L.keyed, a_float = L.a_float, b_float = L.b_float;
    const int64_t lit = L.lit;
#pragma unroll
    for (int r = 0; r < R; r++) {
      int64_t a = v[0][r], b = v[0][r];
#pragma unroll
      for (int c = 1; c < kCols; c++) {
        a = ca == (uint32_t)c ? v[c][r] : a;
        b = cb == (uint32_t)c ? v[c][r] : b;
      }
      const bool a_null = (nulls[r] >> ca) & 1u, b_null = (nulls[r] >> cb) & 1u;
      bool tr, fa;
      if (kind == kRpIsNull) {
        tr = a_null;
        fa = !a_null;
      } else {
        const bool columns = kind == kRpCmpColumns;
        if (keyed) {
          a = rp_key(a, a_float);
          b = rp_key(b, b_float);
        }
        const bool known = !a_null && !(columns && b_null);
        const bool res = rp_compare(op, a, columns ? b : lit);
        tr = known && res;
        fa = known && !res;
      }
      T[r] |= (uint32_t)tr << j;
      F[r] |= (uint32_t)fa << j;
    }
  }
  uint32_t t[R], f[R];
  rp_run<R>(task, T, F, t, f);
#pragma unroll
  for (int r = 0; r < R; r++) {
    satisfied += in[r] ? (t[r] & 1u) : 0u;
    unknown += in[r] ? (~(t[r] | f[r]) & 1u) : 0u;
  }
}

// every row of the batch once, in pairs: rows 2p and 2p + 1 (the last pair of an odd batch has one row)
template <int kCols, bool kKeys>
__device__ __forceinline__ void rp_walk_pairs(const RowPredTask &task, unsigned long long *__restrict__ counts) {
  constexpr int kU = kCols >= 8 ? 1 : kCols >= 4 ? 2 : 4;  // pairs in flight per lane
  constexpr int R = 2 * kU;
  const int64_t length = task.d.length;
  const int64_t n_pairs = (length + 1) >> 1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const uint32_t reads = task.reads;
  uint32_t satisfied = 0, unknown = 0;  // (a workgroup sees fewer than 2^32 rows: side_rows_fit)
  for (int64_t p0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p0 < n_pairs; p0 += (int64_t)kU * stride) {
    int64_t v[kCols][R];
    uint32_t nulls[R];
    bool in[R];
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const int64_t p = p0 + (int64_t)u * stride;
      const bool here = p < n_pairs;
      const int64_t q = here ? p : 0;
      const bool second = 2 * q + 1 < length;  // (false only in the last pair of an odd batch)
      in[2 * u] = here;
      in[2 * u + 1] = here && second;
      nulls[2 * u] = nulls[2 * u + 1] = 0;
#pragma unroll
      for (int c = 0; c < kCols; c++) {
        const TupleCol &col = task.d.cols[c];
        global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)col.validity;
        const int64_t slot = col.offset + 2 * q;
        if (vbits) {
          uint32_t ok2;
          if ((col.offset & 1) == 0) {  // both rows of the pair share a validity byte
            ok2 = ((uint32_t)vbits[slot >> 3] >> (slot & 7)) & 3u;
          } else {
            ok2 = (uint32_t)TGX_VALID_BIT(vbits, slot);
            if (second) ok2 |= (uint32_t)TGX_VALID_BIT(vbits, slot + 1) << 1;
          }
          nulls[2 * u] |= (~ok2 & 1u) << c;
          nulls[2 * u + 1] |= ((~ok2 >> 1) & 1u) << c;
        }
        int64_t lo = 0, hi = 0;
        if ((reads >> c) & 1u) {
          const uintptr_t at = (uintptr_t)col.values + (uintptr_t)slot * 8;
          if ((((uintptr_t)col.values + (uintptr_t)col.offset * 8) & 15) == 0 && second) {
            const rp_i64x2 x = __builtin_nontemporal_load((rp_i64x2_ptr)at);
            lo = x.x;
            hi = x.y;
          } else {
            lo = __builtin_nontemporal_load((global_i64_ptr)at);
            if (second) hi = __builtin_nontemporal_load((global_i64_ptr)at + 1);
          }
        }
        v[c][2 * u] = lo;
        v[c][2 * u + 1] = hi;
      }
    }
    rp_eval_numeric<kCols, R, kKeys>(task, v, nulls, in, satisfied, unknown);
  }
  rp_flush(task, counts, satisfied, unknown);
}

template <int kCols>
__device__ __forceinline__ void rp_dispatch(const RowPredTask &task, unsigned long long *__restrict__ counts) {
  if (task.keys) rp_walk_pairs<kCols, true>(task, counts);
  else rp_walk_pairs<kCols, false>(task, counts);
}

// ---- the general route ---------------------------------------------------------------------------------------------
// component c of row i; an IS_NULL-only numeric column may have no values: its rows are then values of no account
__device__ __forceinline__ TupleComp rp_component(const RowPredTask &task, int c, int64_t i) {
  const TupleCol &col = task.d.cols[c];
  TupleComp none;
  none.kind = 0;
  none.value = 0;
  none.p = 0;
  none.len = 0;
  const int64_t slot = col.offset + i;
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)col.validity;
  if (vbits && !TGX_VALID_BIT(vbits, slot)) return none;
  if (col.kind == 0 && !((task.reads >> c) & 1u)) {
    none.kind = 1;
    return none;
  }
  if (col.kind == 4) {
    const int64_t idx = (int64_t)((global_i32_ptr)(uintptr_t)col.values)[slot];
    if ((uint64_t)idx >= (uint64_t)task.dict_length[c]) return none;  // (a negative index too)
  }
  return tuple_component(task.d, c, i);
}

__device__ __forceinline__ bool rp_bytes_equal(uintptr_t a, uintptr_t b, uint64_t len) {
  global_u8_ptr pa = (global_u8_ptr)a, pb = (global_u8_ptr)b;
  bool same = true;
  for (uint64_t k = 0; k < len && same; k++) same = pa[k] == pb[k];
  return same;
}

}  // namespace

__global__ __launch_bounds__(kRowPredBlock) void row_predicate_numeric_kernel(const RowPredTask *__restrict__ tasks,
                                                                              unsigned long long *__restrict__ counts) {
  const RowPredTask &task = tasks[blockIdx.y];
  const int n = task.d.n_cols;  // 1 .. 8
  if (n <= 1) rp_dispatch<1>(task, counts);
  else if (n <= 2) rp_dispatch<2>(task, counts);
  else if (n <= 4) rp_dispatch<4>(task, counts);
  else rp_dispatch<8>(task, counts);
}

// (5 waves a SIMD, what the kernel had before the string leaves of string_leaf.h: the bound holds it at 96 VGPRs)
__global__ __launch_bounds__(kRowPredBlock, 5) void row_predicate_general_kernel(const RowPredTask *__restrict__ tasks,
                                                                                 unsigned long long *__restrict__ counts) {
  const RowPredTask &task = tasks[blockIdx.y];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int n_cols = task.d.n_cols, n_leaves = (int)task.n_leaves;
  __shared__ uint8_t pool[kRowPredMaxLiteralBytes];
  for (int k = (int)threadIdx.x; k < kRowPredMaxLiteralBytes; k += (int)blockDim.x) pool[k] = task.literals[k];
  __syncthreads();
  uint32_t satisfied = 0, unknown = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < task.d.length; i += stride) {
    TupleComp comps[kMaxTupleCols];
#pragma unroll
    for (int c = 0; c < kMaxTupleCols; c++) {
      comps[c].kind = 0;
      comps[c].value = 0;
      comps[c].p = 0;
      comps[c].len = 0;
      if (c < n_cols) comps[c] = rp_component(task, c, i);
    }
    uint32_t T[1] = {0}, F[1] = {0};
    for (int j = 0; j < n_leaves; j++) {
      const RowPredLeaf &L = task.leaves[j];
      const uint32_t kind = L.kind, ca = L.col, cb = L.col2;
      TupleComp A = comps[0], B = comps[0];
#pragma unroll
      for (int c = 1; c < kMaxTupleCols; c++) {
        if (ca == (uint32_t)c) A = comps[c];
        if (cb == (uint32_t)c) B = comps[c];
      }
      bool tr, fa;
      if (kind == kRpIsNull) {
        tr = A.kind == 0;
        fa = !tr;
      } else {
        bool known = A.kind != 0, res = false;
        if (kind == kRpStrEq) {
          if (known && A.len == (uint64_t)L.lit_len)
            res = rp_bytes_equal(A.p, (uintptr_t)(task.literals + L.lit_offset), A.len);
        } else if (kind == kRpCmpColumns && L.strings) {
          known = known && B.kind != 0;
          if (known && A.len == B.len) res = rp_bytes_equal(A.p, B.p, A.len);
        } else if (kind >= kRpStrCmp) {  // (lit_offset + lit_len <= the pool's size: the setter)
          if (known) {
            TcWordFetch fetch;
            fetch.p = A.p;
            if (kind == kRpStrLength) res = sl::length(fetch, A.len, L.op, L.lit, L.strings != 0);
            else if (kind == kRpStrBlank) res = sl::blank(fetch, A.len);
            else if (kind == kRpStrCmp) res = sl::order(fetch, A.len, L.op, pool + L.lit_offset, L.lit_len);
            else res = sl::like(fetch, A.len, pool + L.lit_offset, L.lit_len, (uint32_t)L.lit);
          }
        } else {
          const bool columns = kind == kRpCmpColumns;
          known = known && !(columns && B.kind == 0);
          int64_t a = (int64_t)A.value, b = (int64_t)B.value;
          if (L.keyed) {
            a = rp_key(a, L.a_float);
            b = rp_key(b, L.b_float);
          }
          res = rp_compare(L.op, a, columns ? b : L.lit);
        }
        tr = known && res;
        fa = known && !res;
      }
      T[0] |= (uint32_t)tr << j;
      F[0] |= (uint32_t)fa << j;
    }
    uint32_t t[1], f[1];
    rp_run<1>(task, T, F, t, f);
    satisfied += t[0] & 1u;
    unknown += ~(t[0] | f[0]) & 1u;
  }
  rp_flush(task, counts, satisfied, unknown);
}

// `tasks`: n_tasks descriptors in device memory, all of one route
void launch_row_predicate(const RowPredTask *tasks, int n_tasks, bool numeric, int blocks_per_task,
                          unsigned long long *counts, hipStream_t stream) {
  const dim3 grid(blocks_per_task, n_tasks), block(kRowPredBlock);
  if (numeric) hipLaunchKernelGGL(row_predicate_numeric_kernel, grid, block, 0, stream, tasks, counts);
  else hipLaunchKernelGGL(row_predicate_general_kernel, grid, block, 0, stream, tasks, counts);
}

}  // namespace tgx
