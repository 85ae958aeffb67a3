// typeclass.hip -- type classes of string columns for gfx950 (TGX_CHECK_TYPE_CLASSES): the per-row classification
// behind the reference's DataTypeAnalyzer (TG/analyzers/advanced/data_type.rs:129-150),
//   SELECT CASE WHEN <boolean> .. WHEN <integer> .. WHEN <double> .. WHEN <date> .. ELSE 'string' END, COUNT(*)
//   FROM t WHERE c IS NOT NULL GROUP BY 1
// Every non-NULL value is read once by the lexer of typeclass_lex.h and lands in exactly one of seven classes
// (include/tgx.h has the contract).
//
//   string route      type_class_kernel, grid = (blocks, tasks): a row per lane (Utf8 / LargeUtf8 / Utf8View through
//                     utf8_value_of's three layouts).  Per lane seven 32-bit class counters and the non-NULL rows (a
//                     lane sees fewer than 2^32 rows: side_rows_fit), reduced within the wave by shuffles and added to
//                     the task's 64-bit counters with one vector atomic per wave and non-zero counter: no LDS, no
//                     per-row atomic, no scratch (the counters are bumped by compares, never indexed).
//   dictionary route  value_counts_dict_count_kernel (dict_count.h) counts the INDICES into one 64-bit cell per entry;
//                     type_class_dict_kernel then takes a lane per entry with a non-zero count, classifies the entry once
//                     and adds its count to the class with 64-bit adds.  Rows of NULL entries and of indices outside the
//                     dictionary are counted nowhere: they are NULL rows.
//
// The bytes of a value are fetched through TcWordFetch (word_fetch.h, shared with the string leaves of
// rowpredicate.hip): the naturally aligned 32-bit word that holds the byte, kept until the lexer leaves it.  Such a word
// always holds at least one byte of the value, so it lies in the value's allocation (allocations start and end on word
// boundaries); nothing else outside [p, p + len) is read.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bin_count.h"
#include "count_table.h"
#include "device_types.h"
#include "dict_count.h"
#include "typeclass_types.h"
#include "word_fetch.h"

namespace tgx {

namespace {

__device__ __forceinline__ int tc_classify(uintptr_t p, uint64_t len) {
  TcWordFetch f;
  f.p = p;
  return type_class_of(f, len);
}

}  // namespace

// ---- string route -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTypeClassBlock) void type_class_kernel(const TypeClassLaunch L) {
  const Utf8ColDesc d = L.cols[blockIdx.y];
  unsigned long long *__restrict__ out = L.counts + L.word[blockIdx.y];
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint32_t non_null = 0, n[kTypeClassCount];
#pragma unroll
  for (int k = 0; k < kTypeClassCount; k++) n[k] = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d.length; i += stride) {
    const int64_t slot = d.offset + i;
    if (vbits && !TGX_VALID_BIT(vbits, slot)) continue;
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, slot, &p, &len);
    const int cls = tc_classify(p, len);
    non_null++;
#pragma unroll
    for (int k = 0; k < kTypeClassCount; k++) n[k] += cls == k ? 1u : 0u;
  }
  // (every lane of the wave is back here: the shuffles take all 64)
  const bool first = (threadIdx.x & 63) == 0;
  const uint32_t nn = wave_sum(non_null);
  if (first && nn) atomicAdd(&out[kTcNonNull], (unsigned long long)nn);
#pragma unroll
  for (int k = 0; k < kTypeClassCount; k++) {
    const uint32_t s = wave_sum(n[k]);
    if (first && s) atomicAdd(&out[k], (unsigned long long)s);
  }
}

// ---- dictionary route ---------------------------------------------------------------------------------------------------
// `d`: the dictionary's values as a string column; a lane per entry with a non-zero count in cells[d.length]
__global__ __launch_bounds__(256) void type_class_dict_kernel(const Utf8ColDesc d,
                                                              const unsigned long long *__restrict__ cells,
                                                              unsigned long long *__restrict__ out) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)d.validity;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < d.length; e += stride) {
    const unsigned long long rows = cells[e];
    const int64_t slot = d.offset + e;
    if (rows == 0 || (vbits && !TGX_VALID_BIT(vbits, slot))) continue;
    uintptr_t p;
    uint64_t len;
    utf8_value_of(d, slot, &p, &len);
    const int cls = tc_classify(p, len);  // 0 .. kTypeClassCount - 1
    atomicAdd(&out[kTcNonNull], rows);
    atomicAdd(&out[cls], rows);
  }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
// (every column of the launch has `length` rows)
void launch_type_classes(const TypeClassLaunch &L, int n_tasks, int64_t length, hipStream_t stream) {
  hipLaunchKernelGGL(type_class_kernel, dim3(grid_for((uint64_t)length), n_tasks), dim3(kTypeClassBlock), 0, stream, L);
}

// `cells`: dict.length 64-bit words, zero; `out`: the task's counters
void launch_type_classes_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, unsigned long long *cells, unsigned long long *out,
                              hipStream_t stream) {
  launch_dict_count(indices, validity, offset, length, dict.length, cells, stream);
  hipLaunchKernelGGL(type_class_dict_kernel, dim3(grid_for((uint64_t)dict.length)), dim3(256), 0, stream, dict, cells,
                     out);
}

}  // namespace tgx
