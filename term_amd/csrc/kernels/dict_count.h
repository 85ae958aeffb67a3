// dict_count.h -- the first step of the dictionary routes that count per ENTRY (valuecounts.hip, keyprobe_strings.hip):
// the rows' indices counted into one 64-bit cell per dictionary entry (up to kValueCountsDictLdsCells entries through
// 32-bit cells in LDS, bin_count.h's idiom; above that with global atomics).  What a kind does with an entry and its
// count is its own second kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "bin_count.h"
#include "device_types.h"
#include "keyset_device.h"

namespace tgx {

// the rows' indices into cells[dict_length]; an index outside the dictionary is a row without a value: it is counted
// as a NULL row (include/tgx.h says so), never read
template <bool kLds>
__global__ __launch_bounds__(256) void value_counts_dict_count_kernel(const int32_t *__restrict__ indices,
                                                                      const uint8_t *__restrict__ validity,
                                                                      int64_t offset, int64_t length, int64_t dict_length,
                                                                      unsigned long long *__restrict__ cells) {
  global_u8_ptr vbits = (global_u8_ptr)(uintptr_t)validity;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // up to kValueCountsDictLdsCells entries: the workgroup's cells are 32-bit counters in LDS (bin_count.h), flushed once
  __shared__ unsigned int lcells[kLds ? kValueCountsDictLdsCells : 1];
  if (kLds) {
    for (uint32_t c = threadIdx.x; c < (uint32_t)dict_length; c += 256) lcells[c] = 0;
    __syncthreads();
  }
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < length; base += stride) {
    const int64_t i = base + threadIdx.x;
    const int64_t slot = offset + i;
    bool live = i < length && (!vbits || TGX_VALID_BIT(vbits, slot));
    int32_t idx = live ? indices[slot] : 0;
    live = live && idx >= 0 && (int64_t)idx < dict_length;
    if (kLds) {
      bin_add(lcells, live, (uint32_t)idx);
      continue;
    }
    const unsigned long long todo = __ballot(live);
    if (todo == 0) continue;
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t first = __shfl(idx, leader, 64);
    const unsigned long long same = __ballot(live && idx == first);
    if (lane == leader) atomicAdd(&cells[first], (unsigned long long)__popcll(same));
    else if (live && idx != first) atomicAdd(&cells[idx], 1ull);
  }
  if (kLds) {
    __syncthreads();
    bin_flush<256>(lcells, (uint32_t)dict_length, cells);
  }
}

// `cells`: dict_length 64-bit words, zero
inline void launch_dict_count(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              int64_t dict_length, unsigned long long *cells, hipStream_t stream) {
  if (dict_length <= (int64_t)kValueCountsDictLdsCells)  // (fewer workgroups: each one flushes its cells once)
    hipLaunchKernelGGL(value_counts_dict_count_kernel<true>, dim3(std::min(grid_for((uint64_t)length), 1024)), dim3(256),
                       0, stream, indices, validity, offset, length, dict_length, cells);
  else
    hipLaunchKernelGGL(value_counts_dict_count_kernel<false>, dim3(grid_for((uint64_t)length)), dim3(256), 0, stream,
                       indices, validity, offset, length, dict_length, cells);
}

}  // namespace tgx
