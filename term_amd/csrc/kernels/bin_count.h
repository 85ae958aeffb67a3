// bin_count.h -- what the counting kernels of the side checks share (jointbins.hip, histogram.hip, temporal.hip).
//
// Count phase: a workgroup's cells are 32-bit counters in LDS (its share of the rows stays below 2^32), flushed to the
// task's 64-bit global counters with vector atomics once, at the end, non-zero cells only; two more counters per lane
// (the task's tail: rows outside, non-finite rows, ...) are reduced within the wave and added behind them.
// Range phase: a per-lane accumulator `Acc` (JointRangeAcc, HistRangeAcc) is folded lanes -> wave -> workgroup -> task.
// A kind gives range_clear(Acc &) and range_fold(Acc &, const Acc &), declared before this header is included.  The
// order of every fold is fixed -- `dlt` from 32 down to 1, the waves of a workgroup in index order, the partials strided
// by 64 and then the wave reduce -- so floating-point sums come out the same from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace tgx {

// the bin index of the equal-width binnings (jointbins.hip, paircounts.hip): the reference's expression, in IEEE double
// arithmetic as written -- subtract, divide (correctly rounded), floor; NaN for a NaN
__device__ __forceinline__ double bin_index(double v, double origin, double width) { return floor((v - origin) / width); }

// cell `cell` += 1 for every live lane.  Equal cells are combined within the wave: the cell of the wave's first live
// lane is broadcast, the lanes that hold the same cell are counted with a ballot and their leader adds the count; only
// the lanes with another cell add for themselves.
__device__ __forceinline__ void bin_add(unsigned int *cells, bool live, uint32_t cell) {
  const unsigned long long todo = __ballot(live);
  if (todo == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)todo) - 1;
  const uint32_t first = (uint32_t)__shfl((int)cell, leader, 64);
  const unsigned long long same = __ballot(live && cell == first);
  if (lane == leader)
    atomicAdd(&cells[first], (unsigned int)__popcll(same));
  else if (live && cell != first)
    atomicAdd(&cells[cell], 1u);
}

// the workgroup's `n` LDS cells into the task's 64-bit counters (the caller has synchronised the workgroup)
template <int kBlock>
__device__ __forceinline__ void bin_flush(const unsigned int *cells, uint32_t n, unsigned long long *__restrict__ out) {
  for (uint32_t c = threadIdx.x; c < n; c += kBlock) {
    const unsigned int v = cells[c];
    if (v) atomicAdd(&out[c], (unsigned long long)v);
  }
}

// the sum of the wave's 64 lanes of an integer term (32- or 64-bit, wrapping), in lane 0; every lane takes part
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) v += __shfl_down(v, dlt, 64);
  return v;
}

// the wave's sums of two per-lane counters into out[0] and out[1]
__device__ __forceinline__ void tail_flush(uint32_t a, uint32_t b, unsigned long long *__restrict__ out) {
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    a += __shfl_down(a, dlt, 64);
    b += __shfl_down(b, dlt, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&out[0], (unsigned long long)a);
    if (b) atomicAdd(&out[1], (unsigned long long)b);
  }
}

// lane 0 ends up with the fold of the wave's 64 accumulators (shuffled word by word)
template <class Acc>
__device__ __forceinline__ void range_wave_reduce(Acc &r) {
  constexpr int kWords = sizeof(Acc) / sizeof(int);
  static_assert(sizeof(Acc) % sizeof(int) == 0, "shuffled in 32-bit words");
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    int mine[kWords], theirs[kWords];
    __builtin_memcpy(mine, &r, sizeof(Acc));
#pragma unroll
    for (int w = 0; w < kWords; w++) theirs[w] = __shfl_down(mine[w], dlt, 64);
    Acc o;
    __builtin_memcpy(&o, theirs, sizeof(Acc));
    range_fold(r, o);
  }
}

// the workgroup's fold into partials[blockIdx.y][blockIdx.x]
template <int kBlock, class Acc>
__device__ __forceinline__ void range_block_store(Acc r, Acc *__restrict__ partials) {
  constexpr int kWaves = kBlock / 64;
  range_wave_reduce(r);
  __shared__ Acc sh[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sh[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc t = sh[0];
    for (int w = 1; w < kWaves; w++) range_fold(t, sh[w]);
    partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// the per-workgroup partials of a launch into the tasks' running states.  grid = tasks, one wave each.  (Local to the
// file that launches it, as the kinds' own range kernels are.)
namespace {
template <class Launch, class Acc>
__global__ __launch_bounds__(64) void range_reduce_kernel(const Launch L, const Acc *__restrict__ partials,
                                                          int blocks_per_task, Acc *__restrict__ accs) {
  const int task = blockIdx.x;
  Acc r;
  range_clear(r);
  for (int i = threadIdx.x; i < blocks_per_task; i += 64) range_fold(r, partials[(size_t)task * blocks_per_task + i]);
  range_wave_reduce(r);
  if (threadIdx.x == 0) range_fold(accs[L.acc_index[task]], r);
}
}  // namespace

}  // namespace tgx
