// jointbins.hip -- joint bin counts of two numeric columns for gfx950 (TGX_CHECK_JOINT_BINS): the two scans behind
// MutualInformationAnalyzer's numeric x numeric branch (TG/analyzers/advanced/mutual_information.rs:143-248).
//
//   pair_range_kernel   n, MIN / MAX of x and y over the rows where both are non-NULL and finite (CAST AS DOUBLE)
//   joint_bins_kernel   per such row i = FLOOR((x - x_origin) / x_width), j likewise, cell (i, j) += 1
//
// Both read what comoments_kernel reads (16 B + 2 validity bits per row) the way it does: one row per lane per load,
// row pairs as one 16-byte load per column where the addresses allow, four loads in flight per column per lane
// (jb_for_rows, row_walk.h).
//
// The cells of a workgroup are 32-bit counters in LDS (a workgroup's share of the rows stays below 2^32), flushed to the
// task's 64-bit global counters with vector atomics once, at the end, non-zero cells only.  What decides the design is
// contention: with 10 bins there are 121 cells, and on sorted or strongly dependent data every lane of a wave wants the
// same one -- 64 serialised adds to one address.  So equal cells are COMBINED WITHIN THE WAVE before the atomic: the
// cell of the wave's first live lane is broadcast, the lanes that hold the same cell are counted with a ballot and their
// leader adds the count; only the lanes with another cell add for themselves.  On sorted data that is one add per wave
// and load, on independent data one ballot more than the plain loop.  (Counter sets replicated per wave were the
// alternative: they spread the waves of a workgroup, but the lanes of ONE wave still meet on one address.)
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "row_walk.h"

namespace tgx {

namespace {

struct JointRangePartial {
  int64_t n, non_finite;
  double x_min, x_max, y_min, y_max;
};

__device__ __forceinline__ void jb_range_fold(JointRangePartial &a, const JointRangePartial &b) {
  a.n += b.n;
  a.non_finite += b.non_finite;
  a.x_min = fmin(a.x_min, b.x_min);
  a.x_max = fmax(a.x_max, b.x_max);
  a.y_min = fmin(a.y_min, b.y_min);
  a.y_max = fmax(a.y_max, b.y_max);
}

constexpr int kJointWaves = kJointBlock / 64;

}  // namespace

__global__ __launch_bounds__(kJointBlock) void pair_range_kernel(const JointLaunch L,
                                                                  JointRangePartial *__restrict__ partials) {
  const ComomentColDesc d = L.pairs[blockIdx.y];
  JointRangePartial r = {0, 0, INFINITY, -INFINITY, INFINITY, -INFINITY};
  jb_for_rows(d, [&](int64_t xb, int64_t yb, bool ok) {
    const double a = d.x_is_float ? __longlong_as_double(xb) : (double)xb;
    const double b = d.y_is_float ? __longlong_as_double(yb) : (double)yb;
    const bool finite = a - a == 0.0 && b - b == 0.0;
    r.non_finite += ok && !finite ? 1 : 0;
    if (ok && finite) {
      r.n++;
      r.x_min = fmin(r.x_min, a);
      r.x_max = fmax(r.x_max, a);
      r.y_min = fmin(r.y_min, b);
      r.y_max = fmax(r.y_max, b);
    }
  });
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    JointRangePartial o;
    o.n = __shfl_down(r.n, dlt, 64);
    o.non_finite = __shfl_down(r.non_finite, dlt, 64);
    o.x_min = __shfl_down(r.x_min, dlt, 64);
    o.x_max = __shfl_down(r.x_max, dlt, 64);
    o.y_min = __shfl_down(r.y_min, dlt, 64);
    o.y_max = __shfl_down(r.y_max, dlt, 64);
    jb_range_fold(r, o);
  }
  __shared__ JointRangePartial sh[kJointWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) sh[wave] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    JointRangePartial t = sh[0];
    for (int w = 1; w < kJointWaves; w++) jb_range_fold(t, sh[w]);
    partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// the per-workgroup partials of a launch into the tasks' running states.  grid = pairs, one wave each.
__global__ __launch_bounds__(64) void pair_range_reduce_kernel(const JointLaunch L,
                                                               const JointRangePartial *__restrict__ partials,
                                                               int blocks_per_pair, JointRangeAcc *__restrict__ accs) {
  const int pair = blockIdx.x;
  JointRangePartial r = {0, 0, INFINITY, -INFINITY, INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < blocks_per_pair; i += 64) jb_range_fold(r, partials[(size_t)pair * blocks_per_pair + i]);
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    JointRangePartial o;
    o.n = __shfl_down(r.n, dlt, 64);
    o.non_finite = __shfl_down(r.non_finite, dlt, 64);
    o.x_min = __shfl_down(r.x_min, dlt, 64);
    o.x_max = __shfl_down(r.x_max, dlt, 64);
    o.y_min = __shfl_down(r.y_min, dlt, 64);
    o.y_max = __shfl_down(r.y_max, dlt, 64);
    jb_range_fold(r, o);
  }
  if (threadIdx.x != 0) return;
  JointRangeAcc &acc = accs[L.acc_index[pair]];
  acc.n += r.n;
  acc.non_finite += r.non_finite;
  acc.x_min = fmin(acc.x_min, r.x_min);
  acc.x_max = fmax(acc.x_max, r.x_max);
  acc.y_min = fmin(acc.y_min, r.y_min);
  acc.y_max = fmax(acc.y_max, r.y_max);
}

// dynamic LDS: joint_cells(bins) 32-bit counters of the pair this workgroup works on
__global__ __launch_bounds__(kJointBlock) void joint_bins_kernel(const JointLaunch L) {
  extern __shared__ unsigned int jb_cells[];
  const ComomentColDesc d = L.pairs[blockIdx.y];
  const JointBinning B = L.binning[blockIdx.y];
  unsigned long long *__restrict__ out = L.counters[blockIdx.y];
  const uint32_t side = B.bins + 1, n_cells = side * side;
  for (uint32_t c = threadIdx.x; c < n_cells; c += kJointBlock) jb_cells[c] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const double top = (double)B.bins;
  uint32_t outside = 0, non_finite = 0;  // (a lane sees fewer than 2^32 rows)
  jb_for_rows(d, [&](int64_t xb, int64_t yb, bool ok) {
    const double a = d.x_is_float ? __longlong_as_double(xb) : (double)xb;
    const double b = d.y_is_float ? __longlong_as_double(yb) : (double)yb;
    const bool finite = a - a == 0.0 && b - b == 0.0;
    non_finite += ok && !finite ? 1u : 0u;
    // the reference's expression, in IEEE double arithmetic as written: subtract, divide (correctly rounded), floor
    const double fi = floor((a - B.x_origin) / B.x_width);
    const double fj = floor((b - B.y_origin) / B.y_width);
    const bool inside = fi >= 0.0 && fi <= top && fj >= 0.0 && fj <= top;  // (false for NaN)
    outside += ok && finite && !inside ? 1u : 0u;
    const bool live = ok && finite && inside;
    const uint32_t cell = live ? (uint32_t)fi * side + (uint32_t)fj : 0u;  // < n_cells: 0 <= fi, fj <= bins
    const unsigned long long todo = __ballot(live);
    if (todo == 0) return;
    const int leader = __ffsll((long long)todo) - 1;
    const uint32_t first = (uint32_t)__shfl((int)cell, leader, 64);
    const unsigned long long same = __ballot(live && cell == first);
    if (lane == leader)
      atomicAdd(&jb_cells[first], (unsigned int)__popcll(same));
    else if (live && cell != first)
      atomicAdd(&jb_cells[cell], 1u);
  });
  __syncthreads();
  for (uint32_t c = threadIdx.x; c < n_cells; c += kJointBlock) {
    const unsigned int v = jb_cells[c];
    if (v) atomicAdd(&out[c], (unsigned long long)v);
  }
#pragma unroll
  for (int dlt = 32; dlt >= 1; dlt >>= 1) {
    outside += __shfl_down(outside, dlt, 64);
    non_finite += __shfl_down(non_finite, dlt, 64);
  }
  if (lane == 0) {
    if (outside) atomicAdd(&out[n_cells], (unsigned long long)outside);
    if (non_finite) atomicAdd(&out[n_cells + 1], (unsigned long long)non_finite);
  }
}

size_t joint_range_partial_bytes() { return sizeof(JointRangePartial); }

void launch_pair_range(const JointLaunch &L, int n_pairs, int blocks_per_pair, void *d_partials, JointRangeAcc *d_accs,
                       hipStream_t stream) {
  hipLaunchKernelGGL(pair_range_kernel, dim3(blocks_per_pair, n_pairs), dim3(kJointBlock), 0, stream, L,
                     (JointRangePartial *)d_partials);
  hipLaunchKernelGGL(pair_range_reduce_kernel, dim3(n_pairs), dim3(64), 0, stream, L,
                     (const JointRangePartial *)d_partials, blocks_per_pair, d_accs);
}

// `lds_bytes`: the counters of the launch's largest binning
void launch_joint_bins(const JointLaunch &L, int n_pairs, int blocks_per_pair, size_t lds_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(joint_bins_kernel, dim3(blocks_per_pair, n_pairs), dim3(kJointBlock), lds_bytes, stream, L);
}

}  // namespace tgx
