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

static __device__ __forceinline__ void range_clear(JointRangeAcc &a) {
  a.n = a.non_finite = 0;
  a.x_min = a.y_min = INFINITY;
  a.x_max = a.y_max = -INFINITY;
}

static __device__ __forceinline__ void range_fold(JointRangeAcc &a, const JointRangeAcc &b) {
  a.n += b.n;
  a.non_finite += b.non_finite;
  a.x_min = fmin(a.x_min, b.x_min);
  a.x_max = fmax(a.x_max, b.x_max);
  a.y_min = fmin(a.y_min, b.y_min);
  a.y_max = fmax(a.y_max, b.y_max);
}

}  // namespace tgx

#include "bin_count.h"

namespace tgx {

static __global__ __launch_bounds__(kJointBlock) void pair_range_kernel(const JointLaunch L,
                                                                         JointRangeAcc *__restrict__ partials) {
  const ComomentColDesc d = L.pairs[blockIdx.y];
  JointRangeAcc r;
  range_clear(r);
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
  range_block_store<kJointBlock>(r, partials);
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
  const double top = (double)B.bins;
  uint32_t outside = 0, non_finite = 0;  // (a lane sees fewer than 2^32 rows)
  jb_for_rows(d, [&](int64_t xb, int64_t yb, bool ok) {
    const double a = d.x_is_float ? __longlong_as_double(xb) : (double)xb;
    const double b = d.y_is_float ? __longlong_as_double(yb) : (double)yb;
    const bool finite = a - a == 0.0 && b - b == 0.0;
    non_finite += ok && !finite ? 1u : 0u;
    const double fi = bin_index(a, B.x_origin, B.x_width);
    const double fj = bin_index(b, B.y_origin, B.y_width);
    const bool inside = fi >= 0.0 && fi <= top && fj >= 0.0 && fj <= top;  // (false for NaN)
    outside += ok && finite && !inside ? 1u : 0u;
    const bool live = ok && finite && inside;
    const uint32_t cell = live ? (uint32_t)fi * side + (uint32_t)fj : 0u;  // < n_cells: 0 <= fi, fj <= bins
    bin_add(jb_cells, live, cell);
  });
  __syncthreads();
  bin_flush<kJointBlock>(jb_cells, n_cells, out);
  tail_flush(outside, non_finite, out + n_cells);
}

void launch_pair_range(const JointLaunch &L, int n_pairs, int blocks_per_pair, JointRangeAcc *d_partials,
                       JointRangeAcc *d_accs, hipStream_t stream) {
  hipLaunchKernelGGL(pair_range_kernel, dim3(blocks_per_pair, n_pairs), dim3(kJointBlock), 0, stream, L, d_partials);
  hipLaunchKernelGGL((range_reduce_kernel<JointLaunch, JointRangeAcc>), dim3(n_pairs), dim3(64), 0, stream, L,
                     (const JointRangeAcc *)d_partials, blocks_per_pair, d_accs);
}

// `lds_bytes`: the counters of the launch's largest binning
void launch_joint_bins(const JointLaunch &L, int n_pairs, int blocks_per_pair, size_t lds_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(joint_bins_kernel, dim3(blocks_per_pair, n_pairs), dim3(kJointBlock), lds_bytes, stream, L);
}

}  // namespace tgx
