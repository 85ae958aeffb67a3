// histogram.hip -- the histogram of one numeric column for gfx950 (TGX_CHECK_HISTOGRAM): the two scans behind
// HistogramAnalyzer (TG/analyzers/advanced/histogram.rs:184-330).
//
//   hist_range_kernel    n, MIN, MAX, SUM(x), SUM(x * x) over the non-NULL, finite rows (CAST AS DOUBLE)
//   hist_counts_kernel   per such row the bucket of the reference's CASE chain against the task's edge table, += 1
//
// Both read 8 B + 1 validity bit per row through the single-column walk of row_walk.h: row pairs as one 16-byte load
// where the address allows, four loads in flight per lane.
//
// The bucket rule (include/tgx.h): the first i in 0 .. B-1 with edges[i] <= x < edges[i+1], else B-1.  edges[0 .. B-1]
// are non-decreasing, so with k = the number of interior edges edges[1 .. B-1] that are <= x the bucket is k when
// x >= edges[0] (k <= B-1; for k == B-1 the row is in the last bucket by its own WHEN or by ELSE), and B-1 otherwise.
// edges[B] only decides whether a row of the last bucket came through ELSE.  k is found from a GUESS --
// (x - edges[0]) * (B-1) / (edges[B-1] - edges[0]) -- that only steers: four independent LDS reads around it are
// compared with x, and when they do not pin k down (edges the caller spaced unevenly) a branch-free binary search
// over the interior edges does (10 dependent reads at B = 1000).  Either way comparisons against the table decide.
//
// The edges (at most 1001 doubles) and the workgroup's 32-bit bucket counters (a workgroup's share of the rows stays
// below 2^32) live in LDS; the counters are flushed to the task's 64-bit global counters with vector atomics once, at
// the end, non-zero buckets only.  As in jointbins.hip equal buckets are COMBINED WITHIN THE WAVE before the LDS atomic:
// on sorted or constant data every lane of a wave wants one bucket, and that is then one add per wave and load.
#include <hip/hip_runtime.h>

#include "device_types.h"
#include "row_walk.h"

namespace tgx {

static __device__ __forceinline__ void range_clear(HistRangeAcc &a) {
  a.n = a.non_finite = 0;
  a.min = INFINITY;
  a.max = -INFINITY;
  a.sum = a.sum_squared = 0.0;
}

static __device__ __forceinline__ void range_fold(HistRangeAcc &a, const HistRangeAcc &b) {
  a.n += b.n;
  a.non_finite += b.non_finite;
  a.min = fmin(a.min, b.min);
  a.max = fmax(a.max, b.max);
  a.sum += b.sum;
  a.sum_squared += b.sum_squared;
}

}  // namespace tgx

#include "bin_count.h"

namespace tgx {

static __global__ __launch_bounds__(kHistBlock) void hist_range_kernel(const HistLaunch L,
                                                                        HistRangeAcc *__restrict__ partials) {
  const ComomentColDesc d = L.cols[blockIdx.y];
  HistRangeAcc r;
  range_clear(r);
  jb_for_rows_single(d, [&](int64_t xb, bool ok) {
    const double a = d.x_is_float ? __longlong_as_double(xb) : (double)xb;
    const bool finite = a - a == 0.0;
    r.non_finite += ok && !finite ? 1 : 0;
    if (ok && finite) {
      r.n++;
      r.min = fmin(r.min, a);
      r.max = fmax(r.max, a);
      r.sum += a;
      r.sum_squared += a * a;  // (the square rounds on its own: the build does not contract)
    }
  });
  range_block_store<kHistBlock>(r, partials);
}

// dynamic LDS: hist_lds_bytes(buckets) of the task this workgroup works on -- B + 1 edges, then B 32-bit counters
__global__ __launch_bounds__(kHistBlock) void hist_counts_kernel(const HistLaunch L) {
  extern __shared__ double hist_lds[];
  const ComomentColDesc d = L.cols[blockIdx.y];
  const uint32_t B = L.buckets[blockIdx.y];
  const double *__restrict__ g_edges = L.edges[blockIdx.y];
  unsigned long long *__restrict__ out = L.counters[blockIdx.y];
  double *edges = hist_lds;                                   // [0, B]
  unsigned int *cells = (unsigned int *)(hist_lds + (B + 1));  // [0, B)
  for (uint32_t c = threadIdx.x; c <= B; c += kHistBlock) edges[c] = g_edges[c];
  for (uint32_t c = threadIdx.x; c < B; c += kHistBlock) cells[c] = 0;
  __syncthreads();
  const uint32_t last = B - 1;  // the last bucket, and the last interior edge (B >= 1)
  const double e0 = edges[0], e_end = edges[B];
  const double span = edges[last] - e0;
  const double scale = span > 0.0 && span - span == 0.0 ? (double)last / span : 0.0;
  const double top = (double)last;
  uint32_t else_rows = 0, non_finite = 0;  // (a lane sees fewer than 2^32 rows)
  jb_for_rows_single(d, [&](int64_t xb, bool ok) {
    const double x = d.x_is_float ? __longlong_as_double(xb) : (double)xb;
    const bool finite = x - x == 0.0;
    non_finite += ok && !finite ? 1u : 0u;
    const bool live = ok && finite;
    // k = the number of interior edges edges[1 .. last] that are <= x.  The guess (NaN and infinities clamp away):
    const uint32_t guess = (uint32_t)fmin(fmax((x - e0) * scale, 0.0), top);
    const uint32_t lo = guess > 0 ? guess - 1 : 0;
    // edges[lo + 1 .. lo + 3], as far as they are interior edges: a prefix of them is <= x
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t t = 1; t <= 3; t++) {
      const uint32_t j = lo + t;
      cnt += j <= last && edges[j <= last ? j : last] <= x ? 1u : 0u;
    }
    uint32_t k = lo + cnt;
    // pinned down: edges[lo] <= x (or lo == 0), and the edge after the counted ones is > x (or there is none)
    const bool pinned = (lo == 0 || edges[lo] <= x) && (cnt < 3 || k == last);
    if (live && !pinned) {
      uint32_t pos = 0, len = last;  // upper bound over the interior edges I[t] = edges[t + 1], t in [0, last)
      while (len > 0) {
        const uint32_t half = len >> 1;
        const bool le = edges[pos + half + 1] <= x;
        pos = le ? pos + half + 1 : pos;
        len = le ? len - half - 1 : half;
      }
      k = pos;
    }
    const bool below = !(x >= e0);
    const uint32_t cell = live ? (below ? last : k) : 0u;  // <= last: k counts at most `last` edges
    else_rows += live && (below || (k == last && !(x < e_end))) ? 1u : 0u;
    bin_add(cells, live, cell);
  });
  __syncthreads();
  bin_flush<kHistBlock>(cells, B, out);
  tail_flush(else_rows, non_finite, out + B);
}

void launch_hist_range(const HistLaunch &L, int n_tasks, int blocks_per_task, HistRangeAcc *d_partials,
                       HistRangeAcc *d_accs, hipStream_t stream) {
  hipLaunchKernelGGL(hist_range_kernel, dim3(blocks_per_task, n_tasks), dim3(kHistBlock), 0, stream, L, d_partials);
  hipLaunchKernelGGL((range_reduce_kernel<HistLaunch, HistRangeAcc>), dim3(n_tasks), dim3(64), 0, stream, L,
                     (const HistRangeAcc *)d_partials, blocks_per_task, d_accs);
}

// `lds_bytes`: hist_lds_bytes of the launch's largest task
void launch_hist_counts(const HistLaunch &L, int n_tasks, int blocks_per_task, size_t lds_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(hist_counts_kernel, dim3(blocks_per_task, n_tasks), dim3(kHistBlock), lds_bytes, stream, L);
}

}  // namespace tgx
