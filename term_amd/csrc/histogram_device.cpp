// histogram_device.cpp -- TGX_CHECK_HISTOGRAM: the two scans behind HistogramAnalyzer
// (TG/analyzers/advanced/histogram.rs:184-330), in two phases (include/tgx.h).
//
// A task is one spec.  Its running state lives on the device -- a HistRangeAcc in the range phase, buckets + 2 64-bit
// counters in the count phase (the buckets, the rows that reached the last bucket through ELSE, the non-finite rows) --
// and is folded by kernels/histogram.hip; rows seen are counted on the host.  The edges of the count-phase tasks are
// uploaded once per state (the plan's edges are fixed once a state exists).  What is merged in from other states or
// read from a blob is kept on the host and added when the state is read: extremes by MIN / MAX, everything else by
// addition.
#include "api_internal.h"

namespace tgx {
void launch_hist_range(const HistLaunch &L, int n_tasks, int blocks_per_task, HistRangeAcc *d_partials,
                       HistRangeAcc *d_accs, hipStream_t stream);
void launch_hist_counts(const HistLaunch &L, int n_tasks, int blocks_per_task, size_t lds_bytes, hipStream_t stream);

namespace {

// one task's state as the host sees it
struct HistHost {
  int64_t total = 0;
  HistRangeAcc range;           // count phase: n and non_finite only
  std::vector<uint64_t> words;  // count phase: the buckets, then the rows that came through ELSE
};

struct HistKind {
  typedef HistTask Task;
  typedef HistHost Host;
  typedef HistRangeAcc Range;
  static constexpr bool kRanged = true;
  static constexpr int kKind = TGX_CHECK_HISTOGRAM;
  static constexpr const char *kDiffers = "edges";
  static constexpr uint32_t kMagic = 0x54534948;  // "HIST"

  static const std::vector<HistTask> &tasks(const tgx_plan *plan) { return plan->hist; }
  static size_t words(const HistTask &t) { return t.counted ? (size_t)t.buckets() + 2 : 0; }
  static HistRangeAcc range_identity() {
    HistRangeAcc a;
    a.n = a.non_finite = 0;
    a.min = INFINITY;
    a.max = -INFINITY;
    a.sum = a.sum_squared = 0.0;
    return a;
  }
  static HistHost fresh(const HistTask &t) {
    HistHost h;
    h.range = range_identity();
    if (t.counted) h.words.assign((size_t)t.buckets() + 1, 0);
    return h;
  }
  static size_t shape(const HistHost &h) { return h.words.size(); }

  static HistHost from_device(const HistTask &t, int64_t rows, const HistRangeAcc &range, const unsigned long long *w) {
    HistHost d = fresh(t);
    d.total = rows;
    if (!t.counted) {
      d.range = range;
    } else {
      const size_t buckets = t.buckets();
      d.words.assign(w, w + buckets + 1);
      for (size_t c = 0; c < buckets; c++) d.range.n += (int64_t)w[c];
      d.range.non_finite = (int64_t)w[buckets + 1];
    }
    return d;
  }

  static void merge_host(HistHost &a, const HistHost &b) {
    a.total += b.total;
    a.range.n += b.range.n;
    a.range.non_finite += b.range.non_finite;
    a.range.min = std::min(a.range.min, b.range.min);
    a.range.max = std::max(a.range.max, b.range.max);
    a.range.sum += b.range.sum;
    a.range.sum_squared += b.range.sum_squared;
    for (size_t i = 0; i < a.words.size() && i < b.words.size(); i++) a.words[i] += b.words[i];
  }

  // per task { u32 counted, u32 buckets, f64 edges[buckets + 1] (count phase only), i64 total, n, non_finite,
  //   f64 min, max, sum, sum_squared, u64 n_words, u64 words[n_words] }
  // n_words = buckets + 1 in the count phase (the buckets, then the rows that came through ELSE), else 0
  static void write(const HistTask &t, const HistHost &h, Writer &w) {
    const uint32_t phase[2] = {t.counted ? 1u : 0u, t.buckets()};
    w.pod(phase);
    w.put(t.edges.data(), t.edges.size() * sizeof(double));
    const int64_t counts[3] = {h.total, h.range.n, h.range.non_finite};
    w.pod(counts);
    const double vals[4] = {h.range.min, h.range.max, h.range.sum, h.range.sum_squared};
    w.pod(vals);
    w.pod((uint64_t)h.words.size());
    w.put(h.words.data(), h.words.size() * sizeof(uint64_t));
  }

  static tgx_status read(const HistTask &t, HistHost &h, Reader &r, size_t k, tgx_error *err) {
    uint32_t phase[2];
    r.get(phase, sizeof(phase));
    if (!r.ok) return TGX_OK;
    if (phase[0] != (t.counted ? 1u : 0u) || phase[1] != t.buckets())
      return fail(err, TGX_INVALID_ARGUMENT,
                  "HISTOGRAM task %zu: the blob was counted under other edges (%u buckets) than the plan's (%u buckets)", k,
                  phase[1], t.buckets());
    std::vector<double> edges(t.edges.size());
    r.get(edges.data(), edges.size() * sizeof(double));
    int64_t counts[3];
    double vals[4];
    r.get(counts, sizeof(counts));
    r.get(vals, sizeof(vals));
    const uint64_t n_words = r.pod<uint64_t>();
    if (!r.ok) return TGX_OK;
    if (!edges.empty() && memcmp(edges.data(), t.edges.data(), edges.size() * sizeof(double)) != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "HISTOGRAM task %zu: the blob was counted under other edges than the plan's (%u buckets)", k, phase[1]);
    size_t bytes = 0;
    if (n_words != h.words.size() || !r.fits(n_words, sizeof(uint64_t), &bytes))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (HISTOGRAM task %zu)", k);
    h.total = counts[0];
    h.range.n = counts[1];
    h.range.non_finite = counts[2];
    h.range.min = vals[0];
    h.range.max = vals[1];
    h.range.sum = vals[2];
    h.range.sum_squared = vals[3];
    r.get(h.words.data(), bytes);
    // what the accessors rely on: counts that add up (nulls = total - n - non_finite), a range that is one
    uint64_t in_buckets = 0;
    for (uint32_t c = 0; c < t.buckets(); c++) in_buckets += h.words[c];
    const bool counts_ok = counts[1] >= 0 && counts[2] >= 0 && counts[1] <= counts[0] && counts[2] <= counts[0] - counts[1];
    const bool phase_ok = t.counted ? in_buckets == (uint64_t)counts[1] && h.words[t.buckets()] <= h.words[t.buckets() - 1]
                                    : counts[1] == 0 || (std::isfinite(vals[0]) && std::isfinite(vals[1]) && vals[0] <= vals[1]);
    if (r.ok && !(counts_ok && phase_ok))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (HISTOGRAM task %zu: inconsistent counts or range)", k);
    return TGX_OK;
  }
};

struct HistCheck final : SideState<HistKind> {
  std::vector<size_t> edge_off;  // per task: first of its edges in d_edges (count phase)
  std::vector<double> edges;     // the count-phase tasks' edges, one after the other (kept alive: uploaded asynchronously)
  DevBuf d_edges;

  explicit HistCheck(const tgx_plan *plan) : SideState(plan) {
    for (const HistTask &t : plan->hist) {
      edge_off.push_back(edges.size());
      edges.insert(edges.end(), t.edges.begin(), t.edges.end());  // (none in the range phase)
    }
  }

  tgx_status device_init_extra(tgx_state *st, tgx_error *err) override {
    if (edges.empty()) return TGX_OK;
    HIP_TRY(d_edges.reserve(edges.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(d_edges.p, edges.data(), edges.size() * sizeof(double), hipMemcpyHostToDevice, st->stream));
    return TGX_OK;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    for (int phase = 0; phase < 2; phase++) {
      auto launch = [&](const int *slots, int n) -> tgx_status {
        HistLaunch L;
        memset(&L, 0, sizeof(L));
        uint64_t bytes = 0;
        size_t lds = 0;
        for (int k = 0; k < n; k++) {
          const int slot = slots[k];
          const HistTask &t = plan->hist[slot];
          const tgx_column &x = dev[t.column];
          if (!is_numeric(x.type)) return fail(err, TGX_UNSUPPORTED, "HISTOGRAM takes numeric columns (%d)", x.type);
          bytes += side_fill_x(L.cols[k], x);
          L.edges[k] = t.counted ? d_edges.as<double>() + edge_off[slot] : nullptr;
          L.buckets[k] = t.buckets();
          L.counters[k] = t.counted ? d_counts.as<unsigned long long>() + word_off[slot] : nullptr;
          L.acc_index[k] = slot;
          if (t.counted) lds = std::max(lds, hist_lds_bytes(t.buckets()));
          device_rows[slot] += nrows;
        }
        // 8 waves a workgroup, up to 4 workgroups a CU (the count phase's LDS, at most 12 KB, leaves room for them)
        const int blocks = side_blocks(nrows, kHistBlock, g_ctx.n_cu, 4, n);
        TGX_TRY(side_rows_fit("HISTOGRAM", nrows, blocks, err));
        (void)hipGetLastError();  // (what the launches below leave is theirs)
        if (phase == 0) {
          HIP_TRY(d_partials.reserve((size_t)n * blocks * sizeof(HistRangeAcc)));
          ProfScope ps(st, "hist_range", bytes);
          launch_hist_range(L, n, blocks, d_partials.as<HistRangeAcc>(), d_range.as<HistRangeAcc>(), st->stream);
        } else {
          ProfScope ps(st, "hist_counts", bytes);
          launch_hist_counts(L, n, blocks, lds, st->stream);
        }
        HIP_TRY(hipGetLastError());
        return TGX_OK;
      };
      TGX_TRY(side_launches(plan->hist, [&](const HistTask &t) { return (int)t.counted == phase; }, launch));
    }
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    std::vector<HistHost> g;
    TGX_TRY(gather(st, &g, err));
    r->total = g[slot].total;
    r->non_null = g[slot].range.n + g[slot].range.non_finite;
    return TGX_OK;
  }
};

}  // namespace

tgx_status hist_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  (void)err;
  HistTask t;
  t.column = plan->specs[spec_index].column;
  plan->hist.push_back(t);
  *slot = (int)plan->hist.size() - 1;
  return TGX_OK;
}

void hist_mark_columns(tgx_plan *plan) {
  for (const HistTask &t : plan->hist) {
    side_mark(plan, HistCheck::kIndex, t.column, true);
    plan->stats_on[t.column] = 1;
  }
}

tgx_status hist_check_column(const tgx_plan *, int column, const tgx_column &c, tgx_error *err) {
  if (!is_numeric(c.type) && !is_widened(c.type))
    return fail(err, TGX_UNSUPPORTED, "column %d: HISTOGRAM takes numeric columns (type %d)", column, c.type);
  return TGX_OK;
}

SideCheck *hist_state_new(const tgx_plan *plan) { return plan->hist.empty() ? nullptr : new HistCheck(plan); }

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_histogram_edges(tgx_plan *plan, size_t spec_index, const double *edges,
                                                   uint32_t buckets, tgx_error *err) try {
  if (!plan || !edges) return fail(err, TGX_INVALID_ARGUMENT, "plan/edges is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_HISTOGRAM, "HISTOGRAM", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the edges of a HISTOGRAM check are fixed once a state of the plan exists");
  if (buckets < 1 || buckets > kHistMaxBuckets)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: %u buckets: between 1 and %u are supported", spec_index, buckets,
                kHistMaxBuckets);
  for (uint32_t i = 0; i <= buckets; i++)
    if (!std::isfinite(edges[i]))
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: edge %u is not finite (a range whose difference overflows has no "
                  "bucket width)", spec_index, i);
  // (the last edge may lie below the one before: the reference's own formula does that on ranges a few ulps wide)
  for (uint32_t i = 1; i < buckets; i++)
    if (edges[i] < edges[i - 1])
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: edge %u lies below edge %u: edges[0 .. buckets-1] must be "
                  "non-decreasing", spec_index, i, i - 1);
  HistTask &t = plan->hist[slot];
  t.counted = true;
  t.edges.assign(edges, edges + buckets + 1);
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_histogram_range_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                              tgx_histogram_range *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_HISTOGRAM, "HISTOGRAM", &slot, err, "bad arguments"));
  std::vector<HistHost> g;
  TGX_TRY(HistCheck::of(st)->gather(st, &g, err));
  const HistHost &h = g[slot];
  const bool ranged = !plan->hist[slot].counted;
  out->total = (uint64_t)h.total;
  out->n = (uint64_t)h.range.n;
  out->non_finite = (uint64_t)h.range.non_finite;
  // (NULLs are what is neither: in the count phase as well)
  out->nulls = (uint64_t)(h.total - h.range.n - h.range.non_finite);
  out->min = ranged && h.range.n > 0 ? h.range.min : NAN;
  out->max = ranged && h.range.n > 0 ? h.range.max : NAN;
  out->sum = ranged ? h.range.sum : NAN;
  out->sum_squared = ranged ? h.range.sum_squared : NAN;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_histogram_counts(const tgx_plan *plan, tgx_state *st, size_t spec_index, uint64_t *counts,
                                           size_t cap, uint64_t *else_rows, uint64_t *non_finite, tgx_error *err) try {
  bind_thread();
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_HISTOGRAM, "HISTOGRAM", &slot, err, "bad arguments"));
  const HistTask &t = plan->hist[slot];
  if (!t.counted)
    return fail(err, TGX_INVALID_ARGUMENT,
                "spec %zu is in its range phase: no edges were set (tgx_plan_set_histogram_edges)", spec_index);
  const size_t n = t.buckets();
  if (!counts || cap < n)
    return fail(err, TGX_INVALID_ARGUMENT, "counts has room for %zu of %zu buckets", counts ? cap : (size_t)0, n);
  std::vector<HistHost> g;
  TGX_TRY(HistCheck::of(st)->gather(st, &g, err));
  memcpy(counts, g[slot].words.data(), n * sizeof(uint64_t));
  if (else_rows) *else_rows = g[slot].words[n];
  if (non_finite) *non_finite = (uint64_t)g[slot].range.non_finite;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
