// histogram_device.cpp -- TGX_CHECK_HISTOGRAM: the two scans behind HistogramAnalyzer
// (TG/analyzers/advanced/histogram.rs:184-330), in two phases (include/tgx.h).
//
// A task is one spec.  Its running state lives on the device -- a HistRangeAcc in the range phase, buckets + 2 64-bit
// counters in the count phase (the buckets, the rows that reached the last bucket through ELSE, the non-finite rows) --
// and is folded by kernels/histogram.hip; rows seen are counted on the host.  The edges of the count-phase tasks are
// uploaded once per state (the plan's edges are fixed once a state exists).  What is merged in from other states or
// read from a blob is kept on the host and added when the state is read: extremes by MIN / MAX, everything else by
// addition.
#include "histogram_device.h"

#include "api_internal.h"

namespace tgx {
size_t hist_range_partial_bytes();
void launch_hist_range(const HistLaunch &L, int n_tasks, int blocks_per_task, void *d_partials, HistRangeAcc *d_accs,
                       hipStream_t stream);
void launch_hist_counts(const HistLaunch &L, int n_tasks, int blocks_per_task, size_t lds_bytes, hipStream_t stream);

namespace {

constexpr uint32_t kHistWireMagic = 0x54534948;  // "HIST"

HistRangeAcc range_identity() {
  HistRangeAcc a;
  a.n = a.non_finite = 0;
  a.min = INFINITY;
  a.max = -INFINITY;
  a.sum = a.sum_squared = 0.0;
  return a;
}

// one task's state as the host sees it
struct HistHost {
  int64_t total = 0;
  HistRangeAcc range = range_identity();  // count phase: n and non_finite only
  std::vector<uint64_t> words;            // count phase: the buckets, then the rows that came through ELSE
};

struct HistState {
  std::vector<HistHost> host;         // merged in / deserialized
  std::vector<int64_t> device_total;  // rows the device part has seen
  std::vector<size_t> word_off;       // per task: first of its counters in d_counts (count phase)
  std::vector<size_t> edge_off;       // per task: first of its edges in d_edges (count phase)
  size_t n_words = 0;
  bool device_ready = false;
  DevBuf d_range, d_counts, d_partials, d_edges;
  std::vector<HistRangeAcc> identity;  // (kept alive: uploaded asynchronously)
  std::vector<double> edges;           // the count-phase tasks' edges, one after the other (kept alive likewise)
};

HistState *hs_of(tgx_state *st) { return (HistState *)st->hist; }

void merge_host(HistHost &a, const HistHost &b) {
  a.total += b.total;
  a.range.n += b.range.n;
  a.range.non_finite += b.range.non_finite;
  a.range.min = std::min(a.range.min, b.range.min);
  a.range.max = std::max(a.range.max, b.range.max);
  a.range.sum += b.range.sum;
  a.range.sum_squared += b.range.sum_squared;
  for (size_t i = 0; i < a.words.size() && i < b.words.size(); i++) a.words[i] += b.words[i];
}

tgx_status device_clear(tgx_state *st, tgx_error *err) {
  HistState *hs = hs_of(st);
  if (!hs->identity.empty())
    HIP_TRY(hipMemcpyAsync(hs->d_range.p, hs->identity.data(), hs->identity.size() * sizeof(HistRangeAcc),
                           hipMemcpyHostToDevice, st->stream));
  if (hs->n_words) HIP_TRY(hipMemsetAsync(hs->d_counts.p, 0, hs->n_words * sizeof(unsigned long long), st->stream));
  return TGX_OK;
}

tgx_status device_init(tgx_state *st, tgx_error *err) {
  HistState *hs = hs_of(st);
  if (hs->device_ready) return TGX_OK;
  const size_t n = st->plan->hist.size();
  hs->identity.assign(n, range_identity());
  HIP_TRY(hs->d_range.reserve(n * sizeof(HistRangeAcc)));
  if (hs->n_words) HIP_TRY(hs->d_counts.reserve(hs->n_words * sizeof(unsigned long long)));
  if (!hs->edges.empty()) {
    HIP_TRY(hs->d_edges.reserve(hs->edges.size() * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(hs->d_edges.p, hs->edges.data(), hs->edges.size() * sizeof(double), hipMemcpyHostToDevice,
                           st->stream));
  }
  TGX_TRY(device_clear(st, err));
  hs->device_ready = true;
  return TGX_OK;
}

// host part + device part of every task (the device part stays where it is)
tgx_status hist_gather(tgx_state *st, std::vector<HistHost> *out, tgx_error *err) {
  HistState *hs = hs_of(st);
  const tgx_plan *plan = st->plan;
  TGX_TRY(coalesce_flush(st, err));  // batches tgx_update has only noted so far
  *out = hs->host;
  if (!hs->device_ready) return TGX_OK;
  std::vector<HistRangeAcc> ranges(plan->hist.size());
  std::vector<unsigned long long> words(hs->n_words);
  HIP_TRY(hipMemcpyAsync(ranges.data(), hs->d_range.p, ranges.size() * sizeof(HistRangeAcc), hipMemcpyDeviceToHost,
                         st->stream));
  if (hs->n_words)
    HIP_TRY(hipMemcpyAsync(words.data(), hs->d_counts.p, words.size() * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, st->stream));
  HIP_TRY(hipStreamSynchronize(st->stream));
  for (size_t k = 0; k < plan->hist.size(); k++) {
    const HistTask &t = plan->hist[k];
    HistHost d;
    d.total = hs->device_total[k];
    if (!t.counted) {
      d.range = ranges[k];
    } else {
      const size_t buckets = t.buckets();
      const unsigned long long *w = words.data() + hs->word_off[k];
      d.words.assign(w, w + buckets + 1);
      for (size_t c = 0; c < buckets; c++) d.range.n += (int64_t)w[c];
      d.range.non_finite = (int64_t)w[buckets + 1];
    }
    merge_host((*out)[k], d);
  }
  return TGX_OK;
}

}  // namespace

tgx_status hist_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  (void)err;
  HistTask t;
  t.column = plan->specs[spec_index].column;
  plan->hist.push_back(t);
  *slot = (int)plan->hist.size() - 1;
  return TGX_OK;
}

void hist_state_init(tgx_state *st) {
  hist_state_free(st);
  const tgx_plan *plan = st->plan;
  if (plan->hist.empty()) return;
  HistState *hs = new HistState();
  hs->host.resize(plan->hist.size());
  hs->device_total.assign(plan->hist.size(), 0);
  hs->word_off.assign(plan->hist.size(), 0);
  hs->edge_off.assign(plan->hist.size(), 0);
  for (size_t k = 0; k < plan->hist.size(); k++) {
    const HistTask &t = plan->hist[k];
    hs->word_off[k] = hs->n_words;
    hs->edge_off[k] = hs->edges.size();
    if (!t.counted) continue;
    hs->n_words += (size_t)t.buckets() + 2;
    hs->edges.insert(hs->edges.end(), t.edges.begin(), t.edges.end());
    hs->host[k].words.assign((size_t)t.buckets() + 1, 0);
  }
  st->hist = hs;
}

void hist_state_free(tgx_state *st) {
  delete hs_of(st);
  st->hist = nullptr;
}

// (the caller has waited for the stream)
tgx_status hist_state_reset(tgx_state *st, tgx_error *err) {
  HistState *hs = hs_of(st);
  if (!hs) return TGX_OK;
  for (HistHost &h : hs->host) {
    h.total = 0;
    h.range = range_identity();
    std::fill(h.words.begin(), h.words.end(), 0);
  }
  std::fill(hs->device_total.begin(), hs->device_total.end(), 0);
  if (hs->device_ready) TGX_TRY(device_clear(st, err));
  return TGX_OK;
}

tgx_status hist_update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) {
  const tgx_plan *plan = st->plan;
  HistState *hs = hs_of(st);
  if (!hs || nrows <= 0) return TGX_OK;
  TGX_TRY(device_init(st, err));
  // the tasks of each phase in launches of up to kMaxHistPerLaunch columns (grid.y)
  for (int phase = 0; phase < 2; phase++) {
    std::vector<int> tasks;
    for (size_t k = 0; k < plan->hist.size(); k++)
      if ((int)plan->hist[k].counted == phase) tasks.push_back((int)k);
    for (size_t t0 = 0; t0 < tasks.size(); t0 += kMaxHistPerLaunch) {
      const int n = (int)std::min<size_t>(kMaxHistPerLaunch, tasks.size() - t0);
      HistLaunch L;
      memset(&L, 0, sizeof(L));
      uint64_t bytes = 0;
      size_t lds = 0;
      for (int k = 0; k < n; k++) {
        const int slot = tasks[t0 + k];
        const HistTask &t = plan->hist[slot];
        const tgx_column &x = dev[t.column];
        if (!is_numeric(x.type)) return fail(err, TGX_UNSUPPORTED, "HISTOGRAM takes numeric columns (%d)", x.type);
        ComomentColDesc &d = L.cols[k];
        d.x = x.values;
        d.xv = x.validity;
        d.xoff = x.offset;
        d.length = x.length;
        d.x_is_float = x.type == TGX_FLOAT64;
        L.edges[k] = t.counted ? hs->d_edges.as<double>() + hs->edge_off[slot] : nullptr;
        L.buckets[k] = t.buckets();
        L.counters[k] = t.counted ? hs->d_counts.as<unsigned long long>() + hs->word_off[slot] : nullptr;
        L.acc_index[k] = slot;
        if (t.counted) lds = std::max(lds, hist_lds_bytes(t.buckets()));
        bytes += (uint64_t)x.length * 8 + (x.validity ? (uint64_t)(x.length + 7) / 8 : 0);
        hs->device_total[slot] += nrows;
      }
      // 8 waves a workgroup, up to 4 workgroups a CU (the count phase's LDS, at most 12 KB, leaves room for them)
      const int blocks = (int)std::min<int64_t>(std::max<int64_t>(1, (nrows + kHistBlock * 16 - 1) / (kHistBlock * 16)),
                                                std::max(32, (g_ctx.n_cu * 4) / n));
      // (a workgroup's buckets are 32-bit counters)
      if (nrows / blocks >= ((int64_t)1 << 32))
        return fail(err, TGX_UNSUPPORTED, "HISTOGRAM: a batch of %lld rows is too long", (long long)nrows);
      (void)hipGetLastError();  // (what the launches below leave is theirs)
      if (phase == 0) {
        HIP_TRY(hs->d_partials.reserve((size_t)n * blocks * hist_range_partial_bytes()));
        ProfScope ps(st, "hist_range", bytes);
        launch_hist_range(L, n, blocks, hs->d_partials.p, hs->d_range.as<HistRangeAcc>(), st->stream);
      } else {
        ProfScope ps(st, "hist_counts", bytes);
        launch_hist_counts(L, n, blocks, lds, st->stream);
      }
      HIP_TRY(hipGetLastError());
    }
  }
  return TGX_OK;
}

tgx_status hist_fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) {
  std::vector<HistHost> g;
  TGX_TRY(hist_gather(st, &g, err));
  r->total = g[slot].total;
  r->non_null = g[slot].range.n + g[slot].range.non_finite;
  return TGX_OK;
}

tgx_status hist_merge_states(tgx_state *dst, tgx_state *src, tgx_error *err) {
  HistState *hd = hs_of(dst);
  if (!hd) return TGX_OK;
  std::vector<HistHost> g;
  TGX_TRY(hist_gather(src, &g, err));
  for (size_t k = 0; k < g.size(); k++) {
    // (states of one plan share its edges; a blob made under other edges was refused by tgx_state_deserialize)
    if (g[k].words.size() != hd->host[k].words.size())
      return fail(err, TGX_INVALID_ARGUMENT, "HISTOGRAM task %zu: the states were counted under different edges", k);
    merge_host(hd->host[k], g[k]);
  }
  return TGX_OK;
}

// section: { u32 magic "HIST", u32 tasks; per task { u32 counted, u32 buckets, f64 edges[buckets + 1] (count phase only),
//   i64 total, n, non_finite, f64 min, max, sum, sum_squared, u64 n_words, u64 words[n_words] } }
// n_words = buckets + 1 in the count phase (the buckets, then the rows that came through ELSE), else 0
tgx_status hist_serialize(tgx_state *st, Writer &w, tgx_error *err) {
  const tgx_plan *plan = st->plan;
  if (plan->hist.empty()) return TGX_OK;
  std::vector<HistHost> g;
  TGX_TRY(hist_gather(st, &g, err));
  w.pod(kHistWireMagic);
  w.pod((uint32_t)plan->hist.size());
  for (size_t k = 0; k < g.size(); k++) {
    const HistTask &t = plan->hist[k];
    const uint32_t phase[2] = {t.counted ? 1u : 0u, t.buckets()};
    w.pod(phase);
    w.put(t.edges.data(), t.edges.size() * sizeof(double));
    const int64_t counts[3] = {g[k].total, g[k].range.n, g[k].range.non_finite};
    w.pod(counts);
    const double vals[4] = {g[k].range.min, g[k].range.max, g[k].range.sum, g[k].range.sum_squared};
    w.pod(vals);
    w.pod((uint64_t)g[k].words.size());
    w.put(g[k].words.data(), g[k].words.size() * sizeof(uint64_t));
  }
  return TGX_OK;
}

tgx_status hist_deserialize(tgx_state *st, Reader &r, tgx_error *err) {
  const tgx_plan *plan = st->plan;
  HistState *hs = hs_of(st);
  if (!hs) return TGX_OK;
  const uint32_t magic = r.pod<uint32_t>(), tasks = r.pod<uint32_t>();
  if (!r.ok || magic != kHistWireMagic || tasks != plan->hist.size())
    return fail(err, TGX_INVALID_ARGUMENT, "state blob was produced by a different plan (HISTOGRAM section)");
  for (size_t k = 0; k < plan->hist.size(); k++) {
    const HistTask &t = plan->hist[k];
    uint32_t phase[2];
    r.get(phase, sizeof(phase));
    if (!r.ok) break;
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
    if (!r.ok) break;
    if (!edges.empty() && memcmp(edges.data(), t.edges.data(), edges.size() * sizeof(double)) != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "HISTOGRAM task %zu: the blob was counted under other edges than the plan's (%u buckets)", k, phase[1]);
    HistHost &h = hs->host[k];
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
  }
  if (!r.ok) return fail(err, TGX_INVALID_ARGUMENT, "truncated state blob");
  return TGX_OK;
}

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
  TGX_TRY(hist_gather(st, &g, err));
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
  TGX_TRY(hist_gather(st, &g, err));
  memcpy(counts, g[slot].words.data(), n * sizeof(uint64_t));
  if (else_rows) *else_rows = g[slot].words[n];
  if (non_finite) *non_finite = (uint64_t)g[slot].range.non_finite;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
