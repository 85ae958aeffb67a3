// temporal_device.cpp -- TGX_CHECK_TEMPORAL: the row predicates behind the reference's TemporalOrderingConstraint
// (TG/constraints/temporal_ordering.rs:346-453; include/tgx.h has the modes and the NULL rules).
//
// A task is one spec.  Its running state on the device is two 64-bit counters folded by kernels/temporal.hip -- the rows
// that are non-NULL and pass the weekday filter, and those of them that pass the predicate; rows seen are counted on the
// host.  What is merged in from other states or read from a blob is kept on the host and added when the state is read.
// {seen, considered, violations} follow from the three numbers and the task's flags (counts_of).
#include "temporal_device.h"

#include "api_internal.h"

namespace tgx {
void launch_temporal(const TemporalLaunch &L, int n_tasks, int blocks_per_task, hipStream_t stream);

namespace {

constexpr uint32_t kTemporalWireMagic = 0x52504d54;  // "TMPR"

// one task's state as the host sees it
struct TemporalHost {
  uint64_t seen = 0, live = 0, passed = 0;  // live: non-NULL and through the weekday filter
};

struct TemporalState {
  std::vector<TemporalHost> host;      // merged in / deserialized
  std::vector<uint64_t> device_seen;   // rows the device part has seen
  bool device_ready = false;
  DevBuf d_counts;  // per task: live, passed
};

TemporalState *ts_of(tgx_state *st) { return (TemporalState *)st->temporal; }

void merge_host(TemporalHost &a, const TemporalHost &b) {
  a.seen += b.seen;
  a.live += b.live;
  a.passed += b.passed;
}

// The SQL's NULL rules (include/tgx.h).  Without KEEP_NULLS the IS NOT NULL terms of the WHERE clause drop a NULL row;
// with it the row is considered and its predicate is SQL NULL: the ELSE branch, a violation.  The weekday term of the
// WHERE clause is NULL for a NULL row, so such a row never gets past it.
tgx_temporal_counts counts_of(const TemporalTask &t, const TemporalHost &h) {
  tgx_temporal_counts c;
  c.seen = h.seen;
  const bool nulls_in = (t.flags & TGX_TEMPORAL_KEEP_NULLS) && !t.params.weekdays_only;
  c.considered = nulls_in ? h.seen : h.live;
  c.violations = c.considered - h.passed;
  return c;
}

// workgroups per task: 16 rows a lane before another workgroup is worth its launch; 8 waves a workgroup, up to 4
// workgroups a CU, shared by the tasks of the launch
int temporal_blocks(int64_t nrows, int n_cu, int n_tasks) {
  return (int)std::min<int64_t>(std::max<int64_t>(1, (nrows + kTemporalBlock * 16 - 1) / (kTemporalBlock * 16)),
                                std::max(32, (n_cu * 4) / n_tasks));
}

tgx_status device_clear(tgx_state *st, tgx_error *err) {
  TemporalState *ts = ts_of(st);
  HIP_TRY(hipMemsetAsync(ts->d_counts.p, 0, ts->host.size() * 2 * sizeof(unsigned long long), st->stream));
  return TGX_OK;
}

tgx_status device_init(tgx_state *st, tgx_error *err) {
  TemporalState *ts = ts_of(st);
  if (ts->device_ready) return TGX_OK;
  HIP_TRY(ts->d_counts.reserve(ts->host.size() * 2 * sizeof(unsigned long long)));
  TGX_TRY(device_clear(st, err));
  ts->device_ready = true;
  return TGX_OK;
}

// host part + device part of every task (the device part stays where it is)
tgx_status temporal_gather(tgx_state *st, std::vector<TemporalHost> *out, tgx_error *err) {
  TemporalState *ts = ts_of(st);
  TGX_TRY(coalesce_flush(st, err));  // batches tgx_update has only noted so far
  *out = ts->host;
  if (!ts->device_ready) return TGX_OK;
  std::vector<unsigned long long> words(ts->host.size() * 2);
  HIP_TRY(hipMemcpyAsync(words.data(), ts->d_counts.p, words.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                         st->stream));
  HIP_TRY(hipStreamSynchronize(st->stream));
  for (size_t k = 0; k < out->size(); k++) {
    TemporalHost d;
    d.seen = ts->device_seen[k];
    d.live = words[2 * k];
    d.passed = words[2 * k + 1];
    merge_host((*out)[k], d);
  }
  return TGX_OK;
}

}  // namespace

tgx_status temporal_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 < -1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: TEMPORAL: column2 is the after column or -1 (%d)", spec_index, sp.column2);
  TemporalTask t;
  memset(&t, 0, sizeof(t));
  t.column = sp.column;
  t.column2 = sp.column2;  // (held against the mode by tgx_plan_set_temporal)
  t.spec_index = spec_index;
  plan->temporal.push_back(t);
  *slot = (int)plan->temporal.size() - 1;
  return TGX_OK;
}

tgx_status temporal_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const TemporalTask &t : plan->temporal)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a TEMPORAL check needs its parameters (tgx_plan_set_temporal)",
                  t.spec_index);
  return TGX_OK;
}

void temporal_state_init(tgx_state *st) {
  temporal_state_free(st);
  const tgx_plan *plan = st->plan;
  if (plan->temporal.empty()) return;
  TemporalState *ts = new TemporalState();
  ts->host.resize(plan->temporal.size());
  ts->device_seen.assign(plan->temporal.size(), 0);
  st->temporal = ts;
}

void temporal_state_free(tgx_state *st) {
  delete ts_of(st);
  st->temporal = nullptr;
}

// (the caller has waited for the stream)
tgx_status temporal_state_reset(tgx_state *st, tgx_error *err) {
  TemporalState *ts = ts_of(st);
  if (!ts) return TGX_OK;
  for (TemporalHost &h : ts->host) h = TemporalHost();
  std::fill(ts->device_seen.begin(), ts->device_seen.end(), 0);
  if (ts->device_ready) TGX_TRY(device_clear(st, err));
  return TGX_OK;
}

tgx_status temporal_update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) {
  const tgx_plan *plan = st->plan;
  TemporalState *ts = ts_of(st);
  if (!ts || nrows <= 0) return TGX_OK;
  TGX_TRY(device_init(st, err));
  // all tasks in launches of up to kMaxTemporalPerLaunch (grid.y)
  for (size_t t0 = 0; t0 < plan->temporal.size(); t0 += kMaxTemporalPerLaunch) {
    const int n = (int)std::min<size_t>(kMaxTemporalPerLaunch, plan->temporal.size() - t0);
    TemporalLaunch L;
    memset(&L, 0, sizeof(L));
    uint64_t bytes = 0;
    for (int k = 0; k < n; k++) {
      const size_t slot = t0 + k;
      const TemporalTask &t = plan->temporal[slot];
      const bool pair = t.params.mode == kTemporalOrder;
      // (Int64 views: update_validate refuses every other type of a column a TEMPORAL check reads)
      const tgx_column &x = dev[t.column], &y = dev[pair ? t.column2 : t.column];
      ComomentColDesc &d = L.cols[k];
      d.x = x.values;
      d.xv = x.validity;
      d.xoff = x.offset;
      d.y = y.values;
      d.yv = y.validity;
      d.yoff = y.offset;
      d.length = x.length;
      L.params[k] = t.params;
      L.counters[k] = ts->d_counts.as<unsigned long long>() + 2 * slot;
      bytes += (uint64_t)x.length * 8 + (x.validity ? (uint64_t)(x.length + 7) / 8 : 0);
      if (pair) bytes += (uint64_t)y.length * 8 + (y.validity ? (uint64_t)(y.length + 7) / 8 : 0);
    }
    const int blocks = temporal_blocks(nrows, g_ctx.n_cu, n);
    // (a lane's and a wave's counters are 32-bit)
    if (nrows / blocks >= ((int64_t)1 << 32))
      return fail(err, TGX_UNSUPPORTED, "TEMPORAL: a batch of %lld rows is too long", (long long)nrows);
    ProfScope ps(st, "temporal", bytes);
    launch_temporal(L, n, blocks, st->stream);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < n; k++) ts->device_seen[t0 + k] += (uint64_t)nrows;  // (only rows the device was given)
  }
  return TGX_OK;
}

tgx_status temporal_fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) {
  std::vector<TemporalHost> g;
  TGX_TRY(temporal_gather(st, &g, err));
  const tgx_temporal_counts c = counts_of(st->plan->temporal[slot], g[slot]);
  r->total = (int64_t)c.seen;
  r->non_null = (int64_t)c.considered;
  r->matches = (int64_t)(c.considered - c.violations);
  return TGX_OK;
}

tgx_status temporal_merge_states(tgx_state *dst, tgx_state *src, tgx_error *err) {
  TemporalState *td = ts_of(dst);
  if (!td) return TGX_OK;
  std::vector<TemporalHost> g;
  TGX_TRY(temporal_gather(src, &g, err));
  for (size_t k = 0; k < g.size(); k++) merge_host(td->host[k], g[k]);
  return TGX_OK;
}

// section: { u32 magic "TMPR", u32 tasks; per task { i32 mode, u32 flags, i64 delta, ticks_per_second, lo, hi (the
//   plan's parameters), u64 seen, live, passed } }
tgx_status temporal_serialize(tgx_state *st, Writer &w, tgx_error *err) {
  const tgx_plan *plan = st->plan;
  if (plan->temporal.empty()) return TGX_OK;
  std::vector<TemporalHost> g;
  TGX_TRY(temporal_gather(st, &g, err));
  w.pod(kTemporalWireMagic);
  w.pod((uint32_t)plan->temporal.size());
  for (size_t k = 0; k < g.size(); k++) {
    const TemporalTask &t = plan->temporal[k];
    const uint32_t head[2] = {(uint32_t)t.params.mode, t.flags};
    w.pod(head);
    const int64_t params[4] = {t.params.delta, t.params.ticks_per_second, t.params.lo, t.params.hi};
    w.pod(params);
    const uint64_t counts[3] = {g[k].seen, g[k].live, g[k].passed};
    w.pod(counts);
  }
  return TGX_OK;
}

tgx_status temporal_deserialize(tgx_state *st, Reader &r, tgx_error *err) {
  const tgx_plan *plan = st->plan;
  TemporalState *ts = ts_of(st);
  if (!ts) return TGX_OK;
  const uint32_t magic = r.pod<uint32_t>(), tasks = r.pod<uint32_t>();
  if (!r.ok || magic != kTemporalWireMagic || tasks != plan->temporal.size())
    return fail(err, TGX_INVALID_ARGUMENT, "state blob was produced by a different plan (TEMPORAL section)");
  for (size_t k = 0; k < plan->temporal.size(); k++) {
    const TemporalTask &t = plan->temporal[k];
    uint32_t head[2];
    int64_t params[4];
    uint64_t counts[3];
    r.get(head, sizeof(head));
    r.get(params, sizeof(params));
    r.get(counts, sizeof(counts));
    if (!r.ok) break;
    const int64_t mine[4] = {t.params.delta, t.params.ticks_per_second, t.params.lo, t.params.hi};
    if (head[0] != (uint32_t)t.params.mode || head[1] != t.flags || memcmp(params, mine, sizeof(mine)) != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "TEMPORAL task %zu: the blob was counted under other parameters (mode %u) than the plan's (mode %d)", k,
                  head[0], t.params.mode);
    if (counts[1] > counts[0] || counts[2] > counts[1])
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (TEMPORAL task %zu)", k);
    ts->host[k].seen = counts[0];
    ts->host[k].live = counts[1];
    ts->host[k].passed = counts[2];
  }
  if (!r.ok) return fail(err, TGX_INVALID_ARGUMENT, "truncated state blob");
  return TGX_OK;
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_temporal(tgx_plan *plan, size_t spec_index, const tgx_temporal_params *p,
                                            tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_TEMPORAL, "TEMPORAL", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the parameters of a TEMPORAL check are fixed once a state of the plan exists");
  TemporalTask &t = plan->temporal[slot];
  if (p->flags & ~(uint32_t)(TGX_TEMPORAL_KEEP_NULLS | TGX_TEMPORAL_WEEKDAYS_ONLY))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: unknown TEMPORAL flags 0x%x", spec_index, p->flags);
  if ((p->flags & TGX_TEMPORAL_WEEKDAYS_ONLY) && p->mode != TGX_TEMPORAL_TIME_OF_DAY)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: WEEKDAYS_ONLY goes with the time-of-day mode only", spec_index);
  TemporalParams d;
  memset(&d, 0, sizeof(d));
  switch (p->mode) {
    case TGX_TEMPORAL_ORDER:
      if (t.column2 < 0) return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the order mode needs column2", spec_index);
      d.mode = kTemporalOrder;
      d.delta = p->delta;
      break;
    case TGX_TEMPORAL_TIME_OF_DAY:
      if (p->ticks_per_second != 1 && p->ticks_per_second != 1000 && p->ticks_per_second != 1000000 &&
          p->ticks_per_second != 1000000000)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: ticks_per_second must be 1, 10^3, 10^6 or 10^9 (%lld)",
                    spec_index, (long long)p->ticks_per_second);
      d.mode = kTemporalTimeOfDay;
      d.ticks_per_second = p->ticks_per_second;
      d.lo = p->tod_lo;
      d.hi = p->tod_hi;
      d.weekdays_only = (p->flags & TGX_TEMPORAL_WEEKDAYS_ONLY) ? 1 : 0;
      break;
    case TGX_TEMPORAL_RANGE:
      d.mode = kTemporalRange;
      d.lo = p->lo;
      d.hi = p->hi;
      break;
    default:
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: unknown TEMPORAL mode %d", spec_index, p->mode);
  }
  if (p->mode != TGX_TEMPORAL_ORDER && t.column2 >= 0)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: column2 goes with the order mode only", spec_index);
  t.params = d;
  t.flags = p->flags;
  t.set = true;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_temporal_get(const tgx_plan *plan, tgx_state *st, size_t spec_index, tgx_temporal_counts *out,
                                       tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_TEMPORAL, "TEMPORAL", &slot, err, "bad arguments"));
  std::vector<TemporalHost> g;
  TGX_TRY(temporal_gather(st, &g, err));
  *out = counts_of(plan->temporal[slot], g[slot]);
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
