// timegap_device.cpp -- TGX_CHECK_TIME_GAP: keeps the non-NULL timestamps (and group keys) of every batch on the device
// and answers at finalize with the sample sort of kernels/sortrank.hip plus one neighbour pass (kernels/timegap.hip;
// include/tgx.h has the rules).  No blob section: timegap_check_mergeable refuses a state that holds rows.
//
// A task is one (timestamp column, group column); its specs differ in their thresholds only and share the retained rows
// and the sort.  The rows lie in two lists of one pair of arrays: rows with a group at the front (timestamp key and
// group key side by side), rows whose group is NULL at the back of the timestamp array (one partition of their own).
//
// Ungrouped (and the NULL-group list): one keys-only sort, then the neighbour pass over the sorted keys.
// Grouped: (1) sort by timestamp with the group key as payload; (2) RANK() of the group keys of that sequence, scattered
// back to the sequence's positions; (3) compose (rank << 32) | position, the timestamp as payload; (4) sort those: every
// partition's rows now lie side by side, in timestamp order; (5) the neighbour pass opens a gap only where the high
// halves of neighbouring composed keys agree.
#include "timegap_device.h"

#include "kernels/sortrank.h"
#include "kernels/timegap.h"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>

namespace tgx {

namespace {
struct TimeGapPlan {
  std::vector<TimeGapTask> tasks;
};
struct TimeGapTaskState {
  DevBuf kt, kg, count;     // timestamp keys, group keys, {rows at the front, rows at the back}
  uint64_t capacity = 0;    // rows the arrays can hold
  uint64_t rows_upper = 0;  // host-side bound on the rows retained so far
  uint64_t total_rows = 0;  // rows seen
  // the last answer, until a batch arrives or the state is reset
  bool cached = false;
  uint64_t rows = 0, gaps = 0, largest = 0;
  std::vector<uint64_t> violations;  // per spec of the task
};
struct TimeGapState {
  std::vector<TimeGapTaskState> tasks;
  // work buffers of the sorts, shared by the tasks (they are answered one after the other) and kept between calls:
  // the passes' ping-pong space (keys, payloads), the outputs of the three sorts, the sorter's tables, counters + status
  DevBuf w[4], t1, g1, ranks, t3, back_sorted, temp, small;
};
constexpr size_t kCounterWords = 2 + kTimeGapThresholds;
constexpr size_t kStatusOffset = 128;  // of the sort's status word in `small`

const TimeGapPlan *tplan(const tgx_plan *p) { return (const TimeGapPlan *)p->timegap; }
TimeGapState *tstate(tgx_state *s) { return (TimeGapState *)s->timegap; }

tgx_status read_counts(tgx_state *st, TimeGapTaskState &ts, unsigned long long out[2], tgx_error *err) {
  out[0] = out[1] = 0;
  if (!ts.count.p) return TGX_OK;
  HIP_TRY(hipMemcpyAsync(out, ts.count.p, 16, hipMemcpyDeviceToHost, st->stream));
  HIP_TRY(hipStreamSynchronize(st->stream));
  return TGX_OK;
}

// the non-NULL-timestamp rows of a batch behind the rows the task holds
tgx_status append_rows(tgx_state *st, const TimeGapTask &task, TimeGapTaskState &ts, const tgx_column &t,
                       const tgx_column *g, tgx_error *err) {
  if (!ts.count.p) {
    HIP_TRY(ts.count.reserve(16));
    HIP_TRY(hipMemsetAsync(ts.count.p, 0, 16, st->stream));
  }
  const uint64_t length = (uint64_t)t.length;
  uint64_t need = ts.rows_upper + length;
  unsigned long long held[2] = {0, 0};
  bool counted = false;
  if (need > 0xFFFFFFFFull) {  // (the bound counts NULL rows too: the exact number decides)
    TGX_TRY(read_counts(st, ts, held, err));
    counted = true;
    ts.rows_upper = held[0] + held[1];
    need = ts.rows_upper + length;
    if (need > 0xFFFFFFFFull)
      return fail(err, TGX_UNSUPPORTED, "TIME_GAP over more than 2^32 - 1 retained rows is not supported (columns %d, %d)",
                  task.col_t, task.col_g);
  }
  if (need > ts.capacity) {
    const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(need, ts.capacity * 2), 0xFFFFFFFFull);
    DevBuf nt, ng;
    HIP_TRY(nt.reserve(cap * 8));
    if (g) HIP_TRY(ng.reserve(cap * 8));
    if (ts.capacity && ts.rows_upper) {
      if (!counted) TGX_TRY(read_counts(st, ts, held, err));
      const uint64_t nf = held[0], nb = held[1];
      if (nf + nb > ts.capacity) return fail(err, TGX_INTERNAL, "TIME_GAP: more rows retained than the arrays hold");
      if (nf) HIP_TRY(hipMemcpyAsync(nt.p, ts.kt.p, nf * 8, hipMemcpyDeviceToDevice, st->stream));
      if (nf && g) HIP_TRY(hipMemcpyAsync(ng.p, ts.kg.p, nf * 8, hipMemcpyDeviceToDevice, st->stream));
      if (nb)
        HIP_TRY(hipMemcpyAsync(nt.as<uint64_t>() + (cap - nb), ts.kt.as<uint64_t>() + (ts.capacity - nb), nb * 8,
                               hipMemcpyDeviceToDevice, st->stream));
      HIP_TRY(hipStreamSynchronize(st->stream));
    }
    ts.kt = std::move(nt);
    ts.kg = std::move(ng);
    ts.capacity = cap;
  }
  TimeGapBatch d;
  d.t = t.values;
  d.tv = t.validity;
  d.toff = t.offset;
  d.g = g ? g->values : nullptr;
  d.gv = g ? g->validity : nullptr;
  d.goff = g ? g->offset : 0;
  d.length = t.length;
  launch_timegap_compact(d, ts.kt.as<uint64_t>(), g ? ts.kg.as<uint64_t>() : nullptr, ts.capacity,
                         ts.count.as<unsigned long long>(), st->stream);
  HIP_TRY(hipGetLastError());
  ts.rows_upper = need;
  return TGX_OK;
}

// One sort / ranking job with the work buffers as its ping-pong space.  Bucket sizes come from a sample of the keys
// when the job is large enough and the device has the room (kernels/sortrank.h); a job that reports a full bucket in its
// status word is run again with counted buckets.
tgx_status run_job(tgx_state *st, TimeGapState *ws, SrJob j, tgx_error *err) {
  const uint64_t n = j.n;
  const bool with_pay = j.pay_bytes != 0;
  const size_t temp_bytes = sr_workspace_bytes(n);
  HIP_TRY(ws->temp.reserve(temp_bytes));
  uint32_t *d_status = (uint32_t *)((char *)ws->small.p + kStatusOffset);
  const uint64_t roomy = sr_roomy_elems(n);
  bool optimistic = n >= sr_tuning().optimistic_min && sr_optimistic_applies(n);
  if (optimistic) {
    size_t free_b = 0, total_b = 0;
    const int arrays = with_pay ? 4 : 2;
    size_t have = 0;
    for (int i = 0; i < arrays; i++) have += ws->w[i].cap;
    const size_t want = (size_t)roomy * 8 * arrays;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || (want > have && free_b < want - have + (2ull << 30)))
      optimistic = false;
  }
  for (int attempt = 0; attempt < 2; attempt++) {
    const uint64_t elems = optimistic ? roomy : n;
    HIP_TRY(ws->w[0].reserve(elems * 8));
    HIP_TRY(ws->w[1].reserve(elems * 8));
    j.k[0] = ws->w[0].as<uint64_t>();
    j.k[1] = ws->w[1].as<uint64_t>();
    if (with_pay) {
      HIP_TRY(ws->w[2].reserve(elems * 8));
      HIP_TRY(ws->w[3].reserve(elems * 8));
      j.p[0] = ws->w[2].p;
      j.p[1] = ws->w[3].p;
    }
    j.optimistic = optimistic;
    j.cap[0] = j.cap[1] = elems;
    j.status = d_status;
    HIP_TRY(sr_run(j, ws->temp.p, temp_bytes, st->stream, nullptr));
    uint32_t status = 0;
    HIP_TRY(hipMemcpyAsync(&status, d_status, sizeof(status), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    if (status == 0) return TGX_OK;
    if (!optimistic) return fail(err, TGX_INTERNAL, "TIME_GAP: the sort failed with counted buckets (status %u)", status);
    optimistic = false;  // a bucket outgrew the room its share of the sample gave it: once more, counting
    if (getenv("TGX_SORT_DEBUG"))
      fprintf(stderr, "tgx time gap: a bucket was full (status %u): again with counted buckets\n", status);
  }
  return TGX_OK;
}

// n keys -> out, in order
tgx_status sort_keys(tgx_state *st, TimeGapState *ws, const uint64_t *keys, uint64_t n, DevBuf &out, tgx_error *err) {
  HIP_TRY(out.reserve(n * 8));
  SrJob j;
  j.keys = keys;
  j.n = n;
  j.pay_bytes = 0;
  j.sink = kSrSorted;
  j.out_keys = out.as<uint64_t>();
  return run_job(st, ws, j, err);
}

// the grouped route: afterwards ws->t3 holds the timestamps and ws->g1 the composed keys, partition by partition
tgx_status sort_grouped(tgx_state *st, TimeGapState *ws, const uint64_t *kt, const uint64_t *kg, uint64_t n,
                        tgx_error *err) {
  HIP_TRY(ws->t1.reserve(n * 8));
  HIP_TRY(ws->g1.reserve(n * 8));
  HIP_TRY(ws->ranks.reserve(n * 8));
  HIP_TRY(ws->t3.reserve(n * 8));
  SrJob a;  // (1) by timestamp, the group key travels along
  a.keys = kt;
  a.pay = kg;
  a.n = n;
  a.pay_bytes = 8;
  a.sink = kSrSorted;
  a.out_keys = ws->t1.as<uint64_t>();
  a.out_pay = ws->g1.p;
  TGX_TRY(run_job(st, ws, a, err));
  SrJob b;  // (2) ranks[i] = RANK() of the group key at position i (the payload is the key's index)
  b.keys = ws->g1.as<uint64_t>();
  b.n = n;
  b.pay_bytes = 4;
  b.sink = kSrRankScatter;
  b.rank_out = ws->ranks.as<uint64_t>();
  TGX_TRY(run_job(st, ws, b, err));
  launch_timegap_compose(ws->ranks.as<uint64_t>(), n, st->stream);  // (3)
  HIP_TRY(hipGetLastError());
  SrJob c;  // (4) by (group rank, position), the timestamp travels along; the group keys' array is free again
  c.keys = ws->ranks.as<uint64_t>();
  c.pay = ws->t1.p;
  c.n = n;
  c.pay_bytes = 8;
  c.sink = kSrSorted;
  c.out_keys = ws->g1.as<uint64_t>();
  c.out_pay = ws->t3.p;
  return run_job(st, ws, c, err);
}

// sorts the task's rows and takes the counters of all its specs
tgx_status answer(tgx_state *st, const TimeGapTask &task, TimeGapTaskState &ts, tgx_error *err) {
  TimeGapState *ws = tstate(st);
  ts.violations.assign(task.specs.size(), 0);
  ts.rows = ts.gaps = ts.largest = 0;
  unsigned long long held[2];
  TGX_TRY(read_counts(st, ts, held, err));
  const uint64_t nf = held[0], nb = held[1];
  ts.rows = nf + nb;
  if (nf + nb > ts.capacity) return fail(err, TGX_INTERNAL, "TIME_GAP: more rows retained than the arrays hold");
  if (std::max(nf, nb) > 0xFFFFFFF0ull)
    return fail(err, TGX_UNSUPPORTED, "TIME_GAP over more than 2^32 - 16 rows in one list is not supported");
  if (ts.rows >= 2) {
    HIP_TRY(ws->small.reserve(256));
    const bool grouped = task.col_g >= 0;
    const uint64_t *front_vals = nullptr, *front_tags = nullptr, *back_vals = nullptr;
    // (profile: the sorts and the neighbour passes apart -- an ungrouped task's "time_gap_sort" is one bare keys-only
    // sort of its rows, the yardstick of tools/bench_time_gap.py)
    std::unique_ptr<ProfScope> sorting(new ProfScope(st, "time_gap_sort", ts.rows * (grouped ? 16 : 8)));
    if (nf >= 2) {
      if (grouped) {
        TGX_TRY(sort_grouped(st, ws, ts.kt.as<uint64_t>(), ts.kg.as<uint64_t>(), nf, err));
        front_vals = ws->t3.as<uint64_t>();
        front_tags = ws->g1.as<uint64_t>();
      } else {
        TGX_TRY(sort_keys(st, ws, ts.kt.as<uint64_t>(), nf, ws->t3, err));
        front_vals = ws->t3.as<uint64_t>();
      }
    }
    if (nb >= 2) {
      TGX_TRY(sort_keys(st, ws, ts.kt.as<uint64_t>() + (ts.capacity - nb), nb, ws->back_sorted, err));
      back_vals = ws->back_sorted.as<uint64_t>();
    }
    sorting.reset();
    ProfScope ps(st, "time_gap_neighbours", (front_tags ? nf * 16 : nf * 8) + nb * 8);
    unsigned long long *d_out = ws->small.as<unsigned long long>();
    for (size_t first = 0; first < task.specs.size(); first += kTimeGapThresholds) {
      TimeGapThresholds T;
      memset(&T, 0, sizeof(T));
      T.n = (int32_t)std::min<size_t>(kTimeGapThresholds, task.specs.size() - first);
      for (int k = 0; k < T.n; k++) T.max_gap[k] = task.specs[first + k].max_gap;
      HIP_TRY(hipMemsetAsync(d_out, 0, kCounterWords * 8, st->stream));
      if (front_vals) launch_timegap_neighbours(front_vals, front_tags, nf, T, d_out, st->stream);
      if (back_vals) launch_timegap_neighbours(back_vals, nullptr, nb, T, d_out, st->stream);
      HIP_TRY(hipGetLastError());
      unsigned long long h[kCounterWords];
      HIP_TRY(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, st->stream));
      HIP_TRY(hipStreamSynchronize(st->stream));
      ts.gaps = h[0];
      ts.largest = h[1];
      for (int k = 0; k < T.n; k++) ts.violations[first + k] = h[2 + k];
    }
  }
  ts.cached = true;
  return TGX_OK;
}

tgx_status counts_of(tgx_state *st, int spec_index, tgx_time_gap_counts *out, tgx_error *err) {
  const int slot = st->plan->bind[spec_index].slot;
  const TimeGapTask &task = tplan(st->plan)->tasks[slot];
  TimeGapTaskState &ts = tstate(st)->tasks[slot];
  if (!ts.cached) TGX_TRY(answer(st, task, ts, err));
  size_t k = 0;
  while (k < task.specs.size() && task.specs[k].spec_index != spec_index) k++;
  if (k == task.specs.size()) return fail(err, TGX_INTERNAL, "TIME_GAP: spec %d has no threshold slot", spec_index);
  out->seen = ts.total_rows;
  out->rows = ts.rows;
  out->gaps = ts.gaps;
  out->violations = ts.violations[k];
  out->largest_gap = ts.largest;
  return TGX_OK;
}
}  // namespace

tgx_status timegap_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  if (!plan->timegap) plan->timegap = new TimeGapPlan();
  TimeGapPlan *tp = (TimeGapPlan *)plan->timegap;
  const tgx_check_spec &s = plan->specs[spec_index];
  if (s.column2 < -1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: TIME_GAP: column2 is the group column or -1 (%d)", spec_index, s.column2);
  size_t i = 0;
  while (i < tp->tasks.size() && !(tp->tasks[i].col_t == s.column && tp->tasks[i].col_g == s.column2)) i++;
  if (i == tp->tasks.size()) tp->tasks.push_back({s.column, s.column2, {}});
  tp->tasks[i].specs.push_back({spec_index, false, 0});
  *slot = (int)i;
  return TGX_OK;
}

void timegap_plan_free(tgx_plan *plan) {
  delete (TimeGapPlan *)plan->timegap;
  plan->timegap = nullptr;
}

size_t timegap_num_tasks(const tgx_plan *plan) { return plan->timegap ? tplan(plan)->tasks.size() : 0; }

tgx_status timegap_plan_ready(const tgx_plan *plan, tgx_error *err) {
  if (!plan->timegap) return TGX_OK;
  for (auto &t : tplan(plan)->tasks)
    for (auto &s : t.specs)
      if (!s.set)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a TIME_GAP check needs its threshold (tgx_plan_set_time_gap)",
                    s.spec_index);
  return TGX_OK;
}

void timegap_mark_used(tgx_plan *plan) {
  plan->timegap_on.assign(plan->n_columns_needed, 0);
  if (!plan->timegap) return;
  for (auto &t : tplan(plan)->tasks) {
    plan->used[t.col_t] = plan->reads_values[t.col_t] = 1;
    plan->timegap_on[t.col_t] |= 1;
    if (t.col_g >= 0) {
      plan->used[t.col_g] = plan->reads_values[t.col_g] = plan->needs_wide[t.col_g] = 1;
      plan->timegap_on[t.col_g] |= 2;
    }
  }
}

tgx_status timegap_check_type(const tgx_plan *plan, int column, int type, tgx_error *err) {
  const char on = plan->timegap_on[column];
  if ((on & 1) && type != TGX_INT64)
    return fail(err, TGX_UNSUPPORTED, "column %d: TIME_GAP takes Int64-shaped timestamp columns (type %d)", column, type);
  const bool group_ok = type == TGX_INT64 || type == TGX_INT32 || (type >= TGX_INT8 && type <= TGX_UINT32);
  if ((on & 2) && !group_ok)
    return fail(err, TGX_UNSUPPORTED, "column %d: TIME_GAP takes group columns that are Int64-shaped or widen to Int64 (type %d)",
                column, type);
  return TGX_OK;
}

void timegap_state_init(tgx_state *st) {
  if (st->timegap || !st->plan->timegap) return;
  TimeGapState *s = new TimeGapState();
  s->tasks.resize(timegap_num_tasks(st->plan));
  st->timegap = s;
}

void timegap_state_free(tgx_state *st) {
  delete tstate(st);
  st->timegap = nullptr;
}

void timegap_state_reset(tgx_state *st) {
  TimeGapState *s = tstate(st);
  if (!s) return;
  for (auto &t : s->tasks) {
    t.rows_upper = 0;
    t.total_rows = 0;
    t.cached = false;
    if (t.count.p) (void)hipMemsetAsync(t.count.p, 0, 16, st->stream);
  }
}

tgx_status timegap_update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) {
  if (!st->plan->timegap || nrows <= 0) return TGX_OK;
  const TimeGapPlan *tp = tplan(st->plan);
  TimeGapState *ws = tstate(st);
  for (size_t i = 0; i < tp->tasks.size(); i++) {
    const TimeGapTask &task = tp->tasks[i];
    const tgx_column &t = dev[task.col_t];
    const tgx_column *g = task.col_g >= 0 ? &dev[task.col_g] : nullptr;
    // (Int64 views: update_validate refuses every other type, and the staging widens the narrow group columns)
    if (t.type != TGX_INT64 || (g && g->type != TGX_INT64))
      return fail(err, TGX_INTERNAL, "TIME_GAP: columns %d, %d did not arrive as Int64 views", task.col_t, task.col_g);
    TimeGapTaskState &ts = ws->tasks[i];
    ts.total_rows += (uint64_t)nrows;
    ts.cached = false;
    ProfScope ps(st, "time_gap_append", (uint64_t)nrows * (g ? 16 : 8));
    TGX_TRY(append_rows(st, task, ts, t, g, err));
  }
  return TGX_OK;
}

tgx_status timegap_fill_result(tgx_state *st, int spec_index, tgx_result *r, tgx_error *err) {
  tgx_time_gap_counts c;
  TGX_TRY(counts_of(st, spec_index, &c, err));
  r->total = (int64_t)c.seen;
  r->non_null = (int64_t)c.gaps;
  r->matches = (int64_t)(c.gaps - c.violations);
  return TGX_OK;
}

tgx_status timegap_check_mergeable(tgx_state *st, const char *what, tgx_error *err) {
  if (!st->timegap) return TGX_OK;
  TGX_TRY(coalesce_flush(st, err));  // (batches tgx_update has only noted so far are rows the state holds)
  for (auto &t : tstate(st)->tasks)
    if (t.total_rows > 0)
      return fail(err, TGX_UNSUPPORTED,
                  "%s: TIME_GAP states hold the rows of one data set and cannot be merged, serialized or reduced "
                  "across ranks (a cross-rank LAG() is a distributed sort)", what);
  return TGX_OK;
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_time_gap(tgx_plan *plan, size_t spec_index, const tgx_time_gap_params *p,
                                            tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_TIME_GAP, "TIME_GAP", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the threshold of a TIME_GAP check is fixed once a state of the plan exists");
  if (p->flags != 0) return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: unknown TIME_GAP flags 0x%x", spec_index, p->flags);
  for (auto &s : ((TimeGapPlan *)plan->timegap)->tasks[slot].specs)
    if (s.spec_index == (int)spec_index) {
      s.max_gap = p->max_gap;
      s.set = true;
    }
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_time_gap_get(const tgx_plan *plan, tgx_state *st, size_t spec_index, tgx_time_gap_counts *out,
                                       tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_TIME_GAP, "TIME_GAP", &slot, err, "bad arguments"));
  TGX_TRY(coalesce_flush(st, err));  // batches tgx_update has only noted so far
  return counts_of(st, (int)spec_index, out, err);
} catch (...) {
  return tgx::abi_exception(err);
}
