// temporal_device.cpp -- TGX_CHECK_TEMPORAL: the row predicates behind the reference's TemporalOrderingConstraint
// (TG/constraints/temporal_ordering.rs:346-453; include/tgx.h has the modes and the NULL rules).
//
// A task is one spec.  Its running state on the device is two 64-bit counters folded by kernels/temporal.hip -- the rows
// that are non-NULL and pass the weekday filter, and those of them that pass the predicate; rows seen are counted on the
// host.  What is merged in from other states or read from a blob is kept on the host and added when the state is read.
// {seen, considered, violations} follow from the three numbers and the task's flags (counts_of).
#include "api_internal.h"

namespace tgx {
void launch_temporal(const TemporalLaunch &L, int n_tasks, int blocks_per_task, hipStream_t stream);

namespace {

// one task's state as the host sees it
struct TemporalHost {
  uint64_t seen = 0, live = 0, passed = 0;  // live: non-NULL and through the weekday filter
};

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

struct NoRange {};

struct TemporalKind {
  typedef TemporalTask Task;
  typedef TemporalHost Host;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_TEMPORAL;
  static constexpr const char *kDiffers = nullptr;  // (every host has the one shape)
  static constexpr uint32_t kMagic = 0x52504d54;  // "TMPR"

  static const std::vector<TemporalTask> &tasks(const tgx_plan *plan) { return plan->temporal; }
  static size_t words(const TemporalTask &) { return 2; }  // live, passed
  static NoRange range_identity() { return NoRange(); }
  static TemporalHost fresh(const TemporalTask &) { return TemporalHost(); }
  static size_t shape(const TemporalHost &) { return 0; }
  static TemporalHost from_device(const TemporalTask &, int64_t rows, const NoRange &, const unsigned long long *w) {
    TemporalHost d;
    d.seen = (uint64_t)rows;
    d.live = w[0];
    d.passed = w[1];
    return d;
  }
  static void merge_host(TemporalHost &a, const TemporalHost &b) {
    a.seen += b.seen;
    a.live += b.live;
    a.passed += b.passed;
  }

  // per task { i32 mode, u32 flags, i64 delta, ticks_per_second, lo, hi (the plan's parameters), u64 seen, live, passed }
  static void write(const TemporalTask &t, const TemporalHost &h, Writer &w) {
    const uint32_t head[2] = {(uint32_t)t.params.mode, t.flags};
    w.pod(head);
    const int64_t params[4] = {t.params.delta, t.params.ticks_per_second, t.params.lo, t.params.hi};
    w.pod(params);
    const uint64_t counts[3] = {h.seen, h.live, h.passed};
    w.pod(counts);
  }

  static tgx_status read(const TemporalTask &t, TemporalHost &h, Reader &r, size_t k, tgx_error *err) {
    uint32_t head[2];
    int64_t params[4];
    uint64_t counts[3];
    r.get(head, sizeof(head));
    r.get(params, sizeof(params));
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    const int64_t mine[4] = {t.params.delta, t.params.ticks_per_second, t.params.lo, t.params.hi};
    if (head[0] != (uint32_t)t.params.mode || head[1] != t.flags || memcmp(params, mine, sizeof(mine)) != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "TEMPORAL task %zu: the blob was counted under other parameters (mode %u) than the plan's (mode %d)", k,
                  head[0], t.params.mode);
    if (counts[1] > counts[0] || counts[2] > counts[1])
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (TEMPORAL task %zu)", k);
    h.seen = counts[0];
    h.live = counts[1];
    h.passed = counts[2];
    return TGX_OK;
  }
};

struct TemporalCheck final : SideState<TemporalKind> {
  using SideState::SideState;

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    auto launch = [&](const int *slots, int n) -> tgx_status {
      TemporalLaunch L;
      memset(&L, 0, sizeof(L));
      uint64_t bytes = 0;
      for (int k = 0; k < n; k++) {
        const TemporalTask &t = plan->temporal[slots[k]];
        const bool pair = t.params.mode == kTemporalOrder;
        // (Int64 views: update_validate refuses every other type of a column a TEMPORAL check reads)
        const tgx_column &x = dev[t.column], &y = dev[pair ? t.column2 : t.column];
        bytes += side_fill_x(L.cols[k], x);
        const uint64_t y_bytes = side_fill_y(L.cols[k], y);
        if (pair) bytes += y_bytes;
        L.params[k] = t.params;
        L.counters[k] = d_counts.as<unsigned long long>() + word_off[slots[k]];
      }
      // 8 waves a workgroup, up to 4 workgroups a CU
      const int blocks = side_blocks(nrows, kTemporalBlock, g_ctx.n_cu, 4, n);
      TGX_TRY(side_rows_fit("TEMPORAL", nrows, blocks, err));
      ProfScope ps(st, "temporal", bytes);
      launch_temporal(L, n, blocks, st->stream);
      HIP_TRY(hipGetLastError());
      for (int k = 0; k < n; k++) device_rows[slots[k]] += nrows;  // (only rows the device was given)
      return TGX_OK;
    };
    return side_launches(plan->temporal, [](const TemporalTask &) { return true; }, launch);
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    std::vector<TemporalHost> g;
    TGX_TRY(gather(st, &g, err));
    const tgx_temporal_counts c = counts_of(st->plan->temporal[slot], g[slot]);
    r->total = (int64_t)c.seen;
    r->non_null = (int64_t)c.considered;
    r->matches = (int64_t)(c.considered - c.violations);
    return TGX_OK;
  }
};

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

void temporal_mark_columns(tgx_plan *plan) {
  for (const TemporalTask &t : plan->temporal)
    for (int c : {t.column, t.column2})
      if (c >= 0) side_mark(plan, TemporalCheck::kIndex, c, false);  // (Int64-shaped columns only: nothing to widen)
}

tgx_status temporal_check_column(const tgx_plan *, int column, const tgx_column &c, tgx_error *err) {
  if (c.type != TGX_INT64)
    return fail(err, TGX_UNSUPPORTED, "column %d: TEMPORAL takes Int64-shaped columns (type %d)", column, c.type);
  return TGX_OK;
}

SideCheck *temporal_state_new(const tgx_plan *plan) {
  return plan->temporal.empty() ? nullptr : new TemporalCheck(plan);
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
  TGX_TRY(TemporalCheck::of(st)->gather(st, &g, err));
  *out = counts_of(plan->temporal[slot], g[slot]);
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
