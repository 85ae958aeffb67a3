// side_check.h -- the check kinds that run beside the fused pass and share one shape.  A kind is registered once, by its
// record in kSideKinds below; its code is in a *_device.cpp of its own.
//
// A task is one spec.  Its running state is a few 64-bit counters on the device, plus a small range accumulator for the
// kinds that have a range phase; rows seen are counted on the host.  What is merged in from other states or read from a
// blob is kept on the host (`host`) and added when the state is read (`gather`).  The rest of the library sees a
// SideCheck per kind in tgx_state::side, in the order of kSideKinds, which is the order of the blob's sections (null: the
// plan has no task of the kind); SideState<K> is everything the kinds have in common, a kind K adds what its tasks count
// and how they are launched.  A kind whose tasks keep more on the device than counters clears and reads that through
// device_clear_extra / gather_extra (counted_state.h: a table of counted keys per task); the other kinds leave both
// alone.
#pragma once
#include <memory>

#include "internal.h"
#include "wire_io.h"

namespace tgx {

struct TGX_HIDDEN SideCheck {
  virtual ~SideCheck() {}
  // (the caller has waited for the stream)
  virtual tgx_status reset(tgx_state *st, tgx_error *err) = 0;
  // may the state take a batch of `nrows` rows at all?  Asked by tgx_update before the batch is noted or run (a kind
  // whose tasks need more than the plan gives them: KEY_PROBE's parent set)
  virtual tgx_status accepts(tgx_state *, int64_t, tgx_error *) { return TGX_OK; }
  // one batch (device views of the plan's columns) through the tasks' kernels
  virtual tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) = 0;
  virtual tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) = 0;
  virtual tgx_status merge_from(tgx_state *st, tgx_state *src, tgx_error *err) = 0;
  // the blob's section: present only when the plan has such tasks (blobs of other plans keep their bytes)
  virtual tgx_status serialize(tgx_state *st, Writer &w, tgx_error *err) = 0;
  virtual tgx_status deserialize(tgx_state *st, Reader &r, tgx_error *err) = 0;
};

// ---- the kinds ---------------------------------------------------------------------------------------------------------
struct TGX_HIDDEN SideKind {
  int kind;  // TGX_CHECK_*
  const char *name;
  // spec `spec_index` as a task of the plan; *slot: the task's index within its kind
  tgx_status (*plan_add)(tgx_plan *plan, int spec_index, int *slot, tgx_error *err);
  // every task has the parameters of its tgx_plan_set_* call?  Null: the kind's tasks run without any
  tgx_status (*plan_ready)(const tgx_plan *plan, tgx_error *err);
  void (*mark_columns)(tgx_plan *plan);  // the per-column flags of the columns its tasks read (side_mark)
  // may column `column` of a batch feed the kind's tasks?  Asked by tgx_update of the columns they read only
  tgx_status (*check_column)(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err);
  SideCheck *(*state_new)(const tgx_plan *plan);  // the fresh state of the plan's tasks, or null when it has none
  bool reads_column2;                             // a spec's column2 is a column of the batch
};

// what every kind's *_device.cpp defines (a plan_ready where the kind has parameters)
#define TGX_SIDE_KIND(prefix)                                                                               \
  tgx_status prefix##_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err);                  \
  void prefix##_mark_columns(tgx_plan *plan);                                                               \
  tgx_status prefix##_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err);  \
  TGX_HIDDEN SideCheck *prefix##_state_new(const tgx_plan *plan);
TGX_SIDE_KIND(joint)
TGX_SIDE_KIND(temporal)
TGX_SIDE_KIND(hist)
TGX_SIDE_KIND(valuerule)
TGX_SIDE_KIND(valuecounts)
TGX_SIDE_KIND(paircounts)
TGX_SIDE_KIND(groupcounts)
TGX_SIDE_KIND(groupsums)
TGX_SIDE_KIND(keyprobe)
TGX_SIDE_KIND(rowpredicate)
TGX_SIDE_KIND(typeclasses)
#undef TGX_SIDE_KIND
tgx_status temporal_plan_ready(const tgx_plan *plan, tgx_error *err);
tgx_status valuerule_plan_ready(const tgx_plan *plan, tgx_error *err);
tgx_status valuecounts_plan_ready(const tgx_plan *plan, tgx_error *err);
tgx_status paircounts_plan_ready(const tgx_plan *plan, tgx_error *err);
tgx_status groupcounts_plan_ready(const tgx_plan *plan, tgx_error *err);
tgx_status groupsums_plan_ready(const tgx_plan *plan, tgx_error *err);
tgx_status keyprobe_plan_ready(const tgx_plan *plan, tgx_error *err);
tgx_status rowpredicate_plan_ready(const tgx_plan *plan, tgx_error *err);
// does a blob of `st` hold a KEY_PROBE task on string keys with a known, non-empty set?  Its identity is made of
// fingerprints: such a blob carries the plan's fingerprint key (wire.cpp)
TGX_HIDDEN bool keyprobe_blob_keyed(tgx_state *st);

// in the order of the blob's sections
inline constexpr SideKind kSideKinds[kNumSide] = {
    {TGX_CHECK_JOINT_BINS, "JOINT_BINS", joint_plan_add, nullptr, joint_mark_columns, joint_check_column,
     joint_state_new, true},
    {TGX_CHECK_TEMPORAL, "TEMPORAL", temporal_plan_add, temporal_plan_ready, temporal_mark_columns,
     temporal_check_column, temporal_state_new, true},
    {TGX_CHECK_HISTOGRAM, "HISTOGRAM", hist_plan_add, nullptr, hist_mark_columns, hist_check_column, hist_state_new,
     false},
    {TGX_CHECK_VALUE_RULE, "VALUE_RULE", valuerule_plan_add, valuerule_plan_ready, valuerule_mark_columns,
     valuerule_check_column, valuerule_state_new, false},
    {TGX_CHECK_VALUE_COUNTS, "VALUE_COUNTS", valuecounts_plan_add, valuecounts_plan_ready, valuecounts_mark_columns,
     valuecounts_check_column, valuecounts_state_new, false},
    {TGX_CHECK_PAIR_COUNTS, "PAIR_COUNTS", paircounts_plan_add, paircounts_plan_ready, paircounts_mark_columns,
     paircounts_check_column, paircounts_state_new, true},
    {TGX_CHECK_GROUP_COUNTS, "GROUP_COUNTS", groupcounts_plan_add, groupcounts_plan_ready, groupcounts_mark_columns,
     groupcounts_check_column, groupcounts_state_new, true},
    {TGX_CHECK_GROUP_SUMS, "GROUP_SUMS", groupsums_plan_add, groupsums_plan_ready, groupsums_mark_columns,
     groupsums_check_column, groupsums_state_new, true},
    {TGX_CHECK_KEY_PROBE, "KEY_PROBE", keyprobe_plan_add, keyprobe_plan_ready, keyprobe_mark_columns,
     keyprobe_check_column, keyprobe_state_new, false},
    {TGX_CHECK_ROW_PREDICATE, "ROW_PREDICATE", rowpredicate_plan_add, rowpredicate_plan_ready,
     rowpredicate_mark_columns, rowpredicate_check_column, rowpredicate_state_new, false},
    {TGX_CHECK_TYPE_CLASSES, "TYPE_CLASSES", typeclasses_plan_add, nullptr, typeclasses_mark_columns,
     typeclasses_check_column, typeclasses_state_new, false},
};

// where `kind` stands in kSideKinds (and in tgx_state::side, tgx_plan::side_on), or -1: not a kind of this file
constexpr int side_index(int kind) {
  for (int i = 0; i < kNumSide; i++)
    if (kSideKinds[i].kind == kind) return i;
  return -1;
}

// column `c` feeds a task of kind `index`, which reads its values; `wide`: as 8-byte values (a 4-byte column is widened)
TGX_HIDDEN inline void side_mark(tgx_plan *plan, int index, int c, bool wide) {
  plan->used[c] = plan->reads_values[c] = plan->side_on[index][c] = 1;
  if (wide) plan->needs_wide[c] = 1;
}

// every task of every kind has its parameters?  Asked before a state of the plan is made
TGX_HIDDEN inline tgx_status side_plans_ready(const tgx_plan *plan, tgx_error *err) {
  for (const SideKind &k : kSideKinds)
    if (k.plan_ready) TGX_TRY(k.plan_ready(plan, err));
  return TGX_OK;
}

// ---- what the kinds' updates share -----------------------------------------------------------------------------------
constexpr int kSidePerLaunch = 8;  // tasks of one launch (grid.y)
static_assert(kMaxJointPerLaunch == kSidePerLaunch && kMaxTemporalPerLaunch == kSidePerLaunch &&
                  kMaxHistPerLaunch == kSidePerLaunch && kMaxValueRuleGroupsPerLaunch == kSidePerLaunch &&
                  kMaxKeyProbePerLaunch == kSidePerLaunch,
              "the kinds' launch descriptors hold kSidePerLaunch tasks");

// the tasks that are `in_phase`, in launches of up to kSidePerLaunch: launch(slots, n)
template <class Task, class InPhase, class Launch>
TGX_HIDDEN inline tgx_status side_launches(const std::vector<Task> &tasks, InPhase in_phase, Launch launch) {
  std::vector<int> slots;
  for (size_t k = 0; k < tasks.size(); k++)
    if (in_phase(tasks[k])) slots.push_back((int)k);
  for (size_t t0 = 0; t0 < slots.size(); t0 += kSidePerLaunch)
    TGX_TRY(launch(slots.data() + t0, (int)std::min<size_t>(kSidePerLaunch, slots.size() - t0)));
  return TGX_OK;
}

// workgroups per task: 16 rows a lane before another workgroup is worth its launch; `per_cu` workgroups a CU, shared by
// the `n_tasks` tasks of the launch
TGX_HIDDEN inline int side_blocks(int64_t nrows, int block, int n_cu, int per_cu, int n_tasks) {
  return (int)std::min<int64_t>(std::max<int64_t>(1, (nrows + block * 16 - 1) / (block * 16)),
                                std::max(32, (n_cu * per_cu) / n_tasks));
}

// (a lane's, a wave's and a workgroup's counters are 32-bit)
TGX_HIDDEN inline tgx_status side_rows_fit(const char *kind, int64_t nrows, int blocks, tgx_error *err) {
  if (nrows / blocks >= ((int64_t)1 << 32))
    return fail(err, TGX_UNSUPPORTED, "%s: a batch of %lld rows is too long", kind, (long long)nrows);
  return TGX_OK;
}

// a column as the x / y side of a launch's descriptor; what reading it moves (the profile's bytes figure)
TGX_HIDDEN inline uint64_t side_fill_x(ComomentColDesc &d, const tgx_column &x) {
  d.x = x.values;
  d.xv = x.validity;
  d.xoff = x.offset;
  d.length = x.length;
  d.x_is_float = x.type == TGX_FLOAT64;
  return (uint64_t)x.length * 8 + (x.validity ? (uint64_t)(x.length + 7) / 8 : 0);
}
TGX_HIDDEN inline uint64_t side_fill_y(ComomentColDesc &d, const tgx_column &y) {
  d.y = y.values;
  d.yv = y.validity;
  d.yoff = y.offset;
  d.y_is_float = y.type == TGX_FLOAT64;
  return (uint64_t)y.length * 8 + (y.validity ? (uint64_t)(y.length + 7) / 8 : 0);
}

// ---- the state of one kind's tasks -----------------------------------------------------------------------------------
// K gives: Task, Host (one task's state as the host sees it), Range (the device's range accumulator; kRanged: whether
// there is one), kKind, kMagic, kDiffers (what two states of one plan can still differ in, or null), and
//   tasks(plan)                         the plan's tasks of the kind
//   words(task)                         64-bit device counters of the task
//   range_identity()
//   fresh(task)                         the identity of `Host`
//   shape(host)                         what must agree before two hosts are merged
//   from_device(task, rows, range, w)   the device part as a Host
//   merge_host(a, b)
//   write(task, host, w)                the task's part of the blob's section
//   read(task, host, r, k, err)         ... read back into a fresh `host`; returns TGX_OK when the blob has run out
template <class K>
struct TGX_HIDDEN SideState : SideCheck {
  typedef typename K::Host Host;
  typedef typename K::Range Range;
  static constexpr int kIndex = side_index(K::kKind);
  static_assert(kIndex >= 0, "the kind has a record in kSideKinds");
  static constexpr const char *kName = kSideKinds[kIndex].name;

  std::vector<Host> host;            // merged in / deserialized
  std::vector<int64_t> device_rows;  // rows the device part has seen
  std::vector<size_t> word_off;      // per task: first of its counters in d_counts
  size_t n_words = 0;
  bool device_ready = false;
  DevBuf d_range, d_counts, d_partials;
  std::vector<Range> identity;  // (kept alive: uploaded asynchronously)

  explicit SideState(const tgx_plan *plan) {
    const auto &tasks = K::tasks(plan);
    device_rows.assign(tasks.size(), 0);
    for (const auto &t : tasks) {
      host.push_back(K::fresh(t));
      word_off.push_back(n_words);
      n_words += K::words(t);
    }
  }

  static SideState *of(tgx_state *st) { return static_cast<SideState *>(st->side[kIndex].get()); }

  // what a kind uploads once per state
  virtual tgx_status device_init_extra(tgx_state *, tgx_error *) { return TGX_OK; }
  // device memory of the kind's own: back to empty (queued on the stream) / folded into the gathered hosts (the stream
  // has been waited for, the counters are already in `out`)
  virtual tgx_status device_clear_extra(tgx_state *, tgx_error *) { return TGX_OK; }
  virtual tgx_status gather_extra(tgx_state *, std::vector<Host> *, tgx_error *) { return TGX_OK; }

  tgx_status device_clear(tgx_state *st, tgx_error *err) {
    if (!identity.empty())
      HIP_TRY(hipMemcpyAsync(d_range.p, identity.data(), identity.size() * sizeof(Range), hipMemcpyHostToDevice,
                             st->stream));
    if (n_words) HIP_TRY(hipMemsetAsync(d_counts.p, 0, n_words * sizeof(unsigned long long), st->stream));
    return device_clear_extra(st, err);
  }

  tgx_status device_init(tgx_state *st, tgx_error *err) {
    if (device_ready) return TGX_OK;
    if (K::kRanged) {
      identity.assign(host.size(), K::range_identity());
      HIP_TRY(d_range.reserve(identity.size() * sizeof(Range)));
    }
    if (n_words) HIP_TRY(d_counts.reserve(n_words * sizeof(unsigned long long)));
    TGX_TRY(device_init_extra(st, err));
    TGX_TRY(device_clear(st, err));
    device_ready = true;
    return TGX_OK;
  }

  // host part + device part of every task (the device part stays where it is)
  tgx_status gather(tgx_state *st, std::vector<Host> *out, tgx_error *err) {
    const auto &tasks = K::tasks(st->plan);
    TGX_TRY(coalesce_flush(st, err));  // batches tgx_update has only noted so far
    *out = host;
    if (!device_ready) return TGX_OK;
    std::vector<Range> ranges(identity.size());
    std::vector<unsigned long long> words(n_words);
    if (!ranges.empty())
      HIP_TRY(hipMemcpyAsync(ranges.data(), d_range.p, ranges.size() * sizeof(Range), hipMemcpyDeviceToHost, st->stream));
    if (n_words)
      HIP_TRY(hipMemcpyAsync(words.data(), d_counts.p, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                             st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    for (size_t k = 0; k < tasks.size(); k++)
      K::merge_host((*out)[k], K::from_device(tasks[k], device_rows[k], K::kRanged ? ranges[k] : Range(),
                                              words.data() + word_off[k]));
    return gather_extra(st, out, err);
  }

  tgx_status reset(tgx_state *st, tgx_error *err) override {
    const auto &tasks = K::tasks(st->plan);
    for (size_t k = 0; k < tasks.size(); k++) host[k] = K::fresh(tasks[k]);
    std::fill(device_rows.begin(), device_rows.end(), 0);
    if (device_ready) TGX_TRY(device_clear(st, err));
    return TGX_OK;
  }

  tgx_status merge_from(tgx_state *, tgx_state *src, tgx_error *err) override {
    std::vector<Host> g;
    TGX_TRY(of(src)->gather(src, &g, err));
    for (size_t k = 0; k < g.size(); k++) {
      // (states of one plan share what the plan fixes; a blob made under something else was refused by
      // tgx_state_deserialize)
      if (K::shape(g[k]) != K::shape(host[k]))
        return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different %s", kName, k,
                    K::kDiffers);
      K::merge_host(host[k], g[k]);
    }
    return TGX_OK;
  }

  // section: { u32 magic, u32 tasks; per task what K::write writes }
  tgx_status serialize(tgx_state *st, Writer &w, tgx_error *err) override {
    const auto &tasks = K::tasks(st->plan);
    std::vector<Host> g;
    TGX_TRY(gather(st, &g, err));
    w.pod(K::kMagic);
    w.pod((uint32_t)tasks.size());
    for (size_t k = 0; k < g.size(); k++) K::write(tasks[k], g[k], w);
    return TGX_OK;
  }

  tgx_status deserialize(tgx_state *st, Reader &r, tgx_error *err) override {
    const auto &tasks = K::tasks(st->plan);
    const uint32_t magic = r.pod<uint32_t>(), n = r.pod<uint32_t>();
    if (!r.ok || magic != K::kMagic || n != tasks.size())
      return fail(err, TGX_INVALID_ARGUMENT, "state blob was produced by a different plan (%s section)", kName);
    for (size_t k = 0; k < tasks.size() && r.ok; k++) TGX_TRY(K::read(tasks[k], host[k], r, k, err));
    if (!r.ok) return fail(err, TGX_INVALID_ARGUMENT, "truncated state blob");
    return TGX_OK;
  }
};

}  // namespace tgx
