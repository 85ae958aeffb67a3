// valuerule_device.cpp -- TGX_CHECK_VALUE_RULE: the numeric row predicates behind the reference's DataTypeConstraint
// (TG/constraints/datatype.rs:144-160, 383-439; include/tgx.h has the modes and their exact semantics).
//
// A task is one spec.  Its running state on the device is three 64-bit counters folded by kernels/valuerule.hip -- the
// rows that pass, the rows on which CAST(col AS INT) fails, the non-NULL rows; rows seen are counted on the host.  What
// is merged in from other states or read from a blob is kept on the host and added when the state is read.  The LAUNCH
// is grouped by column, not by task: one walk of a column evaluates up to eight of its rules, a column with more takes
// another group, and the non-NULL rows are counted once per group, in the counters of its first task (the leader).
// Which key a rule compares and between which bounds is settled here, per batch, from the type the column arrives in
// (device_rule): the kernel's row loop has one range test and the Int32 cast.
#include <math.h>

#include "api_internal.h"

namespace tgx {
void launch_value_rule(const ValueRuleLaunch &L, int n_groups, int blocks_per_group, hipStream_t stream);

namespace {

// one task's state as the host sees it
struct RuleHost {
  uint64_t seen = 0, considered = 0, valid = 0, cast_errors = 0;
};

int64_t key_of(double x) {
  int64_t bits;
  memcpy(&bits, &x, sizeof(bits));
  return f64_total_key(bits);
}

// the rule as the kernel evaluates it on a column of int64 (`is_float` = false) or double values
ValueRule device_rule(const tgx_value_rule_params &p, bool is_float, uint32_t word) {
  ValueRule r;
  memset(&r, 0, sizeof(r));
  r.word = word;
  const bool keyed = is_float || (p.flags & TGX_RULE_BOUNDS_AS_DOUBLE);
  switch (p.mode) {
    case TGX_RULE_GE_ZERO:  // (key(+0.0) is 0, and a key is an integer: > 0 is >= 1)
    case TGX_RULE_GT_ZERO:
      r.kind = is_float ? kRuleRangeKey : kRuleRangeValue;
      r.lo = p.mode == TGX_RULE_GE_ZERO ? 0 : 1;
      r.hi = INT64_MAX;  // (the largest int64, and the key of +NaN with every payload bit set)
      break;
    case TGX_RULE_BETWEEN:
      r.kind = keyed ? kRuleRangeKey : kRuleRangeValue;
      r.lo = keyed ? key_of(p.lo_f) : p.lo_i;
      r.hi = keyed ? key_of(p.hi_f) : p.hi_i;
      break;
    default:
      r.kind = kRuleInteger;
      break;
  }
  return r;
}

struct NoRange {};

struct RuleKind {
  typedef ValueRuleTask Task;
  typedef RuleHost Host;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_VALUE_RULE;
  static constexpr const char *kDiffers = nullptr;  // (every host has the one shape)
  static constexpr uint32_t kMagic = 0x4c525656;  // "VVRL"

  static const std::vector<ValueRuleTask> &tasks(const tgx_plan *plan) { return plan->rules; }
  static size_t words(const ValueRuleTask &) { return kValueRuleWords; }  // valid, cast errors, considered
  static NoRange range_identity() { return NoRange(); }
  static RuleHost fresh(const ValueRuleTask &) { return RuleHost(); }
  static size_t shape(const RuleHost &) { return 0; }
  // (`w`: the task's own counters within the state's array; the leader's lie (slot - leader) tasks before them)
  static RuleHost from_device(const ValueRuleTask &t, int64_t rows, const NoRange &, const unsigned long long *w) {
    RuleHost d;
    d.seen = (uint64_t)rows;
    d.valid = w[0];
    d.cast_errors = w[1];
    d.considered = (w - (ptrdiff_t)(t.slot - t.leader) * kValueRuleWords)[2];
    return d;
  }
  static void merge_host(RuleHost &a, const RuleHost &b) {
    a.seen += b.seen;
    a.considered += b.considered;
    a.valid += b.valid;
    a.cast_errors += b.cast_errors;
  }

  // per task { i32 mode, u32 flags, i64 lo_i, hi_i, f64 lo_f, hi_f (the plan's parameters, as they were set),
  //   u64 seen, considered, valid, cast_errors }
  static void write(const ValueRuleTask &t, const RuleHost &h, Writer &w) {
    w.pod(t.params);
    const uint64_t counts[4] = {h.seen, h.considered, h.valid, h.cast_errors};
    w.pod(counts);
  }

  static tgx_status read(const ValueRuleTask &t, RuleHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_value_rule_params p;
    uint64_t counts[4];
    r.get(&p, sizeof(p));
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    if (memcmp(&p, &t.params, sizeof(p)) != 0)  // (bounds by their bits: -0.0 and +0.0 are different bounds)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "VALUE_RULE task %zu: the blob was counted under other parameters (mode %d) than the plan's (mode %d)", k,
                  p.mode, t.params.mode);
    if (counts[1] > counts[0] || counts[2] > counts[1] || counts[3] > counts[1] - counts[2])
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (VALUE_RULE task %zu)", k);
    h.seen = counts[0];
    h.considered = counts[1];
    h.valid = counts[2];
    h.cast_errors = counts[3];
    return TGX_OK;
  }
};

struct RuleCheck final : SideState<RuleKind> {
  // the launch's column groups: the tasks of one column, at most kValueRulesPerGroup of them, in plan order
  std::vector<std::vector<int>> groups;

  explicit RuleCheck(const tgx_plan *plan) : SideState(plan) {
    std::vector<int> group_of(plan->rules.size(), -1);  // (by leader)
    for (size_t k = 0; k < plan->rules.size(); k++) {
      const int leader = plan->rules[k].leader;
      if (leader == (int)k) {
        group_of[k] = (int)groups.size();
        groups.emplace_back();
      }
      groups[group_of[leader]].push_back((int)k);
    }
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    auto launch = [&](const int *slots, int n) -> tgx_status {
      ValueRuleLaunch L;
      memset(&L, 0, sizeof(L));
      L.counts = d_counts.as<unsigned long long>();
      uint64_t bytes = 0;
      for (int g = 0; g < n; g++) {
        const std::vector<int> &tasks = groups[slots[g]];
        // (an Int64 or Float64 view: update_validate refuses what is neither and is not widened to one)
        const tgx_column &x = dev[plan->rules[tasks[0]].column];
        if (!is_numeric(x.type)) return fail(err, TGX_UNSUPPORTED, "VALUE_RULE takes numeric columns (%d)", x.type);
        bytes += side_fill_x(L.cols[g], x);
        L.n_rules[g] = (int32_t)tasks.size();
        for (size_t r = 0; r < tasks.size(); r++)
          L.rules[g][r] = device_rule(plan->rules[tasks[r]].params, x.type == TGX_FLOAT64, (uint32_t)word_off[tasks[r]]);
      }
      // 8 waves a workgroup, up to 4 workgroups a CU
      const int blocks = side_blocks(nrows, kValueRuleBlock, g_ctx.n_cu, 4, n);
      TGX_TRY(side_rows_fit("VALUE_RULE", nrows, blocks, err));
      ProfScope ps(st, "value_rule", bytes);
      launch_value_rule(L, n, blocks, st->stream);
      HIP_TRY(hipGetLastError());
      for (int g = 0; g < n; g++)
        for (int k : groups[slots[g]]) device_rows[k] += nrows;  // (only rows the device was given)
      return TGX_OK;
    };
    return side_launches(groups, [](const std::vector<int> &) { return true; }, launch);
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    std::vector<RuleHost> g;
    TGX_TRY(gather(st, &g, err));
    r->total = (int64_t)g[slot].seen;
    r->non_null = (int64_t)g[slot].considered;
    r->matches = (int64_t)g[slot].valid;
    r->distinct = (int64_t)g[slot].cast_errors;
    return TGX_OK;
  }
};

}  // namespace

tgx_status valuerule_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 != -1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: VALUE_RULE reads one column: column2 must be -1 (%d)", spec_index,
                sp.column2);
  ValueRuleTask t;
  memset(&t, 0, sizeof(t));
  t.column = sp.column;
  t.spec_index = spec_index;
  t.slot = t.leader = (int)plan->rules.size();
  int earlier = 0;  // tasks of the column so far: every kValueRulesPerGroup-th opens a group
  for (const ValueRuleTask &o : plan->rules)
    if (o.column == t.column) {
      if (++earlier % kValueRulesPerGroup != 0) t.leader = o.leader;
      else t.leader = t.slot;
    }
  plan->rules.push_back(t);
  *slot = (int)plan->rules.size() - 1;
  return TGX_OK;
}

tgx_status valuerule_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const ValueRuleTask &t : plan->rules)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a VALUE_RULE check needs its parameters (tgx_plan_set_value_rule)",
                  t.spec_index);
  return TGX_OK;
}

void valuerule_mark_columns(tgx_plan *plan) {
  for (const ValueRuleTask &t : plan->rules) side_mark(plan, RuleCheck::kIndex, t.column, true);
}

tgx_status valuerule_check_column(const tgx_plan *, int column, const tgx_column &c, tgx_error *err) {
  if (!is_numeric(c.type) && !(is_widened(c.type) && c.type != TGX_BOOL))
    return fail(err, TGX_UNSUPPORTED, "column %d: VALUE_RULE takes numeric columns other than UInt64 (type %d)", column,
                c.type);
  return TGX_OK;
}

SideCheck *valuerule_state_new(const tgx_plan *plan) { return plan->rules.empty() ? nullptr : new RuleCheck(plan); }

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_value_rule(tgx_plan *plan, size_t spec_index, const tgx_value_rule_params *p,
                                              tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_VALUE_RULE, "VALUE_RULE", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the parameters of a VALUE_RULE check are fixed once a state of the plan exists");
  if (p->mode < TGX_RULE_GE_ZERO || p->mode > TGX_RULE_INTEGER)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: unknown VALUE_RULE mode %d", spec_index, p->mode);
  if (p->flags & ~(uint32_t)TGX_RULE_BOUNDS_AS_DOUBLE)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: unknown VALUE_RULE flags 0x%x", spec_index, p->flags);
  if ((p->flags & TGX_RULE_BOUNDS_AS_DOUBLE) && p->mode != TGX_RULE_BETWEEN)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: BOUNDS_AS_DOUBLE goes with the between mode only", spec_index);
  ValueRuleTask &t = plan->rules[slot];
  // (what the mode does not read is kept as zero bits: the blob compares the parameters byte by byte)
  memset(&t.params, 0, sizeof(t.params));
  t.params.mode = p->mode;
  t.params.flags = p->flags;
  if (p->mode == TGX_RULE_BETWEEN) {
    t.params.lo_i = p->lo_i;
    t.params.hi_i = p->hi_i;
    t.params.lo_f = p->lo_f;
    t.params.hi_f = p->hi_f;
  }
  t.set = true;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_value_rule_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                         tgx_value_rule_counts *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_VALUE_RULE, "VALUE_RULE", &slot, err, "bad arguments"));
  std::vector<RuleHost> g;
  TGX_TRY(RuleCheck::of(st)->gather(st, &g, err));
  out->seen = g[slot].seen;
  out->considered = g[slot].considered;
  out->valid = g[slot].valid;
  out->cast_errors = g[slot].cast_errors;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
