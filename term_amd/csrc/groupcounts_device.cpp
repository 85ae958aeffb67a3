// groupcounts_device.cpp -- TGX_CHECK_GROUP_COUNTS: completeness per group, SELECT g, COUNT(*), COUNT(col) GROUP BY g
// for a bounded number of groups (the GROUP BY behind the reference's CompletenessAnalyzer::with_grouping,
// TG/analyzers/basic/grouped_completeness.rs:160-200; include/tgx.h has the exact semantics).
//
// A task is one spec: a (value column, group column) pair.  The tasks that share the group column and both bounds ride
// one WALK of the group column, up to kGroupCountsMembers of them (GroupCountsTask::leader / member): the walk has one
// table on the device, the leader's, filled by kernels/groupcounts.hip, whose slots carry the group's rows and one
// non_null counter per member; the rows with a NULL key, with a long key, without a slot and with the free-slot marker
// for a key are counted in the leader's words, each member's non-NULL rows of those classes in its own.  The host part
// of a task is a map from key (int64, or bytes) to (total, non_null) plus the counters: what was merged in or read
// from a blob, and what the device part is folded into whenever the state is read -- so merges, blobs and the
// cross-rank step unite by VALUE, never by fingerprint.  Rows seen are counted on the host.
//
// A TUPLE task (a spec with a column list and no column2) groups by the tuple of its 2 .. 8 columns: its table always
// holds byte keys, an entry's bytes are the tuple's canonical form (group_key.h), NULL is a value of a component -- there
// is no NULL group -- and the tasks that name the same list in the same order, with the same bounds, ride one walk.
//
// keyed_state.h has what the kind shares with VALUE_COUNTS and GROUP_SUMS; here are its payload (total, non_null), its
// classes, its walks -- the tasks of a walk count in the leader's table (CountedState::owner) -- and its launches.
#include "keyed_state.h"

namespace tgx {
void launch_group_counts_tuples(const KeyProbeTupleDesc &L, bool numeric, const GroupMembers &mem,
                                const GroupCountsTable &t, hipStream_t stream);
void launch_group_counts_i64(const ComomentColDesc &d, const GroupMembers &mem, const GroupCountsTable &t, int blocks,
                             hipStream_t stream);
void launch_group_counts_utf8(const Utf8ColDesc &d, const GroupMembers &mem, const GroupCountsTable &t,
                              hipStream_t stream);
void launch_group_counts_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, const GroupMembers &mem, unsigned long long *cells,
                              const GroupCountsTable &t, hipStream_t stream);

namespace {

struct Counts {
  uint64_t total = 0, non_null = 0;
  Counts &operator+=(const Counts &o) {
    total += o.total;
    non_null += o.non_null;
    return *this;
  }
};

// in a blob: u64 total, u64 non_null
struct CountsWire {
  static constexpr int kWords = 2;
  void put(const Counts &c, uint64_t *w) const {
    w[0] = c.total;
    w[1] = c.non_null;
  }
  Counts get(const uint64_t *w) const { return Counts{w[0], w[1]}; }
  const char *refuse(const uint64_t *w) const { return w[1] > w[0] ? "has non_null > total" : nullptr; }
};

// one task's state as the host sees it
struct GroupsHost : KeyedEntries<Counts> {
  uint64_t seen = 0;
  Counts null_group, overflow, long_keys;
  uint64_t value_non_null() const {
    return counted().non_null + null_group.non_null + overflow.non_null + long_keys.non_null;
  }
};

struct NoRange {};

struct GroupsKind {
  typedef GroupCountsTask Task;
  typedef GroupsHost Host;
  typedef Counts Payload;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_GROUP_COUNTS;
  static constexpr const char *kDiffers = "group column types";
  static constexpr const char *kNoun = "key";
  static constexpr const char *kColumn = "the group column";
  static constexpr uint32_t kMagic = 0x544e4347;  // "GCNT"

  static const std::vector<GroupCountsTask> &tasks(const tgx_plan *plan) { return plan->group_counts; }
  static size_t words(const GroupCountsTask &) { return kGroupCountsWords; }
  static uint32_t bound(const GroupCountsTask &t) { return t.params.max_groups; }
  static uint32_t max_value_bytes(const GroupCountsTask &t) { return t.params.max_value_bytes; }
  static NoRange range_identity() { return NoRange(); }
  static GroupsHost fresh(const GroupCountsTask &) { return GroupsHost(); }
  static size_t shape(const GroupsHost &) { return 0; }  // (integer against string keys: KeyedCheck::merge_from)
  // the counters; the table's entries follow in gather_extra.  `w`: the task's words; every task has
  // kGroupCountsWords of them, so the words of its walk's leader, which hold the walk's rows, lie slot - leader tasks
  // in front
  static GroupsHost from_device(const GroupCountsTask &t, int64_t rows, const NoRange &, const unsigned long long *w) {
    const unsigned long long *lw = w - (size_t)(t.slot - t.leader) * kGroupCountsWords;
    GroupsHost d;
    d.seen = (uint64_t)rows;
    d.null_group.total = lw[kGcNullRows];
    d.null_group.non_null = w[kGcNullNonNull];
    d.long_keys.total = lw[kGcLongRows];
    d.long_keys.non_null = w[kGcLongNonNull];
    d.overflow.total = lw[kGcOverflowRows];
    d.overflow.non_null = w[kGcOverflowNonNull];
    if (lw[kGcMarkerRows]) {
      d.kind = kIntKeys;
      Counts &c = d.ints[(int64_t)kEmptyKey];
      c.total = lw[kGcMarkerRows];
      c.non_null = w[kGcMarkerNonNull];
    }
    return d;
  }
  static void merge_host(GroupsHost &a, const GroupsHost &b) {
    a.seen += b.seen;
    a.null_group += b.null_group;
    a.overflow += b.overflow;
    a.long_keys += b.long_keys;
    a.add_entries(b);
  }

  // per task { u32 max_groups, max_value_bytes (the plan's parameters), u32 kind (0 no keys, 1 int64, 2 bytes),
  //   u32 arity (0: the task groups by one column; 2 .. 8: by a tuple, whose entries are canonical tuple keys),
  //   u64 seen, null_group_rows, null_group_non_null, overflow_rows, overflow_non_null, long_rows, long_non_null,
  //   u64 n_entries,
  //   n_entries x { i64 key, u64 total, u64 non_null }  or  { u32 length, u8 bytes[length], u64 total, u64 non_null },
  //   ascending by key }
  static void write(const GroupCountsTask &t, const GroupsHost &h, Writer &w) {
    w.pod(t.params);
    w.pod((uint32_t)h.kind);
    w.pod((uint32_t)t.n_tuple);
    const uint64_t counts[8] = {h.seen, h.null_group.total, h.null_group.non_null, h.overflow.total, h.overflow.non_null,
                                h.long_keys.total, h.long_keys.non_null, h.size()};
    w.pod(counts);
    keyed_write_entries(h, CountsWire(), w);
  }

  static tgx_status read(const GroupCountsTask &t, GroupsHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_group_counts_params p;
    r.get(&p, sizeof(p));
    const uint32_t kind = r.pod<uint32_t>(), arity = r.pod<uint32_t>();
    uint64_t counts[8];
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    if (p.max_groups != t.params.max_groups || p.max_value_bytes != t.params.max_value_bytes)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "GROUP_COUNTS task %zu: the blob was counted under other parameters (max_groups %u, max_value_bytes "
                  "%u) than the plan's (%u, %u)",
                  k, p.max_groups, p.max_value_bytes, t.params.max_groups, t.params.max_value_bytes);
    const uint64_t n = counts[7];
    if (arity != (uint32_t)t.n_tuple && (arity == 0 || (arity >= 2 && arity <= (uint32_t)kGroupMaxTuple)))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "GROUP_COUNTS task %zu: the blob groups by %u columns, the plan's task by %d (0: a single group column)",
                  k, arity, t.n_tuple);
    if (kind > kByteKeys || arity != (uint32_t)t.n_tuple || (kind == kNoKeys && n != 0) ||
        (arity != 0 && kind == kIntKeys))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (GROUP_COUNTS task %zu: kind)", k);
    uint64_t counted = 0;
    TGX_TRY(keyed_read_entries("GROUP_COUNTS", kNoun, k, r, kind, n, t.params.max_value_bytes, CountsWire(), h, &counted,
                               err));
    if (!r.ok) return TGX_OK;
    TGX_TRY(tuple_keys_ok("GROUP_COUNTS", k, t.n_tuple, h, err));
    // counted + null_group_rows + overflow_rows + long_rows == seen, and no class has more non-NULL values than rows
    if (!terms_make(counts[0], {counted, counts[1], counts[3], counts[5]}) || counts[2] > counts[1] ||
        counts[4] > counts[3] || counts[6] > counts[5])
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (GROUP_COUNTS task %zu: counted + null_group_rows + overflow_rows + long_rows != "
                  "seen, or a class with non_null > rows)", k);
    h.kind = (int)kind;
    h.seen = counts[0];
    h.null_group.total = counts[1];
    h.null_group.non_null = counts[2];
    h.overflow.total = counts[3];
    h.overflow.non_null = counts[4];
    h.long_keys.total = counts[5];
    h.long_keys.non_null = counts[6];
    return TGX_OK;
  }
};

struct GroupsCheck final : KeyedCheck<GroupsKind> {
  std::vector<std::vector<int>> walks;  // the tasks of each walk, leader first

  explicit GroupsCheck(const tgx_plan *plan) : KeyedCheck(plan) {
    std::vector<int> walk_of(tasks.size(), -1);  // (by leader)
    for (size_t k = 0; k < tasks.size(); k++) {
      const int leader = tasks[k].leader;
      if (leader == (int)k) {
        walk_of[k] = (int)walks.size();
        walks.emplace_back();
      }
      walks[walk_of[leader]].push_back((int)k);
      owner[k] = (size_t)leader;
    }
  }

  // behind a walk's totals: one array of non_null counters per member
  size_t non_null_at(size_t leader) const { return table[leader].extra_at(); }

  GroupCountsTable view(const tgx_state *st, size_t leader) const {
    uint8_t *base = table[leader].buf.as<uint8_t>();
    GroupCountsTable t;
    fill_view(st, leader, t);
    t.totals = (unsigned long long *)(base + table[leader].counts_at());
    t.non_null = (unsigned long long *)(base + non_null_at(leader));
    t.words = d_counts.as<unsigned long long>();
    t.shared_word = (uint32_t)word_off[leader];
    return t;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    for (const std::vector<int> &walk : walks) {
      const size_t leader = (size_t)walk[0];
      const tgx_column &g = dev[tasks[leader].group];
      const bool tuples = tasks[leader].n_tuple != 0;
      const Route route = route_of(g);
      // (an Int64 view: update_validate refuses what is neither a string layout nor widened to one)
      if (!tuples && (route == kNoRoute || (route == kIntRoute && !g.values)))
        return fail(err, TGX_UNSUPPORTED, "GROUP_COUNTS groups by integer and string columns (%d)", g.type);
      KeyProbeTupleDesc L;
      bool numeric = true;
      uint64_t tuple_bytes = 0;
      if (tuples)
        TGX_TRY(tuple_desc(plan, tasks[leader].tuple, tasks[leader].n_tuple, dev, &L, &numeric, &tuple_bytes, err));
      TGX_TRY(ensure_keys(st, leader, !tuples && route == kIntRoute ? kIntKeys : kByteKeys, walk.size() * 8, err));
      const GroupCountsTable t = view(st, leader);
      GroupMembers mem;
      memset(&mem, 0, sizeof(mem));
      mem.n = (int32_t)walk.size();
      uint64_t bits = 0;  // (what the members' bitmaps add to the bytes moved)
      for (size_t m = 0; m < walk.size(); m++) {
        const tgx_column &v = dev[tasks[walk[m]].column];
        mem.validity[m] = v.validity;
        mem.offset[m] = v.offset;
        mem.word[m] = (uint32_t)word_off[walk[m]];
        bits += v.validity ? (uint64_t)(nrows + 7) / 8 : 0;
      }
      if (tuples) {
        // (per-wave and LDS counters are 32-bit here too)
        TGX_TRY(side_rows_fit("GROUP_COUNTS", nrows, 1024, err));
        ProfScope ps(st, "group_counts_tuples", tuple_bytes + bits);
        launch_group_counts_tuples(L, numeric, mem, t, st->stream);
      } else if (route == kIntRoute) {
        ComomentColDesc d;
        memset(&d, 0, sizeof(d));
        const uint64_t bytes = side_fill_x(d, g);
        // 16 waves a workgroup and 72 .. 128 KiB of LDS: one workgroup a CU
        const int blocks = side_blocks(nrows, kGroupCountsBlock, g_ctx.n_cu, 1, 1);
        TGX_TRY(side_rows_fit("GROUP_COUNTS", nrows, blocks, err));
        ProfScope ps(st, "group_counts", bytes + bits);
        launch_group_counts_i64(d, mem, t, blocks, st->stream);
      } else if (route == kStringRoute) {
        // (per-wave and LDS counters are 32-bit here too: refused as VALUE_COUNTS refuses it)
        TGX_TRY(side_rows_fit("GROUP_COUNTS", nrows, 1024, err));
        ProfScope ps(st, "group_counts", 0);
        launch_group_counts_utf8(string_desc(g, g.variadic, plan->fp_key), mem, t, st->stream);
      } else {
        const tgx_column *dc;
        TGX_TRY(dictionary_of(g, &dc, err));
        TGX_TRY(side_rows_fit("GROUP_COUNTS", nrows, 1024, err));
        unsigned long long *cells;
        TGX_TRY(clear_cells(st, leader, std::max<size_t>(8, (size_t)dc->length * 8 * (1 + walk.size())), &cells, err));
        ProfScope ps(st, "group_counts", (uint64_t)g.length * 4 + bits);
        // (without entries every row is a NULL-key row: the count kernel says so, the insert kernel is not launched)
        launch_group_counts_dict((const int32_t *)g.values, g.validity, g.offset, g.length,
                                 string_desc(*dc, nullptr, plan->fp_key), mem, cells, t, st->stream);
      }
      HIP_TRY(hipGetLastError());
      for (int k : walk) device_rows[k] += nrows;
    }
    return TGX_OK;
  }

  // slot `s` of the table of task k's walk as task k sees it: the group's rows and its own member's counter
  Counts slot_payload(size_t k, const uint8_t *h, uint64_t s, uint64_t count) const override {
    const size_t leader = owner[k];
    return Counts{count, ((const uint64_t *)(h + non_null_at(leader)))[(uint64_t)tasks[k].member * table[leader].slots + s]};
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    GroupsHost h;
    TGX_TRY(read_task(st, (size_t)slot, &h, err));
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)h.value_non_null();
    r->distinct = (int64_t)h.size();
    r->matches = (int64_t)h.counted().total;
    return TGX_OK;
  }
};

// the walks of the tasks that have their parameters: a task joins the latest walk on its group column and bounds that
// has a place left, or opens one
void assign_walks(std::vector<GroupCountsTask> &tasks) {
  for (size_t k = 0; k < tasks.size(); k++) {
    GroupCountsTask &t = tasks[k];
    t.leader = t.slot;
    t.member = 0;
    if (!t.set) continue;
    int leader = -1, members = 0;
    for (size_t j = 0; j < k; j++) {
      const GroupCountsTask &o = tasks[j];
      if (!o.set || o.group != t.group || o.params.max_groups != t.params.max_groups ||
          o.params.max_value_bytes != t.params.max_value_bytes || o.n_tuple != t.n_tuple ||
          !std::equal(t.tuple, t.tuple + t.n_tuple, o.tuple))  // (tuple tasks: the same list in the same order)
        continue;
      if (o.leader == o.slot) {
        leader = o.slot;
        members = 1;
      } else if (o.leader == leader) {
        members++;
      }
    }
    if (leader >= 0 && members < kGroupCountsMembers) {
      t.leader = leader;
      t.member = members;
    }
  }
}

}  // namespace

tgx_status groupcounts_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 < 0 && sp.n_columns < 2)  // (a column list instead: tgx_plan_create hands it to the task)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: GROUP_COUNTS needs column2, the group column", spec_index);
  GroupCountsTask t;
  memset(&t, 0, sizeof(t));
  t.column = sp.column;
  t.group = sp.column2;
  t.spec_index = spec_index;
  t.slot = t.leader = (int)plan->group_counts.size();
  plan->group_counts.push_back(t);
  *slot = t.slot;
  return TGX_OK;
}

tgx_status groupcounts_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const GroupCountsTask &t : plan->group_counts)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "spec %d: a GROUP_COUNTS check needs its parameters (tgx_plan_set_group_counts)", t.spec_index);
  return TGX_OK;
}

// (the value column brings its validity alone: its values are not read and it is not widened)
void groupcounts_mark_columns(tgx_plan *plan) {
  for (const GroupCountsTask &t : plan->group_counts) {
    side_mark(plan, GroupsCheck::kIndex, t.group, true);
    for (int c = 0; c < t.n_tuple; c++) side_mark(plan, GroupsCheck::kIndex, t.tuple[c], true);
    plan->used[t.column] = plan->side_on[GroupsCheck::kIndex][t.column] = 1;
  }
}

tgx_status groupcounts_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err) {
  bool groups = false;  // (a value column may be of any type)
  for (const GroupCountsTask &t : plan->group_counts) {
    groups |= t.group == column;
    for (int g = 0; g < t.n_tuple; g++) groups |= t.tuple[g] == column;
  }
  if (!groups) return TGX_OK;
  const int type = c.type;
  if (refused_as_key(type))
    return fail(err, TGX_UNSUPPORTED, "column %d: GROUP_COUNTS groups by integer and string columns, not %s (type %d)",
                column, type_name(type), type);
  if (c.length > 0 && !c.values && (is_numeric(type) || is_widened(type)))
    return fail(err, TGX_UNSUPPORTED, "column %d: GROUP_COUNTS reads the group keys: a validity-only column has none",
                column);
  return TGX_OK;
}

SideCheck *groupcounts_state_new(const tgx_plan *plan) {
  return plan->group_counts.empty() ? nullptr : new GroupsCheck(plan);
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_group_counts(tgx_plan *plan, size_t spec_index, const tgx_group_counts_params *p,
                                                tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_GROUP_COUNTS, "GROUP_COUNTS", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the parameters of a GROUP_COUNTS check are fixed once a state of the plan exists");
  if (p->max_groups < 1 || p->max_groups > TGX_GROUP_COUNTS_MAX_GROUPS)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_groups must be 1 .. %d (%u)", spec_index,
                (int)TGX_GROUP_COUNTS_MAX_GROUPS, p->max_groups);
  if (p->max_value_bytes < 1 || p->max_value_bytes > TGX_GROUP_COUNTS_MAX_VALUE_BYTES)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_value_bytes must be 1 .. %d (%u)", spec_index,
                (int)TGX_GROUP_COUNTS_MAX_VALUE_BYTES, p->max_value_bytes);
  GroupCountsTask &t = plan->group_counts[slot];
  t.params = *p;
  t.set = true;
  assign_walks(plan->group_counts);
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_group_counts_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                           tgx_group_counts_summary *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  GroupsHost h;
  TGX_TRY(GroupsCheck::read_spec(plan, st, spec_index, &h, err));
  const Counts counted = h.counted();
  out->seen = h.seen;
  out->groups = h.size();
  out->counted = counted.total;
  out->counted_non_null = counted.non_null;
  out->null_group_rows = h.null_group.total;
  out->null_group_non_null = h.null_group.non_null;
  out->overflow_rows = h.overflow.total;
  out->overflow_non_null = h.overflow.non_null;
  out->long_rows = h.long_keys.total;
  out->long_non_null = h.long_keys.non_null;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_group_counts_entries(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                               tgx_group_count_entry *entries, uint64_t cap, uint64_t *n_entries,
                                               uint8_t *bytes, uint64_t bytes_cap, uint64_t *n_bytes, int32_t *is_bytes,
                                               tgx_error *err) try {
  bind_thread();
  if (!n_entries || !n_bytes || !is_bytes) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  GroupsHost h;
  TGX_TRY(GroupsCheck::read_spec(plan, st, spec_index, &h, err));
  return keyed_entries_out(h, entries, cap, n_entries, bytes, bytes_cap, n_bytes, is_bytes,
                           [](int64_t key, uint64_t at, uint64_t length, const Counts &c) {
                             return tgx_group_count_entry{key, at, length, c.total, c.non_null};
                           }, err);
} catch (...) {
  return tgx::abi_exception(err);
}
