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
#include <map>
#include <string>

#include "api_internal.h"
#include "counted_state.h"

namespace tgx {
void launch_group_counts_i64(const ComomentColDesc &d, const GroupMembers &mem, const GroupCountsTable &t, int blocks,
                             hipStream_t stream);
void launch_group_counts_utf8(const Utf8ColDesc &d, const GroupMembers &mem, const GroupCountsTable &t,
                              hipStream_t stream);
void launch_group_counts_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, const GroupMembers &mem, unsigned long long *cells,
                              const GroupCountsTable &t, hipStream_t stream);

namespace {

enum { kNoKeys = 0, kIntKeys = 1, kByteKeys = 2 };

struct Counts {
  uint64_t total = 0, non_null = 0;
  void add(const Counts &o) {
    total += o.total;
    non_null += o.non_null;
  }
};

// one task's state as the host sees it
struct GroupsHost {
  int kind = kNoKeys;
  uint64_t seen = 0;
  Counts null_group, overflow, long_keys;
  std::map<int64_t, Counts> ints;      // ascending int64
  std::map<std::string, Counts> strs;  // ascending bytewise (std::string compares as unsigned bytes)
  uint64_t groups() const { return ints.size() + strs.size(); }
  Counts counted() const {
    Counts c;
    for (const auto &e : ints) c.add(e.second);
    for (const auto &e : strs) c.add(e.second);
    return c;
  }
  uint64_t value_non_null() const {
    return counted().non_null + null_group.non_null + overflow.non_null + long_keys.non_null;
  }
};

struct NoRange {};

struct GroupsKind {
  typedef GroupCountsTask Task;
  typedef GroupsHost Host;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_GROUP_COUNTS;
  static constexpr const char *kDiffers = "group column types";
  static constexpr uint32_t kMagic = 0x544e4347;  // "GCNT"

  static const std::vector<GroupCountsTask> &tasks(const tgx_plan *plan) { return plan->group_counts; }
  static size_t words(const GroupCountsTask &) { return kGroupCountsWords; }
  static NoRange range_identity() { return NoRange(); }
  static GroupsHost fresh(const GroupCountsTask &) { return GroupsHost(); }
  static size_t shape(const GroupsHost &) { return 0; }  // (integer against string keys: GroupsCheck::merge_from)
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
  static void add_entries(GroupsHost &a, const GroupsHost &b) {
    if (a.kind == kNoKeys) a.kind = b.kind;
    for (const auto &e : b.ints) a.ints[e.first].add(e.second);
    for (const auto &e : b.strs) a.strs[e.first].add(e.second);
  }
  static void merge_host(GroupsHost &a, const GroupsHost &b) {
    a.seen += b.seen;
    a.null_group.add(b.null_group);
    a.overflow.add(b.overflow);
    a.long_keys.add(b.long_keys);
    add_entries(a, b);
  }

  // per task { u32 max_groups, max_value_bytes (the plan's parameters), u32 kind (0 no keys, 1 int64, 2 bytes), u32 0,
  //   u64 seen, null_group_rows, null_group_non_null, overflow_rows, overflow_non_null, long_rows, long_non_null,
  //   u64 n_entries,
  //   n_entries x { i64 key, u64 total, u64 non_null }  or  { u32 length, u8 bytes[length], u64 total, u64 non_null },
  //   ascending by key }
  static void write(const GroupCountsTask &t, const GroupsHost &h, Writer &w) {
    w.pod(t.params);
    w.pod((uint32_t)h.kind);
    w.pod((uint32_t)0);
    const uint64_t counts[8] = {h.seen, h.null_group.total, h.null_group.non_null, h.overflow.total, h.overflow.non_null,
                                h.long_keys.total, h.long_keys.non_null, h.groups()};
    w.pod(counts);
    for (const auto &e : h.ints) {
      w.pod(e.first);
      w.pod(e.second.total);
      w.pod(e.second.non_null);
    }
    for (const auto &e : h.strs) {
      w.pod((uint32_t)e.first.size());
      w.put(e.first.data(), e.first.size());
      w.pod(e.second.total);
      w.pod(e.second.non_null);
    }
  }

  static tgx_status read(const GroupCountsTask &t, GroupsHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_group_counts_params p;
    r.get(&p, sizeof(p));
    const uint32_t kind = r.pod<uint32_t>(), pad = r.pod<uint32_t>();
    uint64_t counts[8];
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    if (p.max_groups != t.params.max_groups || p.max_value_bytes != t.params.max_value_bytes)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "GROUP_COUNTS task %zu: the blob was counted under other parameters (max_groups %u, max_value_bytes "
                  "%u) than the plan's (%u, %u)",
                  k, p.max_groups, p.max_value_bytes, t.params.max_groups, t.params.max_value_bytes);
    const uint64_t n = counts[7];
    if (kind > kByteKeys || pad != 0 || (kind == kNoKeys && n != 0))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (GROUP_COUNTS task %zu: kind)", k);
    uint64_t counted = 0, counted_nn = 0;
    if (kind == kIntKeys) {
      TGX_TRY(counted_read_entries2("GROUP_COUNTS", k, r, n, 24, h.ints, &counted, &counted_nn, [&](int64_t &v) {
        v = r.pod<int64_t>();
        return TGX_OK;
      }, err));
    } else {
      TGX_TRY(counted_read_entries2("GROUP_COUNTS", k, r, n, 20, h.strs, &counted, &counted_nn, [&](std::string &v) {
        const uint32_t len = r.pod<uint32_t>();
        if (!r.ok) return TGX_OK;
        if (len > t.params.max_value_bytes)
          return fail(err, TGX_INVALID_ARGUMENT,
                      "malformed state blob (GROUP_COUNTS task %zu: a key of %u bytes, max_value_bytes is %u)", k, len,
                      t.params.max_value_bytes);
        v.assign(len, '\0');
        r.get(&v[0], len);
        return TGX_OK;
      }, err));
    }
    if (!r.ok) return TGX_OK;
    // counted + null_group_rows + overflow_rows + long_rows == seen (no sum can wrap: each term is held against what is
    // left of seen), and no class has more non-NULL values than rows
    uint64_t left = counts[0];
    bool ok = true;
    const uint64_t terms[4] = {counted, counts[1], counts[3], counts[5]};
    for (uint64_t term : terms) {
      ok = ok && term <= left;
      left -= ok ? term : 0;
    }
    if (!ok || left != 0 || counts[2] > counts[1] || counts[4] > counts[3] || counts[6] > counts[5])
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

struct GroupsCheck final : CountedState<GroupsKind> {
  // a walk's device part besides its table (the leader's; made at the first batch, for the kind of key the group
  // column holds): the per-entry cells of the dictionary route
  struct Dev {
    int kind = kNoKeys;
    DevBuf cells;
  };
  std::vector<Dev> dev_part;                 // by leader
  std::vector<std::vector<int>> walks;       // the tasks of each walk, leader first
  const std::vector<GroupCountsTask> &tasks;  // (the plan's: their parameters are fixed once a state exists)

  explicit GroupsCheck(const tgx_plan *plan)
      : CountedState(plan), dev_part(plan->group_counts.size()), tasks(plan->group_counts) {
    std::vector<int> walk_of(tasks.size(), -1);  // (by leader)
    for (size_t k = 0; k < tasks.size(); k++) {
      const int leader = tasks[k].leader;
      if (leader == (int)k) {
        walk_of[k] = (int)walks.size();
        walks.emplace_back();
      }
      walks[walk_of[leader]].push_back((int)k);
    }
  }

  size_t members(size_t leader) const { return table[leader].extra_counters / 8; }
  size_t non_null_at(size_t leader) const { return table[leader].extra_at(); }
  size_t lens_at(size_t leader) const { return non_null_at(leader) + (size_t)table[leader].slots * 8 * members(leader); }
  size_t store_at(size_t leader) const { return lens_at(leader) + (size_t)table[leader].slots * 4; }

  GroupCountsTable view(const tgx_state *st, size_t leader) const {
    const Dev &d = dev_part[leader];
    const uint64_t slots = table[leader].slots;
    uint8_t *base = table[leader].buf.as<uint8_t>();
    GroupCountsTable t;
    memset(&t, 0, sizeof(t));
    t.keys = (unsigned long long *)base;
    t.keys2 = d.kind == kByteKeys ? t.keys + slots : nullptr;
    t.totals = (unsigned long long *)(base + table[leader].counts_at());
    t.non_null = (unsigned long long *)(base + non_null_at(leader));
    t.lens = d.kind == kByteKeys ? (uint32_t *)(base + lens_at(leader)) : nullptr;
    t.store = d.kind == kByteKeys ? base + store_at(leader) : nullptr;
    t.words = d_counts.as<unsigned long long>();
    t.shared_word = (uint32_t)word_off[leader];
    t.mask = slots - 1;
    t.salt = (uint64_t)st->plan->fp_key.k[0] | ((uint64_t)st->plan->fp_key.k[1] << 32);
    t.max_value_bytes = tasks[leader].params.max_value_bytes;
    return t;
  }

  tgx_status ensure_table(tgx_state *st, const std::vector<int> &walk, int kind, tgx_error *err) {
    const size_t leader = (size_t)walk[0];
    Dev &d = dev_part[leader];
    if (d.kind == kind) return TGX_OK;
    if (d.kind != kNoKeys && device_rows[leader] > 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "GROUP_COUNTS task %zu: the group column changed between integer and string values", leader);
    const tgx_group_counts_params &p = tasks[leader].params;
    const bool strings = kind == kByteKeys;
    const size_t counters = walk.size() * 8;
    TGX_TRY(open_table(st, leader, p.max_groups, strings ? 2 : 1,
                       counters + (strings ? 4 + (size_t)p.max_value_bytes : 0), err, counters));
    d.kind = kind;
    return TGX_OK;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    for (const std::vector<int> &walk : walks) {
      const size_t leader = (size_t)walk[0];
      const tgx_column &g = dev[tasks[leader].group];
      const bool strings = is_any_string(g.type), dict = g.type == TGX_DICT32_UTF8;
      // (an Int64 view: update_validate refuses what is neither a string layout nor widened to one)
      if ((g.type != TGX_INT64 || !g.values) && !strings && !dict)
        return fail(err, TGX_UNSUPPORTED, "GROUP_COUNTS groups by integer and string columns (%d)", g.type);
      TGX_TRY(ensure_table(st, walk, g.type == TGX_INT64 ? kIntKeys : kByteKeys, err));
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
      if (g.type == TGX_INT64) {
        ComomentColDesc d;
        memset(&d, 0, sizeof(d));
        const uint64_t bytes = side_fill_x(d, g);
        // 16 waves a workgroup and 72 .. 128 KiB of LDS: one workgroup a CU
        const int blocks = side_blocks(nrows, kGroupCountsBlock, g_ctx.n_cu, 1, 1);
        TGX_TRY(side_rows_fit("GROUP_COUNTS", nrows, blocks, err));
        ProfScope ps(st, "group_counts", bytes + bits);
        launch_group_counts_i64(d, mem, t, blocks, st->stream);
      } else if (strings) {
        // (per-wave and LDS counters are 32-bit here too: refused as VALUE_COUNTS refuses it)
        TGX_TRY(side_rows_fit("GROUP_COUNTS", nrows, 1024, err));
        ProfScope ps(st, "group_counts", 0);
        launch_group_counts_utf8(string_desc(g, g.variadic, plan->fp_key), mem, t, st->stream);
      } else {
        const tgx_column *dc = g.dictionary;
        if (!dc || !is_string(dc->type)) return fail(err, TGX_INVALID_ARGUMENT, "GROUP_COUNTS: malformed dictionary");
        TGX_TRY(side_rows_fit("GROUP_COUNTS", nrows, 1024, err));
        Dev &d = dev_part[leader];
        const size_t cell_bytes = std::max<size_t>(8, (size_t)dc->length * 8 * (1 + walk.size()));
        HIP_TRY(d.cells.reserve_roomy(cell_bytes));
        HIP_TRY(hipMemsetAsync(d.cells.p, 0, cell_bytes, st->stream));
        ProfScope ps(st, "group_counts", (uint64_t)g.length * 4 + bits);
        // (without entries every row is a NULL-key row: the count kernel says so, the insert kernel is not launched)
        launch_group_counts_dict((const int32_t *)g.values, g.validity, g.offset, g.length,
                                 string_desc(*dc, nullptr, plan->fp_key), mem, d.cells.as<unsigned long long>(), t,
                                 st->stream);
      }
      HIP_TRY(hipGetLastError());
      for (int k : walk) device_rows[k] += nrows;
    }
    return TGX_OK;
  }

  // slot `s` of the table of task k's walk as task k sees it: the group's rows and its own member's counter
  void decode_slot(size_t k, const uint8_t *h, uint64_t s, uint64_t count, GroupsHost &o) const override {
    const size_t leader = (size_t)tasks[k].leader;
    const Dev &d = dev_part[leader];
    const uint64_t slots = table[leader].slots;
    Counts c;
    c.total = count;
    c.non_null = ((const uint64_t *)(h + non_null_at(leader)))[(uint64_t)tasks[k].member * slots + s];
    if (o.kind == kNoKeys) o.kind = d.kind;
    if (d.kind == kIntKeys) {
      o.ints[(int64_t)((const uint64_t *)h)[s]].add(c);
    } else {
      if (((const uint64_t *)h)[slots + s] == kEmptyKey) return;
      const uint32_t most = tasks[leader].params.max_value_bytes,
                     len = std::min(((const uint32_t *)(h + lens_at(leader)))[s], most);
      o.strs[std::string((const char *)h + store_at(leader) + (size_t)s * most, len)].add(c);
    }
  }

  // the walks' tables into the gathered hosts: a table is copied once and decoded for every member of its walk
  tgx_status gather_extra(tgx_state *st, std::vector<GroupsHost> *out, tgx_error *err) override {
    std::vector<uint8_t> h;
    if (!table_cache_ok) table_cache.assign(table.size(), GroupsHost());
    for (size_t w = 0; w < walks.size() && !table_cache_ok; w++) {
      const size_t leader = (size_t)walks[w][0];
      const CountedTable &t = table[leader];
      if (!t.live || device_rows[leader] == 0) continue;
      h.resize(t.bytes());
      HIP_TRY(hipMemcpyAsync(h.data(), t.buf.p, h.size(), hipMemcpyDeviceToHost, st->stream));
      HIP_TRY(hipStreamSynchronize(st->stream));
      const uint64_t *keys = (const uint64_t *)h.data(), *counts = (const uint64_t *)(h.data() + t.counts_at());
      for (uint64_t s = 0; s < t.slots; s++)
        if (keys[s] != kEmptyKey && counts[s] != 0)
          for (int k : walks[w]) decode_slot((size_t)k, h.data(), s, counts[s], table_cache[k]);
    }
    table_cache_ok = true;
    for (size_t k = 0; k < table.size(); k++) GroupsKind::add_entries((*out)[k], table_cache[k]);
    return TGX_OK;
  }

  // (integer keys and string keys do not unite: SideState's merge knows one shape per kind)
  tgx_status merge_from(tgx_state *st, tgx_state *src, tgx_error *err) override {
    std::vector<GroupsHost> theirs, mine;
    TGX_TRY(of(src)->gather(src, &theirs, err));
    TGX_TRY(gather(st, &mine, err));
    for (size_t k = 0; k < theirs.size(); k++)
      if (theirs[k].kind != kNoKeys && mine[k].kind != kNoKeys && theirs[k].kind != mine[k].kind)
        return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different %s", kName, k,
                    GroupsKind::kDiffers);
    for (size_t k = 0; k < theirs.size(); k++) GroupsKind::merge_host(host[k], theirs[k]);
    return TGX_OK;
  }

  // one task, read; a state that was fed integer keys under one column type and strings under another holds both
  tgx_status read_task(tgx_state *st, size_t slot, GroupsHost *out, tgx_error *err) {
    std::vector<GroupsHost> g;
    TGX_TRY(gather(st, &g, err));
    if (!g[slot].ints.empty() && !g[slot].strs.empty())
      return fail(err, TGX_INVALID_ARGUMENT, "GROUP_COUNTS task %zu holds integer and string keys", slot);
    *out = std::move(g[slot]);
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    GroupsHost h;
    TGX_TRY(read_task(st, (size_t)slot, &h, err));
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)h.value_non_null();
    r->distinct = (int64_t)h.groups();
    r->matches = (int64_t)h.counted().total;
    return TGX_OK;
  }
};

const char *type_name(int type) {
  switch (type) {
    case TGX_FLOAT64: return "Float64";
    case TGX_FLOAT32: return "Float32";
    case TGX_UINT64: return "UInt64";
    case TGX_BOOL: return "Boolean";
    default: return "this type";
  }
}

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
          o.params.max_value_bytes != t.params.max_value_bytes)
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
  if (sp.column2 < 0)
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
    plan->used[t.column] = plan->side_on[GroupsCheck::kIndex][t.column] = 1;
  }
}

tgx_status groupcounts_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err) {
  bool groups = false;  // (a value column may be of any type)
  for (const GroupCountsTask &t : plan->group_counts) groups |= t.group == column;
  if (!groups) return TGX_OK;
  const int type = c.type;
  if (type == TGX_FLOAT64 || type == TGX_FLOAT32 || type == TGX_UINT64 || type == TGX_BOOL)
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
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_GROUP_COUNTS, "GROUP_COUNTS", &slot, err, "bad arguments"));
  GroupsHost h;
  TGX_TRY(static_cast<GroupsCheck *>(GroupsCheck::of(st))->read_task(st, slot, &h, err));
  const Counts counted = h.counted();
  out->seen = h.seen;
  out->groups = h.groups();
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
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_GROUP_COUNTS, "GROUP_COUNTS", &slot, err, "bad arguments"));
  GroupsHost h;
  TGX_TRY(static_cast<GroupsCheck *>(GroupsCheck::of(st))->read_task(st, slot, &h, err));
  uint64_t need_bytes = 0;
  for (const auto &e : h.strs) need_bytes += e.first.size();
  *is_bytes = h.kind == kByteKeys ? 1 : 0;
  TGX_TRY(counted_entries_sizes(h.groups(), need_bytes, entries, cap, n_entries, bytes, bytes_cap, n_bytes, err));
  if (!entries) return TGX_OK;
  size_t i = 0;
  uint64_t at = 0;
  for (const auto &e : h.ints) entries[i++] = tgx_group_count_entry{e.first, 0, 0, e.second.total, e.second.non_null};
  for (const auto &e : h.strs) {
    if (!e.first.empty()) memcpy(bytes + at, e.first.data(), e.first.size());
    entries[i++] = tgx_group_count_entry{0, at, (uint64_t)e.first.size(), e.second.total, e.second.non_null};
    at += e.first.size();
  }
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
