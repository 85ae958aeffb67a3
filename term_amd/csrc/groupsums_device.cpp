// groupsums_device.cpp -- TGX_CHECK_GROUP_SUMS: a sum per group, SELECT g, COUNT(*), COUNT(col), SUM(col) GROUP BY g
// for a bounded number of groups (each side of the reference's CrossTableSumConstraint,
// TG/constraints/cross_table_sum.rs:251-262; include/tgx.h has the exact semantics).
//
// A task is one spec: a (value column, group column) pair with a walk and a table of its own on the device, filled by
// kernels/groupsums.hip, whose slots carry the group's rows, its non-NULL values and their sum; the rows with a NULL
// key, with a long key, without a slot and with the free-slot marker for a key are summed in the task's words.  A sum
// is 64 bits that are an integer which wraps or a double, as the value column is; which of the two the device part
// holds is the word kGsFloatFlag, set by the host with the first float batch.  The host part of a task is a map from
// key (int64, or bytes) to (rows, non_null, sum) plus the classes: what was merged in or read from a blob, and what the
// device part is folded into whenever the state is read -- so merges, blobs and the cross-rank step unite by VALUE.
// Rows seen are counted on the host.
//
// A TUPLE task (a spec with a column list and no column2) groups by the tuple of its 2 .. 8 columns, as GROUP_COUNTS's
// tuple tasks do: byte keys always, an entry's bytes the tuple's canonical form (group_key.h), no NULL group.
//
// keyed_state.h has what the kind shares with VALUE_COUNTS and GROUP_COUNTS; here are its payload (rows, non_null, sum),
// its classes, the kind of its sums -- a second thing two batches or two states can differ in -- and its launches.
#include "keyed_state.h"

namespace tgx {
void launch_group_sums_tuples(const KeyProbeTupleDesc &L, bool numeric, const GroupSumsValue &val,
                              const GroupSumsTable &t, bool is_float, hipStream_t stream);
void launch_group_sums_i64(const ComomentColDesc &d, const GroupSumsTable &t, bool is_float, int blocks,
                           hipStream_t stream);
void launch_group_sums_utf8(const Utf8ColDesc &d, const GroupSumsValue &val, const GroupSumsTable &t, bool is_float,
                            hipStream_t stream);
void launch_group_sums_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                            const Utf8ColDesc &dict, const GroupSumsValue &val, unsigned long long *cells,
                            const GroupSumsTable &t, bool is_float, hipStream_t stream);

namespace {

enum SumKind { kNoSums = 0, kIntSums = 1, kFloatSums = 2 };  // (no rows yet: no kind)
constexpr int kGsFloatFlag = kGroupSumsWords;  // the task's word behind the kernels': the device part sums doubles
constexpr int kTaskWords = kGroupSumsWords + 1;

double bits_double(uint64_t b) {
  double d;
  memcpy(&d, &b, 8);
  return d;
}
uint64_t double_bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}

// rows, non-NULL values and their sum: `si` where the values are integers (wrapping), `sf` where they are doubles
struct Sums {
  uint64_t rows = 0, non_null = 0, si = 0;
  double sf = 0.0;
  Sums &operator+=(const Sums &o) {
    rows += o.rows;
    non_null += o.non_null;
    si += o.si;
    sf += o.sf;
    return *this;
  }
  uint64_t bits(bool is_float) const { return is_float ? double_bits(sf) : si; }
  static Sums of(uint64_t rows, uint64_t non_null, uint64_t bits, bool is_float) {
    Sums s;
    s.rows = rows;
    s.non_null = non_null;
    if (is_float) s.sf = bits_double(bits);
    else s.si = bits;
    return s;
  }
  tgx_group_sums_class as_class(bool is_float) const {
    return tgx_group_sums_class{rows, non_null, is_float ? 0 : (int64_t)si, is_float ? sf : (double)(int64_t)si};
  }
};

// an entry's and a class's words in a blob: u64 rows, u64 non_null, u64 sum (the int64 that wrapped, or the double's
// bits); no more values than rows, and no sum without a value
struct SumsWire {
  bool is_float;
  static constexpr int kWords = 3;
  void put(const Sums &s, uint64_t *w) const {
    w[0] = s.rows;
    w[1] = s.non_null;
    w[2] = s.bits(is_float);
  }
  Sums get(const uint64_t *w) const { return Sums::of(w[0], w[1], w[2], is_float); }
  const char *refuse(const uint64_t *w) const {
    return w[1] > w[0] || (w[1] == 0 && w[2] != 0) ? "has non_null > rows, or a sum without a value" : nullptr;
  }
};

// one task's state as the host sees it
struct GroupSumsHost : KeyedEntries<Sums> {
  int values = kNoSums;
  uint64_t seen = 0;
  Sums null_group, overflow, long_keys;
  bool is_float() const { return values == kFloatSums; }
  Sums all() const {
    Sums c = counted();
    c += null_group;
    c += overflow;
    c += long_keys;
    return c;
  }
};

struct NoRange {};

struct GroupSumsKind {
  typedef GroupSumsTask Task;
  typedef GroupSumsHost Host;
  typedef Sums Payload;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_GROUP_SUMS;
  static constexpr const char *kDiffers = "group column types";
  static constexpr const char *kNoun = "key";
  static constexpr const char *kColumn = "a column";
  static constexpr uint32_t kMagic = 0x4d555347;  // "GSUM"

  static const std::vector<GroupSumsTask> &tasks(const tgx_plan *plan) { return plan->group_sums; }
  static size_t words(const GroupSumsTask &) { return kTaskWords; }
  static uint32_t bound(const GroupSumsTask &t) { return t.params.max_groups; }
  static uint32_t max_value_bytes(const GroupSumsTask &t) { return t.params.max_value_bytes; }
  static NoRange range_identity() { return NoRange(); }
  static GroupSumsHost fresh(const GroupSumsTask &) { return GroupSumsHost(); }
  static size_t shape(const GroupSumsHost &) { return 0; }  // (the two kinds of a host: KeyedCheck::merge_from)
  // the classes; the table's entries follow in gather_extra
  static GroupSumsHost from_device(const GroupSumsTask &, int64_t rows, const NoRange &, const unsigned long long *w) {
    GroupSumsHost d;
    if (rows == 0) return d;
    const bool f = w[kGsFloatFlag] != 0;
    d.values = f ? kFloatSums : kIntSums;
    d.seen = (uint64_t)rows;
    d.null_group = Sums::of(w[kGsNull], w[kGsNull + 1], w[kGsNull + 2], f);
    d.long_keys = Sums::of(w[kGsLong], w[kGsLong + 1], w[kGsLong + 2], f);
    d.overflow = Sums::of(w[kGsOverflow], w[kGsOverflow + 1], w[kGsOverflow + 2], f);
    if (w[kGsMarker]) {
      d.kind = kIntKeys;
      d.ints[(int64_t)kEmptyKey] = Sums::of(w[kGsMarker], w[kGsMarker + 1], w[kGsMarker + 2], f);
    }
    return d;
  }
  static void merge_host(GroupSumsHost &a, const GroupSumsHost &b) {
    if (a.values == kNoSums) a.values = b.values;
    a.seen += b.seen;
    a.null_group += b.null_group;
    a.overflow += b.overflow;
    a.long_keys += b.long_keys;
    a.add_entries(b);
  }

  // per task { u32 max_groups, max_value_bytes (the plan's parameters),
  //   u32 key kind (0 no keys, 1 int64, 2 bytes) | arity << 16 (0: the task groups by one column; 2 .. 8: by a tuple,
  //   whose entries are canonical tuple keys -- GROUP_COUNTS's arity word; this record has no spare word for it),
  //   u32 value kind (0 no rows, 1 integer sums, 2 double sums),
  //   u64 seen, then rows, non_null, sum of the NULL group, of overflow, of the long rows, u64 n_entries,
  //   n_entries x { i64 key | u32 length, u8 bytes[length] ; u64 rows, u64 non_null, u64 sum }, ascending by key }
  // (a sum: the int64 that wrapped, or the double's bits)
  static void write(const GroupSumsTask &t, const GroupSumsHost &h, Writer &w) {
    const SumsWire wire{h.is_float()};
    w.pod(t.params);
    w.pod((uint32_t)h.kind | (uint32_t)t.n_tuple << 16);
    w.pod((uint32_t)h.values);
    uint64_t counts[11] = {h.seen};
    wire.put(h.null_group, counts + 1);
    wire.put(h.overflow, counts + 4);
    wire.put(h.long_keys, counts + 7);
    counts[10] = h.size();
    w.pod(counts);
    keyed_write_entries(h, wire, w);
  }

  static tgx_status read(const GroupSumsTask &t, GroupSumsHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_group_sums_params p;
    r.get(&p, sizeof(p));
    const uint32_t kind_word = r.pod<uint32_t>(), values = r.pod<uint32_t>();
    const uint32_t kind = kind_word & 0xffffu, arity = kind_word >> 16;
    uint64_t counts[11];
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    if (p.max_groups != t.params.max_groups || p.max_value_bytes != t.params.max_value_bytes)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "GROUP_SUMS task %zu: the blob was summed under other parameters (max_groups %u, max_value_bytes "
                  "%u) than the plan's (%u, %u)",
                  k, p.max_groups, p.max_value_bytes, t.params.max_groups, t.params.max_value_bytes);
    const uint64_t n = counts[10];
    if (arity != (uint32_t)t.n_tuple && (arity == 0 || (arity >= 2 && arity <= (uint32_t)kGroupMaxTuple)))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "GROUP_SUMS task %zu: the blob groups by %u columns, the plan's task by %d (0: a single group column)", k,
                  arity, t.n_tuple);
    if (kind > kByteKeys || arity != (uint32_t)t.n_tuple || (arity != 0 && kind == kIntKeys) || values > kFloatSums || (kind == kNoKeys && n != 0) ||
        (values == kNoSums && (counts[0] != 0 || kind != kNoKeys)))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (GROUP_SUMS task %zu: kind)", k);
    const SumsWire wire{values == kFloatSums};
    uint64_t counted = 0;
    TGX_TRY(keyed_read_entries("GROUP_SUMS", kNoun, k, r, kind, n, t.params.max_value_bytes, wire, h, &counted, err));
    if (!r.ok) return TGX_OK;
    TGX_TRY(tuple_keys_ok("GROUP_SUMS", k, t.n_tuple, h, err));
    // counted + null_group_rows + overflow_rows + long_rows == seen, no class has more non-NULL values than rows, and
    // none a sum without a value
    bool ok = terms_make(counts[0], {counted, counts[1], counts[4], counts[7]});
    for (int c = 1; c < 10; c += 3) ok = ok && !wire.refuse(counts + c);
    if (!ok)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (GROUP_SUMS task %zu: counted + null_group_rows + overflow_rows + long_rows != "
                  "seen, or a class with non_null > rows or a sum without a value)", k);
    h.kind = (int)kind;
    h.values = (int)values;
    h.seen = counts[0];
    h.null_group = wire.get(counts + 1);
    h.overflow = wire.get(counts + 4);
    h.long_keys = wire.get(counts + 7);
    return TGX_OK;
  }
};

struct GroupSumsCheck final : KeyedCheck<GroupSumsKind> {
  std::vector<int> dev_values;  // per task: what the sums of its device part are (SumKind)

  explicit GroupSumsCheck(const tgx_plan *plan) : KeyedCheck(plan), dev_values(tasks.size(), kNoSums) {}

  // behind the table's rows: the slots' non_null and sum, its two further counters
  size_t non_null_at(size_t k) const { return table[k].extra_at(); }
  size_t sums_at(size_t k) const { return non_null_at(k) + (size_t)table[k].slots * 8; }

  GroupSumsTable view(const tgx_state *st, size_t k) const {
    uint8_t *base = table[k].buf.as<uint8_t>();
    GroupSumsTable t;
    fill_view(st, k, t);
    t.rows = (unsigned long long *)(base + table[k].counts_at());
    t.non_null = (unsigned long long *)(base + non_null_at(k));
    t.sums = (unsigned long long *)(base + sums_at(k));
    t.words = d_counts.as<unsigned long long>() + word_off[k];
    return t;
  }

  tgx_status device_clear_extra(tgx_state *st, tgx_error *err) override {
    std::fill(dev_values.begin(), dev_values.end(), kNoSums);  // (the words are cleared, kGsFloatFlag with them)
    return KeyedCheck::device_clear_extra(st, err);
  }

  // the table made for keys of `kind`, and the device part told what its sums are
  tgx_status ensure_table(tgx_state *st, size_t k, int kind, int values, tgx_error *err) {
    TGX_TRY(ensure_keys(st, k, kind, 16, err));
    if (dev_values[k] == values) return TGX_OK;
    if (device_rows[k] > 0)
      return fail(err, TGX_INVALID_ARGUMENT, "GROUP_SUMS task %zu: a column changed between integer and float values", k);
    unsigned long long *flag = d_counts.as<unsigned long long>() + word_off[k] + kGsFloatFlag;
    HIP_TRY(hipMemsetAsync(flag, values == kFloatSums ? 1 : 0, 1, st->stream));  // (the word's low byte)
    dev_values[k] = values;
    return TGX_OK;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    for (size_t k = 0; k < tasks.size(); k++) {
      const tgx_column &g = dev[tasks[k].group], &v = dev[tasks[k].column];
      const bool tuples = tasks[k].n_tuple != 0;
      const Route route = route_of(g);
      // (Int64 / Float64 views: update_validate refuses what is neither those nor widened to them)
      if (!tuples && (route == kNoRoute || (route == kIntRoute && !g.values)))
        return fail(err, TGX_UNSUPPORTED, "GROUP_SUMS groups by integer and string columns (%d)", g.type);
      KeyProbeTupleDesc L;
      bool numeric = true;
      uint64_t tuple_bytes = 0;
      if (tuples) TGX_TRY(tuple_desc(plan, tasks[k].tuple, tasks[k].n_tuple, dev, &L, &numeric, &tuple_bytes, err));
      if (!is_numeric(v.type) || !v.values)
        return fail(err, TGX_UNSUPPORTED, "GROUP_SUMS sums integer and float columns (%d)", v.type);
      const bool is_float = v.type == TGX_FLOAT64;
      TGX_TRY(ensure_table(st, k, !tuples && route == kIntRoute ? kIntKeys : kByteKeys, is_float ? kFloatSums : kIntSums,
                           err));
      const GroupSumsTable t = view(st, k);
      GroupSumsValue val;
      val.values = v.values;
      val.validity = v.validity;
      val.offset = v.offset;
      const uint64_t value_bytes = (uint64_t)nrows * 8 + (v.validity ? (uint64_t)(nrows + 7) / 8 : 0);
      if (tuples) {
        // (per-wave and LDS counters are 32-bit here too)
        TGX_TRY(side_rows_fit("GROUP_SUMS", nrows, 1024, err));
        ProfScope ps(st, "group_sums_tuples", tuple_bytes + value_bytes);
        launch_group_sums_tuples(L, numeric, val, t, is_float, st->stream);
      } else if (route == kIntRoute) {
        ComomentColDesc d;
        memset(&d, 0, sizeof(d));
        const uint64_t bytes = side_fill_x(d, g) + side_fill_y(d, v);
        // 16 waves a workgroup and 96 KiB of LDS: one workgroup a CU
        const int blocks = side_blocks(nrows, kGroupSumsBlock, g_ctx.n_cu, 1, 1);
        TGX_TRY(side_rows_fit("GROUP_SUMS", nrows, blocks, err));
        ProfScope ps(st, "group_sums", bytes);
        launch_group_sums_i64(d, t, is_float, blocks, st->stream);
      } else if (route == kStringRoute) {
        // (per-wave and LDS counters are 32-bit here too: refused as VALUE_COUNTS refuses it)
        TGX_TRY(side_rows_fit("GROUP_SUMS", nrows, 1024, err));
        ProfScope ps(st, "group_sums", value_bytes);
        launch_group_sums_utf8(string_desc(g, g.variadic, plan->fp_key), val, t, is_float, st->stream);
      } else {
        const tgx_column *dc;
        TGX_TRY(dictionary_of(g, &dc, err));
        TGX_TRY(side_rows_fit("GROUP_SUMS", nrows, 1024, err));
        unsigned long long *cells;
        TGX_TRY(clear_cells(st, k, std::max<size_t>(8, (size_t)dc->length * 8 * 3), &cells, err));
        ProfScope ps(st, "group_sums", (uint64_t)g.length * 4 + value_bytes);
        // (without entries every row is a NULL-key row: the count kernel says so, the insert kernel is not launched)
        launch_group_sums_dict((const int32_t *)g.values, g.validity, g.offset, g.length,
                               string_desc(*dc, nullptr, plan->fp_key), val, cells, t, is_float, st->stream);
      }
      HIP_TRY(hipGetLastError());
      device_rows[k] += nrows;
    }
    return TGX_OK;
  }

  Sums slot_payload(size_t k, const uint8_t *h, uint64_t s, uint64_t count) const override {
    return Sums::of(count, ((const uint64_t *)(h + non_null_at(k)))[s], ((const uint64_t *)(h + sums_at(k)))[s],
                    dev_values[k] == kFloatSums);
  }

  // (integer sums and float sums do not unite either)
  tgx_status merge_refused(size_t k, const GroupSumsHost &theirs, const GroupSumsHost &mine, tgx_error *err) override {
    if (theirs.values != kNoSums && mine.values != kNoSums && theirs.values != mine.values)
      return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different value column types",
                  kName, k);
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    GroupSumsHost h;
    TGX_TRY(read_task(st, (size_t)slot, &h, err));
    const tgx_group_sums_class all = h.all().as_class(h.is_float());
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)all.non_null;
    r->distinct = (int64_t)h.size();
    r->matches = (int64_t)h.counted().rows;
    r->has_value = all.non_null != 0;
    r->sum_i = all.sum_i;
    r->sum_f = all.sum_f;
    return TGX_OK;
  }
};

}  // namespace

tgx_status groupsums_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 < 0 && sp.n_columns < 2)  // (a column list instead: tgx_plan_create hands it to the task)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: GROUP_SUMS needs column2, the group column", spec_index);
  GroupSumsTask t;
  memset(&t, 0, sizeof(t));
  t.column = sp.column;
  t.group = sp.column2;
  t.spec_index = spec_index;
  *slot = (int)plan->group_sums.size();
  plan->group_sums.push_back(t);
  return TGX_OK;
}

tgx_status groupsums_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const GroupSumsTask &t : plan->group_sums)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a GROUP_SUMS check needs its parameters (tgx_plan_set_group_sums)",
                  t.spec_index);
  return TGX_OK;
}

void groupsums_mark_columns(tgx_plan *plan) {
  for (const GroupSumsTask &t : plan->group_sums) {
    side_mark(plan, GroupSumsCheck::kIndex, t.group, true);
    for (int c = 0; c < t.n_tuple; c++) side_mark(plan, GroupSumsCheck::kIndex, t.tuple[c], true);
    side_mark(plan, GroupSumsCheck::kIndex, t.column, true);
  }
}

tgx_status groupsums_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err) {
  bool groups = false, values = false;
  for (const GroupSumsTask &t : plan->group_sums) {
    groups |= t.group == column;
    for (int g = 0; g < t.n_tuple; g++) groups |= t.tuple[g] == column;
    values |= t.column == column;
  }
  const int type = c.type;
  if (groups && refused_as_key(type))
    return fail(err, TGX_UNSUPPORTED, "column %d: GROUP_SUMS groups by integer and string columns, not %s (type %d)",
                column, type_name(type), type);
  if (values && ((!is_numeric(type) && !is_widened(type)) || type == TGX_BOOL))
    return fail(err, TGX_UNSUPPORTED, "column %d: GROUP_SUMS sums integer and float columns, not %s (type %d)", column,
                type_name(type), type);
  if (c.length > 0 && !c.values && (is_numeric(type) || is_widened(type)))
    return fail(err, TGX_UNSUPPORTED, "column %d: GROUP_SUMS reads the column's values: a validity-only column has none",
                column);
  return TGX_OK;
}

SideCheck *groupsums_state_new(const tgx_plan *plan) {
  return plan->group_sums.empty() ? nullptr : new GroupSumsCheck(plan);
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_group_sums(tgx_plan *plan, size_t spec_index, const tgx_group_sums_params *p,
                                              tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_GROUP_SUMS, "GROUP_SUMS", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the parameters of a GROUP_SUMS check are fixed once a state of the plan exists");
  if (p->max_groups < 1 || p->max_groups > TGX_GROUP_SUMS_MAX_GROUPS)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_groups must be 1 .. %d (%u)", spec_index,
                (int)TGX_GROUP_SUMS_MAX_GROUPS, p->max_groups);
  if (p->max_value_bytes < 1 || p->max_value_bytes > TGX_GROUP_SUMS_MAX_VALUE_BYTES)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_value_bytes must be 1 .. %d (%u)", spec_index,
                (int)TGX_GROUP_SUMS_MAX_VALUE_BYTES, p->max_value_bytes);
  GroupSumsTask &t = plan->group_sums[slot];
  t.params = *p;
  t.set = true;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_group_sums_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                         tgx_group_sums_summary *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  GroupSumsHost h;
  TGX_TRY(GroupSumsCheck::read_spec(plan, st, spec_index, &h, err));
  const bool f = h.is_float();
  memset(out, 0, sizeof(*out));
  out->seen = h.seen;
  out->groups = h.size();
  out->is_float = f ? 1 : 0;
  out->counted = h.counted().as_class(f);
  out->null_group = h.null_group.as_class(f);
  out->overflow = h.overflow.as_class(f);
  out->long_rows = h.long_keys.as_class(f);
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_group_sums_entries(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                             tgx_group_sum_entry *entries, uint64_t cap, uint64_t *n_entries,
                                             uint8_t *bytes, uint64_t bytes_cap, uint64_t *n_bytes, int32_t *is_bytes,
                                             tgx_error *err) try {
  bind_thread();
  if (!n_entries || !n_bytes || !is_bytes) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  GroupSumsHost h;
  TGX_TRY(GroupSumsCheck::read_spec(plan, st, spec_index, &h, err));
  const bool f = h.is_float();
  return keyed_entries_out(h, entries, cap, n_entries, bytes, bytes_cap, n_bytes, is_bytes,
                           [f](int64_t key, uint64_t at, uint64_t length, const Sums &s) {
                             const tgx_group_sums_class c = s.as_class(f);
                             return tgx_group_sum_entry{key, at, length, c.rows, c.non_null, c.sum_i, c.sum_f};
                           }, err);
} catch (...) {
  return tgx::abi_exception(err);
}
