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
#include <map>
#include <string>

#include "api_internal.h"
#include "counted_state.h"

namespace tgx {
void launch_group_sums_i64(const ComomentColDesc &d, const GroupSumsTable &t, bool is_float, int blocks,
                           hipStream_t stream);
void launch_group_sums_utf8(const Utf8ColDesc &d, const GroupSumsValue &val, const GroupSumsTable &t, bool is_float,
                            hipStream_t stream);
void launch_group_sums_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                            const Utf8ColDesc &dict, const GroupSumsValue &val, unsigned long long *cells,
                            const GroupSumsTable &t, bool is_float, hipStream_t stream);

namespace {

enum { kNoKeys = 0, kIntKeys = 1, kByteKeys = 2 };
enum { kNoValues = 0, kIntValues = 1, kFloatValues = 2 };
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
  void add(const Sums &o) {
    rows += o.rows;
    non_null += o.non_null;
    si += o.si;
    sf += o.sf;
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

// one task's state as the host sees it
struct GroupSumsHost {
  int kind = kNoKeys, values = kNoValues;
  uint64_t seen = 0;
  Sums null_group, overflow, long_keys;
  std::map<int64_t, Sums> ints;      // ascending int64
  std::map<std::string, Sums> strs;  // ascending bytewise (std::string compares as unsigned bytes)
  bool is_float() const { return values == kFloatValues; }
  uint64_t groups() const { return ints.size() + strs.size(); }
  Sums counted() const {  // (float sums: in ascending key order)
    Sums c;
    for (const auto &e : ints) c.add(e.second);
    for (const auto &e : strs) c.add(e.second);
    return c;
  }
  Sums all() const {
    Sums c = counted();
    c.add(null_group);
    c.add(overflow);
    c.add(long_keys);
    return c;
  }
};

struct NoRange {};

// A task's entries in a blob: n x { key, u64 rows, u64 non_null, u64 sum }, strictly ascending by key, rows > 0,
// non_null <= rows, no sum without a value, into the empty map `m`; *counted: the sum of their rows
template <class Map, class ReadKey>
tgx_status read_entries(size_t k, Reader &r, uint64_t n, size_t least, bool is_float, Map &m, uint64_t *counted,
                        ReadKey read_key, tgx_error *err) {
  size_t bytes = 0;  // (held against the bytes that are left before anything is allocated)
  if (!r.fits(n, least, &bytes)) return TGX_OK;
  *counted = 0;
  for (uint64_t i = 0; i < n; i++) {
    typename Map::key_type key;
    TGX_TRY(read_key(key));
    const uint64_t c = r.pod<uint64_t>(), nn = r.pod<uint64_t>(), sum = r.pod<uint64_t>();
    if (!r.ok) return TGX_OK;
    if (!m.empty() && !(m.rbegin()->first < key))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (GROUP_SUMS task %zu: entry %llu is out of order or repeated)", k,
                  (unsigned long long)i);
    if (c == 0)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (GROUP_SUMS task %zu: entry %llu has a zero count)", k,
                  (unsigned long long)i);
    if (nn > c || (nn == 0 && sum != 0))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (GROUP_SUMS task %zu: entry %llu has non_null > rows, or a sum without a value)", k,
                  (unsigned long long)i);
    if (c > UINT64_MAX - *counted)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (GROUP_SUMS task %zu: counts)", k);
    *counted += c;
    m.emplace_hint(m.end(), std::move(key), Sums::of(c, nn, sum, is_float));
  }
  return TGX_OK;
}

struct GroupSumsKind {
  typedef GroupSumsTask Task;
  typedef GroupSumsHost Host;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_GROUP_SUMS;
  static constexpr const char *kDiffers = "column types";
  static constexpr uint32_t kMagic = 0x4d555347;  // "GSUM"

  static const std::vector<GroupSumsTask> &tasks(const tgx_plan *plan) { return plan->group_sums; }
  static size_t words(const GroupSumsTask &) { return kTaskWords; }
  static NoRange range_identity() { return NoRange(); }
  static GroupSumsHost fresh(const GroupSumsTask &) { return GroupSumsHost(); }
  static size_t shape(const GroupSumsHost &) { return 0; }  // (the two kinds of a host: GroupSumsCheck::merge_from)
  // the classes; the table's entries follow in gather_extra
  static GroupSumsHost from_device(const GroupSumsTask &, int64_t rows, const NoRange &, const unsigned long long *w) {
    GroupSumsHost d;
    if (rows == 0) return d;
    const bool f = w[kGsFloatFlag] != 0;
    d.values = f ? kFloatValues : kIntValues;
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
  static void add_entries(GroupSumsHost &a, const GroupSumsHost &b) {
    if (a.kind == kNoKeys) a.kind = b.kind;
    for (const auto &e : b.ints) a.ints[e.first].add(e.second);
    for (const auto &e : b.strs) a.strs[e.first].add(e.second);
  }
  static void merge_host(GroupSumsHost &a, const GroupSumsHost &b) {
    if (a.values == kNoValues) a.values = b.values;
    a.seen += b.seen;
    a.null_group.add(b.null_group);
    a.overflow.add(b.overflow);
    a.long_keys.add(b.long_keys);
    add_entries(a, b);
  }

  // per task { u32 max_groups, max_value_bytes (the plan's parameters), u32 key kind (0 no keys, 1 int64, 2 bytes),
  //   u32 value kind (0 no rows, 1 integer sums, 2 double sums),
  //   u64 seen, then rows, non_null, sum of the NULL group, of overflow, of the long rows, u64 n_entries,
  //   n_entries x { i64 key | u32 length, u8 bytes[length] ; u64 rows, u64 non_null, u64 sum }, ascending by key }
  // (a sum: the int64 that wrapped, or the double's bits)
  static void write(const GroupSumsTask &t, const GroupSumsHost &h, Writer &w) {
    const bool f = h.is_float();
    w.pod(t.params);
    w.pod((uint32_t)h.kind);
    w.pod((uint32_t)h.values);
    const uint64_t counts[11] = {h.seen,
                                 h.null_group.rows, h.null_group.non_null, h.null_group.bits(f),
                                 h.overflow.rows, h.overflow.non_null, h.overflow.bits(f),
                                 h.long_keys.rows, h.long_keys.non_null, h.long_keys.bits(f),
                                 h.groups()};
    w.pod(counts);
    for (const auto &e : h.ints) {
      w.pod(e.first);
      w.pod(e.second.rows);
      w.pod(e.second.non_null);
      w.pod(e.second.bits(f));
    }
    for (const auto &e : h.strs) {
      w.pod((uint32_t)e.first.size());
      w.put(e.first.data(), e.first.size());
      w.pod(e.second.rows);
      w.pod(e.second.non_null);
      w.pod(e.second.bits(f));
    }
  }

  static tgx_status read(const GroupSumsTask &t, GroupSumsHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_group_sums_params p;
    r.get(&p, sizeof(p));
    const uint32_t kind = r.pod<uint32_t>(), values = r.pod<uint32_t>();
    uint64_t counts[11];
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    if (p.max_groups != t.params.max_groups || p.max_value_bytes != t.params.max_value_bytes)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "GROUP_SUMS task %zu: the blob was summed under other parameters (max_groups %u, max_value_bytes "
                  "%u) than the plan's (%u, %u)",
                  k, p.max_groups, p.max_value_bytes, t.params.max_groups, t.params.max_value_bytes);
    const uint64_t n = counts[10];
    if (kind > kByteKeys || values > kFloatValues || (kind == kNoKeys && n != 0) ||
        (values == kNoValues && (counts[0] != 0 || kind != kNoKeys)))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (GROUP_SUMS task %zu: kind)", k);
    const bool f = values == kFloatValues;
    uint64_t counted = 0;
    if (kind == kIntKeys) {
      TGX_TRY(read_entries(k, r, n, 32, f, h.ints, &counted, [&](int64_t &v) {
        v = r.pod<int64_t>();
        return TGX_OK;
      }, err));
    } else {
      TGX_TRY(read_entries(k, r, n, 28, f, h.strs, &counted, [&](std::string &v) {
        const uint32_t len = r.pod<uint32_t>();
        if (!r.ok) return TGX_OK;
        if (len > t.params.max_value_bytes)
          return fail(err, TGX_INVALID_ARGUMENT,
                      "malformed state blob (GROUP_SUMS task %zu: a key of %u bytes, max_value_bytes is %u)", k, len,
                      t.params.max_value_bytes);
        v.assign(len, '\0');
        r.get(&v[0], len);
        return TGX_OK;
      }, err));
    }
    if (!r.ok) return TGX_OK;
    // counted + null_group_rows + overflow_rows + long_rows == seen (no sum can wrap: each term is held against what is
    // left of seen), no class has more non-NULL values than rows, and none a sum without a value
    uint64_t left = counts[0];
    bool ok = true;
    const uint64_t terms[4] = {counted, counts[1], counts[4], counts[7]};
    for (uint64_t term : terms) {
      ok = ok && term <= left;
      left -= ok ? term : 0;
    }
    for (int c = 1; c < 10; c += 3) ok = ok && counts[c + 1] <= counts[c] && (counts[c + 1] != 0 || counts[c + 2] == 0);
    if (!ok || left != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (GROUP_SUMS task %zu: counted + null_group_rows + overflow_rows + long_rows != "
                  "seen, or a class with non_null > rows or a sum without a value)", k);
    h.kind = (int)kind;
    h.values = (int)values;
    h.seen = counts[0];
    h.null_group = Sums::of(counts[1], counts[2], counts[3], f);
    h.overflow = Sums::of(counts[4], counts[5], counts[6], f);
    h.long_keys = Sums::of(counts[7], counts[8], counts[9], f);
    return TGX_OK;
  }
};

struct GroupSumsCheck final : CountedState<GroupSumsKind> {
  // a task's device part besides its table (made at the first batch, for the kind of key the group column holds):
  // what its sums are, and the per-entry cells of the dictionary route
  struct Dev {
    int kind = kNoKeys, values = kNoValues;
    DevBuf cells;
  };
  std::vector<Dev> dev_part;
  const std::vector<GroupSumsTask> &tasks;  // (the plan's: their parameters are fixed once a state exists)

  explicit GroupSumsCheck(const tgx_plan *plan)
      : CountedState(plan), dev_part(plan->group_sums.size()), tasks(plan->group_sums) {}

  // the table's extra bytes a slot: non_null, sum (the two further counters), then for strings the length and the bytes
  size_t non_null_at(size_t k) const { return table[k].extra_at(); }
  size_t sums_at(size_t k) const { return non_null_at(k) + (size_t)table[k].slots * 8; }
  size_t lens_at(size_t k) const { return sums_at(k) + (size_t)table[k].slots * 8; }
  size_t store_at(size_t k) const { return lens_at(k) + (size_t)table[k].slots * 4; }

  GroupSumsTable view(const tgx_state *st, size_t k) const {
    const Dev &d = dev_part[k];
    const uint64_t slots = table[k].slots;
    uint8_t *base = table[k].buf.as<uint8_t>();
    GroupSumsTable t;
    memset(&t, 0, sizeof(t));
    t.keys = (unsigned long long *)base;
    t.keys2 = d.kind == kByteKeys ? t.keys + slots : nullptr;
    t.rows = (unsigned long long *)(base + table[k].counts_at());
    t.non_null = (unsigned long long *)(base + non_null_at(k));
    t.sums = (unsigned long long *)(base + sums_at(k));
    t.lens = d.kind == kByteKeys ? (uint32_t *)(base + lens_at(k)) : nullptr;
    t.store = d.kind == kByteKeys ? base + store_at(k) : nullptr;
    t.words = d_counts.as<unsigned long long>() + word_off[k];
    t.mask = slots - 1;
    t.salt = (uint64_t)st->plan->fp_key.k[0] | ((uint64_t)st->plan->fp_key.k[1] << 32);
    t.max_value_bytes = tasks[k].params.max_value_bytes;
    return t;
  }

  tgx_status device_clear_extra(tgx_state *st, tgx_error *err) override {
    for (Dev &d : dev_part) d.values = kNoValues;  // (the words are cleared, kGsFloatFlag with them)
    return CountedState::device_clear_extra(st, err);
  }

  tgx_status ensure_table(tgx_state *st, size_t k, int kind, int values, tgx_error *err) {
    Dev &d = dev_part[k];
    if (device_rows[k] > 0 && (d.kind != kind || d.values != values))
      return fail(err, TGX_INVALID_ARGUMENT, "GROUP_SUMS task %zu: a column changed between %s values", k,
                  d.kind != kind ? "integer and string" : "integer and float");
    if (d.kind != kind) {
      const tgx_group_sums_params &p = tasks[k].params;
      const bool strings = kind == kByteKeys;
      TGX_TRY(open_table(st, k, p.max_groups, strings ? 2 : 1, 16 + (strings ? 4 + (size_t)p.max_value_bytes : 0), err,
                         16));
      d.kind = kind;
    }
    if (d.values != values) {
      unsigned long long *flag = d_counts.as<unsigned long long>() + word_off[k] + kGsFloatFlag;
      HIP_TRY(hipMemsetAsync(flag, values == kFloatValues ? 1 : 0, 1, st->stream));  // (the word's low byte)
      d.values = values;
    }
    return TGX_OK;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    for (size_t k = 0; k < tasks.size(); k++) {
      const tgx_column &g = dev[tasks[k].group], &v = dev[tasks[k].column];
      const bool strings = is_any_string(g.type), dict = g.type == TGX_DICT32_UTF8;
      // (Int64 / Float64 views: update_validate refuses what is neither those nor widened to them)
      if ((g.type != TGX_INT64 || !g.values) && !strings && !dict)
        return fail(err, TGX_UNSUPPORTED, "GROUP_SUMS groups by integer and string columns (%d)", g.type);
      if (!is_numeric(v.type) || !v.values)
        return fail(err, TGX_UNSUPPORTED, "GROUP_SUMS sums integer and float columns (%d)", v.type);
      const bool is_float = v.type == TGX_FLOAT64;
      TGX_TRY(ensure_table(st, k, g.type == TGX_INT64 ? kIntKeys : kByteKeys, is_float ? kFloatValues : kIntValues, err));
      const GroupSumsTable t = view(st, k);
      GroupSumsValue val;
      val.values = v.values;
      val.validity = v.validity;
      val.offset = v.offset;
      const uint64_t value_bytes = (uint64_t)nrows * 8 + (v.validity ? (uint64_t)(nrows + 7) / 8 : 0);
      if (g.type == TGX_INT64) {
        ComomentColDesc d;
        memset(&d, 0, sizeof(d));
        const uint64_t bytes = side_fill_x(d, g) + side_fill_y(d, v);
        // 16 waves a workgroup and 96 KiB of LDS: one workgroup a CU
        const int blocks = side_blocks(nrows, kGroupSumsBlock, g_ctx.n_cu, 1, 1);
        TGX_TRY(side_rows_fit("GROUP_SUMS", nrows, blocks, err));
        ProfScope ps(st, "group_sums", bytes);
        launch_group_sums_i64(d, t, is_float, blocks, st->stream);
      } else if (strings) {
        // (per-wave and LDS counters are 32-bit here too: refused as VALUE_COUNTS refuses it)
        TGX_TRY(side_rows_fit("GROUP_SUMS", nrows, 1024, err));
        ProfScope ps(st, "group_sums", value_bytes);
        launch_group_sums_utf8(string_desc(g, g.variadic, plan->fp_key), val, t, is_float, st->stream);
      } else {
        const tgx_column *dc = g.dictionary;
        if (!dc || !is_string(dc->type)) return fail(err, TGX_INVALID_ARGUMENT, "GROUP_SUMS: malformed dictionary");
        TGX_TRY(side_rows_fit("GROUP_SUMS", nrows, 1024, err));
        Dev &d = dev_part[k];
        const size_t cell_bytes = std::max<size_t>(8, (size_t)dc->length * 8 * 3);
        HIP_TRY(d.cells.reserve_roomy(cell_bytes));
        HIP_TRY(hipMemsetAsync(d.cells.p, 0, cell_bytes, st->stream));
        ProfScope ps(st, "group_sums", (uint64_t)g.length * 4 + value_bytes);
        // (without entries every row is a NULL-key row: the count kernel says so, the insert kernel is not launched)
        launch_group_sums_dict((const int32_t *)g.values, g.validity, g.offset, g.length,
                               string_desc(*dc, nullptr, plan->fp_key), val, d.cells.as<unsigned long long>(), t, is_float,
                               st->stream);
      }
      HIP_TRY(hipGetLastError());
      device_rows[k] += nrows;
    }
    return TGX_OK;
  }

  void decode_slot(size_t k, const uint8_t *h, uint64_t s, uint64_t count, GroupSumsHost &o) const override {
    const Dev &d = dev_part[k];
    const uint64_t slots = table[k].slots;
    const Sums c = Sums::of(count, ((const uint64_t *)(h + non_null_at(k)))[s], ((const uint64_t *)(h + sums_at(k)))[s],
                            d.values == kFloatValues);
    if (o.kind == kNoKeys) o.kind = d.kind;
    if (d.kind == kIntKeys) {
      o.ints[(int64_t)((const uint64_t *)h)[s]].add(c);
    } else {
      if (((const uint64_t *)h)[slots + s] == kEmptyKey) return;
      const uint32_t most = tasks[k].params.max_value_bytes, len = std::min(((const uint32_t *)(h + lens_at(k)))[s], most);
      o.strs[std::string((const char *)h + store_at(k) + (size_t)s * most, len)].add(c);
    }
  }

  // (integer keys and string keys, integer sums and float sums do not unite: SideState's merge knows one shape per kind)
  tgx_status merge_from(tgx_state *st, tgx_state *src, tgx_error *err) override {
    std::vector<GroupSumsHost> theirs, mine;
    TGX_TRY(of(src)->gather(src, &theirs, err));
    TGX_TRY(gather(st, &mine, err));
    for (size_t k = 0; k < theirs.size(); k++) {
      if (theirs[k].kind != kNoKeys && mine[k].kind != kNoKeys && theirs[k].kind != mine[k].kind)
        return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different group %s", kName, k,
                    GroupSumsKind::kDiffers);
      if (theirs[k].values != kNoValues && mine[k].values != kNoValues && theirs[k].values != mine[k].values)
        return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different value %s", kName, k,
                    GroupSumsKind::kDiffers);
    }
    for (size_t k = 0; k < theirs.size(); k++) GroupSumsKind::merge_host(host[k], theirs[k]);
    return TGX_OK;
  }

  // one task, read; a state that was fed integer keys under one column type and strings under another holds both
  tgx_status read_task(tgx_state *st, size_t slot, GroupSumsHost *out, tgx_error *err) {
    std::vector<GroupSumsHost> g;
    TGX_TRY(gather(st, &g, err));
    if (!g[slot].ints.empty() && !g[slot].strs.empty())
      return fail(err, TGX_INVALID_ARGUMENT, "GROUP_SUMS task %zu holds integer and string keys", slot);
    *out = std::move(g[slot]);
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    GroupSumsHost h;
    TGX_TRY(read_task(st, (size_t)slot, &h, err));
    const tgx_group_sums_class all = h.all().as_class(h.is_float());
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)all.non_null;
    r->distinct = (int64_t)h.groups();
    r->matches = (int64_t)h.counted().rows;
    r->has_value = all.non_null != 0;
    r->sum_i = all.sum_i;
    r->sum_f = all.sum_f;
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

}  // namespace

tgx_status groupsums_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 < 0)
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
    side_mark(plan, GroupSumsCheck::kIndex, t.column, true);
  }
}

tgx_status groupsums_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err) {
  bool groups = false, values = false;
  for (const GroupSumsTask &t : plan->group_sums) {
    groups |= t.group == column;
    values |= t.column == column;
  }
  const int type = c.type;
  if (groups && (type == TGX_FLOAT64 || type == TGX_FLOAT32 || type == TGX_UINT64 || type == TGX_BOOL))
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
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_GROUP_SUMS, "GROUP_SUMS", &slot, err, "bad arguments"));
  GroupSumsHost h;
  TGX_TRY(static_cast<GroupSumsCheck *>(GroupSumsCheck::of(st))->read_task(st, slot, &h, err));
  const bool f = h.is_float();
  memset(out, 0, sizeof(*out));
  out->seen = h.seen;
  out->groups = h.groups();
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
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_GROUP_SUMS, "GROUP_SUMS", &slot, err, "bad arguments"));
  GroupSumsHost h;
  TGX_TRY(static_cast<GroupSumsCheck *>(GroupSumsCheck::of(st))->read_task(st, slot, &h, err));
  const bool f = h.is_float();
  uint64_t need_bytes = 0;
  for (const auto &e : h.strs) need_bytes += e.first.size();
  *is_bytes = h.kind == kByteKeys ? 1 : 0;
  TGX_TRY(counted_entries_sizes(h.groups(), need_bytes, entries, cap, n_entries, bytes, bytes_cap, n_bytes, err));
  if (!entries) return TGX_OK;
  size_t i = 0;
  uint64_t at = 0;
  for (const auto &e : h.ints) {
    const tgx_group_sums_class c = e.second.as_class(f);
    entries[i++] = tgx_group_sum_entry{e.first, 0, 0, c.rows, c.non_null, c.sum_i, c.sum_f};
  }
  for (const auto &e : h.strs) {
    const tgx_group_sums_class c = e.second.as_class(f);
    if (!e.first.empty()) memcpy(bytes + at, e.first.data(), e.first.size());
    entries[i++] = tgx_group_sum_entry{0, at, (uint64_t)e.first.size(), c.rows, c.non_null, c.sum_i, c.sum_f};
    at += e.first.size();
  }
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
