// valuecounts_device.cpp -- TGX_CHECK_VALUE_COUNTS: how often each value of one column occurs, for a bounded number of
// distinct values (the GROUP BY behind the reference's HistogramConstraint, TG/constraints/histogram.rs:205-391, and
// EntropyAnalyzer, TG/analyzers/advanced/entropy.rs:192-335; include/tgx.h has the exact semantics).
//
// A task is one spec.  Its running state on the device is four 64-bit counters (non-NULL rows, rows holding the value
// whose bits are the free-slot marker, overflow rows, long rows) and one open-addressing table filled by
// kernels/valuecounts.hip: integer keys with their counts, or string keys (two fingerprint words) with their counts,
// lengths and bytes.  The table is allocated at the task's first batch, when the column's kind is known.  The host part
// is a map from value (int64, or bytes) to count plus the same counters: what was merged in or read from a blob, and
// what the device part is folded into whenever the state is read (gather_extra) -- so merges, blobs and the cross-rank
// step unite by VALUE, never by fingerprint.  Rows seen are counted on the host.
#include <map>
#include <string>

#include "api_internal.h"
#include "counted_state.h"

namespace tgx {
void launch_value_counts_i64(const ComomentColDesc &d, const ValueCountsTable &t, int blocks, hipStream_t stream);
void launch_value_counts_utf8(const Utf8ColDesc &d, const ValueCountsTable &t, hipStream_t stream);
void launch_value_counts_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, unsigned long long *cells, const ValueCountsTable &t,
                              hipStream_t stream);

namespace {

enum { kNoValues = 0, kIntValues = 1, kByteValues = 2 };

// one task's state as the host sees it
struct CountsHost {
  int kind = kNoValues;
  uint64_t seen = 0, non_null = 0, overflow_rows = 0, long_rows = 0;
  std::map<int64_t, uint64_t> ints;      // ascending int64
  std::map<std::string, uint64_t> strs;  // ascending bytewise (std::string compares as unsigned bytes)
  uint64_t distinct() const { return ints.size() + strs.size(); }
  uint64_t counted() const {
    uint64_t n = 0;
    for (const auto &e : ints) n += e.second;
    for (const auto &e : strs) n += e.second;
    return n;
  }
};

struct NoRange {};

struct CountsKind {
  typedef ValueCountsTask Task;
  typedef CountsHost Host;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_VALUE_COUNTS;
  static constexpr const char *kDiffers = "column types";
  static constexpr uint32_t kMagic = 0x544e4356;  // "VCNT"

  static const std::vector<ValueCountsTask> &tasks(const tgx_plan *plan) { return plan->value_counts; }
  static size_t words(const ValueCountsTask &) { return kValueCountsWords; }
  static NoRange range_identity() { return NoRange(); }
  static CountsHost fresh(const ValueCountsTask &) { return CountsHost(); }
  static size_t shape(const CountsHost &) { return 0; }  // (integer against string values: CountsCheck::merge_from)
  // the counters; the table's entries follow in gather_extra
  static CountsHost from_device(const ValueCountsTask &, int64_t rows, const NoRange &, const unsigned long long *w) {
    CountsHost d;
    d.seen = (uint64_t)rows;
    d.non_null = w[kVcNonNull];
    d.overflow_rows = w[kVcOverflow];
    d.long_rows = w[kVcLong];
    if (w[kVcMarker]) {
      d.kind = kIntValues;
      d.ints[(int64_t)kEmptyKey] = w[kVcMarker];
    }
    return d;
  }
  static void add_entries(CountsHost &a, const CountsHost &b) {
    if (a.kind == kNoValues) a.kind = b.kind;
    for (const auto &e : b.ints) a.ints[e.first] += e.second;
    for (const auto &e : b.strs) a.strs[e.first] += e.second;
  }
  static void merge_host(CountsHost &a, const CountsHost &b) {
    a.seen += b.seen;
    a.non_null += b.non_null;
    a.overflow_rows += b.overflow_rows;
    a.long_rows += b.long_rows;
    add_entries(a, b);
  }

  // per task { u32 max_distinct, max_value_bytes (the plan's parameters), u32 kind (0 no values, 1 int64, 2 bytes), u32 0,
  //   u64 seen, non_null, overflow_rows, long_rows, u64 n_entries,
  //   n_entries x { i64 value, u64 count }  or  { u32 length, u8 bytes[length], u64 count }, ascending by value }
  static void write(const ValueCountsTask &t, const CountsHost &h, Writer &w) {
    w.pod(t.params);
    w.pod((uint32_t)h.kind);
    w.pod((uint32_t)0);
    const uint64_t counts[5] = {h.seen, h.non_null, h.overflow_rows, h.long_rows, h.distinct()};
    w.pod(counts);
    for (const auto &e : h.ints) {
      w.pod(e.first);
      w.pod(e.second);
    }
    for (const auto &e : h.strs) {
      w.pod((uint32_t)e.first.size());
      w.put(e.first.data(), e.first.size());
      w.pod(e.second);
    }
  }

  static tgx_status read(const ValueCountsTask &t, CountsHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_value_counts_params p;
    r.get(&p, sizeof(p));
    const uint32_t kind = r.pod<uint32_t>(), pad = r.pod<uint32_t>();
    uint64_t counts[5];
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    if (p.max_distinct != t.params.max_distinct || p.max_value_bytes != t.params.max_value_bytes)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "VALUE_COUNTS task %zu: the blob was counted under other parameters (max_distinct %u, max_value_bytes "
                  "%u) than the plan's (%u, %u)",
                  k, p.max_distinct, p.max_value_bytes, t.params.max_distinct, t.params.max_value_bytes);
    const uint64_t n = counts[4];
    if (kind > kByteValues || pad != 0 || (kind == kNoValues && n != 0))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (VALUE_COUNTS task %zu: kind)", k);
    uint64_t counted = 0;
    if (kind == kIntValues) {
      TGX_TRY(counted_read_entries("VALUE_COUNTS", k, r, n, 16, h.ints, &counted, [&](int64_t &v) {
        v = r.pod<int64_t>();
        return TGX_OK;
      }, err));
    } else {
      TGX_TRY(counted_read_entries("VALUE_COUNTS", k, r, n, 12, h.strs, &counted, [&](std::string &v) {
        const uint32_t len = r.pod<uint32_t>();
        if (!r.ok) return TGX_OK;
        if (len > t.params.max_value_bytes)
          return fail(err, TGX_INVALID_ARGUMENT,
                      "malformed state blob (VALUE_COUNTS task %zu: a value of %u bytes, max_value_bytes is %u)", k, len,
                      t.params.max_value_bytes);
        v.assign(len, '\0');
        r.get(&v[0], len);
        return TGX_OK;
      }, err));
    }
    if (!r.ok) return TGX_OK;
    // counted + overflow_rows + long_rows == non_null <= seen (no sum can wrap: each term is held against non_null)
    const uint64_t non_null = counts[1];
    if (non_null > counts[0] || counted > non_null || counts[2] > non_null - counted ||
        counts[3] != non_null - counted - counts[2])
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (VALUE_COUNTS task %zu: counted + overflow_rows + long_rows != non_null)", k);
    h.kind = (int)kind;
    h.seen = counts[0];
    h.non_null = non_null;
    h.overflow_rows = counts[2];
    h.long_rows = counts[3];
    return TGX_OK;
  }
};

struct CountsCheck final : CountedState<CountsKind> {
  // the device part of a task besides its table (made at the first batch, for the kind of value the column holds: one
  // key word and nothing behind the counts for integers, two key words, the lengths and the byte store for strings):
  // the per-entry cells of the dictionary route
  struct Dev {
    int kind = kNoValues;
    DevBuf cells;
  };
  std::vector<Dev> dev_part;
  const std::vector<ValueCountsTask> &tasks;  // (the plan's: their parameters are fixed once a state exists)

  explicit CountsCheck(const tgx_plan *plan)
      : CountedState(plan), dev_part(plan->value_counts.size()), tasks(plan->value_counts) {}

  size_t lens_at(size_t k) const { return table[k].extra_at(); }
  size_t store_at(size_t k) const { return lens_at(k) + (size_t)table[k].slots * 4; }

  ValueCountsTable view(const tgx_state *st, size_t k) const {
    const Dev &d = dev_part[k];
    const uint64_t slots = table[k].slots;
    uint8_t *base = table[k].buf.as<uint8_t>();
    ValueCountsTable t;
    memset(&t, 0, sizeof(t));
    t.keys = (unsigned long long *)base;
    t.keys2 = d.kind == kByteValues ? t.keys + slots : nullptr;
    t.counts = (unsigned long long *)(base + table[k].counts_at());
    t.lens = d.kind == kByteValues ? (uint32_t *)(base + lens_at(k)) : nullptr;
    t.store = d.kind == kByteValues ? base + store_at(k) : nullptr;
    t.words = d_counts.as<unsigned long long>() + word_off[k];
    t.mask = slots - 1;
    t.salt = (uint64_t)st->plan->fp_key.k[0] | ((uint64_t)st->plan->fp_key.k[1] << 32);
    t.max_value_bytes = tasks[k].params.max_value_bytes;
    return t;
  }

  tgx_status ensure_table(tgx_state *st, size_t k, int kind, tgx_error *err) {
    Dev &d = dev_part[k];
    if (d.kind == kind) return TGX_OK;
    if (d.kind != kNoValues && device_rows[k] > 0)
      return fail(err, TGX_INVALID_ARGUMENT, "VALUE_COUNTS task %zu: the column changed between integer and string values",
                  k);
    const tgx_value_counts_params &p = tasks[k].params;
    const bool strings = kind == kByteValues;
    TGX_TRY(open_table(st, k, p.max_distinct, strings ? 2 : 1, strings ? 4 + (size_t)p.max_value_bytes : 0, err));
    d.kind = kind;
    return TGX_OK;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    for (size_t k = 0; k < plan->value_counts.size(); k++) {
      const tgx_column &x = dev[plan->value_counts[k].column];
      const bool strings = is_any_string(x.type), dict = x.type == TGX_DICT32_UTF8;
      // (an Int64 view: update_validate refuses what is neither a string layout nor widened to one)
      if (x.type != TGX_INT64 && !strings && !dict)
        return fail(err, TGX_UNSUPPORTED, "VALUE_COUNTS takes integer and string columns (%d)", x.type);
      TGX_TRY(ensure_table(st, k, x.type == TGX_INT64 ? kIntValues : kByteValues, err));
      const ValueCountsTable t = view(st, k);
      if (x.type == TGX_INT64) {
        ComomentColDesc d;
        memset(&d, 0, sizeof(d));
        const uint64_t bytes = side_fill_x(d, x);
        // 16 waves a workgroup and 96 KiB of LDS: one workgroup a CU
        const int blocks = side_blocks(nrows, kValueCountsBlock, g_ctx.n_cu, 1, 1);
        TGX_TRY(side_rows_fit("VALUE_COUNTS", nrows, blocks, err));
        ProfScope ps(st, "value_counts", bytes);
        launch_value_counts_i64(d, t, blocks, st->stream);
      } else if (strings) {
        // (per-lane and LDS counters are 32-bit here too: the launchers take up to 2048 workgroups, 1024 for the
        //  dictionary's indices, so a batch would need 2^42 rows to wrap one; refused all the same)
        TGX_TRY(side_rows_fit("VALUE_COUNTS", nrows, 1024, err));
        ProfScope ps(st, "value_counts", 0);
        launch_value_counts_utf8(string_desc(x, x.variadic, plan->fp_key), t, st->stream);
      } else {
        const tgx_column *dc = x.dictionary;
        if (!dc || !is_string(dc->type)) return fail(err, TGX_INVALID_ARGUMENT, "VALUE_COUNTS: malformed dictionary");
        TGX_TRY(side_rows_fit("VALUE_COUNTS", nrows, 1024, err));
        if (dc->length > 0) {  // (without entries every row is a row without a value)
          Dev &d = dev_part[k];
          HIP_TRY(d.cells.reserve_roomy((size_t)dc->length * 8));
          HIP_TRY(hipMemsetAsync(d.cells.p, 0, (size_t)dc->length * 8, st->stream));
          ProfScope ps(st, "value_counts", (uint64_t)x.length * 4);
          launch_value_counts_dict((const int32_t *)x.values, x.validity, x.offset, x.length,
                                   string_desc(*dc, nullptr, plan->fp_key), d.cells.as<unsigned long long>(), t,
                                   st->stream);
        }
      }
      HIP_TRY(hipGetLastError());
      device_rows[k] += nrows;
    }
    return TGX_OK;
  }

  void decode_slot(size_t k, const uint8_t *h, uint64_t s, uint64_t count, CountsHost &o) const override {
    const Dev &d = dev_part[k];
    if (o.kind == kNoValues) o.kind = d.kind;
    if (d.kind == kIntValues) {
      o.ints[(int64_t)((const uint64_t *)h)[s]] += count;
    } else {
      const uint32_t most = tasks[k].params.max_value_bytes, len = std::min(((const uint32_t *)(h + lens_at(k)))[s], most);
      o.strs[std::string((const char *)h + store_at(k) + (size_t)s * most, len)] += count;
    }
  }

  // (integer values and string values do not unite: SideState's merge knows one shape per kind)
  tgx_status merge_from(tgx_state *st, tgx_state *src, tgx_error *err) override {
    std::vector<CountsHost> theirs, mine;
    TGX_TRY(of(src)->gather(src, &theirs, err));
    TGX_TRY(gather(st, &mine, err));
    for (size_t k = 0; k < theirs.size(); k++)
      if (theirs[k].kind != kNoValues && mine[k].kind != kNoValues && theirs[k].kind != mine[k].kind)
        return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different %s", kName, k,
                    CountsKind::kDiffers);
    for (size_t k = 0; k < theirs.size(); k++) CountsKind::merge_host(host[k], theirs[k]);
    return TGX_OK;
  }

  // one task, read; a state that was fed integers under one column type and strings under another holds both
  tgx_status read_task(tgx_state *st, size_t slot, CountsHost *out, tgx_error *err) {
    std::vector<CountsHost> g;
    TGX_TRY(gather(st, &g, err));
    if (!g[slot].ints.empty() && !g[slot].strs.empty())
      return fail(err, TGX_INVALID_ARGUMENT, "VALUE_COUNTS task %zu holds integer and string values", slot);
    *out = std::move(g[slot]);
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    CountsHost h;
    TGX_TRY(read_task(st, (size_t)slot, &h, err));
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)h.non_null;
    r->distinct = (int64_t)h.distinct();
    r->matches = (int64_t)h.counted();
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

tgx_status valuecounts_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 != -1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: VALUE_COUNTS reads one column: column2 must be -1 (%d)", spec_index,
                sp.column2);
  ValueCountsTask t;
  memset(&t, 0, sizeof(t));
  t.column = sp.column;
  t.spec_index = spec_index;
  plan->value_counts.push_back(t);
  *slot = (int)plan->value_counts.size() - 1;
  return TGX_OK;
}

tgx_status valuecounts_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const ValueCountsTask &t : plan->value_counts)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "spec %d: a VALUE_COUNTS check needs its parameters (tgx_plan_set_value_counts)", t.spec_index);
  return TGX_OK;
}

void valuecounts_mark_columns(tgx_plan *plan) {
  for (const ValueCountsTask &t : plan->value_counts) side_mark(plan, CountsCheck::kIndex, t.column, true);
}

tgx_status valuecounts_check_column(const tgx_plan *, int column, const tgx_column &c, tgx_error *err) {
  const int type = c.type;
  if (type == TGX_FLOAT64 || type == TGX_FLOAT32 || type == TGX_UINT64 || type == TGX_BOOL)
    return fail(err, TGX_UNSUPPORTED, "column %d: VALUE_COUNTS takes integer and string columns, not %s (type %d)", column,
                type_name(type), type);
  return TGX_OK;
}

SideCheck *valuecounts_state_new(const tgx_plan *plan) {
  return plan->value_counts.empty() ? nullptr : new CountsCheck(plan);
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_value_counts(tgx_plan *plan, size_t spec_index, const tgx_value_counts_params *p,
                                                tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_VALUE_COUNTS, "VALUE_COUNTS", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the parameters of a VALUE_COUNTS check are fixed once a state of the plan exists");
  if (p->max_distinct < 1 || p->max_distinct > TGX_VALUE_COUNTS_MAX_DISTINCT)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_distinct must be 1 .. %d (%u)", spec_index,
                (int)TGX_VALUE_COUNTS_MAX_DISTINCT, p->max_distinct);
  if (p->max_value_bytes < 1 || p->max_value_bytes > TGX_VALUE_COUNTS_MAX_VALUE_BYTES)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_value_bytes must be 1 .. %d (%u)", spec_index,
                (int)TGX_VALUE_COUNTS_MAX_VALUE_BYTES, p->max_value_bytes);
  ValueCountsTask &t = plan->value_counts[slot];
  t.params = *p;
  t.set = true;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_value_counts_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                           tgx_value_counts_summary *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_VALUE_COUNTS, "VALUE_COUNTS", &slot, err, "bad arguments"));
  CountsHost h;
  TGX_TRY(static_cast<CountsCheck *>(CountsCheck::of(st))->read_task(st, slot, &h, err));
  out->seen = h.seen;
  out->non_null = h.non_null;
  out->distinct = h.distinct();
  out->counted = h.counted();
  out->overflow_rows = h.overflow_rows;
  out->long_rows = h.long_rows;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_value_counts_entries(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                               tgx_value_count_entry *entries, uint64_t cap, uint64_t *n_entries,
                                               uint8_t *bytes, uint64_t bytes_cap, uint64_t *n_bytes, int32_t *is_bytes,
                                               tgx_error *err) try {
  bind_thread();
  if (!n_entries || !n_bytes || !is_bytes) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_VALUE_COUNTS, "VALUE_COUNTS", &slot, err, "bad arguments"));
  CountsHost h;
  TGX_TRY(static_cast<CountsCheck *>(CountsCheck::of(st))->read_task(st, slot, &h, err));
  uint64_t need_bytes = 0;
  for (const auto &e : h.strs) need_bytes += e.first.size();
  *is_bytes = h.kind == kByteValues ? 1 : 0;
  TGX_TRY(counted_entries_sizes(h.distinct(), need_bytes, entries, cap, n_entries, bytes, bytes_cap, n_bytes, err));
  if (!entries) return TGX_OK;
  size_t i = 0;
  uint64_t at = 0;
  for (const auto &e : h.ints) entries[i++] = tgx_value_count_entry{e.first, 0, 0, e.second};
  for (const auto &e : h.strs) {
    if (!e.first.empty()) memcpy(bytes + at, e.first.data(), e.first.size());
    entries[i++] = tgx_value_count_entry{0, at, (uint64_t)e.first.size(), e.second};
    at += e.first.size();
  }
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
