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
//
// keyed_state.h has what the kind shares with GROUP_COUNTS and GROUP_SUMS; here are its payload (a bare count), its
// counters and its launches.
#include "keyed_state.h"

namespace tgx {
void launch_value_counts_i64(const ComomentColDesc &d, const ValueCountsTable &t, int blocks, hipStream_t stream);
void launch_value_counts_utf8(const Utf8ColDesc &d, const ValueCountsTable &t, hipStream_t stream);
void launch_value_counts_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, unsigned long long *cells, const ValueCountsTable &t,
                              hipStream_t stream);

namespace {

// one task's state as the host sees it
struct CountsHost : KeyedEntries<uint64_t> {
  uint64_t seen = 0, non_null = 0, overflow_rows = 0, long_rows = 0;
};

struct NoRange {};

struct CountsKind {
  typedef ValueCountsTask Task;
  typedef CountsHost Host;
  typedef uint64_t Payload;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_VALUE_COUNTS;
  static constexpr const char *kDiffers = "column types";
  static constexpr const char *kNoun = "value";
  static constexpr const char *kColumn = "the column";
  static constexpr uint32_t kMagic = 0x544e4356;  // "VCNT"

  static const std::vector<ValueCountsTask> &tasks(const tgx_plan *plan) { return plan->value_counts; }
  static size_t words(const ValueCountsTask &) { return kValueCountsWords; }
  static uint32_t bound(const ValueCountsTask &t) { return t.params.max_distinct; }
  static uint32_t max_value_bytes(const ValueCountsTask &t) { return t.params.max_value_bytes; }
  static NoRange range_identity() { return NoRange(); }
  static CountsHost fresh(const ValueCountsTask &) { return CountsHost(); }
  static size_t shape(const CountsHost &) { return 0; }  // (integer against string values: KeyedCheck::merge_from)
  // the counters; the table's entries follow in gather_extra
  static CountsHost from_device(const ValueCountsTask &, int64_t rows, const NoRange &, const unsigned long long *w) {
    CountsHost d;
    d.seen = (uint64_t)rows;
    d.non_null = w[kVcNonNull];
    d.overflow_rows = w[kVcOverflow];
    d.long_rows = w[kVcLong];
    if (w[kVcMarker]) {
      d.kind = kIntKeys;
      d.ints[(int64_t)kEmptyKey] = w[kVcMarker];
    }
    return d;
  }
  static void merge_host(CountsHost &a, const CountsHost &b) {
    a.seen += b.seen;
    a.non_null += b.non_null;
    a.overflow_rows += b.overflow_rows;
    a.long_rows += b.long_rows;
    a.add_entries(b);
  }

  // per task { u32 max_distinct, max_value_bytes (the plan's parameters), u32 kind (0 no values, 1 int64, 2 bytes), u32 0,
  //   u64 seen, non_null, overflow_rows, long_rows, u64 n_entries,
  //   n_entries x { i64 value, u64 count }  or  { u32 length, u8 bytes[length], u64 count }, ascending by value }
  static void write(const ValueCountsTask &t, const CountsHost &h, Writer &w) {
    w.pod(t.params);
    w.pod((uint32_t)h.kind);
    w.pod((uint32_t)0);
    const uint64_t counts[5] = {h.seen, h.non_null, h.overflow_rows, h.long_rows, h.size()};
    w.pod(counts);
    keyed_write_entries(h, CountWire(), w);
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
    if (kind > kByteKeys || pad != 0 || (kind == kNoKeys && n != 0))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (VALUE_COUNTS task %zu: kind)", k);
    uint64_t counted = 0;
    TGX_TRY(keyed_read_entries("VALUE_COUNTS", kNoun, k, r, kind, n, t.params.max_value_bytes, CountWire(), h, &counted,
                               err));
    if (!r.ok) return TGX_OK;
    // counted + overflow_rows + long_rows == non_null <= seen
    const uint64_t non_null = counts[1];
    if (non_null > counts[0] || !terms_make(non_null, {counted, counts[2], counts[3]}))
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

struct CountsCheck final : KeyedCheck<CountsKind> {
  explicit CountsCheck(const tgx_plan *plan) : KeyedCheck(plan) {}

  ValueCountsTable view(const tgx_state *st, size_t k) const {
    ValueCountsTable t;
    fill_view(st, k, t);
    t.counts = (unsigned long long *)(table[k].buf.as<uint8_t>() + table[k].counts_at());
    t.words = d_counts.as<unsigned long long>() + word_off[k];
    return t;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    for (size_t k = 0; k < tasks.size(); k++) {
      const tgx_column &x = dev[tasks[k].column];
      const Route route = route_of(x);
      // (an Int64 view: update_validate refuses what is neither a string layout nor widened to one)
      if (route == kNoRoute)
        return fail(err, TGX_UNSUPPORTED, "VALUE_COUNTS takes integer and string columns (%d)", x.type);
      TGX_TRY(ensure_keys(st, k, route == kIntRoute ? kIntKeys : kByteKeys, 0, err));
      const ValueCountsTable t = view(st, k);
      if (route == kIntRoute) {
        ComomentColDesc d;
        memset(&d, 0, sizeof(d));
        const uint64_t bytes = side_fill_x(d, x);
        // 16 waves a workgroup and 96 KiB of LDS: one workgroup a CU
        const int blocks = side_blocks(nrows, kValueCountsBlock, g_ctx.n_cu, 1, 1);
        TGX_TRY(side_rows_fit("VALUE_COUNTS", nrows, blocks, err));
        ProfScope ps(st, "value_counts", bytes);
        launch_value_counts_i64(d, t, blocks, st->stream);
      } else if (route == kStringRoute) {
        // (per-lane and LDS counters are 32-bit here too: the launchers take up to 2048 workgroups, 1024 for the
        //  dictionary's indices, so a batch would need 2^42 rows to wrap one; refused all the same)
        TGX_TRY(side_rows_fit("VALUE_COUNTS", nrows, 1024, err));
        ProfScope ps(st, "value_counts", 0);
        launch_value_counts_utf8(string_desc(x, x.variadic, plan->fp_key), t, st->stream);
      } else {
        const tgx_column *dc;
        TGX_TRY(dictionary_of(x, &dc, err));
        TGX_TRY(side_rows_fit("VALUE_COUNTS", nrows, 1024, err));
        if (dc->length > 0) {  // (without entries every row is a row without a value)
          unsigned long long *cells;
          TGX_TRY(clear_cells(st, k, (size_t)dc->length * 8, &cells, err));
          ProfScope ps(st, "value_counts", (uint64_t)x.length * 4);
          launch_value_counts_dict((const int32_t *)x.values, x.validity, x.offset, x.length,
                                   string_desc(*dc, nullptr, plan->fp_key), cells, t, st->stream);
        }
      }
      HIP_TRY(hipGetLastError());
      device_rows[k] += nrows;
    }
    return TGX_OK;
  }

  uint64_t slot_payload(size_t, const uint8_t *, uint64_t, uint64_t count) const override { return count; }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    CountsHost h;
    TGX_TRY(read_task(st, (size_t)slot, &h, err));
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)h.non_null;
    r->distinct = (int64_t)h.size();
    r->matches = (int64_t)h.counted();
    return TGX_OK;
  }
};

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
  if (refused_as_key(c.type))
    return fail(err, TGX_UNSUPPORTED, "column %d: VALUE_COUNTS takes integer and string columns, not %s (type %d)", column,
                type_name(c.type), c.type);
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
  CountsHost h;
  TGX_TRY(CountsCheck::read_spec(plan, st, spec_index, &h, err));
  out->seen = h.seen;
  out->non_null = h.non_null;
  out->distinct = h.size();
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
  CountsHost h;
  TGX_TRY(CountsCheck::read_spec(plan, st, spec_index, &h, err));
  return keyed_entries_out(h, entries, cap, n_entries, bytes, bytes_cap, n_bytes, is_bytes,
                           [](int64_t key, uint64_t at, uint64_t length, uint64_t count) {
                             return tgx_value_count_entry{key, at, length, count};
                           }, err);
} catch (...) {
  return tgx::abi_exception(err);
}
