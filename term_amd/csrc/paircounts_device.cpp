// paircounts_device.cpp -- TGX_CHECK_PAIR_COUNTS: how often each pair of cells of two columns occurs, for a bounded number
// of distinct pairs (the GROUP BY behind the three categorical branches of the reference's MutualInformationAnalyzer,
// TG/analyzers/advanced/mutual_information.rs:249-293; include/tgx.h has the exact semantics).
//
// A task is one spec.  In its count phase its running state on the device is kPairCountsWords 64-bit counters and one
// open-addressing table filled by kernels/paircounts.hip: the pair's two fingerprint words, its count and, per side, the
// value's length and bytes or its bin index.  The table is allocated at the task's first batch.  In its range phase (one
// side is TGX_PAIR_SIDE_RANGE) the running state is a PairRangeAcc.  The host part is a map from (x cell, y cell) to
// count plus the counters and the range: what was merged in or read from a blob, and what the device part is folded
// into whenever the state is read (gather_extra) -- so merges, blobs and the cross-rank step unite by VALUE, never by
// fingerprint.  Rows seen are counted on the host.
#include <map>
#include <string>
#include <utility>

#include "api_internal.h"
#include "counted_state.h"

namespace tgx {
void launch_pair_counts(const PairSide &x, const PairSide &y, const PairCountsTable &t, int64_t length,
                        const FpKey &key, hipStream_t stream);
void launch_pair_side_range(const PairSide &num, const PairSide &other, int64_t length, PairRangeAcc *acc,
                            hipStream_t stream);

namespace {

// a cell: a binned side's index (bytes empty) or a string side's bytes (bin 0); a task's sides never change their mode,
// so comparing (bin, bytes) is comparing bins on a binned side and bytes on a string side (std::string compares as
// unsigned bytes, a prefix first)
typedef std::pair<int64_t, std::string> Cell;
typedef std::pair<Cell, Cell> PairKey;

bool is_range(const PairCountsTask &t) {
  return t.params.x.mode == TGX_PAIR_SIDE_RANGE || t.params.y.mode == TGX_PAIR_SIDE_RANGE;
}

// one task's state as the host sees it
struct PairsHost {
  uint64_t seen = 0, both = 0, overflow_rows = 0, long_rows = 0, non_finite = 0, out_of_range = 0;
  std::map<PairKey, uint64_t> pairs;  // ascending by (x cell, y cell)
  uint64_t n = 0;                     // range phase: rows with a finite numeric side, and their extremes
  double min = INFINITY, max = -INFINITY;
  uint64_t counted() const {
    uint64_t c = 0;
    for (const auto &e : pairs) c += e.second;
    return c;
  }
  void add_entries(const PairsHost &b) {
    for (const auto &e : b.pairs) pairs[e.first] += e.second;
  }
};

double key_to_double(long long key) {
  const int64_t bits = f64_total_key((int64_t)key);  // (its own inverse)
  double v;
  memcpy(&v, &bits, sizeof(v));
  return v;
}

struct PairsKind {
  typedef PairCountsTask Task;
  typedef PairsHost Host;
  typedef PairRangeAcc Range;
  static constexpr bool kRanged = true;
  static constexpr int kKind = TGX_CHECK_PAIR_COUNTS;
  static constexpr const char *kDiffers = "parameters";
  static constexpr uint32_t kMagic = 0x544e4350;  // "PCNT"

  static const std::vector<PairCountsTask> &tasks(const tgx_plan *plan) { return plan->pair_counts; }
  static size_t words(const PairCountsTask &t) { return is_range(t) ? 0 : kPairCountsWords; }
  static PairRangeAcc range_identity() {
    PairRangeAcc a;
    a.both = a.n = a.non_finite = 0;
    a.min_key = INT64_MAX;
    a.max_key = INT64_MIN;
    return a;
  }
  static PairsHost fresh(const PairCountsTask &) { return PairsHost(); }
  static size_t shape(const PairsHost &) { return 0; }  // (states of one plan share the parameters)
  // the counters; the table's entries follow in gather_extra
  static PairsHost from_device(const PairCountsTask &t, int64_t rows, const PairRangeAcc &range,
                               const unsigned long long *w) {
    PairsHost d;
    d.seen = (uint64_t)rows;
    if (is_range(t)) {
      d.both = (uint64_t)range.both;
      d.n = (uint64_t)range.n;
      d.non_finite = (uint64_t)range.non_finite;
      if (range.n > 0) {
        d.min = key_to_double(range.min_key);
        d.max = key_to_double(range.max_key);
      }
    } else {
      d.both = w[kPcBoth];
      d.long_rows = w[kPcLong];
      d.non_finite = w[kPcNonFinite];
      d.out_of_range = w[kPcOutOfRange];
      d.overflow_rows = w[kPcOverflow];
    }
    return d;
  }
  static void merge_host(PairsHost &a, const PairsHost &b) {
    a.seen += b.seen;
    a.both += b.both;
    a.overflow_rows += b.overflow_rows;
    a.long_rows += b.long_rows;
    a.non_finite += b.non_finite;
    a.out_of_range += b.out_of_range;
    a.n += b.n;
    a.min = std::min(a.min, b.min);
    a.max = std::max(a.max, b.max);
    a.add_entries(b);
  }

  // per task { tgx_pair_counts_params (the plan's: u32 max_pairs, max_value_bytes, per side i32 mode, u32 bins, f64
  //   origin, width), u64 seen, both_non_null, overflow_rows, long_rows, non_finite, out_of_range, n, f64 min, max,
  //   u64 n_entries, n_entries x { per side { u32 length, u8 bytes[length] } (a string side) or { i64 bin } (a binned
  //   side); u64 count }, ascending by (x cell, y cell) }
  // n, min, max: the range phase (min / max are +inf / -inf while n is 0); a range-phase task has no entries
  static void write(const PairCountsTask &t, const PairsHost &h, Writer &w) {
    w.pod(t.params);
    const uint64_t counts[7] = {h.seen, h.both, h.overflow_rows, h.long_rows, h.non_finite, h.out_of_range, h.n};
    w.pod(counts);
    const double ext[2] = {h.min, h.max};
    w.pod(ext);
    w.pod((uint64_t)h.pairs.size());
    counted_write_entries(h.pairs, CountWire(), w, [&](const PairKey &key) {
      for (int side = 0; side < 2; side++) {
        const Cell &c = side ? key.second : key.first;
        if ((side ? t.params.y.mode : t.params.x.mode) == TGX_PAIR_SIDE_VALUE) {
          w.pod((uint32_t)c.second.size());
          w.put(c.second.data(), c.second.size());
        } else {
          w.pod(c.first);
        }
      }
    });
  }

  static tgx_status read(const PairCountsTask &t, PairsHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_pair_counts_params p;
    r.get(&p, sizeof(p));
    uint64_t counts[7];
    double ext[2];
    r.get(counts, sizeof(counts));
    r.get(ext, sizeof(ext));
    const uint64_t n = r.pod<uint64_t>();
    if (!r.ok) return TGX_OK;
    if (memcmp(&p, &t.params, sizeof(p)) != 0)  // (binnings compared by their bits)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "PAIR_COUNTS task %zu: the blob was counted under other parameters (max_pairs %u, max_value_bytes %u, "
                  "modes %d / %d, bins %u / %u) than the plan's (%u, %u, %d / %d, %u / %u), or another binning",
                  k, p.max_pairs, p.max_value_bytes, p.x.mode, p.y.mode, p.x.bins, p.y.bins, t.params.max_pairs,
                  t.params.max_value_bytes, t.params.x.mode, t.params.y.mode, t.params.x.bins, t.params.y.bins);
    const uint64_t both = counts[1];
    if (is_range(t)) {
      // n + non_finite == both_non_null <= seen, nothing else counted; extremes only with rows behind them
      const bool ext_ok = counts[6] == 0 ? (ext[0] == INFINITY && ext[1] == -INFINITY)
                                         : (std::isfinite(ext[0]) && std::isfinite(ext[1]) && ext[0] <= ext[1]);
      if (n != 0 || both > counts[0] || counts[6] > both || counts[4] != both - counts[6] || counts[2] || counts[3] ||
          counts[5] || !ext_ok)
        return fail(err, TGX_INVALID_ARGUMENT,
                    "malformed state blob (PAIR_COUNTS task %zu: a range phase with n + non_finite != both_non_null, "
                    "entries, or extremes without rows)", k);
    } else {
      if (counts[6] != 0 || ext[0] != INFINITY || ext[1] != -INFINITY)
        return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (PAIR_COUNTS task %zu: a count phase with a range)", k);
      uint64_t counted = 0;
      TGX_TRY(counted_read_entries("PAIR_COUNTS", k, r, n, 8, CountWire(), h.pairs, &counted, [&](PairKey &key) {
        for (int side = 0; side < 2; side++) {
          const tgx_pair_side &m = side ? t.params.y : t.params.x;
          Cell &c = side ? key.second : key.first;
          c.first = 0;
          if (m.mode == TGX_PAIR_SIDE_VALUE) {
            const uint32_t len = r.pod<uint32_t>();
            if (!r.ok) return TGX_OK;
            if (len > t.params.max_value_bytes)
              return fail(err, TGX_INVALID_ARGUMENT,
                          "malformed state blob (PAIR_COUNTS task %zu: a value of %u bytes, max_value_bytes is %u)", k,
                          len, t.params.max_value_bytes);
            c.second.assign(len, '\0');
            r.get(&c.second[0], len);
          } else {
            c.first = r.pod<int64_t>();
            if (r.ok && (c.first < 0 || c.first > (int64_t)m.bins))
              return fail(err, TGX_INVALID_ARGUMENT,
                          "malformed state blob (PAIR_COUNTS task %zu: bin %lld lies outside [0, %u])", k,
                          (long long)c.first, m.bins);
          }
        }
        return TGX_OK;
      }, err));
      if (!r.ok) return TGX_OK;
      // counted + overflow_rows + long_rows + non_finite + out_of_range == both_non_null <= seen
      if (both > counts[0] || !terms_make(both, {counted, counts[2], counts[3], counts[4], counts[5]}))
        return fail(err, TGX_INVALID_ARGUMENT,
                    "malformed state blob (PAIR_COUNTS task %zu: counted + overflow_rows + long_rows + non_finite + "
                    "out_of_range != both_non_null)", k);
    }
    h.seen = counts[0];
    h.both = both;
    h.overflow_rows = counts[2];
    h.long_rows = counts[3];
    h.non_finite = counts[4];
    h.out_of_range = counts[5];
    h.n = counts[6];
    h.min = ext[0];
    h.max = ext[1];
    return TGX_OK;
  }
};

struct PairsCheck final : CountedState<PairsKind> {
  // a count-phase task's table (made at the first batch): two key words a slot, and behind the counts the two sides'
  // cells (a string's length or a bin index) and the byte stores of the string sides
  const std::vector<PairCountsTask> &tasks;  // (the plan's: their parameters are fixed once a state exists)

  explicit PairsCheck(const tgx_plan *plan) : CountedState(plan), tasks(plan->pair_counts) {}

  uint32_t value_bytes(size_t k) const { return tasks[k].params.max_value_bytes; }
  bool strings(size_t k, int side) const {
    return (side ? tasks[k].params.y : tasks[k].params.x).mode == TGX_PAIR_SIDE_VALUE;
  }
  size_t cell_at(size_t k, int side) const { return table[k].extra_at() + (size_t)side * table[k].slots * 4; }
  size_t store_at(size_t k, int side) const {
    return cell_at(k, 2) + (side && strings(k, 0) ? (size_t)table[k].slots * value_bytes(k) : 0);
  }

  PairCountsTable view(size_t k) const {
    uint8_t *base = table[k].buf.as<uint8_t>();
    PairCountsTable t;
    memset(&t, 0, sizeof(t));
    t.keys = (unsigned long long *)base;
    t.keys2 = t.keys + table[k].slots;
    t.counts = (unsigned long long *)(base + table[k].counts_at());
    for (int side = 0; side < 2; side++) {
      t.cell[side] = (uint32_t *)(base + cell_at(k, side));
      t.store[side] = strings(k, side) ? base + store_at(k, side) : nullptr;
    }
    t.words = d_counts.as<unsigned long long>() + word_off[k];
    t.mask = table[k].slots - 1;
    t.max_value_bytes = value_bytes(k);
    return t;
  }

  tgx_status ensure_table(tgx_state *st, size_t k, tgx_error *err) {
    if (table[k].live) return TGX_OK;
    const size_t stores = (size_t)strings(k, 0) + (size_t)strings(k, 1);
    return open_table(st, k, tasks[k].params.max_pairs, 2, 8 + stores * value_bytes(k), err);
  }

  // column `c` (a device view, widened) as side `m` of a launch
  static tgx_status fill_side(const tgx_column &c, const tgx_pair_side &m, PairSide *s, tgx_error *err) {
    memset(s, 0, sizeof(*s));
    s->validity = c.validity;
    s->offset = c.offset;
    s->mode = m.mode;
    if (m.mode == TGX_PAIR_SIDE_VALUE) {
      const tgx_column *strings = &c;
      if (c.type == TGX_DICT32_UTF8) {
        strings = c.dictionary;
        if (!strings || !is_string(strings->type)) return fail(err, TGX_INVALID_ARGUMENT, "PAIR_COUNTS: malformed dictionary");
        s->indices = (const int32_t *)c.values;
        s->dict_validity = strings->validity;
        s->dict_offset = strings->offset;
        s->dict_length = strings->length;
      } else if (!is_any_string(c.type)) {
        return fail(err, TGX_UNSUPPORTED, "PAIR_COUNTS: a TGX_PAIR_SIDE_VALUE side takes a string column (type %d)", c.type);
      }
      const bool view = strings->type == TGX_UTF8_VIEW;
      s->str_offsets = strings->offsets;
      s->str_data = strings->data;
      s->str_views = view ? strings->values : nullptr;
      s->str_buffers = view ? strings->variadic : nullptr;
      s->large_offsets = strings->type == TGX_LARGE_UTF8;
    } else {
      if (!is_numeric(c.type) || !c.values)
        return fail(err, TGX_UNSUPPORTED, "PAIR_COUNTS: a binned or range side takes a numeric column (type %d)", c.type);
      s->values = c.values;
      s->is_float = c.type == TGX_FLOAT64;
      s->origin = m.origin;
      s->width = m.width;
      s->bins = m.bins;
    }
    return TGX_OK;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    // (per-lane and LDS counters are 32-bit: the launchers take up to kPairCountsMaxBlocks workgroups)
    TGX_TRY(side_rows_fit("PAIR_COUNTS", nrows, kPairCountsMaxBlocks, err));
    for (size_t k = 0; k < plan->pair_counts.size(); k++) {
      const PairCountsTask &t = plan->pair_counts[k];
      const tgx_column &x = dev[t.col_x], &y = dev[t.col_y];
      PairSide sx, sy;
      TGX_TRY(fill_side(x, t.params.x, &sx, err));
      TGX_TRY(fill_side(y, t.params.y, &sy, err));
      if (is_range(t)) {
        const bool x_is_num = t.params.x.mode == TGX_PAIR_SIDE_RANGE;
        ProfScope ps(st, "pair_range", (uint64_t)nrows * 8);
        launch_pair_side_range(x_is_num ? sx : sy, x_is_num ? sy : sx, nrows, d_range.as<PairRangeAcc>() + k, st->stream);
      } else {
        TGX_TRY(ensure_table(st, k, err));
        ProfScope ps(st, "pair_counts", 0);
        launch_pair_counts(sx, sy, view(k), nrows, plan->fp_key, st->stream);
      }
      HIP_TRY(hipGetLastError());
      device_rows[k] += nrows;
    }
    return TGX_OK;
  }

  void decode_slot(size_t k, const uint8_t *h, uint64_t s, uint64_t count, PairsHost &o) const override {
    if (((const uint64_t *)h)[table[k].slots + s] == kEmptyKey) return;
    PairKey key;
    for (int side = 0; side < 2; side++) {
      Cell &c = side ? key.second : key.first;
      const uint32_t word = ((const uint32_t *)(h + cell_at(k, side)))[s];
      c.first = 0;
      if (strings(k, side))
        c.second.assign((const char *)h + store_at(k, side) + (size_t)s * value_bytes(k), std::min(word, value_bytes(k)));
      else
        c.first = (int64_t)word;
    }
    o.pairs[key] += count;
  }

  tgx_status read_task(tgx_state *st, size_t slot, PairsHost *out, tgx_error *err) {
    std::vector<PairsHost> g;
    TGX_TRY(gather(st, &g, err));
    *out = std::move(g[slot]);
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    PairsHost h;
    TGX_TRY(read_task(st, (size_t)slot, &h, err));
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)h.both;
    r->distinct = (int64_t)h.pairs.size();
    r->matches = (int64_t)h.counted();
    return TGX_OK;
  }
};

bool side_is_numeric(const tgx_pair_side &s) { return s.mode != TGX_PAIR_SIDE_VALUE; }

}  // namespace

tgx_status paircounts_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 < 0) return fail(err, TGX_INVALID_ARGUMENT, "spec %d: PAIR_COUNTS needs column2", spec_index);
  PairCountsTask t;
  memset(&t, 0, sizeof(t));
  t.col_x = sp.column;
  t.col_y = sp.column2;
  t.spec_index = spec_index;
  plan->pair_counts.push_back(t);
  *slot = (int)plan->pair_counts.size() - 1;
  return TGX_OK;
}

tgx_status paircounts_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const PairCountsTask &t : plan->pair_counts)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a PAIR_COUNTS check needs its parameters (tgx_plan_set_pair_counts)",
                  t.spec_index);
  return TGX_OK;
}

void paircounts_mark_columns(tgx_plan *plan) {
  for (const PairCountsTask &t : plan->pair_counts)
    for (int c : {t.col_x, t.col_y}) side_mark(plan, PairsCheck::kIndex, c, true);
}

tgx_status paircounts_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err) {
  for (const PairCountsTask &t : plan->pair_counts)
    for (int side = 0; side < 2; side++) {
      if ((side ? t.col_y : t.col_x) != column) continue;
      const tgx_pair_side &m = side ? t.params.y : t.params.x;
      if (m.mode == TGX_PAIR_SIDE_VALUE) {
        if (!is_any_string(c.type) && c.type != TGX_DICT32_UTF8)
          return fail(err, TGX_UNSUPPORTED,
                      "column %d: a TGX_PAIR_SIDE_VALUE side of PAIR_COUNTS takes Utf8, LargeUtf8, Utf8View and "
                      "Dictionary<Int32, Utf8> columns (type %d)", column, c.type);
      } else {
        if (!is_numeric(c.type) && !(is_widened(c.type) && c.type != TGX_BOOL))
          return fail(err, TGX_UNSUPPORTED,
                      "column %d: a binned or range side of PAIR_COUNTS takes the numeric columns JOINT_BINS takes, "
                      "UInt64 and Boolean excepted (type %d)", column, c.type);
        if (c.length > 0 && !c.values)
          return fail(err, TGX_UNSUPPORTED, "column %d: PAIR_COUNTS reads the values: a validity-only column has none",
                      column);
      }
    }
  return TGX_OK;
}

SideCheck *paircounts_state_new(const tgx_plan *plan) {
  return plan->pair_counts.empty() ? nullptr : new PairsCheck(plan);
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_pair_counts(tgx_plan *plan, size_t spec_index, const tgx_pair_counts_params *p,
                                               tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_PAIR_COUNTS, "PAIR_COUNTS", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the parameters of a PAIR_COUNTS check are fixed once a state of the plan exists");
  if (p->max_pairs < 1 || p->max_pairs > TGX_PAIR_COUNTS_MAX_PAIRS)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_pairs must be 1 .. %d (%u)", spec_index,
                (int)TGX_PAIR_COUNTS_MAX_PAIRS, p->max_pairs);
  if (p->max_value_bytes < 1 || p->max_value_bytes > TGX_PAIR_COUNTS_MAX_VALUE_BYTES)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_value_bytes must be 1 .. %d (%u)", spec_index,
                (int)TGX_PAIR_COUNTS_MAX_VALUE_BYTES, p->max_value_bytes);
  tgx_pair_counts_params q;
  memset(&q, 0, sizeof(q));  // (what a mode does not read stays zero: blobs compare the parameters by their bits)
  q.max_pairs = p->max_pairs;
  q.max_value_bytes = p->max_value_bytes;
  for (int side = 0; side < 2; side++) {
    const tgx_pair_side &s = side ? p->y : p->x;
    tgx_pair_side &o = side ? q.y : q.x;
    if (s.mode != TGX_PAIR_SIDE_VALUE && s.mode != TGX_PAIR_SIDE_RANGE && s.mode != TGX_PAIR_SIDE_BINNED)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: unknown mode %d of the %c side", spec_index, s.mode, side ? 'y' : 'x');
    o.mode = s.mode;
    if (s.mode != TGX_PAIR_SIDE_BINNED) continue;
    if (s.bins < 2 || s.bins > TGX_JOINT_MAX_BINS)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: bins of the %c side must be 2 .. %d (%u)", spec_index,
                  side ? 'y' : 'x', (int)TGX_JOINT_MAX_BINS, s.bins);
    if (!std::isfinite(s.origin) || !std::isfinite(s.width) || !(s.width > 0.0))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "spec %zu: the %c side's origin must be finite and its width finite and positive (a range whose "
                  "difference overflows has no bin width)", spec_index, side ? 'y' : 'x');
    o.bins = s.bins;
    o.origin = s.origin;
    o.width = s.width;
  }
  if (side_is_numeric(q.x) && side_is_numeric(q.y))
    return fail(err, TGX_INVALID_ARGUMENT,
                "spec %zu: both sides are numeric: joint bins of two numeric columns are TGX_CHECK_JOINT_BINS", spec_index);
  PairCountsTask &t = plan->pair_counts[slot];
  t.params = q;
  t.set = true;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_pair_counts_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                          tgx_pair_counts_summary *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_PAIR_COUNTS, "PAIR_COUNTS", &slot, err, "bad arguments"));
  PairsHost h;
  TGX_TRY(static_cast<PairsCheck *>(PairsCheck::of(st))->read_task(st, slot, &h, err));
  const bool range = is_range(plan->pair_counts[slot]);
  out->seen = h.seen;
  out->both_non_null = h.both;
  out->distinct = h.pairs.size();
  out->counted = h.counted();
  out->overflow_rows = h.overflow_rows;
  out->long_rows = h.long_rows;
  out->non_finite = range ? 0 : h.non_finite;
  out->out_of_range = h.out_of_range;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_pair_range_get(const tgx_plan *plan, tgx_state *st, size_t spec_index, tgx_pair_range *out,
                                         tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_PAIR_COUNTS, "PAIR_COUNTS", &slot, err, "bad arguments"));
  if (!is_range(plan->pair_counts[slot]))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu is in its count phase: neither side is TGX_PAIR_SIDE_RANGE", spec_index);
  PairsHost h;
  TGX_TRY(static_cast<PairsCheck *>(PairsCheck::of(st))->read_task(st, slot, &h, err));
  out->seen = h.seen;
  out->both_non_null = h.both;
  out->n = h.n;
  out->non_finite = h.non_finite;
  out->min = h.n > 0 ? h.min : NAN;
  out->max = h.n > 0 ? h.max : NAN;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_pair_counts_entries(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                              tgx_pair_count_entry *entries, uint64_t cap, uint64_t *n_entries,
                                              uint8_t *bytes, uint64_t bytes_cap, uint64_t *n_bytes, tgx_error *err) try {
  bind_thread();
  if (!n_entries || !n_bytes) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_PAIR_COUNTS, "PAIR_COUNTS", &slot, err, "bad arguments"));
  PairsHost h;
  TGX_TRY(static_cast<PairsCheck *>(PairsCheck::of(st))->read_task(st, slot, &h, err));
  uint64_t need_bytes = 0;
  for (const auto &e : h.pairs) need_bytes += e.first.first.second.size() + e.first.second.second.size();
  TGX_TRY(counted_entries_sizes(h.pairs.size(), need_bytes, entries, cap, n_entries, bytes, bytes_cap, n_bytes, err));
  if (!entries) return TGX_OK;
  size_t i = 0;
  uint64_t at = 0;
  for (const auto &e : h.pairs) {
    const Cell &x = e.first.first, &y = e.first.second;
    tgx_pair_count_entry o;
    memset(&o, 0, sizeof(o));
    o.x_bin = x.first;
    o.y_bin = y.first;
    if (!x.second.empty()) memcpy(bytes + at, x.second.data(), x.second.size());
    o.x_offset = x.second.empty() ? 0 : at;
    o.x_length = x.second.size();
    at += x.second.size();
    if (!y.second.empty()) memcpy(bytes + at, y.second.data(), y.second.size());
    o.y_offset = y.second.empty() ? 0 : at;
    o.y_length = y.second.size();
    at += y.second.size();
    o.count = e.second;
    entries[i++] = o;
  }
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
