// jointbins_device.cpp -- TGX_CHECK_JOINT_BINS: the joint bin counts behind MutualInformationAnalyzer's numeric x
// numeric branch (TG/analyzers/advanced/mutual_information.rs:143-248), in two phases (include/tgx.h).
//
// A task is one spec.  Its running state lives on the device -- a JointRangeAcc in the range phase, (bins + 1)^2 + 2
// 64-bit counters in the count phase (the cells, the rows outside [0, bins], the non-finite rows) -- and is folded by
// kernels/jointbins.hip; rows seen are counted on the host.  What is merged in from other states or read from a blob
// is kept on the host and added when the state is read: extremes by MIN / MAX, everything else by addition.
#include "api_internal.h"

namespace tgx {
void launch_pair_range(const JointLaunch &L, int n_pairs, int blocks_per_pair, JointRangeAcc *d_partials,
                       JointRangeAcc *d_accs, hipStream_t stream);
void launch_joint_bins(const JointLaunch &L, int n_pairs, int blocks_per_pair, size_t lds_bytes, hipStream_t stream);

namespace {

// one task's state as the host sees it
struct JointHost {
  int64_t total = 0;
  JointRangeAcc range;          // count phase: n and non_finite only
  std::vector<uint64_t> words;  // count phase: the cells, then the rows outside [0, bins]
};

struct JointKind {
  typedef JointTask Task;
  typedef JointHost Host;
  typedef JointRangeAcc Range;
  static constexpr bool kRanged = true;
  static constexpr int kKind = TGX_CHECK_JOINT_BINS;
  static constexpr const char *kDiffers = "binnings";
  static constexpr uint32_t kMagic = 0x42544e4a;  // "JNTB"

  static const std::vector<JointTask> &tasks(const tgx_plan *plan) { return plan->joint; }
  static size_t words(const JointTask &t) { return t.binned ? (size_t)joint_cells(t.binning.bins) + 2 : 0; }
  static JointRangeAcc range_identity() {
    JointRangeAcc a;
    a.n = a.non_finite = 0;
    a.x_min = a.y_min = INFINITY;
    a.x_max = a.y_max = -INFINITY;
    return a;
  }
  static JointHost fresh(const JointTask &t) {
    JointHost h;
    h.range = range_identity();
    if (t.binned) h.words.assign(joint_cells(t.binning.bins) + 1, 0);
    return h;
  }
  static size_t shape(const JointHost &h) { return h.words.size(); }

  static JointHost from_device(const JointTask &t, int64_t rows, const JointRangeAcc &range,
                               const unsigned long long *w) {
    JointHost d = fresh(t);
    d.total = rows;
    if (!t.binned) {
      d.range = range;
    } else {
      const size_t cells = joint_cells(t.binning.bins);
      d.words.assign(w, w + cells + 1);
      for (size_t c = 0; c < cells; c++) d.range.n += (int64_t)w[c];
      d.range.non_finite = (int64_t)w[cells + 1];
    }
    return d;
  }

  static void merge_host(JointHost &a, const JointHost &b) {
    a.total += b.total;
    a.range.n += b.range.n;
    a.range.non_finite += b.range.non_finite;
    a.range.x_min = std::min(a.range.x_min, b.range.x_min);
    a.range.x_max = std::max(a.range.x_max, b.range.x_max);
    a.range.y_min = std::min(a.range.y_min, b.range.y_min);
    a.range.y_max = std::max(a.range.y_max, b.range.y_max);
    for (size_t i = 0; i < a.words.size() && i < b.words.size(); i++) a.words[i] += b.words[i];
  }

  // per task { u32 binned, u32 bins, f64 x_origin, x_width, y_origin, y_width, i64 total, n, non_finite,
  //   f64 x_min, x_max, y_min, y_max, u64 n_words, u64 words[n_words] }
  // n_words = (bins + 1)^2 + 1 in the count phase (the cells, row-major, then the rows outside [0, bins]), else 0
  static void write(const JointTask &t, const JointHost &h, Writer &w) {
    const uint32_t phase[2] = {t.binned ? 1u : 0u, t.binning.bins};
    w.pod(phase);
    const double edges[4] = {t.binning.x_origin, t.binning.x_width, t.binning.y_origin, t.binning.y_width};
    w.pod(edges);
    const int64_t counts[3] = {h.total, h.range.n, h.range.non_finite};
    w.pod(counts);
    const double ext[4] = {h.range.x_min, h.range.x_max, h.range.y_min, h.range.y_max};
    w.pod(ext);
    w.pod((uint64_t)h.words.size());
    w.put(h.words.data(), h.words.size() * sizeof(uint64_t));
  }

  static tgx_status read(const JointTask &t, JointHost &h, Reader &r, size_t k, tgx_error *err) {
    uint32_t phase[2];
    double edges[4], ext[4];
    int64_t counts[3];
    r.get(phase, sizeof(phase));
    r.get(edges, sizeof(edges));
    r.get(counts, sizeof(counts));
    r.get(ext, sizeof(ext));
    const uint64_t n_words = r.pod<uint64_t>();
    if (!r.ok) return TGX_OK;
    const double mine[4] = {t.binning.x_origin, t.binning.x_width, t.binning.y_origin, t.binning.y_width};
    if (phase[0] != (t.binned ? 1u : 0u) || phase[1] != t.binning.bins || memcmp(edges, mine, sizeof(mine)) != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "JOINT_BINS task %zu: the blob was counted under another binning (bins %u) than the plan's (bins %u)", k,
                  phase[1], t.binning.bins);
    size_t bytes = 0;
    if (n_words != h.words.size() || !r.fits(n_words, sizeof(uint64_t), &bytes))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (JOINT_BINS task %zu)", k);
    h.total = counts[0];
    h.range.n = counts[1];
    h.range.non_finite = counts[2];
    h.range.x_min = ext[0];
    h.range.x_max = ext[1];
    h.range.y_min = ext[2];
    h.range.y_max = ext[3];
    r.get(h.words.data(), bytes);
    return TGX_OK;
  }
};

struct JointCheck final : SideState<JointKind> {
  using SideState::SideState;

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    for (int phase = 0; phase < 2; phase++) {
      auto launch = [&](const int *slots, int n) -> tgx_status {
        JointLaunch L;
        memset(&L, 0, sizeof(L));
        uint64_t bytes = 0;
        uint32_t max_cells = 0;
        for (int k = 0; k < n; k++) {
          const int slot = slots[k];
          const JointTask &t = plan->joint[slot];
          const tgx_column &x = dev[t.col_x], &y = dev[t.col_y];
          if (!is_numeric(x.type) || !is_numeric(y.type))
            return fail(err, TGX_UNSUPPORTED, "JOINT_BINS takes numeric columns (%d, %d)", x.type, y.type);
          bytes += side_fill_x(L.pairs[k], x) + side_fill_y(L.pairs[k], y);
          L.binning[k] = t.binning;
          L.counters[k] = t.binned ? d_counts.as<unsigned long long>() + word_off[slot] : nullptr;
          L.acc_index[k] = slot;
          max_cells = std::max(max_cells, t.binned ? joint_cells(t.binning.bins) : 0u);
          device_rows[slot] += nrows;
        }
        // 8 waves a workgroup, up to 4 workgroups a CU; the count phase as many as its LDS counters leave room for
        const size_t lds = (size_t)max_cells * sizeof(unsigned int);
        const int per_cu = phase == 0 ? 4 : (int)std::max<size_t>(1, std::min<size_t>(4, (160u << 10) / std::max<size_t>(lds, 1)));
        const int blocks = side_blocks(nrows, kJointBlock, g_ctx.n_cu, per_cu, n);
        TGX_TRY(side_rows_fit("JOINT_BINS", nrows, blocks, err));
        (void)hipGetLastError();  // (what the launches below leave is theirs: a 64 KiB LDS request can be refused)
        if (phase == 0) {
          HIP_TRY(d_partials.reserve((size_t)n * blocks * sizeof(JointRangeAcc)));
          ProfScope ps(st, "joint_range", bytes);
          launch_pair_range(L, n, blocks, d_partials.as<JointRangeAcc>(), d_range.as<JointRangeAcc>(), st->stream);
        } else {
          ProfScope ps(st, "joint_bins", bytes);
          launch_joint_bins(L, n, blocks, lds, st->stream);
        }
        HIP_TRY(hipGetLastError());
        return TGX_OK;
      };
      TGX_TRY(side_launches(plan->joint, [&](const JointTask &t) { return (int)t.binned == phase; }, launch));
    }
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    std::vector<JointHost> g;
    TGX_TRY(gather(st, &g, err));
    r->total = g[slot].total;
    r->non_null = g[slot].range.n;
    return TGX_OK;
  }
};

}  // namespace

tgx_status joint_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 < 0) return fail(err, TGX_INVALID_ARGUMENT, "spec %d: JOINT_BINS needs column2", spec_index);
  JointTask t;
  memset(&t, 0, sizeof(t));
  t.col_x = sp.column;
  t.col_y = sp.column2;
  plan->joint.push_back(t);
  *slot = (int)plan->joint.size() - 1;
  return TGX_OK;
}

void joint_mark_columns(tgx_plan *plan) {
  for (const JointTask &t : plan->joint)
    for (int c : {t.col_x, t.col_y}) {
      side_mark(plan, JointCheck::kIndex, c, true);
      plan->stats_on[c] = 1;
    }
}

tgx_status joint_check_column(const tgx_plan *, int column, const tgx_column &c, tgx_error *err) {
  if (!is_numeric(c.type) && !is_widened(c.type))
    return fail(err, TGX_UNSUPPORTED, "column %d: JOINT_BINS takes numeric columns (type %d)", column, c.type);
  return TGX_OK;
}

SideCheck *joint_state_new(const tgx_plan *plan) { return plan->joint.empty() ? nullptr : new JointCheck(plan); }

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_joint_binning(tgx_plan *plan, size_t spec_index, const tgx_joint_binning *b,
                                                 tgx_error *err) try {
  if (!plan || !b) return fail(err, TGX_INVALID_ARGUMENT, "plan/binning is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_JOINT_BINS, "JOINT_BINS", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the binning of a JOINT_BINS check is fixed once a state of the plan exists");
  if (b->bins < 2) return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: bins must be at least 2", spec_index);
  if (b->bins > kJointMaxBins)
    return fail(err, TGX_UNSUPPORTED,
                "spec %zu: %u bins: at most %u are supported (the (bins + 1)^2 cells are counted in 64 KiB of LDS; there "
                "is no global-memory path)", spec_index, b->bins, kJointMaxBins);
  if (!std::isfinite(b->x_origin) || !std::isfinite(b->y_origin) || !std::isfinite(b->x_width) ||
      !std::isfinite(b->y_width) || !(b->x_width > 0.0) || !(b->y_width > 0.0))
    return fail(err, TGX_INVALID_ARGUMENT,
                "spec %zu: origins must be finite and widths finite and positive (a range whose difference overflows has "
                "no bin width)", spec_index);
  JointTask &t = plan->joint[slot];
  t.binned = true;
  t.binning.x_origin = b->x_origin;
  t.binning.x_width = b->x_width;
  t.binning.y_origin = b->y_origin;
  t.binning.y_width = b->y_width;
  t.binning.bins = b->bins;
  t.binning.pad = 0;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_joint_range_get(const tgx_plan *plan, tgx_state *st, size_t spec_index, tgx_joint_range *out,
                                          tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_JOINT_BINS, "JOINT_BINS", &slot, err, "bad arguments"));
  std::vector<JointHost> g;
  TGX_TRY(JointCheck::of(st)->gather(st, &g, err));
  const JointHost &h = g[slot];
  out->total = (uint64_t)h.total;
  out->n = (uint64_t)h.range.n;
  out->non_finite = (uint64_t)h.range.non_finite;
  const bool has = !plan->joint[slot].binned && h.range.n > 0;
  out->x_min = has ? h.range.x_min : NAN;
  out->x_max = has ? h.range.x_max : NAN;
  out->y_min = has ? h.range.y_min : NAN;
  out->y_max = has ? h.range.y_max : NAN;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_joint_counts(const tgx_plan *plan, tgx_state *st, size_t spec_index, uint64_t *cells,
                                       uint64_t cap, uint64_t *n_cells, uint64_t *out_of_range, tgx_error *err) try {
  bind_thread();
  if (!n_cells) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_JOINT_BINS, "JOINT_BINS", &slot, err, "bad arguments"));
  const JointTask &t = plan->joint[slot];
  if (!t.binned)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu is in its range phase: no binning was set (tgx_plan_set_joint_binning)",
                spec_index);
  const uint64_t n = joint_cells(t.binning.bins);
  *n_cells = n;
  if (!cells) return TGX_OK;
  if (cap < n) return fail(err, TGX_INVALID_ARGUMENT, "cells has room for %llu of %llu counts", (unsigned long long)cap,
                           (unsigned long long)n);
  std::vector<JointHost> g;
  TGX_TRY(JointCheck::of(st)->gather(st, &g, err));
  memcpy(cells, g[slot].words.data(), (size_t)n * sizeof(uint64_t));
  if (out_of_range) *out_of_range = g[slot].words[n];
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
