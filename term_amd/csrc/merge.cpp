// merge.cpp -- tgx_merge: folds partial states of one plan into another, every aggregate kind (scan, count,
// co-moments, HyperLogLog, exact key sets, KLL, regex, the kinds of side_check.h).  Split off distinct_state.cpp.
#include "api_internal.h"

extern "C" tgx_status tgx_merge(const tgx_plan *plan, tgx_state *dst, tgx_state *const *srcs, size_t n_srcs,
                                tgx_error *err) try {
  bind_thread();
  if (!plan || !dst || dst->plan != plan) return fail(err, TGX_INVALID_ARGUMENT, "dst does not belong to plan");
  TGX_TRY(coalesce_flush(dst, err));
  {  // what can refuse a source is checked for ALL sources before dst takes anything of any of them
    std::vector<int> mode(dst->hll_mode.begin(), dst->hll_mode.end());
    for (size_t i = 0; i < n_srcs; i++) {
      tgx_state *src = srcs ? srcs[i] : nullptr;
      if (!src || src->plan != plan) return fail(err, TGX_INVALID_ARGUMENT, "src %zu does not belong to plan", i);
      if (src == dst) return fail(err, TGX_INVALID_ARGUMENT, "src %zu is dst", i);
      TGX_TRY(spearman_check_mergeable(src, err));
      TGX_TRY(timegap_check_mergeable(src, "tgx_merge", err));
      TGX_TRY(coalesce_flush(src, err));  // (its noted batches decide which form an APPROX_DISTINCT task takes)
      for (size_t k = 0; k < plan->hll.size(); k++) {
        if (src->hll_mode[k] == 0) continue;
        if (mode[k] == 0) mode[k] = src->hll_mode[k];
        if (mode[k] != src->hll_mode[k])
          return fail(err, TGX_INVALID_ARGUMENT,
                      "APPROX_DISTINCT task %zu: one state holds registers, the other a key set (src %zu); nothing was merged",
                      k, i);
      }
    }
  }
  for (size_t i = 0; i < n_srcs; i++) {
    tgx_state *src = srcs[i];
    Gathered g;
    TGX_TRY(gather(src, &g, err));  // the fixed-size parts; the key sets are united set-wise below
    for (size_t k = 0; k < g.scan.size(); k++) scan_acc_merge(dst->h_scan[k], g.scan[k]);
    for (size_t k = 0; k < g.count.size(); k++) {
      dst->h_count[k].total += g.count[k].total;
      dst->h_count[k].non_null += g.count[k].non_null;
    }
    for (size_t k = 0; k < g.como.size(); k++) como_acc_merge(dst->h_como[k], g.como[k]);
    for (size_t k = 0; k < plan->hll.size(); k++) {
      if (src->hll_mode[k] == 0) continue;
      if (dst->hll_mode[k] == 0) dst->hll_mode[k] = src->hll_mode[k];
      if (dst->hll_mode[k] != src->hll_mode[k])
        return fail(err, TGX_INVALID_ARGUMENT, "APPROX_DISTINCT task %zu: one state holds registers, the other a key set", k);
      if (g.hll[k].empty()) continue;
      std::vector<uint8_t> &out = dst->h_hll[k];
      if (out.empty()) {
        out = g.hll[k];
      } else {
        for (int r = 0; r < kHllRegisters; r++) out[r] = std::max(out[r], g.hll[k][r]);
      }
    }
    for (size_t k = 0; k < plan->distinct.size(); k++) {
      DistinctState &s = src->distinct[k];
      DistinctState &d = dst->distinct[k];
      if (s.partitioned || !has_key_set(s)) {
        // owner-partitioned (or count-only) partial: key sets are disjoint by construction
        if (has_key_set(s) && !s.partitioned)
          return fail(err, TGX_INTERNAL, "distinct merge: unexpected state");
        distinct_fold_totals(d, g.distinct[k]);
        if (s.partitioned) d.partitioned = true;
      } else {
        // exact set union on the device
        TGX_TRY(need_device(err));
        const void *recs = nullptr;
        uint64_t cnt = 0;
        TGX_TRY(distinct_export_impl(src, k, 1, &recs, &cnt, err));
        TGX_TRY(state_init_device(dst, err));
        TGX_TRY(distinct_import_records(dst, k, recs, cnt, s.wide, err));
        HIP_TRY(hipStreamSynchronize(dst->stream));
        d.h_total += (uint64_t)s.total_rows + s.h_total;
        unsigned long long c[kNumDistinctCounters];
        TGX_TRY(distinct_read_counters(src, s, c, err));
        d.h_non_null += c[kCntValidRows] + s.h_non_null;
        d.h_distinct += s.h_distinct;
        d.h_twice += s.h_twice;
        d.h_empty_rows += s.h_empty_rows;
      }
    }
    TGX_TRY(kll_merge_states(dst, src, err));
    TGX_TRY(regex_merge_states(dst, src, err));
    for (auto &side : dst->side)
      if (side) TGX_TRY(side->merge_from(dst, src, err));
  }
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
