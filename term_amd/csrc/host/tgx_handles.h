// tgx_handles.h -- what the host layer's files share when they drive the C ABI themselves (the suite runner, the
// analyzer runner, and the constraints that walk their own tables: foreign_key, join_coverage, cross_table_sum).
#pragma once
#include <string.h>

#include <string>

#include "../../../include/tgx.h"

namespace term_guard {

// a plan and its state, destroyed in that order's reverse
struct Handles {
  tgx_plan *plan = nullptr;
  tgx_state *state = nullptr;
  Handles() = default;
  Handles(const Handles &) = delete;
  Handles &operator=(const Handles &) = delete;
  void reset() {
    if (state) tgx_state_destroy(state);
    if (plan) tgx_plan_destroy(plan);
    state = nullptr;
    plan = nullptr;
  }
  ~Handles() { reset(); }
};

// the Arrow name of a column type that TGX_CHECK_KEY_PROBE's integer path does not take, or null
inline const char *off_path_type(int type) {
  switch (type) {
    case TGX_FLOAT64: return "Float64";
    case TGX_FLOAT32: return "Float32";
    case TGX_UINT64: return "UInt64";
    case TGX_BOOL: return "Boolean";
    case TGX_UTF8: return "Utf8";
    case TGX_LARGE_UTF8: return "LargeUtf8";
    case TGX_UTF8_VIEW: return "Utf8View";
    case TGX_DICT32_UTF8: return "Dictionary<Int32, Utf8>";
    default: return nullptr;
  }
}

// The tgx_error of a run of ABI calls and what a failed one becomes: check(tgx_..(.., &check.err)) hands
// "<status name>: <message>" to `failed`, which throws the caller's "query failed" error
struct Checker {
  tgx_error err;
  void (*failed)(const std::string &why);
  explicit Checker(void (*failed_)(const std::string &)) : failed(failed_) { memset(&err, 0, sizeof(err)); }
  void operator()(tgx_status s) const {
    if (s != TGX_OK) failed(std::string(tgx_status_name(s)) + ": " + err.msg);
  }
};

}  // namespace term_guard
