// typeclass_device.cpp -- TGX_CHECK_TYPE_CLASSES: the syntactic classes of a string column's values, the per-row CASE
// behind the reference's DataTypeAnalyzer (TG/analyzers/advanced/data_type.rs:129-150; include/tgx.h has the classes'
// grammar, kernels/typeclass_lex.h the one lexer that the kernels, the host entry point and the fuzzer compile).
//
// A task is one COLUMN: the specs that name it share the task and its walk.  Its running state on the device is eight
// 64-bit counters folded by kernels/typeclass.hip -- the seven classes and the non-NULL rows; rows seen are counted on
// the host.  What is merged in from other states or read from a blob is kept on the host and added when the state is
// read.  String layouts go through one launch of up to eight tasks; a dictionary column counts its indices per entry
// first and classifies each used entry once (cells of its own per task, grown as the dictionaries grow).
#include "api_internal.h"
#include "counted_state.h"
#include "kernels/typeclass_types.h"

namespace tgx {
void launch_type_classes(const TypeClassLaunch &L, int n_tasks, int64_t length, hipStream_t stream);
void launch_type_classes_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                              const Utf8ColDesc &dict, unsigned long long *cells, unsigned long long *out,
                              hipStream_t stream);

namespace {

static_assert(kMaxTypeClassPerLaunch == kSidePerLaunch, "the launch descriptor holds kSidePerLaunch tasks");

// one task's state as the host sees it
struct ClassesHost {
  uint64_t seen = 0, non_null = 0, classes[kTypeClassCount] = {};
};

struct NoRange {};

struct ClassesKind {
  typedef TypeClassesTask Task;
  typedef ClassesHost Host;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_TYPE_CLASSES;
  static constexpr const char *kDiffers = nullptr;  // (every host has the one shape)
  static constexpr uint32_t kMagic = 0x534c4354;    // "TCLS"

  static const std::vector<TypeClassesTask> &tasks(const tgx_plan *plan) { return plan->type_classes; }
  static size_t words(const TypeClassesTask &) { return kTypeClassWords; }
  static NoRange range_identity() { return NoRange(); }
  static ClassesHost fresh(const TypeClassesTask &) { return ClassesHost(); }
  static size_t shape(const ClassesHost &) { return 0; }
  static ClassesHost from_device(const TypeClassesTask &, int64_t rows, const NoRange &, const unsigned long long *w) {
    ClassesHost d;
    d.seen = (uint64_t)rows;
    d.non_null = w[kTcNonNull];
    for (int c = 0; c < kTypeClassCount; c++) d.classes[c] = w[c];
    return d;
  }
  static void merge_host(ClassesHost &a, const ClassesHost &b) {
    a.seen += b.seen;
    a.non_null += b.non_null;
    for (int c = 0; c < kTypeClassCount; c++) a.classes[c] += b.classes[c];
  }

  // per task { u64 seen, non_null, boolean, integer, double, date, datetime, string, undecided }
  static void write(const TypeClassesTask &, const ClassesHost &h, Writer &w) {
    w.pod(h.seen);
    w.pod(h.non_null);
    w.pod(h.classes);
  }

  static tgx_status read(const TypeClassesTask &, ClassesHost &h, Reader &r, size_t k, tgx_error *err) {
    uint64_t counts[2 + kTypeClassCount];
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    // the classes make up the non-NULL rows, which are rows seen (no sum may wrap on the way)
    uint64_t left = counts[1];
    bool exact = counts[1] <= counts[0];
    for (int c = 0; c < kTypeClassCount && exact; c++) {
      exact = counts[2 + c] <= left;
      left -= counts[2 + c];
    }
    if (!exact || left != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (TYPE_CLASSES task %zu: the classes do not add up to non_null <= seen)", k);
    h.seen = counts[0];
    h.non_null = counts[1];
    for (int c = 0; c < kTypeClassCount; c++) h.classes[c] = counts[2 + c];
    return TGX_OK;
  }
};

struct ClassesCheck final : SideState<ClassesKind> {
  std::vector<DevBuf> cells;  // per task: the dictionary route's per-entry row counts

  explicit ClassesCheck(const tgx_plan *plan) : SideState(plan), cells(plan->type_classes.size()) {}

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    const std::vector<TypeClassesTask> &tasks = plan->type_classes;
    if (nrows <= 0) return TGX_OK;
    for (const TypeClassesTask &t : tasks)  // (update_validate has asked check_column of every column of the batch)
      if (!is_any_string(dev[t.column].type) && dev[t.column].type != TGX_DICT32_UTF8)
        return fail(err, TGX_UNSUPPORTED, "TYPE_CLASSES takes string columns (%d)", dev[t.column].type);
    TGX_TRY(device_init(st, err));
    // (a lane's and a wave's counters are 32-bit: the string launch takes up to 2048 workgroups, the dictionary's
    //  index count 1024)
    TGX_TRY(side_rows_fit("TYPE_CLASSES", nrows, 1024, err));
    unsigned long long *counts = d_counts.as<unsigned long long>();
    // the dictionary columns, a task at a time
    for (size_t k = 0; k < tasks.size(); k++) {
      const tgx_column &x = dev[tasks[k].column];
      if (x.type != TGX_DICT32_UTF8) continue;
      const tgx_column *dc = x.dictionary;
      if (!dc || !is_string(dc->type)) return fail(err, TGX_INVALID_ARGUMENT, "TYPE_CLASSES: malformed dictionary");
      if (dc->length > 0) {  // (without entries every row is a row without a value)
        const size_t bytes = (size_t)dc->length * 8;
        HIP_TRY(cells[k].reserve_roomy(bytes));
        HIP_TRY(hipMemsetAsync(cells[k].p, 0, bytes, st->stream));
        ProfScope ps(st, "type_classes", (uint64_t)x.length * 4);
        launch_type_classes_dict((const int32_t *)x.values, x.validity, x.offset, x.length,
                                 string_desc(*dc, nullptr, plan->fp_key), cells[k].as<unsigned long long>(),
                                 counts + word_off[k], st->stream);
        HIP_TRY(hipGetLastError());
      }
      device_rows[k] += nrows;
    }
    // the string layouts, up to kSidePerLaunch tasks a launch
    auto launch = [&](const int *slots, int n) -> tgx_status {
      TypeClassLaunch L;
      memset(&L, 0, sizeof(L));
      L.counts = counts;
      for (int g = 0; g < n; g++) {
        const tgx_column &x = dev[tasks[slots[g]].column];
        L.cols[g] = string_desc(x, x.variadic, plan->fp_key);
        L.word[g] = (uint32_t)word_off[slots[g]];
      }
      ProfScope ps(st, "type_classes", 0);
      launch_type_classes(L, n, nrows, st->stream);
      HIP_TRY(hipGetLastError());
      for (int g = 0; g < n; g++) device_rows[slots[g]] += nrows;  // (only rows the device was given)
      return TGX_OK;
    };
    return side_launches(tasks, [&](const TypeClassesTask &t) { return is_any_string(dev[t.column].type); }, launch);
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    std::vector<ClassesHost> g;
    TGX_TRY(gather(st, &g, err));
    r->total = (int64_t)g[slot].seen;
    r->non_null = (int64_t)g[slot].non_null;
    return TGX_OK;
  }
};

}  // namespace

tgx_status typeclasses_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 != -1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: TYPE_CLASSES reads one column: column2 must be -1 (%d)", spec_index,
                sp.column2);
  for (size_t k = 0; k < plan->type_classes.size(); k++)
    if (plan->type_classes[k].column == sp.column) {  // the column's task
      *slot = (int)k;
      return TGX_OK;
    }
  plan->type_classes.push_back({sp.column, spec_index});
  *slot = (int)plan->type_classes.size() - 1;
  return TGX_OK;
}

void typeclasses_mark_columns(tgx_plan *plan) {
  for (const TypeClassesTask &t : plan->type_classes) side_mark(plan, ClassesCheck::kIndex, t.column, false);
}

tgx_status typeclasses_check_column(const tgx_plan *, int column, const tgx_column &c, tgx_error *err) {
  if (!is_any_string(c.type) && c.type != TGX_DICT32_UTF8)
    return fail(err, TGX_UNSUPPORTED,
                "column %d: TYPE_CLASSES takes Utf8, LargeUtf8, Utf8View and Dictionary<Int32, Utf8> columns (type %d)",
                column, c.type);
  return TGX_OK;
}

SideCheck *typeclasses_state_new(const tgx_plan *plan) {
  return plan->type_classes.empty() ? nullptr : new ClassesCheck(plan);
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_type_classes_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                           tgx_type_classes_counts *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_TYPE_CLASSES, "TYPE_CLASSES", &slot, err, "bad arguments"));
  std::vector<ClassesHost> g;
  TGX_TRY(ClassesCheck::of(st)->gather(st, &g, err));
  const ClassesHost &h = g[slot];
  out->seen = h.seen;
  out->non_null = h.non_null;
  out->boolean_rows = h.classes[kTcBoolean];
  out->integer_rows = h.classes[kTcInteger];
  out->double_rows = h.classes[kTcDouble];
  out->date_rows = h.classes[kTcDate];
  out->datetime_rows = h.classes[kTcDatetime];
  out->string_rows = h.classes[kTcString];
  out->undecided_rows = h.classes[kTcUndecided];
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
