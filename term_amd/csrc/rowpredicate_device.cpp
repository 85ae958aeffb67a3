// rowpredicate_device.cpp -- TGX_CHECK_ROW_PREDICATE: the row predicates behind the reference's Check::satisfies and
// ComplianceAnalyzer (TG/constraints/custom_sql.rs:192-282, TG/analyzers/advanced/compliance.rs:136-204; include/tgx.h
// has the leaves, the program and their exact semantics).
//
// A task is one spec.  Its running state on the device is two 64-bit counters folded by kernels/rowpredicate.hip -- the
// rows on which the predicate is TRUE and those on which it is UNKNOWN; rows seen are counted on the host and the
// failed rows follow from the three.  What a leaf compares is settled here, per batch, from the type each column
// arrives in (describe); a leaf that does not fit its column refuses the batch before anything has run
// (check_column, accepts).  The launch's descriptors live in device memory (rowpredicate_types.h): they are written
// into one of two host buffers, each reused only once its upload has been waited for.
#include <math.h>

#include "api_internal.h"
#include "kernels/rowpredicate_types.h"
#include "kernels/string_leaf.h"

namespace tgx {
void launch_row_predicate(const RowPredTask *tasks, int n_tasks, bool numeric, int blocks_per_task,
                          unsigned long long *counts, hipStream_t stream);

namespace {

static_assert(kRowPredMaxLeaves == TGX_PRED_MAX_LEAVES && kRowPredMaxOps == TGX_PRED_MAX_OPS &&
                  kRowPredMaxLiteralBytes == TGX_PRED_MAX_LITERAL_BYTES && kRowPredicateMaxCols == TGX_PRED_MAX_COLUMNS &&
                  kMaxTupleCols == TGX_PRED_MAX_COLUMNS,
              "the device's limits are the ABI's");
static_assert(kRpIsNull == TGX_PRED_IS_NULL && kRpStrEq == TGX_PRED_STR_EQ && kRpEq == TGX_PRED_EQ &&
                  kRpGe == TGX_PRED_GE && kRpPush == TGX_PRED_PUSH && kRpNot == TGX_PRED_NOT &&
                  kRpStrCmp == TGX_PRED_STR_CMP && kRpStrLength == TGX_PRED_STR_LENGTH &&
                  kRpStrLike == TGX_PRED_STR_LIKE && kRpStrBlank == TGX_PRED_STR_BLANK && (int)sl::kEq == TGX_PRED_EQ &&
                  (int)sl::kGe == TGX_PRED_GE,
              "the device's codes are the ABI's");

struct PredHost {
  uint64_t seen = 0, satisfied = 0, unknown = 0;
};

int64_t key_of(double x) {
  int64_t bits;
  memcpy(&bits, &x, sizeof(bits));
  return f64_total_key(bits);
}

// what a column's Arrow type is to a leaf
enum TypeClass { kClassInt, kClassFloat, kClassString, kClassOther };
TypeClass class_of(int type) {
  if (type == TGX_FLOAT64 || type == TGX_FLOAT32) return kClassFloat;
  if (is_any_string(type) || type == TGX_DICT32_UTF8) return kClassString;
  if (type == TGX_UINT64 || type == TGX_BOOL) return kClassOther;
  return kClassInt;  // Int64, Int32 and the narrow integers
}

bool reads_values(const tgx_row_predicate_leaf &l) { return l.kind != TGX_PRED_IS_NULL; }
// a leaf that fits string layouts only (kind 5 is no kind)
bool string_leaf(int kind) { return kind == TGX_PRED_STR_EQ || (kind >= TGX_PRED_STR_CMP && kind <= TGX_PRED_STR_BLANK); }

struct NoRange {};

struct PredKind {
  typedef RowPredicateTask Task;
  typedef PredHost Host;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_ROW_PREDICATE;
  static constexpr const char *kDiffers = nullptr;  // (every host has the one shape)
  static constexpr uint32_t kMagic = 0x44505252;   // "RRPD"

  static const std::vector<RowPredicateTask> &tasks(const tgx_plan *plan) { return plan->row_predicates; }
  static size_t words(const RowPredicateTask &) { return kRowPredWords; }
  static NoRange range_identity() { return NoRange(); }
  static PredHost fresh(const RowPredicateTask &) { return PredHost(); }
  static size_t shape(const PredHost &) { return 0; }
  static PredHost from_device(const RowPredicateTask &, int64_t rows, const NoRange &, const unsigned long long *w) {
    PredHost d;
    d.seen = (uint64_t)rows;
    d.satisfied = w[0];
    d.unknown = w[1];
    return d;
  }
  static void merge_host(PredHost &a, const PredHost &b) {
    a.seen += b.seen;
    a.satisfied += b.satisfied;
    a.unknown += b.unknown;
  }

  // per task { u32 n_leaves, n_ops, n_literal_bytes, 0; the leaves (48 bytes each); the ops (u16 each); the literal
  //   bytes (the plan's predicate, as it was set); u64 seen, satisfied, unknown }
  static void write(const RowPredicateTask &t, const PredHost &h, Writer &w) {
    const tgx_row_predicate_params &p = t.params;
    const uint32_t head[4] = {p.n_leaves, p.n_ops, p.n_literal_bytes, 0};
    w.pod(head);
    w.put(p.leaves, p.n_leaves * sizeof(tgx_row_predicate_leaf));
    w.put(p.program, p.n_ops * sizeof(uint16_t));
    w.put(p.literals, p.n_literal_bytes);
    const uint64_t counts[3] = {h.seen, h.satisfied, h.unknown};
    w.pod(counts);
  }

  static tgx_status read(const RowPredicateTask &t, PredHost &h, Reader &r, size_t k, tgx_error *err) {
    const tgx_row_predicate_params &p = t.params;
    uint32_t head[4];
    r.get(head, sizeof(head));
    if (!r.ok) return TGX_OK;
    if (head[0] != p.n_leaves || head[1] != p.n_ops || head[2] != p.n_literal_bytes || head[3] != 0)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "ROW_PREDICATE task %zu: the blob was counted under another predicate (%u leaves, %u ops, %u literal "
                  "bytes) than the plan's (%u, %u, %u)", k, head[0], head[1], head[2], p.n_leaves, p.n_ops,
                  p.n_literal_bytes);
    tgx_row_predicate_params q;
    memset(&q, 0, sizeof(q));
    r.get(q.leaves, p.n_leaves * sizeof(tgx_row_predicate_leaf));
    r.get(q.program, p.n_ops * sizeof(uint16_t));
    r.get(q.literals, p.n_literal_bytes);
    uint64_t counts[3];
    r.get(counts, sizeof(counts));
    if (!r.ok) return TGX_OK;
    const char *what = memcmp(q.leaves, p.leaves, sizeof(q.leaves)) != 0     ? "other leaves"
                       : memcmp(q.program, p.program, sizeof(q.program)) != 0 ? "another program"
                       : memcmp(q.literals, p.literals, sizeof(q.literals)) != 0 ? "other literal bytes"
                                                                                 : nullptr;
    if (what)
      return fail(err, TGX_INVALID_ARGUMENT, "ROW_PREDICATE task %zu: the blob was counted under %s than the plan's", k,
                  what);
    if (counts[1] > counts[0] || counts[2] > counts[0] - counts[1])
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (ROW_PREDICATE task %zu)", k);
    h.seen = counts[0];
    h.satisfied = counts[1];
    h.unknown = counts[2];
    return TGX_OK;
  }
};

struct PredCheck final : SideState<PredKind> {
  // the launch's descriptors on the host, twice: a buffer is written again only after its last upload is done
  struct Staging {
    std::vector<RowPredTask> tasks;
    hipEvent_t uploaded = nullptr;
    bool in_flight = false;
  };
  Staging staging[2];
  int next_staging = 0;
  DevBuf d_tasks;

  explicit PredCheck(const tgx_plan *plan) : SideState(plan) {}
  ~PredCheck() override {
    for (Staging &s : staging)
      if (s.uploaded) (void)hipEventDestroy(s.uploaded);
  }

  // may a batch whose columns have the types of st->col_types feed every leaf?  (what one column alone shows has been
  // asked by check_column; here the pairs of CMP_COLUMNS)
  tgx_status accepts(tgx_state *st, int64_t, tgx_error *err) override {
    for (const RowPredicateTask &t : st->plan->row_predicates)
      for (uint32_t j = 0; j < t.params.n_leaves; j++) {
        const tgx_row_predicate_leaf &l = t.params.leaves[j];
        if (l.kind != TGX_PRED_CMP_COLUMNS) continue;
        const TypeClass a = class_of(st->col_types[t.columns[l.col]]), b = class_of(st->col_types[t.columns[l.col2]]);
        if ((a == kClassString) != (b == kClassString))
          return fail(err, TGX_UNSUPPORTED, "spec %d: leaf %u of the ROW_PREDICATE compares a string column with a numeric one",
                      t.spec_index, j);
        if (a == kClassString && l.op != TGX_PRED_EQ)
          return fail(err, TGX_UNSUPPORTED, "spec %d: leaf %u of the ROW_PREDICATE orders two string columns (only = compares strings)",
                      t.spec_index, j);
      }
    return TGX_OK;
  }

  // task k of the plan over the batch's device columns, as the kernels take it; *numeric: the streaming route
  tgx_status describe(tgx_state *st, size_t k, const tgx_column *dev, int64_t nrows, RowPredTask *out, bool *numeric,
                      uint64_t *bytes, tgx_error *err) {
    const RowPredicateTask &task = st->plan->row_predicates[k];
    const tgx_row_predicate_params &p = task.params;
    RowPredTask &D = *out;
    memset(&D, 0, sizeof(D));
    D.d.n_cols = task.n_columns;
    D.d.length = nrows;
    D.n_leaves = p.n_leaves;
    D.n_ops = p.n_ops;
    D.word = (uint32_t)word_off[k];
    memcpy(D.program, p.program, sizeof(D.program));
    memcpy(D.literals, p.literals, sizeof(D.literals));
    for (uint32_t j = 0; j < p.n_leaves; j++)
      if (reads_values(p.leaves[j])) {
        D.reads |= 1u << p.leaves[j].col;
        if (p.leaves[j].kind == TGX_PRED_CMP_COLUMNS) D.reads |= 1u << p.leaves[j].col2;
      }
    *numeric = true;
    TypeClass cls[kRowPredicateMaxCols];
    for (int c = 0; c < task.n_columns; c++) {
      const tgx_column &x = dev[task.columns[c]];
      TupleCol &tc = D.d.cols[c];
      tc.validity = x.validity;
      tc.offset = x.offset;
      cls[c] = class_of(x.type);
      const bool read = (D.reads >> c) & 1u;
      if (is_any_string(x.type)) {
        tc.kind = x.type == TGX_UTF8 ? 1 : x.type == TGX_LARGE_UTF8 ? 2 : 3;
        tc.values = x.type == TGX_UTF8_VIEW ? x.values : nullptr;
        tc.buffers = x.type == TGX_UTF8_VIEW ? x.variadic : nullptr;
        tc.offsets = x.offsets;
        tc.data = x.data;
        *numeric = false;
        *bytes += (uint64_t)nrows * (x.type == TGX_UTF8 ? 4 : x.type == TGX_LARGE_UTF8 ? 8 : 16);
      } else if (x.type == TGX_DICT32_UTF8) {
        const tgx_column *dc = x.dictionary;
        if (!dc || !is_string(dc->type)) return fail(err, TGX_INVALID_ARGUMENT, "ROW_PREDICATE: malformed dictionary");
        tc.kind = 4;
        tc.dict_large = dc->type == TGX_LARGE_UTF8 ? 1 : 0;
        tc.values = x.values;
        tc.offsets = dc->offsets;
        tc.data = dc->data;
        tc.dict_validity = dc->validity;
        tc.dict_offset = dc->offset;
        D.dict_length[c] = dc->length;
        *numeric = false;
        *bytes += (uint64_t)nrows * 4;
      } else {
        // (an Int64 or Float64 view where a leaf reads the values: the staging has widened what is narrower)
        if (read && (!is_numeric(x.type) || !x.values))
          return fail(err, TGX_UNSUPPORTED, "ROW_PREDICATE compares 8-byte numeric values (%d)", x.type);
        tc.kind = 0;
        tc.values = read ? x.values : nullptr;
        if (read) *bytes += (uint64_t)nrows * 8;
      }
      if (x.validity) *bytes += (uint64_t)(nrows + 7) / 8;
    }
    for (uint32_t j = 0; j < p.n_leaves; j++) {
      const tgx_row_predicate_leaf &l = p.leaves[j];
      RowPredLeaf &L = D.leaves[j];
      L.kind = (uint8_t)l.kind;
      L.op = (uint8_t)l.op;
      L.col = (uint8_t)l.col;
      L.col2 = (uint8_t)l.col2;
      L.lit_offset = l.lit_offset;
      L.lit_len = l.lit_len;
      const TypeClass a = cls[l.col], b = cls[l.col2];
      bool fits = true;
      switch (l.kind) {
        case TGX_PRED_IS_NULL:
          break;
        case TGX_PRED_CMP_LITERAL:
          fits = a == kClassInt || a == kClassFloat;
          L.a_float = a == kClassFloat;
          L.keyed = L.a_float || (l.flags & TGX_PRED_LITERAL_IS_DOUBLE);
          L.lit = L.keyed ? key_of(l.lit_f) : l.lit_i;
          break;
        case TGX_PRED_CMP_COLUMNS:
          if (a == kClassString && b == kClassString) {
            fits = l.op == TGX_PRED_EQ;
            L.strings = 1;
          } else {
            fits = (a == kClassInt || a == kClassFloat) && (b == kClassInt || b == kClassFloat);
            L.a_float = a == kClassFloat;
            L.b_float = b == kClassFloat;
            L.keyed = L.a_float || L.b_float;
          }
          break;
        case TGX_PRED_STR_LENGTH:
          fits = a == kClassString;
          L.strings = (l.flags & TGX_PRED_LENGTH_IN_BYTES) != 0;
          L.lit = l.lit_i;
          break;
        case TGX_PRED_STR_LIKE:
          fits = a == kClassString;
          L.lit = (int64_t)sl::like_min_len(p.literals + l.lit_offset, l.lit_len);
          break;
        default:
          fits = a == kClassString;
          break;
      }
      if (!fits)
        return fail(err, TGX_UNSUPPORTED, "spec %d: leaf %u of the ROW_PREDICATE does not fit the type of its column",
                    task.spec_index, j);
      D.keys |= L.keyed;
    }
    return TGX_OK;
  }

  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    const tgx_plan *plan = st->plan;
    const size_t n_tasks = plan->row_predicates.size();
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    Staging &S = staging[next_staging];
    next_staging ^= 1;
    if (!S.uploaded) HIP_TRY(hipEventCreateWithFlags(&S.uploaded, hipEventDisableTiming));
    if (S.in_flight) HIP_TRY(hipEventSynchronize(S.uploaded));
    S.in_flight = false;
    S.tasks.resize(n_tasks);
    // the numeric tasks first, then the general ones: a launch's descriptors stand side by side
    std::vector<RowPredTask> one(1);
    std::vector<char> numeric(n_tasks, 0);
    std::vector<uint64_t> bytes(n_tasks, 0);
    std::vector<int> order;
    size_t n_numeric = 0;
    for (int pass = 0; pass < 2; pass++)
      for (size_t k = 0; k < n_tasks; k++) {
        if (pass == 0) {
          bool is_numeric_task = true;
          TGX_TRY(describe(st, k, dev, nrows, &one[0], &is_numeric_task, &bytes[k], err));
          numeric[k] = is_numeric_task;
          if (!is_numeric_task) continue;
          S.tasks[order.size()] = one[0];
          order.push_back((int)k);
          n_numeric++;
        } else if (!numeric[k]) {
          uint64_t again = 0;
          bool is_numeric_task = false;
          TGX_TRY(describe(st, k, dev, nrows, &S.tasks[order.size()], &is_numeric_task, &again, err));
          order.push_back((int)k);
        }
      }
    HIP_TRY(d_tasks.reserve(n_tasks * sizeof(RowPredTask)));
    HIP_TRY(hipMemcpyAsync(d_tasks.p, S.tasks.data(), n_tasks * sizeof(RowPredTask), hipMemcpyHostToDevice, st->stream));
    HIP_TRY(hipEventRecord(S.uploaded, st->stream));
    S.in_flight = true;
    for (size_t t0 = 0; t0 < n_tasks;) {
      const bool is_numeric_launch = t0 < n_numeric;
      const size_t end = is_numeric_launch ? n_numeric : n_tasks;
      const int n = (int)std::min<size_t>(kSidePerLaunch, end - t0);
      uint64_t moved = 0;
      for (int g = 0; g < n; g++) moved += bytes[order[t0 + g]];
      // 4 waves a workgroup, up to 8 workgroups a CU
      const int blocks = side_blocks(nrows, kRowPredBlock, g_ctx.n_cu, 8, n);
      TGX_TRY(side_rows_fit("ROW_PREDICATE", nrows, blocks, err));
      ProfScope ps(st, "row_predicate", moved);
      launch_row_predicate(d_tasks.as<RowPredTask>() + t0, n, is_numeric_launch, blocks,
                           d_counts.as<unsigned long long>(), st->stream);
      HIP_TRY(hipGetLastError());
      for (int g = 0; g < n; g++) device_rows[order[t0 + g]] += nrows;  // (only rows the device was given)
      t0 += n;
    }
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    std::vector<PredHost> g;
    TGX_TRY(gather(st, &g, err));
    r->total = (int64_t)g[slot].seen;
    r->matches = (int64_t)g[slot].satisfied;
    r->non_null = (int64_t)(g[slot].seen - g[slot].unknown);
    return TGX_OK;
  }
};

}  // namespace

tgx_status rowpredicate_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 != -1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: ROW_PREDICATE names its columns through the column list: column2 must be -1 (%d)",
                spec_index, sp.column2);
  RowPredicateTask t;
  memset(&t, 0, sizeof(t));
  t.spec_index = spec_index;  // (tgx_plan_create gives the task its column list)
  plan->row_predicates.push_back(t);
  *slot = (int)plan->row_predicates.size() - 1;
  return TGX_OK;
}

tgx_status rowpredicate_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const RowPredicateTask &t : plan->row_predicates)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "spec %d: a ROW_PREDICATE check needs its predicate (tgx_plan_set_row_predicate)", t.spec_index);
  return TGX_OK;
}

// (asked at tgx_plan_create, before any predicate is set: the columns are touched.  Which of them are READ, as 8-byte
//  values, is known once the predicate is: tgx_plan_set_row_predicate marks those -- a column that only IS_NULL leaves
//  name brings its validity alone, and may be a validity-only column)
void rowpredicate_mark_columns(tgx_plan *plan) {
  for (const RowPredicateTask &t : plan->row_predicates)
    for (int c = 0; c < t.n_columns; c++)
      plan->used[t.columns[c]] = plan->side_on[PredCheck::kIndex][t.columns[c]] = 1;
}

tgx_status rowpredicate_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err) {
  const TypeClass cls = class_of(c.type);
  for (const RowPredicateTask &t : plan->row_predicates)
    for (uint32_t j = 0; j < t.params.n_leaves; j++) {
      const tgx_row_predicate_leaf &l = t.params.leaves[j];
      const bool first = t.columns[l.col] == column;
      const bool second = l.kind == TGX_PRED_CMP_COLUMNS && t.columns[l.col2] == column;
      if ((!first && !second) || l.kind == TGX_PRED_IS_NULL) continue;
      if (cls == kClassOther)
        return fail(err, TGX_UNSUPPORTED, "column %d: ROW_PREDICATE takes %s columns under IS NULL only (spec %d, leaf %u)",
                    column, c.type == TGX_BOOL ? "Boolean" : "UInt64", t.spec_index, j);
      if (string_leaf(l.kind) && cls != kClassString)
        return fail(err, TGX_UNSUPPORTED, "column %d: a string leaf of the ROW_PREDICATE on a numeric column (spec %d, leaf %u)",
                    column, t.spec_index, j);
      if (l.kind == TGX_PRED_CMP_LITERAL && cls == kClassString)
        return fail(err, TGX_UNSUPPORTED, "column %d: a numeric leaf of the ROW_PREDICATE on a string column (spec %d, leaf %u)",
                    column, t.spec_index, j);
      if (cls != kClassString && c.length > 0 && !c.values)
        return fail(err, TGX_UNSUPPORTED, "column %d: ROW_PREDICATE reads the values: a validity-only column has none (spec %d, leaf %u)",
                    column, t.spec_index, j);
    }
  return TGX_OK;
}

SideCheck *rowpredicate_state_new(const tgx_plan *plan) {
  return plan->row_predicates.empty() ? nullptr : new PredCheck(plan);
}

}  // namespace tgx

using namespace tgx;

extern "C" tgx_status tgx_plan_set_row_predicate(tgx_plan *plan, size_t spec_index, const tgx_row_predicate_params *p,
                                                 tgx_error *err) try {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_ROW_PREDICATE, "ROW_PREDICATE", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the predicate of a ROW_PREDICATE check is fixed once a state of the plan exists");
  RowPredicateTask &t = plan->row_predicates[slot];
  if (p->n_leaves < 1 || p->n_leaves > TGX_PRED_MAX_LEAVES)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: a ROW_PREDICATE has 1..%d leaves (%u)", spec_index,
                TGX_PRED_MAX_LEAVES, p->n_leaves);
  if (p->n_ops < 1 || p->n_ops > TGX_PRED_MAX_OPS)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: a ROW_PREDICATE program has 1..%d ops (%u)", spec_index,
                TGX_PRED_MAX_OPS, p->n_ops);
  if (p->n_literal_bytes > TGX_PRED_MAX_LITERAL_BYTES)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: a ROW_PREDICATE holds up to %d literal bytes (%u)", spec_index,
                TGX_PRED_MAX_LITERAL_BYTES, p->n_literal_bytes);
  // (what a leaf does not read is kept as zero bits: the blob compares the predicate byte by byte)
  tgx_row_predicate_params q;
  memset(&q, 0, sizeof(q));
  q.n_leaves = p->n_leaves;
  q.n_ops = p->n_ops;
  q.n_literal_bytes = p->n_literal_bytes;
  memcpy(q.literals, p->literals, p->n_literal_bytes);
  for (uint32_t j = 0; j < p->n_leaves; j++) {
    const tgx_row_predicate_leaf &l = p->leaves[j];
    tgx_row_predicate_leaf &o = q.leaves[j];
    if (l.kind < TGX_PRED_IS_NULL || l.kind > TGX_PRED_STR_BLANK || l.kind == 5)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: unknown leaf kind %d", spec_index, j, l.kind);
    if (l.col < 0 || l.col >= t.n_columns)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u names column slot %d of a list of %d", spec_index, j, l.col,
                  t.n_columns);
    o.kind = l.kind;
    o.col = l.col;
    const bool compares = l.kind == TGX_PRED_CMP_LITERAL || l.kind == TGX_PRED_CMP_COLUMNS;
    if (compares) {
      if (l.op < TGX_PRED_EQ || l.op > TGX_PRED_GE)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: unknown comparison %d", spec_index, j, l.op);
      o.op = l.op;
    }
    if (l.kind == TGX_PRED_CMP_COLUMNS) {
      if (l.col2 < 0 || l.col2 >= t.n_columns)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u names column slot %d of a list of %d", spec_index, j,
                    l.col2, t.n_columns);
      o.col2 = l.col2;
    }
    if (l.kind == TGX_PRED_CMP_LITERAL) {
      if (l.flags & ~(uint32_t)TGX_PRED_LITERAL_IS_DOUBLE)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: unknown flags 0x%x", spec_index, j, l.flags);
      o.flags = l.flags;
      o.lit_i = l.lit_i;
      o.lit_f = l.lit_f;
    }
    if (l.kind == TGX_PRED_STR_CMP) {
      if (l.op == TGX_PRED_EQ)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: STR_CMP orders (LT .. GE): use STR_EQ for =", spec_index, j);
      if (l.op < TGX_PRED_LT || l.op > TGX_PRED_GE)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: unknown comparison %d", spec_index, j, l.op);
      o.op = l.op;
    }
    if (l.kind == TGX_PRED_STR_LENGTH) {
      if (l.op < TGX_PRED_EQ || l.op > TGX_PRED_GE)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: unknown comparison %d", spec_index, j, l.op);
      if (l.flags & ~(uint32_t)TGX_PRED_LENGTH_IN_BYTES)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: unknown flags 0x%x", spec_index, j, l.flags);
      o.op = l.op;
      o.flags = l.flags;
      o.lit_i = l.lit_i;
    }
    if ((l.kind == TGX_PRED_STR_CMP || l.kind == TGX_PRED_STR_LIKE || l.kind == TGX_PRED_STR_BLANK) && l.flags)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: unknown flags 0x%x", spec_index, j, l.flags);
    if (l.kind == TGX_PRED_STR_EQ || l.kind == TGX_PRED_STR_CMP || l.kind == TGX_PRED_STR_LIKE) {
      if (l.lit_offset > p->n_literal_bytes || l.lit_len > p->n_literal_bytes - l.lit_offset)
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u names literal bytes [%u, %u + %u) of a pool of %u", spec_index,
                    j, l.lit_offset, l.lit_offset, l.lit_len, p->n_literal_bytes);
      o.lit_offset = l.lit_offset;
      o.lit_len = l.lit_len;
      if (l.kind == TGX_PRED_STR_LIKE && memchr(p->literals + l.lit_offset, 0x5C, l.lit_len))
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: leaf %u: a LIKE pattern may not hold a backslash (0x5C): there is no escape",
                    spec_index, j);
    }
  }
  int depth = 0;
  for (uint32_t k = 0; k < p->n_ops; k++) {
    const uint32_t code = p->program[k] & 255u, arg = p->program[k] >> 8;
    switch (code) {
      case TGX_PRED_PUSH:
        if (arg >= p->n_leaves)
          return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: op %u pushes leaf %u of %u", spec_index, k, arg, p->n_leaves);
        if (++depth > TGX_PRED_MAX_DEPTH)
          return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: op %u: the program exceeds depth %d", spec_index, k,
                      TGX_PRED_MAX_DEPTH);
        break;
      case TGX_PRED_AND:
      case TGX_PRED_OR:
      case TGX_PRED_NOT:
        if (arg != 0) return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: op %u: only PUSH takes an argument", spec_index, k);
        if (depth < (code == TGX_PRED_NOT ? 1 : 2))
          return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: op %u: the program underflows its stack", spec_index, k);
        if (code != TGX_PRED_NOT) depth--;
        break;
      default:
        return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: op %u: unknown op code %u", spec_index, k, code);
    }
    q.program[k] = p->program[k];
  }
  if (depth != 1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the program leaves %d values, not one", spec_index, depth);
  t.params = q;
  t.set = true;
  // (no state exists yet: the plan's per-column flags may still grow.  A predicate set over an earlier one leaves the
  //  earlier one's marks behind, which costs a copy and nothing else)
  for (uint32_t j = 0; j < q.n_leaves; j++) {
    const tgx_row_predicate_leaf &l = q.leaves[j];
    if (!reads_values(l)) continue;
    side_mark(plan, side_index(TGX_CHECK_ROW_PREDICATE), t.columns[l.col], true);
    if (l.kind == TGX_PRED_CMP_COLUMNS) side_mark(plan, side_index(TGX_CHECK_ROW_PREDICATE), t.columns[l.col2], true);
  }
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_row_predicate_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                            tgx_row_predicate_counts *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_ROW_PREDICATE, "ROW_PREDICATE", &slot, err, "bad arguments"));
  std::vector<PredHost> g;
  TGX_TRY(PredCheck::of(st)->gather(st, &g, err));
  out->seen = g[slot].seen;
  out->satisfied = g[slot].satisfied;
  out->unknown = g[slot].unknown;
  out->failed = g[slot].seen - g[slot].satisfied - g[slot].unknown;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
