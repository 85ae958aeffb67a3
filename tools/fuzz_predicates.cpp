// fuzz_predicates.cpp -- seeded random and mutated expressions through the predicate compiler of Check::satisfies and
// ComplianceAnalyzer (term_amd/csrc/host/custom_sql.cpp): the parser takes text from users.
//
// A stand-alone host program: no device, no HIP, nothing of the library but custom_sql.cpp.  Build it with the
// sanitizers and run it on a CPU machine:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -DTGX_PREDICATE_COMPILER_ONLY \
//         tools/fuzz_predicates.cpp term_amd/csrc/host/custom_sql.cpp -o fuzz_predicates && ./fuzz_predicates [cases] [seed]
//
// Every case is one of
//   generated   an expression drawn from the grammar, together with the tree it was drawn from.  It must compile, and the
//               compiled program must ROUND-TRIP: interpreted on a table of rows it gives what the tree gives, and the JSON
//               (row_predicate_json) must name as many leaves, ops and literal bytes as the parameters hold
//   mutated     a generated expression with bytes deleted, doubled, swapped or replaced.  It compiles or it is refused
//               with a non-empty message: it must not crash, hang or trip a sanitizer.  What compiles is checked against
//               the ABI's own limits (leaf / op / column / literal ranges, stack depth)
// Exit status 0: every case ran clean.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../term_amd/csrc/host/custom_sql.h"

using namespace term_guard;

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

// ---- a tiny three-valued reference: 0 FALSE, 1 TRUE, 2 UNKNOWN ---------------------------------------------------------
enum { kF = 0, kT = 1, kU = 2 };
int k_not(int a) { return a == kU ? kU : 1 - a; }
int k_and(int a, int b) { return (a == kF || b == kF) ? kF : (a == kU || b == kU) ? kU : kT; }
int k_or(int a, int b) { return (a == kT || b == kT) ? kT : (a == kU || b == kU) ? kU : kF; }

int64_t key_of(double x) {
  int64_t b;
  memcpy(&b, &x, sizeof(b));
  return b ^ (int64_t)(((uint64_t)(b >> 63)) >> 1);
}

// the table: two integer columns (i0, i1) and two string columns (s0, s1); a row holds NULL flags and values
struct Row {
  bool null_i[2], null_s[2];
  int64_t i[2];
  std::string s[2];
};

bool compare(int op, int64_t a, int64_t b) {
  switch (op) {
    case TGX_PRED_EQ: return a == b;
    case TGX_PRED_LT: return a < b;
    case TGX_PRED_LE: return a <= b;
    case TGX_PRED_GT: return a > b;
    default: return a >= b;
  }
}

struct Node {
  enum Kind { And, Or, Not, IsNull, CmpInt, CmpDouble, CmpCols, StrEq } kind;
  std::unique_ptr<Node> a, b;
  int col = 0, col2 = 0, op = TGX_PRED_EQ;  // col: 0, 1 integer columns; 2, 3 string columns
  int64_t lit_i = 0;
  double lit_f = 0;
  std::string text;
};

int eval(const Node &n, const Row &r) {
  switch (n.kind) {
    case Node::And: return k_and(eval(*n.a, r), eval(*n.b, r));
    case Node::Or: return k_or(eval(*n.a, r), eval(*n.b, r));
    case Node::Not: return k_not(eval(*n.a, r));
    case Node::IsNull: return (n.col < 2 ? r.null_i[n.col] : r.null_s[n.col - 2]) ? kT : kF;
    case Node::CmpInt: return r.null_i[n.col] ? kU : compare(n.op, r.i[n.col], n.lit_i);
    case Node::CmpDouble: return r.null_i[n.col] ? kU : compare(n.op, key_of((double)r.i[n.col]), key_of(n.lit_f));
    case Node::CmpCols:
      if (n.col >= 2) return (r.null_s[n.col - 2] || r.null_s[n.col2 - 2]) ? kU : r.s[n.col - 2] == r.s[n.col2 - 2];
      return (r.null_i[n.col] || r.null_i[n.col2]) ? kU : compare(n.op, r.i[n.col], r.i[n.col2]);
    default: return r.null_s[n.col - 2] ? kU : r.s[n.col - 2] == n.text;
  }
}

const char *const kNames[4] = {"i0", "i1", "s0", "s1"};
const char *const kOps[6] = {"", "=", "<", "<=", ">", ">="};
const char *const kStrings[5] = {"", "F", "it's", "open", "a longer value"};

std::string quoted(const std::string &s) {
  std::string o = "'";
  for (char c : s) o += c == '\'' ? std::string("''") : std::string(1, c);
  return o + "'";
}

std::string name_of(Rng &g, int col) {
  switch (g.below(3)) {
    case 0: return kNames[col];
    case 1: return std::string("\"") + kNames[col] + "\"";
    default: {
      std::string n = kNames[col];
      n[0] = (char)(n[0] - 32);  // unquoted identifiers are lowercased
      return n;
    }
  }
}

std::unique_ptr<Node> leaf(Node::Kind k) {
  std::unique_ptr<Node> n(new Node());
  n->kind = k;
  return n;
}
std::unique_ptr<Node> both(Node::Kind k, std::unique_ptr<Node> a, std::unique_ptr<Node> b) {
  std::unique_ptr<Node> n(new Node());
  n->kind = k;
  n->a = std::move(a);
  n->b = std::move(b);
  return n;
}

// an atom of the grammar and the tree it means (SQL's definitions of <>, BETWEEN and IN)
std::unique_ptr<Node> atom(Rng &g, std::string *text, int *leaves) {
  const int form = g.below(8);
  const int icol = g.below(2), scol = 2 + g.below(2);
  const std::string in = name_of(g, icol), sn = name_of(g, scol);
  auto int_leaf = [&](int op, int64_t v) {
    auto n = leaf(Node::CmpInt);
    n->col = icol;
    n->op = op;
    n->lit_i = v;
    (*leaves)++;
    return n;
  };
  auto str_leaf = [&](const std::string &v) {
    auto n = leaf(Node::StrEq);
    n->col = scol;
    n->text = v;
    (*leaves)++;
    return n;
  };
  switch (form) {
    case 0: {  // col op int, or turned round
      const int op = 1 + g.below(5);
      const int64_t v = g.below(7) - 3;
      static const int turned[6] = {0, TGX_PRED_EQ, TGX_PRED_GT, TGX_PRED_GE, TGX_PRED_LT, TGX_PRED_LE};
      if (g.below(2)) *text = in + " " + kOps[op] + " " + std::to_string((long long)v);
      else *text = std::to_string((long long)v) + " " + kOps[turned[op]] + " " + in;
      return int_leaf(op, v);
    }
    case 1: {  // col op double
      const int op = 1 + g.below(5);
      const double v = (g.below(9) - 4) * 0.5;
      char buf[64];
      snprintf(buf, sizeof(buf), g.below(2) ? "%.1f" : "%.2e", v);
      auto n = leaf(Node::CmpDouble);
      n->col = icol;
      n->op = op;
      n->lit_f = strtod(buf, nullptr);
      (*leaves)++;
      *text = in + " " + kOps[op] + " " + buf;
      return n;
    }
    case 2: {  // <> / !=
      const int64_t v = g.below(5) - 2;
      *text = in + (g.below(2) ? " <> " : " != ") + std::to_string((long long)v);
      auto n = leaf(Node::Not);
      n->a = int_leaf(TGX_PRED_EQ, v);
      return n;
    }
    case 3: {  // IS [NOT] NULL
      const bool no = g.below(2), str = g.below(2);
      *text = (str ? sn : in) + (no ? " IS NOT NULL" : " is null");
      auto n = leaf(Node::IsNull);
      n->col = str ? scol : icol;
      (*leaves)++;
      if (!no) return n;
      auto m = leaf(Node::Not);
      m->a = std::move(n);
      return m;
    }
    case 4: {  // [NOT] BETWEEN
      const bool no = g.below(2);
      const int64_t lo = g.below(7) - 3, hi = g.below(7) - 3;
      *text = in + (no ? " NOT BETWEEN " : " BETWEEN ") + std::to_string((long long)lo) + " AND " + std::to_string((long long)hi);
      auto n = both(Node::And, int_leaf(TGX_PRED_GE, lo), int_leaf(TGX_PRED_LE, hi));
      if (!no) return n;
      auto m = leaf(Node::Not);
      m->a = std::move(n);
      return m;
    }
    case 5: {  // [NOT] IN of integers or of strings
      const bool no = g.below(2), str = g.below(2);
      const int count = 1 + g.below(3);
      *text = (str ? sn : in) + (no ? " NOT IN (" : " IN (");
      std::unique_ptr<Node> n;
      for (int k = 0; k < count; k++) {
        std::unique_ptr<Node> one;
        if (str) {
          const std::string v = kStrings[g.below(5)];
          *text += (k ? ", " : "") + quoted(v);
          one = str_leaf(v);
        } else {
          const int64_t v = g.below(7) - 3;
          *text += (k ? ", " : "") + std::to_string((long long)v);
          one = int_leaf(TGX_PRED_EQ, v);
        }
        n = n ? both(Node::Or, std::move(n), std::move(one)) : std::move(one);
      }
      *text += ")";
      if (!no) return n;
      auto m = leaf(Node::Not);
      m->a = std::move(n);
      return m;
    }
    case 6: {  // string = / <> literal
      const bool no = g.below(2);
      const std::string v = kStrings[g.below(5)];
      *text = g.below(2) ? sn + (no ? " <> " : " = ") + quoted(v) : quoted(v) + (no ? " != " : " = ") + sn;
      auto n = str_leaf(v);
      if (!no) return n;
      auto m = leaf(Node::Not);
      m->a = std::move(n);
      return m;
    }
    default: {  // column against column
      auto n = leaf(Node::CmpCols);
      (*leaves)++;
      if (g.below(2)) {
        n->col = 2;
        n->col2 = 3;
        *text = name_of(g, 2) + " = " + name_of(g, 3);
      } else {
        n->col = icol;
        n->col2 = 1 - icol;
        n->op = 1 + g.below(5);
        *text = in + " " + kOps[n->op] + " " + name_of(g, 1 - icol);
      }
      return n;
    }
  }
}

// pred / term / factor with explicit parentheses wherever precedence would otherwise decide
std::unique_ptr<Node> expression(Rng &g, int depth, std::string *text, int *leaves) {
  if (depth == 0 || *leaves >= 20 || g.below(3) == 0) return atom(g, text, leaves);
  const int form = g.below(3);
  if (form == 0) {
    std::string inner;
    auto n = leaf(Node::Not);
    n->a = expression(g, depth - 1, &inner, leaves);
    *text = "NOT (" + inner + ")";
    return n;
  }
  std::string l, r;
  auto a = expression(g, depth - 1, &l, leaves);
  auto b = expression(g, depth - 1, &r, leaves);
  *text = "(" + l + (form == 1 ? ") AND (" : ") or (") + r + ")";
  return both(form == 1 ? Node::And : Node::Or, std::move(a), std::move(b));
}

// ---- the compiled predicate, interpreted ---------------------------------------------------------------------------------
int fail(const char *what, const std::string &text) {
  fprintf(stderr, "FAILED: %s\n  expression: %s\n", what, text.c_str());
  return 1;
}

// the ABI's own limits on what the compiler made; 0 when they hold
int well_formed(const RowPredicate &p, const std::string &text) {
  const tgx_row_predicate_params &q = p.params;
  if (p.columns.empty() || p.columns.size() > TGX_PRED_MAX_COLUMNS) return fail("column count", text);
  if (q.n_leaves < 1 || q.n_leaves > TGX_PRED_MAX_LEAVES || q.n_ops < 1 || q.n_ops > TGX_PRED_MAX_OPS ||
      q.n_literal_bytes > TGX_PRED_MAX_LITERAL_BYTES)
    return fail("counts out of range", text);
  for (uint32_t j = 0; j < q.n_leaves; j++) {
    const tgx_row_predicate_leaf &l = q.leaves[j];
    if (l.kind < TGX_PRED_IS_NULL || l.kind > TGX_PRED_STR_EQ || l.col < 0 || l.col >= (int)p.columns.size() || l.col2 < 0 ||
        l.col2 >= (int)p.columns.size())
      return fail("leaf kind / column out of range", text);
    if (l.kind == TGX_PRED_STR_EQ && (l.lit_offset > q.n_literal_bytes || l.lit_len > q.n_literal_bytes - l.lit_offset))
      return fail("literal range outside the pool", text);
    if ((l.kind == TGX_PRED_CMP_LITERAL || l.kind == TGX_PRED_CMP_COLUMNS) && (l.op < TGX_PRED_EQ || l.op > TGX_PRED_GE))
      return fail("comparison out of range", text);
  }
  int depth = 0;
  for (uint32_t k = 0; k < q.n_ops; k++) {
    const int code = q.program[k] & 255, arg = q.program[k] >> 8;
    if (code == TGX_PRED_PUSH) {
      if (arg >= (int)q.n_leaves || ++depth > TGX_PRED_MAX_DEPTH) return fail("push out of range / too deep", text);
    } else if (code == TGX_PRED_NOT) {
      if (depth < 1) return fail("underflow", text);
    } else if (code == TGX_PRED_AND || code == TGX_PRED_OR) {
      if (depth < 2) return fail("underflow", text);
      depth--;
    } else {
      return fail("unknown op", text);
    }
  }
  if (depth != 1) return fail("the program does not leave one value", text);
  return 0;
}

int run(const RowPredicate &p, const Row &r) {
  int stack[TGX_PRED_MAX_DEPTH + 1], top = 0;
  auto slot = [&](int c) {
    for (int k = 0; k < 4; k++)
      if (p.columns[c] == kNames[k]) return k;
    return -1;
  };
  for (uint32_t k = 0; k < p.params.n_ops; k++) {
    const int code = p.params.program[k] & 255, arg = p.params.program[k] >> 8;
    if (code == TGX_PRED_NOT) {
      stack[top - 1] = k_not(stack[top - 1]);
    } else if (code != TGX_PRED_PUSH) {
      top--;
      stack[top - 1] = code == TGX_PRED_AND ? k_and(stack[top - 1], stack[top]) : k_or(stack[top - 1], stack[top]);
    } else {
      const tgx_row_predicate_leaf &l = p.params.leaves[arg];
      const int c = slot(l.col), c2 = slot(l.col2);
      int v;
      if (c < 0) return -1;
      if (l.kind == TGX_PRED_IS_NULL) {
        v = (c < 2 ? r.null_i[c] : r.null_s[c - 2]) ? kT : kF;
      } else if (l.kind == TGX_PRED_STR_EQ) {
        if (c < 2) return -1;
        v = r.null_s[c - 2] ? kU
                            : r.s[c - 2] == std::string((const char *)p.params.literals + l.lit_offset, l.lit_len);
      } else if (l.kind == TGX_PRED_CMP_LITERAL) {
        if (c >= 2) return -1;
        v = r.null_i[c] ? kU
            : (l.flags & TGX_PRED_LITERAL_IS_DOUBLE) ? (int)compare(l.op, key_of((double)r.i[c]), key_of(l.lit_f))
                                                     : (int)compare(l.op, r.i[c], l.lit_i);
      } else {
        if (c2 < 0 || (c < 2) != (c2 < 2)) return -1;
        if (c >= 2) v = (r.null_s[c - 2] || r.null_s[c2 - 2]) ? kU : r.s[c - 2] == r.s[c2 - 2];
        else v = (r.null_i[c] || r.null_i[c2]) ? kU : (int)compare(l.op, r.i[c], r.i[c2]);
      }
      stack[top++] = v;
    }
  }
  return stack[0];
}

std::string mutate(Rng &g, std::string s) {
  static const char *const pieces[] = {"(", ")", "'", "\"", " AND ", " OR ", " NOT ", " IN (", " BETWEEN ", " IS ", "NULL", ",",
                                       "-", "--", "1e999", "99999999999999999999", ".", "::", "+", " LIKE ", "\0x", "=", "<>",
                                       "<", ">=", "!", ";", "/*", "\xff", " ", "e", "0"};
  const int edits = 1 + g.below(4);
  for (int e = 0; e < edits; e++) {
    const size_t at = s.empty() ? 0 : (size_t)g.below((int)s.size());
    switch (g.below(5)) {
      case 0:
        if (!s.empty()) s.erase(at, 1 + (size_t)g.below(3));
        break;
      case 1:
        s.insert(at, pieces[g.below((int)(sizeof(pieces) / sizeof(pieces[0])))]);
        break;
      case 2:
        if (!s.empty()) s[at] = (char)g.below(256);
        break;
      case 3:
        if (!s.empty()) s.insert(at, s.substr(at, 1 + (size_t)g.below(8)));
        break;
      default:
        if (s.size() > 1) std::swap(s[at], s[(size_t)g.below((int)s.size())]);
        break;
    }
  }
  return s;
}

}  // namespace

int main(int argc, char **argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 200000;
  Rng g{argc > 2 ? (uint64_t)atoll(argv[2]) | 1 : 0x7E570021ull};
  // the rows: every NULL pattern over a few values
  std::vector<Row> rows;
  for (int pattern = 0; pattern < 16; pattern++)
    for (int v = 0; v < 6; v++) {
      Row r;
      r.null_i[0] = pattern & 1;
      r.null_i[1] = pattern & 2;
      r.null_s[0] = pattern & 4;
      r.null_s[1] = pattern & 8;
      r.i[0] = v - 3;
      r.i[1] = (v * 5) % 7 - 3;
      r.s[0] = kStrings[v % 5];
      r.s[1] = kStrings[(v * 2) % 5];
      rows.push_back(r);
    }
  long generated = 0, compiled_mutants = 0, refused_mutants = 0;
  for (long n = 0; n < cases; n++) {
    std::string text;
    int leaves = 0;
    std::unique_ptr<Node> tree = expression(g, 1 + g.below(4), &text, &leaves);
    if (n % 2 == 0) {
      RowPredicate p;
      try {
        p = compile_row_predicate(text);
      } catch (const PredicateRefusal &r) {
        // (only the limits may refuse what the grammar made)
        if (r.what.find("more than") == std::string::npos) return fail(("a generated expression was refused: " + r.what).c_str(), text);
        continue;
      }
      if (well_formed(p, text)) return 1;
      for (const Row &r : rows)
        if (run(p, r) != eval(*tree, r)) return fail("the compiled program and the tree disagree", text);
      const std::string js = row_predicate_json(p);
      size_t kinds = 0;
      for (size_t at = js.find("\"kind\""); at != std::string::npos; at = js.find("\"kind\"", at + 1)) kinds++;
      if (kinds != p.params.n_leaves || js.find("\"literals_hex\"") == std::string::npos)
        return fail("the JSON does not round-trip the leaves", text);
      generated++;
    } else {
      const std::string m = mutate(g, text);
      try {
        const RowPredicate p = compile_row_predicate(m);
        if (well_formed(p, m)) return 1;
        (void)row_predicate_json(p);
        compiled_mutants++;
      } catch (const PredicateRefusal &r) {
        if (r.what.empty()) return fail("a refusal without a message", m);
        refused_mutants++;
      }
      (void)custom_sql_refusal(m);
      (void)compliance_forbidden_keyword(m);
    }
  }
  printf("%ld cases ran clean: %ld generated expressions round-tripped, %ld mutants compiled, %ld mutants refused\n", cases,
         generated, compiled_mutants, refused_mutants);
  return 0;
}
