// custom_sql.cpp -- the predicate compiler, CustomSqlConstraint and the two validators (custom_sql.h).
#include "custom_sql.h"

#include <algorithm>
#include <ctype.h>
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "json.h"

namespace term_guard {

namespace {

// ---- tokens ------------------------------------------------------------------------------------------------------------
struct Token {
  enum Kind { End, Ident, Quoted, Integer, Float, String, Symbol } kind = End;
  std::string text;   // Ident: as written; Quoted / String: unescaped; Integer / Float: the token; Symbol: itself
  std::string upper;  // Ident: upper-cased (keywords are case-insensitive)
};

[[noreturn]] void refuse(const std::string &what) { throw PredicateRefusal{what}; }

std::string shown(const std::string &s) { return s.size() > 40 ? s.substr(0, 40) + ".." : s; }

struct Lexer {
  const std::string &src;
  size_t at = 0;
  explicit Lexer(const std::string &s) : src(s) {}

  Token next() {
    while (at < src.size() && isspace((unsigned char)src[at])) at++;
    Token t;
    if (at >= src.size()) return t;
    const char c = src[at];
    if (isalpha((unsigned char)c) || c == '_') {
      size_t b = at;
      while (at < src.size() && (isalnum((unsigned char)src[at]) || src[at] == '_')) at++;
      t.kind = Token::Ident;
      t.text = src.substr(b, at - b);
      for (char ch : t.text) t.upper += (char)toupper((unsigned char)ch);
      return t;
    }
    if (c == '"' || c == '\'') {  // "" / '' stand for the quote itself
      t.kind = c == '"' ? Token::Quoted : Token::String;
      at++;
      for (;;) {
        if (at >= src.size()) refuse(c == '"' ? "an unterminated quoted identifier" : "an unterminated string literal");
        if (src[at] == c) {
          if (at + 1 < src.size() && src[at + 1] == c) {
            t.text += c;
            at += 2;
            continue;
          }
          at++;
          break;
        }
        t.text += src[at++];
      }
      if (t.kind == Token::Quoted && t.text.empty()) refuse("an empty quoted identifier");
      return t;
    }
    if (isdigit((unsigned char)c)) {
      size_t b = at;
      bool is_float = false;
      while (at < src.size() && isdigit((unsigned char)src[at])) at++;
      if (at < src.size() && src[at] == '.') {
        is_float = true;
        at++;
        while (at < src.size() && isdigit((unsigned char)src[at])) at++;
      }
      if (at < src.size() && (src[at] == 'e' || src[at] == 'E')) {
        size_t e = at + 1;
        if (e < src.size() && (src[e] == '+' || src[e] == '-')) e++;
        if (e < src.size() && isdigit((unsigned char)src[e])) {
          is_float = true;
          at = e;
          while (at < src.size() && isdigit((unsigned char)src[at])) at++;
        }
      }
      t.kind = is_float ? Token::Float : Token::Integer;
      t.text = src.substr(b, at - b);
      if (at < src.size() && (isalpha((unsigned char)src[at]) || src[at] == '_'))
        refuse("a malformed number '" + shown(src.substr(b, at + 1 - b)) + "'");
      return t;
    }
    t.kind = Token::Symbol;
    static const char *const two[] = {"<>", "!=", "<=", ">=", "::", "||"};
    for (const char *s : two)
      if (src.compare(at, 2, s) == 0) {
        t.text = s;
        at += 2;
        return t;
      }
    t.text = std::string(1, c);
    at++;
    return t;
  }
};

// ---- the parser: straight into leaves and postfix ops ------------------------------------------------------------------
struct Operand {
  enum Kind { Column, Number, Text, Length, Trim } kind = Column;  // Length / Trim: lenfn(col) / TRIM(col)
  int col = 0;
  bool in_bytes = false;  // Length: OCTET_LENGTH
  bool is_double = false;
  int64_t i = 0;
  double f = 0;
  std::string text;
};

struct Compiler {
  Lexer lex;
  Token tok;
  RowPredicate out;
  PredicateDialect dialect;
  int depth = 0, max_depth = 0, nesting = 0;

  Compiler(const std::string &s, const PredicateDialect &d) : lex(s), dialect(d) {
    memset(&out.params, 0, sizeof(out.params));
    advance();
  }

  void advance() { tok = lex.next(); }
  bool keyword(const char *k) const { return tok.kind == Token::Ident && tok.upper == k; }
  bool symbol(const char *s) const { return tok.kind == Token::Symbol && tok.text == s; }
  std::string here() const {
    switch (tok.kind) {
      case Token::End: return "the end of the expression";
      case Token::String: return "'" + shown(tok.text) + "'";
      case Token::Quoted: return "\"" + shown(tok.text) + "\"";
      default: return "'" + shown(tok.text) + "'";
    }
  }

  // -- emitting
  int add_leaf(const tgx_row_predicate_leaf &l) {
    if (out.params.n_leaves >= TGX_PRED_MAX_LEAVES) refuse("more than 32 leaves");
    out.params.leaves[out.params.n_leaves] = l;
    return (int)out.params.n_leaves++;
  }
  void emit(int code, int arg = 0) {
    if (out.params.n_ops >= TGX_PRED_MAX_OPS) refuse("more than 64 ops");
    out.params.program[out.params.n_ops++] = (uint16_t)(code | (arg << 8));
    if (code == TGX_PRED_PUSH) {
      if (++depth > TGX_PRED_MAX_DEPTH) refuse("a program deeper than 32");
      max_depth = std::max(max_depth, depth);
    } else if (code != TGX_PRED_NOT) {
      depth--;
    }
  }
  void push_leaf(const tgx_row_predicate_leaf &l) { emit(TGX_PRED_PUSH, add_leaf(l)); }

  int column_slot(const std::string &name) {
    for (size_t i = 0; i < out.columns.size(); i++)
      if (out.columns[i] == name) return (int)i;
    if (out.columns.size() >= TGX_PRED_MAX_COLUMNS) refuse("more than 8 columns");
    out.columns.push_back(name);
    out.literal_compared.push_back(0);
    return (int)out.columns.size() - 1;
  }
  uint32_t pool(const std::string &bytes) {
    if (out.params.n_literal_bytes + bytes.size() > TGX_PRED_MAX_LITERAL_BYTES) refuse("more than 256 literal bytes");
    const uint32_t at = out.params.n_literal_bytes;
    memcpy(out.params.literals + at, bytes.data(), bytes.size());
    out.params.n_literal_bytes += (uint32_t)bytes.size();
    return at;
  }

  static tgx_row_predicate_leaf blank(int kind, int col) {
    tgx_row_predicate_leaf l;
    memset(&l, 0, sizeof(l));
    l.kind = kind;
    l.col = col;
    return l;
  }
  // col <op> literal, op one of TGX_PRED_EQ .. TGX_PRED_GE, onto the stack
  void compare_literal(int col, int op, const Operand &lit) {
    if (lit.kind == Operand::Text) {
      if (op != TGX_PRED_EQ && !dialect.string_functions)
        refuse("a string order comparison (only = and <> compare strings)");
      tgx_row_predicate_leaf l = blank(op == TGX_PRED_EQ ? TGX_PRED_STR_EQ : TGX_PRED_STR_CMP, col);
      if (op != TGX_PRED_EQ) l.op = op;
      l.lit_len = (uint32_t)lit.text.size();
      l.lit_offset = pool(lit.text);
      push_leaf(l);
      return;
    }
    tgx_row_predicate_leaf l = blank(TGX_PRED_CMP_LITERAL, col);
    l.op = op;
    l.flags = lit.is_double ? TGX_PRED_LITERAL_IS_DOUBLE : 0;
    l.lit_i = lit.is_double ? 0 : lit.i;
    l.lit_f = lit.is_double ? lit.f : (double)lit.i;
    out.literal_compared[col] = 1;
    push_leaf(l);
  }

  // -- operands
  Operand number(bool negative) {
    Operand o;
    o.kind = Operand::Number;
    const std::string text = (negative ? "-" : "") + tok.text;
    if (tok.kind == Token::Integer) {
      errno = 0;
      char *end = nullptr;
      const long long v = strtoll(text.c_str(), &end, 10);
      if (errno == ERANGE || !end || *end) refuse("an integer literal outside int64 (" + shown(text) + ")");
      o.i = v;
    } else {
      char *end = nullptr;
      o.is_double = true;
      o.f = strtod(text.c_str(), &end);
      if (!end || *end || !isfinite(o.f)) refuse("a float literal that is not finite (" + shown(text) + ")");
    }
    advance();
    return o;
  }

  Operand operand() {
    Operand o;
    if (tok.kind == Token::Integer || tok.kind == Token::Float) {
      o = number(false);
    } else if (symbol("-")) {
      advance();
      if (tok.kind != Token::Integer && tok.kind != Token::Float) refuse("arithmetic (a unary '-' before " + here() + ")");
      o = number(true);
    } else if (tok.kind == Token::String) {
      o.kind = Operand::Text;
      o.text = tok.text;
      advance();
    } else if (tok.kind == Token::Quoted) {
      const std::string name = tok.text;
      advance();
      if (symbol(".")) refuse("a qualified identifier (\"" + shown(name) + "\".)");
      o.col = column_slot(name);
    } else if (tok.kind == Token::Ident) {
      static const char *const refused[] = {"LIKE", "ILIKE", "CASE", "CAST", "TRY_CAST", "TRUE", "FALSE", "NULL",
                                            "SELECT", "EXISTS", "SIMILAR"};
      static const char *const typed[] = {"INTERVAL", "DATE", "TIMESTAMP", "TIME"};  // (DATE followed by a string)
      static const char *const misplaced[] = {"AND", "OR", "NOT", "IS", "IN", "BETWEEN"};
      for (const char *k : misplaced)
        if (tok.upper == k) refuse("'" + tok.text + "' where a column or a literal should stand");
      std::string name;
      for (char ch : tok.text) name += (char)tolower((unsigned char)ch);
      const std::string written = tok.text, upper = tok.upper;
      advance();
      if (symbol("(") && dialect.string_functions) {
        if (upper == "LTRIM" || upper == "RTRIM" || upper == "BTRIM") refuse(upper + " (only TRIM(col) = '' is taken)");
        const bool chars = upper == "LENGTH" || upper == "CHAR_LENGTH" || upper == "CHARACTER_LENGTH";
        if (chars || upper == "OCTET_LENGTH" || upper == "TRIM") {
          advance();
          if (upper == "TRIM" && (keyword("BOTH") || keyword("LEADING") || keyword("TRAILING"))) refuse("TRIM(.. FROM ..)");
          if (++nesting > 64) refuse("nesting deeper than 64");
          const Operand arg = operand();
          nesting--;
          if (upper == "TRIM" && keyword("FROM")) refuse("TRIM(.. FROM ..)");
          if (arg.kind == Operand::Length || arg.kind == Operand::Trim) refuse("a nested function call (" + upper + "(..(..)))");
          if (arg.kind != Operand::Column) refuse(upper + " of a literal");
          if (symbol(",")) refuse("a function call with several arguments (" + upper + "(.., ..))");
          if (!symbol(")")) refuse(here() + " where " + upper + "'s ')' should stand");
          advance();
          o.kind = upper == "TRIM" ? Operand::Trim : Operand::Length;
          o.col = arg.col;
          o.in_bytes = upper == "OCTET_LENGTH";
          return after_operand(o);
        }
      }
      if (symbol("(")) refuse("a function call (" + shown(written) + "(..))");
      for (const char *k : refused)
        if (upper == k) refuse(upper == "NULL" ? std::string("a NULL literal") : upper);
      for (const char *k : typed)
        if (upper == k && tok.kind == Token::String) refuse("a typed literal (" + upper + " '..')");
      if (symbol(".")) refuse("a qualified identifier (" + shown(written) + ".)");
      o.col = column_slot(name);
    } else {
      refuse(here() + " where a column or a literal should stand");
    }
    return after_operand(o);
  }

  Operand after_operand(const Operand &o) {
    // what may follow an operand is a comparison, a keyword, ')' or ',': an operator is arithmetic
    if (tok.kind == Token::Symbol) {
      static const char *const arithmetic[] = {"+", "-", "*", "/", "%", "||"};
      for (const char *a : arithmetic)
        if (tok.text == a) refuse("arithmetic ('" + tok.text + "')");
      if (tok.text == "::") refuse("a cast (::)");
    }
    return o;
  }

  Operand literal() {
    Operand o = operand();
    if (o.kind == Operand::Length || o.kind == Operand::Trim) refuse("a function call where a literal should stand");
    if (o.kind == Operand::Column) refuse("a column where a literal should stand (" + shown(out.columns[o.col]) + ")");
    return o;
  }

  static int comparison(const Token &t) {  // 0: none; 6: <> / !=
    if (t.kind != Token::Symbol) return 0;
    if (t.text == "=") return TGX_PRED_EQ;
    if (t.text == "<") return TGX_PRED_LT;
    if (t.text == "<=") return TGX_PRED_LE;
    if (t.text == ">") return TGX_PRED_GT;
    if (t.text == ">=") return TGX_PRED_GE;
    if (t.text == "<>" || t.text == "!=") return 6;
    return 0;
  }
  static int turned(int op) {
    return op == TGX_PRED_LT ? TGX_PRED_GT : op == TGX_PRED_GT ? TGX_PRED_LT : op == TGX_PRED_LE ? TGX_PRED_GE
           : op == TGX_PRED_GE ? TGX_PRED_LE : op;
  }

  // -- the grammar
  // -- the atoms of the dialect string_functions
  // lenfn(col) <op> literal, op one of TGX_PRED_EQ .. TGX_PRED_GE, onto the stack
  void compare_length(const Operand &call, int op, const Operand &lit) {
    if (lit.kind == Operand::Column) refuse("a length compared with a column");
    if (lit.kind == Operand::Length || lit.kind == Operand::Trim) refuse("a length compared with a function call");
    if (lit.kind == Operand::Text) refuse("a length compared with a string literal");
    if (lit.is_double) refuse("a length compared with a float literal");
    tgx_row_predicate_leaf l = blank(TGX_PRED_STR_LENGTH, call.col);
    l.op = op;
    l.flags = call.in_bytes ? TGX_PRED_LENGTH_IN_BYTES : 0;
    l.lit_i = lit.i;
    push_leaf(l);
  }
  // TRIM(col) = / <> / != '': `op` as comparison() gives it
  void compare_trim(const Operand &call, int op, const Operand &lit) {
    if (op != TGX_PRED_EQ && op != 6) refuse("TRIM(col) under an order comparison (only = '' and <> '')");
    if (lit.kind != Operand::Text || !lit.text.empty()) refuse("TRIM(col) compared with anything but ''");
    push_leaf(blank(TGX_PRED_STR_BLANK, call.col));
    if (op == 6) emit(TGX_PRED_NOT);
  }
  // what follows lenfn(col) / TRIM(col)
  void call_atom(const Operand &a) {
    const std::string what = a.kind == Operand::Trim ? "TRIM(col)" : "a length";
    bool negated = false;
    if (keyword("IS")) refuse("IS [NOT] NULL of a function call");
    if (keyword("NOT")) {
      negated = true;
      advance();
      if (keyword("IN")) refuse("IN on " + what);
      if (!keyword("BETWEEN") || a.kind == Operand::Trim) refuse("NOT " + here() + " after " + what);
    }
    if (keyword("IN")) refuse("IN on " + what);
    if (keyword("LIKE") || keyword("ILIKE") || keyword("SIMILAR")) refuse(tok.upper + " on " + what);
    if (keyword("BETWEEN")) {
      if (a.kind == Operand::Trim) refuse("TRIM(col) compared with anything but ''");
      advance();
      const Operand lo = literal();
      if (!keyword("AND")) refuse(here() + " where BETWEEN's AND should stand");
      advance();
      const Operand hi = literal();
      compare_length(a, TGX_PRED_GE, lo);
      compare_length(a, TGX_PRED_LE, hi);
      emit(TGX_PRED_AND);
      if (negated) emit(TGX_PRED_NOT);
      return;
    }
    const int op = comparison(tok);
    if (!op) refuse(here() + " where a comparison should stand");
    advance();
    const Operand b = operand();
    if (a.kind == Operand::Trim) return compare_trim(a, op, b);
    compare_length(a, op == 6 ? TGX_PRED_EQ : op, b);
    if (op == 6) emit(TGX_PRED_NOT);
  }
  // col [NOT] LIKE 'pattern'; the token is LIKE
  void like_atom(const Operand &a, bool negated) {
    if (a.kind != Operand::Column) refuse("LIKE of a literal");
    advance();
    if (tok.kind != Token::String) refuse(here() + " where LIKE's pattern should stand (a string literal)");
    const std::string pattern = tok.text;
    advance();
    if (keyword("ESCAPE")) refuse("an ESCAPE clause");
    if (pattern.find('\\') != std::string::npos) refuse("a LIKE pattern with a backslash");
    if (tok.kind == Token::Symbol && tok.text == "||") refuse("arithmetic ('||')");
    tgx_row_predicate_leaf l = blank(TGX_PRED_STR_LIKE, a.col);
    l.lit_len = (uint32_t)pattern.size();
    l.lit_offset = pool(pattern);
    push_leaf(l);
    if (negated) emit(TGX_PRED_NOT);
  }

  void atom() {
    const Operand a = operand();
    if (a.kind == Operand::Length || a.kind == Operand::Trim) return call_atom(a);
    bool negated = false;
    if (keyword("IS")) {
      if (a.kind != Operand::Column) refuse("IS [NOT] NULL of a literal");
      advance();
      if (keyword("NOT")) {
        negated = true;
        advance();
      }
      if (!keyword("NULL")) refuse("IS " + here() + " (only IS [NOT] NULL)");
      advance();
      push_leaf(blank(TGX_PRED_IS_NULL, a.col));
      if (negated) emit(TGX_PRED_NOT);
      return;
    }
    if (keyword("NOT")) {
      negated = true;
      advance();
      if (!keyword("BETWEEN") && !keyword("IN") && !(dialect.string_functions && keyword("LIKE")))
        refuse(keyword("LIKE") || keyword("ILIKE") ? tok.upper : "NOT " + here() + " (only NOT BETWEEN and NOT IN)");
    }
    if (keyword("BETWEEN")) {
      if (a.kind != Operand::Column) refuse("BETWEEN of a literal");
      advance();
      const Operand lo = literal();
      if (!keyword("AND")) refuse(here() + " where BETWEEN's AND should stand");
      advance();
      const Operand hi = literal();
      if ((lo.kind == Operand::Text || hi.kind == Operand::Text) && !dialect.string_functions)
        refuse("a string order comparison (BETWEEN on a string literal)");
      if (lo.kind != hi.kind) refuse("a BETWEEN that mixes strings and numbers");
      compare_literal(a.col, TGX_PRED_GE, lo);
      compare_literal(a.col, TGX_PRED_LE, hi);
      emit(TGX_PRED_AND);
      if (negated) emit(TGX_PRED_NOT);
      return;
    }
    if (keyword("IN")) {
      if (a.kind != Operand::Column) refuse("IN of a literal");
      advance();
      if (!symbol("(")) refuse(here() + " where IN's '(' should stand");
      advance();
      if (keyword("SELECT")) refuse("a subquery");
      int n = 0;
      Operand::Kind kind = Operand::Number;
      for (;;) {
        const Operand lit = literal();
        if (n > 0 && lit.kind != kind) refuse("an IN list that mixes strings and numbers");
        kind = lit.kind;
        compare_literal(a.col, TGX_PRED_EQ, lit);
        if (n++ > 0) emit(TGX_PRED_OR);
        if (symbol(",")) {
          advance();
          continue;
        }
        if (!symbol(")")) refuse(here() + " in an IN list");
        advance();
        break;
      }
      if (negated) emit(TGX_PRED_NOT);
      return;
    }
    if (dialect.string_functions && keyword("LIKE")) return like_atom(a, negated);
    if (keyword("LIKE") || keyword("ILIKE") || keyword("SIMILAR")) refuse(tok.upper);
    const int op = comparison(tok);
    if (!op) refuse(here() + " where a comparison should stand");
    advance();
    const Operand b = operand();
    if (b.kind == Operand::Length || b.kind == Operand::Trim) {  // lit op call: turned round
      if (b.kind == Operand::Trim) return compare_trim(b, op, a);
      compare_length(b, op == 6 ? TGX_PRED_EQ : turned(op), a);
      if (op == 6) emit(TGX_PRED_NOT);
      return;
    }
    const int plain = op == 6 ? TGX_PRED_EQ : op;
    if (a.kind != Operand::Column && b.kind != Operand::Column) refuse("a comparison of two literals");
    if (a.kind == Operand::Column && b.kind == Operand::Column) {
      tgx_row_predicate_leaf l = blank(TGX_PRED_CMP_COLUMNS, a.col);
      l.op = plain;
      l.col2 = b.col;
      push_leaf(l);
    } else if (a.kind == Operand::Column) {
      compare_literal(a.col, plain, b);
    } else {
      compare_literal(b.col, turned(plain), a);
    }
    if (op == 6) emit(TGX_PRED_NOT);
  }

  void factor() {
    if (++nesting > 64) refuse("nesting deeper than 64");
    if (keyword("NOT")) {
      advance();
      factor();
      emit(TGX_PRED_NOT);
    } else if (symbol("(")) {
      advance();
      if (keyword("SELECT")) refuse("a subquery");
      pred();
      if (!symbol(")")) refuse(here() + " where ')' should stand");
      advance();
      if (tok.kind == Token::Symbol && (comparison(tok) || tok.text == "+" || tok.text == "-" || tok.text == "*" ||
                                        tok.text == "/" || tok.text == "%"))
        refuse("a parenthesised operand (" + here() + " after ')')");
    } else {
      atom();
    }
    nesting--;
  }
  void term() {
    factor();
    while (keyword("AND")) {
      advance();
      factor();
      emit(TGX_PRED_AND);
    }
  }
  void pred() {
    term();
    while (keyword("OR")) {
      advance();
      term();
      emit(TGX_PRED_OR);
    }
  }
};

// `word` as a whole word of `text` (\b on both sides: a word character is [A-Za-z0-9_])
bool has_word(const std::string &text, const std::string &word) {
  auto is_word = [](char c) { return isalnum((unsigned char)c) || c == '_'; };
  for (size_t at = text.find(word); at != std::string::npos; at = text.find(word, at + 1)) {
    const bool left = at == 0 || !is_word(text[at - 1]);
    const bool right = at + word.size() >= text.size() || !is_word(text[at + word.size()]);
    if (left && right) return true;
  }
  return false;
}

uint64_t bits_of(double v) {
  uint64_t b;
  memcpy(&b, &v, sizeof(b));
  return b;
}

std::string json_f64(double v) {
  char buf[64];
  snprintf(buf, sizeof(buf), "%.17g", v);
  return buf;
}

}  // namespace

RowPredicate compile_row_predicate(const std::string &expression, const PredicateDialect &dialect) {
  Compiler c(expression, dialect);
  c.pred();
  if (c.tok.kind != Token::End) refuse(c.here() + " after the end of the predicate");
  return std::move(c.out);
}

std::string row_predicate_json(const RowPredicate &p) {
  std::string o = "{\"columns\": [";
  for (size_t i = 0; i < p.columns.size(); i++) o += (i ? ", " : "") + json::quote(p.columns[i]);
  o += "], \"leaves\": [";
  for (uint32_t j = 0; j < p.params.n_leaves; j++) {
    const tgx_row_predicate_leaf &l = p.params.leaves[j];
    o += std::string(j ? ", " : "") + "{\"kind\": " + std::to_string(l.kind) + ", \"op\": " + std::to_string(l.op) +
         ", \"col\": " + std::to_string(l.col) + ", \"col2\": " + std::to_string(l.col2) + ", \"flags\": " +
         std::to_string(l.flags) + ", \"lit_offset\": " + std::to_string(l.lit_offset) + ", \"lit_len\": " +
         std::to_string(l.lit_len) + ", \"lit_i\": " + std::to_string((long long)l.lit_i) + ", \"lit_f\": " +
         json_f64(l.lit_f) + ", \"lit_f_bits\": " + std::to_string((unsigned long long)bits_of(l.lit_f)) + "}";
  }
  o += "], \"program\": [";
  for (uint32_t k = 0; k < p.params.n_ops; k++)
    o += std::string(k ? ", " : "") + "[" + std::to_string(p.params.program[k] & 255) + ", " +
         std::to_string(p.params.program[k] >> 8) + "]";
  o += "], \"literals_hex\": \"";
  static const char hex[] = "0123456789abcdef";
  for (uint32_t k = 0; k < p.params.n_literal_bytes; k++) {
    o += hex[p.params.literals[k] >> 4];
    o += hex[p.params.literals[k] & 15];
  }
  return o + "\"}";
}

SpecRequest row_predicate_request(const RowPredicate &p) {
  SpecRequest r;
  r.kind = TGX_CHECK_ROW_PREDICATE;
  r.columns = p.columns;
  r.column = p.columns.at(0);
  r.row_predicate = p.params;
  return r;
}

std::optional<std::string> custom_sql_refusal(const std::string &sql) {
  static const char *const forbidden[] = {"DROP",    "DELETE",   "INSERT", "UPDATE",   "CREATE",    "ALTER", "TRUNCATE",
                                          "GRANT",   "REVOKE",   "EXECUTE", "EXEC",    "CALL",      "MERGE", "REPLACE",
                                          "RENAME",  "MODIFY",   "SET",    "COMMIT",   "ROLLBACK",  "SAVEPOINT",
                                          "BEGIN",   "START",    "TRANSACTION", "LOCK", "UNLOCK"};
  std::string upper;
  for (char c : sql) upper += (char)toupper((unsigned char)c);  // (ASCII: the words are)
  for (const char *w : forbidden)
    if (has_word(upper, w)) return std::string("SQL expression contains forbidden operation: ") + w;
  if (sql.find(';') != std::string::npos) return std::string("SQL expression cannot contain semicolons");
  if (sql.find("--") != std::string::npos || sql.find("/*") != std::string::npos || sql.find("*/") != std::string::npos)
    return std::string("SQL expression cannot contain comments");
  return std::nullopt;
}

std::optional<std::string> compliance_forbidden_keyword(const std::string &predicate) {
  static const char *const forbidden[] = {"drop",  "delete", "insert",  "update", "create", "alter", "grant", "revoke",
                                          "exec",  "execute", "union",  "select", "--",     "/*",    "*/"};
  std::string lower;
  for (char c : predicate) lower += (char)tolower((unsigned char)c);
  for (const char *w : forbidden)
    if (lower.find(w) != std::string::npos) return std::string(w);
  return std::nullopt;
}

// ---- the constraint ----------------------------------------------------------------------------------------------------
// (tools/fuzz_predicates.cpp builds this file alone, with TGX_PREDICATE_COMPILER_ONLY: everything above stands without
//  the rest of the host layer)
#ifndef TGX_PREDICATE_COMPILER_ONLY
CustomSqlConstraint::CustomSqlConstraint(std::string expression, std::optional<std::string> hint)
    : expression_(std::move(expression)), hint_(std::move(hint)) {
  if (auto refusal = custom_sql_refusal(expression_)) throw TermError{TermError::ValidationFailed, *refusal};
}

std::vector<SpecRequest> CustomSqlConstraint::plan() const {
  try {
    return {row_predicate_request(compile_row_predicate(expression_, dialect()))};
  } catch (const PredicateRefusal &r) {
    throw TermError{TermError::ConstraintEvaluation,
                    "'custom_sql': the expression is not on the GPU path: " + r.what + ". Expression: '" + expression_ + "'"};
  }
}

std::optional<ConstraintResult> CustomSqlConstraint::failure_from_error(const std::string &error) const {
  // a column the table lacks, a leaf that does not fit its column: the reference's query fails, and its evaluate()
  // answers with a Failure that carries the error's text.  Anything else (the subset's refusal, a device error) stands
  if (error.find("Schema error: No field named") == std::string::npos && error.find("TGX_UNSUPPORTED") == std::string::npos)
    return std::nullopt;
  return ConstraintResult::failure("SQL expression error: " + error + ". Expression: '" + expression_ + "'");
}

ConstraintResult CustomSqlConstraint::evaluate(const Inputs &in) const {
  // a CMP_LITERAL on a column declared temporal, decimal, boolean or binary: DataFusion coerces the literal to the
  // column's type (or fails to); the device compares the column's integers with the number as written
  if (!in.list_arrow_types.empty()) {
    RowPredicate p;
    try {
      p = compile_row_predicate(expression_, dialect());
    } catch (const PredicateRefusal &) {
      return plan(), ConstraintResult::success();  // (plan() throws the refusal)
    }
    const std::vector<std::string> &types = in.list_arrow_types[0];
    for (size_t c = 0; c < p.columns.size() && c < types.size(); c++) {
      if (!p.literal_compared[c]) continue;
      static const char *const refused[] = {"Date", "Time", "Timestamp", "Duration", "Interval", "Decimal", "Boolean",
                                            "Binary", "LargeBinary", "FixedSizeBinary", "BinaryView"};
      for (const char *t : refused)
        if (types[c].compare(0, strlen(t), t) == 0)
          return ConstraintResult::failure("SQL expression error: column '" + p.columns[c] + "' is declared " + types[c] +
                                           ", and comparing such a column with a numeric literal is not on the GPU "
                                           "path. Expression: '" + expression_ + "'");
    }
  }
  const tgx_result &r = *in.results.at(0);  // total = rows seen, matches = satisfied
  if (r.total == 0) return ConstraintResult::skipped("No data to validate");
  const double satisfied = (double)r.matches, total = (double)r.total;
  const double ratio = satisfied / total;
  if (ratio == 1.0) return ConstraintResult::success_with_metric(ratio);
  const long long failed = (long long)(total - satisfied);
  if (hint_)
    return ConstraintResult::failure_with_metric(ratio, *hint_ + " (" + std::to_string(failed) + " rows failed the condition)");
  return ConstraintResult::failure_with_metric(ratio, "Custom SQL condition not satisfied for " + std::to_string(failed) +
                                                          " rows. Expression: '" + expression_ + "'");
}

std::vector<std::pair<std::string, std::string>> CustomSqlConstraint::metadata() const {
  std::vector<std::pair<std::string, std::string>> m = {
      {"description", description()}, {"expression", expression_}, {"constraint_type", "custom"}};
  if (hint_) m.push_back({"hint", *hint_});
  return m;
}

Check::Builder &Check::Builder::satisfies(std::string sql_expression, std::optional<std::string> hint,
                                          bool string_functions_on_device) {
  auto c = std::make_shared<CustomSqlConstraint>(std::move(sql_expression), std::move(hint));
  c->string_functions_on_device(string_functions_on_device);
  return constraint(std::move(c));
}
#endif  // TGX_PREDICATE_COMPILER_ONLY

}  // namespace term_guard
