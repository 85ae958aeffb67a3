// fuzz_string_predicates.cpp -- seeded random and mutated (pattern, value) pairs through the string leaves of
// TGX_CHECK_ROW_PREDICATE (term_amd/csrc/kernels/string_leaf.h): STR_CMP, STR_LENGTH, STR_LIKE and STR_BLANK read bytes
// users hand in, a word at a time.
//
// A stand-alone host program: no device, no HIP, nothing of the library but that header.  Build it with the sanitizers
// and run it on a CPU machine:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/fuzz_string_predicates.cpp -o fuzz_string_predicates && ./fuzz_string_predicates [cases] [seed]
//
// Every case is one pattern and one value: drawn byte by byte from an alphabet dense in `%`, `_`, blanks and the bytes
// of multi-byte characters (lead and continuation bytes on their own too: the leaves take bytes, not UTF-8), or one of
// the seeds below with bytes set, dropped, inserted or doubled; now and then the pattern is made from the value, so that
// matches are common.  Both are copied into heap buffers of EXACTLY their length, so a read past either trips
// AddressSanitizer; the value goes through the four functions at all four word alignments (SlHostFetch puts the words
// together from the value's own bytes and fills what lies beside them with 0xFF) and every answer is compared with a
// second, plain statement of the contract's rules (include/tgx.h) in this file: LIKE as a table over (pattern position,
// text position), the rest a byte at a time.
// Exit status 0: every case ran clean and both agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../term_amd/csrc/kernels/string_leaf.h"

using namespace tgx;

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

// ---- the rules, stated plainly ----------------------------------------------------------------------------------------
bool is_cont(unsigned char b) { return (b & 0xC0) == 0x80; }

long plain_characters(const std::string &v) {
  long n = 0;
  for (unsigned char b : v) n += !is_cont(b);
  return n;
}

bool plain_blank(const std::string &v) {
  for (unsigned char b : v)
    if (b != 0x20) return false;
  return true;
}

// < 0, 0, > 0: the first differing byte decides as unsigned; a proper prefix is smaller
int plain_order(const std::string &a, const std::string &b) {
  for (size_t i = 0; i < a.size() && i < b.size(); i++)
    if (a[i] != b[i]) return (unsigned char)a[i] < (unsigned char)b[i] ? -1 : 1;
  return a.size() < b.size() ? -1 : a.size() > b.size() ? 1 : 0;
}

bool plain_compare(int op, long a, long b) {
  switch (op) {
    case sl::kEq: return a == b;
    case sl::kLt: return a < b;
    case sl::kLe: return a <= b;
    case sl::kGt: return a > b;
    default: return a >= b;
  }
}

// m[p][t]: the pattern from p on matches the text from t on.  `%`: any run of bytes; `_`: from a unit's first byte (a
// byte that is no continuation byte, or offset 0) through every continuation byte behind it; any other byte: itself
bool plain_like(const std::string &pat, const std::string &v) {
  const size_t P = pat.size(), N = v.size();
  std::vector<std::vector<char>> m(P + 1, std::vector<char>(N + 1, 0));
  m[P][N] = 1;
  for (size_t p = P; p-- > 0;)
    for (size_t t = N + 1; t-- > 0;) {
      bool ok = false;
      if (pat[p] == '%') {
        ok = m[p + 1][t] || (t < N && m[p][t + 1]);
      } else if (t < N) {
        if (pat[p] == '_') {
          if (t == 0 || !is_cont((unsigned char)v[t])) {
            size_t e = t + 1;
            while (e < N && is_cont((unsigned char)v[e])) e++;
            ok = m[p + 1][e];
          }
        } else {
          ok = pat[p] == v[t] && m[p + 1][t + 1];
        }
      }
      m[p][t] = ok;
    }
  return m[0][0];
}

// ---- the values -------------------------------------------------------------------------------------------------------
const char kAlphabet[] = "aab %%__ \n\xc3\xa9\xe6\x97\xa5\x80\xf0\x9f";
const char *const kSeeds[] = {"", "a", "ab", "aaa", "aaaa", "aaab", "%", "%%", "_", "a%", "%a", "%a%", "a%b", "a_c", "_%", "%_",
                              "__%", "%aa%aa%", "a%ab", "    ", "   \t", "\xe6\x97\xa5\xe6\x9c\xac\xe8\xaa\x9e",
                              "%\xe6\x97\xa5_\xe8\xaa\x9e%", "x\ny", "x_y", "\xc3\xa9\xc3\xa9\xc3\xa9", "\x80", "\x80\x80", "a\x80",
                              "\xe6\x97", "1998-09-01", "1998-09", "bob@competitor.com", "%@competitor.com",
                              "abcdefghijklmnopqrstuvwxyz0123456789abcdefghijklmnopqrstuvwxyz"};

std::string draw(Rng &rng) {
  const int n_alpha = (int)sizeof(kAlphabet) - 1, n_seeds = (int)(sizeof(kSeeds) / sizeof(kSeeds[0]));
  std::string v;
  if (rng.below(100) < 45) {
    const int n = rng.below(rng.below(4) ? 10 : 40);
    for (int i = 0; i < n; i++) v += kAlphabet[rng.below(n_alpha)];
    return v;
  }
  v = kSeeds[rng.below(n_seeds)];
  const int edits = rng.below(4);
  for (int e = 0; e < edits; e++) {
    const size_t at = (size_t)rng.below((int)v.size() + 1);
    switch (rng.below(4)) {
      case 0:
        if (at < v.size()) v[at] = kAlphabet[rng.below(n_alpha)];
        break;
      case 1:
        if (at < v.size()) v.erase(at, 1);
        break;
      case 2:
        v.insert(at, 1, kAlphabet[rng.below(n_alpha)]);
        break;
      default:
        if (at < v.size()) v.insert(at, 1, v[at]);
        break;
    }
  }
  return v;
}

// a pattern that has a chance: the value with stretches replaced by `%` and bytes by `_`
std::string pattern_of(Rng &rng, const std::string &v) {
  std::string p;
  for (size_t i = 0; i < v.size();) {
    const int r = rng.below(10);
    if (r < 3) {
      p += '%';
      i += 1 + (size_t)rng.below(3);
    } else if (r < 5) {
      p += '_';
      i++;
    } else {
      p += v[i++];
    }
  }
  if (rng.below(2)) p.insert((size_t)rng.below((int)p.size() + 1), 1, '%');
  return p;
}

uint8_t *exact_copy(const std::string &s) {
  uint8_t *p = (uint8_t *)malloc(s.size() ? s.size() : 1);
  if (!p) exit(2);
  if (!s.empty()) memcpy(p, s.data(), s.size());
  return p;
}

void show(const char *what, const std::string &s) {
  fprintf(stderr, "%s \"", what);
  for (unsigned char ch : s) fprintf(stderr, ch >= 0x20 && ch < 0x7f ? "%c" : "\\x%02x", ch);
  fprintf(stderr, "\" (%zu bytes)", s.size());
}

}  // namespace

int main(int argc, char **argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 300000;
  Rng rng{argc > 2 ? strtoull(argv[2], nullptr, 10) | 1 : 0x9e3779b97f4a7c15ull};
  long like_true = 0, like_false = 0, blank_true = 0;
  for (long c = 0; c < cases; c++) {
    const std::string v = draw(rng);
    std::string pat = rng.below(3) ? pattern_of(rng, v) : draw(rng);
    for (char &ch : pat)
      if (ch == '\\') ch = '/';  // (the setter refuses a backslash: there is no escape)
    const int op = 1 + rng.below(5), order_op = 2 + rng.below(4);
    const long lit = rng.below(12) - 1;
    uint8_t *value = exact_copy(v), *pattern = exact_copy(pat);
    const bool want_like = plain_like(pat, v), want_blank = plain_blank(v);
    const bool want_chars = plain_compare(op, plain_characters(v), lit), want_bytes = plain_compare(op, (long)v.size(), lit);
    const bool want_order = plain_compare(order_op, plain_order(v, pat), 0);
    for (uint32_t shift = 0; shift < 4; shift++) {
      SlHostFetch f{value, v.size(), shift};
      const bool got_like = sl::like(f, v.size(), pattern, (uint32_t)pat.size(), sl::like_min_len(pattern, (uint32_t)pat.size()));
      const bool got_blank = sl::blank(f, v.size());
      const bool got_chars = sl::length(f, v.size(), (uint32_t)op, lit, false);
      const bool got_bytes = sl::length(f, v.size(), (uint32_t)op, lit, true);
      const bool got_order = sl::order(f, v.size(), (uint32_t)order_op, pattern, (uint32_t)pat.size());
      if (got_like != want_like || got_blank != want_blank || got_chars != want_chars || got_bytes != want_bytes ||
          got_order != want_order) {
        fprintf(stderr, "case %ld, alignment %u: ", c, shift);
        show("value", v);
        show(", pattern", pat);
        fprintf(stderr, ": like %d (plain %d), blank %d (%d), length op %d lit %ld: %d (%d), bytes %d (%d), order op %d: %d (%d)\n",
                got_like, want_like, got_blank, want_blank, op, lit, got_chars, want_chars, got_bytes, want_bytes, order_op,
                got_order, want_order);
        return 1;
      }
    }
    free(value);
    free(pattern);
    like_true += want_like;
    like_false += !want_like;
    blank_true += want_blank;
  }
  printf("fuzz_string_predicates: %ld cases clean at 4 alignments each (LIKE true %ld, false %ld; blank %ld)\n", cases, like_true,
         like_false, blank_true);
  return 0;
}
