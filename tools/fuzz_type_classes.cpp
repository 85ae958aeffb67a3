// fuzz_type_classes.cpp -- seeded random and mutated values through the lexer of TGX_CHECK_TYPE_CLASSES
// (term_amd/csrc/kernels/typeclass_lex.h): the state machine the kernels compile reads bytes users hand in.
//
// A stand-alone host program: no device, no HIP, nothing of the library but that header.  Build it with the sanitizers
// and run it on a CPU machine:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//         tools/fuzz_type_classes.cpp -o fuzz_type_classes && ./fuzz_type_classes [cases] [seed]
//
// Every case is one value: drawn byte by byte from an alphabet dense in the bytes the grammars turn on, or one of the
// seed values below with bytes set, dropped, inserted or doubled.  The value is copied into a heap buffer of EXACTLY its
// length, so a read past `len` trips AddressSanitizer; it goes through type_class_of with the byte fetcher and is
// compared with a second, plain statement of the contract's seven rules (include/tgx.h) in this file: one predicate a
// class, tried in order, each reading the whole value on its own.
// Exit status 0: every case ran clean and both agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../term_amd/csrc/kernels/typeclass_lex.h"

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

// ---- the seven rules, stated plainly --------------------------------------------------------------------------------
bool is_digit(char c) { return c >= '0' && c <= '9'; }
bool all_digits(const std::string &s) {
  if (s.empty()) return false;
  for (char c : s)
    if (!is_digit(c)) return false;
  return true;
}
std::string lower(std::string s) {
  for (char &c : s)
    if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
  return s;
}
bool leap(int y) { return y % 4 == 0 && (y % 100 != 0 || y % 400 == 0); }
bool valid_date(int y, int m, int d) {
  static const int days[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  if (m < 1 || m > 12 || d < 1) return false;
  return d <= (m == 2 && leap(y) ? 29 : days[m - 1]);
}

bool rule_boolean(const std::string &v) { return v == "0" || v == "1" || lower(v) == "true" || lower(v) == "false"; }

bool rule_integer(const std::string &v) {
  const bool neg = !v.empty() && v[0] == '-';
  const std::string body = neg ? v.substr(1) : v;
  if (!all_digits(body)) return false;
  if (body == "0") return !neg;
  if (body[0] == '0' || body.size() > 10) return false;
  const long long n = atoll(body.c_str());
  return neg ? n <= 2147483648ll : n <= 2147483647ll;
}

bool rule_double(const std::string &v) {
  size_t i = (!v.empty() && (v[0] == '+' || v[0] == '-')) ? 1 : 0;
  const std::string rest = lower(v.substr(i));
  if (rest == "nan" || rest == "inf" || rest == "infinity") return true;
  size_t j = 0, n_int = 0, n_frac = 0;
  while (j < rest.size() && is_digit(rest[j])) j++, n_int++;
  if (j < rest.size() && rest[j] == '.') {
    j++;
    while (j < rest.size() && is_digit(rest[j])) j++, n_frac++;
  }
  if (n_int + n_frac == 0) return false;
  if (j == rest.size()) return true;
  if (rest[j] != 'e') return false;
  j++;
  if (j < rest.size() && (rest[j] == '+' || rest[j] == '-')) j++;
  return all_digits(rest.substr(j));
}

bool rule_date(const std::string &v) {
  if (v.size() > 10) return false;
  const size_t a = v.find('-'), b = a == std::string::npos ? a : v.find('-', a + 1);
  if (a != 4 || b == std::string::npos || v.find('-', b + 1) != std::string::npos) return false;
  const std::string y = v.substr(0, 4), m = v.substr(5, b - 5), d = v.substr(b + 1);
  if (!all_digits(y) || !all_digits(m) || !all_digits(d) || m.size() > 2 || d.size() > 2) return false;
  return valid_date(atoi(y.c_str()), atoi(m.c_str()), atoi(d.c_str()));
}

int two(const std::string &v, size_t at) {
  return at + 2 <= v.size() && is_digit(v[at]) && is_digit(v[at + 1]) ? (v[at] - '0') * 10 + (v[at + 1] - '0') : -1;
}

bool rule_datetime(const std::string &v) {
  if (v.size() <= 10 || v.size() < 19) return false;
  if (!all_digits(v.substr(0, 4)) || v[4] != '-' || v[7] != '-' || two(v, 5) < 0 || two(v, 8) < 0) return false;
  if (!valid_date(atoi(v.substr(0, 4).c_str()), two(v, 5), two(v, 8))) return false;
  if (v[10] != 'T' && v[10] != ' ') return false;
  if (v[13] != ':' || v[16] != ':') return false;
  const int hh = two(v, 11), mm = two(v, 14), ss = two(v, 17);
  if (hh < 0 || mm < 0 || ss < 0 || hh > 23 || mm > 59 || ss > 59) return false;
  std::string rest = v.substr(19);
  if (!rest.empty() && rest[0] == '.') {
    size_t k = 1;
    while (k < rest.size() && is_digit(rest[k])) k++;
    if (k - 1 < 1 || k - 1 > 9) return false;
    rest = rest.substr(k);
  }
  if (rest.empty() || rest == "Z") return true;
  if (rest.size() != 6 || (rest[0] != '+' && rest[0] != '-') || rest[3] != ':') return false;
  const int oh = two(rest, 1), om = two(rest, 4);
  return oh >= 0 && om >= 0 && oh <= 23 && om <= 59;
}

bool rule_undecided(const std::string &v) {
  if (v.size() >= 5 && all_digits(v.substr(0, 4)) && v[4] == '-') return true;
  if (!v.empty() && (v[0] == '+' || v[0] == '-')) {
    size_t k = 1;
    while (k < v.size() && is_digit(v[k])) k++;
    return k - 1 >= 4 && k < v.size() && v[k] == '-';
  }
  return false;
}

int plain_class(const std::string &v) {
  if (rule_boolean(v)) return kTcBoolean;
  if (rule_integer(v)) return kTcInteger;
  if (rule_double(v)) return kTcDouble;
  if (rule_date(v)) return kTcDate;
  if (rule_datetime(v)) return kTcDatetime;
  if (rule_undecided(v)) return kTcUndecided;
  return kTcString;
}

// ---- the values -------------------------------------------------------------------------------------------------------
const char kAlphabet[] = "0123456789+-.eE:TtZz naifrulsy\xc3";
const char *const kSeeds[] = {
    "0", "1", "-1", "-0", "+5", "007", "2147483647", "2147483648", "-2147483648", "-2147483649", "true", "FALSE", "tRuE",
    "1.", ".5", "1e5", "1E+5", "+.5e-3", "nan", "-NaN", "+inf", "Infinity", "infinit", "2023-01-01", "2023-1-5",
    "2024-02-29", "1900-02-29", "0000-02-29", "2023-13-01", "2023-1-", "2023-01-01T00:00:00",
    "2023-01-01 23:59:59.123456789Z", "2023-01-01T24:00:00", "2023-01-01T10:00", "2023-01-01T10:00:00+05:30",
    "2023-01-01T10:00:00+0530", "2023-01-01X", "+10999-12-31", "5551-234", "1234", "12-34", "", "9999999999",
    "12345678901234567890123456789012345678901234567890.5e-300"};

std::string draw(Rng &rng) {
  const int n_alpha = (int)sizeof(kAlphabet) - 1, n_seeds = (int)(sizeof(kSeeds) / sizeof(kSeeds[0]));
  std::string v;
  if (rng.below(100) < 35) {
    const int n = rng.below(24);
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

}  // namespace

int main(int argc, char **argv) {
  const long cases = argc > 1 ? atol(argv[1]) : 1000000;
  Rng rng{argc > 2 ? strtoull(argv[2], nullptr, 10) | 1 : 0x9e3779b97f4a7c15ull};
  long per_class[kTypeClassCount] = {0};
  for (long c = 0; c < cases; c++) {
    const std::string v = draw(rng);
    // an exact-size heap copy: byte v.size() is not the value's
    uint8_t *exact = (uint8_t *)malloc(v.size() ? v.size() : 1);
    if (!exact) return 2;
    if (!v.empty()) memcpy(exact, v.data(), v.size());
    TcByteFetch f{v.empty() ? nullptr : exact};
    const int got = type_class_of(f, v.size());
    free(exact);
    const int want = plain_class(v);
    if (got != want || got < 0 || got >= kTypeClassCount) {
      fprintf(stderr, "case %ld: value \"", c);
      for (unsigned char ch : v) fprintf(stderr, ch >= 0x20 && ch < 0x7f ? "%c" : "\\x%02x", ch);
      fprintf(stderr, "\" (%zu bytes): the lexer says class %d, the plain rules say %d\n", v.size(), got, want);
      return 1;
    }
    per_class[got]++;
  }
  printf("fuzz_type_classes: %ld cases clean (boolean %ld, integer %ld, double %ld, date %ld, datetime %ld, string %ld, "
         "undecided %ld)\n",
         cases, per_class[0], per_class[1], per_class[2], per_class[3], per_class[4], per_class[5], per_class[6]);
  return 0;
}
