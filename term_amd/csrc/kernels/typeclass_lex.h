// typeclass_lex.h -- the classifier of TGX_CHECK_TYPE_CLASSES: one value's bytes into one of seven syntactic classes
// (include/tgx.h has the contract; the reference's DataTypeAnalyzer, TG/analyzers/advanced/data_type.rs:129-150, is the
// query it stands in for).  One function, type_class_of, templated on how a byte of the value is fetched, so the same
// state machine is compiled into the kernels (kernels/typeclass.hip), into the host library (tgx_host_type_class) and
// into the stand-alone fuzzer (tools/fuzz_type_classes.cpp).
//
// The classes are tried in the contract's order and the first that fits wins, but no value is read twice: the first
// byte picks the grammars that are still live (a letter: BOOLEAN or a DOUBLE special; a digit, a sign or a point: the
// numeric and the calendar grammars), and reading stops at the first byte that kills them all.  Free text is STRING
// from its first byte or two; only DOUBLE reads a long value to its end.  There are no tables and no arrays: month
// lengths come out of one packed constant, the leap rule divides by constants, an Int32 is ten digits in 64 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TGX_LEX_FN __host__ __device__ inline
#else
#define TGX_LEX_FN inline
#endif

namespace tgx {

// the classes, in the order of the counters of tgx_type_classes_counts behind `non_null`
enum TypeClassCode : int {
  kTcBoolean = 0,
  kTcInteger = 1,
  kTcDouble = 2,
  kTcDate = 3,
  kTcDatetime = 4,
  kTcString = 5,
  kTcUndecided = 6,
  kTypeClassCount = 7
};

// a value whose bytes lie in host memory
struct TcByteFetch {
  const uint8_t *p;
  TGX_LEX_FN uint8_t operator()(uint64_t i) { return p[i]; }
};

namespace tc {

TGX_LEX_FN bool digit(uint32_t c) { return c - (uint32_t)'0' <= 9u; }
TGX_LEX_FN uint32_t fold(uint32_t c) { return c - (uint32_t)'A' <= 25u ? c + 32u : c; }  // ASCII only: 0x80.. stay

// bytes [at, at + n) against the lower-case word packed into `word`, first letter in the low byte (n <= 8)
template <class Fetch>
TGX_LEX_FN bool word_is(Fetch &f, uint64_t at, int n, uint64_t word) {
  for (int k = 0; k < n; k++)
    if (fold(f(at + (uint64_t)k)) != (uint32_t)((word >> (8 * k)) & 255u)) return false;
  return true;
}

constexpr uint64_t pack(const char *s, int n) {
  uint64_t w = 0;
  for (int k = 0; k < n; k++) w |= (uint64_t)(uint8_t)s[k] << (8 * k);
  return w;
}

// the rest of the value from `at` on: nan | inf | infinity, in any ASCII case
template <class Fetch>
TGX_LEX_FN bool special(Fetch &f, uint64_t at, uint64_t len) {
  const uint64_t n = len - at;
  if (n == 3) {
    const uint32_t c = fold(f(at));
    return c == 'n' ? word_is(f, at, 3, pack("nan", 3)) : c == 'i' && word_is(f, at, 3, pack("inf", 3));
  }
  return n == 8 && word_is(f, at, 8, pack("infinity", 8));
}

// a day of the proleptic Gregorian calendar, years 0 .. 9999 (year 0 is a leap year)
TGX_LEX_FN bool valid_date(uint32_t y, uint32_t m, uint32_t d) {
  if (m < 1 || m > 12 || d < 1) return false;
  // days beyond 28, two bits a month from bit 2 on: 3 0 3 2 3 2 3 3 2 3 2 3
  uint32_t days = 28u + ((0x3BBEECCu >> (2 * m)) & 3u);
  const bool leap = y % 4u == 0 && (y % 100u != 0 || y % 400u == 0);
  if (m == 2 && leap) days = 29;
  return d <= days;
}

// two digits at `at` as a number, or 100
template <class Fetch>
TGX_LEX_FN uint32_t two_digits(Fetch &f, uint64_t at) {
  const uint32_t a = f(at), b = f(at + 1);
  return digit(a) && digit(b) ? (a - '0') * 10u + (b - '0') : 100u;
}

// a value that begins DDDD- (year `y`): DATE, DATETIME or UNDECIDED
template <class Fetch>
TGX_LEX_FN int calendar(Fetch &f, uint64_t len, uint32_t y) {
  if (len <= 10) {  // DDDD-D{1,2}-D{1,2}
    uint64_t i = 5;
    uint32_t m = 0, d = 0;
    int nm = 0, nd = 0;
    while (i < len && nm < 2 && digit(f(i))) m = m * 10u + (f(i++) - '0'), nm++;
    if (nm == 0 || i >= len || f(i) != '-') return kTcUndecided;
    i++;
    while (i < len && nd < 2 && digit(f(i))) d = d * 10u + (f(i++) - '0'), nd++;
    if (nd == 0 || i != len) return kTcUndecided;
    return valid_date(y, m, d) ? kTcDate : kTcUndecided;
  }
  // DDDD-DD-DD, T or a space, hh:mm:ss, then [.D{1,9}] [Z | [+-]hh:mm]
  if (len < 19 || f(7) != '-') return kTcUndecided;
  if (!valid_date(y, two_digits(f, 5), two_digits(f, 8))) return kTcUndecided;  // (100: no month, no day)
  if (f(10) != 'T' && f(10) != ' ') return kTcUndecided;
  if (f(13) != ':' || f(16) != ':') return kTcUndecided;
  if (two_digits(f, 11) > 23 || two_digits(f, 14) > 59 || two_digits(f, 17) > 59) return kTcUndecided;
  uint64_t i = 19;
  if (i < len && f(i) == '.') {
    i++;
    int nf = 0;
    while (i < len && nf < 10 && digit(f(i))) i++, nf++;
    if (nf < 1 || nf > 9) return kTcUndecided;
  }
  if (i == len) return kTcDatetime;
  const uint32_t z = f(i);
  if (z == 'Z') return i + 1 == len ? kTcDatetime : kTcUndecided;
  if ((z != '+' && z != '-') || len - i != 6 || f(i + 3) != ':') return kTcUndecided;
  return two_digits(f, i + 1) <= 23 && two_digits(f, i + 4) <= 59 ? kTcDatetime : kTcUndecided;
}

}  // namespace tc

// the class of the value whose byte i (0 <= i < len) is f(i); f is asked for no other byte
template <class Fetch>
TGX_LEX_FN int type_class_of(Fetch &f, uint64_t len) {
  using namespace tc;
  if (len == 0) return kTcString;
  const uint32_t c0 = f(0);
  const uint32_t l0 = fold(c0);
  if (l0 == 't') return len == 4 && word_is(f, 0, 4, pack("true", 4)) ? kTcBoolean : kTcString;
  if (l0 == 'f') return len == 5 && word_is(f, 0, 5, pack("false", 5)) ? kTcBoolean : kTcString;
  if (l0 == 'n' || l0 == 'i') return special(f, 0, len) ? kTcDouble : kTcString;
  const bool sign = c0 == '+' || c0 == '-';
  if (!sign && !digit(c0) && c0 != '.') return kTcString;
  uint64_t i = sign ? 1 : 0;
  if (i == len) return kTcString;
  if (sign) {
    const uint32_t l1 = fold(f(1));
    if (l1 == 'n' || l1 == 'i') return special(f, 1, len) ? kTcDouble : kTcString;
  }
  // the integer part: its digits counted, the first ten of them as a number
  const uint64_t first = i;
  uint64_t value = 0;
  uint32_t lead = 0;
  while (i < len) {
    const uint32_t c = f(i);
    if (!digit(c)) break;
    if (i == first) lead = c;
    if (i - first < 10) value = value * 10u + (c - '0');
    i++;
  }
  const uint64_t nd = i - first;
  if (i == len) {  // [+-]?D+
    if (len == 1 && value <= 1) return kTcBoolean;
    // the canonical text of an Int32: 0 | -?[1-9]D*, within range
    const bool canonical = c0 != '+' && (lead != '0' || len == 1);
    const bool fits = nd <= 10 && value <= (c0 == '-' ? 2147483648ull : 2147483647ull);
    return canonical && fits ? kTcInteger : kTcDouble;
  }
  uint32_t c = f(i);
  if (c == '-' && (sign ? nd >= 4 : nd == 4)) return sign ? kTcUndecided : calendar(f, len, (uint32_t)value);
  // DOUBLE: [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?
  uint64_t mantissa = nd;
  if (c == '.') {
    i++;
    while (i < len && digit(f(i))) i++, mantissa++;
    if (mantissa == 0) return kTcString;
    if (i == len) return kTcDouble;
    c = f(i);
  }
  if (mantissa == 0 || (c != 'e' && c != 'E')) return kTcString;
  i++;
  if (i < len && (f(i) == '+' || f(i) == '-')) i++;
  if (i == len) return kTcString;
  while (i < len && digit(f(i))) i++;
  return i == len ? kTcDouble : kTcString;
}

}  // namespace tgx
