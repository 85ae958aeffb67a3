// string_leaf.h -- the four string leaves of TGX_CHECK_ROW_PREDICATE that read a value's bytes beyond equality:
// STR_CMP, STR_LENGTH, STR_LIKE and STR_BLANK (include/tgx.h has the contract).  Each is one function templated on how
// the value is fetched, so the same code is compiled into the kernel (kernels/rowpredicate.hip, through word_fetch.h's
// TcWordFetch), into the host library (tgx_host_string_leaf) and into the stand-alone fuzzer
// (tools/fuzz_string_predicates.cpp).
//
// A fetch `f` answers three questions about the value's bytes [0, len):
//     f(i)          byte i
//     f.misalign()  m in 0 .. 3: how far byte 0 lies into its naturally aligned 32-bit word
//     f.word(k)     the k-th aligned word counted from the one that holds byte 0: its byte j is the value's byte
//                   4k + j - m where that lies in [0, len), and of no account elsewhere.  Only words that hold a byte of
//                   the value are asked for: k < sl::words(m, len).
// The literal of STR_CMP and the pattern of STR_LIKE are plain bytes behind a pointer (LDS in the kernel).
//
// No function here recurses, keeps an array or writes memory.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TGX_SL_FN __host__ __device__ inline
#else
#define TGX_SL_FN inline
#endif

namespace tgx {

// a value whose bytes lie in host memory, seen as if byte 0 lay `shift` bytes into its word: the words are put together
// from the value's own bytes, and what a word holds beside them is 0xFF (a caller that forgets to mask shows)
struct SlHostFetch {
  const uint8_t *p;
  uint64_t len;
  uint32_t shift;
  TGX_SL_FN uint8_t operator()(uint64_t i) const { return p[i]; }
  TGX_SL_FN uint32_t misalign() const { return shift; }
  TGX_SL_FN uint32_t word(uint64_t k) const {
    uint32_t w = 0;
    for (uint32_t j = 0; j < 4; j++) {
      const uint64_t at = 4 * k + j;  // (+ shift: the value's byte at - shift)
      const uint32_t b = at >= shift && at - shift < len ? p[at - shift] : 0xFFu;
      w |= b << (8 * j);
    }
    return w;
  }
};

namespace sl {

enum { kEq = 1, kLt = 2, kLe = 3, kGt = 4, kGe = 5 };  // TGX_PRED_EQ ..

TGX_SL_FN bool compare(uint32_t op, int64_t a, int64_t b) {
  const bool lt = a < b, eq = a == b;
  return op == kEq ? eq : op == kLt ? lt : op == kLe ? (lt || eq) : op == kGt ? !(lt || eq) : !lt;
}

TGX_SL_FN bool continuation(uint32_t byte) { return (byte & 0xC0u) == 0x80u; }  // 10xxxxxx

TGX_SL_FN uint32_t popcount32(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// the aligned words that hold a byte of a value of `len` bytes whose byte 0 lies m bytes into its word
TGX_SL_FN uint64_t words(uint32_t m, uint64_t len) { return len ? (len + m + 3) / 4 : 0; }

// bit 7 of every byte of word k that is a byte of the value
TGX_SL_FN uint32_t inside(uint32_t m, uint64_t len, uint64_t k) {
  uint32_t mask = 0x80808080u;
  if (k == 0) mask &= 0xFFFFFFFFu << (8 * m);
  const uint64_t end = (uint64_t)m + len - 4 * k;  // the word's bytes [.., end) are the value's; end >= 1
  if (end < 4) mask &= 0xFFFFFFFFu >> (8 * (4 - (uint32_t)end));
  return mask;
}

// ---- STR_LENGTH ----------------------------------------------------------------------------------------------------
// the bytes of the value that are not 10xxxxxx: a word at a time, the head and the tail word masked to the value
template <class Fetch>
TGX_SL_FN uint64_t characters(Fetch &f, uint64_t len) {
  const uint32_t m = f.misalign();
  const uint64_t n = words(m, len);
  uint64_t count = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint32_t w = f.word(k);
    const uint32_t cont = w & ~(w << 1) & 0x80808080u;  // bit 7 set and bit 6 clear
    count += popcount32(~cont & inside(m, len, k));
  }
  return count;
}

// len(col) <op> lit; in_bytes: no byte of the value is read
template <class Fetch>
TGX_SL_FN bool length(Fetch &f, uint64_t len, uint32_t op, int64_t lit, bool in_bytes) {
  return compare(op, (int64_t)(in_bytes ? len : characters(f, len)), lit);
}

// ---- STR_BLANK -----------------------------------------------------------------------------------------------------
// every byte of the value is 0x20 (the empty value too)
template <class Fetch>
TGX_SL_FN bool blank(Fetch &f, uint64_t len) {
  const uint32_t m = f.misalign();
  const uint64_t n = words(m, len);
  for (uint64_t k = 0; k < n; k++) {
    const uint32_t in = inside(m, len, k);
    const uint32_t bytes = in | (in >> 1) | (in >> 2) | (in >> 3) | (in >> 4) | (in >> 5) | (in >> 6) | (in >> 7);
    if ((f.word(k) ^ 0x20202020u) & bytes) return false;
  }
  return true;
}

// ---- STR_CMP -------------------------------------------------------------------------------------------------------
// the value's bytes [i, i + 4) (i a multiple of 4, i < len), byte i lowest; those at or beyond len are of no account
template <class Fetch>
TGX_SL_FN uint32_t chunk(Fetch &f, uint64_t len, uint64_t i) {
  const uint32_t m = f.misalign();
  const uint64_t k = i / 4;
  const uint32_t lo = f.word(k);
  if (m == 0) return lo;
  uint32_t out = lo >> (8 * m);
  if (4 * (k + 1) < (uint64_t)m + len) out |= f.word(k + 1) << (32 - 8 * m);  // (word k + 1 holds a byte of the value)
  return out;
}

TGX_SL_FN uint32_t byte_swap(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}

// col <op> lit[0 .. lit_len), op one of LT / LE / GT / GE: bytewise, the first differing byte decides as unsigned, a
// proper prefix is smaller.  Word-wise up to the shorter length, then the lengths
template <class Fetch, class Bytes>
TGX_SL_FN bool order(Fetch &f, uint64_t len, uint32_t op, Bytes lit, uint32_t lit_len) {
  const uint64_t common = len < (uint64_t)lit_len ? len : (uint64_t)lit_len;
  for (uint64_t i = 0; i < common; i += 4) {
    const uint32_t n = common - i < 4 ? (uint32_t)(common - i) : 4u;
    uint32_t a = chunk(f, len, i), b = 0;
    for (uint32_t j = 0; j < n; j++) b |= (uint32_t)lit[i + j] << (8 * j);
    if (n < 4) a &= 0xFFFFFFFFu >> (8 * (4 - n));
    if (a != b) return compare(op, (int64_t)byte_swap(a), (int64_t)byte_swap(b));  // (the first byte highest)
  }
  return compare(op, (int64_t)len, (int64_t)lit_len);
}

// ---- STR_LIKE ------------------------------------------------------------------------------------------------------
// the pattern's bytes that are not '%': no shorter value can match
template <class Bytes>
TGX_SL_FN uint32_t like_min_len(Bytes pat, uint32_t pat_len) {
  uint32_t n = 0;
  for (uint32_t k = 0; k < pat_len; k++) n += pat[k] != (uint8_t)'%';
  return n;
}

// the first unit boundary after byte t: past t, then past every 10xxxxxx byte
template <class Fetch>
TGX_SL_FN uint64_t next_unit(Fetch &f, uint64_t len, uint64_t t) {
  t++;
  while (t < len && continuation(f(t))) t++;
  return t;
}

// col LIKE pat[0 .. pat_len) without escapes; min_len: like_min_len of the pattern.  One pass with a single restart
// point: after a mismatch behind a '%' the text resumes one unit behind the last start (only a unit's first byte can
// open what follows the '%': '_' by its definition, any byte that is not 10xxxxxx by being one) -- or one BYTE behind
// it where what follows the '%' is itself a 10xxxxxx byte, which only a pattern that is no UTF-8 holds.
template <class Fetch, class Bytes>
TGX_SL_FN bool like(Fetch &f, uint64_t len, Bytes pat, uint32_t pat_len, uint32_t min_len) {
  if (len < (uint64_t)min_len) return false;  // (no byte read)
  if (min_len == 0) return pat_len != 0 || len == 0;  // only '%'s: TRUE; the empty pattern: the empty value only
  uint64_t t = 0, restart_t = 0;
  uint32_t p = 0, restart_p = 0;
  bool restartable = false;
  for (;;) {
    if (p < pat_len && pat[p] == (uint8_t)'%') {
      p++;
      if (p == pat_len) return true;  // a trailing '%' takes the rest
      restartable = true;
      restart_p = p;
      restart_t = t;
      continue;
    }
    if (t >= len) break;
    if (p < pat_len) {
      const uint32_t c = pat[p], b = f(t);
      if (c == (uint32_t)'_') {
        if (t == 0 || !continuation(b)) {
          t = next_unit(f, len, t);
          p++;
          continue;
        }
      } else if (c == b) {
        t++;
        p++;
        continue;
      }
    }
    if (!restartable) return false;
    // (the mismatch was at a t < len and restart_t <= t: the new start is at most len)
    restart_t = continuation(pat[restart_p]) ? restart_t + 1 : next_unit(f, len, restart_t);
    t = restart_t;
    p = restart_p;
  }
  return p == pat_len;
}

}  // namespace sl
}  // namespace tgx
