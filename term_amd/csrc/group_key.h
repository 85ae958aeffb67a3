// group_key.h -- the canonical bytes of a tuple GROUP BY key on the host (include/tgx.h, TGX_CHECK_GROUP_COUNTS;
// kernels/tuple_group.h writes them on the device; term_amd/group_key.py is the Python twin).  A key is its components
// one behind the other:
//   NULL      0x00
//   integer   0x01, the 8 big-endian bytes of value ^ 2^63
//   string    0x02, the length as 2 big-endian bytes, the bytes
// Prefix-free per component, so injective for a given arity; bytewise ascending order is lexicographic by component,
// NULL before integers before strings, integers in numeric order, strings by length and then bytewise.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace tgx {

constexpr int kGroupKeyMaxArity = 8;  // the most columns a tuple key has (kMaxTupleCols)
enum GroupKeyTag { kGroupKeyNull = 0, kGroupKeyInt = 1, kGroupKeyString = 2 };
struct GroupKeyCell {
  int tag = kGroupKeyNull;
  int64_t value = 0;  // kGroupKeyInt
  std::string bytes;  // kGroupKeyString: at most 65 535 bytes
  bool operator==(const GroupKeyCell &o) const { return tag == o.tag && value == o.value && bytes == o.bytes; }
};

// false: a string cell is too long to have a form
inline bool group_key_encode(const std::vector<GroupKeyCell> &cells, std::string *out) {
  out->clear();
  for (const GroupKeyCell &c : cells) {
    out->push_back((char)c.tag);
    if (c.tag == kGroupKeyInt) {
      const uint64_t v = (uint64_t)c.value ^ 0x8000000000000000ULL;
      for (int b = 0; b < 8; b++) out->push_back((char)(uint8_t)(v >> (56 - 8 * b)));
    } else if (c.tag == kGroupKeyString) {
      if (c.bytes.size() > 0xffff) return false;
      out->push_back((char)(uint8_t)(c.bytes.size() >> 8));
      out->push_back((char)(uint8_t)c.bytes.size());
      out->append(c.bytes);
    } else if (c.tag != kGroupKeyNull) {
      return false;
    }
  }
  return true;
}

// the cells of key [p, p + n); false: the bytes are no key (an unknown tag, or a component that runs past the end).
// `out` may be nullptr: the bytes are only walked.  *n_cells: the components found
inline bool group_key_decode(const uint8_t *p, size_t n, std::vector<GroupKeyCell> *out, size_t *n_cells = nullptr) {
  size_t at = 0, cells = 0;
  if (out) out->clear();
  while (at < n) {
    GroupKeyCell c;
    c.tag = p[at++];
    if (c.tag == kGroupKeyInt) {
      if (n - at < 8) return false;
      uint64_t v = 0;
      for (int b = 0; b < 8; b++) v = (v << 8) | p[at + b];
      at += 8;
      c.value = (int64_t)(v ^ 0x8000000000000000ULL);
    } else if (c.tag == kGroupKeyString) {
      if (n - at < 2) return false;
      const size_t len = ((size_t)p[at] << 8) | p[at + 1];
      at += 2;
      if (n - at < len) return false;
      if (out) c.bytes.assign((const char *)p + at, len);
      at += len;
    } else if (c.tag != kGroupKeyNull) {
      return false;
    }
    if (out) out->push_back(std::move(c));
    cells++;
  }
  if (n_cells) *n_cells = cells;
  return true;
}

// are the bytes the key of a tuple of `arity` components?
inline bool group_key_valid(const uint8_t *p, size_t n, int arity) {
  size_t cells = 0;
  return group_key_decode(p, n, nullptr, &cells) && cells == (size_t)arity;
}

}  // namespace tgx
