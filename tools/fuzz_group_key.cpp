// fuzz_group_key.cpp -- seeded round trips and mutated bytes through the host's codec of tuple GROUP BY keys
// (term_amd/csrc/group_key.h): the decoder takes bytes from state blobs, which come from outside.
//
// A stand-alone host program: no device, no HIP, nothing of the library but the header.  Build it with the sanitizers and
// run it on a CPU machine:
//     c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/fuzz_group_key.cpp \
//         -o fuzz_group_key && ./fuzz_group_key [cases] [seed]
//
// Every case is one of
//   round trip  a tuple of 0 .. 8 cells (NULL, an int64 drawn with its extremes, a string of 0 .. 300 bytes): it encodes,
//               the bytes decode to the same cells, group_key_valid agrees on the arity and on no other, and the order of
//               two encoded tuples of one arity is the order of their cells (NULL, integers numerically, strings by length
//               and then bytewise)
//   mutated     encoded bytes with bytes deleted, doubled, flipped or cut short, copied into a heap buffer of EXACTLY their
//               size (so that a read past the end trips the sanitizer): decoding gives cells or refuses; what decodes
//               encodes back to the very bytes
// Exit status 0: every case ran clean.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../term_amd/csrc/group_key.h"

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
  uint64_t below(uint64_t n) { return next() % n; }
};

int failures = 0;
void fail(const char *what, uint64_t at) {
  fprintf(stderr, "case %llu: %s\n", (unsigned long long)at, what);
  failures++;
}

GroupKeyCell cell_of(Rng &rng) {
  static const int64_t kEdges[] = {INT64_MIN, INT64_MIN + 1, -256, -1, 0, 1, 255, 256, INT64_MAX - 1, INT64_MAX};
  GroupKeyCell c;
  switch (rng.below(3)) {
    case 0:
      break;
    case 1:
      c.tag = kGroupKeyInt;
      c.value = rng.below(3) == 0 ? kEdges[rng.below(sizeof(kEdges) / sizeof(kEdges[0]))] : (int64_t)rng.next();
      break;
    default: {
      static const size_t kLengths[] = {0, 1, 2, 3, 12, 255, 256, 300};
      c.tag = kGroupKeyString;
      const size_t len = kLengths[rng.below(sizeof(kLengths) / sizeof(kLengths[0]))];
      for (size_t i = 0; i < len; i++) c.bytes.push_back((char)(rng.below(4) == 0 ? rng.below(3) : rng.below(256)));
    }
  }
  return c;
}

// the stated order of two cells: < 0, 0, > 0
int cell_order(const GroupKeyCell &a, const GroupKeyCell &b) {
  if (a.tag != b.tag) return a.tag < b.tag ? -1 : 1;
  if (a.tag == kGroupKeyInt) return a.value < b.value ? -1 : a.value > b.value ? 1 : 0;
  if (a.tag == kGroupKeyString) {
    if (a.bytes.size() != b.bytes.size()) return a.bytes.size() < b.bytes.size() ? -1 : 1;
    const int c = memcmp(a.bytes.data(), b.bytes.data(), a.bytes.size());
    return c < 0 ? -1 : c > 0 ? 1 : 0;
  }
  return 0;
}

// the bytes in a heap buffer of exactly their size
std::unique_ptr<uint8_t[]> exact(const std::string &bytes) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[bytes.size()]);
  if (!bytes.empty()) memcpy(p.get(), bytes.data(), bytes.size());
  return p;
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 200000;
  Rng rng{argc > 2 ? strtoull(argv[2], nullptr, 10) | 1 : 0x9E3779B97F4A7C15ull};
  std::vector<GroupKeyCell> previous;
  std::string previous_bytes;
  for (uint64_t at = 0; at < cases; at++) {
    std::vector<GroupKeyCell> cells;
    const size_t arity = rng.below(kGroupKeyMaxArity + 1);
    for (size_t i = 0; i < arity; i++) cells.push_back(cell_of(rng));
    std::string bytes;
    if (!group_key_encode(cells, &bytes)) fail("a tuple does not encode", at);
    {
      const std::unique_ptr<uint8_t[]> p = exact(bytes);
      std::vector<GroupKeyCell> back;
      size_t n_cells = 0;
      if (!group_key_decode(p.get(), bytes.size(), &back, &n_cells) || !(back == cells) || n_cells != arity)
        fail("the round trip gives other cells", at);
      for (int a = 0; a <= kGroupKeyMaxArity + 1; a++)
        if (group_key_valid(p.get(), bytes.size(), a) != ((size_t)a == arity)) fail("group_key_valid on the arity", at);
    }
    if (previous.size() == cells.size()) {  // bytewise order == the order of the cells
      int want = 0;
      for (size_t i = 0; i < cells.size() && want == 0; i++) want = cell_order(previous[i], cells[i]);
      const int c = previous_bytes.compare(bytes);  // (std::string compares as unsigned bytes)
      if ((c < 0 ? -1 : c > 0 ? 1 : 0) != want) fail("the bytes' order is not the cells' order", at);
    }
    previous = cells;
    previous_bytes = bytes;
    // mutations of the bytes
    for (int m = 0; m < 4; m++) {
      std::string mutated = bytes;
      const uint64_t how = rng.below(5);
      if (how == 0 && !mutated.empty()) mutated.erase(rng.below(mutated.size()), 1 + rng.below(3));
      else if (how == 1 && !mutated.empty()) mutated.insert(rng.below(mutated.size()), 1, mutated[rng.below(mutated.size())]);
      else if (how == 2 && !mutated.empty()) mutated[rng.below(mutated.size())] ^= (char)(1u << rng.below(8));
      else if (how == 3 && !mutated.empty()) mutated.resize(rng.below(mutated.size()));
      else mutated.push_back((char)rng.below(256));
      const std::unique_ptr<uint8_t[]> p = exact(mutated);
      std::vector<GroupKeyCell> back;
      size_t n_cells = 0;
      if (group_key_decode(p.get(), mutated.size(), &back, &n_cells)) {
        std::string again;
        if (n_cells != back.size() || !group_key_encode(back, &again) || again != mutated)
          fail("bytes that decode do not encode back to themselves", at);
      }
      if (group_key_decode(p.get(), mutated.size(), nullptr, &n_cells) != group_key_decode(p.get(), mutated.size(), &back))
        fail("walking the bytes and decoding them disagree", at);
    }
  }
  printf("%llu cases, %d failures\n", (unsigned long long)cases, failures);
  return failures ? 1 : 0;
}
