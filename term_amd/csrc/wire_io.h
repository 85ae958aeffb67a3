// wire_io.h -- the cursors over a state blob (wire.cpp; term_amd/wire.py documents the layout).  wire.cpp opens one and
// hands it to the check modules, which write and read their own sections through it.
#pragma once
#include <stdint.h>
#include <string.h>

#include "internal.h"

namespace tgx {

// Writes into `buf` while there is room and keeps counting when there is not (or when buf is null: a measuring call);
// tgx_state_serialize compares `len` with `cap` at the end.
struct TGX_HIDDEN Writer {
  uint8_t *buf;
  size_t cap, len = 0;
  void put(const void *p, size_t n) {
    if (n && buf && len + n <= cap) memcpy(buf + len, p, n);  // (n = 0: an empty KLL level, whose `p` is null)
    len += n;
  }
  template <class T>
  void pod(const T &v) { put(&v, sizeof(T)); }
};

// Reads a blob nobody vouches for.  pos <= len always; a read past the end zero-fills, leaves `pos` where it is and
// clears `ok` for good: test `ok` before a value read from the blob sizes an allocation or bounds a loop.
struct TGX_HIDDEN Reader {
  const uint8_t *buf;
  size_t len, pos = 0;
  bool ok = true;
  void get(void *p, size_t n) {
    if (n == 0) return;  // (an empty KLL level: p may be null)
    if (!ok || n > len - pos) {
      ok = false;
      memset(p, 0, n);
      return;
    }
    memcpy(p, buf + pos, n);
    pos += n;
  }
  template <class T>
  T pod() {
    T v;
    get(&v, sizeof(T));
    return v;
  }
  // are `count` elements of `size` bytes still there (`*bytes` of them)?  `count` comes from the blob -- key records, the
  // cells of JOINT_BINS -- so it is held against the bytes that are left BEFORE it is multiplied (a crafted count would
  // wrap the product past the check).  Clears `ok` when they are not.
  bool fits(uint64_t count, size_t size, size_t *bytes) {
    if (!ok || count > (len - pos) / size) return ok = false;
    *bytes = (size_t)count * size;
    return true;
  }
};

}  // namespace tgx
