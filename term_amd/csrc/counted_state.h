// counted_state.h -- what the kinds share whose tasks count keys in a table on the device (VALUE_COUNTS, PAIR_COUNTS, GROUP_COUNTS, GROUP_SUMS: the
// bounded GROUP BY of kernels/count_table.h): the table's size and layout, clearing it, reading it back once between
// batches, and the two places where sizes come from outside -- a blob's entries and the buffers of the *_entries calls.
#pragma once
#include "side_check.h"

namespace tgx {

// slots of a table that counts up to `bound` keys: the smallest power of two >= 2 * bound and >= 2
TGX_HIDDEN inline uint64_t table_slots(uint32_t bound) {
  uint64_t s = 2;
  while (s < 2 * (uint64_t)bound) s <<= 1;
  return s;
}

// one task's table: `key_words` arrays of `slots` 64-bit key words (kEmptyKey: free), the slots' 64-bit counts, then
// `extra` bytes a slot that the kind lays out (arrays of `slots` elements, from extra_at() on); the first
// `extra_counters` bytes a slot of them are further counters of the slot, cleared with its count
struct TGX_HIDDEN CountedTable {
  DevBuf buf;
  bool live = false;  // allocated (at the task's first batch) and cleared
  uint64_t slots = 0;
  int key_words = 0;
  size_t extra = 0, extra_counters = 0;
  size_t key_bytes() const { return (size_t)slots * 8 * key_words; }
  size_t counts_at() const { return key_bytes(); }
  size_t extra_at() const { return counts_at() + (size_t)slots * 8; }
  size_t bytes() const { return extra_at() + (size_t)slots * extra; }
};

// K gives, beyond what SideState asks:
//   add_entries(a, b)   the entries of host `b` added to `a` (the counters came with SideState's words)
template <class K>
struct TGX_HIDDEN CountedState : SideState<K> {
  typedef typename K::Host Host;

  std::vector<CountedTable> table;  // per task
  // what the tables held when they were last read back: a read of the state costs the copy once, until the next batch
  // or reset (the *_get calls, the two calls of *_entries and tgx_finalize all gather)
  std::vector<Host> table_cache;
  bool table_cache_ok = false;

  explicit CountedState(const tgx_plan *plan) : SideState<K>(plan), table(this->host.size()) {}

  // slot `s` of task k's table, whose copy is `h`, into `into`: its first key word is taken and its count is `count` > 0
  virtual void decode_slot(size_t k, const uint8_t *h, uint64_t s, uint64_t count, Host &into) const = 0;

  tgx_status clear_table(tgx_state *st, size_t k, tgx_error *err) {
    const CountedTable &t = table[k];
    if (!t.live) return TGX_OK;
    uint8_t *base = t.buf.template as<uint8_t>();
    HIP_TRY(hipMemsetAsync(base, 0xFF, t.key_bytes(), st->stream));  // (every key word: kEmptyKey)
    HIP_TRY(hipMemsetAsync(base + t.counts_at(), 0, (size_t)t.slots * (8 + t.extra_counters), st->stream));
    return TGX_OK;
  }

  tgx_status device_clear_extra(tgx_state *st, tgx_error *err) override {
    table_cache_ok = false;
    for (size_t k = 0; k < table.size(); k++) TGX_TRY(clear_table(st, k, err));
    return TGX_OK;
  }

  // task k's table made for up to `bound` keys in the given layout, and cleared
  tgx_status open_table(tgx_state *st, size_t k, uint32_t bound, int key_words, size_t extra, tgx_error *err,
                        size_t extra_counters = 0) {
    CountedTable &t = table[k];
    t.slots = table_slots(bound);
    t.key_words = key_words;
    t.extra = extra;
    t.extra_counters = extra_counters;
    HIP_TRY(t.buf.reserve(t.bytes()));
    t.live = true;
    return clear_table(st, k, err);
  }

  // the tables' entries into the gathered hosts (the counters are already there)
  tgx_status gather_extra(tgx_state *st, std::vector<Host> *out, tgx_error *err) override {
    std::vector<uint8_t> h;
    if (!table_cache_ok) table_cache.assign(table.size(), Host());
    for (size_t k = 0; k < table.size() && !table_cache_ok; k++) {
      const CountedTable &t = table[k];
      if (!t.live || this->device_rows[k] == 0) continue;
      h.resize(t.bytes());
      HIP_TRY(hipMemcpyAsync(h.data(), t.buf.p, h.size(), hipMemcpyDeviceToHost, st->stream));
      HIP_TRY(hipStreamSynchronize(st->stream));
      const uint64_t *keys = (const uint64_t *)h.data(), *counts = (const uint64_t *)(h.data() + t.counts_at());
      for (uint64_t s = 0; s < t.slots; s++)
        if (keys[s] != kEmptyKey && counts[s] != 0) decode_slot(k, h.data(), s, counts[s], table_cache[k]);
    }
    table_cache_ok = true;
    for (size_t k = 0; k < table.size(); k++) K::add_entries((*out)[k], table_cache[k]);
    return TGX_OK;
  }
};

// the kernels' view of a string column (a dictionary's values included); `buffers`: the device copy of a Utf8View's
// table of data-buffer pointers
TGX_HIDDEN inline Utf8ColDesc string_desc(const tgx_column &c, const uint8_t *const *buffers, const FpKey &key) {
  Utf8ColDesc d;
  memset(&d, 0, sizeof(d));
  const bool view = c.type == TGX_UTF8_VIEW;
  d.offsets = c.offsets;
  d.data = c.data;
  d.validity = c.validity;
  d.offset = c.offset;
  d.length = c.length;
  d.large_offsets = c.type == TGX_LARGE_UTF8;
  d.views = view ? c.values : nullptr;
  d.buffers = view ? buffers : nullptr;
  d.key = key;
  return d;
}

// A task's entries in a blob: n x { key, u64 count }, strictly ascending by key, into the empty map `m`; *counted: the
// sum of their counts.  `least`: the fewest bytes an entry takes.  read_key(key) reads one key and may refuse it.
// TGX_OK with r.ok cleared: the blob ran out
template <class Map, class ReadKey>
TGX_HIDDEN inline tgx_status counted_read_entries(const char *name, size_t k, Reader &r, uint64_t n, size_t least, Map &m,
                                                  uint64_t *counted, ReadKey read_key, tgx_error *err) {
  size_t bytes = 0;  // (held against the bytes that are left before anything is allocated)
  if (!r.fits(n, least, &bytes)) return TGX_OK;
  *counted = 0;
  for (uint64_t i = 0; i < n; i++) {
    typename Map::key_type key;
    TGX_TRY(read_key(key));
    const uint64_t c = r.pod<uint64_t>();
    if (!r.ok) return TGX_OK;
    if (!m.empty() && !(m.rbegin()->first < key))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: entry %llu is out of order or repeated)",
                  name, k, (unsigned long long)i);
    if (c == 0)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: entry %llu has a zero count)", name, k,
                  (unsigned long long)i);
    if (c > UINT64_MAX - *counted)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: counts)", name, k);
    *counted += c;
    m.emplace_hint(m.end(), std::move(key), c);
  }
  return TGX_OK;
}

// The sibling for entries with a second counter: n x { key, u64 total, u64 non_null }, non_null <= total, into the map
// `m` of key -> Counts{total, non_null}; *counted / *counted_non_null: the sums
template <class Map, class ReadKey>
TGX_HIDDEN inline tgx_status counted_read_entries2(const char *name, size_t k, Reader &r, uint64_t n, size_t least, Map &m,
                                                   uint64_t *counted, uint64_t *counted_non_null, ReadKey read_key,
                                                   tgx_error *err) {
  size_t bytes = 0;  // (held against the bytes that are left before anything is allocated)
  if (!r.fits(n, least, &bytes)) return TGX_OK;
  *counted = *counted_non_null = 0;
  for (uint64_t i = 0; i < n; i++) {
    typename Map::key_type key;
    TGX_TRY(read_key(key));
    const uint64_t c = r.pod<uint64_t>(), nn = r.pod<uint64_t>();
    if (!r.ok) return TGX_OK;
    if (!m.empty() && !(m.rbegin()->first < key))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: entry %llu is out of order or repeated)",
                  name, k, (unsigned long long)i);
    if (c == 0)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: entry %llu has a zero count)", name, k,
                  (unsigned long long)i);
    if (nn > c)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: entry %llu has non_null > total)", name,
                  k, (unsigned long long)i);
    if (c > UINT64_MAX - *counted)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: counts)", name, k);
    *counted += c;
    *counted_non_null += nn;
    typename Map::mapped_type v;
    v.total = c;
    v.non_null = nn;
    m.emplace_hint(m.end(), std::move(key), v);
  }
  return TGX_OK;
}

// The size query of the *_entries calls: what is needed is reported first, then the buffers are held against it.  A call
// without `entries` only asks for the sizes: the caller returns after this
TGX_HIDDEN inline tgx_status counted_entries_sizes(uint64_t need_entries, uint64_t need_bytes, const void *entries,
                                                   uint64_t cap, uint64_t *n_entries, const void *bytes,
                                                   uint64_t bytes_cap, uint64_t *n_bytes, tgx_error *err) {
  *n_entries = need_entries;
  *n_bytes = need_bytes;
  if (entries && cap < need_entries)
    return fail(err, TGX_INVALID_ARGUMENT, "entries holds %llu entries, %llu are needed", (unsigned long long)cap,
                (unsigned long long)need_entries);
  if (bytes && bytes_cap < need_bytes)
    return fail(err, TGX_INVALID_ARGUMENT, "bytes holds %llu bytes, %llu are needed", (unsigned long long)bytes_cap,
                (unsigned long long)need_bytes);
  if (entries && need_bytes && !bytes) return fail(err, TGX_INVALID_ARGUMENT, "string values need a byte buffer");
  return TGX_OK;
}

}  // namespace tgx
