// counted_state.h -- what the kinds share whose tasks count keys in a table on the device (VALUE_COUNTS, PAIR_COUNTS, GROUP_COUNTS, GROUP_SUMS: the
// bounded GROUP BY of kernels/count_table.h): the table's size and layout, clearing it, reading it back once between
// batches, and the two places where sizes come from outside -- a blob's entries and the buffers of the *_entries calls.
// keyed_state.h builds on this for the four kinds whose keys are the values of one column (KEY_PROBE counts the keys
// that are missing from its parent set); PAIR_COUNTS, whose keys are pairs of cells, stands on this file alone.
#pragma once
#include <initializer_list>

#include "side_check.h"

namespace tgx {

// slots of a table that counts up to `bound` keys (below 2^62): the smallest power of two >= 2 * bound and >= 2
TGX_HIDDEN inline uint64_t table_slots(uint64_t bound) {
  uint64_t s = 2;
  while (s < 2 * bound) s <<= 1;
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

// K's Host gives, beyond what SideState asks:
//   a.add_entries(b)   the entries of host `b` added to `a` (the counters came with SideState's words)
template <class K>
struct TGX_HIDDEN CountedState : SideState<K> {
  typedef typename K::Host Host;

  std::vector<CountedTable> table;  // per task
  // per task: the task whose table it counts in -- itself, unless a kind lets tasks share a table; the other tasks of
  // a shared table have none of their own
  std::vector<size_t> owner;
  // what the tables held when they were last read back: a read of the state costs the copy once, until the next batch
  // or reset (the *_get calls, the two calls of *_entries and tgx_finalize all gather)
  std::vector<Host> table_cache;
  bool table_cache_ok = false;

  explicit CountedState(const tgx_plan *plan) : SideState<K>(plan), table(this->host.size()), owner(table.size()) {
    for (size_t k = 0; k < owner.size(); k++) owner[k] = k;
  }

  // slot `s` of the table task k counts in, whose copy is `h`, into `into` as task k sees it: the slot's first key word
  // is taken and its count is `count` > 0
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

  // the tables' entries into the gathered hosts (the counters are already there): a table is copied once and decoded
  // for every task that counts in it
  tgx_status gather_extra(tgx_state *st, std::vector<Host> *out, tgx_error *err) override {
    std::vector<uint8_t> h;
    std::vector<size_t> served;
    if (!table_cache_ok) table_cache.assign(table.size(), Host());
    for (size_t k = 0; k < table.size() && !table_cache_ok; k++) {
      const CountedTable &t = table[k];
      if (!t.live || this->device_rows[k] == 0) continue;
      h.resize(t.bytes());
      HIP_TRY(hipMemcpyAsync(h.data(), t.buf.p, h.size(), hipMemcpyDeviceToHost, st->stream));
      HIP_TRY(hipStreamSynchronize(st->stream));
      served.clear();
      for (size_t j = 0; j < owner.size(); j++)
        if (owner[j] == k) served.push_back(j);
      const uint64_t *keys = (const uint64_t *)h.data(), *counts = (const uint64_t *)(h.data() + t.counts_at());
      for (uint64_t s = 0; s < t.slots; s++)
        if (keys[s] != kEmptyKey && counts[s] != 0)
          for (size_t j : served) decode_slot(j, h.data(), s, counts[s], table_cache[j]);
    }
    table_cache_ok = true;
    for (size_t k = 0; k < table.size(); k++) (*out)[k].add_entries(table_cache[k]);
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

// ---- a task's entries in a blob: n x { key, the payload's 64-bit words }, strictly ascending by key -------------------
// A payload's wire form W gives: kWords, put(payload, words), get(words), and refuse(words): null, or what is wrong with
// an entry's words, as the refusal says it.  The first word is the entry's count, which is never zero.
struct CountWire {  // a bare count
  static constexpr int kWords = 1;
  void put(uint64_t c, uint64_t *w) const { w[0] = c; }
  uint64_t get(const uint64_t *w) const { return w[0]; }
  const char *refuse(const uint64_t *) const { return nullptr; }
};

// write_key(key) writes one key
template <class W, class Map, class WriteKey>
TGX_HIDDEN inline void counted_write_entries(const Map &m, const W &wire, Writer &w, WriteKey write_key) {
  for (const auto &e : m) {
    uint64_t words[W::kWords];
    write_key(e.first);
    wire.put(e.second, words);
    w.pod(words);
  }
}

// ... read into the empty map `m`; *counted: the sum of their counts.  `key_least`: the fewest bytes a key takes.
// read_key(key) reads one key and may refuse it.  TGX_OK with r.ok cleared: the blob ran out
template <class W, class Map, class ReadKey>
TGX_HIDDEN inline tgx_status counted_read_entries(const char *name, size_t k, Reader &r, uint64_t n, size_t key_least,
                                                  const W &wire, Map &m, uint64_t *counted, ReadKey read_key,
                                                  tgx_error *err) {
  size_t bytes = 0;  // (held against the bytes that are left before anything is allocated)
  if (!r.fits(n, key_least + 8 * W::kWords, &bytes)) return TGX_OK;
  *counted = 0;
  for (uint64_t i = 0; i < n; i++) {
    typename Map::key_type key;
    TGX_TRY(read_key(key));
    uint64_t words[W::kWords];
    r.get(words, sizeof(words));
    if (!r.ok) return TGX_OK;
    if (!m.empty() && !(m.rbegin()->first < key))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: entry %llu is out of order or repeated)",
                  name, k, (unsigned long long)i);
    const char *wrong = words[0] == 0 ? "has a zero count" : wire.refuse(words);
    if (wrong)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: entry %llu %s)", name, k,
                  (unsigned long long)i, wrong);
    if (words[0] > UINT64_MAX - *counted)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: counts)", name, k);
    *counted += words[0];
    m.emplace_hint(m.end(), std::move(key), wire.get(words));
  }
  return TGX_OK;
}

// do the terms add up to `whole`?  (No sum can wrap: each term is held against what is left of the whole)
TGX_HIDDEN inline bool terms_make(uint64_t whole, std::initializer_list<uint64_t> terms) {
  bool ok = true;
  for (uint64_t term : terms) {
    ok = ok && term <= whole;
    whole -= ok ? term : 0;
  }
  return ok && whole == 0;
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
