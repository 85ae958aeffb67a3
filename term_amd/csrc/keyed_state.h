// keyed_state.h -- what the kinds share, on top of counted_state.h, whose tasks count the values of ONE column, an int64
// or bytes (VALUE_COUNTS, GROUP_COUNTS, GROUP_SUMS, and KEY_PROBE for its missing keys): the host's entries, key -> payload, with their blob form and their
// *_entries call, and the device table's key half -- its layout, its view, decoding a slot's key, and the refusals of a
// column that changes between integers and strings.  A kind adds a payload (what it keeps per key, with its wire form),
// its row classes beside the keys, and its launches.
#pragma once
#include <map>
#include <string>

#include "api_internal.h"
#include "counted_state.h"
#include "group_key.h"

namespace tgx {

enum KeyKind { kNoKeys = 0, kIntKeys = 1, kByteKeys = 2 };

// a task's entries as the host sees them.  P: the payload, which has += and whose P() is empty
template <class P>
struct TGX_HIDDEN KeyedEntries {
  int kind = kNoKeys;
  std::map<int64_t, P> ints;      // ascending int64
  std::map<std::string, P> strs;  // ascending bytewise (std::string compares as unsigned bytes)
  uint64_t size() const { return ints.size() + strs.size(); }
  uint64_t key_bytes() const {
    uint64_t n = 0;
    for (const auto &e : strs) n += e.first.size();
    return n;
  }
  P counted() const {  // (in ascending key order: a float sum depends on it)
    P c = P();
    for (const auto &e : ints) c += e.second;
    for (const auto &e : strs) c += e.second;
    return c;
  }
  void add_entries(const KeyedEntries &b) {
    if (kind == kNoKeys) kind = b.kind;
    for (const auto &e : b.ints) ints[e.first] += e.second;
    for (const auto &e : b.strs) strs[e.first] += e.second;
  }
};

// the entries in a blob: n x { i64 key, the payload's words }  or  { u32 length, u8 bytes[length], the payload's words },
// ascending by key (W: counted_state.h)
template <class W, class P>
TGX_HIDDEN inline void keyed_write_entries(const KeyedEntries<P> &e, const W &wire, Writer &w) {
  counted_write_entries(e.ints, wire, w, [&](int64_t v) { w.pod(v); });
  counted_write_entries(e.strs, wire, w, [&](const std::string &v) {
    w.pod((uint32_t)v.size());
    w.put(v.data(), v.size());
  });
}

// ... read back: `n` entries of key kind `kind` into the empty `e`.  `noun`: what the kind calls a key
template <class W, class P>
TGX_HIDDEN inline tgx_status keyed_read_entries(const char *name, const char *noun, size_t k, Reader &r, uint32_t kind,
                                                uint64_t n, uint32_t max_value_bytes, const W &wire, KeyedEntries<P> &e,
                                                uint64_t *counted, tgx_error *err) {
  if (kind == kIntKeys)
    return counted_read_entries(name, k, r, n, 8, wire, e.ints, counted, [&](int64_t &v) {
      v = r.pod<int64_t>();
      return TGX_OK;
    }, err);
  return counted_read_entries(name, k, r, n, 4, wire, e.strs, counted, [&](std::string &v) {
    const uint32_t len = r.pod<uint32_t>();
    if (!r.ok) return TGX_OK;
    if (len > max_value_bytes)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (%s task %zu: a %s of %u bytes, max_value_bytes is %u)",
                  name, k, noun, len, max_value_bytes);
    v.assign(len, '\0');
    r.get(&v[0], len);
    return TGX_OK;
  }, err);
}

// the entries a blob brings a task that groups by a tuple of `arity` columns (0: it does not, and nothing is asked):
// every key is the canonical form of such a tuple (group_key.h)
template <class P>
TGX_HIDDEN inline tgx_status tuple_keys_ok(const char *name, size_t k, int arity, const KeyedEntries<P> &e,
                                           tgx_error *err) {
  if (arity == 0) return TGX_OK;
  for (const auto &s : e.strs)
    if (!group_key_valid((const uint8_t *)s.first.data(), s.first.size(), arity))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (%s task %zu: a key that is not the encoded form of a tuple of %d columns)", name,
                  k, arity);
  return TGX_OK;
}

// A *_entries call: the sizes, then the entries -- the integers, then the strings with their bytes laid end to end.
// make(key, offset, length, payload): the ABI's entry
template <class P, class Entry, class Make>
TGX_HIDDEN inline tgx_status keyed_entries_out(const KeyedEntries<P> &h, Entry *entries, uint64_t cap, uint64_t *n_entries,
                                               uint8_t *bytes, uint64_t bytes_cap, uint64_t *n_bytes, int32_t *is_bytes,
                                               Make make, tgx_error *err) {
  *is_bytes = h.kind == kByteKeys ? 1 : 0;
  TGX_TRY(counted_entries_sizes(h.size(), h.key_bytes(), entries, cap, n_entries, bytes, bytes_cap, n_bytes, err));
  if (!entries) return TGX_OK;
  size_t i = 0;
  uint64_t at = 0;
  for (const auto &e : h.ints) entries[i++] = make(e.first, (uint64_t)0, (uint64_t)0, e.second);
  for (const auto &e : h.strs) {
    if (!e.first.empty()) memcpy(bytes + at, e.first.data(), e.first.size());
    entries[i++] = make((int64_t)0, at, (uint64_t)e.first.size(), e.second);
    at += e.first.size();
  }
  return TGX_OK;
}

// the column types that are no keys
TGX_HIDDEN inline bool refused_as_key(int type) {
  return type == TGX_FLOAT64 || type == TGX_FLOAT32 || type == TGX_UINT64 || type == TGX_BOOL;
}
TGX_HIDDEN inline const char *type_name(int type) {
  switch (type) {
    case TGX_FLOAT64: return "Float64";
    case TGX_FLOAT32: return "Float32";
    case TGX_UINT64: return "UInt64";
    case TGX_BOOL: return "Boolean";
    default: return "this type";
  }
}

// K gives, beyond what CountedState asks: Payload; a Host that is a KeyedEntries<Payload>; and
//   bound(task)             the most keys the task counts
//   max_value_bytes(task)   the most bytes a string key keeps: the task's params.max_value_bytes, unless the kind keeps it
//                           beside its ABI struct (KEY_PROBE)
//   kNoun         what the kind calls a key ("value", "key")
//   kColumn       the key column as the refusal of a changed column names it
//   kDiffers      what states with integer and with string keys were counted under
// The state of a table -- its Dev, its layout, its rows -- goes by the table's owner (CountedState::owner).
template <class K>
struct TGX_HIDDEN KeyedCheck : CountedState<K> {
  typedef typename K::Host Host;
  typedef typename K::Payload Payload;
  using CountedState<K>::table;
  using CountedState<K>::owner;
  using CountedState<K>::device_rows;
  using CountedState<K>::kName;

  // a table's device part besides the table (made at the first batch, for the kind of key the column holds: one key
  // word and nothing behind the counters for integers, two key words, the lengths and the byte store for strings): the
  // per-entry cells of the dictionary route
  struct Dev {
    int kind = kNoKeys;
    DevBuf cells;
  };
  std::vector<Dev> dev_part;
  const std::vector<typename K::Task> &tasks;  // (the plan's: their parameters are fixed once a state exists)

  explicit KeyedCheck(const tgx_plan *plan) : CountedState<K>(plan), dev_part(K::tasks(plan).size()), tasks(K::tasks(plan)) {}

  // the most bytes a string key of task k keeps
  uint32_t value_bytes(size_t k) const { return K::max_value_bytes(tasks[k]); }

  // behind a table's counts: its further counters (arrays of `slots` 64-bit words), then for strings the lengths and
  // the bytes
  size_t lens_at(size_t k) const { return table[k].extra_at() + (size_t)table[k].slots * table[k].extra_counters; }
  size_t store_at(size_t k) const { return lens_at(k) + (size_t)table[k].slots * 4; }

  // the fields that the kinds' views of a table have in common; everything else of `t` is cleared
  template <class Table>
  void fill_view(const tgx_state *st, size_t k, Table &t) const {
    const bool strings = dev_part[k].kind == kByteKeys;
    uint8_t *base = table[k].buf.template as<uint8_t>();
    memset(&t, 0, sizeof(t));
    t.keys = (unsigned long long *)base;
    t.keys2 = strings ? t.keys + table[k].slots : nullptr;
    t.lens = strings ? (uint32_t *)(base + lens_at(k)) : nullptr;
    t.store = strings ? base + store_at(k) : nullptr;
    t.mask = table[k].slots - 1;
    t.salt = (uint64_t)st->plan->fp_key.k[0] | ((uint64_t)st->plan->fp_key.k[1] << 32);
    t.max_value_bytes = value_bytes(k);
  }

  // table k made for keys of `kind`, with `counters` bytes a slot of further counters, unless it is
  tgx_status ensure_keys(tgx_state *st, size_t k, int kind, size_t counters, tgx_error *err) {
    Dev &d = dev_part[k];
    if (d.kind == kind) return TGX_OK;
    if (device_rows[k] > 0)  // (rows: a table has been made, for the other kind)
      return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: %s changed between integer and string values", kName, k,
                  K::kColumn);
    const bool strings = kind == kByteKeys;
    TGX_TRY(this->open_table(st, k, K::bound(tasks[k]), strings ? 2 : 1,
                             counters + (strings ? 4 + (size_t)value_bytes(k) : 0), err, counters));
    d.kind = kind;
    return TGX_OK;
  }

  // ---- what the kinds' updates share: the routes of a key column ----
  enum Route { kNoRoute, kIntRoute, kStringRoute, kDictRoute };
  static Route route_of(const tgx_column &c) {
    if (c.type == TGX_INT64) return kIntRoute;
    if (is_any_string(c.type)) return kStringRoute;
    return c.type == TGX_DICT32_UTF8 ? kDictRoute : kNoRoute;
  }
  static tgx_status dictionary_of(const tgx_column &c, const tgx_column **dict, tgx_error *err) {
    *dict = c.dictionary;
    if (!*dict || !is_string((*dict)->type)) return fail(err, TGX_INVALID_ARGUMENT, "%s: malformed dictionary", kName);
    return TGX_OK;
  }
  // The `n` columns `tuple` of a task on tuple keys as the kernels take them (update_validate has refused floats, UInt64
  // and Booleans, and the staging has widened every integer column to 8 bytes); *numeric: every component is an integer
  // column.  *bytes: what a walk reads at the least -- 8 bytes a row of an integer component (a string component's
  // bytes are not known here: its offsets, views or indices) and a bit of validity where there is a bitmap
  static tgx_status tuple_desc(const tgx_plan *plan, const int *tuple, int n, const tgx_column *dev,
                               KeyProbeTupleDesc *L, bool *numeric, uint64_t *bytes, tgx_error *err) {
    memset(L, 0, sizeof(*L));
    L->d.n_cols = n;
    L->d.length = dev[tuple[0]].length;
    L->d.key = plan->fp_key;
    *numeric = true;
    *bytes = 0;
    for (int c = 0; c < n; c++) {
      const tgx_column &x = dev[tuple[c]];
      TupleCol &tc = L->d.cols[c];
      tc.validity = x.validity;
      tc.offset = x.offset;
      switch (route_of(x)) {
        case kIntRoute:
          tc.kind = 0;
          tc.values = x.values;
          break;
        case kStringRoute:
          tc.kind = x.type == TGX_UTF8 ? 1 : x.type == TGX_LARGE_UTF8 ? 2 : 3;
          tc.values = x.type == TGX_UTF8_VIEW ? x.values : nullptr;
          tc.buffers = x.type == TGX_UTF8_VIEW ? x.variadic : nullptr;
          tc.offsets = x.offsets;
          tc.data = x.data;
          *numeric = false;
          break;
        case kDictRoute: {
          const tgx_column *dc;
          TGX_TRY(dictionary_of(x, &dc, err));
          tc.kind = 4;
          tc.dict_large = dc->type == TGX_LARGE_UTF8 ? 1 : 0;
          tc.values = x.values;
          tc.offsets = dc->offsets;
          tc.data = dc->data;
          tc.dict_validity = dc->validity;
          tc.dict_offset = dc->offset;
          L->dict_length[c] = dc->length;
          *numeric = false;
          break;
        }
        default:
          return fail(err, TGX_UNSUPPORTED, "%s on tuple keys takes integer and string columns (%d)", kName, x.type);
      }
      *bytes += (uint64_t)x.length * (tc.kind == 0 || tc.kind == 2 ? 8 : tc.kind == 3 ? 16 : 4) +
                (x.validity ? (uint64_t)(x.length + 7) / 8 : 0);
    }
    return TGX_OK;
  }

  // the dictionary route's cells of table k: `bytes` of them, zero
  tgx_status clear_cells(tgx_state *st, size_t k, size_t bytes, unsigned long long **cells, tgx_error *err) {
    DevBuf &c = dev_part[k].cells;
    HIP_TRY(c.reserve_roomy(bytes));
    HIP_TRY(hipMemsetAsync(c.p, 0, bytes, st->stream));
    *cells = c.template as<unsigned long long>();
    return TGX_OK;
  }

  // what task k keeps for the key of slot `s`, whose count is `count`
  virtual Payload slot_payload(size_t k, const uint8_t *h, uint64_t s, uint64_t count) const = 0;

  void decode_slot(size_t k, const uint8_t *h, uint64_t s, uint64_t count, Host &o) const override {
    const size_t t = owner[k];
    const uint64_t *keys = (const uint64_t *)h;
    if (o.kind == kNoKeys) o.kind = dev_part[t].kind;
    if (dev_part[t].kind == kIntKeys) {
      o.ints[(int64_t)keys[s]] += slot_payload(k, h, s, count);
    } else {
      if (keys[table[t].slots + s] == kEmptyKey) return;  // (claimed, not settled: nothing was counted into it yet)
      const uint32_t most = value_bytes(t), len = std::min(((const uint32_t *)(h + lens_at(t)))[s], most);
      o.strs[std::string((const char *)h + store_at(t) + (size_t)s * most, len)] += slot_payload(k, h, s, count);
    }
  }

  // what else keeps two hosts of task k from uniting
  virtual tgx_status merge_refused(size_t, const Host &, const Host &, tgx_error *) { return TGX_OK; }

  // (integer keys and string keys do not unite: SideState's merge knows one shape per kind)
  tgx_status merge_from(tgx_state *st, tgx_state *src, tgx_error *err) override {
    std::vector<Host> theirs, mine;
    TGX_TRY(this->of(src)->gather(src, &theirs, err));
    TGX_TRY(this->gather(st, &mine, err));
    for (size_t k = 0; k < theirs.size(); k++) {
      if (theirs[k].kind != kNoKeys && mine[k].kind != kNoKeys && theirs[k].kind != mine[k].kind)
        return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different %s", kName, k,
                    K::kDiffers);
      TGX_TRY(merge_refused(k, theirs[k], mine[k], err));
    }
    for (size_t k = 0; k < theirs.size(); k++) K::merge_host(this->host[k], theirs[k]);
    return TGX_OK;
  }

  // one task, read; a state that was fed integers under one column type and strings under another holds both
  tgx_status read_task(tgx_state *st, size_t slot, Host *out, tgx_error *err) {
    std::vector<Host> g;
    TGX_TRY(this->gather(st, &g, err));
    if (!g[slot].ints.empty() && !g[slot].strs.empty())
      return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu holds integer and string %ss", kName, slot, K::kNoun);
    *out = std::move(g[slot]);
    return TGX_OK;
  }

  // the task of spec `spec_index`, read: the head of the kind's *_get and *_entries calls
  static tgx_status read_spec(const tgx_plan *plan, tgx_state *st, size_t spec_index, Host *out, tgx_error *err) {
    size_t slot = 0;
    TGX_TRY(spec_slot(plan, st, spec_index, K::kKind, kName, &slot, err, "bad arguments"));
    return static_cast<KeyedCheck *>(KeyedCheck::of(st))->read_task(st, slot, out, err);
  }
};

}  // namespace tgx
