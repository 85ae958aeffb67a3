// keyprobe_device.cpp -- TGX_CHECK_KEY_PROBE: is each key of a child column in a parent's key set?  (The device side of
// the reference's ForeignKeyConstraint, TG/constraints/foreign_key.rs:152-176; include/tgx.h has the exact semantics.)
//
// A task is one spec.  What a state holds for it:
//   the parent's set   a bitmap or a hash table in device memory, built by tgx_key_probe_set_parent from {key, count}
//                      records (kernels/keyprobe.hip), with its route, the number of its distinct keys and their digest.
//                      It is read-only while batches run, survives tgx_state_reset, and travels nowhere: a blob carries
//                      (parent_keys, parent_digest) only, and a state read from one takes batches again once it has been
//                      given a set with that identity.
//   the counters       four 64-bit words on the device (non-NULL rows, matched rows, missing rows whose key's bits are the
//                      free-slot marker, overflow rows); rows seen are counted on the host.
//   the missing keys   one open-addressing table of counted keys (counted_state.h), allocated at the first batch.
// A COUNTED task (tgx_plan_set_key_probe_counted; the device side of the reference's JoinCoverageConstraint,
// TG/constraints/join_coverage.rs) keeps the records' counts in its set -- a count array or a table of {key, count}
// slots -- and one more counter, `pairs`: the sum over the matched rows of their key's multiplicity in the parent, which
// is COUNT(*) of the inner join.  Its set's identity is (parent_keys, parent_digest, parent_rows, parent_count_digest).
// A ROWS task (tgx_plan_set_key_probe_rows) probes nothing: it gathers its column's non-NULL keys as {key, 1} records in
// device memory, the parent side of a counted probe when the parent's keys repeat (a DISTINCT export knows a key as seen
// once or more than once, not how often).  Its records stay with the state: such a state does not merge or serialize.
// A STRINGS task (tgx_plan_set_key_probe_strings; kernels/keyprobe_strings.hip) reads a string column against a set of
// keyed 128-bit fingerprints (route 5, built from a DISTINCT export's 32-byte records).  Its missing keys keep their bytes:
// its table is laid out as VALUE_COUNTS's string table is, its entries are KeyedEntries::strs, and it has one more row
// class, the missing rows whose value is longer than max_value_bytes (long_rows, in the marker's word: no string has the
// marker's bits).  Merges, blobs and the cross-rank step unite its missing keys by BYTES.
// A COUNTED STRINGS task (tgx_plan_set_key_probe_strings_counted) is both: its set is route 6, the fingerprint table of
// route 5 with one 64-bit count a slot beside it, built from the same 32-byte records with their counts used; its
// identity is the counted one, its blob carries the counted tail and the strings tail.  A ROWS STRINGS task
// (tgx_plan_set_key_probe_rows_strings) gathers a string column as 32-byte {fa, fb, n, 0} records, what such a set is
// built from: a record a non-NULL row, or, a dictionary batch, a record per entry its rows refer to, with their number.
// A TUPLES task (tgx_plan_set_key_probe_tuples*; kernels/keyprobe_tuples.hip) reads the 2 .. 8 columns of its spec's list
// as ONE key, the tuple's keyed fingerprint, against routes 5 and 6; a row with a NULL component matches nothing (SQL's
// join) and is no non-NULL row.  Its table keeps fingerprints only, in the strings layout with one byte of value a slot
// whose LENGTH is the flag "a NULL-bearing tuple"; on the host an entry's key is 17 bytes -- hash_a and hash_b big-endian,
// then the flag -- so KeyedEntries::strs holds the entries ascending by (hash_a, hash_b), and merges, blobs and the
// cross-rank step unite them as they unite a strings task's.  The NULL-bearing rows that found no slot are counted in
// kKpLong's word (a tuple has no long rows).
// `pairs` never wraps: the host holds an upper bound, max_count * rows a batch, in checked arithmetic, and refuses the
// batch, merge or blob that could carry it past 2^64 - 1.
// The host part is a map from missing key to count plus the same counters and the identity of the set they were taken
// under: what was merged in or read from a blob, and what the device part is folded into whenever the state is read.
//
// How the module is put together.  A task has ONE mode (KeyProbeMode, internal.h); kModes says what differs by mode in
// words, and plan_set_mode is the one body of the six tgx_plan_set_key_probe* calls.  ProbeCheck is a KeyedCheck
// (keyed_state.h): the table of missing keys, its views, its decoding and the dictionary route's cells are that
// skeleton's; what KEY_PROBE adds is the parent set with its identity (so merge_from, serialize, collect and read_spec
// are its own), `pairs` with its bound, and the gathered rows.  tgx_key_probe_set_parent is the checks, choose_route,
// and one build function per route that fills a ParentSet, whose view() is what the kernels take.
#include "keyed_state.h"

namespace tgx {
void launch_key_probe_reduce(const void *recs, uint64_t n, bool counted, KeyProbeBuild *b, hipStream_t stream);
void launch_key_probe_build_count_array(const void *recs, uint64_t n, unsigned long long *counts, uint64_t base,
                                        uint64_t range, KeyProbeBuild *b, hipStream_t stream);
void launch_key_probe_build_count_hash(const void *recs, uint64_t n, unsigned long long *slots, uint64_t mask,
                                       KeyProbeBuild *b, hipStream_t stream);
void launch_key_probe_build_bitmap(const void *recs, uint64_t n, uint32_t *bits, uint64_t base, uint64_t range,
                                   KeyProbeBuild *b, hipStream_t stream);
void launch_key_probe_build_hash(const void *recs, uint64_t n, unsigned long long *keys, uint64_t mask, KeyProbeBuild *b,
                                 hipStream_t stream);
void launch_key_probe_rows(const ComomentColDesc &d, unsigned long long *recs, uint64_t cap, unsigned long long *cursor,
                           int blocks, hipStream_t stream);
void launch_key_probe(const KeyProbeLaunch &L, int route, int n_tasks, int blocks, hipStream_t stream);
void launch_key_probe_build_strings(const void *recs, uint64_t n, unsigned long long *slots, uint64_t mask,
                                    KeyProbeStringsBuild *b, hipStream_t stream);
void launch_key_probe_utf8(const Utf8ColDesc &d, const KeyProbeStringSet &set, const ValueCountsTable &t,
                           hipStream_t stream);
void launch_key_probe_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                           const Utf8ColDesc &dict, unsigned long long *cells, const KeyProbeStringSet &set,
                           const ValueCountsTable &t, hipStream_t stream);
void launch_key_probe_build_strings_counted(const void *recs, uint64_t n, unsigned long long *slots,
                                            unsigned long long *counts, uint64_t mask, KeyProbeCountedStringsBuild *b,
                                            hipStream_t stream);
void launch_key_probe_utf8_counted(const Utf8ColDesc &d, const KeyProbeCountedStringSet &set, const ValueCountsTable &t,
                                   hipStream_t stream);
void launch_key_probe_dict_counted(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                                   const Utf8ColDesc &dict, unsigned long long *cells,
                                   const KeyProbeCountedStringSet &set, const ValueCountsTable &t, hipStream_t stream);
void launch_key_probe_rows_utf8(const Utf8ColDesc &d, unsigned long long *recs, uint64_t cap, unsigned long long *words,
                                hipStream_t stream);
void launch_key_probe_rows_dict(const int32_t *indices, const uint8_t *validity, int64_t offset, int64_t length,
                                const Utf8ColDesc &dict, unsigned long long *cells, unsigned long long *recs, uint64_t cap,
                                unsigned long long *words, hipStream_t stream);

void launch_key_probe_tuples(const KeyProbeTupleDesc &L, bool numeric, const KeyProbeStringSet &set,
                             const ValueCountsTable &t, hipStream_t stream);
void launch_key_probe_tuples_counted(const KeyProbeTupleDesc &L, bool numeric, const KeyProbeCountedStringSet &set,
                                     const ValueCountsTable &t, hipStream_t stream);
void launch_key_probe_rows_tuples(const KeyProbeTupleDesc &L, bool numeric, unsigned long long *recs, uint64_t cap,
                                  unsigned long long *words, hipStream_t stream);

namespace {

constexpr uint64_t kMaxParentRecords = (uint64_t)1 << 40;

// one task's state as the host sees it
struct ProbeHost : KeyedEntries<uint64_t> {
  uint64_t seen = 0, non_null = 0, matched = 0, overflow_rows = 0;
  // the set the counts were taken under (`known`: there is one)
  bool known = false;
  uint64_t parent_keys = 0, parent_digest = 0;
  // a counted task: the rest of its set's identity, the set's largest count, and the matched pairs
  uint64_t parent_rows = 0, parent_count_digest = 0, max_count = 0, pairs = 0;
  uint64_t long_rows = 0;  // a strings task: missing rows whose value is longer than max_value_bytes
  uint64_t gathered = 0;   // a task that gathers: the records it has written
  uint64_t null_overflow_rows = 0;  // a tuples task: rows with a NULL component whose tuple found no slot
  bool holds_counts() const { return seen != 0 || size() != 0; }
  bool same_parent(const ProbeHost &o) const {
    return parent_keys == o.parent_keys && parent_digest == o.parent_digest && parent_rows == o.parent_rows &&
           parent_count_digest == o.parent_count_digest;
  }
  void take_parent(const ProbeHost &o) {
    known = true;
    parent_keys = o.parent_keys;
    parent_digest = o.parent_digest;
    parent_rows = o.parent_rows;
    parent_count_digest = o.parent_count_digest;
    max_count = o.max_count;
  }
};

// ---- a tuples task's entries: the key of KeyedEntries::strs is hash_a, hash_b (big-endian: bytewise order is the order
// of the pair) and one byte, 1 for a tuple with a NULL component ----
constexpr uint32_t kTupleEntryBytes = 17;
inline std::string tuple_entry_key(uint64_t fa, uint64_t fb, bool has_null) {
  std::string k(kTupleEntryBytes, '\0');
  for (int i = 0; i < 8; i++) {
    k[i] = (char)(uint8_t)(fa >> (56 - 8 * i));
    k[8 + i] = (char)(uint8_t)(fb >> (56 - 8 * i));
  }
  k[16] = has_null ? 1 : 0;
  return k;
}
inline tgx_key_probe_tuple_entry tuple_entry_of(const std::string &k, uint64_t count) {
  tgx_key_probe_tuple_entry e;
  memset(&e, 0, sizeof(e));
  for (int i = 0; i < 8; i++) {
    e.hash_a = (e.hash_a << 8) | (uint8_t)k[i];
    e.hash_b = (e.hash_b << 8) | (uint8_t)k[8 + i];
  }
  e.count = count;
  e.has_null = (uint8_t)k[16];
  return e;
}
// the two classes of a tuples task's entries
struct TupleClasses {
  uint64_t missing_keys = 0, missing_counted = 0, null_keys = 0, null_counted = 0;
};
template <class Entries>
inline TupleClasses tuple_classes(const Entries &h) {
  TupleClasses c;
  for (const auto &e : h.strs) {
    const bool has_null = e.first.size() == kTupleEntryBytes && e.first[16] != 0;
    (has_null ? c.null_keys : c.missing_keys) += 1;
    (has_null ? c.null_counted : c.missing_counted) += e.second;
  }
  return c;
}

// a + b, or false: the sum is past 2^64 - 1
inline bool add_fits(uint64_t a, uint64_t b, uint64_t *sum) { return !__builtin_add_overflow(a, b, sum); }

struct NoRange {};

struct ProbeKind {
  typedef KeyProbeTask Task;
  typedef ProbeHost Host;
  typedef uint64_t Payload;
  typedef NoRange Range;
  static constexpr bool kRanged = false;
  static constexpr int kKind = TGX_CHECK_KEY_PROBE;
  static constexpr const char *kDiffers = "parent sets";
  static constexpr const char *kNoun = "key";
  static constexpr const char *kColumn = "the column";  // (a task's mode fixes its kind of key: the refusal cannot fire)
  static constexpr uint32_t kMagic = 0x4252504b;  // "KPRB"

  static const std::vector<KeyProbeTask> &tasks(const tgx_plan *plan) { return plan->key_probes; }
  static size_t words(const KeyProbeTask &) { return kKeyProbeWords; }
  // (a tuples task: one allocation whose lower half is the missing tuples' table and whose upper half is the
  // NULL-bearing tuples': max_missing_keys bounds each class as it bounds the one class of the other modes)
  static uint32_t bound(const KeyProbeTask &t) { return (kp_tuples(t.mode) ? 2u : 1u) * t.params.max_missing_keys; }
  // (a tuples task: the one byte a slot whose length is the flag of a NULL-bearing tuple)
  static uint32_t max_value_bytes(const KeyProbeTask &t) { return kp_tuples(t.mode) ? 1u : t.max_value_bytes; }
  static NoRange range_identity() { return NoRange(); }
  static ProbeHost fresh(const KeyProbeTask &) { return ProbeHost(); }
  static size_t shape(const ProbeHost &) { return 0; }  // (the sets' identities: ProbeCheck::merge_from)
  // the counters; the table's entries follow in gather_extra
  static ProbeHost from_device(const KeyProbeTask &t, int64_t rows, const NoRange &, const unsigned long long *w) {
    ProbeHost d;
    d.seen = (uint64_t)rows;
    d.non_null = w[kKpNonNull];
    d.matched = w[kKpMatched];
    d.overflow_rows = w[kKpOverflow];
    d.pairs = w[kKpPairs];
    if (t.mode == kKpRows) d.gathered = d.non_null;
    if (t.mode == kKpRowsStrings || t.mode == kKpRowsTuples) {  // (its cursor stands in the pairs' word)
      d.gathered = w[kKpPairs];
      d.pairs = 0;
      return d;
    }
    if (kp_tuple_set(t.mode)) {  // (no tuple is long: the word counts the NULL-bearing rows that found no slot)
      d.null_overflow_rows = w[kKpLong];
      return d;
    }
    if (kp_string_set(t.mode)) {  // (no string has the marker's bits)
      d.long_rows = w[kKpLong];
      return d;
    }
    if (w[kKpMarker]) {
      d.kind = kIntKeys;
      d.ints[(int64_t)kEmptyKey] = w[kKpMarker];
    }
    return d;
  }
  static void merge_host(ProbeHost &a, const ProbeHost &b) {
    a.seen += b.seen;
    a.non_null += b.non_null;
    a.matched += b.matched;
    a.overflow_rows += b.overflow_rows;
    a.long_rows += b.long_rows;
    a.null_overflow_rows += b.null_overflow_rows;
    a.gathered += b.gathered;
    a.pairs += b.pairs;  // (the callers have held the sum against 2^64 - 1: ProbeCheck::pairs_fit)
    a.add_entries(b);
    if (!a.known && b.known) a.take_parent(b);
  }

  // per task { u32 max_missing_keys, u32 0 (the plan's parameters), u32 known (the counts were taken under a set), u32 0,
  //   u64 parent_keys, parent_digest, u64 seen, non_null, matched, overflow_rows, u64 n_entries,
  //   n_entries x { i64 key, u64 count }, ascending by key }
  // a counted task: the second u32 0 is 1, and { u64 parent_rows, parent_count_digest, max_count, pairs } stand between
  // n_entries and the entries
  // a strings task: the second u32 0 is 2, { u32 max_value_bytes, u32 0, u64 long_rows } stand between n_entries and the
  // entries, and an entry is { u32 length, u8 bytes[length], u64 count }, ascending bytewise
  // a counted strings task: the second u32 0 is 4, and the counted task's four words, then the strings task's
  // { u32 max_value_bytes, u32 0, u64 long_rows }, stand between n_entries and the entries, which are a strings task's
  // a tuples task: the second u32 0 is 6 (counted: 7, and the counted task's four words come first);
  // { u32 arity, u32 0, u64 null_overflow_rows } stand between n_entries and the entries, and an entry is a strings
  // task's with the 17 bytes { hash_a, hash_b big-endian, u8 has_null }
  // (the mode word is the task's mode; a task that gathers, whose state serializes only while it is empty, writes a
  // plain one's)
  static uint32_t mode_word(const KeyProbeTask &t) { return kp_gathers(t.mode) ? (uint32_t)kKpPlain : (uint32_t)t.mode; }
  static void write(const KeyProbeTask &t, const ProbeHost &h, Writer &w) {
    w.pod(t.params);
    w.pod((uint32_t)(h.known ? 1 : 0));
    w.pod(mode_word(t));
    const uint64_t words[7] = {h.parent_keys, h.parent_digest, h.seen, h.non_null, h.matched, h.overflow_rows, h.size()};
    w.pod(words);
    if (kp_counts(t.mode)) {
      const uint64_t more[4] = {h.parent_rows, h.parent_count_digest, h.max_count, h.pairs};
      w.pod(more);
    }
    if (kp_string_set(t.mode)) {
      w.pod(t.max_value_bytes);
      w.pod((uint32_t)0);
      w.pod(h.long_rows);
    }
    if (kp_tuple_set(t.mode)) {
      w.pod((uint32_t)t.n_tuple);
      w.pod((uint32_t)0);
      w.pod(h.null_overflow_rows);
    }
    keyed_write_entries(h, CountWire(), w);
  }

  static tgx_status read(const KeyProbeTask &t, ProbeHost &h, Reader &r, size_t k, tgx_error *err) {
    tgx_key_probe_params p;
    r.get(&p, sizeof(p));
    const uint32_t known = r.pod<uint32_t>(), pad = r.pod<uint32_t>();
    uint64_t words[7], more[4] = {0, 0, 0, 0};
    r.get(words, sizeof(words));
    if (!r.ok) return TGX_OK;
    const bool counted = kp_counts(t.mode), strings = kp_string_set(t.mode), tuples = kp_tuple_set(t.mode);
    if (pad != mode_word(t)) {
      const bool is_mode = pad <= kKpStrings || pad == kKpStringsCounted || pad == kKpTuples || pad == kKpTuplesCounted;
      return fail(err, TGX_INVALID_ARGUMENT,
                  !is_mode ? "malformed state blob (KEY_PROBE task %zu: parent set)"
                  : (is_mode && kp_tuple_set((KeyProbeMode)pad)) != tuples
                      ? "KEY_PROBE task %zu: the blob was counted under the other mode (single / tuple keys) than the plan's"
                  : (is_mode && kp_string_set((KeyProbeMode)pad)) != strings
                      ? "KEY_PROBE task %zu: the blob was counted under the other mode (integer / string keys) than the plan's"
                      : "KEY_PROBE task %zu: the blob was counted under the other mode (plain / counted) than the plan's",
                  k);
    }
    if (counted) r.get(more, sizeof(more));
    uint32_t value_bytes = 0, value_pad = 0;
    uint64_t long_rows = 0;
    if (strings) {
      value_bytes = r.pod<uint32_t>();
      value_pad = r.pod<uint32_t>();
      long_rows = r.pod<uint64_t>();
    }
    uint32_t arity = 0;
    uint64_t null_overflow = 0;
    if (tuples) {
      arity = r.pod<uint32_t>();
      value_pad = r.pod<uint32_t>();
      null_overflow = r.pod<uint64_t>();
    }
    if (!r.ok) return TGX_OK;
    if (tuples && value_pad != 0)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (KEY_PROBE task %zu: tuple keys)", k);
    if (tuples && arity != (uint32_t)t.n_tuple)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "KEY_PROBE task %zu: the blob was counted over tuples of %u columns, the plan's have %d", k, arity,
                  t.n_tuple);
    if (strings && value_pad != 0)
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (KEY_PROBE task %zu: string keys)", k);
    if (strings && value_bytes != t.max_value_bytes)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "KEY_PROBE task %zu: the blob was counted under other parameters (max_value_bytes %u) than the plan's "
                  "(%u)", k, value_bytes, t.max_value_bytes);
    if (p.max_missing_keys != t.params.max_missing_keys || p.reserved != t.params.reserved)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "KEY_PROBE task %zu: the blob was counted under other parameters (max_missing_keys %u) than the plan's "
                  "(%u)", k, p.max_missing_keys, t.params.max_missing_keys);
    const uint64_t seen = words[2], non_null = words[3], n = words[6];
    if (known > 1 || (!known && (words[0] != 0 || words[1] != 0 || seen != 0 || n != 0 || more[0] != 0 || more[1] != 0 ||
                                 more[2] != 0 || more[3] != 0 || long_rows != 0 || null_overflow != 0)))
      return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (KEY_PROBE task %zu: parent set)", k);
    // a counted set: keys <= rows < 2^63, the largest count is one of them; matched <= pairs <= matched * max_count
    if (counted) {
      uint64_t most = 0;
      const bool set_ok = more[0] >= words[0] && more[0] < ((uint64_t)1 << 63) && more[2] <= more[0] &&
                          (more[2] != 0) == (words[0] != 0);
      const bool wraps = __builtin_mul_overflow(words[4], more[2], &most);
      if (!set_ok || more[3] < words[4] || (!wraps && more[3] > most))
        return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (KEY_PROBE task %zu: counted set and pairs)", k);
    }
    uint64_t in_entries = 0;
    TGX_TRY(keyed_read_entries("KEY_PROBE", kNoun, k, r, strings || tuples ? kByteKeys : kIntKeys, n,
                               tuples ? kTupleEntryBytes : t.max_value_bytes, CountWire(), h, &in_entries, err));
    if (!r.ok) return TGX_OK;
    if (tuples) {
      // an entry is 17 bytes whose last is the flag; null_counted + null_overflow_rows == seen - non_null
      for (const auto &e : h.strs)
        if (e.first.size() != kTupleEntryBytes || (uint8_t)e.first[16] > 1)
          return fail(err, TGX_INVALID_ARGUMENT, "malformed state blob (KEY_PROBE task %zu: a tuple entry)", k);
      const TupleClasses c = tuple_classes(h);
      if (non_null > seen || !terms_make(seen - non_null, {c.null_counted, null_overflow}))
        return fail(err, TGX_INVALID_ARGUMENT,
                    "malformed state blob (KEY_PROBE task %zu: null_counted + null_overflow_rows != null_rows)", k);
      in_entries = c.missing_counted;
    }
    // matched + counted + overflow_rows (+ long_rows) == non_null <= seen
    if (non_null > seen || !terms_make(non_null, {words[4], in_entries, words[5], long_rows}))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "malformed state blob (KEY_PROBE task %zu: matched + counted + overflow_rows%s != non_null)", k,
                  strings ? " + long_rows" : "");
    h.kind = !n ? kNoKeys : strings || tuples ? kByteKeys : kIntKeys;
    h.long_rows = long_rows;
    h.null_overflow_rows = null_overflow;
    h.known = known != 0;
    h.parent_keys = words[0];
    h.parent_digest = words[1];
    h.seen = seen;
    h.non_null = non_null;
    h.matched = words[4];
    h.overflow_rows = words[5];
    h.parent_rows = more[0];
    h.parent_count_digest = more[1];
    h.max_count = more[2];
    h.pairs = more[3];
    return TGX_OK;
  }
};

// what differs by mode in words: how a refusal names a spec that was set that way, the suffix of its
// tgx_plan_set_key_probe* call, and the bytes of a record of its parent set (a rows task: of the records it gathers)
struct ModeInfo {
  const char *set_as, *suffix;
  uint32_t record_bytes;
};
constexpr ModeInfo kModes[] = {{"plain", "", 16},
                               {"counted", "_counted", 16},
                               {"to probe string keys", "_strings", 32},
                               {"to gather rows", "_rows", 16},
                               {"to probe string keys, counted", "_strings_counted", 32},
                               {"to gather the rows of a string column", "_rows_strings", 32},
                               {"to probe tuple keys", "_tuples", 32},
                               {"to probe tuple keys, counted", "_tuples_counted", 32},
                               {"to gather the tuples of its columns", "_rows_tuples", 32}};
static_assert(kKpPlain == 0 && kKpCounted == 1 && kKpStrings == 2 && kKpRows == 3 && kKpStringsCounted == 4 &&
                  kKpRowsStrings == 5 && kKpTuples == 6 && kKpTuplesCounted == 7 && kKpRowsTuples == 8,
              "kModes is indexed by the mode");

// the set of one task on the device
struct ParentSet {
  bool has = false;
  int route = kKpRouteEmpty;
  // the bitmap's words, the table's keys, the count array, the table's {key, count} slots or (strings) {fa, fb} slots;
  // route 6: the {fa, fb} slots, and behind them a count a slot
  DevBuf buf;
  uint64_t base = 0, range = 0, mask = 0;
  uint32_t has_marker = 0;
  uint64_t keys = 0, digest = 0;
  uint64_t marker_count = 0, rows = 0, count_digest = 0, max_count = 0;  // a counted set
  void identify(ProbeHost &h) const {
    h.known = true;
    h.parent_keys = keys;
    h.parent_digest = digest;
    h.parent_rows = rows;
    h.parent_count_digest = count_digest;
    h.max_count = max_count;
  }
  // the set as the kernels take it: routes 0 .. 4, and route 5 (or the empty set of a strings task)
  KeyProbeSet view() const {
    KeyProbeSet v;
    memset(&v, 0, sizeof(v));
    v.bits = route == kKpRouteBitmap ? buf.as<uint32_t>() : nullptr;
    v.keys = route == kKpRouteHash ? buf.as<unsigned long long>() : nullptr;
    v.counts = route == kKpRouteCountArray || route == kKpRouteCountHash ? buf.as<unsigned long long>() : nullptr;
    v.base = base;
    v.range = range;
    v.mask = mask;
    v.marker_count = marker_count;
    v.has_marker = has_marker;
    return v;
  }
  KeyProbeStringSet string_view() const {
    return KeyProbeStringSet{route == kKpRouteStrings ? buf.as<unsigned long long>() : nullptr, mask};
  }
  KeyProbeCountedStringSet counted_string_view() const {
    unsigned long long *slots = route == kKpRouteStringsCounted ? buf.as<unsigned long long>() : nullptr;
    return KeyProbeCountedStringSet{slots, mask, slots ? slots + 2 * (mask + 1) : nullptr};
  }
};

// the route of a set of `n` > 0 records of a task of `mode`, whose keys span `range` (0: all of int64, which is not dense).
// A dense set is no larger than the table would be: a bit a key up to 128 * n, a count a key up to 4 * n
int choose_route(KeyProbeMode mode, uint64_t range, uint64_t n) {
  if (mode == kKpStrings || mode == kKpTuples) return kKpRouteStrings;
  if (mode == kKpStringsCounted || mode == kKpTuplesCounted) return kKpRouteStringsCounted;
  const bool counted = mode == kKpCounted;
  const bool dense = range != 0 && range <= (counted ? 4 : 128) * n;
  return counted ? (dense ? kKpRouteCountArray : kKpRouteCountHash) : (dense ? kKpRouteBitmap : kKpRouteHash);
}

struct ProbeCheck final : KeyedCheck<ProbeKind> {
  std::vector<ParentSet> parent;
  bool fed = false;  // a batch with rows has been handed to tgx_update since the state was created or reset
  // per counted task: an upper bound of what the device part's `pairs` can have come to, the sum over the accepted
  // batches of max_count * rows
  std::vector<uint64_t> pairs_bound;
  // per task that gathers: the gathered records and the records there is room for
  std::vector<DevBuf> gathered;
  std::vector<uint64_t> gathered_cap;

  explicit ProbeCheck(const tgx_plan *plan)
      : KeyedCheck(plan), parent(tasks.size()), pairs_bound(tasks.size(), 0), gathered(tasks.size()),
        gathered_cap(tasks.size(), 0) {}

  uint64_t slot_payload(size_t, const uint8_t *, uint64_t, uint64_t count) const override { return count; }

  // a tuples task's slot: the fingerprint and the flag are the key, the slot's length is the flag
  void decode_slot(size_t k, const uint8_t *h, uint64_t s, uint64_t count, ProbeHost &o) const override {
    if (!kp_tuples(tasks[k].mode)) return KeyedCheck::decode_slot(k, h, s, count, o);
    const uint64_t *keys = (const uint64_t *)h;
    const uint64_t fb = keys[table[k].slots + s];
    if (fb == kEmptyKey) return;  // (claimed, not settled: nothing was counted into it yet)
    if (o.kind == kNoKeys) o.kind = kByteKeys;
    o.strs[tuple_entry_key(keys[s], fb, ((const uint32_t *)(h + lens_at(k)))[s] != 0)] += count;
  }

  // a state that has gathered rows keeps them to itself
  tgx_status rows_stay(const char *what, tgx_error *err) const {
    for (size_t k = 0; k < tasks.size(); k++)
      if (kp_gathers(tasks[k].mode) && (device_rows[k] > 0 || host[k].seen > 0))
        return fail(err, TGX_UNSUPPORTED, "spec %d: a KEY_PROBE check that gathers rows does not %s: its records stay with "
                    "the state", tasks[k].spec_index, what);
    return TGX_OK;
  }

  // every task, read: host part + device part, under the identity of the set the state holds
  tgx_status collect(tgx_state *st, std::vector<ProbeHost> *g, tgx_error *err) {
    TGX_TRY(gather(st, g, err));
    for (size_t k = 0; k < g->size(); k++) {
      ProbeHost &h = (*g)[k];
      if (parent[k].has && !h.known) parent[k].identify(h);
    }
    return TGX_OK;
  }

  tgx_status accepts(tgx_state *, int64_t nrows, tgx_error *err) override {
    for (size_t k = 0; k < tasks.size(); k++)
      if (!parent[k].has && !kp_gathers(tasks[k].mode))
        return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a KEY_PROBE check needs its parent set (tgx_key_probe_set_parent)",
                    tasks[k].spec_index);
    // a counted task: host part + bound of the device part + this batch's bound stays within 2^64 - 1, for every task
    // before any bound moves
    std::vector<uint64_t> next(pairs_bound);
    for (size_t k = 0; k < tasks.size(); k++) {
      if (!kp_counts(tasks[k].mode) || nrows <= 0) continue;
      uint64_t batch = 0, all = 0;
      if (__builtin_mul_overflow(parent[k].max_count, (uint64_t)nrows, &batch) || !add_fits(next[k], batch, &next[k]) ||
          !add_fits(next[k], host[k].pairs, &all))
        return fail(err, TGX_UNSUPPORTED,
                    "spec %d: a batch of %lld rows against a set whose largest count is %llu could carry the matched "
                    "pairs past 2^64 - 1", tasks[k].spec_index, (long long)nrows, (unsigned long long)parent[k].max_count);
    }
    pairs_bound.swap(next);
    fed |= nrows > 0;
    return TGX_OK;
  }

  tgx_status reset(tgx_state *st, tgx_error *err) override {
    fed = false;
    std::fill(pairs_bound.begin(), pairs_bound.end(), 0);
    return KeyedCheck::reset(st, err);
  }

  // may `theirs` be added to what this state holds?  (pairs of a plain task are 0)
  tgx_status pairs_fit(const std::vector<ProbeHost> &theirs, tgx_error *err) const {
    for (size_t k = 0; k < theirs.size(); k++) {
      uint64_t all = 0;
      if (!add_fits(host[k].pairs, pairs_bound[k], &all) || !add_fits(all, theirs[k].pairs, &all))
        return fail(err, TGX_UNSUPPORTED, "%s task %zu: the states' matched pairs add up past 2^64 - 1", kName, k);
    }
    return TGX_OK;
  }

  // ---- the parent set: the checks (set_parent), the route (choose_route), one build a route ----
  // what a build kernel left in the build struct `d`: one wait
  template <class Build>
  static tgx_status read_back(tgx_state *st, const DevBuf &d, Build *b, tgx_error *err) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(b, d.p, sizeof(*b), hipMemcpyDeviceToHost, st->stream));
    HIP_TRY(hipStreamSynchronize(st->stream));
    return TGX_OK;
  }
  // a refused set leaves the state without one: the set it had is dropped
  tgx_status drop_set(size_t k, tgx_status refusal) {
    parent[k] = ParentSet();
    return refusal;
  }
  // the set's memory, every byte `fill` (0xFF: every word kEmptyKey)
  static tgx_status set_memory(tgx_state *st, ParentSet *s, size_t bytes, int fill, tgx_error *err) {
    HIP_TRY(s->buf.reserve(bytes));
    HIP_TRY(hipMemsetAsync(s->buf.p, fill, bytes, st->stream));
    return TGX_OK;
  }

  // routes 1 and 3 span [s->base, s->base + s->range); routes 2, 4 and 5 have s->mask + 1 slots
  static tgx_status build_bitmap(tgx_state *st, const void *recs, uint64_t n, KeyProbeBuild *b, ParentSet *s, tgx_error *err) {
    TGX_TRY(set_memory(st, s, (size_t)((s->range + 31) / 32) * 4, 0, err));
    launch_key_probe_build_bitmap(recs, n, s->buf.as<uint32_t>(), s->base, s->range, b, st->stream);
    return TGX_OK;
  }
  static tgx_status build_hash(tgx_state *st, const void *recs, uint64_t n, KeyProbeBuild *b, ParentSet *s, tgx_error *err) {
    TGX_TRY(set_memory(st, s, (size_t)(s->mask + 1) * 8, 0xFF, err));
    launch_key_probe_build_hash(recs, n, s->buf.as<unsigned long long>(), s->mask, b, st->stream);
    return TGX_OK;
  }
  static tgx_status build_count_array(tgx_state *st, const void *recs, uint64_t n, KeyProbeBuild *b, ParentSet *s,
                                      tgx_error *err) {
    TGX_TRY(set_memory(st, s, (size_t)s->range * 8, 0, err));
    launch_key_probe_build_count_array(recs, n, s->buf.as<unsigned long long>(), s->base, s->range, b, st->stream);
    return TGX_OK;
  }
  static tgx_status build_count_hash(tgx_state *st, const void *recs, uint64_t n, KeyProbeBuild *b, ParentSet *s,
                                     tgx_error *err) {
    HIP_TRY(s->buf.reserve((size_t)(s->mask + 1) * 16));  // (the launcher clears the slots: {kEmptyKey, 0})
    launch_key_probe_build_count_hash(recs, n, s->buf.as<unsigned long long>(), s->mask, b, st->stream);
    return TGX_OK;
  }

  // a counted set's reduction, held to its bounds: no zero count, and the sum (three pieces, exact) below 2^63: s->rows
  tgx_status counts_ok(size_t k, unsigned long long zero_counts, const unsigned long long *piece, ParentSet *s,
                       tgx_error *err) {
    if (zero_counts)
      return drop_set(k, fail(err, TGX_INVALID_ARGUMENT, "spec %d: %llu records of the parent set have a count of 0",
                              tasks[k].spec_index, zero_counts));
    const unsigned __int128 total = (unsigned __int128)piece[0] + ((unsigned __int128)piece[1] << kKpPieceBits) +
                                    ((unsigned __int128)piece[2] << (2 * kKpPieceBits));
    if (total >> 63)
      return drop_set(k, fail(err, TGX_UNSUPPORTED, "spec %d: the counts of the parent set sum to 2^63 or more",
                              tasks[k].spec_index));
    s->rows = (uint64_t)total;
    return TGX_OK;
  }

  // routes 1 .. 4: the set of task k from `n` > 0 16-byte {key, count} records; a reduction, the route's build, two waits
  tgx_status build_integers(tgx_state *st, size_t k, const void *recs, uint64_t n, ParentSet *s, tgx_error *err) {
    const KeyProbeMode mode = tasks[k].mode;
    DevBuf d_build;
    HIP_TRY(d_build.reserve(sizeof(KeyProbeBuild)));
    KeyProbeBuild b;
    memset(&b, 0, sizeof(b));
    b.min = INT64_MAX;
    b.max = INT64_MIN;
    HIP_TRY(hipMemcpyAsync(d_build.p, &b, sizeof(b), hipMemcpyHostToDevice, st->stream));
    launch_key_probe_reduce(recs, n, mode == kKpCounted, d_build.as<KeyProbeBuild>(), st->stream);
    TGX_TRY(read_back(st, d_build, &b, err));
    if (mode == kKpCounted) {
      TGX_TRY(counts_ok(k, b.zero_counts, b.sum_piece, s, err));
      s->count_digest = b.count_digest;
    }
    // (unsigned: INT64_MIN and INT64_MAX together wrap the range to 0, which is not dense)
    const uint64_t range = (uint64_t)b.max - (uint64_t)b.min + 1;
    s->route = choose_route(mode, range, n);
    if (s->route == kKpRouteBitmap || s->route == kKpRouteCountArray) {
      s->base = (uint64_t)b.min;
      s->range = range;
    } else {
      s->mask = table_slots(n) - 1;
    }
    KeyProbeBuild *d = d_build.as<KeyProbeBuild>();
    TGX_TRY(s->route == kKpRouteBitmap       ? build_bitmap(st, recs, n, d, s, err)
            : s->route == kKpRouteHash       ? build_hash(st, recs, n, d, s, err)
            : s->route == kKpRouteCountArray ? build_count_array(st, recs, n, d, s, err)
                                             : build_count_hash(st, recs, n, d, s, err));
    TGX_TRY(read_back(st, d_build, &b, err));
    s->has_marker = b.has_marker;
    s->marker_count = b.marker_count;
    s->max_count = b.max_count;
    s->keys = b.keys;
    s->digest = b.digest;
    return TGX_OK;
  }

  // route 5: the set of strings task k from `n` > 0 32-byte {hash_a, hash_b, count, 0} records; one wait
  tgx_status build_strings(tgx_state *st, size_t k, const void *recs, uint64_t n, ParentSet *s, tgx_error *err) {
    DevBuf d_build;
    HIP_TRY(d_build.reserve(sizeof(KeyProbeStringsBuild)));
    HIP_TRY(hipMemsetAsync(d_build.p, 0, sizeof(KeyProbeStringsBuild), st->stream));
    s->route = choose_route(tasks[k].mode, 0, n);
    s->mask = table_slots(n) - 1;
    TGX_TRY(set_memory(st, s, (size_t)(s->mask + 1) * 16, 0xFF, err));
    launch_key_probe_build_strings(recs, n, s->buf.as<unsigned long long>(), s->mask, d_build.as<KeyProbeStringsBuild>(),
                                   st->stream);
    KeyProbeStringsBuild b;
    TGX_TRY(read_back(st, d_build, &b, err));
    if (b.marker_records) return marker_records(k, b.marker_records, err);
    s->keys = b.keys;
    s->digest = b.digest;
    return TGX_OK;
  }

  // the refusal of records that can be no fingerprints
  tgx_status marker_records(size_t k, unsigned long long n, tgx_error *err) {
    return drop_set(k, fail(err, TGX_INVALID_ARGUMENT,
                            "spec %d: %llu records of the parent set hold the free-slot marker (all ones) in hash_a or "
                            "hash_b, which no fingerprint is", tasks[k].spec_index, n));
  }

  // route 6: the set of counted strings task k from `n` > 0 such records, their counts used; one wait
  tgx_status build_strings_counted(tgx_state *st, size_t k, const void *recs, uint64_t n, ParentSet *s, tgx_error *err) {
    DevBuf d_build;
    HIP_TRY(d_build.reserve(sizeof(KeyProbeCountedStringsBuild)));
    HIP_TRY(hipMemsetAsync(d_build.p, 0, sizeof(KeyProbeCountedStringsBuild), st->stream));
    s->route = choose_route(tasks[k].mode, 0, n);
    s->mask = table_slots(n) - 1;
    const size_t slots = (size_t)(s->mask + 1);
    HIP_TRY(s->buf.reserve(slots * 24));  // (16-byte slots, every word kEmptyKey; then the counts, 0)
    HIP_TRY(hipMemsetAsync(s->buf.p, 0xFF, slots * 16, st->stream));
    HIP_TRY(hipMemsetAsync(s->buf.as<uint8_t>() + slots * 16, 0, slots * 8, st->stream));
    unsigned long long *table = s->buf.as<unsigned long long>();
    launch_key_probe_build_strings_counted(recs, n, table, table + 2 * slots, s->mask,
                                           d_build.as<KeyProbeCountedStringsBuild>(), st->stream);
    KeyProbeCountedStringsBuild b;
    TGX_TRY(read_back(st, d_build, &b, err));
    if (b.marker_records) return marker_records(k, b.marker_records, err);
    TGX_TRY(counts_ok(k, b.zero_counts, b.sum_piece, s, err));
    s->count_digest = b.count_digest;
    s->max_count = b.max_count;
    s->keys = b.keys;
    s->digest = b.digest;
    return TGX_OK;
  }

  tgx_status set_parent(tgx_state *st, size_t k, const void *recs, uint64_t n, tgx_error *err) {
    const KeyProbeMode mode = tasks[k].mode;
    if (kp_gathers(mode))
      return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a KEY_PROBE check that gathers rows takes no parent set",
                  tasks[k].spec_index);
    if (fed)
      return fail(err, TGX_INVALID_ARGUMENT,
                  "spec %d: the parent set of a KEY_PROBE check is given before the state's first batch (or after "
                  "tgx_state_reset)", tasks[k].spec_index);
    if (n > kMaxParentRecords)
      return fail(err, TGX_UNSUPPORTED, "spec %d: a parent set of %llu records is too large", tasks[k].spec_index,
                  (unsigned long long)n);
    if (n > 0 && !recs) return fail(err, TGX_INVALID_ARGUMENT, "device_records is NULL");
    TGX_TRY(device_init(st, err));
    ParentSet s;
    s.has = true;
    if (n > 0) {  // (without records: the empty set, route 0)
      ProfScope ps(st, "key_probe_build", n * kModes[mode].record_bytes);
      TGX_TRY(mode == kKpStrings || mode == kKpTuples                 ? build_strings(st, k, recs, n, &s, err)
              : mode == kKpStringsCounted || mode == kKpTuplesCounted ? build_strings_counted(st, k, recs, n, &s, err)
                                                                      : build_integers(st, k, recs, n, &s, err));
    }
    ProbeHost &h = host[k];
    ProbeHost given;
    s.identify(given);
    if (h.known && h.holds_counts() && !h.same_parent(given))
      return fail(err, TGX_INVALID_ARGUMENT,
                  "spec %d: the state holds counts taken under another parent set (%llu keys, digest %016llx) than the "
                  "one given (%llu keys, digest %016llx)", tasks[k].spec_index, (unsigned long long)h.parent_keys,
                  (unsigned long long)h.parent_digest, (unsigned long long)s.keys, (unsigned long long)s.digest);
    s.identify(h);
    parent[k] = std::move(s);
    return TGX_OK;
  }

  // ---- a batch ----
  // the table of missing integer keys of task k as the kernels take it
  KeyProbeTable int_view(const tgx_state *st, size_t k) const {
    uint8_t *base = table[k].buf.as<uint8_t>();
    KeyProbeTable t;
    t.keys = (unsigned long long *)base;
    t.counts = (unsigned long long *)(base + table[k].counts_at());
    t.words = d_counts.as<unsigned long long>() + word_off[k];
    t.mask = table[k].slots - 1;
    t.salt = (uint64_t)st->plan->fp_key.k[0] | ((uint64_t)st->plan->fp_key.k[1] << 32);
    return t;
  }

  // (accepts has seen to it that every task that probes has its set)
  tgx_status update(tgx_state *st, const tgx_column *dev, int64_t nrows, tgx_error *err) override {
    if (nrows <= 0) return TGX_OK;
    TGX_TRY(device_init(st, err));
    table_cache_ok = false;
    for (size_t k = 0; k < tasks.size(); k++) {
      const tgx_column &x = dev[tasks[k].column];
      const Route route = route_of(x);
      if (kp_tuples(tasks[k].mode)) {  // (its columns: walk_tuples)
        if (tasks[k].mode != kKpRowsTuples) TGX_TRY(ensure_keys(st, k, kByteKeys, 0, err));
        continue;
      }
      if (kp_string_column(tasks[k].mode)) {
        if (route != kStringRoute && route != kDictRoute)
          return fail(err, TGX_UNSUPPORTED, "KEY_PROBE on string keys takes string columns (%d)", x.type);
        if (tasks[k].mode == kKpRowsStrings) TGX_TRY(gather_strings(st, k, x, nrows, err));
        else TGX_TRY(ensure_keys(st, k, kByteKeys, 0, err));
        continue;
      }
      // (an Int64 view: update_validate refuses what is not widened to one)
      if (route != kIntRoute) return fail(err, TGX_UNSUPPORTED, "KEY_PROBE takes integer columns (%d)", x.type);
      if (tasks[k].mode == kKpRows) TGX_TRY(gather_rows(st, k, x, nrows, err));
      else TGX_TRY(ensure_keys(st, k, kIntKeys, 0, err));
    }
    for (int route = kKpRouteEmpty; route <= kKpRouteCountHash; route++) {
      // (side_launches asks about the elements of `tasks` themselves: a task's address gives its index)
      auto on_route = [&](const KeyProbeTask &t) {
        return t.mode <= kKpCounted && parent[(size_t)(&t - tasks.data())].route == route;
      };
      TGX_TRY(side_launches(tasks, on_route, [&](const int *slots, int n) -> tgx_status {
        KeyProbeLaunch L;
        memset(&L, 0, sizeof(L));
        uint64_t bytes = 0;
        for (int i = 0; i < n; i++) {
          const size_t k = (size_t)slots[i];
          bytes += side_fill_x(L.cols[i], dev[tasks[k].column]);
          L.sets[i] = parent[k].view();
          L.tables[i] = int_view(st, k);
        }
        // 16 waves a workgroup and 96 KiB of LDS: one workgroup a CU
        const int blocks = side_blocks(nrows, kKeyProbeBlock, g_ctx.n_cu, 1, n);
        TGX_TRY(side_rows_fit("KEY_PROBE", nrows, blocks, err));
        ProfScope ps(st, "key_probe", bytes);
        launch_key_probe(L, route, n, blocks, st->stream);
        HIP_TRY(hipGetLastError());
        return TGX_OK;
      }));
    }
    for (size_t k = 0; k < tasks.size(); k++)
      if (kp_string_set(tasks[k].mode)) TGX_TRY(probe_strings(st, k, dev[tasks[k].column], nrows, err));
    for (size_t k = 0; k < tasks.size(); k++)
      if (kp_tuples(tasks[k].mode)) TGX_TRY(walk_tuples(st, k, dev, nrows, err));
    for (size_t k = 0; k < tasks.size(); k++) device_rows[k] += nrows;
    return TGX_OK;
  }

  // one batch of strings task k: a row per lane, or the dictionary's two steps (VALUE_COUNTS's routes)
  tgx_status probe_strings(tgx_state *st, size_t k, const tgx_column &x, int64_t nrows, tgx_error *err) {
    const tgx_plan *plan = st->plan;
    const bool counted = tasks[k].mode == kKpStringsCounted;
    const KeyProbeStringSet set = parent[k].string_view();
    const KeyProbeCountedStringSet counted_set = parent[k].counted_string_view();
    ValueCountsTable t;
    fill_view(st, k, t);
    t.counts = (unsigned long long *)(table[k].buf.as<uint8_t>() + table[k].counts_at());
    t.words = d_counts.as<unsigned long long>() + word_off[k];  // (the task's kKeyProbeWords counters)
    // (per-lane and LDS counters are 32-bit: the launchers take up to 2048 workgroups, 1024 for the dictionary's indices)
    TGX_TRY(side_rows_fit("KEY_PROBE", nrows, 1024, err));
    if (x.type != TGX_DICT32_UTF8) {
      ProfScope ps(st, "key_probe", 0);
      const Utf8ColDesc d = string_desc(x, x.variadic, plan->fp_key);
      if (counted) launch_key_probe_utf8_counted(d, counted_set, t, st->stream);
      else launch_key_probe_utf8(d, set, t, st->stream);
    } else {
      const tgx_column *dc;
      TGX_TRY(dictionary_of(x, &dc, err));
      if (dc->length > 0) {  // (without entries every row is a row without a value)
        unsigned long long *cells;
        TGX_TRY(clear_cells(st, k, (size_t)dc->length * 8, &cells, err));
        ProfScope ps(st, "key_probe", (uint64_t)x.length * 4);
        const Utf8ColDesc d = string_desc(*dc, nullptr, plan->fp_key);
        if (counted)
          launch_key_probe_dict_counted((const int32_t *)x.values, x.validity, x.offset, x.length, d, cells, counted_set, t,
                                        st->stream);
        else
          launch_key_probe_dict((const int32_t *)x.values, x.validity, x.offset, x.length, d, cells, set, t, st->stream);
      }
    }
    HIP_TRY(hipGetLastError());
    return TGX_OK;
  }

  // one batch of tuples task k: the probe against its set, or the gather of its all-valid tuples
  tgx_status walk_tuples(tgx_state *st, size_t k, const tgx_column *dev, int64_t nrows, tgx_error *err) {
    KeyProbeTupleDesc L;
    bool numeric = true;
    // what the walk reads: KeyedCheck::tuple_desc's figure
    uint64_t bytes = 0;
    TGX_TRY(tuple_desc(st->plan, tasks[k].tuple, tasks[k].n_tuple, dev, &L, &numeric, &bytes, err));
    // (per-lane and LDS counters are 32-bit: the launchers take up to 2048 workgroups)
    TGX_TRY(side_rows_fit("KEY_PROBE", nrows, 1024, err));
    unsigned long long *words = d_counts.as<unsigned long long>() + word_off[k];
    if (tasks[k].mode == kKpRowsTuples) {
      TGX_TRY(gather_room(st, k, nrows, err));
      ProfScope ps(st, "key_probe_rows", bytes + (uint64_t)nrows * 32);
      launch_key_probe_rows_tuples(L, numeric, gathered[k].as<unsigned long long>(), gathered_cap[k], words, st->stream);
    } else {
      ValueCountsTable t;
      fill_view(st, k, t);
      t.counts = (unsigned long long *)(table[k].buf.as<uint8_t>() + table[k].counts_at());
      t.words = words;
      ProfScope ps(st, "key_probe", bytes);
      if (tasks[k].mode == kKpTuplesCounted)
        launch_key_probe_tuples_counted(L, numeric, parent[k].counted_string_view(), t, st->stream);
      else
        launch_key_probe_tuples(L, numeric, parent[k].string_view(), t, st->stream);
    }
    HIP_TRY(hipGetLastError());
    return TGX_OK;
  }

  // one batch of a rows task: room for every row the state has seen and this batch's, then the batch's non-NULL keys
  // behind the records that are there
  // room in task k's buffer of gathered records for every row the state has seen and `nrows` more (a batch makes at
  // most a record a row): at least twice the room there was, the records that are there kept
  tgx_status gather_room(tgx_state *st, size_t k, int64_t nrows, tgx_error *err) {
    const size_t record = kModes[tasks[k].mode].record_bytes;
    const uint64_t need = (uint64_t)device_rows[k] + (uint64_t)nrows;
    if (need <= gathered_cap[k]) return TGX_OK;
    const uint64_t cap = std::max<uint64_t>(need, 2 * gathered_cap[k]);
    DevBuf grown;
    HIP_TRY(grown.reserve((size_t)cap * record));
    if (device_rows[k] > 0) {
      HIP_TRY(hipMemcpyAsync(grown.p, gathered[k].p, (size_t)device_rows[k] * record, hipMemcpyDeviceToDevice, st->stream));
      HIP_TRY(hipStreamSynchronize(st->stream));  // (before the old buffer goes)
    }
    gathered[k] = std::move(grown);
    gathered_cap[k] = cap;
    return TGX_OK;
  }

  tgx_status gather_rows(tgx_state *st, size_t k, const tgx_column &col, int64_t nrows, tgx_error *err) {
    TGX_TRY(gather_room(st, k, nrows, err));
    ComomentColDesc d;
    memset(&d, 0, sizeof(d));
    const uint64_t bytes = side_fill_x(d, col);
    ProfScope ps(st, "key_probe_rows", bytes);
    launch_key_probe_rows(d, gathered[k].as<unsigned long long>(), gathered_cap[k],
                          d_counts.as<unsigned long long>() + word_off[k] + kKpNonNull,
                          side_blocks(nrows, 256, g_ctx.n_cu, 4, 1), st->stream);
    HIP_TRY(hipGetLastError());
    return TGX_OK;
  }

  // one batch of a rows strings task: a {fa, fb, 1, 0} record a non-NULL row, or the dictionary's two steps and a
  // {fa, fb, n, 0} record an entry that n > 0 rows of the batch refer to
  tgx_status gather_strings(tgx_state *st, size_t k, const tgx_column &x, int64_t nrows, tgx_error *err) {
    const tgx_plan *plan = st->plan;
    TGX_TRY(side_rows_fit("KEY_PROBE", nrows, 1024, err));
    TGX_TRY(gather_room(st, k, nrows, err));
    unsigned long long *recs = gathered[k].as<unsigned long long>(), *words = d_counts.as<unsigned long long>() + word_off[k];
    if (x.type != TGX_DICT32_UTF8) {
      ProfScope ps(st, "key_probe_rows", 0);
      launch_key_probe_rows_utf8(string_desc(x, x.variadic, plan->fp_key), recs, gathered_cap[k], words, st->stream);
    } else {
      const tgx_column *dc;
      TGX_TRY(dictionary_of(x, &dc, err));
      if (dc->length > 0) {  // (without entries every row is a row without a value)
        unsigned long long *cells;
        TGX_TRY(clear_cells(st, k, (size_t)dc->length * 8, &cells, err));
        ProfScope ps(st, "key_probe_rows", (uint64_t)x.length * 4);
        launch_key_probe_rows_dict((const int32_t *)x.values, x.validity, x.offset, x.length,
                                   string_desc(*dc, nullptr, plan->fp_key), cells, recs, gathered_cap[k], words, st->stream);
      }
    }
    HIP_TRY(hipGetLastError());
    return TGX_OK;
  }

  // the records of rows task k (device memory, the state's until its next batch or reset)
  tgx_status rows_get(tgx_state *st, size_t k, const void **records, uint64_t *n, tgx_error *err) {
    if (!kp_gathers(tasks[k].mode))
      return fail(err, TGX_INVALID_ARGUMENT, "spec %d: the KEY_PROBE check does not gather rows (tgx_plan_set_key_probe_rows)",
                  tasks[k].spec_index);
    std::vector<ProbeHost> g;
    TGX_TRY(collect(st, &g, err));
    *n = std::min<uint64_t>(g[k].gathered, gathered_cap[k]);
    *records = *n ? gathered[k].p : nullptr;
    return TGX_OK;
  }

  // (KeyedCheck's merge, serialize and read_spec know nothing of a set's identity, of rows that stay, or of `pairs`)
  tgx_status merge_from(tgx_state *st, tgx_state *src, tgx_error *err) override {
    TGX_TRY(rows_stay("merge", err));
    TGX_TRY(static_cast<ProbeCheck *>(of(src))->rows_stay("merge", err));
    std::vector<ProbeHost> theirs, mine;
    TGX_TRY(static_cast<ProbeCheck *>(of(src))->collect(src, &theirs, err));
    TGX_TRY(collect(st, &mine, err));
    for (size_t k = 0; k < theirs.size(); k++)
      if (theirs[k].known && mine[k].known && !theirs[k].same_parent(mine[k]))
        return fail(err, TGX_INVALID_ARGUMENT, "%s task %zu: the states were counted under different %s", kName, k,
                    ProbeKind::kDiffers);
    TGX_TRY(pairs_fit(theirs, err));
    for (size_t k = 0; k < theirs.size(); k++) ProbeKind::merge_host(host[k], theirs[k]);
    return TGX_OK;
  }

  tgx_status serialize(tgx_state *st, Writer &w, tgx_error *err) override {
    TGX_TRY(rows_stay("serialize", err));
    std::vector<ProbeHost> g;
    TGX_TRY(collect(st, &g, err));
    w.pod(ProbeKind::kMagic);
    w.pod((uint32_t)tasks.size());
    for (size_t k = 0; k < g.size(); k++) ProbeKind::write(tasks[k], g[k], w);
    return TGX_OK;
  }

  tgx_status fill_result(tgx_state *st, int slot, tgx_result *r, tgx_error *err) override {
    std::vector<ProbeHost> g;
    TGX_TRY(collect(st, &g, err));
    const ProbeHost &h = g[(size_t)slot];
    r->total = (int64_t)h.seen;
    r->non_null = (int64_t)h.non_null;
    r->distinct = (int64_t)(kp_tuples(tasks[(size_t)slot].mode) ? tuple_classes(h).missing_keys : h.size());
    r->matches = (int64_t)h.matched;
    return TGX_OK;
  }

  // the task of spec `spec_index`, read: the head of tgx_key_probe_get and tgx_key_probe_entries
  static tgx_status read_spec(const tgx_plan *plan, tgx_state *st, size_t spec_index, ProbeHost *out, uint32_t *route,
                              tgx_error *err) {
    size_t slot = 0;
    TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_KEY_PROBE, kName, &slot, err, "bad arguments"));
    ProbeCheck *c = static_cast<ProbeCheck *>(of(st));
    std::vector<ProbeHost> g;
    TGX_TRY(c->collect(st, &g, err));
    *out = std::move(g[slot]);
    if (route) *route = c->parent[slot].has ? (uint32_t)c->parent[slot].route : 0;
    return TGX_OK;
  }
};

}  // namespace

tgx_status keyprobe_plan_add(tgx_plan *plan, int spec_index, int *slot, tgx_error *err) {
  const tgx_check_spec &sp = plan->specs[spec_index];
  if (sp.column2 != -1)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %d: KEY_PROBE reads one column: column2 must be -1 (%d)", spec_index,
                sp.column2);
  KeyProbeTask t;
  memset(&t, 0, sizeof(t));  // (not set; its mode is of no account until it is)
  t.column = sp.column;
  t.spec_index = spec_index;
  plan->key_probes.push_back(t);
  *slot = (int)plan->key_probes.size() - 1;
  return TGX_OK;
}

tgx_status keyprobe_plan_ready(const tgx_plan *plan, tgx_error *err) {
  for (const KeyProbeTask &t : plan->key_probes)
    if (!t.set)
      return fail(err, TGX_INVALID_ARGUMENT, "spec %d: a KEY_PROBE check needs its parameters (tgx_plan_set_key_probe)",
                  t.spec_index);
  return TGX_OK;
}

void keyprobe_mark_columns(tgx_plan *plan) {
  for (const KeyProbeTask &t : plan->key_probes) {
    side_mark(plan, ProbeCheck::kIndex, t.column, true);
    for (int c = 0; c < t.n_tuple; c++) side_mark(plan, ProbeCheck::kIndex, t.tuple[c], true);
  }
}

tgx_status keyprobe_check_column(const tgx_plan *plan, int column, const tgx_column &c, tgx_error *err) {
  const int type = c.type;
  // a strings task takes the string layouts and nothing else; every other task refuses them (below)
  // a tuples task takes both, component by component
  bool strings = false, others = false, in_tuple = false;
  for (const KeyProbeTask &t : plan->key_probes) {
    if (t.n_tuple) {
      for (int c = 0; c < t.n_tuple; c++) in_tuple |= t.tuple[c] == column;
      continue;
    }
    if (t.column == column) (kp_string_column(t.mode) ? strings : others) = true;
  }
  if (in_tuple) {
    if (refused_as_key(type))
      return fail(err, TGX_UNSUPPORTED, "column %d: KEY_PROBE on tuple keys takes integer and string columns, not %s "
                  "(type %d)", column, type_name(type), type);
    if (!is_any_string(type) && type != TGX_DICT32_UTF8 && c.length > 0 && !c.values)
      return fail(err, TGX_UNSUPPORTED, "column %d: KEY_PROBE reads the keys: a validity-only column has none", column);
    if (!strings && !others) return TGX_OK;
  }
  if (strings && !is_any_string(type) && type != TGX_DICT32_UTF8)
    return fail(err, TGX_UNSUPPORTED, "column %d: KEY_PROBE on string keys takes string columns, not %s (type %d)", column,
                refused_as_key(type) ? type_name(type) : "integers", type);
  if (strings && !others) return TGX_OK;
  if (refused_as_key(type))
    return fail(err, TGX_UNSUPPORTED, "column %d: KEY_PROBE takes integer columns, not %s (type %d)", column,
                type_name(type), type);
  if (is_any_string(type) || type == TGX_DICT32_UTF8)
    return fail(err, TGX_UNSUPPORTED, "column %d: KEY_PROBE takes integer columns, not strings (type %d)", column, type);
  if (c.length > 0 && !c.values)
    return fail(err, TGX_UNSUPPORTED, "column %d: KEY_PROBE reads the keys: a validity-only column has none", column);
  return TGX_OK;
}

bool keyprobe_blob_keyed(tgx_state *st) {
  ProbeCheck *c = static_cast<ProbeCheck *>(ProbeCheck::of(st));
  if (!c) return false;
  for (size_t k = 0; k < c->tasks.size(); k++)
    if (kp_fingerprint_set(c->tasks[k].mode) &&
        ((c->parent[k].has && c->parent[k].keys != 0) || (c->host[k].known && c->host[k].parent_keys != 0)))
      return true;
  return false;
}

SideCheck *keyprobe_state_new(const tgx_plan *plan) { return plan->key_probes.empty() ? nullptr : new ProbeCheck(plan); }

}  // namespace tgx

using namespace tgx;

namespace {
// The nine tgx_plan_set_key_probe* calls: `p` is the call's parameters (a spec that gathers has none to give: its own),
// `max_value_bytes` a strings or counted strings spec's.  (A spec keeps the mode of its first call: a call of another mode is refused)
tgx_status plan_set_mode(tgx_plan *plan, size_t spec_index, KeyProbeMode mode, const tgx_key_probe_params *p,
                         uint32_t max_value_bytes, tgx_error *err) {
  if (!plan || !p) return fail(err, TGX_INVALID_ARGUMENT, kp_gathers(mode) ? "plan is NULL" : "plan/params is NULL");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, nullptr, spec_index, TGX_CHECK_KEY_PROBE, "KEY_PROBE", &slot, err, nullptr));
  if (plan_has_state(plan))
    return fail(err, TGX_INVALID_ARGUMENT, "the parameters of a KEY_PROBE check are fixed once a state of the plan exists");
  if (p->max_missing_keys < 1 || p->max_missing_keys > TGX_KEY_PROBE_MAX_MISSING_KEYS)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_missing_keys must be 1 .. %d (%u)", spec_index,
                (int)TGX_KEY_PROBE_MAX_MISSING_KEYS, p->max_missing_keys);
  if (p->reserved != 0) return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: reserved must be 0 (%u)", spec_index, p->reserved);
  if (kp_string_set(mode) && (max_value_bytes < 1 || max_value_bytes > TGX_KEY_PROBE_MAX_VALUE_BYTES))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: max_value_bytes must be 1 .. %d (%u)", spec_index,
                (int)TGX_KEY_PROBE_MAX_VALUE_BYTES, max_value_bytes);
  KeyProbeTask &t = plan->key_probes[slot];
  if (kp_tuples(mode) && !t.n_tuple)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: tgx_plan_set_key_probe%s needs a spec with a column list "
                "(columns / n_columns of 2 .. %d)", spec_index, kModes[mode].suffix, kKeyProbeMaxTuple);
  if (!kp_tuples(mode) && t.n_tuple)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the spec has a column list: it is set with "
                "tgx_plan_set_key_probe_tuples, _tuples_counted or _rows_tuples", spec_index);
  if (t.set && t.mode != mode)
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the check has been set %s (tgx_plan_set_key_probe%s)", spec_index,
                kModes[t.mode].set_as, kModes[t.mode].suffix);
  t.params = *p;
  t.max_value_bytes = max_value_bytes;
  t.mode = mode;
  t.set = true;
  return TGX_OK;
}

// the task of a spec that spec_slot has accepted
const KeyProbeTask &task_of(const tgx_plan *plan, size_t spec_index) {
  for (const KeyProbeTask &t : plan->key_probes)
    if ((size_t)t.spec_index == spec_index) return t;
  return plan->key_probes.front();  // (cannot happen)
}
}  // namespace

extern "C" tgx_status tgx_plan_set_key_probe(tgx_plan *plan, size_t spec_index, const tgx_key_probe_params *p,
                                             tgx_error *err) try {
  return plan_set_mode(plan, spec_index, kKpPlain, p, 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_counted(tgx_plan *plan, size_t spec_index, const tgx_key_probe_params *p,
                                                     tgx_error *err) try {
  return plan_set_mode(plan, spec_index, kKpCounted, p, 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_rows(tgx_plan *plan, size_t spec_index, tgx_error *err) try {
  const tgx_key_probe_params own = {1, 0};
  return plan_set_mode(plan, spec_index, kKpRows, &own, 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_strings(tgx_plan *plan, size_t spec_index,
                                                     const tgx_key_probe_strings_params *p, tgx_error *err) try {
  const tgx_key_probe_params q = {p ? p->max_missing_keys : 0, 0};
  return plan_set_mode(plan, spec_index, kKpStrings, p ? &q : nullptr, p ? p->max_value_bytes : 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_strings_counted(tgx_plan *plan, size_t spec_index,
                                                             const tgx_key_probe_strings_params *p, tgx_error *err) try {
  const tgx_key_probe_params q = {p ? p->max_missing_keys : 0, 0};
  return plan_set_mode(plan, spec_index, kKpStringsCounted, p ? &q : nullptr, p ? p->max_value_bytes : 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_rows_strings(tgx_plan *plan, size_t spec_index, tgx_error *err) try {
  const tgx_key_probe_params own = {1, 0};
  return plan_set_mode(plan, spec_index, kKpRowsStrings, &own, 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_tuples(tgx_plan *plan, size_t spec_index, const tgx_key_probe_params *p,
                                                    tgx_error *err) try {
  return plan_set_mode(plan, spec_index, kKpTuples, p, 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_tuples_counted(tgx_plan *plan, size_t spec_index,
                                                            const tgx_key_probe_params *p, tgx_error *err) try {
  return plan_set_mode(plan, spec_index, kKpTuplesCounted, p, 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_plan_set_key_probe_rows_tuples(tgx_plan *plan, size_t spec_index, tgx_error *err) try {
  const tgx_key_probe_params own = {1, 0};
  return plan_set_mode(plan, spec_index, kKpRowsTuples, &own, 0, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_tuples_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                               tgx_key_probe_tuples *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  ProbeHost h;
  TGX_TRY(ProbeCheck::read_spec(plan, st, spec_index, &h, nullptr, err));
  const KeyProbeTask &t = task_of(plan, spec_index);
  if (!kp_tuples(t.mode))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the KEY_PROBE check does not read tuple keys "
                "(tgx_plan_set_key_probe_tuples)", spec_index);
  const TupleClasses c = tuple_classes(h);
  memset(out, 0, sizeof(*out));
  out->null_counted = c.null_counted;
  out->null_overflow_rows = h.null_overflow_rows;
  out->null_keys = c.null_keys;
  out->arity = (uint32_t)t.n_tuple;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_entries_tuples(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                                   tgx_key_probe_tuple_entry *entries, uint64_t cap,
                                                   uint64_t *n_entries, tgx_error *err) try {
  bind_thread();
  if (!n_entries) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  ProbeHost h;
  TGX_TRY(ProbeCheck::read_spec(plan, st, spec_index, &h, nullptr, err));
  if (!kp_tuples(task_of(plan, spec_index).mode))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the KEY_PROBE check does not read tuple keys: its missing keys are "
                "read with tgx_key_probe_entries or tgx_key_probe_entries_bytes", spec_index);
  uint64_t n_bytes = 0;
  TGX_TRY(counted_entries_sizes(h.strs.size(), 0, entries, cap, n_entries, nullptr, 0, &n_bytes, err));
  if (!entries) return TGX_OK;
  size_t i = 0;
  for (const auto &e : h.strs) entries[i++] = tuple_entry_of(e.first, e.second);
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_strings_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                                tgx_key_probe_strings *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  ProbeHost h;
  TGX_TRY(ProbeCheck::read_spec(plan, st, spec_index, &h, nullptr, err));
  const KeyProbeTask &t = task_of(plan, spec_index);
  if (!kp_string_set(t.mode))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the KEY_PROBE check does not probe string keys "
                "(tgx_plan_set_key_probe_strings)", spec_index);
  memset(out, 0, sizeof(*out));
  out->long_rows = h.long_rows;
  out->max_value_bytes = t.max_value_bytes;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_entries_bytes(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                                  tgx_value_count_entry *entries, uint64_t cap, uint64_t *n_entries,
                                                  uint8_t *bytes, uint64_t bytes_cap, uint64_t *n_bytes,
                                                  tgx_error *err) try {
  bind_thread();
  if (!n_entries || !n_bytes) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  ProbeHost h;
  TGX_TRY(ProbeCheck::read_spec(plan, st, spec_index, &h, nullptr, err));
  if (!kp_string_set(task_of(plan, spec_index).mode))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the KEY_PROBE check does not probe string keys: its missing keys "
                "are read with tgx_key_probe_entries", spec_index);
  int32_t is_bytes = 0;
  return keyed_entries_out(h, entries, cap, n_entries, bytes, bytes_cap, n_bytes, &is_bytes,
                           [](int64_t key, uint64_t at, uint64_t length, uint64_t count) {
                             return tgx_value_count_entry{key, at, length, count};
                           }, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_rows_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                             const void **device_records, uint64_t *n_records, tgx_error *err) try {
  bind_thread();
  if (!device_records || !n_records) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_KEY_PROBE, "KEY_PROBE", &slot, err, "bad arguments"));
  TGX_TRY(need_device(err));
  return static_cast<ProbeCheck *>(ProbeCheck::of(st))->rows_get(st, slot, device_records, n_records, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_set_parent(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                               const void *device_records, uint64_t n_records, tgx_error *err) try {
  bind_thread();
  size_t slot = 0;
  TGX_TRY(spec_slot(plan, st, spec_index, TGX_CHECK_KEY_PROBE, "KEY_PROBE", &slot, err, "bad arguments"));
  TGX_TRY(need_device(err));
  return static_cast<ProbeCheck *>(ProbeCheck::of(st))->set_parent(st, slot, device_records, n_records, err);
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                        tgx_key_probe_summary *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  ProbeHost h;
  uint32_t route = 0;
  TGX_TRY(ProbeCheck::read_spec(plan, st, spec_index, &h, &route, err));
  memset(out, 0, sizeof(*out));
  out->seen = h.seen;
  out->non_null = h.non_null;
  out->null_rows = h.seen - h.non_null;
  out->matched = h.matched;
  // (a tuples spec: the entries of NULL-bearing tuples are no missing keys -- tgx_key_probe_tuples_get)
  const bool tuples = kp_tuples(task_of(plan, spec_index).mode);
  const TupleClasses classes = tuples ? tuple_classes(h) : TupleClasses();
  out->counted = tuples ? classes.missing_counted : h.counted();
  out->overflow_rows = h.overflow_rows;
  out->missing_rows = out->counted + out->overflow_rows + h.long_rows;  // (long rows: a strings spec's only)
  out->missing_keys = tuples ? classes.missing_keys : h.size();
  out->parent_keys = h.parent_keys;
  out->parent_digest = h.parent_digest;
  out->route = route;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_pairs_get(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                              tgx_key_probe_pairs *out, tgx_error *err) try {
  bind_thread();
  if (!out) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  ProbeHost h;
  TGX_TRY(ProbeCheck::read_spec(plan, st, spec_index, &h, nullptr, err));
  if (!kp_counts(task_of(plan, spec_index).mode))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the KEY_PROBE check is not counted (tgx_plan_set_key_probe_counted)",
                spec_index);
  memset(out, 0, sizeof(*out));
  out->pairs = h.pairs;
  // (rows seen are below 2^63; the sum is still held against the word)
  if (!add_fits(h.pairs, h.seen - h.matched, &out->join_rows))
    return fail(err, TGX_UNSUPPORTED, "spec %zu: the join has more than 2^64 - 1 rows", spec_index);
  out->parent_rows = h.parent_rows;
  out->parent_count_digest = h.parent_count_digest;
  out->max_count = h.max_count;
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}

extern "C" tgx_status tgx_key_probe_entries(const tgx_plan *plan, tgx_state *st, size_t spec_index,
                                            tgx_key_probe_entry *entries, uint64_t cap, uint64_t *n_entries,
                                            tgx_error *err) try {
  bind_thread();
  if (!n_entries) return fail(err, TGX_INVALID_ARGUMENT, "bad arguments");
  ProbeHost h;
  TGX_TRY(ProbeCheck::read_spec(plan, st, spec_index, &h, nullptr, err));
  if (kp_string_set(task_of(plan, spec_index).mode))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the KEY_PROBE check probes string keys: its missing keys are read "
                "with tgx_key_probe_entries_bytes", spec_index);
  if (kp_tuples(task_of(plan, spec_index).mode))
    return fail(err, TGX_INVALID_ARGUMENT, "spec %zu: the KEY_PROBE check reads tuple keys: its entries are read with "
                "tgx_key_probe_entries_tuples", spec_index);
  uint64_t n_bytes = 0;
  TGX_TRY(counted_entries_sizes(h.size(), 0, entries, cap, n_entries, nullptr, 0, &n_bytes, err));
  if (!entries) return TGX_OK;
  size_t i = 0;
  for (const auto &e : h.ints) entries[i++] = tgx_key_probe_entry{e.first, e.second};
  return TGX_OK;
} catch (...) {
  return tgx::abi_exception(err);
}
