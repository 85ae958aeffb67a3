// Device-visible descriptors and partial-state layouts shared by the HIP kernels and the C-ABI
// host code (term_amd/csrc/tgx_api.cpp).  gfx950 only.
#pragma once
#include <stdint.h>

#include "kll_types.h"

namespace tgx {

constexpr int kScanBlock = 256;      // 4 waves of 64
constexpr int kWavesPerBlock = 4;
constexpr int kTileRows = 512;       // rows one wave consumes per iteration: 4 x (64 lanes x 16 B)
constexpr int kMaxScanBlocksPerCol = 2048;  // 256 CUs x 8 resident 256-thread blocks

// One numeric column of one batch, as the scan kernel sees it.
struct ScanColDesc {
  const void *values;       // element 0 of the Arrow values buffer (int64 / float64)
  const uint8_t *validity;  // LSB-first bitmap or nullptr
  int64_t offset;           // Arrow offset (slots)
  int64_t length;           // rows
  int64_t head;             // rows [0, head): ragged edge, per-lane path
  int64_t n_tiles;          // full kTileRows tiles starting at row `head` (0 => whole column ragged)
  int32_t is_float;
  int32_t want_variance;
  const double *pivot;      // device scalar: shift for the variance lanes (may be nullptr)
  int32_t elem32;           // 1: `values` holds 4-byte elements (Int32 / Float32), widened as they are loaded
  int32_t skip_stats;       // scan_hll_kernel: nobody asked for MIN / MAX / SUM of this column -- COUNT and registers only
  ScanKll kll;              // kll.picks != nullptr: the column's KLL sampler rides on this scan (kll_types.h)
  uint8_t *hll;             // scan_hll_kernel: [workgroup][kHllRegisters] register bytes of this launch (else nullptr)
  uint8_t *hll_regs;        // ... and the task's running registers the launch is folded into (hll_reduce_kernel)
};

// HyperLogLog lane of the scan (APPROX_DISTINCT, TG/constraints/approx_count_distinct.rs:56-66): 2^14 registers like
// DataFusion's sketch (datafusion-functions-aggregate 50.3.0, hyperloglog.rs: HLL_P = 14).  A value's 64 bits are
// mixed by a bijection into (a, b): register = low 14 bits of a, rank = leading zeros of b + 1 (1 .. 33).
constexpr int kHllBits = 14;
constexpr int kHllRegisters = 1 << kHllBits;
constexpr int kHllMaxRank = 33;
__host__ __device__ inline uint32_t hll_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__host__ __device__ inline void hll_hash(uint64_t bits, uint32_t *a_out, uint32_t *b_out) {
  const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
  uint32_t a = lo ^ hll_rotl32(hi * 0x9E3779B1u, 15);
  a ^= a >> 16;  // Murmur3's 32-bit finaliser
  a *= 0x85EBCA6Bu;
  a ^= a >> 13;
  a *= 0xC2B2AE35u;
  a ^= a >> 16;
  const uint32_t b = (hi ^ hll_rotl32(a, 16)) * 0x27D4EB2Fu;  // (only its leading zeros are used)
  *a_out = a;
  *b_out = b;
}

// Per (column, block) partial written by scan_kernel; reduced in fixed order by scan_reduce_kernel.
struct ScanPartial {
  int64_t non_null;
  int64_t min_k, max_k;     // int64 values, or IEEE totalOrder keys of the doubles
  uint64_t sum_lo;          // int64 columns: 128-bit two's complement sum
  int64_t sum_hi;
  double sum, comp;         // float64 columns: two-sum compensated sum (sum + comp)
  double s1, s2;            // sum(x - pivot), sum((x - pivot)^2) over doubles
};

// Running per-column state (device resident between batches, merged on the host at finalize).
struct ScanAcc {
  int64_t total;            // rows seen
  int64_t non_null;
  int64_t min_k, max_k;
  uint64_t sum_lo;
  int64_t sum_hi;
  double sum, comp;
  // variance lanes as (n, mean, M2) so batches / ranks merge with Chan's formula
  int64_t var_n;
  double var_mean, var_m2;
  int32_t is_float;
  int32_t pad;
};

// Launch descriptors travel BY VALUE in the kernel-argument segment (no host->device copy, no
// synchronisation per batch, nothing to keep alive): at most kMaxColsPerLaunch columns per launch.
constexpr int kMaxColsPerLaunch = 24;
struct ScanLaunch {
  ScanColDesc cols[kMaxColsPerLaunch];
  int32_t acc_index[kMaxColsPerLaunch];  // running-state slot of each column
};

// Two columns scanned TOGETHER by one workgroup (scan_pair_kernel): their own aggregates as above plus the raw
// co-moments over the rows where both are non-NULL -- a COMOMENTS check whose columns also carry NUMERIC_STATS /
// COUNT / KLL checks costs no second pass over them.  Both columns share head / n_tiles (same length, offsets
// congruent modulo 64).
struct ScanPairDesc {
  ScanColDesc x, y;
  int32_t x_acc, y_acc;   // running-state slots of the two columns (-1: the column has no scan task of its own)
  int32_t como_acc;       // running-state slot of the pair's co-moments
  int32_t pad;
};
constexpr int kMaxPairsPerLaunch = 8;
struct ScanPairLaunch {
  ScanPairDesc pairs[kMaxPairsPerLaunch];
};

// Validity-only columns (COUNT(*), COUNT(col)).
struct CountColDesc {
  const uint8_t *validity;  // never nullptr here (no-validity columns are answered on the host)
  int64_t offset;
  int64_t length;
};

struct CountLaunch {
  CountColDesc cols[kMaxColsPerLaunch];
  int32_t acc_index[kMaxColsPerLaunch];
};

struct CountAcc {
  int64_t total;
  int64_t non_null;
};

// Two-column co-moments, accumulated about a per-pair PIVOT (px, py) that the first batch picks near the data
// (como_pivot_kernel): sums of (x - px), (y - py) and their products.  DataFusion's CORR / COVAR_SAMP are online
// (Welford) accumulators (TG/constraints/correlation.rs:260-275): on offset data -- timestamps, ids around 1e9 -- the
// raw sums SUM(x*x), SUM(x*y) cancel catastrophically in n*Sxy - Sx*Sy, the shifted ones do not.  The raw sums the
// CorrelationAnalyzer reports (TG/analyzers/advanced/correlation.rs:239-249) are rebuilt from the shifted ones on the
// host (tgx_finalize).
struct ComomentColDesc {
  const void *x, *y;
  const uint8_t *xv, *yv;
  int64_t xoff, yoff;
  int64_t length;
  int32_t x_is_float, y_is_float;  // (SPEARMAN: 2 = a widened Float32 column, whose rank keys quiet their NaNs)
};

struct ComomentLaunch {
  ComomentColDesc pairs[kMaxColsPerLaunch];
  int32_t acc_index[kMaxColsPerLaunch];
};

// per (pair, block) partial of the co-moment kernels (comoments.hip, scan_pair_kernel): sums about the pair's pivot
struct ComomentPartial {
  int64_t n;
  double s[5], c[5];
};

struct ComomentAcc {
  int64_t total;
  int64_t n;
  // sums of x', y', x'x', y'y', x'y' with x' = x - px, y' = y - py, as (sum, compensation)
  double s[5], c[5];
  double px, py;       // the pivots: fixed once rows have been folded in (n > 0); (0, 0) = the raw sums
  int32_t pivot_set;
  int32_t pad;
};

// Joint bin counts of two numeric columns (kernels/jointbins.hip; TGX_CHECK_JOINT_BINS).  The pairs of a launch travel as
// ComomentColDesc (same loads as the co-moment kernel); `acc_index` is the task's slot.
// Range phase: n, rows with a NaN / infinity, and the extremes over the rows with both sides non-NULL and finite.
struct JointRangeAcc {
  int64_t n, non_finite;
  double x_min, x_max, y_min, y_max;  // identities: +inf / -inf
};
// Count phase: the task's binning; its global counters are [cells][kJointOutOfRange][kJointNonFinite] 64-bit words.
struct JointBinning {
  double x_origin, x_width, y_origin, y_width;
  uint32_t bins;
  uint32_t pad;
};
constexpr uint32_t kJointMaxBins = 127;  // (bins + 1)^2 32-bit LDS counters: 64 KiB
constexpr int kJointBlock = 512;         // threads of a workgroup of the two kernels
constexpr int kMaxJointPerLaunch = 8;
struct JointLaunch {
  ComomentColDesc pairs[kMaxJointPerLaunch];
  JointBinning binning[kMaxJointPerLaunch];
  unsigned long long *counters[kMaxJointPerLaunch];  // count phase: the task's global counters
  int32_t acc_index[kMaxJointPerLaunch];             // range phase: the task's JointRangeAcc
};
__host__ __device__ inline uint32_t joint_cells(uint32_t bins) { return (bins + 1) * (bins + 1); }

// Temporal row predicates over one or two Int64-shaped columns (kernels/temporal.hip; TGX_CHECK_TEMPORAL).  The tasks of
// a launch travel as ComomentColDesc (ORDER: x = before, y = after; the single-column modes read x only).  Per task two
// 64-bit global counters: [0] rows that are non-NULL (both sides in ORDER mode) and pass the weekday filter, [1] those
// of them that pass the predicate.  What a NULL row counts as is decided on the host from these and the rows seen.
enum { kTemporalOrder = 1, kTemporalTimeOfDay = 2, kTemporalRange = 3 };
struct TemporalParams {
  int32_t mode;
  int32_t weekdays_only;
  int64_t delta;             // ORDER: passes iff after - before >= delta (no wrap-around)
  int64_t ticks_per_second;  // TIME_OF_DAY: 1, 10^3, 10^6 or 10^9
  int64_t lo, hi;            // TIME_OF_DAY: ticks into the day; RANGE: the bounds; both ends inclusive
};
constexpr int kTemporalBlock = 512;
constexpr int kMaxTemporalPerLaunch = 8;
struct TemporalLaunch {
  ComomentColDesc cols[kMaxTemporalPerLaunch];
  TemporalParams params[kMaxTemporalPerLaunch];
  unsigned long long *counters[kMaxTemporalPerLaunch];
};

// Numeric value rules over one column (kernels/valuerule.hip; TGX_CHECK_VALUE_RULE).  A launch's tasks are COLUMN
// GROUPS: one walk of a column (ComomentColDesc, the x side only) evaluates up to kValueRulesPerGroup rules of it.  The
// host has reduced every comparison mode to one inclusive range test lo <= k <= hi on a key it names -- the int64 value
// itself, or the IEEE totalOrder key (f64_total_key below) of the value as a double -- so GE_ZERO is [key(+0.0), max],
// GT_ZERO [key(+0.0) + 1, max] and BETWEEN its own bounds, in either domain.  Per rule three 64-bit global counters at
// counts[word]: [0] valid rows, [1] cast errors (kRuleInteger), [2] non-NULL rows -- counted once per group, in the
// counters of its first rule.
enum { kRuleRangeValue = 0, kRuleRangeKey = 1, kRuleInteger = 2 };
struct ValueRule {
  int64_t lo, hi;  // the two range kinds: both ends inclusive, in the key's domain
  uint32_t word;   // first of the rule's three counters
  int32_t kind;
};
constexpr int kValueRuleBlock = 512;
constexpr int kMaxValueRuleGroupsPerLaunch = 8;
constexpr int kValueRulesPerGroup = 8;
constexpr int kValueRuleWords = 3;
struct ValueRuleLaunch {
  ComomentColDesc cols[kMaxValueRuleGroupsPerLaunch];
  ValueRule rules[kMaxValueRuleGroupsPerLaunch][kValueRulesPerGroup];
  int32_t n_rules[kMaxValueRuleGroupsPerLaunch];
  unsigned long long *counts;
};

// Value counts of one column (kernels/valuecounts.hip; TGX_CHECK_VALUE_COUNTS): a bounded GROUP BY.  A task's running
// state on the device is one open-addressing table of `mask + 1` slots (a power of two >= 2 * max_distinct) in one
// allocation, plus kValueCountsWords 64-bit counters.
//   numeric keys: keys[slot] (the int64 value; all-ones = free, the VALUE -1 is counted in a word of its own),
//                 counts[slot]
//   string keys:  keys[slot] / keys2[slot] (the two fingerprint words; fingerprint.h never produces all-ones),
//                 counts[slot], lens[slot] and the value's bytes at store + slot * max_value_bytes, written by the lane
//                 that claimed the slot
// A key that finds no slot within kValueCountsProbes probes adds its weight to the overflow word.
// (kVcLong is not the last word: the kernels flush it as the first of a pair of counters, bin_count.h's tail_flush)
enum { kVcNonNull = 0, kVcMarker = 1, kVcLong = 2, kVcOverflow = 3, kValueCountsWords = 4 };
constexpr int kValueCountsBlock = 1024;       // numeric route: 16 waves share one LDS table
constexpr uint32_t kValueCountsLdsSlots = 8192;  // 8-byte keys + 4-byte counts: 96 KiB of LDS a workgroup
constexpr uint32_t kValueCountsLdsProbes = 8;
constexpr uint32_t kValueCountsStrLdsSlots = 1024;   // string route: two key words, a row and a count: 28 KiB
constexpr uint32_t kValueCountsDictLdsCells = 16384;  // dictionary route: 32-bit cells in LDS up to this many entries
constexpr uint32_t kValueCountsProbes = 256;
struct ValueCountsTable {
  unsigned long long *keys, *keys2, *counts;
  uint32_t *lens;
  uint8_t *store;
  unsigned long long *words;  // kValueCountsWords counters
  uint64_t mask;
  uint64_t salt;  // numeric keys are mixed with it before they are hashed (from the plan's fingerprint key)
  uint32_t max_value_bytes;
  uint32_t pad;
};

// Pair counts of two columns (kernels/paircounts.hip; TGX_CHECK_PAIR_COUNTS): a bounded GROUP BY x, y.  A side is a
// string column (the cell is the value's bytes) or a numeric one (the cell is its bin index).  A task's running state in
// its count phase is one open-addressing table of `mask + 1` slots (a power of two >= 2 * max_pairs) in one allocation,
// keyed by the pair's fingerprint (keys / keys2), plus kPairCountsWords 64-bit counters; per slot and side a 32-bit
// word (a string side: the value's length; a binned side: its bin index) and, for a string side, the value's bytes at
// store + slot * max_value_bytes, written by the lane that claimed the slot.  In its range phase it is a PairRangeAcc.
// (the counters are flushed in pairs, bin_count.h's tail_flush: both | long, non-finite | out of range)
enum { kPcBoth = 0, kPcLong = 1, kPcNonFinite = 2, kPcOutOfRange = 3, kPcOverflow = 4, kPairCountsWords = 5 };
enum { kPairSideValue = 0, kPairSideRange = 1, kPairSideBinned = 2 };  // (TGX_PAIR_SIDE_*)
constexpr int kPairCountsBlock = 256;         // 4 waves share one LDS table of kValueCountsStrLdsSlots slots (28 KiB)
constexpr int64_t kPairCountsRowsPerLane = 16;  // rows a lane takes before another workgroup is worth its flush
constexpr int kPairCountsMaxBlocks = 2048;
// one side of a pair as the kernels see it
struct PairSide {
  const uint8_t *validity;  // the rows' bitmap or nullptr
  int64_t offset;           // the rows' Arrow offset
  const void *values;       // numeric side: 8-byte values (Int64 / Float64 after the widening staging)
  const int32_t *indices;   // dictionary side: the rows' indices into `str` (then `str` is the dictionary)
  const void *str_offsets;  // string side: the layout of utf8_value_of (Utf8ColDesc), of the column or its dictionary
  const uint8_t *str_data;
  const void *str_views;
  const uint8_t *const *str_buffers;
  const uint8_t *dict_validity;  // dictionary side: a NULL entry makes the row a NULL row
  int64_t dict_offset, dict_length;
  double origin, width;  // binned side
  uint32_t bins;
  int32_t mode;          // kPairSide*
  int32_t is_float;      // numeric side
  int32_t large_offsets;
};
struct PairCountsTable {
  unsigned long long *keys, *keys2, *counts;
  uint32_t *cell[2];  // per side: length or bin index
  uint8_t *store[2];  // per string side: the bytes
  unsigned long long *words;  // kPairCountsWords counters
  uint64_t mask;
  uint32_t max_value_bytes;
  uint32_t pad;
};
// range phase: the numeric side over the rows with both sides non-NULL; the extremes as IEEE totalOrder keys
// (f64_total_key: signed order), so that every word is folded with one 64-bit vector atomic
struct PairRangeAcc {
  long long both, n, non_finite;
  long long min_key, max_key;  // identities: INT64_MAX / INT64_MIN
};

// Group counts (kernels/groupcounts.hip; TGX_CHECK_GROUP_COUNTS): a bounded GROUP BY g with COUNT(*) and, for up to
// kGroupCountsMembers value columns that ride the walk, COUNT(col).  The walk's running state is one open-addressing
// table of `mask + 1` slots in one allocation, laid out as ValueCountsTable's is (keys / keys2, totals, lens, store),
// with the members' 64-bit non_null counters between the totals and the lengths: member m's counter of slot s is
// non_null[m * (mask + 1) + s].  Every task has kGroupCountsWords 64-bit counters: the walk's rows with a NULL key,
// with a key longer than max_value_bytes, whose key found no slot, whose key has the bits of the free-slot marker --
// those four in the walk's FIRST task only (`shared_word`) -- and behind each the member's rows of that class whose
// value is non-NULL (GroupMembers::word).
enum {
  kGcNullRows = 0, kGcNullNonNull = 1, kGcLongRows = 2, kGcLongNonNull = 3, kGcOverflowRows = 4, kGcOverflowNonNull = 5,
  kGcMarkerRows = 6, kGcMarkerNonNull = 7, kGroupCountsWords = 8
};
constexpr int kGroupCountsMembers = 8;
constexpr int kGroupCountsBlock = 1024;  // numeric route: 16 waves share one LDS table
// numeric route: slots of the workgroup's LDS table by member count (8-byte key, 4-byte total, 4 bytes a member):
// 128 KiB with one member, 80 .. 128 KiB with two to five, 72 .. 88 KiB with six to eight
__host__ __device__ constexpr uint32_t group_counts_lds_slots(int members) {
  return members <= 1 ? 8192u : members <= 5 ? 4096u : 2048u;
}
constexpr uint32_t kGroupCountsDictLdsCells = 16384;  // dictionary route: 32-bit cells in LDS, (1 + members) an entry
struct GroupMembers {
  const uint8_t *validity[kGroupCountsMembers];  // the value column's bitmap, or nullptr: every row is non-NULL
  int64_t offset[kGroupCountsMembers];           // its Arrow offset, unrelated to the group column's
  uint32_t word[kGroupCountsMembers];            // first of the member's counters in `words`
  int32_t n;
  int32_t pad;
};
struct GroupCountsTable {
  unsigned long long *keys, *keys2, *totals, *non_null;
  uint32_t *lens;
  uint8_t *store;
  unsigned long long *words;  // the state's counters (GroupMembers::word and shared_word index them)
  uint64_t mask;
  uint64_t salt;
  uint32_t max_value_bytes;
  uint32_t shared_word;  // first of the counters of the walk's first task
};

// Group sums (kernels/groupsums.hip; TGX_CHECK_GROUP_SUMS): a bounded GROUP BY g with COUNT(*), COUNT(col) and
// SUM(col) of ONE value column.  A task's running state is one open-addressing table laid out as GroupCountsTable's
// is, with two 64-bit counters a slot behind the rows: non_null[s] and sum[s] (the bits of an int64 that wraps, or of a
// double -- all-zero is +0.0, so clearing is the same).  Every task has kGroupSumsWords 64-bit counters: rows,
// non_null and sum of each of the four classes of rows that are in no slot.
enum {
  kGsNull = 0, kGsLong = 3, kGsOverflow = 6, kGsMarker = 9, kGroupSumsWords = 12  // (+0 rows, +1 non_null, +2 sum)
};
constexpr int kGroupSumsBlock = 1024;  // numeric route: 16 waves share one LDS table
// numeric route: the workgroup's LDS table: 8-byte key, 4-byte rows, 4-byte non_null, 8-byte sum = 24 bytes a slot,
// 96 KiB of the CU's 160 (8192 slots would not fit): one workgroup a CU
constexpr uint32_t kGroupSumsLdsSlots = 4096;
// string route: VcLdsStrings' slots with a non_null and a sum: 40 bytes a slot, 40 KiB
constexpr uint32_t kGroupSumsStrLdsSlots = kValueCountsStrLdsSlots;
// dictionary route: entries whose cells (4-byte rows, 4-byte non_null, 8-byte sum) are kept in LDS: 64 KiB
constexpr uint32_t kGroupSumsDictLdsEntries = 4096;
// the value column of a walk
struct GroupSumsValue {
  const void *values;       // 8-byte values (Int64 / Float64 after the widening staging)
  const uint8_t *validity;  // or nullptr: every row is non-NULL
  int64_t offset;           // its Arrow offset, unrelated to the group column's
};
struct GroupSumsTable {
  unsigned long long *keys, *keys2, *rows, *non_null, *sums;
  uint32_t *lens;
  uint8_t *store;
  unsigned long long *words;  // the task's kGroupSumsWords counters
  uint64_t mask;
  uint64_t salt;
  uint32_t max_value_bytes;
  uint32_t pad;
};

// Key probe (kernels/keyprobe.hip; TGX_CHECK_KEY_PROBE): is each child key in the parent's key set?  The set is read-only
// while rows are walked: a bitmap of 32-bit words over [base, base + range) (route 1), or an open-addressing table of
// `mask + 1` 64-bit keys at load <= 0.5 (route 2: kEmptyKey = free, probed linearly from mix64(key) & mask; the key whose
// bits are the marker is the flag has_marker).  A COUNTED set keeps how often each key occurs in the parent: an array of
// 64-bit counts over [base, base + range) (route 3: 0 = not in the set), or a table of `mask + 1` 16-byte {key, count}
// slots, probed as route 2's is (route 4: the marker key's count is marker_count).  The keys that are NOT in the set are
// counted in a bounded table laid out as ValueCountsTable's integer half is; the missing key whose bits are the marker
// has a counter of its own.
// (kKpNonNull | kKpMatched are flushed as a pair, bin_count.h's tail_flush; kKpPairs: the sum of the multiplicities of
// the matched rows' keys, which only a counted task adds to; a task that gathers a STRING column probes nothing and
// keeps its cursor, the records it has written, in that word: a dictionary batch makes fewer records than it has rows)
enum { kKpNonNull = 0, kKpMatched = 1, kKpMarker = 2, kKpOverflow = 3, kKpPairs = 4, kKeyProbeWords = 5 };
enum { kKpRouteEmpty = 0, kKpRouteBitmap = 1, kKpRouteHash = 2, kKpRouteCountArray = 3, kKpRouteCountHash = 4 };
constexpr int kKeyProbeBlock = 1024;              // 16 waves share one LDS table of missing keys
constexpr uint32_t kKeyProbeLdsSlots = 8192;      // 8-byte keys + 4-byte counts: 96 KiB of LDS a workgroup
constexpr uint32_t kKeyProbeLdsProbes = 8;
constexpr uint32_t kKeyProbeProbes = 256;         // of the task's global table of missing keys
constexpr int kMaxKeyProbePerLaunch = 8;
struct KeyProbeSet {
  const uint32_t *bits;              // route 1: (range + 31) / 32 words
  const unsigned long long *keys;    // route 2: mask + 1 slots
  const unsigned long long *counts;  // route 3: `range` counts; route 4: mask + 1 slots of {key, count}, 16-byte aligned
  uint64_t base, range;              // routes 1, 3: the cell of key k is k - base, for k - base < range (unsigned)
  uint64_t mask;                     // routes 2, 4
  uint64_t marker_count;             // route 4: how often the key whose bits are kEmptyKey occurs in the parent
  uint32_t has_marker;               // route 2: the key whose bits are kEmptyKey is in the set
  uint32_t pad;
};
struct KeyProbeTable {
  unsigned long long *keys, *counts;  // the missing keys and their rows
  unsigned long long *words;          // the task's kKeyProbeWords counters
  uint64_t mask;
  uint64_t salt;
};
struct KeyProbeLaunch {
  ComomentColDesc cols[kMaxKeyProbePerLaunch];
  KeyProbeSet sets[kMaxKeyProbePerLaunch];
  KeyProbeTable tables[kMaxKeyProbePerLaunch];
};
// what the build of a set leaves behind: a reduction over the records, then the counts of the distinct inserts
struct KeyProbeBuild {
  long long min, max;                  // identities: INT64_MAX / INT64_MIN
  unsigned long long keys, digest;     // distinct keys and the wrapping sum of mix64(key ^ kKeyProbeDigestSalt) over them
  unsigned int has_marker, pad;
  // a counted set's reduction: records whose count is 0; the counts' sum in three pieces (bits 0..20, 21..41, 42..63 of
  // every count, summed apart: no piece's sum can wrap below 2^40 records, so the host has the exact total); the wrapping
  // sum of count * mix64(key ^ kKeyProbeCountSalt); and, from the build, the largest count a key has come to
  // and the marker key's count
  unsigned long long zero_counts, sum_piece[3], count_digest, max_count, marker_count;
};
// A STRINGS task (kernels/keyprobe_strings.hip): the child column is a string column and the set holds the parent's
// values as keyed 128-bit fingerprints (route 5: `mask + 1` 16-byte {fa, fb} slots at load <= 0.5, probed linearly from
// fa & mask; a slot is free while its fa word is kEmptyKey, which fingerprint.h never produces).  The missing keys are
// counted in a table laid out as ValueCountsTable's string half is (a ValueCountsTable whose `words` are the task's
// kKeyProbeWords counters).  No string has the marker's bits: the word counts the missing rows whose value is longer
// than max_value_bytes instead.
enum { kKpLong = kKpMarker, kKpRouteStrings = 5 };
struct KeyProbeStringSet {
  const unsigned long long *slots;  // mask + 1 slots of {fa, fb}, 16-byte aligned; null: the empty set
  uint64_t mask;
};
// what the build of such a set leaves behind: the distinct fingerprints, the wrapping sum of
// mix64(mix64(fa ^ kKeyProbeDigestSalt) ^ fb) over them, and the records that hold a marker word (refused by the host)
struct KeyProbeStringsBuild {
  unsigned long long keys, digest, marker_records;
};
// A COUNTED strings task: route 6 is route 5's slot table with, beside it, one 64-bit count per slot -- how often the
// slot's value occurs in the parent.  A miss touches the slot table only; a hit reads its slot's count.  (A type of its
// own: the kernels take the set as a template parameter, and the plain task's instantiation stays what it was.)
enum { kKpRouteStringsCounted = 6 };
struct KeyProbeCountedStringSet {
  const unsigned long long *slots;   // as KeyProbeStringSet's
  uint64_t mask;
  const unsigned long long *counts;  // mask + 1 counts, parallel to the slots
};
// what the build of such a set leaves behind: KeyProbeStringsBuild's three, and KeyProbeBuild's counted reduction with
// count * mix64(mix64(fa ^ kKeyProbeCountSalt) ^ fb) as the count digest's term
struct KeyProbeCountedStringsBuild {
  unsigned long long keys, digest, marker_records;
  unsigned long long zero_counts, sum_piece[3], count_digest, max_count;
};
constexpr uint64_t kKeyProbeDigestSalt = 0x9e3779b97f4a7c15ULL;
constexpr uint64_t kKeyProbeCountSalt = 0xc2b2ae3d27d4eb4fULL;
constexpr int kKpPieceBits = 21;

// Histogram of one numeric column (kernels/histogram.hip; TGX_CHECK_HISTOGRAM).  The columns of a launch travel as
// ComomentColDesc (the x side only: the single-column walk of row_walk.h); `acc_index` is the task's slot.
// Range phase: n, rows with a NaN / infinity, the extremes and the raw sums over the non-NULL, finite rows.
struct HistRangeAcc {
  int64_t n, non_finite;
  double min, max;          // identities: +inf / -inf
  double sum, sum_squared;  // plain sums of x and of the rounded squares x * x
};
// Count phase: the task's `buckets + 1` edges in device memory; its global counters are
// [buckets][kHistElse][kHistNonFinite] 64-bit words.
constexpr uint32_t kHistMaxBuckets = 1000;
constexpr int kHistBlock = 512;  // threads of a workgroup of the two kernels
constexpr int kMaxHistPerLaunch = 8;
struct HistLaunch {
  ComomentColDesc cols[kMaxHistPerLaunch];
  const double *edges[kMaxHistPerLaunch];           // count phase
  uint32_t buckets[kMaxHistPerLaunch];              // count phase
  unsigned long long *counters[kMaxHistPerLaunch];  // count phase: the task's global counters
  int32_t acc_index[kMaxHistPerLaunch];             // range phase: the task's HistRangeAcc
};
// dynamic LDS of a count-phase workgroup: the edges, then 32-bit bucket counters
__host__ __device__ inline size_t hist_lds_bytes(uint32_t buckets) {
  return (size_t)(buckets + 1) * sizeof(double) + (size_t)buckets * sizeof(unsigned int);
}

// One (column, batch) window of the library-side batch coalescing (kernels/gather.hip): where the window lives and
// where it lands in the coalesced column.  A table of these is uploaded per flush; one workgroup per entry.
struct GatherSeg {
  const void *src_values;       // kind 0: first value of the window; kinds 1 / 2: its first offset (length + 1 offsets)
  const uint8_t *src_validity;  // byte holding the window's first validity bit, or nullptr (no nulls)
  const uint8_t *src_data;      // strings: the window's first value byte (offset value data_first)
  void *dst_values;             // the coalesced column's values / offsets buffer (element 0)
  uint8_t *dst_validity;        // the coalesced bitmap (zeroed before the gather), or nullptr (no segment has nulls)
  uint8_t *dst_data;            // strings: the coalesced value bytes
  int64_t src_bit0;             // bit of row 0 within *src_validity (0..7)
  int64_t length;               // rows
  int64_t dst_row;              // first row in the coalesced column
  int64_t data_first, data_base, data_len;  // strings: first source offset value, destination byte position, bytes
  int32_t elem_bytes;           // kind 0: 8 or 4
  int32_t kind;                 // 0 fixed width, 1 Utf8 (int32 offsets), 2 LargeUtf8 (int64 offsets),
                                // 3 Utf8View (16-byte views), 4 dictionary indices (int32, shifted)
  // kind 3: the stretches of the window's data buffers its long views point into (at most kGatherViewBufs buffers per
  // window): stretch k is bytes [vb_min, vb_min + vb_len) of source buffer vb_index, copied from vb_src to
  // dst_data + vb_base; a long view (buffer, offset) becomes (0, vb_base + offset - vb_min)
  int32_t vb_count;
  int32_t index_shift;          // kind 4: added to every index (where the window's dictionary starts in the coalesced one)
  int32_t vb_index[4];
  int64_t vb_min[4], vb_len[4], vb_base[4];
  const uint8_t *vb_src[4];
};
constexpr int kGatherViewBufs = 4;

// tgx_state_reset: the small per-state accumulators back to their identities with ONE launch (a copy and five fills
// were five trips through the runtime: 35 us of a 1.8 ms step)
constexpr int kResetRegions = 8;
struct StateResetArgs {
  void *zero[kResetRegions];       // regions to clear (16-byte aligned allocations)
  uint32_t zero_bytes[kResetRegions];
  int32_t n_zero;
  ScanAcc *ident;                  // the scan accumulators: set to their identity (MIN = INT64_MAX, MAX = INT64_MIN, else 0)
  uint32_t n_ident;
};

// Scratch of the pivot kernels' grid-wide search for a first valid row (kernels/pivot_search.h): one per scan slot and
// one per COMOMENTS task, zero between launches (the search's finishing kernel clears it again).
struct PivotSearch {
  unsigned long long best;  // ~(first row found by this launch); 0: none
  unsigned long long pad;
};
constexpr int64_t kPivotSearchRows = 1 << 18;  // rows per workgroup of the search (grids of at most kPivotSearchBlocks)
constexpr int kPivotSearchBlocks = 4096;

__host__ __device__ inline int64_t f64_total_key(int64_t bits) {
  return bits ^ (int64_t)(((uint64_t)(bits >> 63)) >> 1);
}

// The bits of a Float32 as the bits of the Float64 it stands for, bit-preserving (include/tgx.h, TGX_FLOAT32): the
// hardware conversion (IEEE mode) quiets a signalling NaN, which would make 0x7F800001 and 0x7FC00001 one key, so a
// NaN is rebuilt from its own sign and payload, quiet bit as it was.  Subnormals convert exactly (f32 denormals are
// kept: the kernels' float_denorm_mode_32 is 3).
__device__ __forceinline__ int64_t f32_widen_bits(uint32_t u) {
  const int64_t hw = __double_as_longlong((double)__uint_as_float(u));
  const uint64_t nan = ((uint64_t)(u & 0x80000000u) << 32) | 0x7FF0000000000000ull | ((uint64_t)(u & 0x7FFFFFu) << 29);
  return (u & 0x7FFFFFFFu) > 0x7F800000u ? (int64_t)nan : hw;
}

}  // namespace tgx
