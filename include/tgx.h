/*
 * tgx.h -- C ABI of libtgx, the MI355X (gfx950) execution path for term-guard's Arrow-batch
 * check evaluator.
 *
 * The reference (term-guard 0.0.2, /root/reference/term-guard/src = "TG/") has no FFI of its own:
 * every check is a SQL string handed to DataFusion (`ctx.sql(..).collect()`), e.g.
 * TG/constraints/completeness.rs:158-167.  The drop-in boundary is therefore the reference's own
 * extension traits -- `Constraint::evaluate` (TG/core/constraint.rs:187-225) and
 * `Analyzer::{compute_state_from_data, merge_states, compute_metric_from_state}`
 * (TG/analyzers/traits.rs:65-148).  A `GpuConstraint: Constraint` on the Rust side (INTEGRATION.md
 * shows the binding) streams the table's RecordBatches, hands the raw Arrow buffers of each needed
 * column to `tgx_update`, and reads the aggregates back with `tgx_finalize`; each entry point
 * below names the reference interface it stands in for.
 *
 * Conventions
 *   - plain C, no C++ / torch / HIP types in any signature; HIP streams travel as `void*`.
 *   - every function returns a tgx_status and, when `err` is non-NULL, fills it on failure;
 *     nothing aborts or throws across the boundary (maps to TermError::Internal, TG/error.rs:89-90).
 *   - column buffers follow the Arrow C Data Interface layout (LSB-first validity bitmap, NULL
 *     when the array has no nulls; `offset` counts slots and applies to validity and values alike).
 *   - the caller owns column buffers; HOST buffers may be released when tgx_update returns, DEVICE
 *     buffers must stay alive AND UNMODIFIED until the next tgx_finalize / tgx_state_sync on that
 *     state (work is queued, small batches are only noted, a key set may walk a batch a second
 *     time, a SPEARMAN pair's first batch is ranked from the columns themselves: see tgx_update).
 *   - handles are not thread-safe; distinct handles are independent.  One HIP stream per state.
 *   - there is NO CPU fallback: without a usable gfx950 device tgx_init fails with TGX_NO_DEVICE
 *     and every compute entry point fails with it too.
 */
#ifndef TGX_H
#define TGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: tgx_column grew the Utf8View fields, tgx_check_spec the column list and LENGTH bounds,
 *    tgx_distinct_adopt_slices a slice stride */
/* 3: tgx_comm / tgx_allreduce (the cross-rank step behind the C ABI) */
/* 4: tgx_result grew the centred co-moments (co_*) at its end; state blobs are version 2 */
/* 5: tgx_type grew Int8 .. UInt64 / Boolean, tgx_memspace TGX_MEM_HOST_RETAINED; tgx_trim, tgx_cache_stats_get,
 *    tgx_state_pending (no struct changed its layout) */
/* 6: keyed fingerprints (tgx_plan_set_fingerprint_key / _get_, tgx_blob_fingerprint_key), TGX_FLAG_EXACT_KEYS; state
 *    blobs are version 3 (they carry the key) */
#define TGX_ABI_VERSION 6

typedef enum tgx_status {
  TGX_OK = 0,
  TGX_INVALID_ARGUMENT = 1,
  TGX_UNSUPPORTED = 2, /* type/shape/pattern outside the path: caller falls back to the stock SQL constraint */
  TGX_DEVICE_ERROR = 3,
  TGX_OUT_OF_MEMORY = 4,
  TGX_INTERNAL = 5,
  TGX_NO_DEVICE = 6
} tgx_status;

typedef struct tgx_error {
  int32_t code; /* tgx_status */
  char msg[256];
} tgx_error;

/* ---- column views (Arrow layout) ------------------------------------------------------- */
typedef enum tgx_type {
  TGX_INT64 = 1,
  TGX_FLOAT64 = 2,
  TGX_UTF8 = 3,        /* int32 offsets */
  TGX_LARGE_UTF8 = 4,  /* int64 offsets */
  /* Dictionary<Int32, Utf8|LargeUtf8>: int32 indices in `values` (validity/offset/length describe the
   * indices), the dictionary is a Utf8 column view of its own (any memory space). COUNT, DISTINCT and
   * REGEX_MATCH give the results of the decoded column: string work runs once per dictionary entry,
   * every batch may bring its own dictionary (unused and repeated entries allowed). A row whose dictionary
   * VALUE is NULL is a NULL row for every check (Arrow's logical nulls). */
  TGX_DICT32_UTF8 = 5,
  /* Utf8View (what DataFusion reads Parquet strings as): 16-byte views in `values` -- {int32 length, 12 inline
   * bytes} for length <= 12, else {int32 length, 4-byte prefix, int32 buffer index, int32 offset} -- and
   * `n_variadic` data buffers.  `variadic` is a HOST array of the buffers' pointers (the buffers themselves live
   * in `mem`); `variadic_sizes` (bytes, host array) is required for TGX_MEM_HOST columns, which are staged.
   * COUNT, DISTINCT and REGEX_MATCH give the results of the same values held as Utf8. */
  TGX_UTF8_VIEW = 6,
  /* 4-byte numerics: Int32 (also Date32, Time32) and Float32.  `values` holds 4 bytes per row.  Every check sees
   * exactly the Int64 / Float64 column the values stand for -- DataFusion's own coercion for SUM / AVG (Float64
   * accumulators), value-preserving for MIN / MAX / COUNT(DISTINCT): COUNT and NUMERIC_STATS read the 4-byte values
   * in place (widened in registers); for DISTINCT, KLL, COMOMENTS and SPEARMAN the batch's window is widened into a
   * staging buffer on the device first (one extra pass over those columns).  Int64-shaped Arrow types (Timestamp, Date64, Time64, Duration) are passed as
   * TGX_INT64 as they are.
   * Float32 widens bit-preservingly: normal and subnormal values exactly, a NaN to the Float64 NaN of the same sign and
   * payload, its quiet bit as it was -- a signalling NaN and the quiet NaN of its payload stay two keys for DISTINCT,
   * multiplicity and APPROX_DISTINCT, and MIN / MAX order the widened bits.  SPEARMAN ranks CAST(x AS DOUBLE), where
   * every NaN is quiet. */
  TGX_INT32 = 7,
  TGX_FLOAT32 = 8,
  /* Narrow and unsigned integers (round 5): the reference's completeness / uniqueness SQL takes any column type
   * (TG/constraints/completeness.rs:158-163, uniqueness.rs:612-617) and Parquet tables are full of these.  `values`
   * holds 1 / 2 / 4 bytes per row; the batch's window is widened to Int64 on the device (value-preserving: every check
   * then sees the Int64 column the values stand for -- SUM in Int64 as DataFusion's for signed inputs; its UInt64 sum
   * of unsigned inputs has the same value while it fits).  Small HOST batches are coalesced like Int64 ones (widened
   * on their way into the pinned arena); DEVICE batches of these types are launched as they arrive. */
  TGX_INT8 = 9,
  TGX_INT16 = 10,
  TGX_UINT8 = 11,
  TGX_UINT16 = 12,
  TGX_UINT32 = 13,
  /* UInt64: 8 bytes per row read in place.  COUNT and DISTINCT only (a key is its bit pattern: COUNT(DISTINCT) is exact);
   * a plan that asks a statistic, a sketch or a correlation of such a column gets TGX_UNSUPPORTED from tgx_update --
   * the reference itself cannot read MIN / MAX / SUM of a UInt64 column (statistics.rs:277-308). */
  TGX_UINT64 = 14,
  /* Boolean: `values` is a bit-packed buffer like `validity` (bit `offset + i` = row i).  COUNT and DISTINCT only
   * (false and true are the keys 0 and 1); anything else is TGX_UNSUPPORTED (MIN / MAX of a Boolean column come back
   * Boolean in DataFusion: "Failed to extract statistic value" in the reference). */
  TGX_BOOL = 15
} tgx_type;

typedef enum tgx_memspace {
  TGX_MEM_HOST = 0,
  TGX_MEM_DEVICE = 1,
  /* HOST buffers the caller keeps alive AND unmodified until the next flushing call (tgx_finalize, tgx_state_sync,
   * tgx_state_serialize, tgx_merge, tgx_allreduce, tgx_state_reset) -- the contract DEVICE buffers have.  What it
   * buys: a small batch (coalesced, below) is only NOTED -- its windows are copied into the pinned arena by the
   * library's copy threads at some point between this call and the flush (every few MB of noted windows are handed to
   * the threads that are idle; the flush waits for them and copies the rest), instead of window by window on the
   * calling thread inside tgx_update (one core moves ~27 GB/s: the cap of a stream of 8192-row batches).  A consumer of
   * DataFusion's `execute_stream()` holds the RecordBatches (Arc'd buffers) until it syncs.  Batches that are not
   * coalesced are read before tgx_update returns, as TGX_MEM_HOST ones are.  All HOST columns of a batch should be
   * given the same way (a batch that mixes the two is taken as TGX_MEM_HOST). */
  TGX_MEM_HOST_RETAINED = 2
} tgx_memspace;

typedef struct tgx_column {
  int32_t type;            /* tgx_type */
  int32_t mem;             /* tgx_memspace: where every buffer below lives */
  int64_t length;          /* rows */
  int64_t offset;          /* Arrow `offset`: first logical slot */
  int64_t null_count;      /* -1 = unknown */
  const uint8_t *validity; /* may be NULL (no nulls) */
  const void *values;      /* fixed-width values / dictionary indices */
  const void *offsets;     /* Utf8: length+1 (+offset) int32/int64 offsets */
  const uint8_t *data;     /* Utf8: value bytes */
  const struct tgx_column *dictionary; /* TGX_DICT32_UTF8 only */
  const uint8_t *const *variadic;      /* TGX_UTF8_VIEW only: host array of n_variadic data buffer pointers */
  const int64_t *variadic_sizes;       /* TGX_UTF8_VIEW only: host array of their sizes in bytes (HOST columns) */
  int32_t n_variadic;
  int32_t reserved;
} tgx_column;

/* ---- check specs: the aggregates the reference's constraints emit as SQL ------------------ */
typedef enum tgx_check_kind {
  /* COUNT(*), COUNT(col)                       TG/constraints/completeness.rs:158-163,
   *                                            TG/analyzers/basic/{size,completeness}.rs */
  TGX_CHECK_COUNT = 1,
  /* MIN MAX SUM AVG [STDDEV VARIANCE]          TG/constraints/statistics.rs:45-74, :263;
   *                                            TG/analyzers/basic/{min_max,mean,sum}.rs */
  TGX_CHECK_NUMERIC_STATS = 2,
  /* COUNT(DISTINCT col) [+ GROUP BY col counts] TG/constraints/uniqueness.rs:612-617, 671-681, 709-715 */
  TGX_CHECK_DISTINCT = 3,
  /* COUNT(CASE WHEN [TRIM(]c[)] ~|~* 'pat' [OR c IS NULL] THEN 1 END), COUNT(*)
   *                                            TG/constraints/format.rs:750-776 */
  TGX_CHECK_REGEX_MATCH = 4,
  /* KllSketch::update over the column's non-NULL, non-NaN values (Int64 CAST AS DOUBLE)
   *                                            TG/analyzers/advanced/kll_sketch.rs:195-229
   * The sketch itself does not depend on kll_k (512-item runs, < 1024 raw items): k sets the stated bound
   * tgx_kll_relative_error_bound(k) = 1.65/sqrt(k) and the merge check only.  Its actual rank error is about
   * 0.1-0.2 %, so the bound holds up to k = 65536 (0.64 %) but not for k above roughly 10^6. */
  TGX_CHECK_KLL = 5,
  /* n, Sx, Sy, Sxx, Syy, Sxy over rows with both columns non-NULL (CAST AS DOUBLE)
   *                                            TG/analyzers/advanced/correlation.rs:239-249
   * and the centred moments behind CORR / COVAR_SAMP   TG/constraints/correlation.rs:260-275 */
  TGX_CHECK_COMOMENTS = 6,
  /* n and the sums of SQL RANK() ranks (min-rank ties) of both columns over rows with both non-NULL
   * (CAST AS DOUBLE), reported in sum_x .. sum_xy          TG/analyzers/advanced/correlation.rs:334-350 */
  TGX_CHECK_SPEARMAN = 7,
  /* COUNT(CASE WHEN LENGTH(c) >= length_min AND LENGTH(c) <= length_max OR c IS NULL THEN 1 END), COUNT(*):
   * LENGTH counts characters (code points), NULL rows always count    TG/constraints/length.rs:36-45, 167-171.
   * Result: total, matches. */
  TGX_CHECK_LENGTH = 8,
  /* APPROX_DISTINCT(col): a HyperLogLog estimate of COUNT(DISTINCT col)   TG/constraints/approx_count_distinct.rs:56-66.
   * One more lane of the numeric scan (2^14 one-byte registers like DataFusion's sketch; mergeable by max, so it
   * shards, merges and serializes like every other state): the column is read once at streaming speed instead of
   * going through the exact key set.  Result: `distinct` = the estimate (standard error 1.04 / sqrt(2^14) = 0.8 %; the
   * reference's own tests allow 3 %), total, non_null.  Int64 / Float64 / Int32 / Float32 columns (Float64 by bit
   * pattern, like DISTINCT); on string and dictionary columns -- and whenever the plan also holds an exact DISTINCT
   * check of the column -- the exact count answers (it satisfies every bound the estimate does). */
  TGX_CHECK_APPROX_DISTINCT = 9,
  /* The joint bin counts behind MutualInformationAnalyzer's numeric x numeric branch
   *                                            TG/analyzers/advanced/mutual_information.rs:143-248
   * over the pair (`column`, `column2`), every value CAST AS DOUBLE, in TWO PHASES -- the bin edges depend on the whole
   * table, so the reference scans twice and so does the caller here:
   *   range phase (no binning set on the spec): n and MIN / MAX of both columns over the rows where both sides are
   *     non-NULL and finite; read with tgx_joint_range_get;
   *   count phase (tgx_plan_set_joint_binning was called for the spec): per such row
   *     i = FLOOR((x - x_origin) / x_width), j = FLOOR((y - y_origin) / y_width), evaluated in IEEE double arithmetic
   *     exactly as written (the division is correctly rounded), and cell (i, j) of a (bins + 1) x (bins + 1) table of
   *     64-bit counts goes up by one (the column's maximum lands in bin `bins` or `bins - 1`); read with
   *     tgx_joint_counts.
   * A row with a NULL on either side is dropped (as COMOMENTS does).  A row with a NaN or an infinity on either side
   * is left out of n, the range and the cells and counted as `non_finite` (the reference's own behaviour there is an
   * accident of FLOOR(NaN) and pinned by nothing).  tgx_result carries total (rows seen) and non_null (n).
   * Columns: Int64, Float64, and Int32 / Float32 / Int8 .. UInt32 through the widening staging; UInt64, Boolean and every
   * string layout are TGX_UNSUPPORTED.  The state is additive: tgx_merge, state blobs and tgx_allreduce combine the
   * extremes by MIN / MAX and n and the cells by addition. */
  TGX_CHECK_JOINT_BINS = 10,
  /* The row predicates behind TemporalOrderingConstraint's three pure-scan modes
   *                                            TG/constraints/temporal_ordering.rs:346-453
   * each a SELECT COUNT(*), SUM(CASE WHEN <predicate> THEN 0 ELSE 1 END) FROM t WHERE ... over one or two Int64-shaped
   * columns (Timestamp / Date64 / Int64), everything in the column's own ticks.  `column` is the timestamp column, or the
   * BEFORE column in order mode; `column2` is the AFTER column in order mode and -1 otherwise.  The mode and its
   * parameters come with tgx_plan_set_temporal (below); a spec without them makes tgx_state_create fail.  Read with
   * tgx_temporal_get; tgx_result carries total = rows seen, non_null = rows considered, matches = considered -
   * violations.  Every other column type is TGX_UNSUPPORTED from tgx_update.  The state is three counters: tgx_merge,
   * state blobs and tgx_allreduce add them. */
  TGX_CHECK_TEMPORAL = 11,
  /* The two scans behind HistogramAnalyzer         TG/analyzers/advanced/histogram.rs:184-330
   * over `column`, every value CAST AS DOUBLE, in TWO PHASES -- the bucket edges depend on the whole table, so the
   * reference scans twice and so does the caller here:
   *   range phase (no edges set on the spec): n, MIN, MAX, SUM(c) and SUM(c * c) over the rows that are non-NULL and
   *     finite; the sums are plain double sums (they carry the reference's own cancellation; nothing is pivoted); read
   *     with tgx_histogram_range_get;
   *   count phase (tgx_plan_set_histogram_edges was called for the spec, with buckets + 1 edges): per such row x the
   *     bucket is the first i in 0 .. buckets-1 with edges[i] <= x < edges[i+1], else buckets-1 -- the reference's
   *     CASE WHEN .. ELSE num_buckets (histogram.rs:262-294) taken literally, including for rows below edges[0] or at
   *     or above edges[buckets]; read with tgx_histogram_counts.
   * A NULL row is dropped (WHERE c IS NOT NULL).  A NaN or an infinity is left out of n, the range, the sums and the
   * buckets and counted as `non_finite` (the reference's own behaviour there is an accident of comparisons with NaN and
   * pinned by nothing).  tgx_result carries total (rows seen) and non_null (the non-NULL rows: n + non_finite).
   * Columns: Int64, Float64, and Int32 / Float32 / Int8 .. UInt32 through the widening staging; UInt64, Boolean and every
   * string layout are TGX_UNSUPPORTED.  The state is additive: tgx_merge, state blobs and tgx_allreduce combine the
   * extremes by MIN / MAX and n, the sums and the buckets by addition. */
  TGX_CHECK_HISTOGRAM = 12,
  /* The window query behind TemporalOrderingConstraint's MaxTimeGap mode
   *                                            TG/constraints/temporal_ordering.rs:454-481
   *   SELECT ts - LAG(ts) OVER ([PARTITION BY g] ORDER BY ts) FROM t WHERE ts IS NOT NULL
   * `column` is the timestamp column t (Int64-shaped: Timestamp / Date64 / Duration / Int64, in its own ticks), `column2`
   * the group column g or -1.  The threshold comes with tgx_plan_set_time_gap (below); a spec without it makes
   * tgx_state_create fail.  The rules:
   *   - a row whose t is NULL is seen and otherwise ignored (the query's WHERE clause; there is no flag that keeps it);
   *   - without g the remaining rows form one partition; with g there is one partition per value of g, and ALL rows
   *     whose g is NULL form one partition of their own (SQL's PARTITION BY);
   *   - within a partition the timestamps are put in non-decreasing order; every row but the first has a gap
   *     t_i - t_(i-1), taken as an unsigned 64-bit value (INT64_MAX - INT64_MIN is 2^64 - 1, not -1); equal timestamps
   *     give gap 0, so the answer depends only on the multiset of (g, t), never on tie order or batching;
   *   - gaps = non-NULL rows - non-empty partitions; violations = gaps with gap > max_gap (a negative max_gap makes every
   *     gap a violation, a gap equal to max_gap is none); largest_gap = the maximum gap, unsigned, 0 when there is none.
   * The reference compares EXTRACT(EPOCH FROM ts - LAG(ts)), a Float64 number of seconds, with the literal; this check
   * compares ticks exactly (the two agree for every gap below 2^53 ticks).
   * Read with tgx_time_gap_get; tgx_result carries total = rows seen, non_null = gaps, matches = gaps - violations.
   * Group columns: Int64-shaped, and Int32 / Date32 / Int8 .. UInt32 through the widening staging; UInt64, Boolean, floats
   * and every string or binary layout are TGX_UNSUPPORTED from tgx_update, as is every timestamp column that is not
   * Int64-shaped.  The state RETAINS its rows on the device until it is reset (8 B per row, 16 B with a group) and sorts
   * them when it is read; specs on the same (t, g) that differ only in max_gap share one copy and one sort.  More than
   * 2^32 - 1 retained rows in a task are TGX_UNSUPPORTED.  Such a state is not additive: tgx_merge, tgx_state_serialize
   * and tgx_allreduce on a state whose TIME_GAP task holds rows return TGX_UNSUPPORTED (an empty one passes). */
  TGX_CHECK_TIME_GAP = 13,
  /* The numeric row predicates behind DataTypeConstraint
   *                                            TG/constraints/datatype.rs:144-160, 383-439
   *   SELECT COUNT(*) AS total, SUM(CASE WHEN <predicate> THEN 1 ELSE 0 END) AS valid FROM t WHERE col IS NOT NULL
   * over one numeric column: `column` names it, `column2` is -1.  The rule and its bounds come with
   * tgx_plan_set_value_rule (below, which also holds the rules' exact semantics); a spec without them makes
   * tgx_state_create fail.  Read with tgx_value_rule_get; tgx_result carries total = rows seen, non_null = rows
   * considered (the non-NULL rows), matches = valid rows, distinct = cast errors (INTEGER mode).
   * Columns: the Int64-shaped ones (Int64 / Timestamp / Date64 / Duration), Float64, and Int32 / Date32 / Float32 /
   * Int8 .. UInt32 through the widening staging; UInt64, Boolean and every string layout are TGX_UNSUPPORTED from
   * tgx_update, and the state stays usable afterwards.  The state is four counters: tgx_merge, state blobs and
   * tgx_allreduce add them.  A blob counted under other parameters is refused. */
  TGX_CHECK_VALUE_RULE = 14,
  /* How often each value of one column occurs: the GROUP BY behind HistogramConstraint and EntropyAnalyzer
   *                          TG/constraints/histogram.rs:205-391, TG/analyzers/advanced/entropy.rs:192-335
   *   SELECT col, COUNT(*) FROM t WHERE col IS NOT NULL GROUP BY col
   * for a BOUNDED number of distinct values: `column` names the column, `column2` is -1, the bounds come with
   * tgx_plan_set_value_counts (below); a spec without them makes tgx_state_create fail.  Read with
   * tgx_value_counts_get and tgx_value_counts_entries; tgx_result carries total = rows seen, non_null, distinct = values
   * held, matches = rows counted in them.
   * The counts are exact.  Everything beyond the bounds is reported, never approximated: a non-NULL row is in exactly
   * one of an entry, overflow_rows (its value found no slot in the table) and long_rows (a string longer than
   * max_value_bytes), so counted + overflow_rows + long_rows == non_null always holds.
   * Columns: the Int64-shaped ones, Int32 / Date32 and Int8 .. UInt32 through the widening staging (the value is the
   * widened int64), Utf8, LargeUtf8, Utf8View and Dictionary<Int32, Utf8> (the value is the string's bytes; the empty
   * string is a value; rows whose dictionary entry is NULL, or whose index lies outside the dictionary, are NULL rows).
   * The value of a string layout is its BYTES: a Binary column handed over in a string layout is counted as well, and
   * what its values read as is the caller's business (the host layer refuses columns declared Binary).  Float32 / Float64, UInt64 and Boolean are
   * TGX_UNSUPPORTED from tgx_update, and the state stays usable afterwards.
   * Within one state strings are grouped by their 128-bit keyed fingerprint -- the guarantee the library gives for keys
   * that cross a state boundary (TGX_CHECK_DISTINCT without TGX_FLAG_EXACT_KEYS) -- and every entry keeps its bytes;
   * across states, blobs and ranks entries are united by their bytes.  Integer and dictionary-index counts are exact by
   * construction.  tgx_merge, state blobs and tgx_allreduce unite by value and add the counters. */
  TGX_CHECK_VALUE_COUNTS = 15,
  /* How often each PAIR of cells of two columns occurs: the GROUP BY behind MutualInformationAnalyzer's three
   * categorical branches (string x string, numeric x string, string x numeric)
   *                          TG/analyzers/advanced/mutual_information.rs:249-293
   *   SELECT cell(x), cell(y), COUNT(*) FROM t WHERE x IS NOT NULL AND y IS NOT NULL GROUP BY 1, 2
   * for a BOUNDED number of distinct pairs: `column` is x, `column2` is y, the bounds and what a cell is on either side
   * come with tgx_plan_set_pair_counts (below); a spec without them makes tgx_state_create fail.  A side is
   *   TGX_PAIR_SIDE_VALUE   a string column (Utf8, LargeUtf8, Utf8View, Dictionary<Int32, Utf8>): the cell is the string's
   *                         bytes, the empty string is a value; a row whose dictionary entry is NULL, or whose index lies
   *                         outside the dictionary, is a NULL row (the rules of TGX_CHECK_VALUE_COUNTS);
   *   TGX_PAIR_SIDE_BINNED  a numeric column (the types JOINT_BINS takes): the cell is the integer
   *                         FLOOR((CAST(v AS DOUBLE) - origin) / width) in IEEE double arithmetic as written (the one
   *                         index function of JOINT_BINS); a row holding a NaN or an infinity is counted in non_finite, a
   *                         row whose index falls outside [0, bins] in out_of_range;
   *   TGX_PAIR_SIDE_RANGE   a numeric column, and the spec is in its RANGE phase: nothing is counted into a table; the
   *                         state is n, MIN, MAX (as doubles) and non_finite of that side over the rows where BOTH sides
   *                         are non-NULL (rows with a NaN or an infinity left out, as JOINT_BINS does); read with
   *                         tgx_pair_range_get.
   * Two numeric sides are refused by tgx_plan_set_pair_counts: that is TGX_CHECK_JOINT_BINS.  A side whose mode does
   * not fit its column, and a UInt64, Boolean, binary, decimal or validity-only column on either side, are
   * TGX_UNSUPPORTED from tgx_update, and the state stays usable afterwards.
   * Read with tgx_pair_counts_get and tgx_pair_counts_entries; tgx_result carries total = rows seen, non_null = rows
   * with both sides non-NULL, distinct = pairs held, matches = rows counted in them.
   * The counts are exact.  Everything beyond the bounds is reported, never approximated: a row with both sides non-NULL
   * is in exactly one of an entry, overflow_rows (its pair found no slot in the table), long_rows (a string on either
   * side longer than max_value_bytes), non_finite and out_of_range, so
   *   counted + overflow_rows + long_rows + non_finite + out_of_range == both_non_null
   * always holds.
   * The grouping guarantee is the one of TGX_CHECK_VALUE_COUNTS: within one state pairs are grouped by a 128-bit keyed
   * fingerprint of the PAIR (each string side reduced to its fingerprint, a binned side to its index, the two cells
   * chained as the components of a tuple key are -- never a concatenation of the bytes: ("ab", "c") and ("a", "bc") are
   * different pairs) and every entry keeps its bytes; across states, blobs and ranks entries are united by their bytes
   * (and bin indices).  tgx_merge, state blobs and tgx_allreduce unite by value and add the counters; a range-phase
   * state merges MIN / MAX / counters as JOINT_BINS's does. */
  TGX_CHECK_PAIR_COUNTS = 16,
  /* Completeness per group, "metrics per segment": the GROUP BY behind CompletenessAnalyzer::with_grouping
   *                          TG/analyzers/grouped.rs, TG/analyzers/basic/grouped_completeness.rs:160-200
   *   SELECT g, COUNT(*) AS total_count, COUNT(col) AS non_null_count FROM t GROUP BY g
   * for a BOUNDED number of groups: `column` is the value column col, of which only the validity is read (every type
   * TGX_CHECK_COUNT takes, validity-only columns included), `column2` is the group column g; the bounds come with
   * tgx_plan_set_group_counts (below); a spec without them makes tgx_state_create fail.
   * Rows with a NULL group key are a group, as in SQL: they are counted apart (null_group_rows, null_group_non_null),
   * not in the table.  A row whose dictionary entry is NULL, or whose index lies outside the dictionary, is a NULL-key
   * row (the rule of TGX_CHECK_VALUE_COUNTS).
   * Group columns: those of TGX_CHECK_VALUE_COUNTS -- the Int64-shaped ones, Int32 / Date32 and Int8 .. UInt32 through
   * the widening staging, Utf8, LargeUtf8, Utf8View and Dictionary<Int32, Utf8>.  Float32 / Float64, UInt64, Boolean
   * and validity-only group columns are TGX_UNSUPPORTED from tgx_update, and the state stays usable afterwards.
   * Nothing is approximated: every row is in exactly one of an entry, the NULL group, overflow_rows (its key found no
   * slot in the table) and long_rows (a string key longer than max_value_bytes), and so is every row with a non-NULL
   * value:
   *   counted + null_group_rows + overflow_rows + long_rows == seen
   *   counted_non_null + null_group_non_null + overflow_non_null + long_non_null == COUNT(col)
   * Specs that share the group column and both bounds share one walk of the group column and one table on the device
   * (up to eight value columns a walk, each adding one validity bit a row); the walk's shared counters are reported in
   * every member's summary.  The grouping guarantee is the one of TGX_CHECK_VALUE_COUNTS: within one state string keys
   * are grouped by their 128-bit keyed fingerprint and every entry keeps its bytes; across states, blobs and ranks
   * entries are united by their bytes.  tgx_merge, state blobs and tgx_allreduce unite by value and add every counter.
   * Read with tgx_group_counts_get and tgx_group_counts_entries; tgx_result carries total = rows seen, non_null =
   * COUNT(col), distinct = groups held (the NULL group not among them), matches = rows counted in them.
   *
   * GROUP BY SEVERAL COLUMNS.  A spec with column2 == -1 and a column list (columns / n_columns, 2 .. 8) groups by the
   * TUPLE of the listed columns, in the list's order; `column` stays the value column (the list does not overwrite it,
   * as it does for the other kinds that take a list).  A list together with column2 >= 0, a list of one column, more
   * than 8 columns, a NULL list and a negative index are refused by tgx_plan_create; the bounds, the reads and the
   * summary are the ones above.
   *   Components   are read as TGX_CHECK_KEY_PROBE's tuples read them: integers widened to int64 (the Int64-shaped
   *                types, Int32 / Date32, Int8 .. UInt32), strings of any of the four layouts; a dictionary component
   *                whose index is negative or outside the dictionary, or whose entry is NULL, is a NULL component and
   *                is never read; each component sits under its own Arrow offset.  Float32 / Float64, UInt64, Boolean
   *                and validity-only group columns are TGX_UNSUPPORTED from tgx_update, refused before anything runs.
   *   NULL         is a value, as in SQL's GROUP BY: (NULL, 'a'), ('', 'a') and (NULL, NULL) are three groups and are
   *                entries like any other; null_group_rows and null_group_non_null are always 0.
   *   An entry's key is the concatenation of its components' canonical bytes:
   *                NULL      0x00
   *                integer   0x01, then the 8 big-endian bytes of value ^ 2^63
   *                string    0x02, then the length as 2 big-endian bytes, then the bytes
   *                The form is prefix-free per component, so injective for a given arity; a narrow column and a wide one
   *                give the same bytes; bytewise ascending order -- the order of the entries, which come with
   *                *is_bytes = 1 -- is lexicographic by component, NULL before integers before strings, integers in
   *                numeric order, strings by length and then bytewise.  A row whose encoded key is longer than max_value_bytes is a long row (long_rows); a
   *                string component of 65 536 bytes or more makes one by construction.
   *   Grouping     on the device rows are grouped by the tuple's keyed 128-bit fingerprint -- the function, bit for bit,
   *                that TGX_CHECK_DISTINCT and TGX_CHECK_KEY_PROBE give a tuple -- and the entry keeps the encoded
   *                bytes: grouped by fingerprint within a state, united by bytes across states, blobs and ranks.
   *   Walks        tuple specs that name the same list in the same order, with the same bounds, share one walk (up to
   *                eight value columns).
   * The identities above hold unchanged.  In a state blob the task's record carries its arity (0 for a single group
   * column); a blob whose arity differs from the plan's task is refused, as is one whose keys are not encoded tuples of
   * that arity. */
  TGX_CHECK_GROUP_COUNTS = 17,
  /* A sum per group: each side of the reference's CrossTableSumConstraint
   *                          TG/constraints/cross_table_sum.rs:251-262
   *   SELECT g, COUNT(*) AS rows, COUNT(col) AS non_null, SUM(col) AS sum FROM t GROUP BY g
   * for a BOUNDED number of groups: `column` is the value column col, `column2` is the group column g (the same column
   * is allowed); the bounds come with tgx_plan_set_group_sums (below); a spec without them makes tgx_state_create fail.
   * Group columns, the NULL group, the NULL-entry and index-outside-the-dictionary rules, the free-slot marker and the
   * grouping guarantee are those of TGX_CHECK_GROUP_COUNTS.
   * Value columns and what the sum is:
   *   Int64-shaped, Int32 / Date32, Int8 .. UInt32 (widened)   a 64-bit WRAPPING integer sum, the sum_i of tgx_result
   *                         (DataFusion's SUM for these inputs): exact, so independent of batching, association, merge
   *                         order and rank count.  Reported in sum_i; sum_f is (double)sum_i.
   *   Float64, Float32 (widened)   a plain IEEE double sum in whatever order the device adds.  NaN and +-inf propagate
   *                         by IEEE rules; there is no non_finite class.  A group that holds only -0.0 may come out as
   *                         +0.0.  Reported in sum_f; sum_i is 0.
   *   UInt64, Boolean, string and validity-only value columns are TGX_UNSUPPORTED from tgx_update (as are the group
   *   columns TGX_CHECK_GROUP_COUNTS refuses), and the state stays usable afterwards.
   * Nothing is approximated: every row is in exactly one of an entry, the NULL group, overflow (its key found no slot
   * in the table) and long rows (a string key longer than max_value_bytes).  Each class carries rows, non_null and sum:
   *   counted + null_group_rows + overflow_rows + long_rows == seen
   *   counted_non_null + null_group_non_null + overflow_non_null + long_non_null == COUNT(col)
   * and, for integer value columns, exact in wrapping arithmetic,
   *   counted.sum_i + null_group.sum_i + overflow.sum_i + long_rows.sum_i == SUM(col).
   * One value column a walk: two specs on one group column each walk it.  tgx_merge, state blobs and tgx_allreduce
   * unite by value; integer sums add with wrap, float sums add in state order and rank order.  A state that summed
   * integers and one that summed floats do not merge, nor do integer-key and string-key states.
   * Read with tgx_group_sums_get and tgx_group_sums_entries; tgx_result carries total = rows seen, non_null =
   * COUNT(col), distinct = groups held, matches = rows counted in them, sum_i / sum_f = the sum over all classes,
   * has_value = 0 when COUNT(col) is 0.
   * GROUP BY SEVERAL COLUMNS: a spec with column2 == -1 and a column list of 2 .. 8 columns groups by the tuple of the
   * listed columns, with the row rules, the canonical key bytes, the grouping guarantee and the blob rule written down
   * for TGX_CHECK_GROUP_COUNTS; `column` stays the value column (it may be one of the listed columns), the null_group
   * class is always empty, and the identities hold unchanged. */
  TGX_CHECK_GROUP_SUMS = 18,
  /* Is each key of a child column in a parent's key set?  The device side of the reference's ForeignKeyConstraint
   *                          TG/constraints/foreign_key.rs:152-176
   *   SELECT COUNT(*), COUNT(DISTINCT child.c) FROM child LEFT JOIN parent ON child.c = parent.p
   *   WHERE parent.p IS NULL [AND child.c IS NOT NULL]
   * for integer keys: `column` is the child key column c (column2 must be -1); the bound on the missing keys that are
   * kept comes with tgx_plan_set_key_probe (below); a spec without it makes tgx_state_create fail.  The parent's key set
   * belongs to a STATE: tgx_key_probe_set_parent gives it, before the state's first batch; tgx_update on a state whose
   * task has none is TGX_INVALID_ARGUMENT naming the spec.  tgx_state_reset clears the counters and the missing keys and
   * keeps the set.
   * Child columns: the Int64-shaped ones, Int32 / Date32 and Int8 .. UInt32 through the widening staging (the key is the
   * sign- or zero-extended value, which is what TGX_CHECK_DISTINCT keeps for a parent column of those types: a narrow
   * parent joins a wide child as SQL's coercion does).  Float32 / Float64, UInt64, Boolean and every string layout are
   * TGX_UNSUPPORTED from tgx_update, and the state stays usable afterwards.
   * The counts are exact and nothing is approximated: a NULL row is in null_rows; a non-NULL row is matched (its key is
   * in the set) or missing, and a missing row is in exactly one of an entry of the missing keys and overflow_rows (its
   * key found no slot in the table of 2 * max_missing_keys slots, probed as TGX_CHECK_VALUE_COUNTS's is), so
   *   seen == non_null + null_rows,  non_null == matched + missing_rows,  missing_rows == counted + overflow_rows
   * always hold, and with overflow_rows == 0 missing_keys is the exact COUNT(DISTINCT) of the violating keys.  The key
   * whose bits are the table's free-slot marker (int64 -1) is an ordinary key on both sides.
   * tgx_merge, state blobs and tgx_allreduce add the counters and unite the missing keys by value; states whose parent
   * sets differ (parent_keys, parent_digest) do not merge.  A deserialized state holds no set: it can be read and merged,
   * and takes batches again once tgx_key_probe_set_parent has given it a set with the same (parent_keys, parent_digest).
   * Read with tgx_key_probe_get and tgx_key_probe_entries; tgx_result carries total = rows seen, non_null = non-NULL
   * rows, matches = matched rows, distinct = missing keys held.
   * Two further modes of a spec, each with a plan call of its own: COUNTED (tgx_plan_set_key_probe_counted: the set keeps
   * the parent's multiplicities and the state sums them over the matched rows -- the join's matched pairs,
   * tgx_key_probe_pairs_get) and ROWS (tgx_plan_set_key_probe_rows: the spec gathers its column as {key, 1} records for
   * such a set instead of probing it, tgx_key_probe_rows_get).  String keys have the same three: STRINGS
   * (tgx_plan_set_key_probe_strings), COUNTED STRINGS (tgx_plan_set_key_probe_strings_counted) and ROWS STRINGS
   * (tgx_plan_set_key_probe_rows_strings).  A spec with a column list (`columns` / `n_columns` of 2 .. 8) reads TUPLE
   * keys -- a composite join key, JoinCoverageConstraint::on_multiple -- and has the same three again: TUPLES
   * (tgx_plan_set_key_probe_tuples), COUNTED TUPLES (tgx_plan_set_key_probe_tuples_counted) and ROWS TUPLES
   * (tgx_plan_set_key_probe_rows_tuples); the row rules stand beside tgx_key_probe_tuples_get. */
  TGX_CHECK_KEY_PROBE = 19,
  /* A row predicate over 1 .. 8 columns: the rows on which a closed boolean expression is TRUE, and those on which it is
   * UNKNOWN -- the device side of the reference's Check::satisfies (TG/constraints/custom_sql.rs:192-282) and of its
   * ComplianceAnalyzer (TG/analyzers/advanced/compliance.rs:136-204), both one
   *     SELECT COUNT(CASE WHEN <expr> THEN 1 END), COUNT(*) FROM t
   * The spec names its columns through `columns` / `n_columns` (1 .. 8; `column2` must be -1); the predicate -- leaves,
   * a postfix program over them and a pool of literal bytes -- comes with tgx_plan_set_row_predicate (below, which also
   * holds the exact semantics); a spec without it makes tgx_state_create fail.  Read with tgx_row_predicate_get;
   * tgx_result carries total = rows seen, matches = satisfied rows, non_null = seen - unknown.  The state is additive
   * counters: tgx_merge, blobs and tgx_allreduce add them; a blob counted under another predicate is refused. */
  TGX_CHECK_ROW_PREDICATE = 20,
  /* The type classes of one STRING column: every non-NULL value is read once and put into exactly one of seven classes
   * -- the device side of the reference's DataTypeAnalyzer (TG/analyzers/advanced/data_type.rs:129-150), one
   *     SELECT CASE WHEN <boolean> .. WHEN <integer> .. WHEN <double> .. WHEN <date> .. WHEN <timestamp> .. ELSE 'string'
   *            END, COUNT(*) FROM t WHERE c IS NOT NULL GROUP BY 1
   * One column (`column`; `column2` must be -1; no column list), no parameters.  Specs on the same column share one
   * task and one walk.  Read with tgx_type_classes_get (below, which holds the classes' exact grammar); tgx_result
   * carries total = rows seen and non_null.  Utf8, LargeUtf8, Utf8View and Dictionary<Int32, Utf8> columns are taken (a
   * NULL dictionary entry and an index outside the dictionary are NULL rows, as for VALUE_COUNTS); every other type is
   * TGX_UNSUPPORTED from tgx_update, before anything runs, and the state stays usable.  The state is nine additive
   * counters: tgx_merge, blobs (a section of its own, behind all others, only for plans with such specs) and
   * tgx_allreduce add them. */
  TGX_CHECK_TYPE_CLASSES = 21
} tgx_check_kind;

enum {
  TGX_FLAG_VARIANCE = 1u << 0,          /* NUMERIC_STATS: also sample variance / stddev */
  TGX_FLAG_MULTIPLICITY = 1u << 1,      /* DISTINCT: also #groups with cnt == 1 (NULL is a group) */
  TGX_FLAG_TRIM = 1u << 2,              /* REGEX: TRIM(col) (U+0020 only) before matching */
  TGX_FLAG_CASE_INSENSITIVE = 1u << 3,  /* REGEX: `~*` */
  TGX_FLAG_NULL_IS_VALID = 1u << 4,     /* REGEX: `OR col IS NULL` */
  /* SPEARMAN: exact sums instead of the reference's UInt64 arithmetic, whose rank products and sums wrap
   * modulo 2^64 (from about 3.8 M rows on) */
  TGX_FLAG_EXACT_RANK_SUMS = 1u << 5,
  /* DISTINCT over Utf8 / LargeUtf8 / Utf8View / Dictionary / tuple keys: an EXACT key set.  Without the flag such
   * keys are counted by their 128-bit KEYED fingerprints (tgx_plan_set_fingerprint_key): two distinct values count as
   * one only if all 128 bits agree under a key the data's producer does not know.  With it the state keeps the bytes of
   * every distinct key it has been fed (a device-side key store) and an equal fingerprint is confirmed by comparing
   * bytes -- `COUNT(DISTINCT c)` as DataFusion computes it (hash + equality, TG/constraints/uniqueness.rs:612-617,
   * 671-681, 709-715), for every input including one built against the fingerprint function.  What crosses a state
   * boundary (tgx_merge, state blobs, tgx_distinct_export / tgx_allreduce) travels as keyed fingerprints either way:
   * bytes never leave the device that was fed them.  One more place where keys go on as fingerprints: a first DEVICE
   * batch of 2 Mi rows or more is deduplicated in lists that refer to its rows (equal fingerprints are settled on the
   * rows' bytes); tgx_finalize hands the batch back to the caller, so a state that is FED AGAIN after tgx_finalize holds
   * that batch's keys by fingerprint from then on -- tgx_state_sync (instead of, or before, tgx_finalize) moves them
   * into the table with their bytes.  Numeric keys are exact regardless of the flag. */
  TGX_FLAG_EXACT_KEYS = 1u << 6
};

typedef struct tgx_check_spec {
  int32_t kind;         /* tgx_check_kind */
  int32_t column;       /* index into the columns array handed to tgx_update */
  int32_t column2;      /* COMOMENTS / SPEARMAN / JOINT_BINS / TEMPORAL (order mode): second column; otherwise -1 */
  uint32_t flags;
  const char *pattern;  /* REGEX: pattern bytes (Rust `regex` syntax), not NUL-terminated */
  uint64_t pattern_len;
  uint32_t kll_k;       /* KLL: k >= 2 */
  uint32_t reserved;
  /* DISTINCT over a tuple of 2..8 columns -- COUNT(DISTINCT (a, b)), GROUP BY a, b
   * (TG/constraints/uniqueness.rs:557-562, 687-699, 709-715): `columns` lists them (then `column` is ignored).
   * A tuple is a value of its own: NULL components take part like any other value (SQL struct / GROUP BY
   * semantics), Float64 components compare by bit pattern, a string component is the row's string whatever the
   * layout (Utf8 / LargeUtf8 / Utf8View / Dictionary<Int32, Utf8>: a NULL dictionary entry is a NULL component).
   * Result: total = rows, non_null = rows whose every
   * component is non-NULL (the primary-key NULL check), distinct = tuples, groups_once with MULTIPLICITY.
   * n_columns == 0 or 1: the single-column check on `column`.
   * KEY_PROBE over a tuple of 2..8 columns: the spec's key is the tuple (tgx_plan_set_key_probe_tuples).  More than 8
   * columns or a NULL list is refused by tgx_plan_create.
   * ROW_PREDICATE: the 1 .. 8 columns its leaves name by position in this list (a list of length 1 too).
   * Every other kind refuses a column list. */
  const int32_t *columns;
  uint32_t n_columns;
  uint32_t reserved2;
  uint64_t length_min;  /* LENGTH: inclusive bounds in characters; length_max = UINT64_MAX: no upper bound */
  uint64_t length_max;
} tgx_check_spec;

/* One result per spec.  Fields outside the spec's kind are zero. */
typedef struct tgx_result {
  int32_t kind;
  int32_t is_float;     /* NUMERIC_STATS: column type */
  int64_t total;        /* COUNT(*)  (rows seen) */
  int64_t non_null;     /* COUNT(col); COMOMENTS: rows with both sides non-NULL */
  /* NUMERIC_STATS */
  int32_t has_value;    /* 0 => MIN/MAX/SUM/AVG are SQL NULL (no non-NULL rows) */
  int32_t has_variance; /* 0 => STDDEV/VARIANCE are SQL NULL (fewer than 2 rows) */
  int64_t min_i, max_i; /* Int64 columns */
  double min_f, max_f;  /* Float64 columns: IEEE totalOrder; Int64 columns: the same as double */
  int64_t sum_i;        /* SUM(Int64), wrapping */
  double sum_f;         /* SUM(Float64) / SUM(CAST(Int64 AS DOUBLE)) */
  double mean;          /* AVG */
  double var_samp, stddev_samp;
  /* DISTINCT */
  int64_t distinct;     /* COUNT(DISTINCT col) */
  int64_t groups_once;  /* SUM(CASE WHEN cnt = 1 ...) over GROUP BY col; only with TGX_FLAG_MULTIPLICITY, else 0 */
  /* REGEX_MATCH */
  int64_t matches;
  /* COMOMENTS */
  double sum_x, sum_y, sum_x2, sum_y2, sum_xy;
  /* KLL: read through tgx_kll_* below */
  uint64_t kll_n;
  /* COMOMENTS, centred: means, M2x = SUM((x - mean_x)^2), M2y, Cxy = SUM((x - mean_x)(y - mean_y)) over the rows
   * with both sides non-NULL.  CORR(x, y) = Cxy / sqrt(M2x M2y) (0 when either M2 is 0), COVAR_SAMP = Cxy / (n - 1),
   * COVAR_POP = Cxy / n -- what DataFusion's online accumulators arrive at (TG/constraints/correlation.rs:260-275).
   * The library sums about a pivot near the data, so these hold their precision on offset columns (timestamps,
   * ids around 1e9) where n * sum_xy - sum_x * sum_y has cancelled; sum_x .. sum_xy above are the raw sums of
   * TG/analyzers/advanced/correlation.rs:239-249 and carry that analyzer's own cancellation. */
  double co_mean_x, co_mean_y, co_m2_x, co_m2_y, co_c_xy;
} tgx_result;

enum {
  /* every batch is launched as it arrives: no library-side coalescing of small batches (see tgx_update) */
  TGX_OPT_NO_COALESCE = 1u << 0
};

typedef struct tgx_options {
  int32_t device_id;       /* -1 = current HIP device */
  uint32_t flags;          /* TGX_OPT_* */
  uint64_t distinct_capacity_hint; /* expected rows per DISTINCT column (0 = grow on demand) */
} tgx_options;

typedef struct tgx_plan tgx_plan;
typedef struct tgx_state tgx_state;

/* ---- lifecycle ------------------------------------------------------------------------------ */
uint32_t tgx_abi_version(void);
/* Selects the device and checks it is gfx950.  No reference counterpart (the reference has no
 * device); called once per process before any other compute entry point. */
tgx_status tgx_init(const tgx_options *opts, tgx_error *err);
tgx_status tgx_shutdown(void);
const char *tgx_status_name(int32_t status);

/* Device memory between runs.  `ValidationSuite::run` (TG/core/suite.rs:399) is called once per table: a state is
 * created, fed, read and dropped.  The device (and pinned host) blocks of a destroyed state are kept by the library, by
 * size class, and handed to the next state -- from the second state of a process on, tgx_state_create .. tgx_finalize
 * performs no hipMalloc (a GB-sized hipMalloc costs milliseconds, hipFree waits for the whole device).  Bounded by
 * TGX_DEVICE_CACHE_MAX_BYTES (default: a quarter of the device's memory, at most 64 GiB); TGX_DEVICE_CACHE=0 turns it
 * off.  tgx_trim() returns everything cached to the driver (tgx_shutdown does too); no reference counterpart. */
typedef struct tgx_cache_stats {
  uint64_t device_cached_bytes;  /* held by the cache right now (not by live states) */
  uint64_t device_cached_blocks;
  uint64_t device_hits;          /* allocations served from the cache since the process started */
  uint64_t device_misses;        /* allocations that went to hipMalloc */
  uint64_t pinned_cached_bytes;
  uint64_t pinned_hits;
  uint64_t pinned_misses;
} tgx_cache_stats;
tgx_status tgx_trim(void);
tgx_status tgx_cache_stats_get(tgx_cache_stats *out);

/* Plan = the fused set of aggregates a ValidationSuite needs, grouped so each column buffer is
 * read once.  Replaces the per-constraint `format!("SELECT ...")` + `ctx.sql()` planning in
 * TG/core/suite.rs:67-100 (one scan per constraint). Regex patterns are validated
 * (TG/security.rs:152-183) and compiled here. */
tgx_status tgx_plan_create(const tgx_check_spec *specs, size_t n_specs, tgx_plan **out,
                           tgx_error *err);
void tgx_plan_destroy(tgx_plan *plan);
size_t tgx_plan_num_specs(const tgx_plan *plan);
/* The 128-bit key of the plan's string / tuple fingerprints (kernels/distinct128.hip: Chaskey-8).  tgx_plan_create
 * draws one from the operating system (getrandom); TGX_FINGERPRINT_KEY=<32 hex digits> fixes it for a process.
 * States, blobs and ranks can only be united when their fingerprints were made under ONE key: a plan that is to read
 * another process's blobs (tgx_state_deserialize says which key a blob carries in its error message and through
 * tgx_blob_fingerprint_key) or to take part in tgx_allreduce (every rank: the ranks compare keys in the facts round,
 * a mismatch is TGX_INVALID_ARGUMENT) is given the shared key here, BEFORE its first tgx_state_create -- afterwards
 * the call is refused.  No reference counterpart (DataFusion's hash sets keep the values themselves). */
tgx_status tgx_plan_set_fingerprint_key(tgx_plan *plan, const uint8_t key[16], tgx_error *err);
tgx_status tgx_plan_get_fingerprint_key(const tgx_plan *plan, uint8_t key_out[16]);

/* TGX_CHECK_JOINT_BINS: the binning of spec `spec_index`, which puts the spec into its COUNT phase.  Like the
 * fingerprint key it can be set until the plan's first state exists; afterwards (and for a spec of another kind) the
 * call is refused with TGX_INVALID_ARGUMENT.  `bins` runs from 2 to TGX_JOINT_MAX_BINS: the (bins + 1)^2 cells are
 * counted in a workgroup's LDS with 32-bit counters (128^2 x 4 B = 64 KiB); more bins are TGX_UNSUPPORTED (there is no
 * global-memory path).  Origins must be finite and widths finite and positive: a range whose difference MAX - MIN
 * overflows to infinity has no bin width and is an error (TGX_INVALID_ARGUMENT) here.  The reference's values are
 * origin = MIN, width = (MAX - MIN) > 0 ? (MAX - MIN) / bins : 1.0 (mutual_information.rs:219-233). */
#define TGX_JOINT_MAX_BINS 127
typedef struct tgx_joint_binning {
  double x_origin, x_width, y_origin, y_width;
  uint32_t bins;
  uint32_t reserved;
} tgx_joint_binning;
tgx_status tgx_plan_set_joint_binning(tgx_plan *plan, size_t spec_index, const tgx_joint_binning *binning,
                                      tgx_error *err);

/* TGX_CHECK_TEMPORAL: the mode and parameters of spec `spec_index`.  Like the fingerprint key they can be set until the
 * plan's first state exists; afterwards, and for a spec of another kind, the call is refused with
 * TGX_INVALID_ARGUMENT.
 *   TGX_TEMPORAL_ORDER        the row passes iff after - before >= delta, the difference taken without wrap-around
 *                             (INT64_MAX - INT64_MIN is a large positive number, not -1).  The reference's four comparisons
 *                             (temporal_ordering.rs:352-368) are delta = tolerance for >= and tolerance + 1 for >.
 *   TGX_TEMPORAL_TIME_OF_DAY  the row passes iff tod_lo <= floormod(t, 86400 * ticks_per_second) <= tod_hi (floor forms:
 *                             timestamps before 1970 are negative).  ticks_per_second is 1, 10^3, 10^6 or 10^9.
 *   TGX_TEMPORAL_RANGE        the row passes iff lo <= t <= hi; INT64_MIN / INT64_MAX mean "no bound".
 * Flags:
 *   TGX_TEMPORAL_KEEP_NULLS     the reference's allow_nulls(true): the IS NOT NULL terms leave the WHERE clause.  A NULL row
 *                               (either side, in order mode) is then CONSIDERED, its predicate is SQL NULL, it lands in the
 *                               ELSE 1 branch: a violation.  Without the flag a NULL row is seen and not considered.
 *   TGX_TEMPORAL_WEEKDAYS_ONLY  time-of-day mode only: the WHERE term EXTRACT(DOW FROM t) BETWEEN 1 AND 5, with
 *                               dow = floormod(floordiv(t, ticks per day) + 4, 7) (1970-01-01 is a Thursday, DOW 0 is
 *                               Sunday).  It takes rows out of `considered`; it does not make them violations.  A NULL
 *                               row never passes this filter, with or without KEEP_NULLS. */
enum { TGX_TEMPORAL_ORDER = 1, TGX_TEMPORAL_TIME_OF_DAY = 2, TGX_TEMPORAL_RANGE = 3 };
enum { TGX_TEMPORAL_KEEP_NULLS = 1u << 0, TGX_TEMPORAL_WEEKDAYS_ONLY = 1u << 1 };
typedef struct tgx_temporal_params {
  int32_t mode;             /* TGX_TEMPORAL_ORDER / _TIME_OF_DAY / _RANGE */
  uint32_t flags;           /* TGX_TEMPORAL_KEEP_NULLS | TGX_TEMPORAL_WEEKDAYS_ONLY */
  int64_t delta;            /* ORDER */
  int64_t ticks_per_second; /* TIME_OF_DAY */
  int64_t tod_lo, tod_hi;   /* TIME_OF_DAY: ticks into the day, both ends inclusive */
  int64_t lo, hi;           /* RANGE: both ends inclusive */
} tgx_temporal_params;
tgx_status tgx_plan_set_temporal(tgx_plan *plan, size_t spec_index, const tgx_temporal_params *params, tgx_error *err);

/* TGX_CHECK_TIME_GAP: the threshold of spec `spec_index`, in the timestamp column's ticks.  Like the TEMPORAL parameters
 * it can be set until the plan's first state exists; afterwards, and for a spec of another kind, the call is refused
 * with TGX_INVALID_ARGUMENT.  `flags` must be 0. */
typedef struct tgx_time_gap_params {
  int64_t max_gap; /* a gap is a violation iff gap > max_gap (negative: every gap is one) */
  uint32_t flags;  /* 0 */
} tgx_time_gap_params;
tgx_status tgx_plan_set_time_gap(tgx_plan *plan, size_t spec_index, const tgx_time_gap_params *params, tgx_error *err);

/* TGX_CHECK_VALUE_RULE: the rule of spec `spec_index`.  Like the TEMPORAL parameters it can be set until the plan's
 * first state exists; afterwards, and for a spec of another kind, the call is refused with TGX_INVALID_ARGUMENT.
 *
 * A row's value is an int64 when the column's Arrow type is an integer type (Int8 .. Int64, UInt8 .. UInt32, Date32,
 * Date64, Timestamp, Duration) and a double when it is Float32 or Float64; widening preserves both (a Float32 NaN keeps
 * its sign and payload).  A NULL row is seen and never considered.
 *
 * The semantics are DataFusion 50 / arrow 56 as the reference's query reaches them.  arrow-ord's comparison kernels
 * order floats by IEEE totalOrder, for `=` as well:
 *     -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN
 * so every float comparison below is a comparison of totalOrder keys, key(x) = b ^ ((b >> 63) & 0x7fffffffffffffff)
 * over the bits b of x taken as an int64 (arithmetic shift) -- not `<` / `==` on doubles.  (This rests on arrow-ord's
 * documented behaviour: the reference cannot be built beside this library.  INTEGRATION.md lists it as unverified.)
 *
 *   TGX_RULE_GE_ZERO   col >= 0.  Integer column: v >= 0.  Float column: key(x) >= key(+0.0).
 *   TGX_RULE_GT_ZERO   col > 0.   Integer column: v > 0.   Float column: key(x) > key(+0.0).
 *                      So -0.0 fails both, +0.0 passes GE_ZERO and fails GT_ZERO, +NaN passes both, -NaN fails both.
 *   TGX_RULE_BETWEEN   col BETWEEN lo AND hi, the three operands coerced to one type.  Integer column without
 *                      TGX_RULE_BOUNDS_AS_DOUBLE: lo_i <= v <= hi_i as int64.  With the flag, or on a float column
 *                      (where the flag changes nothing): key(lo_f) <= key((double)v) <= key(hi_f), an int64 converted
 *                      round-to-nearest-even as CAST(col AS DOUBLE) does.  lo > hi is allowed and matches nothing.
 *                      lo_i / hi_i are read only without the flag on an integer column, lo_f / hi_f only otherwise.
 *   TGX_RULE_INTEGER   col = CAST(col AS INT), INT being Int32.  SQL CAST is not TRY_CAST: a value that does not fit
 *                      fails the whole query, so such rows are COUNTED as cast_errors (never raised; the caller turns
 *                      cast_errors > 0 into its error).  A row is a cast error when it is an integer value outside
 *                      [-2^31, 2^31 - 1], a float that is NaN or +-inf, or a float whose truncation toward zero lies
 *                      outside that range (num-traits' rule: -2147483648.9 is in range, 2147483648.0 is not).  A row
 *                      that casts is valid iff v == (int32)v for integers (always), and
 *                      key(x) == key((double)(int32)trunc(x)) for floats: 2.0 is valid, 2.5 is not, and -0.0 is not
 *                      (its cast gives +0.0).  A cast error is considered and not valid.
 * Flags: TGX_RULE_BOUNDS_AS_DOUBLE, BETWEEN only (TGX_INVALID_ARGUMENT with another mode). */
enum { TGX_RULE_GE_ZERO = 1, TGX_RULE_GT_ZERO = 2, TGX_RULE_BETWEEN = 3, TGX_RULE_INTEGER = 4 };
enum { TGX_RULE_BOUNDS_AS_DOUBLE = 1u << 0 };
typedef struct tgx_value_rule_params {
  int32_t mode;       /* TGX_RULE_* */
  uint32_t flags;     /* TGX_RULE_BOUNDS_AS_DOUBLE */
  int64_t lo_i, hi_i; /* BETWEEN, int64 domain: both ends inclusive */
  double lo_f, hi_f;  /* BETWEEN, double domain: both ends inclusive, by totalOrder (a NaN bound is a key like any other) */
} tgx_value_rule_params;
tgx_status tgx_plan_set_value_rule(tgx_plan *plan, size_t spec_index, const tgx_value_rule_params *params,
                                   tgx_error *err);

/* TGX_CHECK_ROW_PREDICATE: the predicate of spec `spec_index`.  Like the VALUE_RULE parameters it can be set until the
 * plan's first state exists; afterwards, and for a spec of another kind, the call is refused with TGX_INVALID_ARGUMENT.
 * This is a closed predicate subset, not SQL: what is written here is all there is, and it is what the exact reference
 * of the tests is held to.
 *
 * LEAVES (1 .. TGX_PRED_MAX_LEAVES).  Each leaf is TRUE, FALSE or UNKNOWN for a row.  `col` / `col2` are positions in the
 * spec's column list.  A row's value is an int64 or a double as for VALUE_RULE (above); a string column's value is the
 * row's bytes whatever the layout (Utf8, LargeUtf8, Utf8View, Dictionary<Int32, Utf8>), and a row whose dictionary
 * entry is NULL, or whose index lies outside the dictionary, is a NULL row (the rule of VALUE_COUNTS).
 *   TGX_PRED_IS_NULL      col IS NULL: TRUE on a NULL row, FALSE otherwise; never UNKNOWN.  Takes every column type.
 *   TGX_PRED_CMP_LITERAL  col <op> literal, op one of TGX_PRED_EQ / LT / LE / GT / GE.  UNKNOWN when col is NULL.  The
 *                         literal is carried as int64 (lit_i) and as double (lit_f); TGX_PRED_LITERAL_IS_DOUBLE says it was
 *                         written with a point or an exponent.  What is compared follows the column's type in the batch:
 *                           integer column, integer literal:   v <op> lit_i as int64;
 *                           integer column, double literal:    key((double)v) <op> key(lit_f), the conversion
 *                                                              round-to-nearest-even as CAST(col AS DOUBLE) does;
 *                           float column:                      key(x) <op> key(lit_f) (the caller gives an integer
 *                                                              literal's lit_f = (double)lit_i).
 *                         key is the IEEE totalOrder key of VALUE_RULE (above), for `=` as well: -0.0 < +0.0 and a NaN
 *                         equals the NaN with the same bits.  (This rests on arrow-ord's documented ordering, as for
 *                         VALUE_RULE; INTEGRATION.md lists it as unverified.)
 *   TGX_PRED_CMP_COLUMNS  col <op> col2.  UNKNOWN when either side is NULL.  Both integer: int64 compare.  Any float:
 *                         both sides as double keys (an integer side converted as above).  Two string columns:
 *                         TGX_PRED_EQ only, by bytes.
 *   TGX_PRED_STR_EQ       col = the literal bytes [lit_offset, lit_offset + lit_len) of the pool, by bytes; the empty
 *                         string is a value.  UNKNOWN when col is NULL.
 * Four more kinds read a string value's bytes; each is UNKNOWN when col is NULL.  KIND 5 IS UNASSIGNED and stays an
 * unknown leaf kind.  A byte of the form 10xxxxxx is called a continuation byte below; nothing asks the value or the
 * literal to be UTF-8.
 *   TGX_PRED_STR_CMP      col <op> the literal bytes, op one of TGX_PRED_LT / LE / GT / GE (TGX_PRED_EQ is refused: use
 *                         STR_EQ, so that a predicate has one spelling).  Bytewise lexicographic: the first differing
 *                         byte decides, as unsigned; a proper prefix is smaller.  (What arrow-ord does on Utf8.)
 *   TGX_PRED_STR_LENGTH   len(col) <op> lit_i as int64, any of the five ops.  len is the number of bytes that are no
 *                         continuation bytes -- on valid UTF-8 the code points, DataFusion's LENGTH = character_length
 *                         -- or, under the flag TGX_PRED_LENGTH_IN_BYTES, the number of bytes (OCTET_LENGTH).
 *   TGX_PRED_STR_LIKE     col LIKE the pattern bytes [lit_offset, lit_offset + lit_len) of the pool.  `%` matches any
 *                         run of bytes, the empty one included.  `_` matches exactly one unit: one byte that is no
 *                         continuation byte plus all continuation bytes directly after it; at offset 0 the first byte
 *                         opens a unit whatever it is.  Every other byte matches itself.  The match is anchored at both
 *                         ends and case-sensitive; `_` and `%` match a line feed.  The empty pattern matches the empty
 *                         string only.  There is no escape: a pattern that holds the byte 0x5C is refused.
 *   TGX_PRED_STR_BLANK    TRUE iff every byte of the value is 0x20, the empty string included: TRIM(col) = ''.
 * A leaf that does not fit the type its column arrives in -- a string leaf on a numeric column, a numeric leaf on a
 * string column, a string column against a numeric one, UInt64 / Boolean / validity-only columns under anything but
 * IS_NULL -- makes tgx_update fail with TGX_UNSUPPORTED; the batch is not counted and the state stays usable.
 *
 * PROGRAM (1 .. TGX_PRED_MAX_OPS ops, postfix).  An op is `code | arg << 8`: TGX_PRED_PUSH (arg: the leaf), TGX_PRED_AND,
 * TGX_PRED_OR, TGX_PRED_NOT (arg 0).  The logic is Kleene's: AND is FALSE if either side is FALSE, else UNKNOWN if either
 * is UNKNOWN, else TRUE; OR is the dual; NOT UNKNOWN is UNKNOWN.  The program must leave exactly one value, never pop
 * an empty stack and never hold more than TGX_PRED_MAX_DEPTH values.  `<>`, BETWEEN and IN are not device notions: the
 * caller lowers them by SQL's own definitions (NOT(x = l); x >= a AND x <= b; an OR of equalities).
 *
 * The setter refuses with TGX_INVALID_ARGUMENT: counts out of range, an unknown leaf kind / comparison / flag / op, a
 * column position outside the spec's list, a literal range outside the pool, a PUSH of a leaf that does not exist,
 * underflow, a depth above 32, and a program that leaves more or fewer than one value; of the kinds 6 .. 9 also a
 * comparison outside the kind's ops (STR_CMP: LT .. GE; STR_LENGTH: EQ .. GE), a flag other than
 * TGX_PRED_LENGTH_IN_BYTES on STR_LENGTH and any flag on the other three, and a 0x5C in a LIKE pattern.  What a leaf
 * does not read is kept as zero bits (the blob compares the predicate byte by byte). */
enum { TGX_PRED_MAX_COLUMNS = 8, TGX_PRED_MAX_LEAVES = 32, TGX_PRED_MAX_OPS = 64, TGX_PRED_MAX_DEPTH = 32,
       TGX_PRED_MAX_LITERAL_BYTES = 256 };
enum { TGX_PRED_IS_NULL = 1, TGX_PRED_CMP_LITERAL = 2, TGX_PRED_CMP_COLUMNS = 3, TGX_PRED_STR_EQ = 4,
       /* 5: unassigned */
       TGX_PRED_STR_CMP = 6, TGX_PRED_STR_LENGTH = 7, TGX_PRED_STR_LIKE = 8, TGX_PRED_STR_BLANK = 9 };
enum { TGX_PRED_EQ = 1, TGX_PRED_LT = 2, TGX_PRED_LE = 3, TGX_PRED_GT = 4, TGX_PRED_GE = 5 };
enum { TGX_PRED_LITERAL_IS_DOUBLE = 1u << 0, TGX_PRED_LENGTH_IN_BYTES = 1u << 1 };
enum { TGX_PRED_PUSH = 1, TGX_PRED_AND = 2, TGX_PRED_OR = 3, TGX_PRED_NOT = 4 };
typedef struct tgx_row_predicate_leaf {
  int32_t kind;        /* TGX_PRED_IS_NULL .. TGX_PRED_STR_BLANK */
  int32_t op;          /* CMP_LITERAL / CMP_COLUMNS / STR_CMP / STR_LENGTH: TGX_PRED_EQ .. TGX_PRED_GE; otherwise 0 */
  int32_t col, col2;   /* positions in the spec's column list; col2: CMP_COLUMNS only, otherwise 0 */
  uint32_t flags;      /* CMP_LITERAL: TGX_PRED_LITERAL_IS_DOUBLE; STR_LENGTH: TGX_PRED_LENGTH_IN_BYTES */
  uint32_t lit_offset; /* STR_EQ / STR_CMP / STR_LIKE: the literal's bytes in the pool */
  uint32_t lit_len;
  uint32_t reserved;   /* 0 */
  int64_t lit_i;       /* CMP_LITERAL; STR_LENGTH: the length compared with */
  double lit_f;
} tgx_row_predicate_leaf;
typedef struct tgx_row_predicate_params {
  uint32_t n_leaves, n_ops, n_literal_bytes, reserved;
  tgx_row_predicate_leaf leaves[TGX_PRED_MAX_LEAVES];
  uint16_t program[TGX_PRED_MAX_OPS];
  uint8_t literals[TGX_PRED_MAX_LITERAL_BYTES];
} tgx_row_predicate_params;
tgx_status tgx_plan_set_row_predicate(tgx_plan *plan, size_t spec_index, const tgx_row_predicate_params *params,
                                      tgx_error *err);

/* TGX_CHECK_VALUE_COUNTS: the bounds of spec `spec_index`.  Like the VALUE_RULE parameters they can be set until the
 * plan's first state exists; afterwards, and for a spec of another kind, the call is refused with TGX_INVALID_ARGUMENT.
 * max_distinct (1 .. TGX_VALUE_COUNTS_MAX_DISTINCT) sizes the task's table on the device: a power of two of at least
 * 2 * max_distinct slots, so a column with up to max_distinct values is counted without overflow; a column with more may
 * still fit (the caller compares `distinct` with its bound) or leave rows in overflow_rows.  max_value_bytes
 * (1 .. TGX_VALUE_COUNTS_MAX_VALUE_BYTES) is read for string columns only: longer rows are counted in long_rows. */
enum { TGX_VALUE_COUNTS_MAX_DISTINCT = 65536, TGX_VALUE_COUNTS_MAX_VALUE_BYTES = 256 };
typedef struct tgx_value_counts_params {
  uint32_t max_distinct;
  uint32_t max_value_bytes;
} tgx_value_counts_params;
tgx_status tgx_plan_set_value_counts(tgx_plan *plan, size_t spec_index, const tgx_value_counts_params *params,
                                     tgx_error *err);

/* TGX_CHECK_PAIR_COUNTS: the bounds of spec `spec_index` and what a cell is on either side.  Like the VALUE_COUNTS
 * parameters they can be set until the plan's first state exists; afterwards, and for a spec of another kind, the call is
 * refused with TGX_INVALID_ARGUMENT.  max_pairs (1 .. TGX_PAIR_COUNTS_MAX_PAIRS) sizes the task's table on the device: a
 * power of two of at least 2 * max_pairs slots, probed as VALUE_COUNTS's is; max_value_bytes
 * (1 .. TGX_PAIR_COUNTS_MAX_VALUE_BYTES) holds per string side.  A TGX_PAIR_SIDE_BINNED side gives origin (finite),
 * width (finite, positive) and bins (2 .. TGX_JOINT_MAX_BINS); the other modes leave the three zero.  Two numeric sides
 * (any two of BINNED and RANGE) are refused with TGX_INVALID_ARGUMENT: joint bins of two numeric columns are
 * TGX_CHECK_JOINT_BINS.  The reference's values are origin = MIN, width = (MAX - MIN) > 0 ? (MAX - MIN) / bins : 1.0
 * (mutual_information.rs:219-233), with MIN / MAX from a first pass in the RANGE mode. */
enum { TGX_PAIR_SIDE_VALUE = 0, TGX_PAIR_SIDE_RANGE = 1, TGX_PAIR_SIDE_BINNED = 2 };
enum { TGX_PAIR_COUNTS_MAX_PAIRS = 65536, TGX_PAIR_COUNTS_MAX_VALUE_BYTES = 256 };
typedef struct tgx_pair_side {
  int32_t mode;  /* TGX_PAIR_SIDE_* */
  uint32_t bins; /* BINNED */
  double origin, width; /* BINNED */
} tgx_pair_side;
typedef struct tgx_pair_counts_params {
  uint32_t max_pairs;
  uint32_t max_value_bytes;
  tgx_pair_side x, y;
} tgx_pair_counts_params;
tgx_status tgx_plan_set_pair_counts(tgx_plan *plan, size_t spec_index, const tgx_pair_counts_params *params,
                                    tgx_error *err);

/* TGX_CHECK_GROUP_COUNTS: the bounds of spec `spec_index`.  Lifetime and refusals are those of
 * tgx_plan_set_value_counts.  max_groups (1 .. TGX_GROUP_COUNTS_MAX_GROUPS) sizes the walk's table on the device: a
 * power of two of at least 2 * max_groups slots, probed as VALUE_COUNTS's is; max_value_bytes
 * (1 .. TGX_GROUP_COUNTS_MAX_VALUE_BYTES) is read for string group columns only: rows with a longer key are counted in
 * long_rows / long_non_null. */
enum { TGX_GROUP_COUNTS_MAX_GROUPS = 65536, TGX_GROUP_COUNTS_MAX_VALUE_BYTES = 256 };
typedef struct tgx_group_counts_params {
  uint32_t max_groups;
  uint32_t max_value_bytes;
} tgx_group_counts_params;
tgx_status tgx_plan_set_group_counts(tgx_plan *plan, size_t spec_index, const tgx_group_counts_params *params,
                                     tgx_error *err);

/* TGX_CHECK_GROUP_SUMS: the bounds of spec `spec_index`, with the meaning, lifetime and refusals of
 * tgx_plan_set_group_counts. */
enum { TGX_GROUP_SUMS_MAX_GROUPS = 65536, TGX_GROUP_SUMS_MAX_VALUE_BYTES = 256 };
typedef struct tgx_group_sums_params {
  uint32_t max_groups;
  uint32_t max_value_bytes;
} tgx_group_sums_params;
tgx_status tgx_plan_set_group_sums(tgx_plan *plan, size_t spec_index, const tgx_group_sums_params *params,
                                   tgx_error *err);

/* TGX_CHECK_KEY_PROBE: the bound of spec `spec_index`.  Lifetime and refusals are those of tgx_plan_set_value_counts.
 * max_missing_keys (1 .. TGX_KEY_PROBE_MAX_MISSING_KEYS) sizes the task's table of missing keys on the device: a power
 * of two of at least 2 * max_missing_keys slots; `reserved` must be 0. */
enum { TGX_KEY_PROBE_MAX_MISSING_KEYS = 65536 };
typedef struct tgx_key_probe_params {
  uint32_t max_missing_keys;
  uint32_t reserved;
} tgx_key_probe_params;
tgx_status tgx_plan_set_key_probe(tgx_plan *plan, size_t spec_index, const tgx_key_probe_params *params, tgx_error *err);
/* The same bound, and the spec becomes COUNTED: its parent set keeps how often each key occurs in the parent (the
 * records' counts), and the state also sums the multiplicities of the matched rows' keys -- the matched PAIRS, COUNT(*)
 * of the inner join, which the reference's JoinCoverageConstraint asks for (TG/constraints/join_coverage.rs).  A spec
 * takes one of the two calls: the other one on the same spec afterwards is TGX_INVALID_ARGUMENT.  See
 * tgx_key_probe_pairs_get. */
tgx_status tgx_plan_set_key_probe_counted(tgx_plan *plan, size_t spec_index, const tgx_key_probe_params *params,
                                          tgx_error *err);
/* The spec GATHERS its column instead of probing it: every non-NULL key of every batch becomes a 16-byte {key, 1}
 * record in device memory, read with tgx_key_probe_rows_get -- the parent side of a counted probe when the parent's
 * keys repeat (a TGX_CHECK_DISTINCT export knows a key as seen once or more than once, not how often; duplicate
 * records of a counted set add up).  Such a spec takes no parent set and no other tgx_plan_set_key_probe* call; its
 * state costs 16 bytes a row it has seen, tgx_state_reset empties it, and a state that has gathered rows does not merge
 * or serialize (TGX_UNSUPPORTED).  tgx_key_probe_get gives seen, non_null and null_rows. */
tgx_status tgx_plan_set_key_probe_rows(tgx_plan *plan, size_t spec_index, tgx_error *err);
/* The spec probes STRING keys: its column is Utf8, LargeUtf8, Utf8View or Dictionary<Int32, Utf8>, and its parent set
 * holds the parent's values as keyed 128-bit fingerprints (tgx_key_probe_set_parent below).  max_missing_keys
 * (1 .. TGX_KEY_PROBE_MAX_MISSING_KEYS) sizes the table of missing keys as for a plain spec; a missing key keeps its
 * bytes when it has at most max_value_bytes (1 .. TGX_KEY_PROBE_MAX_VALUE_BYTES) of them, and is a long row otherwise.
 * Lifetime and refusals are those of tgx_plan_set_key_probe.  A spec takes exactly one of the six
 * tgx_plan_set_key_probe* calls: any second one on the same spec is TGX_INVALID_ARGUMENT.  An integer, float, UInt64 or
 * Boolean column on such a spec is TGX_UNSUPPORTED from tgx_update (the state stays usable), as a string column is on
 * every other KEY_PROBE spec. */
enum { TGX_KEY_PROBE_MAX_VALUE_BYTES = 256 };
typedef struct tgx_key_probe_strings_params {
  uint32_t max_missing_keys;
  uint32_t max_value_bytes;
} tgx_key_probe_strings_params;
tgx_status tgx_plan_set_key_probe_strings(tgx_plan *plan, size_t spec_index, const tgx_key_probe_strings_params *params,
                                          tgx_error *err);
/* The same, and the spec becomes a COUNTED strings spec: its parent set keeps how often each value occurs in the parent
 * (the records' counts) and the state sums the multiplicities of the matched rows' values -- JoinCoverageConstraint on
 * string keys.  Bounds, refusals and column types are those of tgx_plan_set_key_probe_strings.  See
 * tgx_key_probe_pairs_get and the COUNTED STRINGS paragraph beside tgx_key_probe_strings_get. */
tgx_status tgx_plan_set_key_probe_strings_counted(tgx_plan *plan, size_t spec_index,
                                                  const tgx_key_probe_strings_params *params, tgx_error *err);
/* The spec GATHERS its STRING column (Utf8, LargeUtf8, Utf8View or Dictionary<Int32, Utf8>) instead of probing it, as
 * 32-byte {uint64 hash_a, uint64 hash_b, uint64 count, uint64 0} records in device memory: the values' fingerprints
 * under the plan's key, in the record format of a string column's TGX_CHECK_DISTINCT export -- the parent side of a
 * counted strings probe.  A plain string layout gives one {hash_a, hash_b, 1, 0} record per non-NULL row.  A dictionary
 * column gives, per batch, one {hash_a, hash_b, n, 0} record for each entry that n > 0 rows of the batch refer to; rows
 * of NULL entries and of indices outside the dictionary are NULL rows, as in the strings probe.  Lifetime, reset and
 * the refusals of a parent set, of any other tgx_plan_set_key_probe* call, of merge and of serialize are those of
 * tgx_plan_set_key_probe_rows.  The state costs 32 bytes a row it has seen (the room it keeps; a dictionary column's
 * records come to 32 bytes per live entry per batch).  Read with tgx_key_probe_rows_get. */
tgx_status tgx_plan_set_key_probe_rows_strings(tgx_plan *plan, size_t spec_index, tgx_error *err);
/* The three calls of a spec with a COLUMN LIST (tgx_check_spec::columns, 2 .. 8 columns): its key is the TUPLE of the
 * row's components.  _tuples: a plain probe against a set of route 5; _tuples_counted: a counted probe against a set of
 * route 6 (tgx_key_probe_pairs_get works on it under its bound); _rows_tuples: the spec gathers its tuples as 32-byte
 * {hash_a, hash_b, 1, 0} records (tgx_key_probe_rows_get), one per row whose every component is non-NULL, 32 bytes a
 * gathered row; such a state does not merge or serialize.  max_missing_keys bounds each of the two classes of entries
 * (below).  A spec takes exactly one of the nine tgx_plan_set_key_probe* calls: any second one on the same spec is
 * TGX_INVALID_ARGUMENT, and so is one of these three on a spec without a column list and one of the other six on a spec
 * with one.  The rules of a row and the reads: tgx_key_probe_tuples_get. */
tgx_status tgx_plan_set_key_probe_tuples(tgx_plan *plan, size_t spec_index, const tgx_key_probe_params *params,
                                         tgx_error *err);
tgx_status tgx_plan_set_key_probe_tuples_counted(tgx_plan *plan, size_t spec_index, const tgx_key_probe_params *params,
                                                 tgx_error *err);
tgx_status tgx_plan_set_key_probe_rows_tuples(tgx_plan *plan, size_t spec_index, tgx_error *err);

/* TGX_CHECK_HISTOGRAM: the `buckets + 1` edges of spec `spec_index`, which puts the spec into its COUNT phase.  Like a
 * JOINT_BINS binning they can be set until the plan's first state exists; afterwards (and for a spec of another kind)
 * the call is refused with TGX_INVALID_ARGUMENT.  1 <= buckets <= TGX_HISTOGRAM_MAX_BUCKETS; every edge must be finite
 * and edges[0 .. buckets-1] non-decreasing (TGX_INVALID_ARGUMENT otherwise).  edges[buckets] MAY lie below
 * edges[buckets-1]: the reference's own formula produces that on a range a few ulps wide, where max + width * 0.001
 * rounds to max while min + (buckets-1) * width has rounded up.  The reference's values are
 * width = (MAX - MIN) > 0 && buckets > 1 ? (MAX - MIN) / buckets : 1.0, edges[i] = MIN + i * width for i < buckets and
 * edges[buckets] = MAX + width * 0.001 (histogram.rs:253-275). */
#define TGX_HISTOGRAM_MAX_BUCKETS 1000
tgx_status tgx_plan_set_histogram_edges(tgx_plan *plan, size_t spec_index, const double *edges, uint32_t buckets,
                                        tgx_error *err);

/* State = `Analyzer::State` for every spec of the plan (TG/analyzers/traits.rs:154-179).
 * `hip_stream` is a hipStream_t (NULL = a stream the library creates).  Everything the state does on the device is
 * queued on that stream and nowhere else: a DEVICE buffer handed to tgx_update has to be COMPLETE as far as that
 * stream is concerned -- written by work on the same stream, or by work the caller has waited for (an event the stream
 * waits on, or a synchronisation); the library's own stream does not wait for the legacy default stream. */
tgx_status tgx_state_create(const tgx_plan *plan, void *hip_stream, tgx_state **out, tgx_error *err);
void tgx_state_destroy(tgx_state *state);
/* How many of the batches handed to tgx_update so far are only NOTED (coalesced, not yet run): the LAST `*batches`
 * NON-EMPTY ones -- a batch of zero rows is never noted (tgx_update returns at once for it) and is not counted, so a
 * caller that keeps a window of retained batches must leave empty batches out of that window.
 * A caller that feeds TGX_MEM_HOST_RETAINED (or DEVICE) buffers of a long stream may release every batch before those
 * -- the library flushes by itself every few tens of MB -- instead of holding the whole table until tgx_finalize.
 * (DEVICE batches a sampled-range key set retains for a repair are the exception stated at tgx_update.)  Makes no
 * device call. */
tgx_status tgx_state_pending(const tgx_state *state, uint64_t *batches, uint64_t *rows);

/* One call per RecordBatch: replaces DataFusion's accumulator `update_batch` for the plan's
 * aggregates (`Analyzer::compute_state_from_data`, TG/analyzers/traits.rs:98-111).  `columns[i]` is
 * column i of the batch; unused columns may be zeroed.
 *
 * SMALL BATCHES ARE COALESCED.  DataFusion streams 8192-row RecordBatches (TG/core/context.rs:28-38): a batch of up to
 * 2^16 rows whose used columns are Int64 / Float64 / Int32 / Float32 (HOST or DEVICE) or HOST Utf8 / LargeUtf8 is only
 * NOTED by this call -- HOST windows are copied into a pinned arena first, so HOST buffers may still be released when
 * the call returns; DEVICE buffers must stay alive AND UNMODIFIED until the next tgx_finalize / tgx_state_sync (a noted
 * DEVICE window is read by a later flush, not by this call: a producer that recycles its device buffers in stream order
 * behind tgx_update -- fine for the kernels this call queues -- would have the flush read the next batch's bytes; such a
 * producer sets TGX_OPT_NO_COALESCE, or calls tgx_state_sync before it overwrites a buffer).  The pending
 * batches of every column are gathered into ONE contiguous device column and run as one batch when 4 Mi rows (or
 * 4096 batches, or a full arena) are pending, when a batch arrives that is not coalesced, and by every call that looks
 * at the state (tgx_finalize, tgx_state_sync, tgx_merge, tgx_state_serialize, tgx_allreduce, tgx_kll_*,
 * tgx_distinct_*).  Results do not depend on the batching: integers, key sets and pattern hits are those of the table;
 * float sums move in their last digits with the association, as they do between any two batchings.  Two arenas and two
 * sets of device regions take turns, so the host copies batch k+1 while the device works on flush k and nothing is
 * synchronised per batch: 8192-row batches of 8 columns run at 21 G rows/s from DEVICE buffers (0.4 us per call) and at
 * 0.70 G rows/s from HOST buffers (the copy into the arena, shared with three helper threads).  TGX_OPT_NO_COALESCE
 * turns it off.
 *
 * A batch that is NOT coalesced (more than 2^16 rows, Utf8View / dictionary columns, DEVICE strings) has its kernels
 * queued on the state's stream at once, and the call returns without waiting for them, except:
 *   - the FIRST batch (of 2^16 rows or more) an Int64 DISTINCT task sees waits for a sample of at most 2^16 of its
 *     values (that is: for whatever the stream still holds, plus ~20 us) to lay out the key set; later batches of
 *     the task never wait (keys outside the sampled range are counted and repaired at tgx_finalize /
 *     tgx_state_sync / tgx_state_serialize / tgx_merge / tgx_allreduce);
 *   - a hash key set that may have to grow reads its fill back first;
 *   (a Utf8 / LargeUtf8 / Utf8View DISTINCT task never waits: its first batch of 2^21 rows or more -- like that of
 *    a numeric task whose keys have no dense range -- is deduplicated in partitioned lists instead of the table, and
 *    should a list overflow -- heavily repeated values -- the batch is read once more at the next of the calls
 *    above: one more reason DEVICE buffers stay alive until then)
 *   - HOST batches: buffers copied straight from the caller's memory are borrowed only until the call returns, so
 *     it waits for the copies (small buffers travel through a pinned arena and do not). */
tgx_status tgx_update(const tgx_plan *plan, tgx_state *state, const tgx_column *columns,
                      size_t n_columns, tgx_error *err);

/* `AnalyzerState::merge` (TG/analyzers/traits.rs:160-170): folds srcs into dst.  Exact for every
 * kind, including DISTINCT (set union), unlike the reference's DistinctnessState::merge upper
 * bound (TG/analyzers/basic/distinctness.rs:77-92). */
tgx_status tgx_merge(const tgx_plan *plan, tgx_state *dst, tgx_state *const *srcs, size_t n_srcs,
                     tgx_error *err);

/* `Analyzer::compute_metric_from_state` inputs (TG/analyzers/traits.rs:113-122): waits for the
 * stream and writes one tgx_result per spec. Ratios, thresholds, assertions and messages stay
 * on the caller's side (TG/constraints/ *.rs). The state stays usable. */
tgx_status tgx_finalize(const tgx_plan *plan, tgx_state *state, tgx_result *results,
                        size_t n_results, tgx_error *err);
tgx_status tgx_state_sync(tgx_state *state, tgx_error *err);
tgx_status tgx_state_reset(const tgx_plan *plan, tgx_state *state, tgx_error *err);

/* Wire form of a state (the counterpart of the serde_json states the reference's
 * IncrementalAnalysisRunner stores, TG/analyzers/incremental/runner.rs:71-111); used to ship
 * partial states between ranks. `*len` receives the size needed/written. */
tgx_status tgx_state_serialize(const tgx_plan *plan, tgx_state *state, uint8_t *buf, size_t cap,
                               size_t *len, tgx_error *err);
tgx_status tgx_state_deserialize(const tgx_plan *plan, const uint8_t *buf, size_t len,
                                 tgx_state **out, tgx_error *err);
/* The fingerprint key a blob was made under (tgx_plan_set_fingerprint_key): `*keyed` = 0 when the blob holds no string /
 * tuple keys (then any plan of the same shape reads it), else 1 and `key_out` is the key.  tgx_state_deserialize refuses
 * a keyed blob under a plan with another key (TGX_INVALID_ARGUMENT). */
tgx_status tgx_blob_fingerprint_key(const uint8_t *buf, size_t len, uint8_t key_out[16], int32_t *keyed);

/* ---- KllSketch accessors (TG/analyzers/advanced/kll_sketch.rs:246-322, 368-399) ------------- */
tgx_status tgx_kll_quantile(const tgx_plan *plan, tgx_state *state, size_t spec_index, double phi,
                            double *out, tgx_error *err);
tgx_status tgx_kll_summary(const tgx_plan *plan, tgx_state *state, size_t spec_index, uint64_t *n,
                           double *min_value, double *max_value, uint64_t *num_levels,
                           uint64_t *num_retained, tgx_error *err);
/* copies level `level`'s items (weight 2^level each); *count receives the item count */
tgx_status tgx_kll_level_items(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                               uint64_t level, double *out, uint64_t cap, uint64_t *count,
                               tgx_error *err);
double tgx_kll_relative_error_bound(uint32_t k);

/* ---- joint bin counts (TGX_CHECK_JOINT_BINS; TG/analyzers/advanced/mutual_information.rs:143-248) --------------- */
typedef struct tgx_joint_range {
  uint64_t total;       /* rows seen */
  uint64_t n;           /* rows with both sides non-NULL and finite */
  uint64_t non_finite;  /* rows with both sides non-NULL and a NaN or an infinity on either side */
  double x_min, x_max, y_min, y_max; /* over the n rows; NaN when n == 0 */
} tgx_joint_range;
/* a spec in its range phase; a spec in its count phase answers total, n (the sum of its cells) and non_finite and
 * leaves the extremes NaN */
tgx_status tgx_joint_range_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_joint_range *out,
                               tgx_error *err);
/* a spec in its count phase: the (bins + 1)^2 cell counts, row-major (cell (i, j) at i * (bins + 1) + j), into the
 * caller's `cells` (`cap` entries; NULL / too small: only *n_cells is written and the call returns
 * TGX_INVALID_ARGUMENT when cells is non-NULL).  *out_of_range = rows whose index fell outside [0, bins] on either
 * side -- a table that changed between the two passes; they are in no cell. */
tgx_status tgx_joint_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index, uint64_t *cells, uint64_t cap,
                            uint64_t *n_cells, uint64_t *out_of_range, tgx_error *err);

/* ---- histogram of a numeric column (TGX_CHECK_HISTOGRAM; TG/analyzers/advanced/histogram.rs:184-330) ------------- */
typedef struct tgx_histogram_range {
  uint64_t total;       /* rows seen */
  uint64_t nulls;       /* NULL rows */
  uint64_t non_finite;  /* non-NULL rows holding a NaN or an infinity */
  uint64_t n;           /* non-NULL, finite rows */
  double min, max;      /* over the n rows; NaN when n == 0 */
  double sum, sum_squared; /* SUM(x), SUM(x * x) over the n rows as plain double sums; 0 when n == 0 */
} tgx_histogram_range;
/* a spec in its range phase; a spec in its count phase answers total, nulls, non_finite and n (the sum of its buckets)
 * and leaves the extremes and the sums NaN */
tgx_status tgx_histogram_range_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_histogram_range *out,
                                   tgx_error *err);
/* a spec in its count phase: its `buckets` counts into the caller's `counts` (`cap` entries; fewer than `buckets`:
 * TGX_INVALID_ARGUMENT).  *else_rows = the rows that reached the last bucket through ELSE rather than through its own
 * WHEN (below edges[0], or at or above edges[buckets]); they are part of counts[buckets-1].  *non_finite as above;
 * either may be NULL. */
tgx_status tgx_histogram_counts(const tgx_plan *plan, tgx_state *state, size_t spec_index, uint64_t *counts, size_t cap,
                                uint64_t *else_rows, uint64_t *non_finite, tgx_error *err);

/* ---- temporal row predicates (TGX_CHECK_TEMPORAL; TG/constraints/temporal_ordering.rs:346-453) -------------------- */
typedef struct tgx_temporal_counts {
  uint64_t seen;        /* rows handed to tgx_update */
  uint64_t considered;  /* the SQL's COUNT(*): rows the WHERE clause lets through */
  uint64_t violations;  /* the SQL's SUM(CASE WHEN <predicate> THEN 0 ELSE 1 END); 0 when nothing was considered */
} tgx_temporal_counts;
tgx_status tgx_temporal_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_temporal_counts *out,
                            tgx_error *err);

/* ---- time gaps between neighbouring timestamps (TGX_CHECK_TIME_GAP; TG/constraints/temporal_ordering.rs:454-481) -- */
typedef struct tgx_time_gap_counts {
  uint64_t seen;        /* rows handed to tgx_update */
  uint64_t rows;        /* of them, rows whose timestamp is not NULL */
  uint64_t gaps;        /* rows - non-empty partitions */
  uint64_t violations;  /* gaps above the spec's max_gap */
  uint64_t largest_gap; /* unsigned ticks; 0 when there is no gap */
} tgx_time_gap_counts;
/* Sorts the retained rows (the answer is kept until the next batch or reset: a second read does not sort again). */
tgx_status tgx_time_gap_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_time_gap_counts *out,
                            tgx_error *err);

/* ---- numeric value rules (TGX_CHECK_VALUE_RULE; TG/constraints/datatype.rs:383-439) ----------------------------- */
typedef struct tgx_value_rule_counts {
  uint64_t seen;        /* rows handed to tgx_update */
  uint64_t considered;  /* the SQL's COUNT(*): the non-NULL rows */
  uint64_t valid;       /* the SQL's SUM(CASE WHEN <predicate> THEN 1 ELSE 0 END): considered rows that pass */
  uint64_t cast_errors; /* INTEGER mode: considered rows on which CAST(col AS INT) fails the reference's query; else 0 */
} tgx_value_rule_counts;
tgx_status tgx_value_rule_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_value_rule_counts *out,
                              tgx_error *err);

/* ---- row predicates (TGX_CHECK_ROW_PREDICATE; TG/constraints/custom_sql.rs:192-282) -------------------------------- */
typedef struct tgx_row_predicate_counts {
  uint64_t seen;      /* rows handed to tgx_update: the SQL's COUNT(*) */
  uint64_t satisfied; /* rows on which the predicate is TRUE: the SQL's COUNT(CASE WHEN <expr> THEN 1 END) */
  uint64_t unknown;   /* rows on which it is UNKNOWN */
  uint64_t failed;    /* rows on which it is FALSE: seen - satisfied - unknown */
} tgx_row_predicate_counts;
tgx_status tgx_row_predicate_get(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                 tgx_row_predicate_counts *out, tgx_error *err);

/* ---- type classes (TGX_CHECK_TYPE_CLASSES; TG/analyzers/advanced/data_type.rs:129-150) ----------------------------- *
 * The classes are SYNTACTIC: defined on the value's bytes, closed, and tried in the order below -- the first that fits
 * wins.  D is an ASCII digit.  The letters of BOOLEAN, of the DOUBLE specials and the exponent's e are compared under
 * ASCII case folding only; the T and the Z of DATETIME are upper case.  No whitespace is trimmed.  A byte at or above
 * 0x80 fits no grammar.
 *   BOOLEAN    exactly 0 or 1, or true / false in any ASCII case.
 *   INTEGER    0 | -?[1-9]D*  with the value in [-2^31, 2^31 - 1]: the canonical text of an Int32 (so that
 *              CAST(TRY_CAST(c AS INT) AS VARCHAR) = c holds however lenient a parser is).  +5, 007, -0 and 2147483648
 *              are not INTEGER and go on to DOUBLE.
 *   DOUBLE     [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)?  or  [+-]?(nan|inf|infinity), of any length; no value is out of
 *              range (overflow is +-inf, not a failure).
 *   DATE       at most 10 bytes, DDDD-D{1,2}-D{1,2}, a valid day of the proleptic Gregorian calendar in the years
 *              0000 .. 9999 (year 0 is a leap year).
 *   DATETIME   more than 10 bytes: DDDD-DD-DD as a valid date; then T or one space; then hh:mm:ss with hh <= 23,
 *              mm <= 59, ss <= 59; optionally . and 1 .. 9 digits; optionally Z or [+-]hh:mm with hh <= 23, mm <= 59.
 *   UNDECIDED  none of the above, and the value begins DDDD- or [+-]D{4,}- : everything a date or timestamp parser
 *              could conceivably take in a form this contract does not spell out (single-digit fields in odd places, t,
 *              hh:mm without seconds, offsets without a colon, named zones, leap seconds, signed extended years, invalid
 *              calendar dates).  Reported, never guessed.
 *   STRING     everything else, the empty string included.
 * Identities:  seen == non_null + NULL rows;
 *              non_null == boolean_rows + integer_rows + double_rows + date_rows + datetime_rows + string_rows +
 *                          undecided_rows. */
enum {
  TGX_TYPE_CLASS_BOOLEAN = 0,
  TGX_TYPE_CLASS_INTEGER = 1,
  TGX_TYPE_CLASS_DOUBLE = 2,
  TGX_TYPE_CLASS_DATE = 3,
  TGX_TYPE_CLASS_DATETIME = 4,
  TGX_TYPE_CLASS_STRING = 5,
  TGX_TYPE_CLASS_UNDECIDED = 6
};
typedef struct tgx_type_classes_counts {
  uint64_t seen;     /* rows handed to tgx_update */
  uint64_t non_null; /* the SQL's WHERE c IS NOT NULL */
  uint64_t boolean_rows;
  uint64_t integer_rows;
  uint64_t double_rows;
  uint64_t date_rows;
  uint64_t datetime_rows;
  uint64_t string_rows;
  uint64_t undecided_rows;
} tgx_type_classes_counts;
tgx_status tgx_type_classes_get(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                tgx_type_classes_counts *out, tgx_error *err);

/* ---- value counts (TGX_CHECK_VALUE_COUNTS; TG/constraints/histogram.rs:205-391) ----------------------------------- */
typedef struct tgx_value_counts_summary {
  uint64_t seen;          /* rows handed to tgx_update */
  uint64_t non_null;      /* non-NULL rows (a row whose dictionary entry is NULL is a NULL row) */
  uint64_t distinct;      /* values held; may exceed max_distinct: the caller compares */
  uint64_t counted;       /* rows counted in the entries: the sum of their counts */
  uint64_t overflow_rows; /* non-NULL rows whose value found no slot */
  uint64_t long_rows;     /* string rows longer than max_value_bytes: they are in no entry */
} tgx_value_counts_summary; /* counted + overflow_rows + long_rows == non_null */
tgx_status tgx_value_counts_get(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                tgx_value_counts_summary *out, tgx_error *err);
/* One value and its count.  Integer columns: `value`; string columns: bytes [offset, offset + length) of the caller's
 * byte buffer (value is 0 there; offset and length are 0 for integers). */
typedef struct tgx_value_count_entry {
  int64_t value;
  uint64_t offset, length;
  uint64_t count;
} tgx_value_count_entry;
/* Copies the entries, ascending by value: int64 order for integer columns, bytewise (unsigned bytes, a prefix first) for
 * strings, so two reads of equal states are byte-identical.  The convention of tgx_joint_counts: *n_entries and *n_bytes
 * always receive what is needed; `entries` (cap entries) and `bytes` (bytes_cap bytes) may be NULL for a size query; a
 * non-NULL buffer that is too small makes the call return TGX_INVALID_ARGUMENT with nothing copied.  *is_bytes = 1 when
 * the values are strings, 0 when they are integers or the state has seen no value yet. */
tgx_status tgx_value_counts_entries(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                    tgx_value_count_entry *entries, uint64_t cap, uint64_t *n_entries, uint8_t *bytes,
                                    uint64_t bytes_cap, uint64_t *n_bytes, int32_t *is_bytes, tgx_error *err);

/* ---- pair counts (TGX_CHECK_PAIR_COUNTS; TG/analyzers/advanced/mutual_information.rs:249-293) -------------------- */
typedef struct tgx_pair_counts_summary {
  uint64_t seen;          /* rows handed to tgx_update */
  uint64_t both_non_null; /* rows with both sides non-NULL (a row whose dictionary entry is NULL is a NULL row) */
  uint64_t distinct;      /* pairs held; may exceed max_pairs: the caller compares */
  uint64_t counted;       /* rows counted in the entries: the sum of their counts */
  uint64_t overflow_rows; /* rows whose pair found no slot */
  uint64_t long_rows;     /* rows with a string longer than max_value_bytes on either side: they are in no entry */
  uint64_t non_finite;    /* rows, not long ones, whose binned side holds a NaN or an infinity */
  uint64_t out_of_range;  /* rows, neither long nor non-finite, whose bin index fell outside [0, bins] */
} tgx_pair_counts_summary; /* counted + overflow_rows + long_rows + non_finite + out_of_range == both_non_null */
/* A spec in its RANGE phase answers seen and both_non_null and leaves the rest zero. */
tgx_status tgx_pair_counts_get(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                               tgx_pair_counts_summary *out, tgx_error *err);
/* A spec in its RANGE phase: the numeric side over the rows with both sides non-NULL.  A spec in its count phase is
 * refused with TGX_INVALID_ARGUMENT. */
typedef struct tgx_pair_range {
  uint64_t seen;          /* rows handed to tgx_update */
  uint64_t both_non_null; /* rows with both sides non-NULL */
  uint64_t n;             /* those of them whose numeric side is finite */
  uint64_t non_finite;    /* those of them whose numeric side is a NaN or an infinity: n + non_finite == both_non_null */
  double min, max;        /* CAST AS DOUBLE, over the n rows; NaN when n == 0 */
} tgx_pair_range;
tgx_status tgx_pair_range_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_pair_range *out,
                              tgx_error *err);
/* One pair and its count.  A string side: bytes [offset, offset + length) of the caller's byte buffer (its bin is 0); a
 * binned side: its bin index (offset and length are 0). */
typedef struct tgx_pair_count_entry {
  int64_t x_bin, y_bin;
  uint64_t x_offset, x_length;
  uint64_t y_offset, y_length;
  uint64_t count;
} tgx_pair_count_entry;
/* Copies the entries, ascending by (x cell, y cell): strings bytewise (unsigned bytes, a prefix first), bins as
 * integers, so two reads of equal states are byte-identical.  The convention of tgx_value_counts_entries: *n_entries
 * and *n_bytes always receive what is needed; `entries` (cap entries) and `bytes` (bytes_cap bytes) may be NULL for a
 * size query; a non-NULL buffer that is too small makes the call return TGX_INVALID_ARGUMENT with nothing copied.  A
 * spec in its RANGE phase has no entries. */
tgx_status tgx_pair_counts_entries(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                   tgx_pair_count_entry *entries, uint64_t cap, uint64_t *n_entries, uint8_t *bytes,
                                   uint64_t bytes_cap, uint64_t *n_bytes, tgx_error *err);

/* ---- group counts (TGX_CHECK_GROUP_COUNTS; TG/analyzers/basic/grouped_completeness.rs:160-200) ----------------------- */
typedef struct tgx_group_counts_summary {
  uint64_t seen;                /* rows handed to tgx_update */
  uint64_t groups;              /* non-NULL keys held; may exceed max_groups: the caller compares */
  uint64_t counted;             /* rows counted in the entries: the sum of their totals */
  uint64_t counted_non_null;    /* ... of them with a non-NULL value: the sum of the entries' non_null */
  uint64_t null_group_rows;     /* rows whose group key is NULL */
  uint64_t null_group_non_null; /* ... of them with a non-NULL value */
  uint64_t overflow_rows;       /* rows whose key found no slot */
  uint64_t overflow_non_null;
  uint64_t long_rows;           /* rows whose string key is longer than max_value_bytes: they are in no entry */
  uint64_t long_non_null;
} tgx_group_counts_summary; /* counted + null_group_rows + overflow_rows + long_rows == seen, and the same of the
                             * *_non_null counters == COUNT(value column) */
tgx_status tgx_group_counts_get(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                tgx_group_counts_summary *out, tgx_error *err);
/* One group: its key and its two counts.  Integer keys: `value`; string keys: bytes [offset, offset + length) of the
 * caller's byte buffer (value is 0 there; offset and length are 0 for integers). */
typedef struct tgx_group_count_entry {
  int64_t value;
  uint64_t offset, length;
  uint64_t total;    /* COUNT(*) of the group */
  uint64_t non_null; /* COUNT(col) of the group */
} tgx_group_count_entry;
/* Copies the entries, ascending by key, in the convention of tgx_value_counts_entries (order, size query, a too-small
 * buffer is TGX_INVALID_ARGUMENT with nothing copied, *is_bytes).  The NULL group is not an entry: it is in the summary. */
tgx_status tgx_group_counts_entries(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                    tgx_group_count_entry *entries, uint64_t cap, uint64_t *n_entries, uint8_t *bytes,
                                    uint64_t bytes_cap, uint64_t *n_bytes, int32_t *is_bytes, tgx_error *err);

/* ---- group sums (TGX_CHECK_GROUP_SUMS; TG/constraints/cross_table_sum.rs:251-262) ------------------------------------ */
/* one class of rows: COUNT(*), COUNT(col) and SUM(col) over it.  Integer value columns: sum_i is the wrapping sum and
 * sum_f is (double)sum_i; float value columns: sum_f is the sum and sum_i is 0 */
typedef struct tgx_group_sums_class {
  uint64_t rows;
  uint64_t non_null;
  int64_t sum_i;
  double sum_f;
} tgx_group_sums_class;
typedef struct tgx_group_sums_summary {
  uint64_t seen;   /* rows handed to tgx_update */
  uint64_t groups; /* non-NULL keys held; may exceed max_groups: the caller compares */
  int32_t is_float; /* the sums are doubles (a Float64 / Float32 value column); 0 while no row was seen */
  int32_t reserved;
  tgx_group_sums_class counted;    /* the entries together (float sums: added in ascending key order) */
  tgx_group_sums_class null_group; /* rows whose group key is NULL */
  tgx_group_sums_class overflow;   /* rows whose key found no slot */
  tgx_group_sums_class long_rows;  /* rows whose string key is longer than max_value_bytes: they are in no entry */
} tgx_group_sums_summary; /* the four classes' rows add up to seen, their non_null to COUNT(col), their sum_i (integer
                           * value columns, wrapping) to SUM(col) */
tgx_status tgx_group_sums_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_group_sums_summary *out,
                              tgx_error *err);
/* One group: its key as in tgx_group_count_entry, its two counts and its sum (sum_i / sum_f as in tgx_group_sums_class;
 * has no value, in SQL's sense, when non_null is 0: both sums are 0 then) */
typedef struct tgx_group_sum_entry {
  int64_t value;
  uint64_t offset, length;
  uint64_t rows;     /* COUNT(*) of the group */
  uint64_t non_null; /* COUNT(col) of the group */
  int64_t sum_i;
  double sum_f;
} tgx_group_sum_entry;
/* Copies the entries, ascending by key, in the convention of tgx_group_counts_entries. */
tgx_status tgx_group_sums_entries(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                  tgx_group_sum_entry *entries, uint64_t cap, uint64_t *n_entries, uint8_t *bytes,
                                  uint64_t bytes_cap, uint64_t *n_bytes, int32_t *is_bytes, tgx_error *err);

/* ---- key probe (TGX_CHECK_KEY_PROBE; TG/constraints/foreign_key.rs:152-176) ----------------------------------------- */
/* The parent's key set of spec `spec_index` of `state`: n_records 16-byte {uint64 key, uint64 count} records in device
 * memory -- what tgx_distinct_export(.., world = 1, ..) hands out for a numeric key set, the extra record of the all-ones
 * key included.  Counts are ignored (by a plain spec; a counted one: below), duplicate records are allowed,
 * n_records == 0 is a valid, empty set.  The call
 * builds the state's own probe structure (a bitmap over [MIN, MAX] when MAX - MIN + 1 <= 128 * n_records, else a hash
 * table of the smallest power of two >= 2 * n_records slots) and has waited for it when it returns: the caller's
 * records are not kept.  Allowed only on a state that has seen no batch since it was created or reset
 * (TGX_INVALID_ARGUMENT otherwise); a state that holds counts -- merged in or deserialized -- refuses a set whose
 * (parent_keys, parent_digest) differ from the ones those counts were taken under. */
tgx_status tgx_key_probe_set_parent(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                    const void *device_records, uint64_t n_records, tgx_error *err);
typedef struct tgx_key_probe_summary {
  uint64_t seen;          /* rows handed to tgx_update */
  uint64_t non_null;
  uint64_t null_rows;     /* seen == non_null + null_rows */
  uint64_t matched;       /* non-NULL rows whose key is in the set */
  uint64_t missing_rows;  /* ... whose key is not: non_null == matched + missing_rows */
  uint64_t counted;       /* missing rows counted in the entries: the sum of their counts */
  uint64_t overflow_rows; /* missing rows whose key found no slot: missing_rows == counted + overflow_rows */
  uint64_t missing_keys;  /* entries held; may exceed max_missing_keys: the caller compares */
  uint64_t parent_keys;   /* distinct keys of the set (0 while the state knows of none) */
  uint64_t parent_digest; /* the wrapping 64-bit sum of mix64(key ^ 0x9e3779b97f4a7c15) over them, mix64 the splitmix64
                           * finaliser: independent of order, computed by the device during the build */
  uint32_t route;         /* of the set this state holds: 0 none or empty, 1 bitmap, 2 hash table */
  uint32_t reserved;
} tgx_key_probe_summary;
tgx_status tgx_key_probe_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_key_probe_summary *out,
                             tgx_error *err);
/* One missing key and the rows that hold it. */
typedef struct tgx_key_probe_entry {
  int64_t value;
  uint64_t count;
} tgx_key_probe_entry;
/* Copies the missing keys, ascending by value.  *n_entries always receives what is needed; `entries` (cap entries) may
 * be NULL for a size query; a non-NULL buffer that is too small is TGX_INVALID_ARGUMENT with nothing copied. */
tgx_status tgx_key_probe_entries(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                 tgx_key_probe_entry *entries, uint64_t cap, uint64_t *n_entries, tgx_error *err);
/* A COUNTED spec (tgx_plan_set_key_probe_counted).  tgx_key_probe_set_parent uses the records' counts: duplicate records
 * of one key add up, as a merge of two exports would; a record whose count is 0 is TGX_INVALID_ARGUMENT and a set whose
 * counts sum to 2^63 or more is TGX_UNSUPPORTED, and the state is then left without a set.  The routes are 3, an array of
 * 64-bit counts over [MIN, MAX] when MAX - MIN + 1 (unsigned, not 0) <= 4 * n_records, and 4, a hash table of the smallest
 * power of two >= 2 * n_records 16-byte {key, count} slots.  The three calls above work unchanged (`route` reads 3 or 4,
 * 0 for none or empty); the set's identity, which blobs carry and merges compare, is (parent_keys, parent_digest,
 * parent_rows, parent_count_digest).
 * For L LEFT JOIN R ON L.l = R.r with R's DISTINCT export as the set and L.l as the column, pairs is
 * SUM(CASE WHEN R.r IS NOT NULL ..) and join_rows is COUNT(*); pairs is the same number from either side.
 * pairs is exact whenever it is reported: the library keeps the upper bound sum over batches of max_count * rows in
 * checked arithmetic, and tgx_update refuses (TGX_UNSUPPORTED, nothing noted or run, the state stays usable) the batch
 * that would carry the bound past 2^64 - 1; merges and blobs add pairs under the same check.
 * TGX_INVALID_ARGUMENT on a plain spec. */
typedef struct tgx_key_probe_pairs {
  uint64_t pairs;               /* the sum over matched rows of the key's multiplicity in the set */
  uint64_t join_rows;           /* pairs + missing_rows + null_rows: COUNT(*) of the outer join from this side */
  uint64_t parent_rows;         /* the sum of the set's counts: the parent's non-NULL rows */
  uint64_t parent_count_digest; /* the wrapping sum of count * mix64(key ^ 0xc2b2ae3d27d4eb4f) over the records */
  uint64_t max_count;           /* the largest multiplicity of the set */
} tgx_key_probe_pairs;
tgx_status tgx_key_probe_pairs_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_key_probe_pairs *out,
                                   tgx_error *err);
/* The records a rows spec (tgx_plan_set_key_probe_rows) has gathered: *n_records 16-byte {key, 1} records in device
 * memory the state owns, valid until its next batch or reset; in no particular order.  A rows strings spec
 * (tgx_plan_set_key_probe_rows_strings): *n_records 32-byte {hash_a, hash_b, count, 0} records.  TGX_INVALID_ARGUMENT on
 * any other spec. */
tgx_status tgx_key_probe_rows_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, const void **device_records,
                                  uint64_t *n_records, tgx_error *err);
/* A STRINGS spec (tgx_plan_set_key_probe_strings).  tgx_key_probe_set_parent takes n_records 32-byte
 * {uint64 hash_a, uint64 hash_b, uint64 count, uint64 0} records in device memory -- what
 * tgx_distinct_export(.., world = 1, ..) hands out for a string column, with or without TGX_FLAG_EXACT_KEYS on the
 * parent's spec.  Counts are ignored, duplicate records are allowed, n_records == 0 is the empty set.  The records must
 * have been made under the fingerprint key that the child's plan carries: copy it with
 * tgx_plan_get_fingerprint_key(parent plan) into tgx_plan_set_fingerprint_key(child plan) before the child plan's first
 * state.  THE LIBRARY CANNOT VERIFY THIS: a set made under another key simply matches nothing.  A record whose hash_a or
 * hash_b is all ones (the free-slot marker, which no fingerprint is) is TGX_INVALID_ARGUMENT, and the state is then left
 * without a set.  The set is route 5: a hash table of the smallest power of two >= 2 * n_records 16-byte slots; its
 * identity, which blobs carry and merges compare, is (parent_keys, parent_digest) with parent_digest the wrapping sum
 * over the distinct fingerprints of mix64(mix64(hash_a ^ 0x9e3779b97f4a7c15) ^ hash_b).
 * tgx_key_probe_get works unchanged (`route` reads 5, 0 for none or empty) with
 *   seen == non_null + null_rows,  non_null == matched + missing_rows,  missing_rows == counted + overflow_rows + long_rows
 * where long_rows (tgx_key_probe_strings_get) are the MISSING rows whose value is longer than max_value_bytes; a long
 * value that is in the set is matched like any other.  Rows of a dictionary column whose entry is NULL or whose index
 * lies outside the dictionary are NULL rows.
 * The guarantee is the one of VALUE_COUNTS and of DISTINCT without TGX_FLAG_EXACT_KEYS: all counts are exact over
 * FINGERPRINTS.  A child value that is not in the parent is reported as matched only if all 128 bits of its fingerprint
 * agree with a parent value's, under a key that the data's producer does not know; the missing keys keep their bytes.
 * A blob that holds such a task with a known, non-empty set is a KEYED blob: its header carries the plan's fingerprint
 * key, and tgx_state_deserialize under a plan with another key refuses it; a blob that holds such a task and carries no
 * key is malformed.  States of different identities, of different
 * max_value_bytes, or of an integer and a strings spec do not merge.
 * tgx_key_probe_entries, tgx_key_probe_pairs_get and tgx_key_probe_rows_get are TGX_INVALID_ARGUMENT on such a spec, and
 * the two calls below on every spec that is neither such a spec nor a counted strings spec.
 * A COUNTED STRINGS spec (tgx_plan_set_key_probe_strings_counted) is a strings spec whose set keeps counts.
 * tgx_key_probe_set_parent takes the same 32-byte records and uses their counts: duplicate records of one fingerprint
 * add up (within one call's records); a count of 0 and a marker word in hash_a or hash_b are TGX_INVALID_ARGUMENT,
 * counts that sum to 2^63 or more are TGX_UNSUPPORTED, and the state is then left without a set.  The set is route 6:
 * route 5's table of 16-byte slots, and beside it one 64-bit count per slot (a miss reads the slot table only, a hit 8
 * bytes more).  Its identity, which blobs carry and merges compare, is (parent_keys, parent_digest, parent_rows,
 * parent_count_digest): parent_digest is route 5's, parent_count_digest the wrapping sum over the distinct fingerprints
 * of count * mix64(mix64(hash_a ^ 0xc2b2ae3d27d4eb4f) ^ hash_b).  tgx_key_probe_get (`route` reads 6), the two calls
 * below and tgx_key_probe_pairs_get work on it: pairs is the sum over the matched rows of their fingerprint's count,
 * join_rows = pairs + missing_rows + null_rows (long rows are missing rows), under tgx_key_probe_pairs_get's bound.
 * Its blob is keyed as a strings spec's is; a counted strings spec, a strings spec and an integer spec never merge
 * with one another. */
typedef struct tgx_key_probe_strings {
  uint64_t long_rows;       /* missing rows whose value is longer than max_value_bytes */
  uint32_t max_value_bytes; /* the plan's */
  uint32_t reserved;
} tgx_key_probe_strings;
tgx_status tgx_key_probe_strings_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_key_probe_strings *out,
                                     tgx_error *err);
/* Copies the missing keys, ascending bytewise: entry i's bytes are bytes[offset .. offset + length), its `value` is 0.
 * Sizes and buffers as for tgx_value_counts_entries: *n_entries and *n_bytes always receive what is needed; `entries`
 * may be NULL for a size query; a non-NULL buffer that is too small is TGX_INVALID_ARGUMENT with nothing copied. */
tgx_status tgx_key_probe_entries_bytes(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                       tgx_value_count_entry *entries, uint64_t cap, uint64_t *n_entries, uint8_t *bytes,
                                       uint64_t bytes_cap, uint64_t *n_bytes, tgx_error *err);
/* A TUPLES spec (a column list, tgx_plan_set_key_probe_tuples / _tuples_counted): the join key is the tuple
 * (c0, c1, ..) of the row's components -- JoinCoverageConstraint::on_multiple, TG/constraints/join_coverage.rs:127-138,
 * the join condition at :192-197.
 *   components    the sign- or zero-extended int64 of an Int64-shaped, Int32 / Date32 or Int8 .. UInt32 column, or the
 *                 row's string in any of the four string layouts.  A NULL dictionary entry and an index outside the
 *                 dictionary are a NULL component.  Float32 / Float64 (SQL's = is not bit equality), UInt64, Boolean and
 *                 validity-only components are TGX_UNSUPPORTED from tgx_update: nothing is noted, the state stays usable.
 *   the key       the tuple's keyed 128-bit fingerprint, the one TGX_CHECK_DISTINCT keeps for a tuple of the same
 *                 components, bit for bit: a narrow column joins a wide one, any string layout joins any other,
 *                 ("ab","c") != ("a","bc") and (1,2) != (2,1).
 *   the set       tgx_key_probe_set_parent takes 32-byte {hash_a, hash_b, count, 0} records as a strings spec does, with
 *                 the same refusals (marker words, zero counts, sums of 2^63 or more) and the same identities; `route`
 *                 reads 5 (plain) or 6 (counted).  The records must be tuple fingerprints of the SAME ARITY under the
 *                 plan's fingerprint key -- what a rows tuples spec gathers, or a tuple DISTINCT's export.  THE LIBRARY
 *                 CANNOT VERIFY THIS: records of another arity, another key or of single values simply match nothing.
 *   NULLs         SQL's join: a row with at least one NULL component matches nothing -- a parent tuple with a NULL in
 *                 the same place included, although the two fingerprint alike.  Such a row is never looked up; it is a
 *                 null_rows row, and non_null counts the rows whose every component is non-NULL.  A rows tuples spec
 *                 emits no record for it.  The three identities of tgx_key_probe_summary hold verbatim over the all-valid
 *                 rows; there are no long rows, since the table keeps fingerprints and no bytes.
 *   two classes   the reference's examples query is SELECT DISTINCT l0, l1 .. WHERE R.r0 IS NULL, where a NULL-bearing
 *                 tuple is a distinct value of its own: those rows are counted per distinct tuple too, apart from the
 *                 missing keys (tgx_key_probe_summary's counted, overflow_rows and missing_keys speak of the missing
 *                 tuples only):  null_rows == null_counted + null_overflow_rows.  max_missing_keys bounds EACH class as it
 *                 bounds the missing keys of the other modes: each has a table of its own, a power of two of at
 *                 least 2 * max_missing_keys slots, so neither class can crowd the other out; missing_keys and
 *                 null_keys may each exceed max_missing_keys, and the caller compares.
 * tgx_state_reset clears counters and entries and keeps the set.  tgx_merge, blobs and tgx_allreduce behave as for a
 * strings spec: the blob is keyed and carries the arity, a deserialized state holds no set, and states of different
 * arity, mode or identity, and a tuples spec with a strings or an integer spec, do not merge.
 * tgx_key_probe_entries, tgx_key_probe_entries_bytes and tgx_key_probe_strings_get are TGX_INVALID_ARGUMENT on such a
 * spec, the two calls below on every other spec. */
typedef struct tgx_key_probe_tuples {
  uint64_t null_counted;       /* rows with a NULL component that are counted in the entries */
  uint64_t null_overflow_rows; /* ... whose tuple found no slot */
  uint64_t null_keys;          /* entries of NULL-bearing tuples held */
  uint32_t arity;              /* the plan's: columns of the tuple */
  uint32_t reserved;
} tgx_key_probe_tuples;
tgx_status tgx_key_probe_tuples_get(const tgx_plan *plan, tgx_state *state, size_t spec_index, tgx_key_probe_tuples *out,
                                    tgx_error *err);
/* One tuple that is not in the set, or that holds a NULL, and its rows.  Only its fingerprint is kept. */
typedef struct tgx_key_probe_tuple_entry {
  uint64_t hash_a;
  uint64_t hash_b;
  uint64_t count;
  uint32_t has_null; /* 1: a tuple with at least one NULL component; 0: an all-valid tuple missing from the set */
  uint32_t reserved;
} tgx_key_probe_tuple_entry;
/* Copies the entries of both classes together, ascending by (hash_a, hash_b).  Sizes as for tgx_key_probe_entries. */
tgx_status tgx_key_probe_entries_tuples(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                                        tgx_key_probe_tuple_entry *entries, uint64_t cap, uint64_t *n_entries,
                                        tgx_error *err);

/* ---- exact DISTINCT across ranks: hash-owner key exchange -------------
 * export: partitions this state's key set by owner = mix(key) % world into `world` contiguous
 *   runs of fixed-size records (tgx_distinct_record_bytes) in device memory the state owns (valid until the next call on the
 *   state); counts[r] = records for rank r.
 * import: replaces the state's key set with the union of the given records (device memory),
 *   marking the state "owner-partitioned" so that tgx_merge adds its counts instead of uniting. */
/* bytes per exchange record: 16 ({key, count}) for Int64/Float64 columns, 32 ({hash_a, hash_b, count, 0})
 * for Utf8 columns, whose values travel as 128-bit fingerprints */
size_t tgx_distinct_record_bytes(const tgx_plan *plan, const tgx_state *state, size_t spec_index);
tgx_status tgx_distinct_export(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                               uint32_t world, const void **device_records, uint64_t *counts,
                               tgx_error *err);
tgx_status tgx_distinct_import(const tgx_plan *plan, tgx_state *state, size_t spec_index,
                               const void *device_records, uint64_t n_records, tgx_error *err);

/* Range-bitmap shortcut of the exchange, for Int64 columns whose global value range is dense:
 *   1. all ranks agree on the column's global [lo, hi] (all-reduce of their MIN/MAX) and call
 *      tgx_distinct_range_hint before the first batch: every rank then builds a bitmap with base = lo, so the
 *      bitmaps are congruent; keys outside [lo, hi] are counted and make tgx_finalize fail (never a wrong count);
 *   2. tgx_distinct_bitmap_view exposes the bitmap (device pointers, 32-bit words); ranks all-to-all equal
 *      slices of it (a few hundred MB per rank instead of 16 bytes per key);
 *   3. tgx_distinct_adopt_slices ORs the received slices (`n_slices` slices of `slice_words` words, slice i at
 *      word offset i * `slice_stride_words` -- 0 means packed, i.e. slice_words -- so the receive buffer of an
 *      all-to-all that carries several columns per peer is used in place; the "seen twice" slices too when
 *      the check wants multiplicity) into the rank's owned slice, whose first bit stands for key `slice_base`,
 *      and marks the state owner-partitioned.
 * tgx_distinct_bitmap_view returns TGX_UNSUPPORTED when the set is a hash table: use export / import then. */
tgx_status tgx_distinct_range_hint(const tgx_plan *plan, tgx_state *state, size_t spec_index, int64_t lo, int64_t hi,
                                   tgx_error *err);
tgx_status tgx_distinct_bitmap_view(const tgx_plan *plan, tgx_state *state, size_t spec_index, int64_t *base,
                                    uint64_t *n_words, const void **seen, const void **twice, tgx_error *err);
tgx_status tgx_distinct_adopt_slices(const tgx_plan *plan, tgx_state *state, size_t spec_index, int64_t slice_base,
                                     const void *seen_slices, const void *twice_slices, uint32_t n_slices,
                                     uint64_t slice_words, uint64_t slice_stride_words, tgx_error *err);

/* ---- the cross-rank step ------------------------------------------------
 * Rows shard by row range, one process per GPU.  Every rank runs tgx_update on its shard; tgx_allreduce then turns
 * each rank's state into the state of the WHOLE table -- `AnalyzerState::merge` (TG/analyzers/traits.rs:160-170)
 * applied across ranks:
 *   1. the ranks all-gather a few scalars per DISTINCT column: its MIN / MAX (the running values of the scan), the
 *      kind of key set the rank built, its rows;
 *   2. exact DISTINCT sets swap ONE all-to-all: where every rank holds a range bitmap, equal slices of the bitmaps,
 *      re-based on the agreed global range on the fly (the local bitmaps need not be congruent), all columns in one
 *      collective -- range / 8 bytes per rank and column; otherwise fixed-size key records by hash owner;
 *   3. the packed partial states (a few KiB; KLL about 100 KiB) travel in one all-gather and are folded in rank
 *      order, so every rank ends with bit-identical results.
 * After the call tgx_finalize(state) returns the global results on every rank; the state keeps its device buffers
 * for the next tgx_state_reset / tgx_update round.
 *   0. (before the above, for plans with SPEARMAN checks) RANK() over the union of the ranks' pairs: rank-based
 *      states do not merge (TG's neither, analyzers/advanced/correlation.rs:103-109), so the call runs a distributed
 *      sort per column -- local sort, world-1 splitters agreed from regular samples, every key to the rank that owns
 *      its value range (equal keys meet there), ranked, the rank back to its row: two all-to-all-v of 8 bytes per pair
 *      and column -- and adds up the five rank sums.  Every rank then answers with the sums of the whole table; such
 *      a state takes no further batches until it is reset, and still neither merges nor serializes.
 *
 * A tgx_comm is the transport: RCCL over xGMI (tgx_comm_create_rccl: the library dlopens librccl.so.1, calls
 * ncclCommInitRank itself and owns the communicator; tgx_comm_adopt_rccl wraps a caller-owned ncclComm_t), or any
 * transport of the caller's through tgx_comm_ops (MPI, gloo, the threaded stand-in of the tests).  All ranks must
 * call tgx_allreduce with the same plan, in the same order. */
typedef struct tgx_comm tgx_comm;
typedef struct tgx_comm_ops {
  void *ctx;
  int32_t rank, world;
  /* 1: the collectives below take DEVICE pointers and are ordered on `hip_stream`; 0: they take HOST pointers
   * (the library stages through pinned memory and synchronises the stream itself) and may block */
  int32_t device_buffers;
  int32_t reserved;
  /* every rank sends `bytes_per_peer` bytes to every rank: send / recv hold world blocks, block r goes to / comes
   * from rank r */
  int32_t (*alltoall)(void *ctx, const void *send, void *recv, size_t bytes_per_peer, void *hip_stream);
  /* block r of send holds send_counts[r] elements of elem_bytes for rank r (packed back to back); recv likewise */
  int32_t (*alltoallv)(void *ctx, const void *send, const uint64_t *send_counts, void *recv,
                       const uint64_t *recv_counts, size_t elem_bytes, void *hip_stream);
  /* every rank contributes `bytes` bytes; recv holds world blocks in rank order */
  int32_t (*allgather)(void *ctx, const void *send, void *recv, size_t bytes, void *hip_stream);
} tgx_comm_ops; /* every callback returns 0 on success */

#define TGX_RCCL_UNIQUE_ID_BYTES 128
tgx_status tgx_comm_create(const tgx_comm_ops *ops, tgx_comm **out, tgx_error *err);
/* rank 0 makes the id (ncclGetUniqueId) and hands it to the other ranks by any means */
tgx_status tgx_comm_rccl_unique_id(uint8_t id[TGX_RCCL_UNIQUE_ID_BYTES], tgx_error *err);
tgx_status tgx_comm_create_rccl(const uint8_t id[TGX_RCCL_UNIQUE_ID_BYTES], int32_t rank, int32_t world,
                                tgx_comm **out, tgx_error *err);
tgx_status tgx_comm_adopt_rccl(void *nccl_comm, int32_t rank, int32_t world, tgx_comm **out, tgx_error *err);
void tgx_comm_destroy(tgx_comm *comm);
tgx_status tgx_allreduce(const tgx_plan *plan, tgx_state *state, tgx_comm *comm, tgx_error *err);

/* ---- measurement ----------------------------------------------------------------------------
 * Per-kernel HIP-event timing on the state's stream (what bench.py's `roofline` uses).
 * Kernel names: "scan", "count", "distinct", "regex", "kll", "comoments", "joint_range", "joint_bins", "temporal", "value_rule", "value_counts", "pair_range", "pair_counts", "group_counts", "group_counts_tuples", "group_sums", "group_sums_tuples", "key_probe", "key_probe_build", "key_probe_rows", "row_predicate", "type_classes","hist_range",
 * "hist_counts"; "distinct_lists" is the share of
 * "distinct" spent on big Utf8 batches that were deduplicated through partitioned fingerprint lists. */
tgx_status tgx_profile_enable(tgx_state *state, int32_t on);
tgx_status tgx_profile_get(tgx_state *state, const char *kernel, double *total_ms,
                           uint64_t *launches, uint64_t *algorithmic_bytes, tgx_error *err);
tgx_status tgx_profile_reset(tgx_state *state);

/* ---- host-side rules the Rust shim shares with the reference -------------------------------- */
/* SqlSecurity::validate_regex_pattern (TG/security.rs:152-183) + "does the engine cover it". */
tgx_status tgx_regex_validate(const char *pattern, size_t len, uint32_t flags, tgx_error *err);
/* Host-side `is_match` of the compiled automaton for one value (debug / small inputs). */
tgx_status tgx_regex_is_match(const char *pattern, size_t plen, uint32_t flags, const uint8_t *value,
                              size_t vlen, int32_t *matched, tgx_error *err);
/* What the device's launch decides from, for one pattern: the size of the compiled automaton (states x byte classes
 * picks the table's place: byte-indexed, in LDS, or in global memory) and its character count -- *len_min / *len_max
 * are -1 unless the pattern is an automaton AND a count (`^C{m,n}$`).  The same compile as tgx_plan_create's; launches
 * and allocates nothing on the device. */
tgx_status tgx_regex_table_info(const char *pattern, size_t len, uint32_t flags, uint32_t *n_states,
                                uint32_t *n_classes, int64_t *len_min, int64_t *len_max, tgx_error *err);

/* Host-side walk of the PRODUCT automaton of up to 4 patterns -- the form in which several pattern checks of one
 * column are evaluated on the device (one walk over the value decides all of them).  Bit k of *mask: pattern k
 * matches `value`.  *grouped = 0 when the product exceeds the device's table limit: the patterns then run one by
 * one (and *mask is computed that way).  TRIM is applied per pattern here; on the device only patterns with the same
 * TRIM flag share a walk. */
tgx_status tgx_regex_match_group(const char *const *patterns, const size_t *pattern_lens, const uint32_t *flags,
                                 size_t n_patterns, const uint8_t *value, size_t vlen, uint32_t *mask,
                                 int32_t *grouped, tgx_error *err);

#ifdef __cplusplus
}
#endif
#endif /* TGX_H */
