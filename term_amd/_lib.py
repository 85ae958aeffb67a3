"""ctypes binding of libtgx.so (include/tgx.h).  Fails loudly when the library is missing."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)

# enums of include/tgx.h
COUNT, NUMERIC_STATS, DISTINCT, REGEX_MATCH, KLL, COMOMENTS, SPEARMAN, LENGTH = 1, 2, 3, 4, 5, 6, 7, 8
APPROX_DISTINCT = 9
JOINT_BINS = 10  # joint bin counts of a numeric pair, in two phases (Plan.set_joint_binning)
JOINT_MAX_BINS = 127
TEMPORAL = 11  # row predicates over timestamp columns (Plan.set_temporal)
TEMPORAL_ORDER, TEMPORAL_TIME_OF_DAY, TEMPORAL_RANGE = 1, 2, 3
TEMPORAL_KEEP_NULLS, TEMPORAL_WEEKDAYS_ONLY = 1, 2
HISTOGRAM = 12  # the histogram of a numeric column, in two phases (Plan.set_histogram_edges)
HISTOGRAM_MAX_BUCKETS = 1000
TIME_GAP = 13  # gaps between neighbouring timestamps, whole table or per group (Plan.set_time_gap)
VALUE_RULE = 14  # numeric value rules: >= 0, > 0, between, whole (Plan.set_value_rule)
RULE_GE_ZERO, RULE_GT_ZERO, RULE_BETWEEN, RULE_INTEGER = 1, 2, 3, 4
RULE_BOUNDS_AS_DOUBLE = 1
VALUE_COUNTS = 15  # how often each value of a column occurs, for a bounded number of values (Plan.set_value_counts)
VALUE_COUNTS_MAX_DISTINCT, VALUE_COUNTS_MAX_VALUE_BYTES = 65536, 256
PAIR_COUNTS = 16  # how often each pair of cells of two columns occurs, for a bounded number of pairs (Plan.set_pair_counts)
PAIR_SIDE_VALUE, PAIR_SIDE_RANGE, PAIR_SIDE_BINNED = 0, 1, 2
PAIR_COUNTS_MAX_PAIRS, PAIR_COUNTS_MAX_VALUE_BYTES = 65536, 256
GROUP_COUNTS = 17  # COUNT(*) and COUNT(col) per group of a second column, for a bounded number of groups (Plan.set_group_counts)
GROUP_COUNTS_MAX_GROUPS, GROUP_COUNTS_MAX_VALUE_BYTES = 65536, 256
KEY_PROBE = 19  # is each key of a child column in a parent's key set (Plan.set_key_probe, State.key_probe_set_parent)
KEY_PROBE_MAX_MISSING_KEYS = 65536
KEY_PROBE_MAX_VALUE_BYTES = 256  # of a missing key a spec on string keys keeps (Plan.set_key_probe_strings)
ROW_PREDICATE = 20  # the rows on which a closed boolean predicate over 1 .. 8 columns is TRUE / UNKNOWN (Plan.set_row_predicate)
PRED_MAX_COLUMNS, PRED_MAX_LEAVES, PRED_MAX_OPS, PRED_MAX_DEPTH, PRED_MAX_LITERAL_BYTES = 8, 32, 64, 32, 256
PRED_IS_NULL, PRED_CMP_LITERAL, PRED_CMP_COLUMNS, PRED_STR_EQ = 1, 2, 3, 4
PRED_STR_CMP, PRED_STR_LENGTH, PRED_STR_LIKE, PRED_STR_BLANK = 6, 7, 8, 9  # (5 is no kind)
PRED_EQ, PRED_LT, PRED_LE, PRED_GT, PRED_GE = 1, 2, 3, 4, 5
PRED_LITERAL_IS_DOUBLE = 1
PRED_LENGTH_IN_BYTES = 2
PRED_PUSH, PRED_AND, PRED_OR, PRED_NOT = 1, 2, 3, 4
TYPE_CLASSES = 21  # the syntactic class of every non-NULL value of a string column (State.type_classes)
# the classes in the order they are tried (TGX_TYPE_CLASS_*: what host_type_class answers)
(TYPE_CLASS_BOOLEAN, TYPE_CLASS_INTEGER, TYPE_CLASS_DOUBLE, TYPE_CLASS_DATE, TYPE_CLASS_DATETIME, TYPE_CLASS_STRING,
 TYPE_CLASS_UNDECIDED) = range(7)
TYPE_CLASS_NAMES = ("boolean", "integer", "double", "date", "datetime", "string", "undecided")
GROUP_SUMS = 18  # COUNT(*), COUNT(col) and SUM(col) per group of a second column, for a bounded number of groups (Plan.set_group_sums)
GROUP_SUMS_MAX_GROUPS, GROUP_SUMS_MAX_VALUE_BYTES = 65536, 256
FLAG_VARIANCE, FLAG_MULTIPLICITY, FLAG_TRIM, FLAG_CASE_INSENSITIVE, FLAG_NULL_IS_VALID = 1, 2, 4, 8, 16
FLAG_EXACT_RANK_SUMS = 32
FLAG_EXACT_KEYS = 64  # DISTINCT over string / tuple keys: equal fingerprints confirmed byte by byte
ABI_VERSION = 6  # include/tgx.h TGX_ABI_VERSION: the struct layouts below
INT64, FLOAT64, UTF8, LARGE_UTF8, DICT32_UTF8, UTF8_VIEW, INT32, FLOAT32 = 1, 2, 3, 4, 5, 6, 7, 8
INT8, INT16, UINT8, UINT16, UINT32, UINT64, BOOL = 9, 10, 11, 12, 13, 14, 15  # (include/tgx.h: narrow / unsigned / Boolean)
MEM_HOST, MEM_DEVICE, MEM_HOST_RETAINED = 0, 1, 2
STATUS_NAMES = {0: "TGX_OK", 1: "TGX_INVALID_ARGUMENT", 2: "TGX_UNSUPPORTED", 3: "TGX_DEVICE_ERROR",
                4: "TGX_OUT_OF_MEMORY", 5: "TGX_INTERNAL", 6: "TGX_NO_DEVICE"}


class TgxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (STATUS_NAMES.get(code, code), msg))
        self.code = code
        self.status = STATUS_NAMES.get(code, str(code))
        self.msg = msg


class _Error(C.Structure):
    _fields_ = [("code", C.c_int32), ("msg", C.c_char * 256)]


class _Column(C.Structure):
    pass


_Column._fields_ = [
    ("type", C.c_int32), ("mem", C.c_int32), ("length", C.c_int64), ("offset", C.c_int64),
    ("null_count", C.c_int64), ("validity", C.c_void_p), ("values", C.c_void_p), ("offsets", C.c_void_p),
    ("data", C.c_void_p), ("dictionary", C.POINTER(_Column)),
    ("variadic", C.POINTER(C.c_void_p)), ("variadic_sizes", C.POINTER(C.c_int64)), ("n_variadic", C.c_int32),
    ("reserved", C.c_int32),
]


class CheckSpec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("column", C.c_int32), ("column2", C.c_int32), ("flags", C.c_uint32),
                ("pattern", C.c_char_p), ("pattern_len", C.c_uint64), ("kll_k", C.c_uint32),
                ("reserved", C.c_uint32), ("columns", C.POINTER(C.c_int32)), ("n_columns", C.c_uint32),
                ("reserved2", C.c_uint32), ("length_min", C.c_uint64), ("length_max", C.c_uint64)]


class Result(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("is_float", C.c_int32), ("total", C.c_int64), ("non_null", C.c_int64),
        ("has_value", C.c_int32), ("has_variance", C.c_int32), ("min_i", C.c_int64), ("max_i", C.c_int64),
        ("min_f", C.c_double), ("max_f", C.c_double), ("sum_i", C.c_int64), ("sum_f", C.c_double),
        ("mean", C.c_double), ("var_samp", C.c_double), ("stddev_samp", C.c_double),
        ("distinct", C.c_int64), ("groups_once", C.c_int64), ("matches", C.c_int64),
        ("sum_x", C.c_double), ("sum_y", C.c_double), ("sum_x2", C.c_double), ("sum_y2", C.c_double),
        ("sum_xy", C.c_double), ("kll_n", C.c_uint64),
        ("co_mean_x", C.c_double), ("co_mean_y", C.c_double), ("co_m2_x", C.c_double), ("co_m2_y", C.c_double),
        ("co_c_xy", C.c_double),
    ]


class JointBinning(C.Structure):
    """tgx_joint_binning (include/tgx.h)"""
    _fields_ = [("x_origin", C.c_double), ("x_width", C.c_double), ("y_origin", C.c_double), ("y_width", C.c_double),
                ("bins", C.c_uint32), ("reserved", C.c_uint32)]


class JointRange(C.Structure):
    """tgx_joint_range (include/tgx.h)"""
    _fields_ = [("total", C.c_uint64), ("n", C.c_uint64), ("non_finite", C.c_uint64), ("x_min", C.c_double),
                ("x_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double)]


class TemporalParams(C.Structure):
    """tgx_temporal_params (include/tgx.h)"""
    _fields_ = [("mode", C.c_int32), ("flags", C.c_uint32), ("delta", C.c_int64), ("ticks_per_second", C.c_int64),
                ("tod_lo", C.c_int64), ("tod_hi", C.c_int64), ("lo", C.c_int64), ("hi", C.c_int64)]


class TemporalCounts(C.Structure):
    """tgx_temporal_counts (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("considered", C.c_uint64), ("violations", C.c_uint64)]


class TimeGapParams(C.Structure):
    """tgx_time_gap_params (include/tgx.h)"""
    _fields_ = [("max_gap", C.c_int64), ("flags", C.c_uint32)]


class TimeGapCounts(C.Structure):
    """tgx_time_gap_counts (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("rows", C.c_uint64), ("gaps", C.c_uint64), ("violations", C.c_uint64),
                ("largest_gap", C.c_uint64)]


class ValueRuleParams(C.Structure):
    """tgx_value_rule_params (include/tgx.h)"""
    _fields_ = [("mode", C.c_int32), ("flags", C.c_uint32), ("lo_i", C.c_int64), ("hi_i", C.c_int64),
                ("lo_f", C.c_double), ("hi_f", C.c_double)]


class ValueRuleCounts(C.Structure):
    """tgx_value_rule_counts (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("considered", C.c_uint64), ("valid", C.c_uint64), ("cast_errors", C.c_uint64)]


class RowPredicateLeaf(C.Structure):
    """tgx_row_predicate_leaf (include/tgx.h)"""
    _fields_ = [("kind", C.c_int32), ("op", C.c_int32), ("col", C.c_int32), ("col2", C.c_int32), ("flags", C.c_uint32),
                ("lit_offset", C.c_uint32), ("lit_len", C.c_uint32), ("reserved", C.c_uint32), ("lit_i", C.c_int64),
                ("lit_f", C.c_double)]


class RowPredicateParams(C.Structure):
    """tgx_row_predicate_params (include/tgx.h)"""
    _fields_ = [("n_leaves", C.c_uint32), ("n_ops", C.c_uint32), ("n_literal_bytes", C.c_uint32), ("reserved", C.c_uint32),
                ("leaves", RowPredicateLeaf * PRED_MAX_LEAVES), ("program", C.c_uint16 * PRED_MAX_OPS),
                ("literals", C.c_uint8 * PRED_MAX_LITERAL_BYTES)]


class RowPredicateCounts(C.Structure):
    """tgx_row_predicate_counts (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("satisfied", C.c_uint64), ("unknown", C.c_uint64), ("failed", C.c_uint64)]


class TypeClassesCounts(C.Structure):
    """tgx_type_classes_counts (include/tgx.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("seen", "non_null", "boolean_rows", "integer_rows", "double_rows", "date_rows",
                                          "datetime_rows", "string_rows", "undecided_rows")]


class ValueCountsParams(C.Structure):
    """tgx_value_counts_params (include/tgx.h)"""
    _fields_ = [("max_distinct", C.c_uint32), ("max_value_bytes", C.c_uint32)]


class ValueCountsSummary(C.Structure):
    """tgx_value_counts_summary (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("non_null", C.c_uint64), ("distinct", C.c_uint64), ("counted", C.c_uint64),
                ("overflow_rows", C.c_uint64), ("long_rows", C.c_uint64)]


class ValueCountEntry(C.Structure):
    """tgx_value_count_entry (include/tgx.h)"""
    _fields_ = [("value", C.c_int64), ("offset", C.c_uint64), ("length", C.c_uint64), ("count", C.c_uint64)]


class PairSide(C.Structure):
    """tgx_pair_side (include/tgx.h)"""
    _fields_ = [("mode", C.c_int32), ("bins", C.c_uint32), ("origin", C.c_double), ("width", C.c_double)]


class PairCountsParams(C.Structure):
    """tgx_pair_counts_params (include/tgx.h)"""
    _fields_ = [("max_pairs", C.c_uint32), ("max_value_bytes", C.c_uint32), ("x", PairSide), ("y", PairSide)]


class PairCountsSummary(C.Structure):
    """tgx_pair_counts_summary (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("both_non_null", C.c_uint64), ("distinct", C.c_uint64), ("counted", C.c_uint64),
                ("overflow_rows", C.c_uint64), ("long_rows", C.c_uint64), ("non_finite", C.c_uint64),
                ("out_of_range", C.c_uint64)]


class PairRange(C.Structure):
    """tgx_pair_range (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("both_non_null", C.c_uint64), ("n", C.c_uint64), ("non_finite", C.c_uint64),
                ("min", C.c_double), ("max", C.c_double)]


class PairCountEntry(C.Structure):
    """tgx_pair_count_entry (include/tgx.h)"""
    _fields_ = [("x_bin", C.c_int64), ("y_bin", C.c_int64), ("x_offset", C.c_uint64), ("x_length", C.c_uint64),
                ("y_offset", C.c_uint64), ("y_length", C.c_uint64), ("count", C.c_uint64)]


class GroupCountsParams(C.Structure):
    """tgx_group_counts_params (include/tgx.h)"""
    _fields_ = [("max_groups", C.c_uint32), ("max_value_bytes", C.c_uint32)]


class GroupCountsSummary(C.Structure):
    """tgx_group_counts_summary (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("groups", C.c_uint64), ("counted", C.c_uint64), ("counted_non_null", C.c_uint64),
                ("null_group_rows", C.c_uint64), ("null_group_non_null", C.c_uint64), ("overflow_rows", C.c_uint64),
                ("overflow_non_null", C.c_uint64), ("long_rows", C.c_uint64), ("long_non_null", C.c_uint64)]


class GroupCountEntry(C.Structure):
    """tgx_group_count_entry (include/tgx.h)"""
    _fields_ = [("value", C.c_int64), ("offset", C.c_uint64), ("length", C.c_uint64), ("total", C.c_uint64),
                ("non_null", C.c_uint64)]


class GroupSumsParams(C.Structure):
    """tgx_group_sums_params (include/tgx.h)"""
    _fields_ = [("max_groups", C.c_uint32), ("max_value_bytes", C.c_uint32)]


class GroupSumsClass(C.Structure):
    """tgx_group_sums_class (include/tgx.h)"""
    _fields_ = [("rows", C.c_uint64), ("non_null", C.c_uint64), ("sum_i", C.c_int64), ("sum_f", C.c_double)]


class GroupSumsSummary(C.Structure):
    """tgx_group_sums_summary (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("groups", C.c_uint64), ("is_float", C.c_int32), ("reserved", C.c_int32),
                ("counted", GroupSumsClass), ("null_group", GroupSumsClass), ("overflow", GroupSumsClass),
                ("long_rows", GroupSumsClass)]


class GroupSumEntry(C.Structure):
    """tgx_group_sum_entry (include/tgx.h)"""
    _fields_ = [("value", C.c_int64), ("offset", C.c_uint64), ("length", C.c_uint64), ("rows", C.c_uint64),
                ("non_null", C.c_uint64), ("sum_i", C.c_int64), ("sum_f", C.c_double)]


class KeyProbeParams(C.Structure):
    """tgx_key_probe_params (include/tgx.h)"""
    _fields_ = [("max_missing_keys", C.c_uint32), ("reserved", C.c_uint32)]


class KeyProbeSummary(C.Structure):
    """tgx_key_probe_summary (include/tgx.h)"""
    _fields_ = [("seen", C.c_uint64), ("non_null", C.c_uint64), ("null_rows", C.c_uint64), ("matched", C.c_uint64),
                ("missing_rows", C.c_uint64), ("counted", C.c_uint64), ("overflow_rows", C.c_uint64),
                ("missing_keys", C.c_uint64), ("parent_keys", C.c_uint64), ("parent_digest", C.c_uint64),
                ("route", C.c_uint32), ("reserved", C.c_uint32)]


class KeyProbeEntry(C.Structure):
    """tgx_key_probe_entry (include/tgx.h)"""
    _fields_ = [("value", C.c_int64), ("count", C.c_uint64)]


class KeyProbePairs(C.Structure):
    """tgx_key_probe_pairs (include/tgx.h)"""
    _fields_ = [("pairs", C.c_uint64), ("join_rows", C.c_uint64), ("parent_rows", C.c_uint64),
                ("parent_count_digest", C.c_uint64), ("max_count", C.c_uint64)]


class KeyProbeStringsParams(C.Structure):
    """tgx_key_probe_strings_params (include/tgx.h)"""
    _fields_ = [("max_missing_keys", C.c_uint32), ("max_value_bytes", C.c_uint32)]


class KeyProbeStrings(C.Structure):
    """tgx_key_probe_strings (include/tgx.h)"""
    _fields_ = [("long_rows", C.c_uint64), ("max_value_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class KeyProbeTuples(C.Structure):
    """tgx_key_probe_tuples (include/tgx.h)"""
    _fields_ = [("null_counted", C.c_uint64), ("null_overflow_rows", C.c_uint64), ("null_keys", C.c_uint64),
                ("arity", C.c_uint32), ("reserved", C.c_uint32)]


class KeyProbeTupleEntry(C.Structure):
    """tgx_key_probe_tuple_entry (include/tgx.h)"""
    _fields_ = [("hash_a", C.c_uint64), ("hash_b", C.c_uint64), ("count", C.c_uint64), ("has_null", C.c_uint32),
                ("reserved", C.c_uint32)]


class HistogramRange(C.Structure):
    """tgx_histogram_range (include/tgx.h)"""
    _fields_ = [("total", C.c_uint64), ("nulls", C.c_uint64), ("non_finite", C.c_uint64), ("n", C.c_uint64),
                ("min", C.c_double), ("max", C.c_double), ("sum", C.c_double), ("sum_squared", C.c_double)]


class _Options(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("flags", C.c_uint32), ("distinct_capacity_hint", C.c_uint64)]


def lib_path():
    # TGX_LIB: another build of the same library (the host-side sanitizer build, tools/run_host_asan.sh)
    return os.environ.get("TGX_LIB") or os.path.join(_HERE, "libtgx.so")


def abi_symbols():
    """Every function name include/tgx.h declares (parsed from the header)."""
    names = set()
    for header in ("tgx.h", "tgx_host.h"):
        with open(os.path.join(_ROOT, "include", header)) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names.update(re.findall(r"\b(tgx_[a-z0-9_]+)\s*\(", text))
    return sorted(names)


_LIB = None


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch's wheel carries its own libamdhip64.so (same SONAME as
    /opt/rocm's); if libtgx.so pulled in the system copy first and torch its own copy later, the second
    runtime to initialise finds no device.  Loading torch's copy first makes both resolve to it."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        found = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        found = None
    if found is None or not found.origin:
        return
    cand = os.path.join(os.path.dirname(found.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    global _LIB
    if _LIB is None:
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError(
                "term_amd/libtgx.so is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C term_amd/csrc` (hipcc, gfx950). term_amd has no CPU fallback.")
        _preload_hip_runtime()
        L = C.CDLL(path)
        vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
        E = C.POINTER(_Error)
        L.tgx_abi_version.restype = C.c_uint32
        if L.tgx_abi_version() != ABI_VERSION:
            raise ImportError("term_amd/libtgx.so speaks ABI %d, this binding ABI %d: rebuild it (make -C term_amd/csrc)"
                              % (L.tgx_abi_version(), ABI_VERSION))
        L.tgx_status_name.restype = C.c_char_p
        L.tgx_status_name.argtypes = [C.c_int32]
        L.tgx_init.argtypes = [C.POINTER(_Options), E]
        L.tgx_plan_create.argtypes = [C.POINTER(CheckSpec), sz, C.POINTER(vp), E]
        L.tgx_plan_destroy.argtypes = [vp]
        L.tgx_plan_destroy.restype = None
        L.tgx_plan_num_specs.argtypes = [vp]
        L.tgx_plan_num_specs.restype = sz
        L.tgx_blob_fingerprint_key.argtypes = [C.c_char_p, sz, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
        L.tgx_plan_set_fingerprint_key.argtypes = [vp, C.c_char_p, E]
        L.tgx_plan_get_fingerprint_key.argtypes = [vp, C.POINTER(C.c_uint8)]
        L.tgx_state_create.argtypes = [vp, vp, C.POINTER(vp), E]
        L.tgx_state_destroy.argtypes = [vp]
        L.tgx_state_destroy.restype = None
        L.tgx_update.argtypes = [vp, vp, C.POINTER(_Column), sz, E]
        L.tgx_merge.argtypes = [vp, vp, C.POINTER(vp), sz, E]
        L.tgx_finalize.argtypes = [vp, vp, C.POINTER(Result), sz, E]
        L.tgx_comm_create.argtypes = [C.POINTER(CommOps), C.POINTER(vp), E]
        L.tgx_comm_rccl_unique_id.argtypes = [vp, E]
        L.tgx_comm_create_rccl.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp), E]
        L.tgx_comm_adopt_rccl.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(vp), E]
        L.tgx_comm_destroy.argtypes = [vp]
        L.tgx_comm_destroy.restype = None
        L.tgx_allreduce.argtypes = [vp, vp, vp, E]
        L.tgx_state_sync.argtypes = [vp, E]
        L.tgx_state_reset.argtypes = [vp, vp, E]
        L.tgx_state_serialize.argtypes = [vp, vp, vp, sz, C.POINTER(sz), E]
        L.tgx_state_deserialize.argtypes = [vp, vp, sz, C.POINTER(vp), E]
        L.tgx_kll_quantile.argtypes = [vp, vp, sz, C.c_double, C.POINTER(C.c_double), E]
        L.tgx_kll_summary.argtypes = [vp, vp, sz, C.POINTER(u64), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(u64), C.POINTER(u64), E]
        L.tgx_kll_level_items.argtypes = [vp, vp, sz, u64, vp, u64, C.POINTER(u64), E]
        L.tgx_kll_relative_error_bound.argtypes = [C.c_uint32]
        L.tgx_kll_relative_error_bound.restype = C.c_double
        L.tgx_distinct_export.argtypes = [vp, vp, sz, C.c_uint32, C.POINTER(vp), C.POINTER(u64), E]
        L.tgx_distinct_import.argtypes = [vp, vp, sz, vp, u64, E]
        L.tgx_distinct_range_hint.argtypes = [vp, vp, sz, C.c_int64, C.c_int64, E]
        L.tgx_distinct_bitmap_view.argtypes = [vp, vp, sz, C.POINTER(C.c_int64), C.POINTER(u64), C.POINTER(vp), C.POINTER(vp), E]
        L.tgx_distinct_adopt_slices.argtypes = [vp, vp, sz, C.c_int64, vp, vp, C.c_uint32, u64, u64, E]
        L.tgx_distinct_record_bytes.argtypes = [vp, vp, sz]
        L.tgx_distinct_record_bytes.restype = sz
        L.tgx_profile_enable.argtypes = [vp, C.c_int32]
        L.tgx_profile_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(u64), C.POINTER(u64), E]
        L.tgx_profile_reset.argtypes = [vp]
        L.tgx_regex_validate.argtypes = [C.c_char_p, sz, C.c_uint32, E]
        L.tgx_regex_is_match.argtypes = [C.c_char_p, sz, C.c_uint32, C.c_char_p, sz, C.POINTER(C.c_int32), E]
        L.tgx_regex_match_group.argtypes = [C.POINTER(C.c_char_p), C.POINTER(sz), C.POINTER(C.c_uint32), sz, C.c_char_p, sz,
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_int32), E]
        L.tgx_regex_table_info.argtypes = [C.c_char_p, sz, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), E]
        L.tgx_cache_stats_get.argtypes = [C.POINTER(CacheStats)]
        L.tgx_state_pending.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.tgx_plan_set_joint_binning.argtypes = [vp, sz, C.POINTER(JointBinning), E]
        L.tgx_joint_range_get.argtypes = [vp, vp, sz, C.POINTER(JointRange), E]
        L.tgx_joint_counts.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), C.POINTER(u64), E]
        L.tgx_plan_set_temporal.argtypes = [vp, sz, C.POINTER(TemporalParams), E]
        L.tgx_temporal_get.argtypes = [vp, vp, sz, C.POINTER(TemporalCounts), E]
        L.tgx_plan_set_time_gap.argtypes = [vp, sz, C.POINTER(TimeGapParams), E]
        L.tgx_time_gap_get.argtypes = [vp, vp, sz, C.POINTER(TimeGapCounts), E]
        L.tgx_plan_set_value_rule.argtypes = [vp, sz, C.POINTER(ValueRuleParams), E]
        L.tgx_value_rule_get.argtypes = [vp, vp, sz, C.POINTER(ValueRuleCounts), E]
        L.tgx_plan_set_row_predicate.argtypes = [vp, sz, C.POINTER(RowPredicateParams), E]
        L.tgx_row_predicate_get.argtypes = [vp, vp, sz, C.POINTER(RowPredicateCounts), E]
        L.tgx_type_classes_get.argtypes = [vp, vp, sz, C.POINTER(TypeClassesCounts), E]
        L.tgx_host_type_class.argtypes = [C.c_char_p, u64]
        L.tgx_host_type_class.restype = C.c_int32
        L.tgx_host_string_leaf.argtypes = [C.c_int32, C.c_int32, C.c_uint32, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p,
                                           u64, C.POINTER(C.c_int)]
        L.tgx_plan_set_value_counts.argtypes = [vp, sz, C.POINTER(ValueCountsParams), E]
        L.tgx_value_counts_get.argtypes = [vp, vp, sz, C.POINTER(ValueCountsSummary), E]
        L.tgx_value_counts_entries.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64),
                                               C.POINTER(C.c_int32), E]
        L.tgx_plan_set_pair_counts.argtypes = [vp, sz, C.POINTER(PairCountsParams), E]
        L.tgx_pair_counts_get.argtypes = [vp, vp, sz, C.POINTER(PairCountsSummary), E]
        L.tgx_pair_range_get.argtypes = [vp, vp, sz, C.POINTER(PairRange), E]
        L.tgx_pair_counts_entries.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), E]
        L.tgx_plan_set_group_counts.argtypes = [vp, sz, C.POINTER(GroupCountsParams), E]
        L.tgx_group_counts_get.argtypes = [vp, vp, sz, C.POINTER(GroupCountsSummary), E]
        L.tgx_plan_set_group_sums.argtypes = [vp, sz, C.POINTER(GroupSumsParams), E]
        L.tgx_group_sums_get.argtypes = [vp, vp, sz, C.POINTER(GroupSumsSummary), E]
        L.tgx_group_sums_entries.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64),
                                             C.POINTER(C.c_int32), E]
        L.tgx_group_counts_entries.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64),
                                               C.POINTER(C.c_int32), E]
        L.tgx_plan_set_key_probe.argtypes = [vp, sz, C.POINTER(KeyProbeParams), E]
        L.tgx_plan_set_key_probe_counted.argtypes = [vp, sz, C.POINTER(KeyProbeParams), E]
        L.tgx_plan_set_key_probe_rows.argtypes = [vp, sz, E]
        L.tgx_key_probe_rows_get.argtypes = [vp, vp, sz, C.POINTER(vp), C.POINTER(u64), E]
        L.tgx_key_probe_pairs_get.argtypes = [vp, vp, sz, C.POINTER(KeyProbePairs), E]
        L.tgx_key_probe_set_parent.argtypes = [vp, vp, sz, vp, u64, E]
        L.tgx_key_probe_get.argtypes = [vp, vp, sz, C.POINTER(KeyProbeSummary), E]
        L.tgx_key_probe_entries.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), E]
        L.tgx_plan_set_key_probe_strings.argtypes = [vp, sz, C.POINTER(KeyProbeStringsParams), E]
        L.tgx_plan_set_key_probe_strings_counted.argtypes = [vp, sz, C.POINTER(KeyProbeStringsParams), E]
        L.tgx_plan_set_key_probe_rows_strings.argtypes = [vp, sz, E]
        L.tgx_key_probe_strings_get.argtypes = [vp, vp, sz, C.POINTER(KeyProbeStrings), E]
        L.tgx_key_probe_entries_bytes.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64), E]
        L.tgx_plan_set_key_probe_tuples.argtypes = [vp, sz, C.POINTER(KeyProbeParams), E]
        L.tgx_plan_set_key_probe_tuples_counted.argtypes = [vp, sz, C.POINTER(KeyProbeParams), E]
        L.tgx_plan_set_key_probe_rows_tuples.argtypes = [vp, sz, E]
        L.tgx_key_probe_tuples_get.argtypes = [vp, vp, sz, C.POINTER(KeyProbeTuples), E]
        L.tgx_key_probe_entries_tuples.argtypes = [vp, vp, sz, vp, u64, C.POINTER(u64), E]
        L.tgx_plan_set_histogram_edges.argtypes = [vp, sz, C.POINTER(C.c_double), C.c_uint32, E]
        L.tgx_histogram_range_get.argtypes = [vp, vp, sz, C.POINTER(HistogramRange), E]
        L.tgx_histogram_counts.argtypes = [vp, vp, sz, vp, sz, C.POINTER(u64), C.POINTER(u64), E]
        _LIB = L
    return _LIB


class CacheStats(C.Structure):
    """tgx_cache_stats (include/tgx.h)"""
    _fields_ = [("device_cached_bytes", C.c_uint64), ("device_cached_blocks", C.c_uint64), ("device_hits", C.c_uint64),
                ("device_misses", C.c_uint64), ("pinned_cached_bytes", C.c_uint64), ("pinned_hits", C.c_uint64),
                ("pinned_misses", C.c_uint64)]


def cache_stats():
    """tgx_cache_stats_get: what the library's cache of device / pinned blocks holds and has served"""
    out = CacheStats()
    rc = lib().tgx_cache_stats_get(C.byref(out))
    if rc != 0:
        raise TgxError(rc, "tgx_cache_stats_get")
    return out


def trim():
    """tgx_trim: the cached blocks of destroyed states go back to the driver"""
    rc = lib().tgx_trim()
    if rc != 0:
        raise TgxError(rc, "tgx_trim")


def _check(status, err):
    if status != 0:
        raise TgxError(status, err.msg.decode("utf-8", "replace"))


_INITED = False


OPT_NO_COALESCE = 1


def init(device_id=-1, distinct_capacity_hint=0, flags=0):
    """tgx_init: selects the gfx950 device. Raises TgxError(TGX_NO_DEVICE) when there is none.
    flags: OPT_NO_COALESCE = every batch is launched as it arrives"""
    global _INITED
    err = _Error()
    opts = _Options(device_id, flags, distinct_capacity_hint)
    _check(lib().tgx_init(C.byref(opts), C.byref(err)), err)
    _INITED = True


def host_type_class(value):
    """tgx_host_type_class: the class (TYPE_CLASS_*) the lexer of TYPE_CLASSES gives the bytes of `value` (bytes, or a
    str taken as UTF-8) -- the function the kernels compile, run on the host; needs no device"""
    b = value.encode("utf-8") if isinstance(value, str) else bytes(value)
    return lib().tgx_host_type_class(b, len(b))


def host_string_leaf(kind, value, op=0, flags=0, lit_i=0, pattern=b"", align=0):
    """tgx_host_string_leaf: one string leaf of ROW_PREDICATE (PRED_STR_CMP .. PRED_STR_BLANK) on one non-NULL value
    (bytes, or a str taken as UTF-8), through the functions the kernel compiles, run on the host: True or False.
    `pattern`: STR_CMP's literal / STR_LIKE's pattern; `align` (0 .. 3): where the value's first byte lies in its 32-bit
    word.  TgxError (TGX_INVALID_ARGUMENT) for a leaf the setter refuses.  Needs no device"""
    v = value.encode("utf-8") if isinstance(value, str) else bytes(value)
    pat = pattern.encode("utf-8") if isinstance(pattern, str) else bytes(pattern)
    raw = C.create_string_buffer(len(v) + 8)
    base = C.addressof(raw)
    at = base + ((align - base) & 3)
    C.memmove(at, v, len(v))
    out = C.c_int(0)
    rc = lib().tgx_host_string_leaf(kind, op, flags, lit_i, pat, len(pat), at, len(v), C.byref(out))
    if rc != 0:
        raise TgxError(rc, "tgx_host_string_leaf refuses the leaf (kind %d, op %d, flags 0x%x)" % (kind, op, flags))
    return bool(out.value)


def _ptr_of(buf):
    """address of a numpy array / torch tensor / int / None, plus whether it is device memory"""
    if buf is None:
        return None, None
    if isinstance(buf, int):
        return buf, None
    if hasattr(buf, "data_ptr"):  # torch tensor
        return buf.data_ptr(), buf.is_cuda
    if hasattr(buf, "ctypes"):  # numpy
        return buf.ctypes.data, False
    raise TypeError("unsupported buffer type %r" % type(buf))


class Column:
    """A tgx_column view. Keeps the Python buffers alive while the view exists."""

    def __init__(self, type, length, values=None, validity=None, offsets=None, data=None, offset=0,
                 null_count=-1, mem=None, dictionary=None, variadic=None):
        self._keep = (values, validity, offsets, data, dictionary, variadic)
        c = _Column()
        c.type = type
        c.length = length
        c.offset = offset
        c.null_count = null_count
        spaces = set()
        for name, buf in (("values", values), ("validity", validity), ("offsets", offsets), ("data", data)):
            p, is_dev = _ptr_of(buf)
            setattr(c, name, p)
            if is_dev is not None:
                spaces.add(bool(is_dev))
        if variadic is not None:
            # Utf8View data buffers: a host array of their pointers (+ sizes, needed to stage HOST buffers)
            ptrs = (C.c_void_p * max(1, len(variadic)))()
            sizes = (C.c_int64 * max(1, len(variadic)))()
            for k, buf in enumerate(variadic):
                pk, is_dev = _ptr_of(buf)
                ptrs[k] = pk
                sizes[k] = int(buf.nbytes) if hasattr(buf, "nbytes") else int(buf.numel() * buf.element_size())
                if is_dev is not None:
                    spaces.add(bool(is_dev))
            c.variadic = C.cast(ptrs, C.POINTER(C.c_void_p))
            c.variadic_sizes = C.cast(sizes, C.POINTER(C.c_int64))
            c.n_variadic = len(variadic)
            self._keep += (ptrs, sizes)
        if mem is None:
            if len(spaces) > 1:
                raise ValueError("a column's buffers must all live in one memory space")
            mem = MEM_DEVICE if (spaces and spaces.pop()) else MEM_HOST
        c.mem = mem
        if dictionary is not None:
            c.dictionary = C.pointer(dictionary.c)
        self.c = c

    def sliced(self, offset, length):
        """Arrow's Array::slice: the same buffers viewed from `offset` (relative to this view) for `length` rows"""
        import copy

        if offset < 0 or length < 0 or offset + length > self.c.length:
            raise ValueError("slice [%d, %d) outside a column of %d rows" % (offset, offset + length, self.c.length))
        out = copy.copy(self)  # shares the keep-alive references of the buffers
        c = _Column()
        C.memmove(C.byref(c), C.byref(self.c), C.sizeof(_Column))
        c.offset = self.c.offset + offset
        c.length = length
        c.null_count = -1
        out.c = c
        return out

    @staticmethod
    def int64(values, validity=None, length=None, offset=0):
        n = (len(values) - offset) if length is None else length
        return Column(INT64, n, values=values, validity=validity, offset=offset)

    @staticmethod
    def float64(values, validity=None, length=None, offset=0):
        n = (len(values) - offset) if length is None else length
        return Column(FLOAT64, n, values=values, validity=validity, offset=offset)

    @staticmethod
    def int32(values, validity=None, length=None, offset=0):
        """Int32 / Date32 / Time32: widened to Int64 on the device"""
        n = (len(values) - offset) if length is None else length
        return Column(INT32, n, values=values, validity=validity, offset=offset)

    @staticmethod
    def float32(values, validity=None, length=None, offset=0):
        """Float32: widened to Float64 on the device"""
        n = (len(values) - offset) if length is None else length
        return Column(FLOAT32, n, values=values, validity=validity, offset=offset)

    @staticmethod
    def narrow(type_id, values, validity=None, length=None, offset=0):
        """Int8 / Int16 / UInt8 / UInt16 / UInt32 (widened to Int64 on the device) and UInt64 (read in place, COUNT /
        DISTINCT only): `values` holds one element per row"""
        n = (len(values) - offset) if length is None else length
        return Column(type_id, n, values=values, validity=validity, offset=offset)

    @staticmethod
    def boolean(bits, length, validity=None, offset=0):
        """Boolean: `bits` is the bit-packed values buffer (uint8, bit `offset + i` = row i); COUNT / DISTINCT only"""
        return Column(BOOL, length, values=bits, validity=validity, offset=offset)

    @staticmethod
    def utf8(offsets, data, validity=None, length=None, offset=0):
        n = (len(offsets) - 1 - offset) if length is None else length
        return Column(UTF8, n, offsets=offsets, data=data, validity=validity, offset=offset)

    @staticmethod
    def large_utf8(offsets, data, validity=None, length=None, offset=0):
        n = (len(offsets) - 1 - offset) if length is None else length
        return Column(LARGE_UTF8, n, offsets=offsets, data=data, validity=validity, offset=offset)

    @staticmethod
    def utf8_view(views, buffers, validity=None, length=None, offset=0):
        """Utf8View: `views` = 16 bytes per row (uint8 buffer of 16 * rows bytes), `buffers` = list of data buffers"""
        n = (len(views) // 16 - offset) if length is None else length
        return Column(UTF8_VIEW, n, values=views, validity=validity, offset=offset, variadic=list(buffers))

    @staticmethod
    def dict32_utf8(indices, dictionary, validity=None, length=None, offset=0):
        """Dictionary<Int32, Utf8>: int32 `indices` into `dictionary` (a utf8 / large_utf8 Column)."""
        n = (len(indices) - offset) if length is None else length
        return Column(DICT32_UTF8, n, values=indices, validity=validity, offset=offset, dictionary=dictionary)

    @staticmethod
    def from_arrow(arr):
        """pyarrow Array (Int64 / Float64 / Utf8 / LargeUtf8 / Dictionary<Int32, Utf8>, host memory) -> Column
        view of its buffers."""
        import numpy as np
        import pyarrow as pa

        bufs = arr.buffers()

        def view(b, dtype):
            return None if b is None else np.frombuffer(b, dtype=dtype)

        validity = view(bufs[0], np.uint8) if arr.null_count else None
        if pa.types.is_int64(arr.type):
            return Column(INT64, len(arr), values=view(bufs[1], np.int64), validity=validity, offset=arr.offset,
                          null_count=arr.null_count)
        if pa.types.is_float64(arr.type):
            return Column(FLOAT64, len(arr), values=view(bufs[1], np.float64), validity=validity,
                          offset=arr.offset, null_count=arr.null_count)
        t = arr.type
        if pa.types.is_int32(t) or pa.types.is_date32(t) or pa.types.is_time32(t):
            return Column(INT32, len(arr), values=view(bufs[1], np.int32), validity=validity, offset=arr.offset,
                          null_count=arr.null_count)
        if pa.types.is_float32(t):
            return Column(FLOAT32, len(arr), values=view(bufs[1], np.float32), validity=validity, offset=arr.offset,
                          null_count=arr.null_count)
        for is_t, type_id, dtype in ((pa.types.is_int8, INT8, np.int8), (pa.types.is_int16, INT16, np.int16),
                                     (pa.types.is_uint8, UINT8, np.uint8), (pa.types.is_uint16, UINT16, np.uint16),
                                     (pa.types.is_uint32, UINT32, np.uint32), (pa.types.is_uint64, UINT64, np.uint64)):
            if is_t(t):
                return Column(type_id, len(arr), values=view(bufs[1], dtype), validity=validity, offset=arr.offset,
                              null_count=arr.null_count)
        if pa.types.is_boolean(t):
            return Column(BOOL, len(arr), values=view(bufs[1], np.uint8), validity=validity, offset=arr.offset,
                          null_count=arr.null_count)
        if pa.types.is_timestamp(t) or pa.types.is_date64(t) or pa.types.is_time64(t) or pa.types.is_duration(t):
            # Int64-shaped: the checks see the stored integer (microseconds, milliseconds, ...)
            return Column(INT64, len(arr), values=view(bufs[1], np.int64), validity=validity, offset=arr.offset,
                          null_count=arr.null_count)
        if pa.types.is_string(arr.type):
            data = view(bufs[2], np.uint8) if bufs[2] is not None and bufs[2].size else np.zeros(1, np.uint8)
            return Column(UTF8, len(arr), offsets=view(bufs[1], np.int32), data=data, validity=validity,
                          offset=arr.offset, null_count=arr.null_count)
        if pa.types.is_large_string(arr.type):
            data = view(bufs[2], np.uint8) if bufs[2] is not None and bufs[2].size else np.zeros(1, np.uint8)
            return Column(LARGE_UTF8, len(arr), offsets=view(bufs[1], np.int64), data=data, validity=validity,
                          offset=arr.offset, null_count=arr.null_count)
        if hasattr(pa.types, "is_string_view") and pa.types.is_string_view(arr.type):
            return Column(UTF8_VIEW, len(arr), values=view(bufs[1], np.uint8), validity=validity, offset=arr.offset,
                          null_count=arr.null_count, variadic=[view(b, np.uint8) for b in bufs[2:]])
        if (pa.types.is_dictionary(arr.type) and pa.types.is_int32(arr.type.index_type)
                and (pa.types.is_string(arr.type.value_type) or pa.types.is_large_string(arr.type.value_type))):
            return Column(DICT32_UTF8, len(arr), values=view(bufs[1], np.int32), validity=validity,
                          offset=arr.offset, null_count=arr.null_count,
                          dictionary=Column.from_arrow(arr.dictionary))
        # Binary / LargeBinary / BinaryView have the string layouts: COUNT and COUNT(DISTINCT) compare bytes, which is what
        # the reference's SQL does with them (a pattern or LENGTH check on such a column is the caller's to refuse)
        if pa.types.is_binary(t) or pa.types.is_large_binary(t):
            data = view(bufs[2], np.uint8) if bufs[2] is not None and bufs[2].size else np.zeros(1, np.uint8)
            return Column(LARGE_UTF8 if pa.types.is_large_binary(t) else UTF8, len(arr),
                          offsets=view(bufs[1], np.int64 if pa.types.is_large_binary(t) else np.int32), data=data,
                          validity=validity, offset=arr.offset, null_count=arr.null_count)
        if hasattr(pa.types, "is_binary_view") and pa.types.is_binary_view(t):
            return Column(UTF8_VIEW, len(arr), values=view(bufs[1], np.uint8), validity=validity, offset=arr.offset,
                          null_count=arr.null_count, variadic=[view(b, np.uint8) for b in bufs[2:]])
        # fixed-width values of w bytes (FixedSizeBinary(w), Decimal128 = 16, Decimal256 = 32): equality of values is
        # equality of bytes (one precision / scale per column), so COUNT(DISTINCT) sees them as w-byte strings -- the
        # offsets 0, w, 2 w, ... are made here (4 bytes per row of host work; the values are not copied)
        width = t.byte_width if (pa.types.is_fixed_size_binary(t) or pa.types.is_decimal(t)) else 0
        if width:
            n = len(arr)
            offs = (np.arange(n + 1, dtype=np.int64) + arr.offset) * width
            if offs[-1] < 2**31:
                col = Column(UTF8, n, offsets=offs.astype(np.int32), data=view(bufs[1], np.uint8), validity=None, offset=0,
                             null_count=arr.null_count)
            else:
                col = Column(LARGE_UTF8, n, offsets=offs, data=view(bufs[1], np.uint8), validity=None, offset=0,
                             null_count=arr.null_count)
            if validity is not None:  # (the validity bitmap keeps the array's own offset: re-aligned to row 0)
                mask = np.unpackbits(validity, bitorder="little")[arr.offset:arr.offset + n]
                v = np.concatenate([np.packbits(mask, bitorder="little"), np.zeros(8, np.uint8)])
                col = Column(col.c.type, n, offsets=col._keep[2], data=col._keep[3], validity=v, offset=0,
                             null_count=arr.null_count)
            return col
        raise TgxError(2, "unsupported Arrow type %s" % arr.type)

    @staticmethod
    def validity_only(arr):
        """ANY pyarrow Array as a column for checks that read no values (completeness / COUNT: the validity bitmap and
        the length are all they need -- `SELECT COUNT(*), COUNT(c)` takes every column type, completeness.rs:158-163)"""
        import numpy as np

        bufs = arr.buffers()
        validity = np.frombuffer(bufs[0], dtype=np.uint8) if (arr.null_count and bufs and bufs[0] is not None) else None
        if validity is None and arr.null_count:  # NullArray: no bitmap, every row NULL
            return Column(INT64, len(arr), values=None, validity=np.zeros((len(arr) + 7) // 8 + 8, np.uint8), null_count=len(arr))
        return Column(INT64, len(arr), values=None, validity=validity, offset=arr.offset, null_count=arr.null_count)


def spec(kind, column, column2=-1, flags=0, pattern=None, kll_k=0, columns=None, length_min=0, length_max=None):
    """columns=[a, b, ...]: DISTINCT over the tuple of those columns (COUNT(DISTINCT (a, b))), or a KEY_PROBE whose key is
    that tuple (Plan.set_key_probe_tuples), or the 1 .. 8 columns a ROW_PREDICATE's leaves name by position, or -- with
    column2 left at -1 -- the 2 .. 8 columns a GROUP_COUNTS / GROUP_SUMS spec groups by, `column` staying its value column
    (the entries' keys are then term_amd.group_key's encoded tuples);
    length_min / length_max (None = unbounded): LENGTH bounds in characters"""
    pat = pattern.encode("utf-8") if isinstance(pattern, str) else pattern
    s = CheckSpec(kind, column, column2, flags, pat, len(pat) if pat else 0, kll_k, 0)
    s.length_min = length_min
    s.length_max = (1 << 64) - 1 if length_max is None else length_max
    if columns is not None and (len(columns) >= 2 or (kind == ROW_PREDICATE and columns)):
        arr = (C.c_int32 * len(columns))(*columns)
        s.columns = C.cast(arr, C.POINTER(C.c_int32))
        s.n_columns = len(columns)
        s._keep_columns = arr
        if not (kind in (GROUP_COUNTS, GROUP_SUMS) and column2 < 0):
            s.column = columns[0]
    return s


# ---- the cross-rank step: transports and tgx_allreduce (include/tgx.h) ----------------------------------------
_ALLTOALL_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_ALLTOALLV_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64),
                            C.c_size_t, C.c_void_p)
_ALLGATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class CommOps(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int32), ("world", C.c_int32), ("device_buffers", C.c_int32),
                ("reserved", C.c_int32), ("alltoall", _ALLTOALL_FN), ("alltoallv", _ALLTOALLV_FN),
                ("allgather", _ALLGATHER_FN)]


RCCL_UNIQUE_ID_BYTES = 128


class Comm:
    """tgx_comm: the transport tgx_allreduce runs over."""

    def __init__(self, handle, rank, world, keep=None):
        self.h, self.rank, self.world, self._keep = handle, rank, world, keep

    def __del__(self):
        if getattr(self, "h", None):
            lib().tgx_comm_destroy(self.h)
            self.h = None

    @staticmethod
    def rccl_unique_id():
        buf = (C.c_uint8 * RCCL_UNIQUE_ID_BYTES)()
        err = _Error()
        _check(lib().tgx_comm_rccl_unique_id(buf, C.byref(err)), err)
        return bytes(buf)

    @staticmethod
    def rccl(unique_id, rank, world):
        """RCCL over xGMI: the library calls ncclCommInitRank itself (collective: every rank must call)"""
        buf = (C.c_uint8 * RCCL_UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        h = C.c_void_p()
        err = _Error()
        _check(lib().tgx_comm_create_rccl(buf, rank, world, C.byref(h), C.byref(err)), err)
        return Comm(h, rank, world)

    @staticmethod
    def custom(rank, world, alltoall, alltoallv, allgather, device_buffers=False):
        """any transport: three Python callables over raw pointers (see tgx_comm_ops in include/tgx.h); they return
        nothing and raise on failure"""
        def guard(fn):
            def wrapped(*a):
                try:
                    fn(*a[1:])  # drop ctx
                    return 0
                except Exception:  # noqa: BLE001 -- must not unwind through the C frames
                    import traceback

                    traceback.print_exc()
                    return 1
            return wrapped

        ops = CommOps()
        ops.rank, ops.world, ops.device_buffers = rank, world, 1 if device_buffers else 0
        cbs = (_ALLTOALL_FN(guard(alltoall)), _ALLTOALLV_FN(guard(alltoallv)), _ALLGATHER_FN(guard(allgather)))
        ops.alltoall, ops.alltoallv, ops.allgather = cbs
        h = C.c_void_p()
        err = _Error()
        _check(lib().tgx_comm_create(C.byref(ops), C.byref(h), C.byref(err)), err)
        return Comm(h, rank, world, keep=cbs)  # the C side keeps the function pointers: keep the thunks alive


def blob_fingerprint_key(blob):
    """the fingerprint key a state blob was made under, or None when it holds no string / tuple keys"""
    out, keyed = (C.c_uint8 * 16)(), C.c_int32()
    rc = lib().tgx_blob_fingerprint_key(bytes(blob), len(blob), out, C.byref(keyed))
    if rc != 0:
        raise TgxError(rc, "not a tgx state blob of this version")
    return bytes(out) if keyed.value else None


class Plan:
    def __init__(self, specs, fingerprint_key=None):
        """`fingerprint_key`: 16 bytes -- the key of the plan's string / tuple fingerprints (tgx_plan_set_fingerprint_key);
        None: the one tgx_plan_create drew from the operating system"""
        self._specs = list(specs)
        arr = (CheckSpec * max(1, len(self._specs)))(*self._specs)
        h = C.c_void_p()
        err = _Error()
        _check(lib().tgx_plan_create(arr, len(self._specs), C.byref(h), C.byref(err)), err)
        self.h = h
        self.n = len(self._specs)
        self.histogram_buckets = {}  # spec index -> buckets, once set_histogram_edges was called
        self.pair_sides = {}  # spec index -> the two sides' modes, once set_pair_counts was called
        if fingerprint_key is not None:
            self.set_fingerprint_key(fingerprint_key)

    def set_fingerprint_key(self, key):
        key = bytes(key)
        if len(key) != 16:
            raise ValueError("a fingerprint key is 16 bytes")
        err = _Error()
        _check(lib().tgx_plan_set_fingerprint_key(self.h, key, C.byref(err)), err)

    def set_joint_binning(self, spec_index, x_origin, x_width, y_origin, y_width, bins):
        """tgx_plan_set_joint_binning: puts a JOINT_BINS spec into its count phase (before the plan's first state)"""
        b = JointBinning(x_origin, x_width, y_origin, y_width, bins, 0)
        err = _Error()
        _check(lib().tgx_plan_set_joint_binning(self.h, spec_index, C.byref(b), C.byref(err)), err)

    def set_histogram_edges(self, spec_index, edges):
        """tgx_plan_set_histogram_edges: puts a HISTOGRAM spec into its count phase (before the plan's first state);
        `edges` are the buckets + 1 edges, lowest first"""
        edges = [float(e) for e in edges]
        if not edges:
            raise ValueError("a histogram needs at least two edges")
        buckets = len(edges) - 1
        arr = (C.c_double * len(edges))(*edges)
        err = _Error()
        _check(lib().tgx_plan_set_histogram_edges(self.h, spec_index, arr, buckets, C.byref(err)), err)
        self.histogram_buckets[spec_index] = buckets

    def set_temporal(self, spec_index, mode, flags=0, delta=0, ticks_per_second=0, tod_lo=0, tod_hi=0,
                     lo=-(1 << 63), hi=(1 << 63) - 1):
        """tgx_plan_set_temporal: the mode and parameters of a TEMPORAL spec (before the plan's first state)"""
        p = TemporalParams(mode, flags, delta, ticks_per_second, tod_lo, tod_hi, lo, hi)
        err = _Error()
        _check(lib().tgx_plan_set_temporal(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_time_gap(self, spec_index, max_gap, flags=0):
        """tgx_plan_set_time_gap: the threshold of a TIME_GAP spec, in the column's ticks (before the plan's first state)"""
        p = TimeGapParams(max_gap, flags)
        err = _Error()
        _check(lib().tgx_plan_set_time_gap(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_value_rule(self, spec_index, mode, flags=0, lo_i=0, hi_i=0, lo_f=0.0, hi_f=0.0):
        """tgx_plan_set_value_rule: the rule of a VALUE_RULE spec (before the plan's first state)"""
        p = ValueRuleParams(mode, flags, lo_i, hi_i, lo_f, hi_f)
        err = _Error()
        _check(lib().tgx_plan_set_value_rule(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_row_predicate(self, spec_index, leaves, program, literals=b"", n_leaves=None, n_ops=None,
                          n_literal_bytes=None):
        """tgx_plan_set_row_predicate: the predicate of a ROW_PREDICATE spec (before the plan's first state).  `leaves`:
        dicts with the fields of tgx_row_predicate_leaf (those left out are 0); `program`: (code, arg) pairs or packed
        ints; `literals`: the pool's bytes.  The n_* arguments override the counts (for a call that is to be refused)."""
        p = RowPredicateParams()
        for j, leaf in enumerate(list(leaves)[:PRED_MAX_LEAVES]):
            for k, v in leaf.items():
                setattr(p.leaves[j], k, v)
        for k, op in enumerate(list(program)[:PRED_MAX_OPS]):
            p.program[k] = op if isinstance(op, int) else (op[0] | (op[1] << 8))
        literals = bytes(literals)
        for k, b in enumerate(literals[:PRED_MAX_LITERAL_BYTES]):
            p.literals[k] = b
        p.n_leaves = len(leaves) if n_leaves is None else n_leaves
        p.n_ops = len(program) if n_ops is None else n_ops
        p.n_literal_bytes = len(literals) if n_literal_bytes is None else n_literal_bytes
        err = _Error()
        _check(lib().tgx_plan_set_row_predicate(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_value_counts(self, spec_index, max_distinct=10000, max_value_bytes=256):
        """tgx_plan_set_value_counts: the bounds of a VALUE_COUNTS spec (before the plan's first state)"""
        p = ValueCountsParams(max_distinct, max_value_bytes)
        err = _Error()
        _check(lib().tgx_plan_set_value_counts(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_group_counts(self, spec_index, max_groups=10000, max_value_bytes=256):
        """tgx_plan_set_group_counts: the bounds of a GROUP_COUNTS spec (before the plan's first state)"""
        p = GroupCountsParams(max_groups, max_value_bytes)
        err = _Error()
        _check(lib().tgx_plan_set_group_counts(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_group_sums(self, spec_index, max_groups=10000, max_value_bytes=256):
        """tgx_plan_set_group_sums: the bounds of a GROUP_SUMS spec (before the plan's first state)"""
        p = GroupSumsParams(max_groups, max_value_bytes)
        err = _Error()
        _check(lib().tgx_plan_set_group_sums(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_key_probe(self, spec_index, max_missing_keys=10000, reserved=0):
        """tgx_plan_set_key_probe: the bound of a KEY_PROBE spec (before the plan's first state)"""
        p = KeyProbeParams(max_missing_keys, reserved)
        err = _Error()
        _check(lib().tgx_plan_set_key_probe(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_key_probe_counted(self, spec_index, max_missing_keys=10000, reserved=0):
        """tgx_plan_set_key_probe_counted: the same bound, and the spec's parent set keeps the parent's multiplicities
        (State.key_probe_pairs).  A spec takes one of the two calls"""
        p = KeyProbeParams(max_missing_keys, reserved)
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_counted(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_key_probe_strings(self, spec_index, max_missing_keys=10000, max_value_bytes=256):
        """tgx_plan_set_key_probe_strings: the spec probes STRING keys against a set of fingerprints
        (State.key_probe_strings); a missing key of up to max_value_bytes bytes keeps its bytes.  A spec takes one of
        the six set_key_probe* calls"""
        p = KeyProbeStringsParams(max_missing_keys, max_value_bytes)
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_strings(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_key_probe_strings_counted(self, spec_index, max_missing_keys=10000, max_value_bytes=256):
        """tgx_plan_set_key_probe_strings_counted: a strings spec whose set keeps the parent's multiplicities
        (State.key_probe_strings and State.key_probe_pairs read it)"""
        p = KeyProbeStringsParams(max_missing_keys, max_value_bytes)
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_strings_counted(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_key_probe_rows_strings(self, spec_index):
        """tgx_plan_set_key_probe_rows_strings: the spec gathers its STRING column as 32-byte {hash_a, hash_b, count,
        0} records (State.key_probe_rows; State.key_probe_rows_records copies them to the host): the parent side of a
        counted strings probe"""
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_rows_strings(self.h, spec_index, C.byref(err)), err)

    def set_key_probe_tuples(self, spec_index, max_missing_keys=10000, reserved=0):
        """tgx_plan_set_key_probe_tuples: a spec with a column list (spec(KEY_PROBE, 0, columns=[..])) probes the TUPLE of
        its columns against a set of tuple fingerprints (State.key_probe_tuples).  A spec takes one of the nine
        set_key_probe* calls"""
        p = KeyProbeParams(max_missing_keys, reserved)
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_tuples(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_key_probe_tuples_counted(self, spec_index, max_missing_keys=10000, reserved=0):
        """tgx_plan_set_key_probe_tuples_counted: a tuples spec whose set keeps the parent's multiplicities
        (State.key_probe_tuples and State.key_probe_pairs read it)"""
        p = KeyProbeParams(max_missing_keys, reserved)
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_tuples_counted(self.h, spec_index, C.byref(p), C.byref(err)), err)

    def set_key_probe_rows_tuples(self, spec_index):
        """tgx_plan_set_key_probe_rows_tuples: the spec gathers the all-valid tuples of its columns as 32-byte
        {hash_a, hash_b, 1, 0} records (State.key_probe_rows): the parent side of a tuples probe"""
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_rows_tuples(self.h, spec_index, C.byref(err)), err)

    def set_key_probe_rows(self, spec_index):
        """tgx_plan_set_key_probe_rows: the spec gathers its column's non-NULL keys as {key, 1} records
        (State.key_probe_rows): the parent side of a counted probe when the parent's keys repeat"""
        err = _Error()
        _check(lib().tgx_plan_set_key_probe_rows(self.h, spec_index, C.byref(err)), err)

    def set_pair_counts(self, spec_index, x=None, y=None, max_pairs=10000, max_value_bytes=256):
        """tgx_plan_set_pair_counts: the bounds and the sides of a PAIR_COUNTS spec (before the plan's first state).  A
        side is None or "value" (a string column: PAIR_SIDE_VALUE), "range" (a numeric column: the spec is in its range
        phase) or a binning (origin, width, bins) of a numeric column"""
        def side(s):
            if s is None or s == "value":
                return PairSide(PAIR_SIDE_VALUE, 0, 0.0, 0.0)
            if s == "range":
                return PairSide(PAIR_SIDE_RANGE, 0, 0.0, 0.0)
            if isinstance(s, PairSide):
                return s
            origin, width, bins = s
            return PairSide(PAIR_SIDE_BINNED, bins, origin, width)
        sx, sy = side(x), side(y)
        p = PairCountsParams(max_pairs, max_value_bytes, sx, sy)
        err = _Error()
        _check(lib().tgx_plan_set_pair_counts(self.h, spec_index, C.byref(p), C.byref(err)), err)
        self.pair_sides[spec_index] = (sx.mode, sy.mode)

    def fingerprint_key(self):
        out = (C.c_uint8 * 16)()
        lib().tgx_plan_get_fingerprint_key(self.h, out)
        return bytes(out)

    def __del__(self):
        if getattr(self, "h", None):
            lib().tgx_plan_destroy(self.h)
            self.h = None


class State:
    def __init__(self, plan, stream=None, _handle=None):
        self.plan = plan
        if _handle is not None:
            self.h = _handle
            return
        h = C.c_void_p()
        err = _Error()
        _check(lib().tgx_state_create(plan.h, stream, C.byref(h), C.byref(err)), err)
        self.h = h

    def close(self):
        """tgx_state_destroy now (not when the garbage collector gets to it)"""
        if getattr(self, "h", None):
            lib().tgx_state_destroy(self.h)
            self.h = None
        self._keep = None

    def __del__(self):
        self.close()

    def update(self, columns):
        cols = list(columns)
        arr = (_Column * max(1, len(cols)))(*[c.c if c is not None else _Column() for c in cols])
        err = _Error()
        _check(lib().tgx_update(self.plan.h, self.h, arr, len(cols), C.byref(err)), err)
        # DEVICE buffers must outlive the asynchronous kernels of EVERY batch queued since the last finalize / sync
        # (include/tgx.h): a streamed `update(b1); del b1; update(b2)` would otherwise hand b1's memory back to the
        # allocator while the scan of b1 is still reading it
        # HOST buffers are borrowed only until tgx_update returns: holding them would pin a whole streamed table in
        # host memory until finalize
        # (TGX_MEM_HOST_RETAINED buffers are promised to stay as they are until the next flushing call: held likewise)
        held = [c for c in cols if c is not None and (c.c.mem != 0 or (c.c.dictionary and c.c.dictionary.contents.mem != 0))]
        if held:
            if getattr(self, "_keep", None) is None:
                self._keep = []
            self._keep.append(held)

    def pending(self):
        """(batches, rows) that tgx_update has only noted so far: the last ones fed"""
        b, r = C.c_uint64(), C.c_uint64()
        lib().tgx_state_pending(self.h, C.byref(b), C.byref(r))
        return b.value, r.value

    def finalize(self):
        res = (Result * max(1, self.plan.n))()
        err = _Error()
        _check(lib().tgx_finalize(self.plan.h, self.h, res, self.plan.n, C.byref(err)), err)
        self._keep = None
        return list(res)[: self.plan.n]

    def sync(self):
        err = _Error()
        _check(lib().tgx_state_sync(self.h, C.byref(err)), err)
        self._keep = None

    def reset(self):
        err = _Error()
        _check(lib().tgx_state_reset(self.plan.h, self.h, C.byref(err)), err)  # waits for the stream
        self._keep = None

    def allreduce(self, comm):
        """tgx_allreduce: this rank's state becomes the state of the whole table (collective)"""
        err = _Error()
        _check(lib().tgx_allreduce(self.plan.h, self.h, comm.h, C.byref(err)), err)
        self._keep = None  # the step ends with the stream drained

    def merge(self, others):
        hs = (C.c_void_p * max(1, len(others)))(*[o.h for o in others])
        err = _Error()
        _check(lib().tgx_merge(self.plan.h, self.h, hs, len(others), C.byref(err)), err)

    def serialize(self):
        """packed partial state.  One library call when the blob fits the buffer kept from the last call (every call
        reads the accumulators back from the device), a second one with the reported size otherwise."""
        n = C.c_size_t()
        err = _Error()
        buf = getattr(self, "_ser_buf", None)
        if buf is None:
            buf = self._ser_buf = (C.c_uint8 * 8192)()
        rc = lib().tgx_state_serialize(self.plan.h, self.h, buf, len(buf), C.byref(n), C.byref(err))
        if rc != 0 and n.value > len(buf):  # "buffer too small": the needed size has been reported
            buf = self._ser_buf = (C.c_uint8 * (n.value + n.value // 4))()
            err = _Error()
            rc = lib().tgx_state_serialize(self.plan.h, self.h, buf, len(buf), C.byref(n), C.byref(err))
        _check(rc, err)
        return bytes(memoryview(buf)[: n.value])

    @staticmethod
    def deserialize(plan, blob):
        h = C.c_void_p()
        err = _Error()
        buf = (C.c_uint8 * max(1, len(blob))).from_buffer_copy(blob) if blob else (C.c_uint8 * 1)()
        _check(lib().tgx_state_deserialize(plan.h, buf, len(blob), C.byref(h), C.byref(err)), err)
        return State(plan, _handle=h)

    # KLL
    def kll_quantile(self, spec_index, phi):
        out = C.c_double()
        err = _Error()
        _check(lib().tgx_kll_quantile(self.plan.h, self.h, spec_index, phi, C.byref(out), C.byref(err)), err)
        return out.value

    def kll_summary(self, spec_index):
        n, lv, rt = C.c_uint64(), C.c_uint64(), C.c_uint64()
        mn, mx = C.c_double(), C.c_double()
        err = _Error()
        _check(lib().tgx_kll_summary(self.plan.h, self.h, spec_index, C.byref(n), C.byref(mn), C.byref(mx),
                                     C.byref(lv), C.byref(rt), C.byref(err)), err)
        return dict(n=n.value, min=mn.value, max=mx.value, num_levels=lv.value, num_retained=rt.value)

    def kll_level_items(self, spec_index, level):
        import numpy as np

        cnt = C.c_uint64()
        err = _Error()
        _check(lib().tgx_kll_level_items(self.plan.h, self.h, spec_index, level, None, 0, C.byref(cnt),
                                         C.byref(err)), err)
        out = np.zeros(max(1, cnt.value), dtype=np.float64)
        _check(lib().tgx_kll_level_items(self.plan.h, self.h, spec_index, level, out.ctypes.data, cnt.value,
                                         C.byref(cnt), C.byref(err)), err)
        return out[: cnt.value]

    # joint bin counts
    def joint_range(self, spec_index):
        """tgx_joint_range_get: dict(total, n, non_finite, x_min, x_max, y_min, y_max)"""
        out = JointRange()
        err = _Error()
        _check(lib().tgx_joint_range_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return {name: getattr(out, name) for name, _ in JointRange._fields_}

    def joint_counts(self, spec_index):
        """tgx_joint_counts: (the (bins + 1)^2 cell counts, row-major, as a list of ints; rows outside [0, bins])"""
        n, outside = C.c_uint64(), C.c_uint64()
        err = _Error()
        _check(lib().tgx_joint_counts(self.plan.h, self.h, spec_index, None, 0, C.byref(n), None, C.byref(err)), err)
        cells = (C.c_uint64 * max(1, n.value))()
        _check(lib().tgx_joint_counts(self.plan.h, self.h, spec_index, cells, n.value, C.byref(n), C.byref(outside),
                                      C.byref(err)), err)
        return list(cells)[: n.value], outside.value

    # histogram of a numeric column
    def histogram_range(self, spec_index):
        """tgx_histogram_range_get: dict(total, nulls, non_finite, n, min, max, sum, sum_squared)"""
        out = HistogramRange()
        err = _Error()
        _check(lib().tgx_histogram_range_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return {name: getattr(out, name) for name, _ in HistogramRange._fields_}

    def histogram_counts(self, spec_index):
        """tgx_histogram_counts: (the bucket counts as a list of ints, else_rows, non_finite)"""
        n = self.plan.histogram_buckets.get(spec_index, 0)
        counts = (C.c_uint64 * max(1, n))()
        else_rows, non_finite = C.c_uint64(), C.c_uint64()
        err = _Error()
        _check(lib().tgx_histogram_counts(self.plan.h, self.h, spec_index, counts, n, C.byref(else_rows),
                                          C.byref(non_finite), C.byref(err)), err)
        return list(counts)[:n], else_rows.value, non_finite.value

    # temporal row predicates
    def temporal_counts(self, spec_index):
        """tgx_temporal_get: (seen, considered, violations)"""
        out = TemporalCounts()
        err = _Error()
        _check(lib().tgx_temporal_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return out.seen, out.considered, out.violations

    # time gaps
    def time_gap_counts(self, spec_index):
        """tgx_time_gap_get: (seen, rows, gaps, violations, largest_gap)"""
        out = TimeGapCounts()
        err = _Error()
        _check(lib().tgx_time_gap_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return out.seen, out.rows, out.gaps, out.violations, out.largest_gap

    # numeric value rules
    def value_rule_counts(self, spec_index):
        """tgx_value_rule_get: (seen, considered, valid, cast_errors)"""
        out = ValueRuleCounts()
        err = _Error()
        _check(lib().tgx_value_rule_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return out.seen, out.considered, out.valid, out.cast_errors

    def row_predicate_counts(self, spec_index):
        """tgx_row_predicate_get: (seen, satisfied, unknown, failed)"""
        out = RowPredicateCounts()
        err = _Error()
        _check(lib().tgx_row_predicate_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return out.seen, out.satisfied, out.unknown, out.failed

    def type_classes(self, spec_index):
        """tgx_type_classes_get: {"seen", "non_null", "boolean_rows", "integer_rows", "double_rows", "date_rows",
        "datetime_rows", "string_rows", "undecided_rows"}"""
        out = TypeClassesCounts()
        err = _Error()
        _check(lib().tgx_type_classes_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return {name: getattr(out, name) for name, _ in TypeClassesCounts._fields_}

    def _counted_entries(self, call, entry_type, spec_index, *more):
        """the two calls of a *_entries function: ask for the sizes, allocate, fetch; (the entries, the bytes their
        offsets point into).  `more`: the call's arguments between n_bytes and the error"""
        err = _Error()
        n, nb = C.c_uint64(), C.c_uint64()
        _check(call(self.plan.h, self.h, spec_index, None, 0, C.byref(n), None, 0, C.byref(nb), *more, C.byref(err)), err)
        entries = (entry_type * max(n.value, 1))()
        buf = (C.c_uint8 * max(nb.value, 1))()
        _check(call(self.plan.h, self.h, spec_index, entries, n.value, C.byref(n), buf, nb.value, C.byref(nb), *more,
                    C.byref(err)), err)
        return entries[:n.value], bytes(buf)

    # value counts
    def value_counts(self, spec_index):
        """tgx_value_counts_get + tgx_value_counts_entries: (summary, counts) -- summary a dict of the six counters
        (seen, non_null, distinct, counted, overflow_rows, long_rows), counts a dict value -> count in the library's
        order (ascending by value); its keys are ints for an integer column and bytes for a string column"""
        L, err = lib(), _Error()
        s = ValueCountsSummary()
        _check(L.tgx_value_counts_get(self.plan.h, self.h, spec_index, C.byref(s), C.byref(err)), err)
        is_bytes = C.c_int32()
        entries, raw = self._counted_entries(L.tgx_value_counts_entries, ValueCountEntry, spec_index, C.byref(is_bytes))
        counts = {}
        for e in entries:
            counts[raw[e.offset:e.offset + e.length] if is_bytes.value else e.value] = e.count
        summary = {f: getattr(s, f) for f, _ in ValueCountsSummary._fields_}
        return summary, counts

    # pair counts
    def pair_counts(self, spec_index):
        """tgx_pair_counts_get + tgx_pair_counts_entries: (summary, counts) -- summary a dict of the eight counters (seen,
        both_non_null, distinct, counted, overflow_rows, long_rows, non_finite, out_of_range), counts a dict
        (x cell, y cell) -> count in the library's order (ascending by x cell, then y cell); a cell is bytes for a string
        side and an int (the bin index) for a binned side"""
        L, err = lib(), _Error()
        s = PairCountsSummary()
        _check(L.tgx_pair_counts_get(self.plan.h, self.h, spec_index, C.byref(s), C.byref(err)), err)
        entries, raw = self._counted_entries(L.tgx_pair_counts_entries, PairCountEntry, spec_index)
        mx, my = self.plan.pair_sides.get(spec_index, (PAIR_SIDE_VALUE, PAIR_SIDE_VALUE))
        counts = {}
        for e in entries:
            cx = raw[e.x_offset:e.x_offset + e.x_length] if mx == PAIR_SIDE_VALUE else e.x_bin
            cy = raw[e.y_offset:e.y_offset + e.y_length] if my == PAIR_SIDE_VALUE else e.y_bin
            counts[(cx, cy)] = e.count
        summary = {f: getattr(s, f) for f, _ in PairCountsSummary._fields_}
        return summary, counts

    # group counts
    def group_counts(self, spec_index):
        """tgx_group_counts_get + tgx_group_counts_entries: (summary, groups) -- summary a dict of the ten counters (seen,
        groups, counted, counted_non_null, null_group_rows, null_group_non_null, overflow_rows, overflow_non_null,
        long_rows, long_non_null), groups a dict key -> (total, non_null) in the library's order (ascending by key); its
        keys are ints for an integer group column and bytes for a string one; a spec that groups by several columns
        (spec(GROUP_COUNTS, value, columns=[..])) has bytes keys that are encoded tuples: term_amd.group_key.decode.  The
        NULL group is in the summary"""
        L, err = lib(), _Error()
        s = GroupCountsSummary()
        _check(L.tgx_group_counts_get(self.plan.h, self.h, spec_index, C.byref(s), C.byref(err)), err)
        is_bytes = C.c_int32()
        entries, raw = self._counted_entries(L.tgx_group_counts_entries, GroupCountEntry, spec_index, C.byref(is_bytes))
        groups = {}
        for e in entries:
            groups[raw[e.offset:e.offset + e.length] if is_bytes.value else e.value] = (e.total, e.non_null)
        summary = {f: getattr(s, f) for f, _ in GroupCountsSummary._fields_}
        return summary, groups

    # group sums
    def group_sums(self, spec_index):
        """tgx_group_sums_get + tgx_group_sums_entries: (summary, groups) -- summary a dict of seen, groups, is_float and
        the four classes counted, null_group, overflow, long_rows, each a tuple (rows, non_null, sum); groups a dict
        key -> (rows, non_null, sum) in the library's order (ascending by key), its keys ints for an integer group column
        and bytes for a string one.  A sum is an int (the wrapping Int64 sum, sum_i) for an integer value column and a
        float (sum_f) for a float one.  A spec that groups by several columns has bytes keys that are encoded tuples
        (term_amd.group_key.decode).  The NULL group is in the summary"""
        L, err = lib(), _Error()
        s = GroupSumsSummary()
        _check(L.tgx_group_sums_get(self.plan.h, self.h, spec_index, C.byref(s), C.byref(err)), err)
        is_bytes = C.c_int32()
        entries, raw = self._counted_entries(L.tgx_group_sums_entries, GroupSumEntry, spec_index, C.byref(is_bytes))
        is_float = bool(s.is_float)
        groups = {}
        for e in entries:
            key = raw[e.offset:e.offset + e.length] if is_bytes.value else e.value
            groups[key] = (e.rows, e.non_null, e.sum_f if is_float else e.sum_i)
        summary = {"seen": s.seen, "groups": s.groups, "is_float": is_float}
        for name in ("counted", "null_group", "overflow", "long_rows"):
            c = getattr(s, name)
            summary[name] = (c.rows, c.non_null, c.sum_f if is_float else c.sum_i)
        return summary, groups

    # key probe
    def key_probe_set_parent(self, spec_index, device_ptr, n_records):
        """tgx_key_probe_set_parent: the parent's key set of a KEY_PROBE spec, n_records {key, count} records in device
        memory (what distinct_export(spec, 1) of the parent's state hands out), before the state's first batch"""
        err = _Error()
        _check(lib().tgx_key_probe_set_parent(self.plan.h, self.h, spec_index, device_ptr, int(n_records), C.byref(err)),
               err)

    def key_probe(self, spec_index):
        """tgx_key_probe_get + tgx_key_probe_entries: (summary, missing) -- summary a dict of the fields of
        tgx_key_probe_summary (reserved left out), missing a dict key -> rows in the library's order (ascending)"""
        L, err = lib(), _Error()
        s = KeyProbeSummary()
        _check(L.tgx_key_probe_get(self.plan.h, self.h, spec_index, C.byref(s), C.byref(err)), err)
        n = C.c_uint64()
        _check(L.tgx_key_probe_entries(self.plan.h, self.h, spec_index, None, 0, C.byref(n), C.byref(err)), err)
        entries = (KeyProbeEntry * max(n.value, 1))()
        _check(L.tgx_key_probe_entries(self.plan.h, self.h, spec_index, entries, n.value, C.byref(n), C.byref(err)), err)
        summary = {f: getattr(s, f) for f, _ in KeyProbeSummary._fields_ if f != "reserved"}
        return summary, {e.value: e.count for e in entries[:n.value]}

    def key_probe_strings(self, spec_index):
        """tgx_key_probe_get + tgx_key_probe_strings_get + tgx_key_probe_entries_bytes of a strings spec: (summary,
        missing) -- summary the fields of tgx_key_probe_summary plus long_rows and max_value_bytes, missing a dict
        bytes -> rows in the library's order (ascending bytewise)"""
        L, err = lib(), _Error()
        s, more = KeyProbeSummary(), KeyProbeStrings()
        _check(L.tgx_key_probe_get(self.plan.h, self.h, spec_index, C.byref(s), C.byref(err)), err)
        _check(L.tgx_key_probe_strings_get(self.plan.h, self.h, spec_index, C.byref(more), C.byref(err)), err)
        entries, raw = self._counted_entries(L.tgx_key_probe_entries_bytes, ValueCountEntry, spec_index)
        summary = {f: getattr(s, f) for f, _ in KeyProbeSummary._fields_ if f != "reserved"}
        summary["long_rows"], summary["max_value_bytes"] = more.long_rows, more.max_value_bytes
        return summary, {raw[e.offset:e.offset + e.length]: e.count for e in entries}

    def key_probe_tuples(self, spec_index):
        """tgx_key_probe_get + tgx_key_probe_tuples_get + tgx_key_probe_entries_tuples of a tuples spec: (summary,
        entries) -- summary the fields of tgx_key_probe_summary plus null_counted, null_overflow_rows, null_keys and
        arity; entries a list of (hash_a, hash_b, count, has_null) in the library's order (ascending by the pair)"""
        L, err = lib(), _Error()
        s, more = KeyProbeSummary(), KeyProbeTuples()
        _check(L.tgx_key_probe_get(self.plan.h, self.h, spec_index, C.byref(s), C.byref(err)), err)
        _check(L.tgx_key_probe_tuples_get(self.plan.h, self.h, spec_index, C.byref(more), C.byref(err)), err)
        n = C.c_uint64(0)
        _check(L.tgx_key_probe_entries_tuples(self.plan.h, self.h, spec_index, None, 0, C.byref(n), C.byref(err)), err)
        entries = (KeyProbeTupleEntry * max(n.value, 1))()
        _check(L.tgx_key_probe_entries_tuples(self.plan.h, self.h, spec_index, entries, n.value, C.byref(n), C.byref(err)),
               err)
        summary = {f: getattr(s, f) for f, _ in KeyProbeSummary._fields_ if f != "reserved"}
        summary.update({f: getattr(more, f) for f, _ in KeyProbeTuples._fields_ if f != "reserved"})
        return summary, [(e.hash_a, e.hash_b, e.count, e.has_null) for e in entries[:n.value]]

    def key_probe_rows(self, spec_index):
        """tgx_key_probe_rows_get: (device pointer or None, n_records) of a rows spec's 16-byte {key, 1} records, or of
        a rows strings spec's 32-byte {hash_a, hash_b, count, 0} records"""
        ptr, n, err = C.c_void_p(), C.c_uint64(), _Error()
        _check(lib().tgx_key_probe_rows_get(self.plan.h, self.h, spec_index, C.byref(ptr), C.byref(n), C.byref(err)), err)
        return ptr.value, n.value

    def key_probe_rows_records(self, spec_index, record_bytes):
        """the gathered records as a host array of uint64 rows, record_bytes // 8 words each (16: a rows spec, 32: a
        rows strings spec; tests: the records are device memory)"""
        import numpy as np
        import torch

        ptr, total = self.key_probe_rows(spec_index)
        if total == 0:
            return np.zeros((0, record_bytes // 8), np.uint64)

        class P:
            __cuda_array_interface__ = {"shape": (total * record_bytes,), "typestr": "|u1", "data": (ptr, False),
                                        "version": 2}

        raw = torch.as_tensor(P(), device="cuda").clone().cpu().numpy()
        return raw.view(np.uint64).reshape(total, record_bytes // 8)

    def key_probe_pairs(self, spec_index):
        """tgx_key_probe_pairs_get: dict(pairs, join_rows, parent_rows, parent_count_digest, max_count) of a counted
        KEY_PROBE spec"""
        out = KeyProbePairs()
        err = _Error()
        _check(lib().tgx_key_probe_pairs_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return {name: getattr(out, name) for name, _ in KeyProbePairs._fields_}

    def pair_range(self, spec_index):
        """tgx_pair_range_get: dict(seen, both_non_null, n, non_finite, min, max) of a spec in its range phase"""
        out = PairRange()
        err = _Error()
        _check(lib().tgx_pair_range_get(self.plan.h, self.h, spec_index, C.byref(out), C.byref(err)), err)
        return {name: getattr(out, name) for name, _ in PairRange._fields_}

    # distinct key exchange
    def distinct_export(self, spec_index, world):
        ptr = C.c_void_p()
        counts = (C.c_uint64 * world)()
        err = _Error()
        _check(lib().tgx_distinct_export(self.plan.h, self.h, spec_index, world, C.byref(ptr), counts,
                                         C.byref(err)), err)
        return ptr.value, list(counts)

    def distinct_export_records(self, spec_index):
        """the key records of a DISTINCT task as a host array of uint64 rows: (key, count) for numeric keys,
        (fingerprint word a, word b, count, 0) for string / tuple keys (tests: the records are device memory)"""
        import numpy as np
        import torch

        ptr, counts = self.distinct_export(spec_index, 1)
        width = self.distinct_record_bytes(spec_index)
        total = counts[0]
        if total == 0:
            return np.zeros((0, width // 8), np.uint64)

        class P:
            __cuda_array_interface__ = {"shape": (total * width,), "typestr": "|u1", "data": (ptr, False), "version": 2}

        raw = torch.as_tensor(P(), device="cuda").clone().cpu().numpy()
        return raw.view(np.uint64).reshape(total, width // 8)

    def distinct_range_hint(self, spec_index, lo, hi):
        err = _Error()
        _check(lib().tgx_distinct_range_hint(self.plan.h, self.h, spec_index, int(lo), int(hi), C.byref(err)), err)

    def distinct_bitmap_view(self, spec_index):
        """(base, n_words, seen_ptr, twice_ptr or None); raises TGX_UNSUPPORTED when the set is a hash table"""
        base, n = C.c_int64(), C.c_uint64()
        seen, twice = C.c_void_p(), C.c_void_p()
        err = _Error()
        _check(lib().tgx_distinct_bitmap_view(self.plan.h, self.h, spec_index, C.byref(base), C.byref(n),
                                              C.byref(seen), C.byref(twice), C.byref(err)), err)
        return base.value, n.value, seen.value, twice.value

    def distinct_adopt_slices(self, spec_index, slice_base, seen_ptr, twice_ptr, n_slices, slice_words,
                              slice_stride_words=0):
        err = _Error()
        _check(lib().tgx_distinct_adopt_slices(self.plan.h, self.h, spec_index, int(slice_base), seen_ptr, twice_ptr,
                                               n_slices, slice_words, slice_stride_words, C.byref(err)), err)

    def distinct_record_bytes(self, spec_index):
        return lib().tgx_distinct_record_bytes(self.plan.h, self.h, spec_index)

    def distinct_import(self, spec_index, device_ptr, n_records):
        err = _Error()
        _check(lib().tgx_distinct_import(self.plan.h, self.h, spec_index, device_ptr, n_records, C.byref(err)),
               err)

    # profiling
    def profile_enable(self, on=True):
        lib().tgx_profile_enable(self.h, int(on))

    def profile_reset(self):
        lib().tgx_profile_reset(self.h)

    def profile_get(self, kernel):
        ms, n, b = C.c_double(), C.c_uint64(), C.c_uint64()
        err = _Error()
        _check(lib().tgx_profile_get(self.h, kernel.encode(), C.byref(ms), C.byref(n), C.byref(b), C.byref(err)),
               err)
        return dict(total_ms=ms.value, launches=n.value, bytes=b.value)
