"""Python face of the host-side mirror of term-guard's builder API (term_amd/csrc/host/term_guard.h).

Same names and argument meaning as the reference (core/check.rs, core/suite.rs, constraints/assertion.rs,
core/builder_extensions.rs); a suite is serialised to the JSON of include/tgx_host.h and run by libtgx:

    suite = (ValidationSuite.builder("users").table_name("users")
             .check(Check.builder("required").level(Level.ERROR)
                    .completeness("user_id", CompletenessOptions.full())
                    .has_min("age", Assertion.GreaterThanOrEqual(0.0)).build())
             .build())
    result = suite.run({"user_id": col, "age": col})     # dict of term_amd.Column, or a pyarrow Table
    result.is_success(), result.report.issues, result.to_json()
"""
import ctypes as C
import json
import re

from . import _lib
from ._lib import MEM_HOST, MEM_HOST_RETAINED, Column, TgxError, _Column, _Error


class Level:
    INFO, WARNING, ERROR = "info", "warning", "error"
    Info, Warning, Error = INFO, WARNING, ERROR


class Assertion:
    """constraints/assertion.rs:27-46"""

    def __init__(self, kind, *args):
        self.kind, self.args = kind, [float(a) for a in args]

    @staticmethod
    def Equals(v): return Assertion("equals", v)
    @staticmethod
    def NotEquals(v): return Assertion("not_equals", v)
    @staticmethod
    def GreaterThan(v): return Assertion("greater_than", v)
    @staticmethod
    def GreaterThanOrEqual(v): return Assertion("greater_than_or_equal", v)
    @staticmethod
    def LessThan(v): return Assertion("less_than", v)
    @staticmethod
    def LessThanOrEqual(v): return Assertion("less_than_or_equal", v)
    @staticmethod
    def Between(lo, hi): return Assertion("between", lo, hi)
    @staticmethod
    def NotBetween(lo, hi): return Assertion("not_between", lo, hi)

    def to_json(self):
        return {"kind": self.kind, "args": self.args}

    def evaluate(self, value):
        holds = C.c_int32()
        err = _Error()
        _host_check(_host().tgx_host_assertion_json(json.dumps(self.to_json()).encode(), float(value), C.byref(holds),
                                                    None, C.byref(err)), err)
        return bool(holds.value)

    def description(self):
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_assertion_json(json.dumps(self.to_json()).encode(), 0.0, None, C.byref(out),
                                                    C.byref(err)), err)
        return _take(out)

    __str__ = description


class LogicalOperator:
    """core/logical.rs:32-45"""
    All, Any = "all", "any"

    @staticmethod
    def Exactly(n): return {"exactly": int(n)}
    @staticmethod
    def AtLeast(n): return {"at_least": int(n)}
    @staticmethod
    def AtMost(n): return {"at_most": int(n)}


class CompletenessOptions:
    """core/builder_extensions.rs:14-80"""

    def __init__(self, threshold=1.0, operator=LogicalOperator.All):
        self.threshold_, self.operator_ = threshold, operator

    @staticmethod
    def full(): return CompletenessOptions(1.0)
    @staticmethod
    def threshold(t): return CompletenessOptions(t)
    @staticmethod
    def at_least(n): return CompletenessOptions(1.0, LogicalOperator.AtLeast(n))
    @staticmethod
    def any(): return CompletenessOptions(1.0, LogicalOperator.Any)

    def with_operator(self, op):
        self.operator_ = op
        return self


class ConstraintOptions(CompletenessOptions):
    """core/unified.rs:131-191"""

    @staticmethod
    def new(): return ConstraintOptions()

    def with_threshold(self, t):
        self.threshold_ = t
        return self


class FormatOptions:
    """constraints/format.rs:367-470"""

    def __init__(self, case_sensitive=True, trim_before_check=False, null_is_valid=True):
        self.case_sensitive_, self.trim_, self.null_is_valid_ = case_sensitive, trim_before_check, null_is_valid

    @staticmethod
    def new(): return FormatOptions()
    @staticmethod
    def case_insensitive(): return FormatOptions(case_sensitive=False)
    @staticmethod
    def strict(): return FormatOptions(null_is_valid=False)
    @staticmethod
    def lenient(): return FormatOptions(False, True, True)
    @staticmethod
    def with_trimming(): return FormatOptions(trim_before_check=True)

    def case_sensitive(self, v):
        self.case_sensitive_ = v
        return self

    def trim_before_check(self, v):
        self.trim_ = v
        return self

    def null_is_valid(self, v):
        self.null_is_valid_ = v
        return self

    def to_json(self):
        return {"case_sensitive": self.case_sensitive_, "trim_before_check": self.trim_,
                "null_is_valid": self.null_is_valid_}


class NullHandling:
    Exclude, Include, Distinct = "exclude", "include", "distinct"


def _cols(columns):
    return [columns] if isinstance(columns, str) else list(columns)


class CheckBuilder:
    """core/check.rs:217-2310 (the hot-path subset listed in SURVEY.md section 8a)"""

    def __init__(self, name):
        self._c = {"name": name, "level": Level.WARNING, "constraints": []}

    def level(self, level):
        self._c["level"] = level
        return self

    def description(self, d):
        self._c["description"] = d
        return self

    def _add(self, **kw):
        self._c["constraints"].append(kw)
        return self

    def has_size(self, assertion):
        return self._add(type="size", assertion=assertion.to_json())

    def has_approx_count_distinct(self, column, assertion):
        """core/check.rs:379-390; the metric is the exact number of distinct non-NULL values"""
        return self._add(type="approx_count_distinct", column=column, assertion=assertion.to_json())

    def completeness(self, columns, options=None):
        o = options or CompletenessOptions.full()
        return self._add(type="completeness", columns=_cols(columns), operator=o.operator_, threshold=o.threshold_)

    def any_complete(self, columns):
        return self._add(type="completeness", columns=_cols(columns), operator="any", threshold=1.0)

    def at_least_complete(self, n, columns, threshold):
        return self._add(type="completeness", columns=_cols(columns), operator={"at_least": n}, threshold=threshold)

    def exactly_complete(self, n, columns, threshold):
        return self._add(type="completeness", columns=_cols(columns), operator={"exactly": n}, threshold=threshold)

    def statistic(self, column, statistic, assertion, p=0.5):
        return self._add(type="statistic", column=column, statistic=statistic, p=p, assertion=assertion.to_json())

    def has_min(self, column, assertion): return self.statistic(column, "min", assertion)
    def has_max(self, column, assertion): return self.statistic(column, "max", assertion)
    def has_mean(self, column, assertion): return self.statistic(column, "mean", assertion)
    def has_sum(self, column, assertion): return self.statistic(column, "sum", assertion)
    def has_standard_deviation(self, column, assertion): return self.statistic(column, "standard_deviation", assertion)
    def has_variance(self, column, assertion): return self.statistic(column, "variance", assertion)

    def uniqueness(self, columns, kind, threshold=1.0, assertion=None, null_handling=NullHandling.Exclude):
        kw = dict(type="uniqueness", columns=_cols(columns), kind=kind, threshold=threshold, null_handling=null_handling)
        if assertion is not None:
            kw["assertion"] = assertion.to_json()
        return self._add(**kw)

    def validates_uniqueness(self, columns, threshold): return self.uniqueness(columns, "full_uniqueness", threshold)
    def validates_distinctness(self, columns, assertion): return self.uniqueness(columns, "distinctness", assertion=assertion)
    def validates_unique_value_ratio(self, columns, assertion):
        return self.uniqueness(columns, "unique_value_ratio", assertion=assertion)
    def validates_primary_key(self, columns): return self.uniqueness(columns, "primary_key")
    def validates_uniqueness_with_nulls(self, columns, threshold, null_handling):
        return self.uniqueness(columns, "unique_with_nulls", threshold, null_handling=null_handling)

    def primary_key(self, columns):
        return self.completeness(columns, CompletenessOptions.full()).validates_uniqueness(columns, 1.0)

    def is_contained_in(self, column, allowed_values):
        """constraints/values.rs:200-330: every non-NULL value is one of `allowed_values`"""
        return self._add(type="containment", column=column, allowed_values=list(allowed_values))

    # check.rs:518-623, 1777-1785 (constraints/length.rs)
    def length(self, column, kind, a=0, b=0):
        """kind: min | max | between | exactly | not_empty"""
        return self._add(type="length", column=column, kind=kind, a=a, b=b)

    def has_min_length(self, column, n): return self.length(column, "min", n)
    def has_max_length(self, column, n): return self.length(column, "max", n)
    def has_length_between(self, column, lo, hi): return self.length(column, "between", lo, hi)
    def has_exact_length(self, column, n): return self.length(column, "exactly", n)
    def is_not_empty(self, column): return self.length(column, "not_empty")

    def has_format(self, column, fmt, threshold, options=None, **kw):
        return self._add(type="format", column=column, format=fmt, threshold=threshold,
                         options=(options or FormatOptions()).to_json(), **kw)

    def validates_regex(self, column, pattern, threshold): return self.has_format(column, "regex", threshold, pattern=pattern)
    def validates_regex_with_options(self, column, pattern, threshold, options):
        return self.has_format(column, "regex", threshold, options, pattern=pattern)
    def validates_email(self, column, threshold): return self.has_format(column, "email", threshold)
    def validates_url(self, column, threshold, allow_localhost=False):
        return self.has_format(column, "url", threshold, allow_localhost=allow_localhost)
    def validates_credit_card(self, column, threshold, detect_only=False):
        return self.has_format(column, "credit_card", threshold, detect_only=detect_only)
    def validates_phone(self, column, threshold, country=None):
        kw = {"country": country} if country else {}
        return self.has_format(column, "phone", threshold, FormatOptions.with_trimming(), **kw)
    def validates_postal_code(self, column, threshold, country):
        return self.has_format(column, "postal_code", threshold, FormatOptions.with_trimming(), country=country)
    def validates_uuid(self, column, threshold): return self.has_format(column, "uuid", threshold)
    def validates_ipv4(self, column, threshold): return self.has_format(column, "ipv4", threshold)
    def validates_ipv6(self, column, threshold): return self.has_format(column, "ipv6", threshold)
    def validates_json(self, column, threshold): return self.has_format(column, "json", threshold)
    def validates_iso8601_datetime(self, column, threshold): return self.has_format(column, "iso8601_datetime", threshold)
    def email(self, column, threshold): return self.has_format(column, "email", threshold, FormatOptions(True, True, False))
    def contains_ssn(self, column, threshold):
        return self.has_format(column, "social_security_number", threshold, FormatOptions.with_trimming())

    def has_approx_quantile(self, column, quantile, assertion):
        return self._add(type="quantile", column=column, quantile=quantile, assertion=assertion.to_json())

    def has_correlation(self, column1, column2, assertion):
        return self._add(type="correlation", column1=column1, column2=column2, assertion=assertion.to_json())

    def temporal_ordering(self, table_name):
        """core/check.rs:2125-2179: pushes TemporalOrderingConstraint::new(table) as it stands -- empty column names, so
        evaluating it fails identifier validation, as in the reference; a configured object goes through constraint()"""
        return self.constraint(TemporalOrderingConstraint(table_name))

    def cross_table_sum(self, left_column, right_column):
        """core/check.rs:2054-2065: pushes CrossTableSumConstraint::new(left, right); a configured object goes through
        constraint()"""
        return self.constraint(CrossTableSumConstraint(left_column, right_column))

    def foreign_key(self, child_column, parent_column):
        """pushes ForeignKeyConstraint::new(child, parent); a configured object goes through constraint()"""
        return self.constraint(ForeignKeyConstraint(child_column, parent_column))

    def join_coverage(self, left_table, right_table):
        """core/check.rs:2112-2123: pushes JoinCoverageConstraint::new(left, right) -- without join keys, which is an
        evaluation error, as in the reference; a configured object goes through constraint()"""
        return self.constraint(JoinCoverageConstraint(left_table, right_table))

    def has_consistent_data_type(self, column, threshold):
        """core/check.rs:651-657: DataTypeConstraint::type_consistency(column, threshold)"""
        return self.constraint(DataTypeConstraint.type_consistency(column, threshold))

    def satisfies(self, sql_expression, hint=None, string_functions_on_device=False):
        """core/check.rs:685-694: CustomSqlConstraint::new(sql_expression, hint); raises where the reference's builder
        panics on the constructor's Err.  string_functions_on_device: the constraint's opt-in of that name"""
        c = CustomSqlConstraint(sql_expression, hint)
        if string_functions_on_device:
            c.string_functions_on_device(True)
        return self.constraint(c)

    def has_histogram(self, column, measures, max_distinct=10000):
        """Check::has_histogram: HistogramConstraint.new(column, measures) -- `measures` is what stands for the
        reference's assertion function here: a list of HistogramMeasure entries that must all hold"""
        return self.constraint(HistogramConstraint(column, measures, max_distinct=max_distinct))

    def has_histogram_with_description(self, column, measures, description, max_distinct=10000):
        return self.constraint(HistogramConstraint(column, measures, description, max_distinct))

    def constraint(self, c):
        """core/check.rs:263: a constraint object (MultiStatisticalConstraint, QuantileConstraint,
        CorrelationConstraint below) instead of a builder shorthand"""
        return self._add(**c.spec)

    def build(self):
        return Check(self._c)


class StatisticType:
    """constraints/statistics.rs:24-43"""
    Min, Max, Mean, Sum = "min", "max", "mean", "sum"
    StandardDeviation, Variance, Median = "standard_deviation", "variance", "median"

    @staticmethod
    def Percentile(p): return ("percentile", p)


class MultiStatisticalConstraint:
    """constraints/statistics.rs:376-417: `statistics` = [(StatisticType, Assertion), ...] of one column"""

    def __init__(self, column, statistics):
        stats = []
        for st, a in statistics:
            name, p = st if isinstance(st, tuple) else (st, 0.5)
            stats.append({"statistic": name, "p": p, "assertion": a.to_json()})
        self.spec = {"type": "multi_statistic", "column": column, "statistics": stats}


class QuantileCheck:
    """constraints/quantile.rs:36-58"""

    def __init__(self, quantile, assertion):
        self.quantile, self.assertion = quantile, assertion

    def to_json(self):
        return {"quantile": self.quantile, "assertion": self.assertion.to_json()}


class QuantileConstraint:
    """constraints/quantile.rs:144-225 (QuantileValidation::Single / Multiple / Monotonic / Distribution / Custom)"""

    def __init__(self, column, **spec):
        self.spec = dict(type="quantile", column=column, **spec)

    @staticmethod
    def median(column, assertion):
        return QuantileConstraint.percentile(column, 0.5, assertion)

    @staticmethod
    def percentile(column, quantile, assertion):
        return QuantileConstraint(column, validation="single", quantile=quantile, assertion=assertion.to_json())

    @staticmethod
    def multiple(column, checks):
        return QuantileConstraint(column, validation="multiple", checks=[c.to_json() for c in checks])

    @staticmethod
    def monotonic(column, quantiles, strict):
        return QuantileConstraint(column, validation="monotonic", quantiles=list(quantiles), strict=bool(strict))

    @staticmethod
    def distribution(column):
        return QuantileConstraint(column, validation="distribution")


class CorrelationType:
    """constraints/correlation.rs:19-36"""
    Pearson, Spearman, KendallTau = "pearson", "spearman", "kendall_tau"
    MutualInformation, Covariance, Custom = "mutual_information", "covariance", "custom"


class CorrelationConstraint:
    """constraints/correlation.rs:147-263 (CorrelationValidation::Pairwise / Range / Independence / MultiColumn /
    Stability)"""

    def __init__(self, **spec):
        self.spec = dict(type="correlation", **spec)

    @staticmethod
    def pairwise(column1, column2, correlation_type, assertion, sql_expression=""):
        return CorrelationConstraint(validation="pairwise", column1=column1, column2=column2,
                                     correlation_type=correlation_type, assertion=assertion.to_json(),
                                     sql_expression=sql_expression)

    @staticmethod
    def pearson(column1, column2, assertion):
        return CorrelationConstraint.pairwise(column1, column2, CorrelationType.Pearson, assertion)

    @staticmethod
    def spearman(column1, column2, assertion):
        return CorrelationConstraint.pairwise(column1, column2, CorrelationType.Spearman, assertion)

    @staticmethod
    def covariance(column1, column2, assertion):
        return CorrelationConstraint.pairwise(column1, column2, CorrelationType.Covariance, assertion)

    @staticmethod
    def range(column1, column2, correlation_type, min, max):
        return CorrelationConstraint(validation="range", column1=column1, column2=column2,
                                     correlation_type=correlation_type, min=min, max=max)

    @staticmethod
    def independence(column1, column2, max_correlation):
        return CorrelationConstraint(validation="independence", column1=column1, column2=column2,
                                     max_correlation=max_correlation)

    @staticmethod
    def multi_column(columns, correlation_type=CorrelationType.Pearson):
        return CorrelationConstraint(validation="multi_column", columns=list(columns), correlation_type=correlation_type)


class TemporalOrderingConstraint:
    """constraints/temporal_ordering.rs:106-288, one method per builder call of the reference.  BeforeAfter,
    BusinessHours and DateRange run on the device (TGX_CHECK_TEMPORAL); MaxTimeGap evaluates to an error unless
    window_on_device(True) asks for it (TGX_CHECK_TIME_GAP); EventSequence evaluates to an error"""

    def __init__(self, table_name):
        self.spec = {"type": "temporal_ordering", "table": table_name, "allow_nulls": False, "tolerance_seconds": 0}

    def _type(self, validation, **fields):
        keep = {k: self.spec[k] for k in ("type", "table", "allow_nulls", "tolerance_seconds")}
        self.spec = dict(keep, validation=validation, **fields)
        return self

    def before_after(self, before_column, after_column):
        return self._type("before_after", before_column=before_column, after_column=after_column, allow_equal=False)

    def before_or_equal(self, before_column, after_column):
        return self._type("before_after", before_column=before_column, after_column=after_column, allow_equal=True)

    def business_hours(self, timestamp_column, start_time, end_time):
        return self._type("business_hours", timestamp_column=timestamp_column, start_time=start_time,
                          end_time=end_time, weekdays_only=False, timezone=None)

    def weekdays_only(self, weekdays_only):
        if self.spec.get("validation") == "business_hours":
            self.spec["weekdays_only"] = bool(weekdays_only)
        return self

    def with_timezone(self, timezone):
        if self.spec.get("validation") == "business_hours":
            self.spec["timezone"] = timezone
        return self

    def date_range(self, timestamp_column, min_date=None, max_date=None):
        return self._type("date_range", timestamp_column=timestamp_column, min_date=min_date, max_date=max_date)

    def max_time_gap(self, timestamp_column, max_gap_seconds):
        return self._type("max_time_gap", timestamp_column=timestamp_column, max_gap_seconds=int(max_gap_seconds),
                          group_by_column=None)

    def group_by(self, column):
        if self.spec.get("validation") == "max_time_gap":
            self.spec["group_by_column"] = column
        return self

    def window_on_device(self, on):
        """MaxTimeGap only (this layer's own call): run the LAG() window on the device.  Off by default -- the check
        keeps 8 B per row (16 B with a group) on the device until the verdict, and its state cannot be merged,
        serialized or reduced across ranks"""
        if self.spec.get("validation") == "max_time_gap":
            self.spec["window_on_device"] = bool(on)
        return self

    def allow_nulls(self, allow):
        self.spec["allow_nulls"] = bool(allow)
        return self

    def tolerance_seconds(self, seconds):
        self.spec["tolerance_seconds"] = int(seconds)
        return self


class CrossTableSumConstraint:
    """constraints/cross_table_sum.rs:87-140, one method per builder call of the reference: SUM(left) against SUM(right),
    `left_column` / `right_column` qualified as "table.column", over the whole tables or per group of ONE group column
    that both tables have.  Each side is one walk of its table on the device (TGX_CHECK_GROUP_SUMS, or NUMERIC_STATS for
    the ungrouped form); the outer join runs on the host.  It needs ValidationSuite.run(table, tables={name: table})"""

    def __init__(self, left_column, right_column):
        self.spec = {"type": "cross_table_sum", "left_column": left_column, "right_column": right_column, "group_by": [],
                     "tolerance": 0.0, "max_violations_reported": 100, "max_groups": _lib.GROUP_SUMS_MAX_GROUPS}

    def group_by(self, columns):
        self.spec["group_by"] = _cols(columns)
        return self

    def tolerance(self, tolerance):
        self.spec["tolerance"] = abs(float(tolerance))  # (:129-132)
        return self

    def max_violations_reported(self, n):
        self.spec["max_violations_reported"] = int(n)
        return self

    def max_groups(self, n):
        """this layer's own: the groups a side's table on the device is sized for (1 .. 65 536, the default).  A side
        with more (overflow rows), or with keys longer than 256 bytes, makes the constraint an error that names the
        bound -- never a verdict on partial sums"""
        self.spec["max_groups"] = int(n)
        return self

    def composite_groups_on_device(self, on=True):
        """an opt-in: 2 .. 8 group_by columns are one GROUP_SUMS walk a side on the tuple of the columns, joined on the
        host by their encoded keys; a key with a NULL component never joins.  Off, several columns are an error"""
        if on:
            self.spec["composite_groups_on_device"] = True
        else:
            self.spec.pop("composite_groups_on_device", None)
        return self

    def name(self): return "cross_table_sum"
    def left_column(self): return self.spec["left_column"]
    def right_column(self): return self.spec["right_column"]
    def group_by_columns(self): return list(self.spec["group_by"])

    def verdict_from_sums(self, left, right):
        """the join and the verdict on given sums (no device): left / right are numbers for the ungrouped form, else
        dicts {"groups": [[key, sum], ..] ascending by key, "null_group": sum or None, "overflow_rows", "long_rows"}"""
        out, err = C.c_char_p(), _Error()
        _host_check(_host().tgx_host_cross_table_sum_json(json.dumps(self.spec).encode(),
                                                          json.dumps({"left": left, "right": right}).encode(),
                                                          C.byref(out), C.byref(err)), err)
        v = json.loads(_take(out))
        for k in ("metric", "total_left_sum", "total_right_sum", "max_difference"):
            if isinstance(v[k], str):
                v[k] = float(v[k])
        return v


class ForeignKeyConstraint:
    """constraints/foreign_key.rs:78-117, one method per builder call of the reference: every non-NULL value of
    `child_column` is a value of `parent_column`, both qualified as "table.column".  The parent's column is walked once
    under a DISTINCT spec, its key set handed to a KEY_PROBE spec over the child's column, and the child walked once:
    integer keys, or string keys when both columns are string layouts (Utf8, LargeUtf8, Utf8View, Dictionary<Int32,
    Utf8>; the parent's values then travel as keyed 128-bit fingerprints).  Any other column type, and a pair of an
    integer and a string column, is the constraint's own error, which says it is not on the GPU path.  It
    needs ValidationSuite.run(table, tables={name: table})"""

    def __init__(self, child_column, parent_column):
        self.spec = {"type": "foreign_key", "child_column": child_column, "parent_column": parent_column,
                     "allow_nulls": False, "use_left_join": True, "max_violations_reported": 100,
                     "max_missing_keys": 10000}

    def allow_nulls(self, allow):
        self.spec["allow_nulls"] = bool(allow)
        return self

    def use_left_join(self, use_left_join):
        """accepted as the reference accepts it; there is one strategy here"""
        self.spec["use_left_join"] = bool(use_left_join)
        return self

    def max_violations_reported(self, n):
        self.spec["max_violations_reported"] = int(n)
        return self

    def max_missing_keys(self, n):
        """this layer's own: the missing keys the child's table on the device is sized for (1 .. 65 536, default
        10 000).  Rows beyond it are counted as overflow rows: the verdict and the metric stand, and `unique` reads
        "at least n" """
        self.spec["max_missing_keys"] = int(n)
        return self

    def max_value_bytes(self, n):
        """this layer's own, string keys only: the bytes a missing key may have to be kept (1 .. 256, default 256).
        Missing rows with a longer value are counted as long rows: the verdict and the metric stand, and `unique` reads
        "at least n" """
        self.spec["max_value_bytes"] = int(n)
        return self

    def name(self): return "foreign_key"
    def child_column(self): return self.spec["child_column"]
    def parent_column(self): return self.spec["parent_column"]

    def verdict_from_counts(self, counts):
        """the verdict on given counts (no device): a dict {"null_rows", "missing_rows", "overflow_rows",
        "missing_keys", "entries": [[key, count], ..] ascending by key, "examples": bool}; string keys: the keys are
        strings, ascending bytewise, and "long_rows" counts the missing rows whose value was too long to keep"""
        out, err = C.c_char_p(), _Error()
        _host_check(_host().tgx_host_foreign_key_json(json.dumps(self.spec).encode(), json.dumps(counts).encode(),
                                                      C.byref(out), C.byref(err)), err)
        return json.loads(_take(out))


class CoverageType:
    """constraints/join_coverage.rs:83-91"""
    Left, Right, Bidirectional = "left", "right", "bidirectional"


class JoinCoverageConstraint:
    """constraints/join_coverage.rs:94-163, one method per builder call of the reference: the match rate of
    `left_table` LEFT JOIN `right_table` on one key pair, SUM(CASE WHEN the far key IS NOT NULL ..) / COUNT(*), against
    expect_match_rate.  COUNT(*) over a join counts matched pairs: the far side's non-NULL keys are gathered as {key, 1}
    records and handed to a counted KEY_PROBE spec over the near side's column.  One key pair only: integer keys, or
    string keys when both columns are string layouts (Utf8, LargeUtf8, Utf8View, Dictionary<Int32, Utf8>; the far
    side's values then travel as keyed 128-bit fingerprints).  Composite keys (on_multiple with 2 .. 8 pairs) run on
    the device after composite_keys_on_device(True); without it they, other column types and a pair of an
    integer and a string column are the constraint's own error.  It needs
    ValidationSuite.run(table, tables={name: table})"""

    def __init__(self, left_table, right_table):
        self.spec = {"type": "join_coverage", "left_table": left_table, "right_table": right_table, "join_keys": [],
                     "expected_match_rate": 1.0, "coverage_type": CoverageType.Left, "distinct_only": False,
                     "max_examples_reported": 100, "max_missing_keys": 10000}

    @classmethod
    def from_spec(cls, spec):
        """the constraint of its JSON form (a dict as `spec` holds it)"""
        c = cls(spec["left_table"], spec["right_table"])
        c.on_multiple(spec.get("join_keys", []))
        c.expect_match_rate(spec.get("expected_match_rate", 1.0))
        c.coverage_type(spec.get("coverage_type", CoverageType.Left))
        c.distinct_only(spec.get("distinct_only", False))
        c.max_examples_reported(spec.get("max_examples_reported", 100))
        if "max_value_bytes" in spec:
            c.max_value_bytes(spec["max_value_bytes"])
        if "composite_keys_on_device" in spec:
            c.composite_keys_on_device(spec["composite_keys_on_device"])
        return c.max_missing_keys(spec.get("max_missing_keys", 10000))

    def on(self, left_column, right_column):
        self.spec["join_keys"] = [[left_column, right_column]]
        return self

    def on_multiple(self, keys):
        self.spec["join_keys"] = [[l, r] for l, r in keys]
        return self

    def expect_match_rate(self, rate):
        rate = float(rate)
        self.spec["expected_match_rate"] = min(1.0, max(0.0, rate))  # rate.clamp(0.0, 1.0) (:139-142)
        return self

    def coverage_type(self, coverage_type):
        if coverage_type not in (CoverageType.Left, CoverageType.Right, CoverageType.Bidirectional):
            raise ValueError("coverage_type is CoverageType.Left, .Right or .Bidirectional")
        self.spec["coverage_type"] = coverage_type
        return self

    def distinct_only(self, distinct):
        """total becomes COUNT(DISTINCT left column) under the same numerator, as the reference's SQL has it: the rate can
        exceed 1.  Left only: Bidirectional ignores it, with Right it is the constraint's error"""
        self.spec["distinct_only"] = bool(distinct)
        return self

    def max_examples_reported(self, n):
        self.spec["max_examples_reported"] = int(n)
        return self

    def max_missing_keys(self, n):
        """this layer's own, as ForeignKeyConstraint's: the missing keys the probe's table on the device is sized for"""
        self.spec["max_missing_keys"] = int(n)
        return self

    def max_value_bytes(self, n):
        """this layer's own, string keys only, as ForeignKeyConstraint's: the bytes a missing key may have to be kept
        (1 .. 256, default 256).  Missing rows with a longer value are counted as long rows: the rate stands, and the
        examples read "at least n" """
        self.spec["max_value_bytes"] = int(n)
        return self

    def composite_keys_on_device(self, on=True):
        """this layer's own, an opt-in: a join on 2 .. 8 key pairs (on_multiple) runs on the device under KEY_PROBE's
        tuple modes, each pair two integer or two string columns.  A row with a NULL in any key column joins nothing;
        the examples are counted over the tuples' fingerprints, a tuple with a NULL component being a value of its own.
        The key is written into `spec` only when this is called; without it a composite join stays the constraint's
        error"""
        self.spec["composite_keys_on_device"] = bool(on)
        return self

    def name(self): return "join_coverage"

    def verdict_from_counts(self, counts):
        """the verdict on given counts (no device): a dict {"left": {"pairs", "join_rows"}, "right": {..},
        "left_distinct", "examples": {"missing_keys", "null_rows", "overflow_rows", "long_rows", and for composite keys
        "null_keys", "null_overflow_rows"}} (include/tgx_host.h)"""
        out, err = C.c_char_p(), _Error()
        _host_check(_host().tgx_host_join_coverage_json(json.dumps(self.spec).encode(), json.dumps(counts).encode(),
                                                        C.byref(out), C.byref(err)), err)
        return json.loads(_take(out))


class NumericValidation:
    """constraints/datatype.rs:42-59"""
    NonNegative, Positive, Integer, Finite = ({"numeric": k} for k in ("non_negative", "positive", "integer", "finite"))

    @staticmethod
    def Range(min, max):
        # (JSON has no inf / NaN: such a bound travels as text and is the constraint's error when it is evaluated)
        def text(b):
            b = float(b)
            return b if b == b and abs(b) != float("inf") else ("NaN" if b != b else "inf" if b > 0 else "-inf")
        return {"numeric": "range", "min": text(min), "max": text(max)}


class StringTypeValidation:
    """constraints/datatype.rs:61-75"""
    NotEmpty, ValidUtf8, NotBlank = ({"string": k} for k in ("not_empty", "valid_utf8", "not_blank"))

    @staticmethod
    def MaxBytes(n): return {"string": "max_bytes", "max_bytes": int(n)}


class TemporalValidation:
    """constraints/datatype.rs:77-91"""
    PastDate, FutureDate, ValidTimezone = ({"temporal": k} for k in ("past_date", "future_date", "valid_timezone"))

    @staticmethod
    def DateRange(start, end): return {"temporal": "date_range", "start": start, "end": end}


class DataTypeValidation:
    """constraints/datatype.rs:21-40"""

    @staticmethod
    def SpecificType(data_type): return {"validation": "specific_type", "data_type": data_type}
    @staticmethod
    def Consistency(threshold): return {"validation": "consistency", "threshold": float(threshold)}
    @staticmethod
    def Numeric(v): return dict(v, validation="numeric")
    @staticmethod
    def String(v): return dict(v, validation="string")
    @staticmethod
    def Temporal(v): return dict(v, validation="temporal")
    @staticmethod
    def Custom(sql_predicate): return {"validation": "custom", "sql_predicate": sql_predicate}


class DataTypeConstraint:
    """constraints/datatype.rs:233-288.  The numeric NonNegative / Positive / Integer / Range validations run on the
    device (TGX_CHECK_VALUE_RULE); SpecificType reads the column's Arrow type, Consistency is the reference's placeholder;
    Finite and every String, Temporal and Custom validation evaluate to the constraint's own error.  The constructor
    raises what DataTypeConstraint::new returns as Err: a column name that is no identifier, a consistency threshold
    outside [0, 1].

    string_functions_on_device(True) is an opt-in for the four String validations: NotEmpty (LENGTH(c) > 0), ValidUtf8
    (c IS NOT NULL), NotBlank (TRIM(c) != '') and MaxBytes (OCTET_LENGTH(c) <= n) then plan one TGX_CHECK_ROW_PREDICATE
    request on [column], count the valid rows among the non-NULL ones and answer with the reference's
    "{:.1}% of values satisfy .." verdict; a column declared non-string is the constraint's error.  Without it, and for
    every other validation with or without it, the constraint answers as it did"""

    def __init__(self, column, validation):
        validate_identifier(column)
        if validation.get("validation") == "consistency" and not 0.0 <= validation["threshold"] <= 1.0:
            raise TgxError(1, "Configuration error: Threshold must be between 0.0 and 1.0")
        self.spec = dict(validation, type="datatype", column=column)

    def string_functions_on_device(self, on=True):
        """the opt-in of the class's docstring; the key is written into the constraint's JSON only when this is called"""
        self.spec["string_functions_on_device"] = bool(on)
        return self

    @staticmethod
    def non_negative(column):
        return DataTypeConstraint(column, DataTypeValidation.Numeric(NumericValidation.NonNegative))

    @staticmethod
    def type_consistency(column, threshold):
        return DataTypeConstraint(column, DataTypeValidation.Consistency(threshold))

    @staticmethod
    def specific_type(column, data_type):
        return DataTypeConstraint(column, DataTypeValidation.SpecificType(data_type))


class CustomSqlConstraint:
    """constraints/custom_sql.rs:24-93, 192-303: every row satisfies a boolean expression.  The expression is compiled by
    the library's closed predicate subset (row_predicate(); include/tgx.h TGX_CHECK_ROW_PREDICATE) and counted on the
    device; one outside the subset evaluates to the constraint's own error ("... not on the GPU path: <what>").  The
    constructor raises what CustomSqlConstraint::new returns as Err (validate_sql_expression, :100-190): of several
    forbidden words the first in the list's written order is named.

    string_functions_on_device(True) is an opt-in: the expression is then compiled under the dialect that also takes
    `col [NOT] LIKE 'pattern'` (no escapes: a backslash is refused), LENGTH / CHAR_LENGTH / CHARACTER_LENGTH /
    OCTET_LENGTH of a column against an integer, TRIM(col) = '' / <> '' and order comparisons of a string column with a
    string literal, by bytes (row_predicate(expression, string_functions=True)).  Without it such an expression is "not
    on the GPU path", as it was"""

    FORBIDDEN = ("DROP", "DELETE", "INSERT", "UPDATE", "CREATE", "ALTER", "TRUNCATE", "GRANT", "REVOKE", "EXECUTE", "EXEC",
                 "CALL", "MERGE", "REPLACE", "RENAME", "MODIFY", "SET", "COMMIT", "ROLLBACK", "SAVEPOINT", "BEGIN", "START",
                 "TRANSACTION", "LOCK", "UNLOCK")

    def __init__(self, expression, hint=None):
        refusal = self.refusal(expression)
        if refusal:
            raise TgxError(1, "Validation failed: " + refusal)
        self.expression, self.hint = expression, hint
        self.spec = {"type": "custom_sql", "expression": expression}
        if hint is not None:
            self.spec["hint"] = hint

    try_new = classmethod(lambda cls, expression, hint=None: cls(expression, hint))

    def string_functions_on_device(self, on=True):
        """the opt-in of the class's docstring; the key is written into the constraint's JSON only when this is called"""
        self.spec["string_functions_on_device"] = bool(on)
        return self

    @classmethod
    def refusal(cls, sql):
        """validate_sql_expression: the reference's message, or None for an expression it accepts"""
        upper = "".join(chr(ord(c) - 32) if "a" <= c <= "z" else c for c in sql)  # (ASCII, as the words are)
        for word in cls.FORBIDDEN:
            if re.search(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % word, upper):
                return "SQL expression contains forbidden operation: " + word
        if ";" in sql:
            return "SQL expression cannot contain semicolons"
        if "--" in sql or "/*" in sql or "*/" in sql:
            return "SQL expression cannot contain comments"
        return None

    def name(self):
        return "custom_sql"

    def metadata(self):
        """custom_sql.rs:288-302"""
        m = {"description": "Checks that all rows satisfy the SQL expression: " + self.expression,
             "expression": self.expression, "constraint_type": "custom"}
        if self.hint is not None:
            m["hint"] = self.hint
        return m

    def verdict(self, satisfied, total):
        """custom_sql.rs:234-281 on given counts: (status, metric, message)"""
        if total == 0:
            return "skipped", None, "No data to validate"
        ratio = float(satisfied) / float(total)
        if ratio == 1.0:
            return "success", ratio, None
        failed = int(float(total) - float(satisfied))
        if self.hint is not None:
            return "failure", ratio, "%s (%d rows failed the condition)" % (self.hint, failed)
        return "failure", ratio, ("Custom SQL condition not satisfied for %d rows. Expression: '%s'"
                                  % (failed, self.expression))


class HistogramMeasure:
    """One named measure of a column's value histogram held to an Assertion (constraints/histogram.rs:37-127): the form a
    histogram assertion takes where no function can travel (JSON, Python)"""

    @staticmethod
    def _of(measure, assertion, **extra):
        return dict(extra, measure=measure, assertion=assertion.to_json())

    @staticmethod
    def most_common_ratio(assertion): return HistogramMeasure._of("most_common_ratio", assertion)
    @staticmethod
    def least_common_ratio(assertion): return HistogramMeasure._of("least_common_ratio", assertion)
    @staticmethod
    def bucket_count(assertion): return HistogramMeasure._of("bucket_count", assertion)
    @staticmethod
    def entropy(assertion): return HistogramMeasure._of("entropy", assertion)
    @staticmethod
    def null_ratio(assertion): return HistogramMeasure._of("null_ratio", assertion)
    @staticmethod
    def top_n_ratio(n, assertion): return HistogramMeasure._of("top_n_ratio", assertion, n=int(n))
    @staticmethod
    def value_ratio(value, assertion): return HistogramMeasure._of("value_ratio", assertion, value=value)


class HistogramConstraint:
    """constraints/histogram.rs:154-410 over TGX_CHECK_VALUE_COUNTS: the column's value -> count map is counted on the
    device for at most `max_distinct` values (a column beyond that, or with strings above 256 bytes, is the constraint's
    error, with the numbers).  Buckets are ordered by count descending, then by the value's text; ratio = count / (total
    - nulls); the metric is the histogram's entropy in nats; no non-NULL row is Skipped ("No data to analyze").  Every
    measure must hold.  Value text is the string itself or the decimal text of an integer: a date, time, timestamp,
    duration, float, decimal, boolean or binary column is the constraint's error ("... not on the GPU path")"""

    def __init__(self, column, measures, description=None, max_distinct=10000):
        self.spec = {"type": "histogram", "column": column, "measures": list(measures), "max_distinct": int(max_distinct)}
        if description is not None:
            self.spec["description"] = description


class Check:
    def __init__(self, spec):
        self.spec = spec

    @staticmethod
    def builder(name):
        return CheckBuilder(name)

    def name(self): return self.spec["name"]
    def level(self): return self.spec["level"]


class Issue:
    def __init__(self, d):
        self.check_name, self.constraint_name = d["check_name"], d["constraint_name"]
        self.level, self.message, self.metric = d["level"], d["message"], d.get("metric")


class Metrics:
    def __init__(self, d):
        self.total_checks, self.passed_checks = d["total_checks"], d["passed_checks"]
        self.failed_checks, self.skipped_checks = d["failed_checks"], d["skipped_checks"]
        self.execution_time_ms, self.custom_metrics = d["execution_time_ms"], d.get("custom_metrics", {})


class Report:
    def __init__(self, d):
        self.suite_name, self.timestamp = d["suite_name"], d["timestamp"]
        self.metrics = Metrics(d["metrics"])
        self.issues = [Issue(i) for i in d["issues"]]

    def has_errors(self): return any(i.level == Level.ERROR for i in self.issues)
    def has_warnings(self): return any(i.level == Level.WARNING for i in self.issues)


class ValidationResult:
    """core/result.rs:123-196"""

    def __init__(self, text):
        self._json = text
        d = json.loads(text)
        self.status = d["status"]
        self.report = Report(d["report"])

    def is_success(self): return self.status == "success"
    def is_failure(self): return self.status == "failure"
    def metrics(self): return self.report.metrics if self.is_success() else None
    def to_json(self): return self._json


class ValidationSuiteBuilder:
    def __init__(self, name):
        self._s = {"name": name, "table_name": "data", "checks": []}

    def description(self, d):
        self._s["description"] = d
        return self

    def table_name(self, t):
        self._s["table_name"] = t
        return self

    def check(self, c):
        self._s["checks"].append(c.spec)
        return self

    def with_optimizer(self, _enabled):
        return self

    def strict_reference_types(self, on):
        """True (default): statistics the reference cannot read off a column's type are errors, as there
        (constraints/statistics.rs:277-308: the aggregate must come back Int64 or Float64 -- MIN / MAX of an Int32,
        Date32, Float32 or Timestamp column does not); False: the widened column's value answers (a deviation)"""
        self._s["strict_reference_types"] = bool(on)
        return self

    def exact_string_keys(self, on):
        """True (default): uniqueness checks over string / binary / tuple keys count by VALUE (equal fingerprints are
        confirmed byte by byte, TGX_FLAG_EXACT_KEYS) -- COUNT(DISTINCT c) as the reference computes it
        (constraints/uniqueness.rs:612-617); False: by keyed 128-bit fingerprint alone (deviations)"""
        self._s["exact_string_keys"] = bool(on)
        return self

    def column_type(self, column, arrow_type):
        """the Arrow DataType of a column of the table ("Int32", "Date32", "Timestamp(Nanosecond, None)", ...); a
        pyarrow table handed to run() declares its own"""
        self._s.setdefault("column_types", {})[column] = arrow_type
        return self

    def build(self):
        return ValidationSuite(self._s)


def _arrow_batches(table):
    """pyarrow Table / RecordBatch -> (names, [[Column, ...] per batch])"""
    import pyarrow as pa

    if isinstance(table, pa.RecordBatch):
        table = pa.Table.from_batches([table])
    names = table.column_names
    batches = []
    def view(arr):
        try:
            return Column.from_arrow(arr)
        except TgxError:
            # a type outside the path (lists, structs, ...): its validity bitmap and length travel all the same --
            # completeness / size checks need nothing else -- and a check that reads its values fails with the library's
            # own error ("values is NULL")
            return Column.validity_only(arr)

    for rb in table.to_batches():
        batches.append([view(rb.column(i)) for i in range(rb.num_columns)])
    if not batches:
        batches = []
    return names, batches


class ValidationSuite:
    def __init__(self, spec):
        self.spec = spec

    @staticmethod
    def builder(name):
        return ValidationSuiteBuilder(name)

    def name(self): return self.spec["name"]

    def run(self, table, tables=None):
        """table: dict name -> term_amd.Column (one batch), a list of such dicts (batches), a pyarrow Table /
        RecordBatch, or None (no table registered).  tables: {name: table} of further tables, each registered under its
        name beside the suite's own (which is registered under the suite's table_name): what cross-table constraints
        read."""
        name_arr, n_cols, col_arr, n_batches, _keep = _flatten_table(table)
        out = C.c_char_p()
        err = _Error()
        spec = self.spec
        declared = _arrow_type_names(table)
        if declared:  # (what the builder declared wins)
            spec = dict(spec, column_types=dict(declared, **spec.get("column_types", {})))
        if tables is None:
            _host_check(_host().tgx_host_run_suite_json(json.dumps(spec).encode(), name_arr, n_cols, col_arr,
                                                        n_batches, C.byref(out), C.byref(err)), err)
            return ValidationResult(_take(out))
        flat = [] if n_cols == 0 else [(spec.get("table_name", "data"), name_arr, n_cols, col_arr, n_batches, _keep)]
        further = {}
        for name, t in tables.items():
            flat.append((name,) + tuple(_flatten_table(t)))
            # (what the layout does not say: a Binary column arrives in a string layout)
            binary = {c: kind for c, kind in _arrow_type_names(t).items() if kind == "Binary"}
            if binary:
                further[name] = binary
        if further:
            spec = dict(spec, table_column_types=further)
        arr = (_HostTable * max(1, len(flat)))()
        for slot, (name, names, nc, cols, nb, _k) in zip(arr, flat):
            slot.name = name.encode()
            slot.column_names = C.cast(names, C.POINTER(C.c_char_p))
            slot.n_columns = nc
            slot.columns = C.cast(cols, C.POINTER(_Column))
            slot.n_batches = nb
        _host_check(_host().tgx_host_run_suite_tables_json(json.dumps(spec).encode(), arr, len(flat), C.byref(out),
                                                           C.byref(err)), err)
        return ValidationResult(_take(out))  # (`flat` kept every table's buffers alive through the call)


def _arrow_type_names(table):
    """{column: DataType in arrow-rs's Debug spelling} of a pyarrow table (the reference's result-type rule needs the
    type the caller holds, not the 4- / 8-byte layout it is handed over as); {} for anything else"""
    try:
        import pyarrow as pa
    except ImportError:
        return {}
    if not isinstance(table, (pa.Table, pa.RecordBatch)):
        return {}
    simple = {pa.int8(): "Int8", pa.int16(): "Int16", pa.int32(): "Int32", pa.int64(): "Int64", pa.uint8(): "UInt8",
              pa.uint16(): "UInt16", pa.uint32(): "UInt32", pa.uint64(): "UInt64", pa.float16(): "Float16",
              pa.float32(): "Float32", pa.float64(): "Float64", pa.date32(): "Date32", pa.date64(): "Date64",
              pa.bool_(): "Boolean"}
    out = {}
    for f in table.schema:
        t = f.type
        if t in simple:
            out[f.name] = simple[t]
        elif pa.types.is_timestamp(t):
            unit = {"s": "Second", "ms": "Millisecond", "us": "Microsecond", "ns": "Nanosecond"}[t.unit]
            out[f.name] = "Timestamp(%s, %s)" % (unit, "None" if t.tz is None else 'Some("%s")' % t.tz)
        elif pa.types.is_time(t) or pa.types.is_duration(t) or pa.types.is_decimal(t):
            out[f.name] = str(t)
        elif pa.types.is_binary(t) or pa.types.is_large_binary(t) or pa.types.is_fixed_size_binary(t) or \
                (hasattr(pa.types, "is_binary_view") and pa.types.is_binary_view(t)):
            out[f.name] = "Binary"
    return out


def _arrow_flat(table):
    """pyarrow Table / RecordBatch -> the arguments of the host calls, the column structs filled in place: a table that
    arrives as thousands of 8192-row record batches costs a few microseconds per (batch, column) here instead of the
    11 us a Column object takes (16 M rows x 3 columns as 8192-row batches: 67 ms of Python before the library saw a
    row).  The first batch's columns go through Column.from_arrow -- which knows every layout -- and say what the
    column's chunks are; chunks of fixed-width and string / binary columns are then described from their buffers'
    addresses alone, every other layout keeps taking the long way."""
    import pyarrow as pa

    if isinstance(table, pa.RecordBatch):
        table = pa.Table.from_batches([table])
    names = table.column_names
    batches = table.to_batches()
    n_cols, n_batches = len(names), len(batches)
    col_arr = (_Column * max(1, n_cols * n_batches))()
    keep = [table, batches]
    if n_batches == 0:
        return (C.c_char_p * max(1, n_cols))(*[n.encode() for n in names]), n_cols, col_arr, 0, keep

    def long_way(arr):
        try:
            return Column.from_arrow(arr)
        except TgxError:
            # a type outside the path (lists, structs, ...): its validity bitmap and length travel all the same --
            # completeness / size checks need nothing else -- and a check that reads its values fails with the library's
            # own error ("values is NULL")
            return Column.validity_only(arr)

    lean = []  # per column: None (the long way), ("fixed", type id) or ("string", type id)
    for ci, field in enumerate(table.schema):
        t = field.type
        first = long_way(batches[0].column(ci))
        if pa.types.is_primitive(t) and not pa.types.is_boolean(t) and first.c.values:
            lean.append(("fixed", first.c.type))
        elif (pa.types.is_string(t) or pa.types.is_large_string(t) or pa.types.is_binary(t) or pa.types.is_large_binary(t)) \
                and first.c.type in (_lib.UTF8, _lib.LARGE_UTF8):
            lean.append(("string", first.c.type))
        else:
            lean.append(None)
    import struct

    fmt = struct.Struct("<iiqqqQQQQQQQii")  # tgx_column, field by field (its size is checked below)
    assert fmt.size == C.sizeof(_Column)
    pack, size = fmt.pack_into, fmt.size
    # the columns' chunks are the record batches' columns when every column is cut alike (a table made of record
    # batches is): reading them column by column spares a RecordBatch.column() call per (batch, column), 1 us each
    chunked = [table.column(ci).chunks for ci in range(n_cols)]
    if not all(len(ch) == n_batches and all(len(a) == len(rb) for a, rb in zip(ch, batches)) for ch in chunked):
        chunked = [[rb.column(ci) for rb in batches] for ci in range(n_cols)]
    slow = []  # the slots filled the long way: marked as retained afterwards (the packed ones already are)
    for ci in range(n_cols):
        how = lean[ci]
        at = ci
        for arr in chunked[ci]:
            slot_at = at
            at += n_cols
            bufs = None if how is None else arr.buffers()
            if how is None or bufs[1] is None:  # (an array without rows may come without buffers)
                if how is None or len(arr):
                    col = long_way(arr)
                    keep.append(col)
                    C.memmove(C.byref(col_arr[slot_at]), C.byref(col.c), C.sizeof(_Column))
                else:
                    col_arr[slot_at].type = how[1]
                slow.append(slot_at)
                continue
            nulls = arr.null_count
            validity = bufs[0].address if (nulls and bufs[0] is not None) else 0
            if how[0] == "fixed":
                pack(col_arr, slot_at * size, how[1], MEM_HOST_RETAINED, len(arr), arr.offset, nulls, validity, bufs[1].address, 0, 0, 0, 0, 0, 0, 0)
            else:
                pack(col_arr, slot_at * size, how[1], MEM_HOST_RETAINED, len(arr), arr.offset, nulls, validity, 0, bufs[1].address,
                     bufs[2].address if bufs[2] is not None else 0, 0, 0, 0, 0, 0)
    name_arr = (C.c_char_p * max(1, n_cols))(*[n.encode() for n in names])
    keep.append(_mark_retained(col_arr, slow))
    return name_arr, n_cols, col_arr, n_batches, keep


def _mark_retained(col_arr, which):
    """The host calls run the whole table and return: every buffer handed over is alive and unmodified until then, which
    is all TGX_MEM_HOST_RETAINED asks for -- a table that arrives as 8192-row record batches is then copied by the
    library's copy threads beside the noting of the next batches instead of inside every tgx_update.  (The structs in
    `col_arr` are copies: the caller's Column objects are not touched; a dictionary's struct is copied too.)"""
    dict_copies = []
    for i in (range(which) if isinstance(which, int) else which):
        if col_arr[i].mem != MEM_HOST:
            continue
        if col_arr[i].dictionary:
            if col_arr[i].dictionary.contents.mem != MEM_HOST:
                continue
            d = _Column()
            C.memmove(C.byref(d), col_arr[i].dictionary, C.sizeof(_Column))
            d.mem = MEM_HOST_RETAINED
            dict_copies.append(d)
            col_arr[i].dictionary = C.pointer(d)
        col_arr[i].mem = MEM_HOST_RETAINED
    return dict_copies


def _flatten_table(table):
    if table is None:
        names, batches = [], []
    elif isinstance(table, dict):
        names, batches = list(table.keys()), [list(table.values())]
    elif isinstance(table, (list, tuple)):
        names = list(table[0].keys()) if table else []
        batches = [[b[n] for n in names] for b in table]
    else:
        return _arrow_flat(table)
    n_cols, n_batches = len(names), len(batches)
    name_arr = (C.c_char_p * max(1, n_cols))(*[n.encode() for n in names])
    flat = [c.c for b in batches for c in b]
    col_arr = (_Column * max(1, len(flat)))(*flat)
    return name_arr, n_cols, col_arr, n_batches, (batches, _mark_retained(col_arr, len(flat)))


# ---------------------------------------------------------------------------------------------- analyzers
class _Analyzer:
    """mirror of TG/analyzers/traits.rs Analyzer: name / metric_key / merge_states / compute_metric_from_state"""

    def __init__(self, spec):
        self.spec = spec

    def name(self):
        t = self.spec["type"]
        if t == "grouped_completeness":  # (the wrapper keeps the analyzer's name: grouped.rs:280-282)
            return "completeness"
        return "entropy" if t == "value_entropy" else t  # (the tag "entropy" was taken: see EntropyAnalyzer)

    def metric_key(self):
        t = self.name()
        if t in ("size", "standard_deviation", "histogram", "compliance"):  # (these analyzers do not override metric_key)
            return t
        if t == "correlation":
            return "correlation_%s_%s_%s" % (self.spec.get("method", "pearson"), self.spec["column1"], self.spec["column2"])
        if t == "mutual_information":
            return "mutual_information_%s_%s" % (self.spec["column1"], self.spec["column2"])
        if self.spec["type"] == "grouped_completeness":  # grouped.rs:288-294
            return "completeness.%s_grouped_by_%s" % (self.spec["column"], "_".join(self.spec["group_by"]))
        return "%s.%s" % (t, self.spec["column"])

    def with_grouping(self, config):
        """TG/analyzers/grouped.rs GroupedAnalyzer::with_grouping: the analyzer's metric per group of config.columns.  The
        reference implements it for CompletenessAnalyzer alone (basic/grouped_completeness.rs), and so does this"""
        if self.spec["type"] != "completeness":
            raise TypeError("with_grouping: only CompletenessAnalyzer has a grouped form (the reference implements "
                            "GroupedAnalyzer for it alone), not %s" % self.name())
        spec = {"type": "grouped_completeness", "column": self.spec["column"], "group_by": list(config.columns),
                "max_groups": config.max_groups, "include_overall": bool(config.include_overall)}
        if not config.strict_reference_types:
            spec["strict_reference_types"] = False
        if config.composite_on_device:
            spec["composite_groups_on_device"] = True
        return _Analyzer(spec)

    def state_text_from_group_counts(self, summary, entries):
        """the state (the bytes the library wrote) a grouped_completeness analyzer builds from given group counts:
        `entries` is a list of (key, total, non_null) in the library's order, a key being str / bytes or int"""
        key = lambda k: list(k) if isinstance(k, (bytes, bytearray)) else k  # noqa: E731
        doc = {"summary": summary, "entries": [[key(k), t, n] for k, t, n in entries]}
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_group_counts_state_json(json.dumps(self.spec).encode(), json.dumps(doc).encode(),
                                                             C.byref(out), C.byref(err)), err)
        return _take(out)

    def merge_states(self, states):
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_merge_states_json(json.dumps(self.spec).encode(), json.dumps(states).encode(),
                                                       C.byref(out), C.byref(err)), err)
        return json.loads(_take(out))

    def merge_states_text(self, states):
        """merge_states, but the bytes the library wrote (what serde_json would be handed)"""
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_merge_states_json(json.dumps(self.spec).encode(), json.dumps(states).encode(),
                                                       C.byref(out), C.byref(err)), err)
        return _take(out)

    def planned_requests(self, column_types):
        """what the analyzer plans for columns of the given tgx_types (parallel to its columns): a list of dicts with
        kind, column, column2 and, for a PAIR_COUNTS request, pair_counts"""
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_analyzer_plan_json(json.dumps(self.spec).encode(), json.dumps(list(column_types)).encode(),
                                                        C.byref(out), C.byref(err)), err)
        return json.loads(_take(out))["requests"]

    def state_text_from_pair_counts(self, summary, entries):
        """the state (the bytes the library wrote) a mutual_information analyzer builds from given pair counts: `entries`
        is a list of (x, y, count) in the library's order, a cell being str / bytes (a value) or int (a bin)"""
        cell = lambda c: list(c) if isinstance(c, (bytes, bytearray)) else c  # noqa: E731
        doc = {"summary": summary, "entries": [[cell(x), cell(y), n] for x, y, n in entries]}
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_pair_counts_state_json(json.dumps(self.spec).encode(), json.dumps(doc).encode(),
                                                            C.byref(out), C.byref(err)), err)
        return _take(out)

    def state_text_from_type_classes(self, counts):
        """the state (the bytes the library wrote) a data_type analyzer builds from given counts: the dict of
        State.type_classes (a string column), or {"results": [{"total", "non_null", "matches"}, ..]}, the results that
        answer what the analyzer plans for an integer or a float column"""
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_data_type_state_json(json.dumps(self.spec).encode(), json.dumps(counts).encode(),
                                                          C.byref(out), C.byref(err)), err)
        return _take(out)

    def compute_metric_from_state(self, state):
        """-> MetricValue as {"type": "Double"|"Long"|"Map", "value": ...}; raises TgxError with the
        reference's AnalyzerError text (e.g. 'No data available for analysis')"""
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_metric_from_state_json(json.dumps(self.spec).encode(), json.dumps(state).encode(),
                                                            C.byref(out), C.byref(err)), err)
        return json.loads(_take(out))


class GroupingConfig:
    """TG/analyzers/grouped.rs:14-66 GroupingConfig: the group columns, max_groups (default 10000: the first max_groups
    groups by the metric, descending, are kept; also the bound of the table on the device, capped at
    GROUP_COUNTS_MAX_GROUPS), include_overall (default true) and the overflow strategy, which the reference carries and
    never reads.  strict_reference_types (default true): only a group column declared Utf8 is taken, the one type the
    reference reads by value; off, strings of every layout group by value and integers print as decimal text.
    composite_groups_on_device (default false, an opt-in): 2 .. 8 group columns are one GROUP_COUNTS walk on the tuple
    of the columns; off, more than one group column is the analyzer's error"""

    def __init__(self, columns, max_groups=10000, include_overall=True, overflow_strategy="TopK",
                 strict_reference_types=True, composite_groups_on_device=False):
        self.columns = [columns] if isinstance(columns, str) else list(columns)
        self.max_groups, self.include_overall = max_groups, include_overall
        self.overflow_strategy, self.strict_reference_types = overflow_strategy, strict_reference_types
        self.composite_on_device = bool(composite_groups_on_device)

    def composite_groups_on_device(self, on=True):
        self.composite_on_device = bool(on)
        return self

    def with_max_groups(self, n):
        self.max_groups = int(n)
        return self

    def with_overall(self, include):
        self.include_overall = bool(include)
        return self

    def with_overflow_strategy(self, strategy):
        self.overflow_strategy = strategy
        return self


def SizeAnalyzer(): return _Analyzer({"type": "size"})
def CompletenessAnalyzer(column): return _Analyzer({"type": "completeness", "column": column})
def DistinctnessAnalyzer(column): return _Analyzer({"type": "distinctness", "column": column})
def ApproxCountDistinctAnalyzer(column): return _Analyzer({"type": "approx_count_distinct", "column": column})
def MeanAnalyzer(column): return _Analyzer({"type": "mean", "column": column})
def MinAnalyzer(column): return _Analyzer({"type": "min", "column": column})
def MaxAnalyzer(column): return _Analyzer({"type": "max", "column": column})
def SumAnalyzer(column): return _Analyzer({"type": "sum", "column": column})
def StandardDeviationAnalyzer(column): return _Analyzer({"type": "standard_deviation", "column": column})


def CorrelationAnalyzer(column1, column2, method="pearson"):
    return _Analyzer({"type": "correlation", "column1": column1, "column2": column2, "method": method})


def MutualInformationAnalyzer(column1, column2, bins=10, max_pairs=None, max_value_bytes=None, arrow_types=None):
    """TG/analyzers/advanced/mutual_information.rs, numeric x numeric pairs: two passes on the device (the range of
    both columns, then the joint bin counts); `bins` = max(bins, 2), at most JOINT_MAX_BINS (include/tgx.h).
    `max_pairs` opts into the reference's three categorical branches (TGX_CHECK_PAIR_COUNTS): with it a pair with at
    least one string column is counted by (value, value) or (bin, value) -- string x string in one pass, a mixed pair in
    two -- for up to max_pairs distinct pairs of values of up to `max_value_bytes` (default 256) bytes; beyond the
    bounds, for a column declared binary and for a string value that may parse as a number (the reference would bin
    such a column) the analyzer fails with its own error.  Without it the analyzer does what it always did.
    `arrow_types`: the two columns' Arrow DataTypes where the table is not a pyarrow one"""
    spec = {"type": "mutual_information", "column1": column1, "column2": column2, "bins": max(int(bins), 2)}
    if max_pairs is not None:
        spec["max_pairs"] = int(max_pairs)
        if max_value_bytes is not None:
            spec["max_value_bytes"] = int(max_value_bytes)
    if arrow_types is not None:
        spec["arrow_types"] = list(arrow_types)
    return _Analyzer(spec)


def HistogramAnalyzer(column, num_buckets=10, strict_reference_types=True):
    """TG/analyzers/advanced/histogram.rs: two passes on the device (MIN / MAX / COUNT / SUM / SUM of squares, then the
    counts of `num_buckets` equal-width buckets, clamped to 1..1000); the metric is a MetricValue of type "Histogram".
    The reference reads MIN as Float64 only, so a column of another type is the analyzer's error unless
    `strict_reference_types` is off (then it runs CAST AS DOUBLE)"""
    spec = {"type": "histogram", "column": column, "num_buckets": min(max(int(num_buckets), 1), _lib.HISTOGRAM_MAX_BUCKETS)}
    if not strict_reference_types:
        spec["strict_reference_types"] = False
    return _Analyzer(spec)


COMPLIANCE_FORBIDDEN = ("drop", "delete", "insert", "update", "create", "alter", "grant", "revoke", "exec", "execute",
                        "union", "select", "--", "/*", "*/")


def compliance_forbidden_keyword(predicate):
    """ComplianceAnalyzer::validate_predicate (advanced/compliance.rs:88-108): the first forbidden keyword, in the list's
    order, that the lower-cased predicate CONTAINS (a substring test: `created_at` holds `create`), or None"""
    lower = predicate.lower()
    return next((w for w in COMPLIANCE_FORBIDDEN if w in lower), None)


def ComplianceAnalyzer(name, predicate, string_functions_on_device=False):
    """advanced/compliance.rs:37-204: the fraction of rows on which `predicate` is TRUE, counted on the device under the
    library's closed predicate subset (TGX_CHECK_ROW_PREDICATE).  State {"compliant_count", "total_count"}; the metric is
    a Double, 1.0 on an empty table; metric_key is "compliance".  A forbidden keyword or a predicate outside the subset
    is the analyzer's error when it runs, as the reference validates in compute_state_from_data.
    string_functions_on_device: CustomSqlConstraint's opt-in of that name (LIKE, LENGTH, TRIM(c) = '', string order)"""
    spec = {"type": "compliance", "name": name, "predicate": predicate}
    if string_functions_on_device:
        spec["string_functions_on_device"] = True
    return _Analyzer(spec)


def EntropyAnalyzer(column, max_unique_values=10000, arrow_type=None):
    """TG/analyzers/advanced/entropy.rs over TGX_CHECK_VALUE_COUNTS: entropy (bits), normalized entropy, Gini impurity,
    effective and unique values, the ten most frequent values; the state is {value_counts, total_count, truncated}.
    name() is "entropy"; the JSON tag is "value_entropy" ("entropy" is what the tests of unknown analyzer types use).
    A column with more than max(max_unique_values, 10) values is the analyzer's error, with the numbers: the reference's
    truncated top-N sampling is not reproduced.  `arrow_type`: the column's Arrow DataType where the table is not a
    pyarrow one (a date, time, float, decimal, boolean or binary column is the analyzer's error)"""
    spec = {"type": "value_entropy", "column": column, "max_unique_values": max(int(max_unique_values), 10)}
    if arrow_type:
        spec["arrow_type"] = arrow_type
    return _Analyzer(spec)


def DataTypeAnalyzer(column, arrow_type=None):
    """TG/analyzers/advanced/data_type.rs: how many non-NULL values of `column` read as boolean, integer, double, date
    or string.  A string column is classified on the device (TGX_CHECK_TYPE_CLASSES: syntactic classes, include/tgx.h;
    DATETIME values count as "date"); a declared integer column takes two VALUE_RULE range counts, a float column a
    COUNT.  State {"type_counts": {label: n}, "total_count": n}, a label without rows absent; the metric is a Map of
    Long; metric_key is "data_type.<column>".  Values that look like dates in a form the device does not decide, and a
    declared temporal, decimal, boolean, binary or UInt64 column, are the analyzer's own error.  `arrow_type`: the
    column's Arrow DataType where the table is not a pyarrow one"""
    spec = {"type": "data_type", "column": column}
    if arrow_type:
        spec["arrow_type"] = arrow_type
    return _Analyzer(spec)


def data_type_dominant_type(state):
    """DataTypeState::dominant_type (data_type.rs:71-79): (label, fraction) of the most common type, or None"""
    if not state["type_counts"]:
        return None
    label, count = max(state["type_counts"].items(), key=lambda kv: kv[1])
    return label, count / state["total_count"]


def data_type_consistency(state):
    """DataTypeState::type_consistency (data_type.rs:82-90): 1.0 without rows, else the dominant type's fraction"""
    if state["total_count"] == 0:
        return 1.0
    top = data_type_dominant_type(state)
    return top[1] if top else 0.0


class AnalyzerContext:
    """TG/analyzers/context.rs: metrics by key, errors; plus the analyzers' states (for merges across shards)"""

    def __init__(self, text):
        d = json.loads(text)
        self.text = text  # as written by the library (integer / float token kinds matter to serde_json readers)
        self.metrics, self.states, self._errors = d["metrics"], d["states"], d["errors"]

    def get_metric(self, key):
        return self.metrics.get(key)

    def has_errors(self):
        return bool(self._errors)

    def errors(self):
        return self._errors


class AnalysisRunner:
    """TG/analyzers/runner.rs:64-202 -- but ONE pass over the table for all analyzers"""

    def __init__(self):
        self._analyzers, self._continue, self._table = [], True, "data"

    def add(self, analyzer):
        self._analyzers.append(analyzer)
        return self

    def continue_on_error(self, flag):
        self._continue = bool(flag)
        return self

    def table_name(self, name):
        self._table = name
        return self

    def analyzer_count(self):
        return len(self._analyzers)

    def run(self, table):
        declared = _arrow_type_names(table)  # (analyzers that read a column's values as text need its Arrow type)
        specs = [dict(a.spec, arrow_type=declared[a.spec["column"]])
                 if a.spec["type"] in ("value_entropy", "data_type") and "arrow_type" not in a.spec and a.spec["column"] in declared
                 else dict(a.spec, arrow_types=[declared.get(a.spec["column1"], ""), declared.get(a.spec["column2"], "")])
                 if a.spec["type"] == "mutual_information" and "max_pairs" in a.spec and "arrow_types" not in a.spec
                 else dict(a.spec, group_arrow_type=declared[a.spec["group_by"][0]])
                 if a.spec["type"] == "grouped_completeness" and len(a.spec["group_by"]) == 1 and
                 a.spec["group_by"][0] in declared and "group_arrow_type" not in a.spec
                 else dict(a.spec, group_arrow_types=[declared.get(g, "") for g in a.spec["group_by"]])
                 if a.spec["type"] == "grouped_completeness" and len(a.spec["group_by"]) > 1 and
                 "group_arrow_types" not in a.spec
                 else a.spec for a in self._analyzers]
        spec = {"table_name": self._table, "continue_on_error": self._continue, "analyzers": specs}
        name_arr, n_cols, col_arr, n_batches, _keep = _flatten_table(table)
        out = C.c_char_p()
        err = _Error()
        _host_check(_host().tgx_host_run_analysis_json(json.dumps(spec).encode(), name_arr, n_cols, col_arr, n_batches,
                                                       C.byref(out), C.byref(err)), err)
        return AnalyzerContext(_take(out))


# ---------------------------------------------------------------------------------------------- bridge
_HOST = None


class _HostTable(C.Structure):
    """tgx_host_table (include/tgx_host.h)"""
    _fields_ = [("name", C.c_char_p), ("column_names", C.POINTER(C.c_char_p)), ("n_columns", C.c_size_t),
                ("columns", C.POINTER(_Column)), ("n_batches", C.c_size_t)]


def _host():
    global _HOST
    if _HOST is None:
        L = _lib.lib()
        E = C.POINTER(_Error)
        L.tgx_host_run_suite_json.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(_Column),
                                              C.c_size_t, C.POINTER(C.c_char_p), E]
        L.tgx_host_constraint_plan_json.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_constraint_verdict_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_temporal_params_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_value_rule_params_json.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_row_predicate_json.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_row_predicate_json_ex.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_validate_identifier.argtypes = [C.c_char_p, E]
        L.tgx_host_assertion_json.argtypes = [C.c_char_p, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), E]
        L.tgx_host_run_analysis_json.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(_Column),
                                                 C.c_size_t, C.POINTER(C.c_char_p), E]
        L.tgx_host_merge_states_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_metric_from_state_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_analyzer_plan_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_pair_counts_state_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_group_counts_state_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_data_type_state_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_run_suite_tables_json.argtypes = [C.c_char_p, C.POINTER(_HostTable), C.c_size_t,
                                                     C.POINTER(C.c_char_p), E]
        L.tgx_host_cross_table_sum_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_foreign_key_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_join_coverage_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), E]
        L.tgx_host_free.argtypes = [C.c_void_p]
        L.tgx_host_free.restype = None
        _HOST = L
    return _HOST


def _host_check(status, err):
    if status != 0:
        raise TgxError(status, err.msg.decode("utf-8", "replace"))


def _take(out):
    text = out.value.decode("utf-8")
    _host().tgx_host_free(C.cast(out, C.c_void_p))
    return text


def constraint_plan(constraint):
    """the aggregates one constraint (a dict as CheckBuilder builds them) asks for"""
    out = C.c_char_p()
    err = _Error()
    _host_check(_host().tgx_host_constraint_plan_json(json.dumps(constraint).encode(), C.byref(out), C.byref(err)), err)
    return json.loads(_take(out))


def constraint_verdict(constraint, results):
    """Constraint::evaluate's verdict half on given aggregates (list of dicts with tgx_result field names)"""
    out = C.c_char_p()
    err = _Error()
    _host_check(_host().tgx_host_constraint_verdict_json(json.dumps(constraint).encode(), json.dumps(results).encode(),
                                                         C.byref(out), C.byref(err)), err)
    return json.loads(_take(out))


def temporal_params(constraint, arrow_types):
    """a temporal_ordering constraint (its dict) + {column: Arrow DataType name} -> the tgx_temporal_params of its
    TEMPORAL spec as a dict (tgx_host_temporal_params_json) -- for max_time_gap with window_on_device, the
    tgx_time_gap_params of its TIME_GAP spec ({column, column2, kind, max_gap, flags}); TgxError with the constraint's
    error text otherwise"""
    out = C.c_char_p()
    err = _Error()
    _host_check(_host().tgx_host_temporal_params_json(json.dumps(constraint).encode(), json.dumps(arrow_types).encode(),
                                                      C.byref(out), C.byref(err)), err)
    return json.loads(_take(out))


def value_rule_params(constraint):
    """a datatype constraint with a numeric validation (its dict) -> the tgx_value_rule_params of its VALUE_RULE spec as
    a dict ({column, kind, mode, flags, lo_i, hi_i, lo_f, hi_f}; tgx_host_value_rule_params_json); TgxError with the
    constraint's error text for what stays off the device"""
    out = C.c_char_p()
    err = _Error()
    _host_check(_host().tgx_host_value_rule_params_json(json.dumps(constraint).encode(), C.byref(out), C.byref(err)), err)
    return json.loads(_take(out))


def row_predicate(expression, string_functions=False):
    """what the predicate compiler of Check.satisfies / ComplianceAnalyzer makes of `expression`
    (tgx_host_row_predicate_json): {"columns", "leaves", "program", "literals_hex"}; TgxError (TGX_UNSUPPORTED) naming
    the first thing outside the subset otherwise.  string_functions: compile under the dialect of that name
    (tgx_host_row_predicate_json_ex), what string_functions_on_device opts into.  Needs no device"""
    out = C.c_char_p()
    err = _Error()
    if string_functions:
        options = json.dumps({"string_functions": True}).encode()
        _host_check(_host().tgx_host_row_predicate_json_ex(expression.encode(), options, C.byref(out), C.byref(err)), err)
    else:
        _host_check(_host().tgx_host_row_predicate_json(expression.encode(), C.byref(out), C.byref(err)), err)
    return json.loads(_take(out))


def validate_identifier(identifier):
    err = _Error()
    _host_check(_host().tgx_host_validate_identifier(identifier.encode(), C.byref(err)), err)


# ---------------------------------------------------------------------------------------------- incremental analysis
class InMemoryStateStore:
    """TG/analyzers/incremental/state_store.rs StateStore: partition -> {metric_key: state}"""

    def __init__(self):
        self._p = {}

    def load_state(self, partition):
        return dict(self._p.get(partition, {}))

    def save_state(self, partition, state_map):
        self._p[partition] = dict(state_map)

    def list_partitions(self):
        return sorted(self._p)

    def delete_partition(self, partition):
        self._p.pop(partition, None)


class FileSystemStateStore:
    """state_store.rs:37-190: <base>/<partition>/<metric_key>.json, each file the serde_json form of the analyzer's
    state struct -- the states produced here use the reference's field names, so a directory written by either side
    can be read by the other."""

    def __init__(self, base_path):
        import os

        self._base = str(base_path)
        os.makedirs(self._base, exist_ok=True)

    def _dir(self, partition):
        import os

        return os.path.join(self._base, partition)

    def load_state(self, partition):
        import os

        out, d = {}, self._dir(partition)
        if not os.path.isdir(d):
            return out
        for name in sorted(os.listdir(d)):
            if name.endswith(".json"):
                with open(os.path.join(d, name)) as f:
                    out[name[:-5]] = json.load(f)
        return out

    def save_state(self, partition, state_map):
        import os

        d = self._dir(partition)
        os.makedirs(d, exist_ok=True)
        for key, state in state_map.items():
            with open(os.path.join(d, key + ".json"), "w") as f:
                json.dump(state, f)

    def list_partitions(self):
        import os

        return sorted(n for n in os.listdir(self._base) if os.path.isdir(os.path.join(self._base, n)))

    def delete_partition(self, partition):
        import shutil

        shutil.rmtree(self._dir(partition), ignore_errors=True)


def _state_is_empty(analyzer, state):
    """AnalyzerState::is_empty of the mirrored state types"""
    t = analyzer.spec["type"]
    if t in ("size", "mean", "standard_deviation"):
        return state.get("count", 0) == 0
    if t in ("completeness", "distinctness", "approx_count_distinct", "data_type"):
        return state.get("total_count", 0) == 0
    if t in ("min", "max"):
        return state.get("min") is None and state.get("max") is None
    if t == "sum":
        return not state.get("has_values", False)
    return False  # correlation: the trait default


class IncrementalAnalysisRunner:
    """TG/analyzers/incremental/runner.rs:102-430.  Each partition's states come from ONE fused pass on the GPU
    (AnalysisRunner); merging and metrics are the reference's state algebra (csrc/host/analyzers.cpp)."""

    def __init__(self, state_store, fail_fast=True, save_empty_states=False, max_merge_batch_size=100):
        self._store, self._analyzers = state_store, []
        self._fail_fast, self._save_empty, self._batch = fail_fast, save_empty_states, max_merge_batch_size

    def add_analyzer(self, analyzer):
        self._analyzers.append(analyzer)
        return self

    def analyzer_count(self):
        return len(self._analyzers)

    def list_partitions(self):
        return self._store.list_partitions()

    def delete_partition(self, partition):
        self._store.delete_partition(partition)

    def _fresh(self, table):
        r = AnalysisRunner().continue_on_error(True)
        for a in self._analyzers:
            r.add(a)
        ctx = r.run(table)
        if ctx.has_errors() and self._fail_fast:
            raise TgxError(1, ctx.errors()[0]["error"])
        return ctx

    def analyze_partition(self, table, partition):
        """runner.rs:139-213: states of `table` saved under `partition`, metrics returned"""
        ctx = self._fresh(table)
        states = {a.metric_key(): ctx.states[a.metric_key()] for a in self._analyzers if a.metric_key() in ctx.states}
        self._store.save_state(partition, {k: v for k, v in states.items()
                                           if self._save_empty or not _state_is_empty(self._by_key(k), v)})
        return ctx

    def _by_key(self, key):
        return next(a for a in self._analyzers if a.metric_key() == key)

    def _finish(self, merged_by_key, errors):
        metrics = {}
        for a in self._analyzers:
            key = a.metric_key()
            if key not in merged_by_key:
                continue
            try:
                metrics[key] = a.compute_metric_from_state(merged_by_key[key])
            except TgxError as e:
                if self._fail_fast:
                    raise
                errors.append({"analyzer_name": a.name(), "error": e.msg})
        return AnalyzerContext(json.dumps({"metrics": metrics, "states": merged_by_key, "errors": errors}))

    def analyze_incremental(self, table, partition):
        """runner.rs:216-317: new data's states merged into the partition's stored states"""
        existing = self._store.load_state(partition)
        ctx = self._fresh(table)
        merged, errors = {}, list(ctx.errors())
        for a in self._analyzers:
            key = a.metric_key()
            if key not in ctx.states:
                continue
            new = ctx.states[key]
            try:
                merged[key] = a.merge_states([existing[key], new]) if key in existing else new
            except TgxError as e:
                if self._fail_fast:
                    raise
                errors.append({"analyzer_name": a.name(), "error": e.msg})
        self._store.save_state(partition, {k: v for k, v in merged.items()
                                           if self._save_empty or not _state_is_empty(self._by_key(k), v)})
        return self._finish(merged, errors)

    def analyze_partitions(self, partitions):
        """runner.rs:320-414: metrics over the union of stored partitions, no data access"""
        partitions = list(partitions)
        by_key, errors = {}, []
        for i in range(0, len(partitions), self._batch):
            for p in partitions[i:i + self._batch]:
                for key, st in self._store.load_state(p).items():
                    by_key.setdefault(key, []).append(st)
        merged = {}
        for a in self._analyzers:
            key = a.metric_key()
            if not by_key.get(key):
                continue
            try:
                merged[key] = a.merge_states(by_key[key])
            except TgxError as e:
                if self._fail_fast:
                    raise
                errors.append({"analyzer_name": a.name(), "error": e.msg})
        return self._finish(merged, errors)

