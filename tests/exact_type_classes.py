"""An exact reference for TGX_CHECK_TYPE_CLASSES, written from the contract comment in include/tgx.h and from nothing
else: classify() walks a value's bytes by hand, classify_re() states the same seven rules a second time with `re` and
`datetime`; the two are held equal on the edge table and on seeded strings (tests/test_exact_type_classes.py).  EDGES is
the hand-listed table with the class each value must get; counts() is what a column's nine counters must be."""
import datetime
import random
import re

BOOLEAN, INTEGER, DOUBLE, DATE, DATETIME, STRING, UNDECIDED = range(7)
NAMES = ("boolean", "integer", "double", "date", "datetime", "string", "undecided")
COUNTERS = ("seen", "non_null") + tuple(n + "_rows" for n in NAMES)

_DIGITS = b"0123456789"


def _is_digit(c):
    return 0x30 <= c <= 0x39


def _lower(b):
    """ASCII case folding only: bytes at or above 0x80 stay as they are"""
    return bytes(c + 32 if 0x41 <= c <= 0x5A else c for c in b)


def _valid_date(y, m, d):
    if not 1 <= m <= 12 or d < 1:
        return False
    leap = y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)
    return d <= (31, 29 if leap else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[m - 1]


def _all_digits(b):
    return len(b) > 0 and all(_is_digit(c) for c in b)


def _is_boolean(v):
    return v in (b"0", b"1") or _lower(v) in (b"true", b"false")


def _is_integer(v):
    body = v[1:] if v[:1] == b"-" else v
    if not _all_digits(body):
        return False
    if body == b"0":
        return v == b"0"  # (-0 is not canonical)
    if body[0] == 0x30:
        return False
    if len(body) > 10:
        return False
    n = int(body)
    return n <= (1 << 31) if v[:1] == b"-" else n <= (1 << 31) - 1


def _is_double(v):
    i = 1 if v[:1] in (b"+", b"-") else 0
    rest = v[i:]
    if _lower(rest) in (b"nan", b"inf", b"infinity"):
        return True
    # mantissa
    j, n_int = 0, 0
    while j < len(rest) and _is_digit(rest[j]):
        j, n_int = j + 1, n_int + 1
    n_frac = 0
    if j < len(rest) and rest[j] == 0x2E:
        j += 1
        while j < len(rest) and _is_digit(rest[j]):
            j, n_frac = j + 1, n_frac + 1
    if n_int + n_frac == 0:
        return False
    if j == len(rest):
        return True
    if rest[j] not in b"eE":
        return False
    j += 1
    if j < len(rest) and rest[j] in b"+-":
        j += 1
    return _all_digits(rest[j:])


def _date_fields(v):
    """DDDD-D{1,2}-D{1,2} -> (y, m, d), or None"""
    parts = v.split(b"-")
    if len(parts) != 3 or len(parts[0]) != 4 or not 1 <= len(parts[1]) <= 2 or not 1 <= len(parts[2]) <= 2:
        return None
    if not all(_all_digits(p) for p in parts):
        return None
    return int(parts[0]), int(parts[1]), int(parts[2])


def _is_date(v):
    if len(v) > 10:
        return False
    f = _date_fields(v)
    return f is not None and _valid_date(*f)


def _two(b):
    return int(b) if len(b) == 2 and _all_digits(b) else None


def _is_datetime(v):
    if len(v) <= 10 or len(v) < 19:
        return False
    year, month, day = v[0:4], _two(v[5:7]), _two(v[8:10])  # DDDD-DD-DD
    if not _all_digits(year) or v[4:5] != b"-" or v[7:8] != b"-" or None in (month, day):
        return False
    if not _valid_date(int(year), month, day):
        return False
    if v[10:11] not in (b"T", b" "):
        return False
    hh, mm, ss = _two(v[11:13]), _two(v[14:16]), _two(v[17:19])
    if v[13:14] != b":" or v[16:17] != b":" or None in (hh, mm, ss) or hh > 23 or mm > 59 or ss > 59:
        return False
    rest = v[19:]
    if rest[:1] == b".":
        k = 1
        while k < len(rest) and _is_digit(rest[k]):
            k += 1
        if not 1 <= k - 1 <= 9:
            return False
        rest = rest[k:]
    if rest in (b"", b"Z"):
        return True
    if len(rest) != 6 or rest[:1] not in (b"+", b"-") or rest[3:4] != b":":
        return False
    oh, om = _two(rest[1:3]), _two(rest[4:6])
    return None not in (oh, om) and oh <= 23 and om <= 59


def _looks_like_a_date(v):
    """begins DDDD- or [+-]D{4,}-"""
    if len(v) >= 5 and _all_digits(v[:4]) and v[4:5] == b"-":
        return True
    if v[:1] in (b"+", b"-"):
        k = 1
        while k < len(v) and _is_digit(v[k]):
            k += 1
        return k - 1 >= 4 and v[k:k + 1] == b"-"
    return False


def classify(v):
    """the class of the bytes `v`: the seven rules in the contract's order, the first that fits"""
    v = bytes(v)
    for cls, fits in ((BOOLEAN, _is_boolean), (INTEGER, _is_integer), (DOUBLE, _is_double), (DATE, _is_date),
                      (DATETIME, _is_datetime), (UNDECIDED, _looks_like_a_date)):
        if fits(v):
            return cls
    return STRING


# ---- the twin: the same contract through `re` and `datetime` -------------------------------------------------------------
_RE_BOOL = re.compile(rb"\A(?:[01]|[tT][rR][uU][eE]|[fF][aA][lL][sS][eE])\Z")
_RE_INT = re.compile(rb"\A(?:0|-?[1-9][0-9]*)\Z")
_RE_DOUBLE = re.compile(rb"\A[+-]?(?:(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[nN][aA][nN]|"
                        rb"[iI][nN][fF](?:[iI][nN][iI][tT][yY])?)\Z")
_RE_DATE = re.compile(rb"\A([0-9]{4})-([0-9]{1,2})-([0-9]{1,2})\Z")
_RE_DATETIME = re.compile(rb"\A([0-9]{4})-([0-9]{2})-([0-9]{2})[T ]([0-9]{2}):([0-9]{2}):([0-9]{2})(?:\.[0-9]{1,9})?"
                          rb"(?:Z|[+-]([0-9]{2}):([0-9]{2}))?\Z")
_RE_UNDECIDED = re.compile(rb"\A(?:[0-9]{4}-|[+-][0-9]{4,}-)")


def _calendar_day(y, m, d):
    if y == 0:  # datetime starts at year 1; year 0 has the calendar of year 400 (a leap year)
        y = 400
    try:
        datetime.date(y, m, d)
        return True
    except ValueError:
        return False


def classify_re(v):
    v = bytes(v)
    if _RE_BOOL.match(v):
        return BOOLEAN
    if _RE_INT.match(v) and -(1 << 31) <= int(v) <= (1 << 31) - 1:
        return INTEGER
    if _RE_DOUBLE.match(v):
        return DOUBLE
    m = _RE_DATE.match(v)
    if m and len(v) <= 10 and _calendar_day(*(int(g) for g in m.groups())):
        return DATE
    m = _RE_DATETIME.match(v)
    if m and len(v) > 10:
        y, mo, d, hh, mm, ss = (int(g) for g in m.groups()[:6])
        offset_ok = m.group(7) is None or (int(m.group(7)) <= 23 and int(m.group(8)) <= 59)
        if _calendar_day(y, mo, d) and hh <= 23 and mm <= 59 and ss <= 59 and offset_ok:
            return DATETIME
    if _RE_UNDECIDED.match(v):
        return UNDECIDED
    return STRING


# ---- the edge table -------------------------------------------------------------------------------------------------------
_B, _I, _F, _D, _T, _S, _U = BOOLEAN, INTEGER, DOUBLE, DATE, DATETIME, STRING, UNDECIDED
EDGES = [
    (b"0", _B), (b"1", _B), (b"2", _I), (b"-1", _I), (b"-0", _F), (b"+5", _F), (b"007", _F), (b"2147483647", _I),
    (b"2147483648", _F), (b"-2147483648", _I), (b"-2147483649", _F), (b"00", _F), (b"+0", _F), (b"-", _S), (b"+", _S),
    (b"9999999999", _F), (b"10000000000", _F), (b"-1234567890123", _F), (b"1 ", _S), (b" 1", _S),
    (b"true", _B), (b"TRUE", _B), (b"tRuE", _B), (b"truE ", _S), ("falſe".encode(), _S), (b"yes", _S), (b"t", _S),
    (b"false", _B), (b"FALSE", _B), (b"False", _B), (b"fals", _S), (b"falsee", _S), (b"tru", _S), (b"truee", _S),
    (b"f", _S), (b"T", _S), (b"no", _S), (b"n", _S), (b"i", _S),
    (b"1.", _F), (b".5", _F), (b".", _S), (b"1e", _S), (b"1e5", _F), (b"1E+5", _F), (b"e5", _S), (b"+.5e-3", _F),
    (b"nan", _F), (b"-NaN", _F), (b"+inf", _F), (b"Infinity", _F), (b"infinit", _S), (b"1_0", _S), (b"0x10", _S),
    (b"-infinity", _F), (b"INF", _F), (b"nan ", _S), (b"nanx", _S), (b"infinityy", _S), (b"+-1", _S), (b"--1", _S),
    (b"1e+", _S), (b"1e-", _S), (b"1e5.", _S), (b"1.5.3", _S), (b"1.e5", _F), (b".e5", _S), (b"-.", _S), (b"+.", _S),
    (b"1.5e10", _F), (b"1.5E-10", _F), (b"1e5x", _S), (b"0.0", _F), (b"-0.0", _F), (b"1,5", _S), (b"1d5", _S),
    (b"12345678", _I), (b"123456789", _I), (b"1234567.5", _F), (b"\xc3\xa9", _S), (b"1\xff", _S), (b"\x80", _S),
    (b"2023-01-01", _D), (b"2023-1-5", _D), (b"2023-02-29", _U), (b"2024-02-29", _D), (b"1900-02-29", _U),
    (b"2000-02-29", _D), (b"0000-02-29", _D), (b"2023-13-01", _U), (b"2023-00-10", _U), (b"2023-1-", _U),
    (b"2023-12-31", _D), (b"2023-04-31", _U), (b"2023-04-30", _D), (b"2023-1-05", _D), (b"2023-01-5", _D),
    (b"2023-01-00", _U), (b"2023-01-32", _U), (b"9999-12-31", _D), (b"0000-01-01", _D), (b"2023-", _U),
    (b"2023-01", _U), (b"2023-01-", _U), (b"2023-01-01 ", _U), (b"2023-1-5x", _U), (b"2023-001-1", _U),
    (b"2023/01/01", _S), (b"2023-01-1x", _U), (b"2100-02-29", _U), (b"2400-02-29", _D),
    (b"2023-01-01T00:00:00", _T), (b"2023-01-01 23:59:59.123456789Z", _T), (b"2023-01-01T24:00:00", _U),
    (b"2023-01-01T10:00", _U), (b"2023-01-01T10:00:00+05:30", _T), (b"2023-01-01T10:00:00+0530", _U),
    (b"2023-01-01X", _U), (b"2023-01-01t00:00:00", _U), (b"2023-01-01T00:00:00z", _U), (b"2023-01-01T00:00:00Z", _T),
    (b"2023-01-01T00:00:60", _U), (b"2023-01-01T00:60:00", _U), (b"2023-01-01T23:59:59", _T),
    (b"2023-01-01T00:00:00.", _U), (b"2023-01-01T00:00:00.1", _T), (b"2023-01-01T00:00:00.1234567890", _U),
    (b"2023-01-01T00:00:00-23:59", _T), (b"2023-01-01T00:00:00+24:00", _U), (b"2023-01-01T00:00:00+00:60", _U),
    (b"2023-01-01T00:00:00.5+01:00", _T), (b"2023-01-01T00:00:00ZZ", _U), (b"2023-01-01T00:00:00 UTC", _U),
    (b"2023-02-29T00:00:00", _U), (b"2023-1-05T00:00:00", _U), (b"2023-01-01  00:00:00", _U),
    (b"2023-01-01T0:00:00", _U), (b"2023-01-01T00-00-00", _U), (b"2023-01-01T00:00:00+1:00", _U),
    (b"+10999-12-31", _U), (b"5551-234", _U), (b"1234", _I), (b"12-34", _S), (b"-2023-01-01", _U), (b"+999-1-1", _S),
    (b"12345-01-01", _S), (b"-12345-", _U), (b"+1234", _F), (b"1234-", _U), (b"123-", _S),
    (b"", _S), (b"7" * 4096, _F), (b"7" * 4095 + b"x", _S), (b"hello world, this is forty bytes of text!", _S),
]

# the fuzz alphabet: dense in the bytes the grammars turn on
ALPHABET = b"0123456789+-.eE:TtZz nNaAiIfFrRuUlLsSyY\xc3"
_SEEDS = [v for v, _ in EDGES if 0 < len(v) <= 32]


def seeded_strings(n, seed=20261021):
    """`n` values: random draws from ALPHABET and mutations (a byte set, dropped, inserted or doubled) of edge values"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        if rng.random() < 0.35:
            v = bytes(rng.choice(ALPHABET) for _ in range(rng.randrange(0, 14)))
        else:
            v = bytearray(rng.choice(_SEEDS))
            for _ in range(rng.randrange(0, 3)):
                at = rng.randrange(0, len(v) + 1)
                how = rng.randrange(4)
                if how == 0 and at < len(v):
                    v[at] = rng.choice(ALPHABET)
                elif how == 1 and at < len(v):
                    del v[at]
                elif how == 2:
                    v.insert(at, rng.choice(ALPHABET))
                elif at < len(v):
                    v.insert(at, v[at])
            v = bytes(v)
        out.append(v)
    return out


def counts(values):
    """the nine counters of a column whose rows are `values` (bytes, or None for a NULL row)"""
    out = dict.fromkeys(COUNTERS, 0)
    for v in values:
        out["seen"] += 1
        if v is None:
            continue
        out["non_null"] += 1
        out[NAMES[classify(v)] + "_rows"] += 1
    return out


def add(a, b):
    return {k: a[k] + b[k] for k in COUNTERS}
