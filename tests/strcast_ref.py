"""The String casts of include/dbhip.h a24 in plain Python, written from the header's text: the reference of tests/test_strcast_host_cpu.py
and tests/test_gpu_strcast.py. It does not use int() / Decimal() / datetime to parse or print (they accept '_', Unicode digits and
exponents, and know nothing of "declined"); tests/test_strcast_ref_cpu.py holds it to them where both are defined.

parse(value, dtype, ...) -> (status, number): status OK / ERROR / DECLINED; the number is the integer, the decimal's unscaled integer, the
Date's days or the Timestamp's UTC microseconds (0 unless OK). text(number, dtype, ...) -> bytes, or None for the row error.
`quirk` switches ONE rule off, for the negative controls: "no_carry", "unsigned_minus", "leap_1900"."""
from databend_amd import _lib as T

OK, ERROR, DECLINED = 0, 1, 2
MAX_BYTES = 256
SPACE = (0x20, 0x09, 0x0A, 0x0B, 0x0C, 0x0D)
INT_RANGE = {T.T_I8: (-2**7, 2**7 - 1), T.T_I16: (-2**15, 2**15 - 1), T.T_I32: (-2**31, 2**31 - 1), T.T_I64: (-2**63, 2**63 - 1),
             T.T_U8: (0, 2**8 - 1), T.T_U16: (0, 2**16 - 1), T.T_U32: (0, 2**32 - 1), T.T_U64: (0, 2**64 - 1)}
DATE_MIN, DATE_MAX = -719162, 2932896
TS_MIN, TS_MAX = -62135596800000000, 253402300799999999
MAX_OFFSET_S = 64800
DAY_US = 86400 * 10**6


def is_digit(c):
    return 0x30 <= c <= 0x39


def number(digits):
    v = 0
    for c in digits:
        v = v * 10 + (c - 0x30)
    return v


def trim(b):
    s, e = 0, len(b)
    while s < e and b[s] in SPACE:
        s += 1
    while e > s and b[e - 1] in SPACE:
        e -= 1
    return b[s:e]


def take_digits(b, p):
    q = p
    while q < len(b) and is_digit(b[q]):
        q += 1
    return b[p:q], q


# ---- calendar: days since 1970-01-01 of the proleptic Gregorian calendar ------------------------------------------------------------------
def is_leap(y, quirk=None):
    if quirk == "leap_1900" and y == 1900:
        return True
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def month_days(y, m, quirk=None):
    return (31, 29 if is_leap(y, quirk) else 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)[m - 1]


def days_of(y, m, d):
    """(y >= 1, m, d) -> days since 1970-01-01: whole years since year 1, whole months of the year, days"""
    p = y - 1
    n = p * 365 + p // 4 - p // 100 + p // 400
    for k in range(1, m):
        n += month_days(y, k)
    return n + (d - 1) - 719162


def civil_of(days):
    """days since 1970-01-01 -> (y, m, d), years below 1 included"""
    n = days + 719162                      # days since 0001-01-01
    cycles, n = divmod(n, 146097)          # 400 years
    y = 1 + 400 * cycles
    c = min(n // 36524, 3)                 # centuries: the fourth is a day longer
    n -= c * 36524
    q = min(n // 1461, 24)
    n -= q * 1461
    a = min(n // 365, 3)
    n -= a * 365
    y += 100 * c + 4 * q + a
    m = 1
    while n >= month_days(y, m):
        n -= month_days(y, m)
        m += 1
    return y, m, n + 1


# ---- parse --------------------------------------------------------------------------------------------------------------------------------
def parse_int(b, dtype, quirk=None):
    lo, hi = INT_RANGE[dtype]
    if not b:
        return ERROR, 0
    p = 1 if b[0] in b"+-" else 0
    digits, q = take_digits(b, p)
    if not digits or q != len(b):
        if all(is_digit(c) or c in b"+-.eE" for c in b) and any(c in b".eE" for c in b):
            return DECLINED, 0
        return ERROR, 0
    neg = b[0] == 0x2D
    if neg and lo == 0 and quirk != "unsigned_minus":
        return ERROR, 0
    v = -number(digits) if neg else number(digits)
    if v < lo or v > hi:
        return ERROR, 0
    return OK, v


def parse_decimal(b, precision, scale, rounding=False, quirk=None):
    if not b:
        return ERROR, 0
    p = 1 if b[0] in b"+-" else 0
    whole, p = take_digits(b, p)
    frac = b""
    if p < len(b) and b[p] == 0x2E:
        frac, p = take_digits(b, p + 1)
    if not whole and not frac:
        return ERROR, 0
    if p < len(b):
        return (DECLINED if b[p] in b"eE" else ERROR), 0
    v = number(whole + frac[:scale]) * 10 ** (scale - len(frac[:scale]))
    if rounding and len(frac) > scale and frac[scale] >= 0x35 and quirk != "no_carry":
        v += 1
    if v >= 10 ** precision:
        return ERROR, 0
    return OK, (-v if b[0] == 0x2D else v)


def date_form(b, quirk=None):
    """-> (form matched, calendar day valid, (y, m, d), position behind the match)"""
    if len(b) < 8 or not all(is_digit(c) for c in b[:4]):
        return False, False, None, 0
    y, p, parts = number(b[:4]), 4, []
    for _ in range(2):
        if p >= len(b) or b[p] != 0x2D:
            return False, False, None, 0
        x, q = take_digits(b, p + 1)
        x = x[:2]
        if not x:
            return False, False, None, 0
        parts.append(number(x))
        p += 1 + len(x)
    m, d = parts
    valid = 1 <= y <= 9999 and 1 <= m <= 12 and 1 <= d <= month_days(y, m, quirk)
    return True, valid, (y, m, d), p


def parse_date(b, quirk=None):
    if not b:
        return ERROR, 0
    form, valid, ymd, p = date_form(b, quirk)
    if not form:
        return (DECLINED if all(is_digit(c) for c in b) else ERROR), 0
    if not valid:
        return ERROR, 0
    if p < len(b):
        return (DECLINED if b[p] in b" T" else ERROR), 0
    return OK, days_of(*ymd)


def two(b, p):
    return number(b[p:p + 2]) if len(b) >= p + 2 and is_digit(b[p]) and is_digit(b[p + 1]) else None


def parse_timestamp(b, offset_s=0, quirk=None):
    if not b:
        return ERROR, 0
    form, valid, ymd, p = date_form(b, quirk)
    if not form:
        return (DECLINED if all(is_digit(c) for c in b) else ERROR), 0
    if not valid:
        return ERROR, 0
    sod, us, off = 0, 0, offset_s
    if p < len(b) and b[p] in b" T":
        hh, mi, ss = two(b, p + 1), two(b, p + 4), 0
        if hh is None or mi is None or b[p + 3] != 0x3A:
            return ERROR, 0
        p += 6
        if p < len(b) and b[p] == 0x3A:
            ss = two(b, p + 1)
            if ss is None:
                return ERROR, 0
            p += 3
            if p < len(b) and b[p] == 0x2E:
                f, p = take_digits(b, p + 1)
                if not f:
                    return ERROR, 0
                us = number((f + b"000000")[:6])
        if hh > 23 or mi > 59 or ss > 59:
            return ERROR, 0
        sod = hh * 3600 + mi * 60 + ss
    if p < len(b):
        if b[p] == 0x5A:
            off, p = 0, p + 1
        elif b[p] in b"+-":
            sign = -1 if b[p] == 0x2D else 1
            zh, zm = two(b, p + 1), 0
            if zh is None:
                return ERROR, 0
            p += 3
            if p < len(b):
                if b[p] == 0x3A:
                    p += 1
                zm = two(b, p)
                if zm is None:
                    return ERROR, 0
                p += 2
            if zm > 59 or zh * 3600 + zm * 60 > MAX_OFFSET_S:
                return ERROR, 0
            off = sign * (zh * 3600 + zm * 60)
        if p != len(b):
            return ERROR, 0
    utc = (days_of(*ymd) * 86400 + sod - off) * 10**6 + us
    if utc < TS_MIN or utc > TS_MAX:
        return ERROR, 0
    return OK, utc


def parse(value, dtype, precision=0, scale=0, rounding=False, offset_s=0, quirk=None):
    value = bytes(value)
    if len(value) > MAX_BYTES:
        return DECLINED, 0
    b = trim(value)
    if dtype in INT_RANGE:
        return parse_int(b, dtype, quirk)
    if dtype in (T.T_DEC64, T.T_DEC128):
        return parse_decimal(b, precision, scale, rounding, quirk)
    if dtype == T.T_DATE:
        return parse_date(b, quirk)
    assert dtype == T.T_TIMESTAMP
    return parse_timestamp(b, offset_s, quirk)


# ---- format ---------------------------------------------------------------------------------------------------------------------------------
def digits_of(v, width=1):
    out = b""
    while v:
        v, d = divmod(v, 10)
        out = bytes([0x30 + d]) + out
    return b"0" * (width - len(out)) + out


def text(v, dtype, scale=0, offset_s=0):
    if dtype in INT_RANGE:
        return (b"-" if v < 0 else b"") + digits_of(abs(v))
    if dtype in (T.T_DEC64, T.T_DEC128):
        whole, frac = divmod(abs(v), 10 ** scale)
        return (b"-" if v < 0 else b"") + digits_of(whole) + (b"." + digits_of(frac, scale) if scale else b"")
    if dtype == T.T_DATE:
        if v < DATE_MIN or v > DATE_MAX:
            return None
        y, m, d = civil_of(v)
        return digits_of(y, 4) + b"-" + digits_of(m, 2) + b"-" + digits_of(d, 2)
    assert dtype == T.T_TIMESTAMP
    if v < TS_MIN or v > TS_MAX:
        return None
    days, rest = divmod(v + offset_s * 10**6, DAY_US)
    y, m, d = civil_of(days)
    if y < 1 or y > 9999:
        return None
    sod, us = divmod(rest, 10**6)
    return (digits_of(y, 4) + b"-" + digits_of(m, 2) + b"-" + digits_of(d, 2) + b" " + digits_of(sod // 3600, 2) + b":" + digits_of(sod // 60 % 60, 2) + b":" +
            digits_of(sod % 60, 2) + b"." + digits_of(us, 6))


def view(t, offset):
    """the 16 bytes of a result's view: inline and canonical up to 12 bytes, else {len, first four bytes, buffer 0, offset}"""
    t = t or b""
    if len(t) <= 12:
        return len(t).to_bytes(4, "little") + t.ljust(12, b"\0")
    return len(t).to_bytes(4, "little") + t[:4] + (0).to_bytes(4, "little") + offset.to_bytes(4, "little")


def format_column(values, valid, dtype, scale=0, offset_s=0, capacity=None):
    """-> (views [bytes], out_data bytes, rows that got the empty view instead of a text): what dbhip_str_format leaves; with `capacity`
    the long rows that would end past it are empty and counted"""
    views, data, errs = [], b"", 0
    off = 0
    for v, ok in zip(values, valid):
        t = text(v, dtype, scale, offset_s) if ok else b""
        if t is None:
            errs += 1
            t = b""
        if len(t) > 12:
            if capacity is not None and off + len(t) > capacity:
                errs += 1
                off += len(t)
                views.append(view(b"", 0))
                continue
            views.append(view(t, off))
            data += t
            off += len(t)
        else:
            views.append(view(t, 0))
    return views, data, errs
