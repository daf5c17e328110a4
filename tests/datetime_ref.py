"""Plain reference for the Date / Timestamp functions (include/dbhip.h a21) on numpy datetime64 arithmetic only. It shares nothing with
databend_amd/csrc/dev_datetime.h: year, month, day and day of year come from astype('M8[Y]') / astype('M8[M]'), the ISO week from the
Thursday of the row's week, add-months from a month index with the day clamped to the month's length, the time-zone lookup from
np.searchsorted. tests/test_datetime_ref_cpu.py holds this file to Python's datetime; the host and GPU tests hold the library to it.

Dates are int64 arrays of days since 1970-01-01, Timestamps int64 arrays of microseconds. Results are int64 arrays."""
import numpy as np

DATE_MIN, DATE_MAX = -719162, 2932896                        # 0001-01-01 .. 9999-12-31
TS_MIN, TS_MAX = -62135596800000000, 253402300799999999
DAY_US = 86400 * 10**6

(YEAR, QUARTER, MONTH, DAY, DAY_OF_YEAR, DOW_ISO, DOW_SUNDAY0, ISO_YEAR, ISO_WEEK, HOUR, MINUTE, SECOND, MICROSECOND, EPOCH_SECOND,
 YYYYMM, YYYYMMDD, YYYYMMDDHH, YYYYMMDDHHMMSS, DATE) = range(19)
PART_NAMES = ["YEAR", "QUARTER", "MONTH", "DAY", "DAY_OF_YEAR", "DOW_ISO", "DOW_SUNDAY0", "ISO_YEAR", "ISO_WEEK", "HOUR", "MINUTE", "SECOND",
              "MICROSECOND", "EPOCH_SECOND", "YYYYMM", "YYYYMMDD", "YYYYMMDDHH", "YYYYMMDDHHMMSS", "DATE"]
TIME_PARTS = (HOUR, MINUTE, SECOND, MICROSECOND, EPOCH_SECOND, YYYYMMDDHH, YYYYMMDDHHMMSS, DATE)
DATE_PARTS = tuple(p for p in range(19) if p not in TIME_PARTS)
U_YEAR, U_QUARTER, U_MONTH, U_WEEK, U_DAY, U_HOUR, U_MINUTE, U_SECOND = range(8)
UNIT_NAMES = ["YEAR", "QUARTER", "MONTH", "WEEK", "DAY", "HOUR", "MINUTE", "SECOND"]
WEEK_SUNDAY = 1
SRC_DATE, SRC_TS = "date", "ts"
UNIT_US = {U_WEEK: 7 * DAY_US, U_DAY: DAY_US, U_HOUR: 3600 * 10**6, U_MINUTE: 60 * 10**6, U_SECOND: 10**6}


class Tz:
    """dbhip_tz: offset_s before the first transition, offset_after_s[k] from at_utc_s[k] on"""

    def __init__(self, offset_s=0, at_utc_s=(), offset_after_s=()):
        self.offset_s = int(offset_s)
        self.at = np.asarray(at_utc_s, dtype=np.int64)
        self.after = np.asarray(offset_after_s, dtype=np.int64)


def _tz(tz):
    return tz if isinstance(tz, Tz) else Tz(0 if tz is None else tz)


def tz_offset(ts, tz):
    """the offset in seconds in force at each utc value"""
    tz = _tz(tz)
    ts = np.asarray(ts, dtype=np.int64)
    if len(tz.at) == 0:
        return np.full(ts.shape, tz.offset_s, dtype=np.int64)
    k = np.searchsorted(tz.at, np.floor_divide(ts, 10**6), "right")
    return np.where(k == 0, tz.offset_s, tz.after[np.maximum(k, 1) - 1])


def civil(days):
    """-> year, month, day, day of year"""
    d = np.asarray(days, dtype=np.int64).astype("M8[D]")
    y, m = d.astype("M8[Y]"), d.astype("M8[M]")
    year = y.astype(np.int64) + 1970
    month = m.astype(np.int64) - y.astype("M8[M]").astype(np.int64) + 1
    day = (d - m.astype("M8[D]")).astype(np.int64) + 1
    doy = (d - y.astype("M8[D]")).astype(np.int64) + 1
    return year, month, day, doy


def dow_iso(days):
    """Monday = 1 .. Sunday = 7 (1970-01-01 was a Thursday)"""
    return (np.asarray(days, dtype=np.int64) + 3) % 7 + 1


def iso(days):
    """-> ISO year, ISO week: those of the Thursday of the row's week"""
    days = np.asarray(days, dtype=np.int64)
    year, _, _, doy = civil(days - (dow_iso(days) - 1) + 3)
    return year, (doy - 1) // 7 + 1


def split_ts(local_us):
    """-> local days, microsecond of the day (floor)"""
    local_us = np.asarray(local_us, dtype=np.int64)
    days = np.floor_divide(local_us, DAY_US)
    return days, local_us - days * DAY_US


def add_months(days, months):
    """calendar addition: the day of month is clamped to the last day of the target month"""
    d = np.asarray(days, dtype=np.int64).astype("M8[D]")
    m = d.astype("M8[M]")
    dom = (d - m.astype("M8[D]")).astype(np.int64)
    t = m.astype(np.int64) + np.asarray(months, dtype=np.int64)
    first = t.astype("M8[M]").astype("M8[D]").astype(np.int64)
    length = (t + 1).astype("M8[M]").astype("M8[D]").astype(np.int64) - first
    return first + np.minimum(dom, length - 1)


def part(p, values, src, tz=None, impl=None):
    f = impl or _SELF
    values = np.asarray(values, dtype=np.int64)
    if src == SRC_DATE:
        assert p in DATE_PARTS
        days, usod = values, np.zeros_like(values)
    else:
        days, usod = f.split_ts(values + tz_offset(values, tz) * 10**6)
    sod = usod // 10**6
    h, mi, s = sod // 3600, sod // 60 % 60, sod % 60
    if p in (YEAR, QUARTER, MONTH, DAY, DAY_OF_YEAR, YYYYMM, YYYYMMDD, YYYYMMDDHH, YYYYMMDDHHMMSS):
        y, m, d, doy = f.civil(days)
        ymd = y * 10000 + m * 100 + d
        return {YEAR: y, QUARTER: (m + 2) // 3, MONTH: m, DAY: d, DAY_OF_YEAR: doy, YYYYMM: y * 100 + m, YYYYMMDD: ymd, YYYYMMDDHH: ymd * 100 + h,
                YYYYMMDDHHMMSS: ymd * 10**6 + h * 10000 + mi * 100 + s}[p]
    if p == DOW_ISO:
        return f.dow_iso(days)
    if p == DOW_SUNDAY0:
        return f.dow_iso(days) % 7
    if p in (ISO_YEAR, ISO_WEEK):
        return f.iso(days)[0 if p == ISO_YEAR else 1]
    if p == EPOCH_SECOND:
        return np.floor_divide(values, 10**6)
    return {HOUR: h, MINUTE: mi, SECOND: s, MICROSECOND: usod % 10**6, DATE: days}[p]


def _trunc_days(unit, flags, days):
    d = days.astype("M8[D]")
    if unit == U_YEAR:
        return d.astype("M8[Y]").astype("M8[D]").astype(np.int64)
    if unit == U_QUARTER:
        mi = d.astype("M8[M]").astype(np.int64)          # months since 1970-01: a multiple of 3 is the first month of a quarter
        return (mi - mi % 3).astype("M8[M]").astype("M8[D]").astype(np.int64)
    if unit == U_MONTH:
        return d.astype("M8[M]").astype("M8[D]").astype(np.int64)
    if unit == U_WEEK:
        return days - (dow_iso(days) % 7 if flags & WEEK_SUNDAY else dow_iso(days) - 1)
    return days


def trunc(unit, flags, values, src, out, offset_s=0):
    """the result is clamped into the output type's range (the start of year 1: Sunday weeks, zones east of UTC)"""
    values = np.asarray(values, dtype=np.int64)
    if src == SRC_DATE:
        days, usod = values, np.zeros_like(values)
    else:
        days, usod = split_ts(values + offset_s * 10**6)
    tdays = _trunc_days(unit, flags, days)
    if out == SRC_DATE:
        assert unit <= U_DAY
        return np.clip(tdays, DATE_MIN, DATE_MAX)
    q = {U_HOUR: 3600 * 10**6, U_MINUTE: 60 * 10**6, U_SECOND: 10**6}.get(unit)
    tus = usod - usod % q if q else np.zeros_like(usod)
    assert src == SRC_TS or q is None
    return np.clip(tdays * DAY_US + tus - offset_s * 10**6, TS_MIN, TS_MAX)


def add(unit, values, delta, src, offset_s=0, impl=None):
    """-> (result with 0 in the error rows, bool array: the row raises `date out of range`). Raised when the input is outside the
    type's range or the result leaves it; a delta too large to stay inside the range is clipped first so that nothing here wraps."""
    f = impl or _SELF
    values = np.asarray(values, dtype=np.int64)
    delta = np.broadcast_to(np.asarray(delta, dtype=np.int64), values.shape)
    lo, hi = (DATE_MIN, DATE_MAX) if src == SRC_DATE else (TS_MIN, TS_MAX)
    bad = (values < lo) | (values > hi)
    v = np.where(bad, 0, values)
    if unit <= U_MONTH:
        months = np.clip(delta, -10**7, 10**7) * {U_YEAR: 12, U_QUARTER: 3, U_MONTH: 1}[unit]
        if src == SRC_DATE:
            r = f.add_months(v, months)
        else:
            days, usod = split_ts(v + offset_s * 10**6)
            r = f.add_months(days, months) * DAY_US + usod - offset_s * 10**6
    elif src == SRC_DATE:
        assert unit in (U_WEEK, U_DAY)
        r = v + np.clip(delta, -10**7, 10**7) * (7 if unit == U_WEEK else 1)
    else:
        b = 2 * (TS_MAX - TS_MIN) // UNIT_US[unit]
        r = v + np.clip(delta, -b, b) * UNIT_US[unit]
    bad |= (r < lo) | (r > hi)
    return np.where(bad, 0, r), bad


def diff(unit, a, b, src, offset_s=0):
    """boundaries of `unit` crossed from a to b"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    if src == SRC_TS:
        a, b = a + offset_s * 10**6, b + offset_s * 10**6
        if unit >= U_HOUR:
            return np.floor_divide(b, UNIT_US[unit]) - np.floor_divide(a, UNIT_US[unit])
        a, b = split_ts(a)[0], split_ts(b)[0]
    assert unit <= U_DAY
    if unit == U_DAY:
        return b - a
    if unit == U_WEEK:
        return np.floor_divide(b + 3, 7) - np.floor_divide(a + 3, 7)
    (ya, ma, _, _), (yb, mb, _, _) = civil(a), civil(b)
    if unit == U_YEAR:
        return yb - ya
    if unit == U_QUARTER:
        return (yb * 4 + (mb - 1) // 3) - (ya * 4 + (ma - 1) // 3)
    return (yb * 12 + mb) - (ya * 12 + ma)


class _Self:
    civil = staticmethod(civil)
    dow_iso = staticmethod(dow_iso)
    iso = staticmethod(iso)
    split_ts = staticmethod(split_ts)
    add_months = staticmethod(add_months)


_SELF = _Self


# ---- shared inputs of the host and GPU tests -------------------------------------------------------------------------------------------
OFFSETS = (0, 19800, -34200, 64800, -64800)
ADD_DELTAS = (0, 1, -1, 11, -11, 12, -12, 13, -13, 1200, -1200, 119987, -119987, -2**63, 2**63 - 1)


def synthetic_tz():
    """5 transitions, two of them one second apart"""
    return Tz(-18000, [-5 * 10**9, 0, 1, 10**9, 4 * 10**9], [3600, -7200, 20700, 0, 50400])


def all_dates():
    return np.arange(DATE_MIN, DATE_MAX + 1, dtype=np.int64)


def timestamp_set():
    """both ends of the range, k * 86400e6 + {-1, 0, 1} for 4,096 seeded days, 2^20 seeded uniform values"""
    rng = np.random.default_rng(2101)
    days = rng.integers(DATE_MIN + 1, DATE_MAX, 4096, dtype=np.int64)
    edges = (days[:, None] * DAY_US + np.array([-1, 0, 1], dtype=np.int64)[None, :]).reshape(-1)
    uniform = rng.integers(TS_MIN, TS_MAX + 1, 1 << 20, dtype=np.int64)
    return np.concatenate([np.array([TS_MIN, TS_MIN + 1, TS_MAX - 1, TS_MAX, -1, 0, 1], dtype=np.int64), edges, uniform])
