"""CPU: tests/datetime_ref.py (numpy datetime64) held to Python's own calendar — datetime.date, date.isocalendar, isoweekday,
timetuple().tm_yday, calendar.monthrange — over the first and last 400 days of the range, every Feb 27 .. Mar 1 of the years divisible
by 4, and 200,000 seeded random days. Python's datetime covers years 1..9999, the whole range. Each deliberately wrong variant of the
reference (the negative controls) must be caught by the very same assertions."""
import calendar
import datetime
import types

import numpy as np
import pytest

from tests import datetime_ref as R

EPOCH_ORD = datetime.date(1970, 1, 1).toordinal()


def sample_days():
    rng = np.random.default_rng(2100)
    leap = [datetime.date(y, m, d).toordinal() - EPOCH_ORD for y in range(4, 10000, 4) for m, d in ((2, 27), (2, 28), (3, 1))]
    leap += [datetime.date(y, 2, 29).toordinal() - EPOCH_ORD for y in range(4, 10000, 4) if calendar.isleap(y)]
    return np.unique(np.concatenate([np.arange(R.DATE_MIN, R.DATE_MIN + 400), np.arange(R.DATE_MAX - 399, R.DATE_MAX + 1), np.array(leap),
                                     rng.integers(R.DATE_MIN, R.DATE_MAX + 1, 200_000)]).astype(np.int64))


@pytest.fixture(scope="module")
def python_calendar():
    """days -> what Python says, computed once"""
    days = sample_days()
    rows = []
    for x in days.tolist():
        d = datetime.date.fromordinal(x + EPOCH_ORD)
        iy, iw, idow = d.isocalendar()
        rows.append((d.year, d.month, d.day, d.timetuple().tm_yday, d.isoweekday(), iy, iw, idow))
    return days, np.array(rows, dtype=np.int64)


def check_calendar(impl, days, py):
    y, m, d, doy = impl.civil(days)
    assert np.array_equal(y, py[:, 0]) and np.array_equal(m, py[:, 1]) and np.array_equal(d, py[:, 2])
    assert np.array_equal(doy, py[:, 3])
    assert np.array_equal(impl.dow_iso(days), py[:, 4]) and np.array_equal(py[:, 4], py[:, 7])
    iy, iw = impl.iso(days)
    assert np.array_equal(iy, py[:, 5]) and np.array_equal(iw, py[:, 6])
    # the parts built from them
    for p, col in ((R.YEAR, 0), (R.MONTH, 1), (R.DAY, 2), (R.DAY_OF_YEAR, 3), (R.DOW_ISO, 4), (R.ISO_YEAR, 5), (R.ISO_WEEK, 6)):
        assert np.array_equal(R.part(p, days, R.SRC_DATE, impl=impl), py[:, col]), R.PART_NAMES[p]
    assert np.array_equal(R.part(R.DOW_SUNDAY0, days, R.SRC_DATE, impl=impl), py[:, 4] % 7)
    assert np.array_equal(R.part(R.QUARTER, days, R.SRC_DATE, impl=impl), (py[:, 1] + 2) // 3)
    assert np.array_equal(R.part(R.YYYYMMDD, days, R.SRC_DATE, impl=impl), py[:, 0] * 10000 + py[:, 1] * 100 + py[:, 2])


def py_add_months(x, k):
    d = datetime.date.fromordinal(x + EPOCH_ORD)
    t = d.year * 12 + d.month - 1 + k
    y, m = divmod(t, 12)
    if not 1 <= y <= 9999:
        return None
    return datetime.date(y, m + 1, min(d.day, calendar.monthrange(y, m + 1)[1])).toordinal() - EPOCH_ORD


def check_add_months(impl):
    days = np.array([datetime.date(y, m, d).toordinal() - EPOCH_ORD for y in (1, 1900, 1999, 2000, 2023, 2024, 9998)
                     for m, d in ((1, 28), (1, 29), (1, 30), (1, 31), (2, 28), (3, 31), (5, 31), (8, 31), (10, 31), (12, 31), (6, 15))], dtype=np.int64)
    for k in (0, 1, -1, 2, 11, -11, 12, -12, 13, -13, 1200, -1200, 47, -49):
        exp = [py_add_months(x, k) for x in days.tolist()]
        keep = np.array([e is not None for e in exp])
        got = impl.add_months(days[keep], np.full(int(keep.sum()), k, dtype=np.int64))
        assert np.array_equal(got, np.array([e for e in exp if e is not None], dtype=np.int64)), k


def check_floor_split(impl):
    """negative micros: one microsecond before a midnight belongs to the day before"""
    rng = np.random.default_rng(2102)
    days = rng.integers(R.DATE_MIN + 1, R.DATE_MAX, 2000)
    us = rng.integers(0, R.DAY_US, 2000)
    ts = np.concatenate([days * R.DAY_US + us, np.array([-1, 0, 1, -R.DAY_US, -R.DAY_US - 1, R.TS_MIN, R.TS_MAX])]).astype(np.int64)
    gd, gu = impl.split_ts(ts)
    for t, d, u in zip(ts.tolist(), gd.tolist(), gu.tolist()):
        assert (d, u) == divmod(t, R.DAY_US), t
    # through the parts, against datetime
    for t, h, mi, s, day in zip(ts.tolist(), *(R.part(p, ts, R.SRC_TS, impl=impl).tolist() for p in (R.HOUR, R.MINUTE, R.SECOND, R.DAY))):
        dt = datetime.datetime(1970, 1, 1) + datetime.timedelta(microseconds=t)
        assert (dt.hour, dt.minute, dt.second, dt.day) == (h, mi, s, day), t


def test_reference_agrees_with_python(python_calendar):
    days, py = python_calendar
    assert len(days) > 200_000 and days[0] == R.DATE_MIN and days[-1] == R.DATE_MAX
    check_calendar(R._SELF, days, py)
    check_add_months(R._SELF)
    check_floor_split(R._SELF)
    # the facts the header relies on: 0001-01-01 is a Monday, 9999-12-31 a Friday of week 52, every ISO year of the range is 1..9999
    assert R.dow_iso(np.array([R.DATE_MIN]))[0] == 1 and R.dow_iso(np.array([R.DATE_MAX]))[0] == 5
    assert [int(v[0]) for v in R.iso(np.array([R.DATE_MAX]))] == [9999, 52] and [int(v[0]) for v in R.iso(np.array([R.DATE_MIN]))] == [1, 1]


def variant(**replaced):
    ns = types.SimpleNamespace(civil=R.civil, dow_iso=R.dow_iso, iso=R.iso, split_ts=R.split_ts, add_months=R.add_months)
    for k, v in replaced.items():
        setattr(ns, k, v)
    return ns


def julian_civil(days):
    """every 4th year a leap year"""
    n = np.asarray(days, dtype=np.int64) + 719468                # days since 0000-03-01, in a calendar that never skips a leap day
    y = (4 * n + 3) // 1461
    ny = n - 1461 * y // 4
    m0 = (5 * ny + 2) // 153
    day = ny - (153 * m0 + 2) // 5 + 1
    return y + (m0 >= 10), np.where(m0 >= 10, m0 - 9, m0 + 3), day, R.civil(days)[3]


def truncating_split(local_us):
    local_us = np.asarray(local_us, dtype=np.int64)
    days = np.where(local_us >= 0, local_us // R.DAY_US, -((-local_us) // R.DAY_US))
    return days, local_us - days * R.DAY_US


def add_months_unclamped(days, months):
    d = np.asarray(days, dtype=np.int64).astype("M8[D]")
    m = d.astype("M8[M]")
    return (m.astype(np.int64) + months).astype("M8[M]").astype("M8[D]").astype(np.int64) + (d - m.astype("M8[D]")).astype(np.int64)


def test_negative_controls_are_caught(python_calendar):
    days, py = python_calendar
    with pytest.raises(AssertionError):                    # the Julian leap rule
        check_calendar(variant(civil=julian_civil), days, py)
    with pytest.raises(AssertionError):                    # Sunday-based DOW passed as ISO
        check_calendar(variant(dow_iso=lambda d: R.dow_iso(d) % 7), days, py)
    with pytest.raises(AssertionError):                    # truncating instead of floor division for negative micros
        check_floor_split(variant(split_ts=truncating_split))
    with pytest.raises(AssertionError):                    # add-months without the day clamp
        check_add_months(variant(add_months=add_months_unclamped))
    # and the unmodified reference passes the same three
    check_calendar(variant(), days, py)
    check_floor_split(variant())
    check_add_months(variant())


def test_time_zone_lookup():
    tz = R.synthetic_tz()
    at = tz.at.tolist()
    probe = np.array([x * 10**6 + e for x in at for e in (-1, 0, 1, 999_999, 10**6)] + [R.TS_MIN, R.TS_MAX], dtype=np.int64)
    got = R.tz_offset(probe, tz)
    for t, g in zip(probe.tolist(), got.tolist()):
        sec = t // 10**6
        k = sum(1 for a in at if a <= sec)
        assert g == (tz.offset_s if k == 0 else int(tz.after[k - 1])), t
    assert np.array_equal(R.tz_offset(probe, 19800), np.full(len(probe), 19800))
