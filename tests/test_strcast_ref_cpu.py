"""CPU: tests/strcast_ref.py — the plain-Python reference of the String casts (include/dbhip.h a24) — held to Python's own operations on
the inputs where both are defined: int(), decimal.Decimal.quantize (ROUND_DOWN / ROUND_HALF_UP), datetime.date / datetime arithmetic,
str() / format() for the format side; and negative controls: a reference with one rule switched off must disagree."""
import datetime
import decimal
import random
import re

import pytest

from databend_amd import _lib as T
from tests import strcast_cases as K
from tests import strcast_ref as R

EPOCH = datetime.date(1970, 1, 1)
EPOCH_TS = datetime.datetime(1970, 1, 1)
INT_RE = re.compile(rb"[+-]?[0-9]+\Z")
DEC_RE = re.compile(rb"[+-]?([0-9]+\.?[0-9]*|\.[0-9]+)\Z")


def test_case_list_holds_what_it_should():
    K.check_coverage()


@pytest.mark.parametrize("dtype", K.INT_TYPES)
def test_integers_against_int(dtype, quirk=None):
    lo, hi = R.INT_RANGE[dtype]
    seen = set()
    for v in K.int_values(dtype):
        b = R.trim(v)
        if len(v) > R.MAX_BYTES or not INT_RE.match(b):
            continue                                  # int() is not defined there (or accepts what the header does not)
        x = int(b.decode())
        st, got = R.parse(v, dtype, quirk=quirk)
        unsigned_minus = lo == 0 and b[:1] == b"-"
        want = R.OK if lo <= x <= hi and not unsigned_minus else R.ERROR
        assert (st, got) == (want, x if want == R.OK else 0), v[:40]
        seen.add(st)
    assert seen == {R.OK, R.ERROR}


@pytest.mark.parametrize("rounding", [False, True])
@pytest.mark.parametrize("p,s", [(18, 0), (18, 18), (38, 0), (38, 38), (15, 2), (3, 2), (3, 1)])
def test_decimals_against_quantize(p, s, rounding, quirk=None):
    ctx = decimal.Context(prec=400)
    seen = set()
    for v in K.decimal_values(p, s):
        b = R.trim(v)
        if len(v) > R.MAX_BYTES or not DEC_RE.match(b):
            continue
        q = decimal.Decimal(b.decode()).quantize(decimal.Decimal(1).scaleb(-s), rounding=decimal.ROUND_HALF_UP if rounding else decimal.ROUND_DOWN, context=ctx)
        x = int(q.scaleb(s, context=ctx))
        st, got = R.parse(v, T.T_DEC64 if p <= 18 else T.T_DEC128, p, s, rounding, quirk=quirk)
        want = R.OK if abs(x) < 10**p else R.ERROR
        assert (st, got) == (want, x if want == R.OK else 0), v[:40]
        seen.add(st)
    assert seen == {R.OK, R.ERROR}


def test_known_decimal_answers():
    D = T.T_DEC64
    assert R.parse(b"9.995", D, 3, 2, False) == (R.OK, 999) and R.parse(b"9.995", D, 3, 2, True) == (R.ERROR, 0)
    assert R.parse(b"99.99", D, 3, 1, False) == (R.OK, 999) and R.parse(b"99.99", D, 3, 1, True) == (R.ERROR, 0)
    assert R.parse(b".5", D, 3, 1) == (R.OK, 5) and R.parse(b"5.", D, 3, 1) == (R.OK, 50) and R.parse(b"-0.0", D, 3, 1) == (R.OK, 0)
    for bad in (b".", b"-", b"+.", b""):
        assert R.parse(bad, D, 3, 1) == (R.ERROR, 0)
    for declined in (b"1e5", b"1.5E3", b"0" * 300):
        assert R.parse(declined, D, 3, 1) == (R.DECLINED, 0)
    for declined in (b"1.5", b"1e5", b"0" * 300):
        assert R.parse(declined, T.T_I32) == (R.DECLINED, 0)
    assert R.parse(b"0" * 250 + b"1", T.T_I8) == (R.OK, 1) and R.parse(b"-0", T.T_U8) == (R.ERROR, 0) and R.parse(b"+7", T.T_U8) == (R.OK, 7)


def test_calendar_against_datetime():
    rng = random.Random(5)
    days = [R.DATE_MIN, R.DATE_MAX, 0, -1, 59, 60, 11016, 11017] + [rng.randint(R.DATE_MIN, R.DATE_MAX) for _ in range(3000)]
    for d in days:
        want = EPOCH + datetime.timedelta(days=d)
        assert R.civil_of(d) == (want.year, want.month, want.day)
        assert R.days_of(want.year, want.month, want.day) == d
        assert R.text(d, T.T_DATE) == want.isoformat().encode()
        assert R.parse(want.isoformat().encode(), T.T_DATE) == (R.OK, d)
    assert R.text(R.DATE_MIN - 1, T.T_DATE) is None and R.text(R.DATE_MAX + 1, T.T_DATE) is None
    assert R.civil_of(R.DATE_MIN - 1) == (0, 12, 31) and R.civil_of(R.DATE_MAX + 1) == (10000, 1, 1)


def test_dates_against_datetime(quirk=None):
    seen = set()
    for v in K.date_values():
        st, got = R.parse(v, T.T_DATE, quirk=quirk)
        m = re.match(rb"([0-9]{4})-([0-9]{1,2})-([0-9]{1,2})\Z", R.trim(v))
        if not m or len(v) > R.MAX_BYTES:
            assert st != R.OK, v[:40]
            continue
        try:
            want = (R.OK, (datetime.date(*(int(x) for x in m.groups())) - EPOCH).days)
        except ValueError:
            want = (R.ERROR, 0)
        assert (st, got) == want, v
        seen.add(st)
    assert seen == {R.OK, R.ERROR}


@pytest.mark.parametrize("offset_s", [0, 19800, -64800])
def test_timestamps_against_datetime(offset_s):
    rng = random.Random(offset_s)
    us = [R.TS_MIN + 64800 * 10**6, R.TS_MAX - 64800 * 10**6, 0, -1, 1709210096123456] + [rng.randint(R.TS_MIN + 64800 * 10**6, R.TS_MAX - 64800 * 10**6) for _ in range(2000)]
    for t in us:
        local = EPOCH_TS + datetime.timedelta(microseconds=t + offset_s * 10**6)
        txt = local.strftime("%Y-%m-%d %H:%M:%S.%f").encode()
        if local.year < 1000:
            txt = b"%04d" % local.year + txt[txt.index(b"-"):]       # (strftime does not pad the year everywhere)
        assert R.text(t, T.T_TIMESTAMP, offset_s=offset_s) == txt
        assert R.parse(txt, T.T_TIMESTAMP, offset_s=offset_s) == (R.OK, t)
        assert R.parse(txt.replace(b" ", b"T") + b"Z", T.T_TIMESTAMP, offset_s=offset_s) == (R.OK, t + offset_s * 10**6)
        zone = b"%s%02d:%02d" % (b"-" if offset_s < 0 else b"+", abs(offset_s) // 3600, abs(offset_s) // 60 % 60)
        assert R.parse(txt + zone, T.T_TIMESTAMP, offset_s=77) == (R.OK, t)
    assert R.parse(b"0001-01-01 05:00:00+05:00", T.T_TIMESTAMP) == (R.OK, R.TS_MIN) and R.parse(b"0001-01-01 04:59:59.999999+05:00", T.T_TIMESTAMP) == (R.ERROR, 0)
    assert R.parse(b"9999-12-31 18:59:59.999999-05:00", T.T_TIMESTAMP) == (R.OK, R.TS_MAX) and R.parse(b"9999-12-31 19:00:00-05:00", T.T_TIMESTAMP) == (R.ERROR, 0)
    assert R.parse(b"2024-02-29 12:34+18:00", T.T_TIMESTAMP)[0] == R.OK and R.parse(b"2024-02-29 12:34+18:01", T.T_TIMESTAMP)[0] == R.ERROR
    assert R.parse(b"2024-02-29 12:34:60", T.T_TIMESTAMP)[0] == R.ERROR and R.parse(b"2024-02-29 24:00", T.T_TIMESTAMP)[0] == R.ERROR
    assert R.parse(b"2024-02-29T12:34:56.123456789012", T.T_TIMESTAMP) == R.parse(b"2024-02-29 12:34:56.123456", T.T_TIMESTAMP)
    assert R.parse(b"20240229", T.T_TIMESTAMP) == (R.DECLINED, 0) and R.parse(b"2024-02-29 x", T.T_DATE) == (R.DECLINED, 0)


def test_format_against_str_and_format():
    for name, sp, numbers in K.format_groups():
        for v in numbers:
            t = R.text(v, sp["dtype"], sp["scale"], sp["offset_s"])
            if sp["dtype"] in R.INT_RANGE:
                assert t == str(v).encode()
            elif sp["dtype"] in (T.T_DEC64, T.T_DEC128):
                want = format(decimal.Context(prec=60).scaleb(decimal.Decimal(v), -sp["scale"]), "f")
                if v == 0:
                    want = want.lstrip("-")
                assert t == want.encode(), (name, v)
            if t is not None:
                assert len(t) <= 41 and R.view(t, 5)[:4] == len(t).to_bytes(4, "little")


def test_negative_controls():
    """a reference with one rule switched off disagrees with Python: the checks above can fail"""
    with pytest.raises(AssertionError):
        test_decimals_against_quantize(3, 2, True, quirk="no_carry")
    with pytest.raises(AssertionError):
        test_integers_against_int(T.T_U8, quirk="unsigned_minus")
    with pytest.raises(AssertionError):
        test_dates_against_datetime(quirk="leap_1900")
    assert R.parse(b"1900-02-29", T.T_DATE) == (R.ERROR, 0) and R.parse(b"1900-02-29", T.T_DATE, quirk="leap_1900")[0] == R.OK
    assert R.parse(b"9.995", T.T_DEC64, 3, 2, True, quirk="no_carry") == (R.OK, 999)
    assert R.parse(b"-5", T.T_U8, quirk="unsigned_minus")[0] != R.parse(b"-5", T.T_U8)[0] or R.parse(b"-0", T.T_U8, quirk="unsigned_minus") == (R.OK, 0)
