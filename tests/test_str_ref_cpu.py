"""CPU: tests/str_ref.py — the reference the String function tests compare against — held to Python's own bytes / str operations where
the definitions coincide, to the known answers of include/dbhip.h a22, and to negative controls: a reference with an off-by-one start,
or a trim that strips single bytes instead of whole pads, must fail these same checks."""
import numpy as np
import pytest

from tests import str_ref as R
from tests import strfn_cases as K


def utf8_pool():
    rng = np.random.default_rng(3)
    alphabet = ["a", "Z", " ", "é", "ß", "€", "中", "😀", "𝄞"]
    return ["".join(alphabet[k] for k in rng.integers(0, len(alphabet), int(n))) for n in list(range(0, 9)) + [12, 13, 40, 300]]


def py_substr(s, pos, ln):
    """SQL substr on a str, by code points"""
    u = len(s)
    if pos == 0 or (ln is not None and ln <= 0):
        return ""
    start = pos - 1 if pos > 0 else u + pos
    if start < 0 or start >= u:
        return ""
    return s[start:] if ln is None else s[start:start + ln]


def check_slices(ref):
    for s in utf8_pool():
        v = s.encode()
        u = len(s)
        assert ref.length(v) == u and ref.length(v, True) == len(v)
        for pos in (0, 1, -1, 2, u - 1, -(u - 1), u, -u, u + 1, -(u + 1), R.INT64_MIN, R.INT64_MAX):
            for ln in (None, 0, -1, 1, 2, u - 1, u, u + 1, R.INT64_MAX, R.INT64_MIN):
                assert ref.substr(v, pos, ln).decode() == py_substr(s, pos, ln), (s, pos, ln)
                assert ref.substr(v, pos, ln, True) == py_substr(v.decode("latin-1"), pos, ln).encode("latin-1"), (v, pos, ln)
        for k in (0, -1, 1, 2, u - 1, u, u + 1, R.INT64_MAX, R.INT64_MIN):
            assert ref.left(v, k).decode() == (s[:k] if k > 0 else "")
            assert ref.right(v, k).decode() == (s[-k:] if 0 < k < u else (s if k > 0 else ""))
            assert ref.left(v, k, True) == (v[:k] if k > 0 else b"") and ref.right(v, k, True) == (v[-k:] if 0 < k < len(v) else (v if k > 0 else b""))


def py_trim(v, pad, where):
    if pad:
        if where in (R.TRIM_LEADING, R.TRIM_BOTH):
            while v.startswith(pad):
                v = v.removeprefix(pad)
        if where in (R.TRIM_TRAILING, R.TRIM_BOTH):
            while v.endswith(pad):
                v = v.removesuffix(pad)
    return v


def check_trims(ref):
    values = K.values() + [b"ababxab", b"aba", b"aaa", b"  x  ", b"xx", b"abab", b"", b"a"]
    for v in values:
        for pad in K.PADS + [b"a", b"aa", b"x"]:
            for where in (R.TRIM_LEADING, R.TRIM_TRAILING, R.TRIM_BOTH):
                assert ref.trim(v, pad, where) == py_trim(v, pad, where), (v[:30], pad, where)


def check_known_answers(ref):
    assert ref.substr(b"hello", 2, 3) == b"ell" and ref.substr(b"hello", -3, 2) == b"ll" and ref.substr(b"hello", 0, 3) == b""
    assert ref.substr(b"hello", 6) == b"" and ref.substr(b"hello", 5) == b"o" and ref.substr(b"hello", -5) == b"hello" and ref.substr(b"hello", -6) == b""
    assert ref.trim(b"ababxab", b"ab", R.TRIM_BOTH) == b"x" and ref.trim(b"aba", b"ab", R.TRIM_LEADING) == b"a" and ref.trim(b"aaa", b"aa", R.TRIM_BOTH) == b"a"


def test_slices_against_python_str():
    check_slices(R)


def test_trims_against_removeprefix_and_removesuffix():
    check_trims(R)


def test_known_answers():
    check_known_answers(R)


def test_units_on_arbitrary_bytes():
    """the definition itself on bytes that are no UTF-8: every byte not of the form 10xxxxxx starts a unit, and so does position 0"""
    assert R.length(b"\x80\x80a\xbf") == 2 and R.length(b"\x80") == 1 and R.length(b"\xbf\xbf\xbf") == 1 and R.length(b"a\x80b\x80\x80") == 2
    assert R.substr(b"\x80\x80a\xbf", 1, 1) == b"\x80\x80" and R.substr(b"\x80\x80a\xbf", 2) == b"a\xbf" and R.right(b"\x80\x80a\xbf", 1) == b"a\xbf"
    assert R.left(b"a\x80b\x80\x80", 1) == b"a\x80" and R.substr(b"a\x80b\x80\x80", -1) == b"b\x80\x80"


def test_concat_and_case_mapping_against_bytes():
    for op, args in K.build_rows():
        joined = b"".join(args)
        assert R.build(op, args) == (joined if op == R.CONCAT else (joined.upper() if op == R.UPPER else joined.lower()))
        assert R.non_ascii(args) == (not joined.isascii())
    assert R.build(R.CONCAT, [b"a", None]) is None and not R.non_ascii([b"\xff", None])
    assert R.build(R.UPPER, [b"@[`{az"]) == b"@[`{AZ" and R.build(R.LOWER, [b"@[`{AZ"]) == b"@[`{az"


def test_views():
    assert R.view(b"abc") == b"\x03\0\0\0abc" + bytes(9) and R.view(b"") == bytes(16) and len(R.view(b"x" * 12)) == 16
    assert R.view(b"0123456789abc", 2, 77) == b"\x0d\0\0\0" + b"0123" + b"\x02\0\0\0" + b"\x4d\0\0\0"
    assert R.slice_view(b"0123456789abcdef", (2, 16), 1, 100) == b"\x0e\0\0\0" + b"2345" + b"\x01\0\0\0" + b"\x66\0\0\0"
    assert R.slice_view(b"0123456789abcdef", (2, 5), 1, 100) == R.view(b"234")


# ---- negative controls: a wrong reference must fail the checks above ------------------------------------------------------------------------
class OffByOneStart:
    """substr whose start is one unit late"""
    def __getattr__(self, name):
        return getattr(R, name)

    @staticmethod
    def substr(v, pos, ln=None, unit_byte=False):
        return R.substr(v, pos + 1 if pos > 0 else pos, ln, unit_byte)


class ByteStrippingTrim:
    """a trim that strips any byte of the pad instead of whole pads"""
    def __getattr__(self, name):
        return getattr(R, name)

    @staticmethod
    def trim(v, pad=b" ", where=R.TRIM_BOTH):
        if where in (R.TRIM_LEADING, R.TRIM_BOTH):
            v = v.lstrip(pad) if pad else v
        if where in (R.TRIM_TRAILING, R.TRIM_BOTH):
            v = v.rstrip(pad) if pad else v
        return v


def test_negative_controls():
    for wrong, checks in ((OffByOneStart(), (check_slices, check_known_answers)), (ByteStrippingTrim(), (check_trims, check_known_answers))):
        for check in checks:
            with pytest.raises(AssertionError):
                check(wrong)
