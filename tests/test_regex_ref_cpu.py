"""CPU: tests/regex_ref.py — the plain-Python restatement of the regular-expression predicates (include/dbhip.h a25) that the host
checker and the GPU tests are held to — against Python's `re` wherever the two are defined alike, and against negative controls where
the a25 comment defines something else on purpose."""
import re

import pytest

from tests import regex_cases as K
from tests import regex_ref as R


def re_flags(flags):
    return (re.I if flags & K.CI else 0) | (re.S if flags & K.NL else 0)


def re_bytes(pattern, flags):
    """the pattern for `re` on bytes: `$` matches only at the very end there when it is written \\Z"""
    out, i, in_class = b"", 0, False
    while i < len(pattern):
        c = pattern[i:i + 1]
        if c == b"\\":
            out += pattern[i:i + 2]
            i += 2
            continue
        if c == b"[" and not in_class:
            in_class = True
        elif c == b"]":
            in_class = False
        out += rb"\Z" if c == b"$" and not in_class else c
        i += 1
    return re.compile(out, re_flags(flags))


def expect_re(pattern, flags, value, as_str):
    rx = re_bytes(pattern, flags)
    if as_str:
        rx = re.compile(rx.pattern.decode("utf-8"), re_flags(flags))
        value = value.decode("utf-8")
    return bool(rx.fullmatch(value) if flags & K.FM else rx.search(value))


def is_utf8(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def uses_ascii_sets(pattern, flags):
    return R.needs_ascii(pattern, flags)


def test_byte_unit_against_re_on_bytes():
    """UNIT_BYTE: every value, valid UTF-8 or not"""
    values = K.FIXED + K.byte_values(21, 600) + K.random_values(22, 300) + K.length_values()[:40]
    n = 0
    for pattern, flags in K.PATTERNS:
        if not flags & K.UB:
            continue
        for v in values:
            got = R.match(pattern, flags, v)
            if got == R.DECLINED:
                assert uses_ascii_sets(pattern, flags) and any(b >= 0x80 for b in v)
                continue
            assert got == expect_re(pattern, flags, v, False), (pattern, flags, v)
            n += 1
    assert n > 5000


def test_unit_mode_against_re_on_str():
    """without UNIT_BYTE, on valid UTF-8: one unit is one code point"""
    values = [v for v in K.FIXED if is_utf8(v)] + K.utf8_values(23, 800) + K.random_values(24, 300)
    values = [v for v in values if is_utf8(v)]
    n = 0
    for pattern, flags in K.PATTERNS:
        if flags & K.UB or uses_ascii_sets(pattern, flags):
            continue
        for v in values:
            assert R.match(pattern, flags, v) == expect_re(pattern, flags, v, True), (pattern, flags, v)
            n += 1
    assert n > 20000


def test_ascii_sets_and_folding_against_re_on_bytes():
    """CASE_INSENSITIVE and \\d \\w \\s: ASCII-only values against `re` on bytes (whose sets are the ASCII ones); others are declined"""
    values = [v for v in K.FIXED + K.random_values(25, 600) + K.length_values()[:40]]
    n = declined = 0
    for pattern, flags in K.PATTERNS:
        if not uses_ascii_sets(pattern, flags):
            continue
        for v in values:
            got = R.match(pattern, flags, v)
            if any(b >= 0x80 for b in v):
                assert got == R.DECLINED
                declined += 1
                continue
            assert got == expect_re(pattern, flags, v, False), (pattern, flags, v)
            n += 1
    assert n > 3000 and declined > 300


def test_needs_ascii_rows():
    for pattern, flags, want in [(b"a", 0, False), (b"a", K.CI, True), (b"1", K.CI, True), (rb"\d", 0, True), (rb"[\w]", 0, True), (rb"\S", K.UB, True),
                                 (rb"\\d", 0, False), (rb"[^a]\.", K.NL | K.FM, False)]:
        assert R.needs_ascii(pattern, flags) == want, (pattern, flags)


def test_where_the_definition_differs_from_re_on_purpose():
    """the check above has teeth: here the restatement and `re` must NOT agree"""
    assert R.match(b"a$", 0, b"a\n") is False and re.search("a$", "a\n")
    assert R.match(rb"\s", 0, b"\x1c") is False and re.search(r"\s", "\x1c")
    assert R.match(b"k", K.CI, "\u212a".encode()) == R.DECLINED and re.search("k", "\u212a", re.I)
    assert R.match(rb"\d", 0, "\u0661".encode()) == R.DECLINED and re.search(r"\d", "\u0661")
    assert R.match(b"^.$", 0, b"\xa9") is False and re.search(rb"^.\Z", b"\xa9")          # a continuation byte that follows no lead byte
    assert R.match(b"^.$", 0, b"\xc3\xa9\xa9") is True and not re.search(rb"^.\Z", b"\xc3\xa9\xa9")   # a lead byte takes EVERY continuation byte behind it
    assert R.match(b"^.$", K.UB, "é".encode()) is False and R.match(b"^.$", 0, "é".encode()) is True


@pytest.mark.parametrize("pattern", [rb"a\b", rb"a*+", rb"(?i)a", rb"a{,3}", rb"[[:alpha:]]", rb"[a&&b]", rb"\1", rb"(?=a)", rb"[]a]", rb"\xe9", b"\xff"])
def test_outside_the_grammar(pattern):
    assert not R.supported(pattern, 0)


def test_limits():
    assert R.supported(b"a" * 1024) and not R.supported(b"a" * 1025)
    assert R.supported(b"a{1000}") and not R.supported(b"a{1001}") and not R.supported(b"a{2,1}")
    assert R.supported(b"(a{1000}){4}") and not R.supported(b"(a{1000}){5}") and not R.supported(b".{1000}.{400}")
    assert R.supported(rb"\xe9", K.UB) and not R.supported("é".encode(), K.CI) and R.supported("é+".encode(), 0)
