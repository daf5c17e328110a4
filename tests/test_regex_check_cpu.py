"""CPU: dbhip_regex_check (include/dbhip.h a25) needs no device and no dbhip_init — the pattern is compiled on the host — so the
refusals, the argument checks, the limits and the reported figures are tested here through the raw binding; dbhip_regex_create refuses
the same patterns before any device call. tests/test_gpu_regex.py runs the accepted ones."""
import ctypes as C

import pytest

from databend_amd import _lib as T
from tests import regex_cases as K
from tests import regex_ref as R


def host(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")


def check(pattern, flags=0, length=None, want_info=True):
    info = (C.c_int32 * 4)(-1, -1, -1, -1)
    rc = T.lib().dbhip_regex_check(host(pattern) if pattern is not None else None, C.c_int32(len(pattern or b"") if length is None else length), C.c_int32(flags),
                                   info if want_info else None)
    return rc, list(info)


def refused(pattern, flags, code, what):
    rc, info = check(pattern, flags)
    assert rc == code, (what, pattern, rc)
    msg = T.lib().dbhip_last_error()
    assert msg and b"DBHIP_" not in msg, (what, msg)
    assert info == [-1, -1, -1, -1], "a refusal writes nothing"
    h = C.c_void_p()
    assert T.lib().dbhip_regex_create(host(pattern), C.c_int32(len(pattern)), C.c_int32(flags), C.byref(h)) == code and h.value is None, what
    assert b"DBHIP_" not in T.lib().dbhip_last_error()


UNSUPPORTED = [
    (rb"a{,3}", 0, "a { that forms no counted repetition"), (rb"a{2", 0, "an open {"), (rb"a{x}", 0, "a { with no number"), (rb"{2}", 0, "a { at the start"),
    (rb"a{1001}", 0, "m above 1000"), (rb"a{1,1001}", 0, "n above 1000"), (rb"a{3,2}", 0, "n below m"),
    (rb"^*", 0, "a quantifier on ^"), (rb"a$+", 0, "a quantifier on $"), (rb"*a", 0, "a quantifier at the start"), (rb"a|+b", 0, "a quantifier at the start of a branch"),
    (rb"(?:?a)", 0, "a quantifier at the start of a group"), (rb"a**", 0, "a quantifier on a quantifier"), (rb"a?+", 0, "a possessive quantifier"),
    (rb"[a&&b]", 0, "&&"), (rb"[a--b]", 0, "--"), (rb"[a~~b]", 0, "~~"), (rb"[[:alpha:]]", 0, "a POSIX class"), ("[é]".encode(), 0, "a byte above 7F in a class"),
    (rb"[\D]", 0, r"\D in a class"), (rb"[\W]", 0, r"\W in a class"), (rb"[\S]", 0, r"\S in a class"), (rb"[]a]", 0, "an unescaped ] first"), (rb"[a[]", 0, "an unescaped ["),
    (rb"[a^]", 0, "an unescaped ^"), (rb"[a\]", 0, "a class that does not end"), (rb"[z-a]", 0, "a descending range"), (rb"[a-c-e]", 0, "a - that forms no range"),
    (rb"\xe9", 0, r"\x above 7F without UNIT_BYTE"), (rb"\xg1", 0, r"\x without two digits"), (rb"\b", 0, r"\b"), (rb"\B", 0, r"\B"), (rb"\A", 0, r"\A"), (rb"\z", 0, r"\z"),
    (rb"\Z", 0, r"\Z"), (rb"\p{L}", 0, r"\p"), (rb"(a)\1", 0, "a backreference"), (rb"\0", 0, r"\0"), (rb"\e", 0, "an unknown escape"), (b"a\\", 0, "a trailing backslash"),
    (rb"(?i)a", 0, "inline flags"), (rb"(?m)^a", 0, "multi-line mode"), (rb"(?=a)", 0, "look-ahead"), (rb"(?<!a)b", 0, "look-behind"), (rb"(?<n>a)", 0, "another group form"),
    (rb"(?P<1>a)", 0, "a group name that is no identifier"), (rb"(?P=n)", 0, "a named backreference"), (rb"(a", 0, "an open group"), (rb"a)", 0, "a stray )"),
    (b"a\xffb", 0, "a byte that is no UTF-8"), (b"\xc3", 0, "a truncated UTF-8 sequence"), (b"\xed\xa0\x80", 0, "a surrogate"), (b"\xc0\xaf", 0, "an overlong sequence"),
    ("é".encode(), T.REGEX_CASE_INSENSITIVE, "a byte above 7F with CASE_INSENSITIVE"),
    (b"a" * 1025, 0, "a pattern of 1025 bytes"), (rb"(a{1000}){5}", 0, "5000 NFA positions"), (rb".{1000}.{400}", 0, "4200 NFA positions"),
    (rb"(a|b)*a(a|b){14}$", 0, "a minimal DFA of more than 2^15 states"), (rb"(a|b)*a(a|b){9}(c|d|e|f|g|h|i|j|k|l|m|n|o|p|q|r)$", 0, "a table beyond 32 KiB: about 1,000 states of 19 classes"),
    (b"(" * 65 + b"a" + b")" * 65, 0, "groups nested 65 deep"),
]


@pytest.mark.parametrize("pattern,flags,what", UNSUPPORTED, ids=[w for _, _, w in UNSUPPORTED])
def test_unsupported(pattern, flags, what):
    assert not R.supported(pattern, flags) or "DFA" in what or "table" in what       # (the restatement has no DFA and so no DFA caps)
    refused(pattern, flags, T.ERR_UNSUPPORTED, what)


def test_invalid_arguments():
    refused(b"a", 16, T.ERR_INVALID, "an unknown flag bit")
    refused(b"a", -1, T.ERR_INVALID, "negative flags")
    assert check(b"a", length=-1)[0] == T.ERR_INVALID and b"DBHIP_" not in T.lib().dbhip_last_error()
    assert check(None, length=3)[0] == T.ERR_INVALID
    assert T.lib().dbhip_regex_create(host(b"a"), C.c_int32(1), C.c_int32(0), None) == T.ERR_INVALID
    assert T.lib().dbhip_regex_destroy(None) == T.OK
    out = C.c_void_p()
    cc = T.Col()
    assert T.lib().dbhip_regex_eval(None, C.byref(cc), C.c_int32(0), C.c_int64(0), None, None, None, None) == T.ERR_INVALID


def test_what_is_accepted_and_reported():
    assert check(None, length=0) == (T.OK, [1, 1, 2, 0]), "the empty pattern: one sticky state"
    assert check(b"a", want_info=False)[0] == T.OK
    for pattern, flags in K.PATTERNS:
        rc, (states, classes, nbytes, ascii_rows) = check(pattern, flags)
        assert rc == T.OK, (pattern, flags, T.lib().dbhip_last_error())
        assert 1 <= states <= T.REGEX_MAX_STATES and 1 <= classes <= 256 and nbytes == states * classes * 2 <= T.REGEX_MAX_TABLE_BYTES
        assert ascii_rows == int(R.needs_ascii(pattern, flags)), (pattern, flags)
    for pattern, flags, want in [(b"a", 0, 0), (b"a", T.REGEX_CASE_INSENSITIVE, 1), (b"1", T.REGEX_CASE_INSENSITIVE, 1), (rb"\d", 0, 1), (rb"[\w]", 0, 1), (rb"\s", 0, 1),
                                 (rb"\D", 0, 1), (rb"\W", 0, 1), (rb"\S", T.REGEX_UNIT_BYTE, 1), (rb"\\d", 0, 0), (rb"[^a].", T.REGEX_DOT_NL | T.REGEX_FULL_MATCH, 0)]:
        assert check(pattern, flags)[1][3] == want, (pattern, flags)


def test_the_limits_themselves_are_accepted():
    assert check(b"a" * 1024)[0] == T.OK and check(b"a{1000}")[0] == T.OK and check(b"(a{1000}){4}")[0] == T.OK and check(b"a{0,1000}")[0] == T.OK
    assert check(rb"\xe9", T.REGEX_UNIT_BYTE)[0] == T.OK and check(b"a\xffb", T.REGEX_UNIT_BYTE)[0] == T.OK and check("é+".encode())[0] == T.OK
    assert check(b"(" * 64 + b"a" + b")" * 64)[0] == T.OK


def test_a_thousand_states_and_a_table_of_more_than_one_staging_round():
    """state numbers above 255, and more than 256 lanes * 16 bytes of table. The exact counts depend on the construction and are not
    asserted."""
    rc, (states, classes, nbytes, ascii_rows) = check(K.BIG)
    assert rc == T.OK and states > 1000 and classes >= 11 and nbytes > 20000 and ascii_rows == 0
    rc, (states, classes, nbytes, _) = check(K.DOT255)
    assert rc == T.OK and states >= 256
