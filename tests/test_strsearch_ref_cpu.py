"""CPU: tests/strsearch_ref.py — the plain reference of include/dbhip.h a28 — held to Python's own bytes / str operations where the
definitions coincide, to hand-written known answers and to negative controls; and the coverage conditions of tests/strsearch_cases.py
evaluated against it, so they are known to hold before any GPU run."""
import numpy as np
import pytest

from tests import str_ref as S
from tests import strsearch_cases as K
from tests import strsearch_ref as R


def samples():
    rng = np.random.default_rng(28)
    out = [b"", b"a", b"aaaaa", b"ababa", b"a,b,,c", b",", b",,"]
    for _ in range(300):
        n = int(rng.integers(0, 40))
        out.append(bytes(rng.choice(np.frombuffer(b"ab,-", dtype=np.uint8), n)))
    return out


def test_position_is_bytes_find_in_byte_mode():
    for v in samples():
        for nd in (b"a", b"ab", b",", b"aa", b"aba", b""):
            for start in range(1, len(v) + 2):
                assert R.position(v, nd, start, unit_byte=True) == v.find(nd, start - 1) + 1, (v, nd, start)
            assert R.position(v, nd, 0, True) == 0 and R.position(v, nd, len(v) + 2, True) == 0 and R.position(v, nd, -1, True) == 0


def test_position_is_str_find_on_valid_utf8():
    text = "aé€😀b€éa😀😀€"
    v = text.encode()
    for nd in ("€", "é", "😀😀", "a", "b€", "zz"):
        for start in range(1, len(text) + 2):
            assert R.position(v, nd.encode(), start) == text.find(nd, start - 1) + 1, (nd, start)


def test_replace_is_bytes_replace():
    for v in samples():
        for frm in (b"a", b"ab", b",", b"aa", b"aba"):
            for to in (b"", b"x", b"aa", b"abab"):
                assert R.replace(v, frm, to) == v.replace(frm, to), (v, frm, to)
                assert R.rewrite_len(R.REPLACE, v, x=frm, y=to) == len(v.replace(frm, to))
        assert R.replace(v, b"", b"x") == v


def test_fields_are_bytes_split():
    for v in samples():
        for d in (b",", b"ab", b"aa", b"-"):
            assert [v[s:e] for s, e in R.fields(v, d)] == v.split(d), (v, d)
            parts = v.split(d)
            for k in range(1, len(parts) + 1):
                assert R.split_part(v, d, k) == parts[k - 1] and R.split_part(v, d, -k) == parts[-k]
            assert R.split_part(v, d, len(parts) + 1) == b"" and R.split_part(v, d, -len(parts) - 1) == b""
        assert R.fields(v, b"") == [(0, len(v))]


def test_reverse_and_pads_are_pythons_on_valid_utf8():
    for text in ("", "a", "héllo", "€uro 😀!", "ab" * 20 + "é"):
        v = text.encode()
        assert R.reverse(v) == text[::-1].encode()
        assert R.reverse(v, unit_byte=True) == v[::-1]
        for k in range(0, len(text) + 6):
            for pad in ("*", "€"):
                want_l = text.rjust(k, pad) if k >= len(text) else text[:k]
                want_r = text.ljust(k, pad) if k >= len(text) else text[:k]
                assert R.lpad(v, k, pad.encode()) == want_l.encode() and R.rpad(v, k, pad.encode()) == want_r.encode(), (text, k, pad)
        assert R.repeat(v, 3) == v * 3 and R.repeat(v, 0) == b"" and R.repeat(v, -2) == b""


def test_known_answers():
    assert R.occurrences(b"aaaaa", b"aa") == [0, 2]
    assert [R.split_part(b"a,b,,c", b",", p) for p in (1, 3, 4, 5, -1, -4, -5, 0)] == [b"a", b"", b"c", b"", b"c", b"a", b"", b"a"]
    assert R.lpad(b"hi", 5, b"xy") == b"xyxhi" and R.rpad(b"hi", 1, b"x") == b"h" and R.lpad(b"hi", 5, b"") == b""
    assert R.position(b"abc", b"", 4) == 4 and R.position(b"abc", b"", 5) == 0
    assert R.repeat(b"x", R.INT64_MAX) == R.TOO_LONG and R.lpad(b"x", R.INT64_MAX, b"ab") == R.TOO_LONG
    assert R.split_part(b"abc", b",", R.INT64_MIN) == b"" and R.split_part(b"abc", b",", R.INT64_MAX) == b""
    assert R.lpad(b"h" + S.E3, 4, b"a" + S.E2) == b"a" + S.E2 + b"h" + S.E3 and R.rpad(b"ab", 5, b"\x80x\xbf") == b"ab\x80x\xbf\x80"
    assert R.reverse(b"a" + S.E3 + b"\x80") == S.E3 + b"\x80a"


# ---- negative controls: a reference with one of the definition's rules dropped is caught by a named assertion -----------------------------
def ignores_start(v, nd, start=1, unit_byte=False):
    return R.position(v, nd, 1, unit_byte)


def overlapping(v, needle):
    return [p for p in range(len(v) - len(needle) + 1) if v[p:p + len(needle)] == needle]


def part_zero_is_empty(v, delim, part):
    return b"" if part == 0 else R.split_part(v, delim, part)


def check_start(position):
    assert position(b"abcabc", b"abc", 2) == 4, "start is honoured"


def check_non_overlapping(occurrences):
    assert occurrences(b"aaaaa", b"aa") == [0, 2], "occurrences do not overlap"


def check_part_zero(split_part):
    assert split_part(b"a,b", b",", 0) == b"a", "part 0 is part 1"


def test_negative_controls():
    check_start(R.position)
    check_non_overlapping(R.occurrences)
    check_part_zero(R.split_part)
    for check, broken, name in ((check_start, ignores_start, "start is honoured"), (check_non_overlapping, overlapping, "occurrences do not overlap"),
                                (check_part_zero, part_zero_is_empty, "part 0 is part 1")):
        with pytest.raises(AssertionError, match=name):
            check(broken)


def test_the_case_list_covers_what_it_must():
    pos = [R.position(v, nd, s) for v, nd, s in K.position_rows(False)]
    split = [R.split_range(v, d, p) for v, d, p in K.split_rows()]
    rew = [R.rewrite(op, v, k, x, y, ub) for op, v, k, x, y, ub in K.rewrite_rows()]
    K.coverage(pos, split, rew)
    assert max(len(a) for a in rew if a != R.TOO_LONG) < 1 << 20, "no case builds a huge value"
