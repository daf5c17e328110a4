"""The case list shared by tests/test_strsearch_host_cpu.py (dev_strsearch.h compiled for the host) and tests/test_gpu_strsearch.py (the
kernels): values built around every needle, and per value the start / part / length / count arguments that the issue of group a28
names. Deterministic. coverage() states what the list must contain as conditions on the reference's answers; the CPU test evaluates
it, so it is known to hold before any GPU run."""
from tests import str_ref as S
from tests import strfn_cases as K
from tests import strsearch_ref as R

E2, E3, E4 = S.E2, S.E3, S.E4
# needles / delimiters of 1, 2, 4, 5, 13 and 255 bytes, and the empty one
N255 = (b"Qr" + E3 + b"st" + E2 + b"uvw" + E4) * 15 + b"Qrstuvwxyz01234"
NEEDLES = [b"-", b"aa", b"abab", b"ab" + E3, b"abcdefghijklm", N255, b""]
assert [len(x) for x in NEEDLES] == [1, 2, 4, 5, 13, 255, 0]
# pads: one 1-byte unit, one 3-byte unit, mixed units, a stray continuation byte in front, two bytes, none
PADS = [b"*", E3, b"a" + E2 + E3 + b"z", b"\x80x\xbf", b"xy", b""]
# replace: grows, shrinks, keeps the length, deletes; long constants; nothing to find
REPLACES = [(b"-", b"--+"), (b"abab", b"z"), (b"aa", b"bb"), (b"-", b""), (b"abcdefghijklm", N255), (N255, b""), (b"ab" + E3, b"0123456789ABC"), (b"", b"never"),
            (b"aa", b"aaa")]


def fill(n, k=0):
    """n bytes that hold no needle: ASCII and 2-byte units, cut anywhere (a cut unit leaves stray bytes: still defined)"""
    unit = b"x." + E2 + b"y"
    return (unit * (n // len(unit) + 2))[k % len(unit):][:n]


def around(nd):
    """values built around a non-empty needle: an occurrence at 0, at the end, straddling a 4-byte word at every phase, straddling byte
    256 (positions 250..262), twice in a row, separated, none (also one byte short), the value equal to the needle"""
    out = [nd, nd + fill(9), fill(9) + nd, nd[:-1] + b"~", fill(30), nd + nd, nd + nd + nd[:-1], fill(2) + nd + fill(1) + nd + fill(3) + nd]
    out += [fill(k, k) + nd + fill(7 - k) for k in range(1, 8)]
    out += [fill(p, p) + nd + fill(5) for p in range(250, 263)]
    out += [fill(300) + nd[:-1], fill(700, 1) + nd + fill(300) + nd]
    return out


OVERLAPS = [b"aaaaa", b"ababa", b"aaaa", b"abababab", b"aaaaaaaaaaaaa", b"ab" * 150 + b"a", b"a" * 600]


def pool(nd):
    """the values one needle is tried on"""
    return K.values() + OVERLAPS + (around(nd) if nd else around(b"-"))


def _edges(u):
    return sorted({0, 1, -1, u - 1, -(u - 1), u, -u, u + 1, -(u + 1), u + 2, R.INT64_MIN, R.INT64_MAX})


def position_rows(unit_byte):
    """(value, needle, start): the values of the a22 list at three starts, the values around the needle at every edge of the start"""
    rows = []
    for nd in NEEDLES:
        base = len(K.values())
        for i, v in enumerate(pool(nd)):
            u = S.length(v, unit_byte)
            starts = [1, 2 + i % 5, u] if i < base else _edges(u) + [2, 3, 5]
            rows += [(v, nd, s) for s in starts]
    return rows


def split_rows():
    """(value, delimiter, part): part over the edges of the FIELD count"""
    rows = []
    for nd in NEEDLES:
        base = len(K.values())
        for i, v in enumerate(pool(nd)):
            f = len(R.fields(v, nd))
            parts = [1, -1, 2 + i % 3] if i < base else _edges(f) + [2, -2, 3]
            rows += [(v, nd, p) for p in parts]
    # the issue's own example
    rows += [(b"a,b,,c", b",", p) for p in (1, 3, 4, 5, -1, -4, -5, 0)]
    return rows


def _some_values():
    """three values per length of the a22 list: mixed UTF-8, arbitrary bytes, stray continuation bytes"""
    vals = K.values()
    return [vals[8 * g + j] for g in range(len(K.LENGTHS)) for j in (1, 3, 4)]


def rewrite_rows():
    """(op, value, k, x, y, unit_byte)"""
    rows = []
    for frm, to in REPLACES:
        rows += [(R.REPLACE, v, 0, frm, to, False) for v in pool(frm)]
    for vi, v in enumerate(_some_values() + [b"hi", b"h" + E3 + b"!", E2 * 3]):
        for unit_byte in (False, True):
            for ki, k in enumerate(_edges(S.length(v, unit_byte)) + [5, 12, 13, 256, 257, 600]):
                pad = PADS[(vi + ki) % len(PADS)]
                rows += [(R.LPAD, v, k, pad, b"", unit_byte), (R.RPAD, v, k, pad, b"", unit_byte)]
    for v in K.values():
        rows += [(R.REPEAT, v, k, b"", b"", False) for k in (0, 1, -1, 2, 3, R.INT64_MIN, R.INT64_MAX, (1 << 32) // max(len(v), 1) + 1)]
    for v in K.values() + OVERLAPS + around(b"ab" + E3) + [b"\x80" * 300, b"a" + b"\xbf" * 70 + b"b" + b"\x80" * 130 + E4 * 30]:
        rows += [(R.REVERSE, v, 0, b"", b"", False), (R.REVERSE, v, 0, b"", b"", True)]
    # results of 0, 12, 13, 256 and 257 bytes from inline and from long sources
    dashed = b"".join(b"x" * 6 + b"-" for _ in range(43))
    rows += [(R.REPLACE, b"---", 0, b"-", b"", False), (R.REPLACE, b"-" * 300, 0, b"-", b"", False), (R.REPEAT, b"abc", 4, b"", b"", False),
             (R.LPAD, b"hi", 13, b"xy", b"", False), (R.REPEAT, b"abcd", 64, b"", b"", False), (R.LPAD, b"a", 257, b"xy", b"", False),
             (R.RPAD, fill(300), 12, b"*", b"", True), (R.RPAD, fill(300), 13, b"*", b"", True),
             (R.REPLACE, dashed[:299], 0, b"-", b"", False), (R.REPLACE, dashed[:299] + b"q", 0, b"-", b"", False),
             (R.REPLACE, b"a-b-c-d-e-f-", 0, b"-", N255, False), (R.RPAD, b"x" * 255, 256, E3, b"", True), (R.LPAD, b"x" * 255, 257, E3, b"", True),
             (R.REPEAT, b"x", R.INT64_MAX, b"", b"", False), (R.LPAD, b"x", R.INT64_MAX, b"ab", b"", False), (R.LPAD, fill(400), R.INT64_MAX, b"ab", b"", False),
             (R.LPAD, b"hi", 5, b"xy", b"", False), (R.RPAD, b"hi", 1, b"x", b"", False), (R.LPAD, b"hi", 5, b"", b"", False)]
    return rows


def coverage(position_answers, split_answers, rewrite_answers):
    """the conditions the list must meet, on the reference's answers: lists parallel to position_rows(False), split_rows() (byte ranges or
    None) and rewrite_rows() (bytes or R.TOO_LONG)"""
    prow = position_rows(False)
    hits = [(v, nd, s, a) for (v, nd, s), a in zip(prow, position_answers) if a > 0 and nd]
    at = {(len(nd), R.find_from(v, nd, S.bounds(v)[s - 1])) for v, nd, s, a in hits}
    for m in (1, 2, 4, 5, 13, 255):
        ps = {p for mm, p in at if mm == m}
        assert 0 in ps, ("an occurrence at 0", m)
        assert any(p < 256 < p + m for p in ps) or m == 1, ("an occurrence straddling byte 256", m)
        assert any(p % 4 + m > 4 for p in ps) or m == 1, ("an occurrence straddling a 4-byte word", m)
        assert any(p == 256 for p in ps), ("an occurrence that starts the second step", m)
    assert any(a == 0 for a in position_answers) and any(v == nd and a == 1 for v, nd, s, a in hits)
    assert any(nd == b"" and a == s > 1 for (v, nd, s), a in zip(prow, position_answers)), "an empty needle at a start past 1"
    assert any(r is None for r in split_answers) and any(r is not None and r[0] == r[1] for r in split_answers), "a part beyond the list, an empty field"
    assert any(r is not None and r[1] - r[0] > 12 and r[0] > 256 for r in split_answers), "a long field behind byte 256"
    for inline in (True, False):
        lens = {len(a) for (op, v, k, x, y, ub), a in zip(rewrite_rows(), rewrite_answers) if a != R.TOO_LONG and (len(v) <= 12) == inline}
        assert {0, 12, 13, 256, 257} <= lens, ("result lengths from inline / long sources", inline, sorted(lens)[:40])
    assert sum(a == R.TOO_LONG for a in rewrite_answers) >= 3
    grew = {(len(a) > len(v)) - (len(a) < len(v)) for (op, v, k, x, y, ub), a in zip(rewrite_rows(), rewrite_answers) if op == R.REPLACE and a != v}
    assert grew == {-1, 0, 1}, "replace that grows, shrinks and keeps the length"
