"""The case list shared by tests/test_strfn_host_cpu.py (dev_strfn.h compiled for the host) and tests/test_gpu_strfn.py (the kernels): the
values, and per value the position / length / count arguments and the pads that the issue of group a22 names. Deterministic."""
import numpy as np

from tests import str_ref as R

LENGTHS = [0, 1, 3, 4, 5, 11, 12, 13, 16, 17, 255, 256, 257, 1000]
PADS = [b" ", b"ab", b"abcdefghijklm", b"", b"\x80", b"x" * 255]


def _fit(unit, ln):
    """`unit` repeated and cut to ln bytes"""
    return (unit * (ln // len(unit) + 1))[:ln]


def values():
    """per length: ASCII, valid UTF-8 with 2-, 3- and 4-byte code points (cut to whole code points and filled with ASCII), arbitrary bytes
    with stray continuation bytes (also as the first and as the last byte), and values made of pads"""
    rng = np.random.default_rng(22)
    out = []
    for ln in LENGTHS:
        out.append(bytes(rng.integers(0x20, 0x7F, ln, dtype=np.uint8)))
        mixed, k = b"", 0
        units = [b"a", R.E2, R.E3, R.E4, b"Z", R.E3, R.E2]
        while len(mixed) + len(units[k % 7]) <= ln:
            mixed += units[k % 7]
            k += 1
        out.append(mixed + b"q" * (ln - len(mixed)))
        out.append(_fit(R.E4 + R.E2, ln - ln % 6) + b"." * (ln % 6))
        raw = bytearray(rng.integers(0, 256, ln, dtype=np.uint8))
        if ln:
            raw[0] = 0x80
            raw[-1] = 0xBF
        out.append(bytes(raw))
        out.append(_fit(b"\x80\x80a\xbf", ln))
        out.append(_fit(b"ab", ln))                                   # made only of the pad `ab` (an odd length leaves an `a`)
        out.append(_fit(b" ", min(ln, 3)) + _fit(b"x y", max(ln - 6, 0)) + _fit(b" ", max(min(ln - 3, 3), 0)))
        out.append(_fit(b"abcdefghijklm", ln))
    return out


def slice_args(v, unit_byte):
    """(op, a, b) for one value: pos / len / k over 0, +-1, +-(U - 1), +-U, +-(U + 1), the i64 extremes, len <= 0, and 12 / 13"""
    u = R.length(v, unit_byte)
    pos = sorted({0, 1, -1, 2, u - 1, -(u - 1), u, -u, u + 1, -(u + 1), 5, -12, -13, R.INT64_MIN, R.INT64_MAX})
    lens = [None, 0, -1, 1, 2, 12, 13, u - 1, u, u + 1, R.INT64_MIN, R.INT64_MAX]
    out = [(R.SUBSTR, p, ln) for p in pos for ln in lens]
    ks = sorted({0, 1, -1, 2, 12, 13, u - 1, u, u + 1, R.INT64_MIN, R.INT64_MAX})
    out += [(op, k, None) for op in (R.LEFT, R.RIGHT) for k in ks]
    return out


def build_rows():
    """rows of (op, [argument values]) for concat / upper / lower: 1, 2 and 8 arguments, totals of 0, 12, 13, 256 and 257 bytes, and the
    bytes next to the letter ranges"""
    a = b"abcdefghijkl"
    rows = [(R.CONCAT, [b""]), (R.CONCAT, [a]), (R.CONCAT, [a + b"m"]), (R.CONCAT, [b"", b""]), (R.CONCAT, [a[:5], a[:7]]), (R.CONCAT, [a[:6], a[:7]]),
            (R.CONCAT, [a * 20, a + b"wxyz"]), (R.CONCAT, [a * 20 + b"w", a + b"wxyz"]), (R.CONCAT, [b"x" * 300, R.E3 * 100]),
            (R.CONCAT, [b"a", b"", b"bc", R.E2, b"d", b"", b"e", b"fgh"]), (R.CONCAT, [a, b"-", a * 3, b"-", R.E4, a * 18, b"", b"0123456789abcdef" * 2]),
            (R.CONCAT, [b"1234", b"5678", b"9abc", b"", b"", b"", b"", b""]), (R.CONCAT, [b"1234", b"5678", b"9abc", b"d", b"", b"", b"", b""])]
    for op in (R.UPPER, R.LOWER):
        rows += [(op, [b""]), (op, [b"@AZ[`az{"]), (op, [b"Hello, World"]), (op, [b"Hello, World!"]), (op, [b"mIxEd " + R.E2 + b" \xc0\xff\x80 Case" * 3]),
                 (op, [bytes(range(256))]), (op, [bytes(range(256)) + b"a"]), (op, [b"abcXYZ" * 60])]
    return rows
