"""Plain-Python reference for String search and rewrite (include/dbhip.h a28: position, split_part, replace, lpad / rpad, repeat,
reverse), written from the header's definition and from nothing in the library. tests/test_strsearch_ref_cpu.py holds it to Python's own
bytes / str operations where the definitions coincide, to the header's known answers and to negative controls.

A value is `bytes`. Units and boundaries are tests/str_ref.py's (a22). A result longer than 2^32 - 1 bytes is TOO_LONG."""
from tests import str_ref as S

INT64_MIN, INT64_MAX = S.INT64_MIN, S.INT64_MAX
REPLACE, LPAD, RPAD, REPEAT, REVERSE = range(5)
MAX_LEN = (1 << 32) - 1
TOO_LONG = "too long"


def occurrences(v, needle):
    """the greedy left-to-right non-overlapping occurrences of a non-empty needle"""
    out, p, m = [], 0, len(needle)
    while p + m <= len(v):
        if v[p:p + m] == needle:
            out.append(p)
            p += m
        else:
            p += 1
    return out


def find_from(v, needle, b):
    """the smallest p >= b where the needle lies, None when there is none"""
    for p in range(b, len(v) - len(needle) + 1):
        if v[p:p + len(needle)] == needle:
            return p
    return None


def position(v, needle, start=1, unit_byte=False):
    b = S.bounds(v, unit_byte)
    u = len(b) - 1
    if start <= 0 or start > u + 1:
        return 0
    if not needle:
        return start
    p = find_from(v, needle, b[start - 1])
    if p is None:
        return 0
    return 1 + sum(1 for q in b if 0 < q <= p)


def fields(v, delim):
    """the byte ranges of the fields between the occurrences of delim"""
    if not delim:
        return [(0, len(v))]
    out, s = [], 0
    for p in occurrences(v, delim):
        out.append((s, p))
        s = p + len(delim)
    return out + [(s, len(v))]


def split_range(v, delim, part):
    """the byte range of split_part's result, None when the part lies beyond the list"""
    f = fields(v, delim)
    if part == 0:
        part = 1
    k = part - 1 if part > 0 else len(f) + part
    return f[k] if 0 <= k < len(f) else None


def split_part(v, delim, part):
    r = split_range(v, delim, part)
    return b"" if r is None else v[r[0]:r[1]]


def units(v, unit_byte=False):
    b = S.bounds(v, unit_byte)
    return [v[s:e] for s, e in zip(b, b[1:])]


def rewrite_len(op, v, k=0, x=b"", y=b"", unit_byte=False):
    """the result's length, decided without building it; TOO_LONG past 2^32 - 1"""
    if op == REPLACE:
        n = len(v) + len(occurrences(v, x)) * (len(y) - len(x)) if x else len(v)
    elif op in (LPAD, RPAD):
        vu, pu = units(v, unit_byte), units(x, unit_byte)
        if k <= 0:
            n = 0
        elif k <= len(vu):
            n = sum(len(t) for t in vu[:k])
        elif not pu:
            n = 0
        elif k > MAX_LEN:
            return TOO_LONG
        else:
            f = k - len(vu)
            n = len(v) + (f // len(pu)) * len(x) + sum(len(t) for t in pu[:f % len(pu)])
    elif op == REPEAT:
        n = 0 if k <= 0 else len(v) * k
    else:
        n = len(v)
    return TOO_LONG if n > MAX_LEN else n


def rewrite(op, v, k=0, x=b"", y=b"", unit_byte=False):
    if rewrite_len(op, v, k, x, y, unit_byte) == TOO_LONG:
        return TOO_LONG
    if op == REPLACE:
        if not x:
            return v
        out, s = b"", 0
        for p in occurrences(v, x):
            out += v[s:p] + y
            s = p + len(x)
        return out + v[s:]
    if op in (LPAD, RPAD):
        vu, pu = units(v, unit_byte), units(x, unit_byte)
        if k <= 0:
            return b""
        if k <= len(vu):
            return b"".join(vu[:k])
        if not pu:
            return b""
        fill = b"".join(pu[i % len(pu)] for i in range(k - len(vu)))
        return fill + v if op == LPAD else v + fill
    if op == REPEAT:
        return b"" if k <= 0 else v * k
    return b"".join(reversed(units(v, unit_byte)))


def replace(v, frm, to):
    return rewrite(REPLACE, v, x=frm, y=to)


def lpad(v, length, pad, unit_byte=False):
    return rewrite(LPAD, v, length, pad, unit_byte=unit_byte)


def rpad(v, length, pad, unit_byte=False):
    return rewrite(RPAD, v, length, pad, unit_byte=unit_byte)


def repeat(v, k):
    return rewrite(REPEAT, v, k)


def reverse(v, unit_byte=False):
    return rewrite(REVERSE, v, unit_byte=unit_byte)
