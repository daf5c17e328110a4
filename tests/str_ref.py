"""Plain-Python reference for the String functions of include/dbhip.h a22 (length, substr / left / right, trim, concat, upper / lower),
written from the header's definition and from nothing in the library. tests/test_str_ref_cpu.py holds it to Python's own bytes / str
operations where the definitions coincide, to the header's known answers and to negative controls.

A value is `bytes`; None is NULL. A slice is returned as its byte range (start, end) of the source, so that a test can also check WHERE a
long result points."""
import functools
import struct

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
SUBSTR, LEFT, RIGHT, TRIM_LEADING, TRIM_TRAILING, TRIM_BOTH = range(6)
CONCAT, UPPER, LOWER = range(3)
INLINE_MAX = 12
E2, E3, E4 = "é".encode(), "€".encode(), "😀".encode()


def is_cont(c):
    return (c & 0xC0) == 0x80


@functools.lru_cache(maxsize=4096)
def bounds(v, unit_byte=False):
    """the unit boundaries of v: position 0, every byte not of the form 10xxxxxx, position len (each once, ascending)"""
    if unit_byte:
        return tuple(range(len(v) + 1))
    return tuple(sorted({0, len(v)} | {i for i in range(1, len(v)) if not is_cont(v[i])}))


def length(v, unit_byte=False):
    return len(bounds(v, unit_byte)) - 1


def substr_range(v, pos, ln=None, unit_byte=False):
    b = bounds(v, unit_byte)
    u = len(b) - 1
    if pos == 0:
        return 0, 0
    start = pos - 1 if pos > 0 else u + pos
    if start < 0 or start >= u:
        return 0, 0
    if ln is not None and ln <= 0:
        return 0, 0
    cnt = u - start if ln is None else min(ln, u - start)
    return b[start], b[start + cnt]


def left_range(v, k, unit_byte=False):
    b = bounds(v, unit_byte)
    return (0, 0) if k <= 0 else (0, b[min(k, len(b) - 1)])


def right_range(v, k, unit_byte=False):
    b = bounds(v, unit_byte)
    u = len(b) - 1
    return (0, 0) if k <= 0 else (b[u - min(k, u)], len(v))


def trim_range(v, pad, where=TRIM_BOTH):
    s, e, p = 0, len(v), len(pad)
    if p:
        if where in (TRIM_LEADING, TRIM_BOTH):
            while e - s >= p and v[s:s + p] == pad:
                s += p
        if where in (TRIM_TRAILING, TRIM_BOTH):
            while e - s >= p and v[e - p:e] == pad:
                e -= p
    return s, e


def slice_range(op, v, a=0, b=None, pad=b"", unit_byte=False):
    if op == SUBSTR:
        return substr_range(v, a, b, unit_byte)
    if op == LEFT:
        return left_range(v, a, unit_byte)
    if op == RIGHT:
        return right_range(v, a, unit_byte)
    return trim_range(v, pad, op)


def cut(v, rng):
    s, e = rng
    return v[s:e] if e > s else b""


def substr(v, pos, ln=None, unit_byte=False):
    return cut(v, substr_range(v, pos, ln, unit_byte))


def left(v, k, unit_byte=False):
    return cut(v, left_range(v, k, unit_byte))


def right(v, k, unit_byte=False):
    return cut(v, right_range(v, k, unit_byte))


def trim(v, pad=b" ", where=TRIM_BOTH):
    return cut(v, trim_range(v, pad, where))


def map_byte(op, c):
    if op == UPPER and 0x61 <= c <= 0x7A:
        return c - 0x20
    if op == LOWER and 0x41 <= c <= 0x5A:
        return c + 0x20
    return c


def build(op, args):
    """concat / upper / lower of one row's arguments: None when any is NULL"""
    if any(a is None for a in args):
        return None
    return bytes(map_byte(op, c) for a in args for c in a)


def non_ascii(args):
    return all(a is not None for a in args) and any(c >= 0x80 for a in args for c in a)


# ---- views ------------------------------------------------------------------------------------------------------------------------------
ZERO_VIEW = bytes(16)


def view(v, index=0, offset=0):
    """the 16 bytes of v's view: canonical inline up to 12 bytes, else {len, first four bytes, index, offset}"""
    if len(v) <= INLINE_MAX:
        return struct.pack("<I", len(v)) + v + bytes(INLINE_MAX - len(v))
    return struct.pack("<I", len(v)) + v[:4] + struct.pack("<II", index, offset)


def slice_view(v, rng, index=0, offset=0):
    """the view of the slice rng of a value whose own (long) view is {.., index, offset}"""
    s, e = rng
    return view(cut(v, rng), index, (offset + s) & 0xFFFFFFFF)
