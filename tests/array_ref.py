"""The reference for the Array functions (include/dbhip.h a29) over Python lists, in plain Python: independent of the device code and
of csrc/dev_array.h. A row is a list of elements, None = a NULL element; integers, dates and decimals are Python ints (exact), floats
are Python floats or numpy scalars judged with tests/float_ref.py (of_cmp for equality and order, sum_expected for SUM), Strings are
bytes.

* row_runs            the runs of an offsets list: (start, len, bad) per row; a bad row is an empty run
* length / get        get is 1-based, negative from the end, None outside the run or on a NULL element
* indexof / contains  the FIRST equal non-NULL element; a NULL needle finds nothing
* reduce              COUNT / SUM / MIN / MAX with NULLs skipped; None for SUM / MIN / MAX without a value; OVERFLOW for a Decimal128 sum
                      outside the decimal range
* unnest_sel          the parent row of every unnested element
tests/test_array_ref_cpu.py holds it to Python's own len, indexing, list.index, sum, min and max and to negative controls."""
from tests import float_ref as F

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
COUNT, SUM, MIN, MAX = range(4)
CONTAINS, INDEXOF = range(2)
DEC128_MAX = 10 ** 38 - 1
OVERFLOW = "overflow"

# how a type's SUM behaves: wrapping to 64 bits signed / unsigned, a double sum, the checked Decimal128 sum; None: no SUM
SUM_CLASS = {"i8": "i64", "i16": "i64", "i32": "i64", "i64": "i64", "u8": "u64", "u16": "u64", "u32": "u64", "u64": "u64", "f32": "f", "f64": "f",
             "dec64": "i64", "dec128": "dec128", "date": None, "timestamp": None}


def row_runs(offsets, n_elems):
    out = []
    for r in range(len(offsets) - 1):
        a, b = offsets[r], offsets[r + 1]
        out.append((0, 0, True) if a > b or b > n_elems else (a, b - a, False))
    return out


def rows_of(offsets, elems):
    """the rows of an offsets list over the child's elements (a bad row is empty)"""
    return [elems[s:s + ln] for s, ln, _ in row_runs(offsets, len(elems))]


def length(row):
    return len(row)


def get(row, i):
    """arr[i]: None outside 1 .. len and -len .. -1, and for a NULL element"""
    n = len(row)
    if 1 <= i <= n:
        return row[i - 1]
    if -n <= i <= -1:
        return row[n + i]
    return None


def equal(a, b, is_float):
    return F.of_cmp(a, b) == 0 if is_float else a == b


def indexof(row, x, is_float=False):
    """1-based position of the first non-NULL element equal to x, 0 when there is none or x is NULL"""
    if x is None:
        return 0
    for k, e in enumerate(row):
        if e is not None and equal(e, x, is_float):
            return k + 1
    return 0


def contains(row, x, is_float=False):
    return indexof(row, x, is_float) != 0


def wrap(v, signed):
    v &= (1 << 64) - 1
    return v - (1 << 64) if signed and v >> 63 else v


def reduce(kind, row, tname):
    """tname: a key of SUM_CLASS. COUNT -> int; SUM -> int (wrapped) | float_ref.sum_expected tuple | OVERFLOW | None; MIN / MAX -> the
    value | None (floats by of_cmp: NaN greatest; among equals any is right, float_ref.same_value says so)"""
    vals = [e for e in row if e is not None]
    if kind == COUNT:
        return len(vals)
    if not vals:
        return None
    is_float = tname in ("f32", "f64")
    if kind == SUM:
        cls = SUM_CLASS[tname]
        assert cls is not None, "no SUM over " + tname
        if cls == "f":
            return F.sum_expected(vals)
        s = sum(vals)
        if cls == "dec128":
            return OVERFLOW if abs(s) > DEC128_MAX else s
        return wrap(s, cls == "i64")
    if is_float:
        return F.extreme([float(v) for v in vals], kind == MAX)
    return min(vals) if kind == MIN else max(vals)


def unnest_sel(offsets, n_elems):
    """out_sel[k - offsets[0]] = r for the elements k of row r, as a dict slot -> row (a well-formed column fills 0 .. num_out - 1)"""
    out = {}
    for r, (s, ln, _) in enumerate(row_runs(offsets, n_elems)):
        for k in range(s, s + ln):
            if k >= offsets[0]:
                out[k - offsets[0]] = r
    return out
