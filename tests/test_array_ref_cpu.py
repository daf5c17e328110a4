"""CPU: tests/array_ref.py, the reference of the Array functions, held to Python's own len, indexing, list.index, sum, min and max over
the case list (tests/array_cases.py), and to negative controls: a reference (or a kernel) with an off-by-one in get, a NULL element
that matches, an empty run that is not NULL or a first match that is not the first differs from it on that list."""
import math

import numpy as np
import pytest

from tests import array_cases as K
from tests import array_ref as R
from tests import float_ref as F


def all_rows(tname, for_sum=False):
    return [row for _, rows in K.columns(tname, for_sum) for row in rows]


def test_the_case_list_reaches_every_shape():
    for tname in K.TYPES:
        cols = dict(K.columns(tname))
        lens = {len(r) for r in cols["edges"]}
        assert {0, 1, 63, 64, 65, K.T - 1, K.T, K.T + 1, K.LONG_ROW} <= lens
        assert len(cols["edges"][0]) == 0 and len(cols["edges"][-1]) == 0
        assert [len(cols["n%d" % n]) for n in K.N_ROWS] == K.N_ROWS
        es = K.TYPES[tname][2]
        for d in (-1, 0, 1):
            group = cols["stage%+d" % d][64:128]
            assert sum(len(r) for r in group) == K.STAGE_BYTES // es + d and sum(1 for r in group if len(r) > K.T) <= 1
        assert all(len(r) == 0 for r in cols["all_empty"])
        rows = all_rows(tname)
        assert any(r and all(e is None for e in r) for r in rows), "a run of NULLs"
        assert any(r and all(e is not None for e in r) for r in rows)
    assert sorted(len(x) for x in K.STR_NEEDLES) == [0, 1, 4, 12, 13, 255]
    assert {len(s) % 4 for s in K.STRINGS if len(s) > 12} == {0, 1, 2, 3}, "long values at every alignment of a packed buffer"


@pytest.mark.parametrize("tname", ["i64", "u8", "string"])
def test_length_and_get_are_pythons(tname):
    for row in all_rows(tname):
        assert R.length(row) == len(row)
        for i in K.get_indexes([row])[0]:
            if i > 0 and i <= len(row):
                exp = row[i - 1]
            elif i < 0 and -i <= len(row):
                exp = row[i]                                   # Python's own negative indexing
            else:
                exp = None
            assert R.get(row, i) == exp, (len(row), i)


@pytest.mark.parametrize("tname", ["i16", "u64", "dec128", "string"])
def test_indexof_is_list_index(tname):
    hits = 0
    for _, rows in K.columns(tname):
        for row, x in zip(rows, K.needles(tname, rows, 5)):
            clean = [e if e is not None else object() for e in row]          # a NULL equals nothing
            exp = clean.index(x) + 1 if x is not None and x in clean else 0
            assert R.indexof(row, x) == exp and R.contains(row, x) == (exp != 0)
            hits += exp > 1
    assert hits > 10, "matches behind the first element"


@pytest.mark.parametrize("tname", ["f32", "f64"])
def test_float_equality_is_of_cmp(tname):
    dt = K.TYPES[tname][1]
    nan, zero = (F.NAN32, F.ZERO32) if tname == "f32" else (F.NAN64, F.ZERO64)
    assert R.indexof([dt(1.0), nan[1], nan[0]], nan[3], True) == 2           # NaN equals NaN whatever the sign or payload
    assert R.indexof([dt(1.0), zero[1]], zero[0], True) == 2                 # -0.0 equals 0.0
    assert R.indexof([dt(1.0), None, dt(2.0)], dt(2.5), True) == 0
    assert R.indexof([nan[0]], dt(math.inf), True) == 0


@pytest.mark.parametrize("tname", K.NUMBERS)
def test_reduce_is_sum_min_max(tname):
    cls = R.SUM_CLASS[tname]
    for row in all_rows(tname, for_sum=True):
        vals = [e for e in row if e is not None]
        assert R.reduce(R.COUNT, row, tname) == len(vals)
        if not vals:
            assert R.reduce(R.MIN, row, tname) is None and R.reduce(R.MAX, row, tname) is None
            assert cls is None or R.reduce(R.SUM, row, tname) is None
            continue
        if cls == "f":
            c, s, sabs, n = R.reduce(R.SUM, row, tname)
            assert n == len(vals)
            if c == "finite":
                assert s == math.fsum(float(v) for v in vals)
            lo, hi = R.reduce(R.MIN, row, tname), R.reduce(R.MAX, row, tname)
            assert all(F.of_cmp(lo, v) <= 0 <= F.of_cmp(hi, v) for v in vals)
            assert any(F.of_cmp(lo, v) == 0 for v in vals) and any(F.of_cmp(hi, v) == 0 for v in vals)
            continue
        assert R.reduce(R.MIN, row, tname) == min(vals) and R.reduce(R.MAX, row, tname) == max(vals)
        if cls in ("i64", "u64"):
            got = R.reduce(R.SUM, row, tname)
            assert (got - sum(vals)) % (1 << 64) == 0 and (-(1 << 63) <= got < (1 << 63) if cls == "i64" else 0 <= got < (1 << 64))
        elif cls == "dec128":
            got = R.reduce(R.SUM, row, tname)
            assert got == (sum(vals) if abs(sum(vals)) <= R.DEC128_MAX else R.OVERFLOW)


def test_integer_sums_wrap_in_the_case_list():
    wrapped = sum(1 for row in all_rows("i64") if [e for e in row if e is not None] and R.reduce(R.SUM, row, "i64") != sum(e for e in row if e is not None))
    assert wrapped > 5


def test_dec128_overflow_rows():
    got = [R.reduce(R.SUM, row, "dec128") for row in K.dec128_overflow_rows()]
    assert got == [R.OVERFLOW, R.DEC128_MAX, R.OVERFLOW, 5, R.OVERFLOW, R.OVERFLOW, 0, 7]


def test_unnest_sel_is_the_expansion():
    for _, rows in K.columns("i32"):
        for first in (0, 9):
            off = K.offsets_of(rows, first)
            sel = R.unnest_sel(off, off[-1])
            exp = [r for r, row in enumerate(rows) for _ in row]
            assert [sel[k] for k in range(len(exp))] == exp and len(sel) == len(exp)


def test_bad_rows_are_empty():
    off = [0, 3, 2, 5, 40, 6]
    assert R.row_runs(off, 10) == [(0, 3, False), (0, 0, True), (2, 3, False), (0, 0, True), (0, 0, True)]
    assert R.rows_of(off, list(range(10))) == [[0, 1, 2], [], [2, 3, 4], [], []]


# ---- negative controls: each wrong function must differ from the reference somewhere on the case list -------------------------------------
def differs(wrong, right, inputs):
    return any(wrong(*a) != right(*a) for a in inputs)


def test_negative_controls():
    rows = all_rows("i64")
    gets = [(row, i) for row in rows for i in K.get_indexes([row])[0]]
    finds = [(row, x) for _, cols in K.columns("i64") for row, x in zip(cols, K.needles("i64", cols, 5))]
    finds += [(row, K.indexof_lane_rows()[1]) for row in K.indexof_lane_rows()[0]]

    def get_off_by_one(row, i):                 # 0-based where it should be 1-based
        return R.get(row, i + 1) if i >= 0 else R.get(row, i)

    def get_last_is_len(row, i):                # a negative index one too far
        return R.get(row, i - 1) if i < 0 else R.get(row, i)

    def null_matches(row, x):                   # a NULL element takes part in the comparison as the zero value
        return R.indexof([0 if e is None else e for e in row], x)

    def last_match(row, x):                     # a match, but not the first
        hits = [k + 1 for k, e in enumerate(row) if e is not None and x is not None and e == x]
        return hits[-1] if hits else 0

    def empty_is_zero(kind, row, tname):        # SUM of nothing is 0, not NULL
        got = R.reduce(kind, row, tname)
        return 0 if got is None else got

    def sum_counts_nulls(kind, row, tname):     # COUNT of the run, not of its values
        return len(row) if kind == R.COUNT else R.reduce(kind, row, tname)

    assert differs(get_off_by_one, R.get, gets) and differs(get_last_is_len, R.get, gets)
    assert differs(null_matches, R.indexof, finds) and differs(last_match, R.indexof, finds)
    reduces = [(k, row, "i64") for row in rows for k in (R.COUNT, R.SUM, R.MIN, R.MAX)]
    assert differs(empty_is_zero, R.reduce, reduces) and differs(sum_counts_nulls, R.reduce, reduces)
    assert [R.indexof(row, 7) for row in K.indexof_lane_rows()[0]] == K.indexof_lane_rows()[2]
    assert differs(lambda row, x: last_match(row, x), R.indexof, [(row, 7) for row in K.indexof_lane_rows()[0]])


def test_float_min_max_put_nan_last():
    for tname in ("f32", "f64"):
        for row in all_rows(tname):
            vals = [float(e) for e in row if e is not None]
            if not vals:
                continue
            hi, lo = R.reduce(R.MAX, row, tname), R.reduce(R.MIN, row, tname)
            assert math.isnan(hi) == any(v != v for v in vals)
            assert math.isnan(lo) == all(v != v for v in vals)
    assert np.isnan(R.reduce(R.MAX, [np.float32(math.inf), F.NAN32[1]], "f32"))
