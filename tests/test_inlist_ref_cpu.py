"""CPU: tests/inlist_ref.py — the reference every IN-list test is held to — against Python's own `in`, numpy.isin, hand-written
known answers, and negative controls: a reference with one rule broken must fail the very check that the intact one passes."""
import random

import numpy as np
import pytest

from databend_amd import _lib as L
from tests import inlist_ref as R

NAN = float("nan")
INF = float("inf")


def known_answers(broken=None):
    """[(what, got, expected)]: the hand-written answers; `broken` evaluates them with one rule of the reference switched off"""
    ev = lambda *a, **k: R.evaluate(*a, broken=broken, **k)
    other_nan = np.frombuffer(np.uint64(0xFFF0000000000123).tobytes(), np.float64)[0]
    return [
        ("NaN IN (NaN)", ev(L.T_F64, [NAN, other_nan, 1.0], None, [NAN]), ([True, True, False], [True, True, True])),
        ("-0.0 IN (0.0)", ev(L.T_F64, [-0.0, 0.0], None, [0.0]), ([True, True], [True, True])),
        ("0.0 IN (-0.0)", ev(L.T_F32, [0.0], None, [-0.0]), ([True], [True])),
        ("1 NOT IN (2, NULL)", ev(L.T_I32, [1], None, [2], has_null=True, negate=True), ([False], [False])),
        ("1 IN (2, NULL)", ev(L.T_I32, [1], None, [2], has_null=True), ([False], [False])),
        ("2 IN (2, NULL)", ev(L.T_I32, [2], None, [2], has_null=True), ([True], [True])),
        ("2 NOT IN (2, NULL)", ev(L.T_I32, [2], None, [2], has_null=True, negate=True), ([False], [True])),
        ("NULL IN (..)", ev(L.T_I32, [2, 2], [False, True], [2]), ([False, True], [False, True])),
        ("NULL NOT IN (..)", ev(L.T_I32, [7, 7], [False, True], [2], negate=True), ([False, True], [False, True])),
        ("IN ()", ev(L.T_I64, [1, 2], [True, False], []), ([False, False], [True, False])),
        ("NOT IN ()", ev(L.T_I64, [1, 2], [True, False], [], negate=True), ([True, False], [True, False])),
        ("IN (NULL)", ev(L.T_I64, [1], None, [], has_null=True), ([False], [False])),
        ("Inf", ev(L.T_F32, [INF, -INF, 3.0], None, [INF]), ([True, False, False], [True, True, True])),
        ("strings", ev(L.T_STRING, [b"", b"a", b"ab", b"a\0"], None, [b"a", b""]), ([True, True, False, False], [True] * 4)),
        ("duplicates", ev(L.T_U8, [5, 6], None, [5, 5, 5]), ([True, False], [True, True])),
    ]


def test_known_answers():
    for what, got, exp in known_answers():
        assert got == exp, what


@pytest.mark.parametrize("broken", R.BROKEN)
def test_a_reference_with_one_rule_broken_fails(broken):
    assert [what for what, got, exp in known_answers(broken) if got != exp], broken


@pytest.mark.parametrize("dtype,np_type", [(L.T_I8, np.int8), (L.T_U16, np.uint16), (L.T_I32, np.int32), (L.T_U64, np.uint64), (L.T_I64, np.int64)])
def test_integers_against_python_in_and_numpy_isin(dtype, np_type):
    rng = random.Random(int(dtype))
    info = np.iinfo(np_type)
    pool = [info.min, info.max, 0, 1] + [rng.randint(info.min, info.max) for _ in range(40)]
    items = [rng.choice(pool) for _ in range(17)]
    rows = [rng.choice(pool) for _ in range(300)]
    valid = [rng.random() < 0.8 for _ in rows]
    for negate in (False, True):
        bits, vals = R.evaluate(dtype, rows, valid, items, negate=negate)
        assert bits == [v and ((x in items) != negate) for x, v in zip(rows, valid)]
        assert vals == valid
        isin = np.isin(np.array(rows, dtype=np_type), np.array(items, dtype=np_type), invert=negate)
        assert bits == list(isin & np.array(valid))
    assert any(bits) and not all(bits)


def test_floats_without_nan_against_numpy_isin():
    rng = random.Random(5)
    pool = [0.5, -0.5, 1e30, -1e-30, INF, -INF, 3.0] + [rng.uniform(-9, 9) for _ in range(20)]
    items = pool[::2]
    rows = [rng.choice(pool) for _ in range(200)]
    bits, _ = R.evaluate(L.T_F64, rows, None, items)
    assert bits == list(np.isin(np.array(rows), np.array(items))) == [x in items for x in rows]


def test_strings_against_python_in():
    pool = [b"", b"a", b"ab", b"abc" * 4, b"abc" * 4 + b"d", b"x" * 40, b"x" * 39 + b"y", "é".encode()]
    items = pool[1::2]
    bits, _ = R.evaluate(L.T_STRING, pool, None, items)
    assert bits == [s in items for s in pool]


def test_restated_hash_spreads_and_slots_are_powers_of_two():
    assert [R.inl_slots(n) for n in (0, 1, 2, 3, 16, 17, 32, 33, 1024)] == [4, 4, 4, 8, 32, 64, 64, 128, 2048]
    homes = [R.home(L.T_I32, i, 64) for i in range(4096)]
    assert len(set(homes)) == 64
    got = R.colliding(L.T_I64, 8, 64, 63, range(1, 1 << 20))
    assert len(set(got)) == 8 and all(R.home(L.T_I64, x, 64) == 63 for x in got)
    assert R.key_image(L.T_I64, -1)[0] == R.EMPTY and R.key_image(L.T_DEC128, -1)[:2] == (R.EMPTY, R.EMPTY)
    assert R.key_image(L.T_STRING, b"abcdefghijklm") == (13 | int.from_bytes(b"abcd", "little") << 32, 0, True)
    assert R.key_image(L.T_F32, -0.0) == R.key_image(L.T_F32, 0.0) and R.key_image(L.T_F64, NAN)[0] == 0x7FF8000000000000
