"""CPU: tests/math_ref.py — the statement the host checker and the GPU tests compare with — held to independent authorities on the
shared case list (tests/math_cases.py): the decimal module's quantize for every decimal case, math.ceil / floor / trunc / sqrt and
Decimal(x).quantize(1, ROUND_HALF_UP) for the float cases at digits 0. Three negative controls show that the case list tells a wrong
rounding from the right one: half to even, floor(|x| + 0.5), and 10.0 ** 23 in place of the literal 1e23."""
import decimal
import math
from decimal import Decimal

import numpy as np
import pytest

from tests import math_cases as K
from tests import math_ref as R

CTX = decimal.Context(prec=1300, Emin=-9999, Emax=9999)
MODE = {R.ROUND: decimal.ROUND_HALF_UP, R.TRUNCATE: decimal.ROUND_DOWN, R.CEIL: decimal.ROUND_CEILING, R.FLOOR: decimal.ROUND_FLOOR}


def authority_decimal(fn, v, p, s, digits):
    """the stored integer of the result, from decimal arithmetic on the VALUE v / 10^s"""
    x = Decimal(v).scaleb(-s, context=CTX)
    if fn == R.ABS:
        return int(x.copy_abs().scaleb(s, context=CTX))
    if fn == R.SIGN:
        return int(x.compare(Decimal(0)))
    to = 0 if fn in (R.CEIL, R.FLOOR) else digits
    rs = R.clamp(to, 0, s)
    if to >= s:
        return v
    return int(x.quantize(Decimal(1).scaleb(-to, context=CTX), rounding=MODE[fn], context=CTX).scaleb(rs, context=CTX))


@pytest.mark.parametrize("p,s", K.DEC_SIZES)
def test_decimals_against_the_decimal_module(p, s):
    values = K.decimal_values(p)
    assert len(values) > 4096 + 8 * p
    for fn, digits in K.decimal_calls(p, s):
        got = R.decimal(fn, values, p, s, digits)
        exp = [authority_decimal(fn, v, p, s, digits) for v in values]
        bad = [i for i in range(len(values)) if got[i] != exp[i]]
        assert not bad, (R.NAMES[fn], p, s, digits, values[bad[0]], got[bad[0]], exp[bad[0]])
        assert R.result(fn, R.T_DEC64 if p <= 18 else R.T_DEC128, p, s, digits)[3] == (R.clamp(digits, 0, s) if fn in (R.ROUND, R.TRUNCATE) else
                                                                                     0 if fn in (R.CEIL, R.FLOOR, R.SIGN) else s)


def test_a_decimal_result_may_have_one_more_digit():
    assert R.decimal(R.ROUND, [999, -999, 994], 3, 0, -1) == [1000, -1000, 990]
    assert R.decimal(R.ROUND, [15, -15, 14, -14, 5, 4], 2, 1, 0) == [2, -2, 1, -1, 1, 0]
    assert R.decimal(R.CEIL, [15, -15, 10, -10, 1, -1, 0], 2, 1) == [2, -1, 1, -1, 1, 0, 0]
    assert R.decimal(R.FLOOR, [15, -15, 10, -10, 1, -1, 0], 2, 1) == [1, -2, 1, -1, 0, -1, 0]
    assert R.decimal(R.TRUNCATE, [19, -19], 2, 1, 0) == [1, -1]
    assert R.decimal(R.ABS, [-2**63], 18, 0) == [-2**63]          # wrapping


def finite_f64(typ):
    with np.errstate(invalid="ignore"):          # (a signalling NaN among the Float32 cases)
        x = K.floats(typ).astype(np.float64)
    return x[np.isfinite(x)]


def same_value_and_zero_sign(got, exp, x):
    assert got == exp and math.copysign(1.0, got) == math.copysign(1.0, exp), (x, got, exp)


@pytest.mark.parametrize("typ", R.FLOATS)
def test_floats_at_digits_zero_against_math(typ):
    x = finite_f64(typ)
    c, f, t, q = R.number(R.CEIL, x), R.number(R.FLOOR, x), R.number(R.TRUNCATE, x, 0), R.number(R.SQRT, x)
    for i, v in enumerate(x.tolist()):
        ec, ef, et = float(math.ceil(v)), float(math.floor(v)), float(math.trunc(v))
        # an integer result of zero carries the sign of the source where the source rounds toward it
        if ec == 0.0 and v < 0:
            ec = -0.0
        if et == 0.0 and math.copysign(1.0, v) < 0:
            et = -0.0
        if v == 0.0:
            ec = ef = v
        same_value_and_zero_sign(float(c[i]), ec, v)
        same_value_and_zero_sign(float(f[i]), ef, v)
        same_value_and_zero_sign(float(t[i]), et, v)
        if v >= 0 or v == 0.0:
            same_value_and_zero_sign(float(q[i]), math.sqrt(v), v)
        else:
            assert math.isnan(q[i]), v
    # the values that are not finite pass through
    for fn in (R.CEIL, R.FLOOR, R.ROUND, R.TRUNCATE):
        out = R.number(fn, np.array([np.inf, -np.inf, np.nan]), 0)
        assert out[0] == np.inf and out[1] == -np.inf and np.isnan(out[2])
    out = R.number(R.SQRT, np.array([np.inf, -np.inf, np.nan, -0.0]))
    assert out[0] == np.inf and np.isnan(out[1]) and np.isnan(out[2]) and out[3] == 0 and np.signbit(out[3])


def authority_round(v):
    r = float(Decimal(v).quantize(Decimal(1), rounding=decimal.ROUND_HALF_UP, context=CTX))
    return -0.0 if r == 0.0 and math.copysign(1.0, v) < 0 else r


def round_sample(typ):
    """the special values and every 16th of the rest: the exact decimal expansion of a double is slow"""
    x = finite_f64(typ)
    return np.concatenate([x[:64], x[64::16]])


@pytest.mark.parametrize("typ", R.FLOATS)
def test_float_round_against_the_decimal_module(typ):
    x = round_sample(typ)
    got = R.number(R.ROUND, x, 0)
    for i, v in enumerate(x.tolist()):
        same_value_and_zero_sign(float(got[i]), authority_round(v), v)


def test_integers_go_through_float64_to_nearest_even():
    x = np.array([2**53 + 1, 2**53 + 3, -(2**53) - 1, 2**63 - 1, -2**63], dtype=np.int64)
    assert R.number(R.CEIL, x).tolist() == [float(2**53), float(2**53 + 4), -float(2**53), float(2**63), -float(2**63)]
    u = np.array([2**64 - 1, 2**53 + 1], dtype=np.uint64)
    assert R.number(R.FLOOR, u).tolist() == [float(2**64), float(2**53)]
    assert R.number(R.ABS, np.array([-128, 127, -1, 0], dtype=np.int8)).tolist() == [128, 127, 1, 0]
    assert R.number(R.ABS, np.array([-2**63], dtype=np.int64)).tolist() == [2**63]
    assert R.number(R.SIGN, np.array([np.nan, 0.0, -0.0, -3.5, np.inf])).tolist() == [0, 0, 0, -1, 1]
    a = R.number(R.ABS, np.array([0xFFF0000000000001 | 0xABCDEF0123456], dtype=np.uint64).view(np.float64))
    assert a.view(np.uint64)[0] == 0x7FF0000000000001 | 0xABCDEF0123456          # the payload stays


# ---- negative controls: a wrong rounding is told apart on the case list -------------------------------------------------------------
def test_control_half_to_even_is_rejected():
    x = round_sample(R.T_F64)
    wrong = np.round(x)
    bad = [v for v, w in zip(x.tolist(), wrong.tolist()) if w != authority_round(v)]
    assert len(bad) > 100 and 2.5 in bad and -0.5 in bad


def test_control_floor_of_abs_plus_half_is_rejected():
    x = round_sample(R.T_F64)
    wrong = np.copysign(np.floor(np.abs(x) + 0.5), x)
    bad = [v for v, w in zip(x.tolist(), wrong.tolist()) if w != authority_round(v)]
    assert 0.49999999999999994 in bad and -0.49999999999999994 in bad
    assert 2.0**52 + 0.5 not in bad          # (2^52 + 0.5 is not a double: the case is 2^52, where both agree)
    right = R.number(R.ROUND, x, 0)
    assert not [v for v, w in zip(x.tolist(), right.tolist()) if w != authority_round(v)]


def test_control_a_computed_power_of_ten_is_rejected():
    assert 10.0**23 != R.P[23] and 10.0**22 == R.P[22]
    x = K.floats(R.T_F64)
    with np.errstate(all="ignore"):
        for fn, rnd in ((R.ROUND, R.round_half_away), (R.TRUNCATE, np.trunc)):
            wrong_up = rnd(x * 10.0**23) / 10.0**23
            wrong_down = rnd(x / 10.0**23) * 10.0**23
            assert len(R.same_bits(wrong_up, R.number(fn, x, 23), True)) > 0
            assert len(R.same_bits(wrong_down, R.number(fn, x, -23), True)) > 0
    # and a running product leaves the literal too
    acc, prod = 1.0, []
    for k in range(31):
        prod.append(acc)
        acc *= 10.0
    assert [k for k in range(31) if prod[k] != R.P[k]] and prod[:23] == R.P[:23]
