"""The math functions of include/dbhip.h group a26, restated in numpy (numbers) and Python ints (decimals). Shares no text with
databend_amd/csrc/dev_math.h. tests/test_math_ref_cpu.py holds this file to the decimal module and to math.ceil / floor / trunc / sqrt.

Numbers go through float64 with numpy's IEEE operations (each correctly rounded). round is half away from zero, built from trunc: with
t = trunc(x) the difference x - t is exact, so |x - t| >= 0.5 decides without the double rounding of floor(|x| + 0.5) (wrong at
0.49999999999999994) and without numpy's half-to-even np.round. P[k] is the float nearest to 10^k: the decimal literal."""
import numpy as np

ABS, SIGN, CEIL, FLOOR, ROUND, TRUNCATE, SQRT = range(7)
NAMES = ["abs", "sign", "ceil", "floor", "round", "truncate", "sqrt"]
P = [float("1e%d" % k) for k in range(31)]

# dbhip_type codes
T_I8, T_I16, T_I32, T_I64, T_U8, T_U16, T_U32, T_U64, T_F32, T_F64 = range(2, 12)
T_BOOL, T_DATE, T_TIMESTAMP, T_DEC64, T_DEC128, T_STRING, T_DEC256 = 1, 12, 13, 14, 15, 16, 17
NP = {T_I8: np.int8, T_I16: np.int16, T_I32: np.int32, T_I64: np.int64, T_U8: np.uint8, T_U16: np.uint16, T_U32: np.uint32,
      T_U64: np.uint64, T_F32: np.float32, T_F64: np.float64}
SIGNED, UNSIGNED, FLOATS = (T_I8, T_I16, T_I32, T_I64), (T_U8, T_U16, T_U32, T_U64), (T_F32, T_F64)
NUMBERS = SIGNED + UNSIGNED + FLOATS
OK, INVALID, UNSUPPORTED = 0, 1, 7


def clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


def result(fn, typ, p=0, s=0, digits=0):
    """-> (status, result type, precision, scale), what dbhip_math_result answers"""
    if fn not in range(7):
        return INVALID, None, 0, 0
    if typ in NUMBERS:
        if fn == ABS:
            if typ in UNSIGNED:
                return INVALID, None, 0, 0
            return OK, (typ + 4 if typ in SIGNED else typ), 0, 0
        return OK, (T_I8 if fn == SIGN else T_F64), 0, 0
    if typ == T_DEC256:
        return UNSUPPORTED, None, 0, 0
    if typ in (T_DEC64, T_DEC128):
        if fn == SQRT:
            return INVALID, None, 0, 0
        if not (1 <= p <= (18 if typ == T_DEC64 else 38) and s <= p):
            return INVALID, None, 0, 0
        if fn == SIGN:
            return OK, T_I8, 0, 0
        if fn in (CEIL, FLOOR):
            return OK, typ, p, 0
        if fn in (ROUND, TRUNCATE):
            return OK, typ, p, clamp(digits, 0, s)
        return OK, typ, p, s
    return INVALID, None, 0, 0


# ---- numbers ----------------------------------------------------------------------------------------------------------------------
def round_half_away(x):
    t = np.trunc(x)
    with np.errstate(invalid="ignore"):
        far = np.abs(x - t) >= 0.5          # (Inf - Inf and NaN compare false: t is the answer)
    return np.where(far, t + np.copysign(1.0, x), t)


def number(fn, values, digits=0):
    """fn over a numpy array of one of the ten number types -> numpy array of the result type"""
    values = np.asarray(values)
    kind = values.dtype.kind
    if fn == ABS:
        if kind == "i":
            u = np.dtype("u%d" % values.dtype.itemsize)
            w = values.astype(u)            # two's complement bits
            return np.where(values < 0, (np.zeros(1, u) - w).astype(u), w).astype(u)
        assert kind == "f"
        bits = values.view("u%d" % values.dtype.itemsize)
        return (bits & bits.dtype.type((1 << (8 * values.dtype.itemsize - 1)) - 1)).view(values.dtype)
    if fn == SIGN:
        return ((values > 0).astype(np.int8) - (values < 0).astype(np.int8)).astype(np.int8)
    with np.errstate(all="ignore"):
        x = values.astype(np.float64)
        if fn == CEIL:
            return np.ceil(x)
        if fn == FLOOR:
            return np.floor(x)
        if fn == SQRT:
            return np.sqrt(x)
        assert fn in (ROUND, TRUNCATE)
        rnd = round_half_away if fn == ROUND else np.trunc
        d = clamp(digits, -30, 30)
        if d == 0:
            return rnd(x)
        if d > 0:
            return rnd(x * P[d]) / P[d]
        return rnd(x / P[-d]) * P[-d]


def same_bits(got, exp, nan_any):
    """indices where got and exp differ bit for bit; nan_any: a NaN matches any NaN (every function but ABS)"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    if got.dtype.kind == "f":
        u = "u%d" % got.dtype.itemsize
        bad = got.view(u) != exp.view(u)
        if nan_any:
            bad &= ~(np.isnan(got) & np.isnan(exp))
    else:
        bad = got != exp
    return np.nonzero(bad)[0]


# ---- decimals: Python ints ----------------------------------------------------------------------------------------------------------
def tdiv(a, b):
    """a / b truncated toward zero, b > 0"""
    q = abs(a) // b
    return -q if a < 0 else q


def wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def decimal_one(fn, v, p, s, digits=0):
    if fn == ABS:
        return -v if v < 0 else v
    if fn == SIGN:
        return (v > 0) - (v < 0)
    if fn == CEIL:
        return tdiv(v + 10**s - 1, 10**s) if v > 0 else tdiv(v, 10**s)
    if fn == FLOOR:
        return tdiv(v - 10**s + 1, 10**s) if v < 0 else tdiv(v, 10**s)
    assert fn in (ROUND, TRUNCATE)
    k = s - digits
    if k <= 0:
        return v
    if k > p:
        return 0
    h = 10**k // 2 if fn == ROUND else 0
    q = (abs(v) + h) // 10**k
    if digits < 0:
        q *= 10 ** (-digits)
    return -q if v < 0 else q


def decimal(fn, values, p, s, digits=0, bits=None):
    """fn over a list of stored integers -> list of stored integers (SIGN: -1, 0, 1), wrapped to the storage"""
    bits = bits or (64 if p <= 18 else 128)
    if fn == SIGN:
        return [decimal_one(fn, int(v), p, s) for v in values]
    return [wrap(decimal_one(fn, int(v), p, s, digits), bits) for v in values]
