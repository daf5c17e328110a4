"""The one case list of the math functions (include/dbhip.h a26), shared by the reference's own test, the host checker and the GPU
tests. Everything is seeded and built once per process."""
import functools

import numpy as np

from tests import math_ref as R

FLOAT_DIGITS = (-31, -30, -3, -1, 0, 1, 2, 15, 22, 23, 30, 31)
DEC64_SIZES = ((1, 0), (1, 1), (9, 2), (18, 0), (18, 4), (18, 18))
DEC128_SIZES = ((19, 2), (30, 25), (38, 0), (38, 10), (38, 38))
DEC_SIZES = DEC64_SIZES + DEC128_SIZES
NUMBER_FNS = (R.ABS, R.SIGN, R.CEIL, R.FLOOR, R.ROUND, R.TRUNCATE, R.SQRT)
DECIMAL_FNS = (R.ABS, R.SIGN, R.CEIL, R.FLOOR, R.ROUND, R.TRUNCATE)


@functools.lru_cache(maxsize=None)
def integers(typ):
    """every value of the 8- and 16-bit types; the extremes, 0, +-1 and 4096 random values of the wider ones"""
    dt = np.dtype(R.NP[typ])
    info = np.iinfo(dt)
    if dt.itemsize <= 2:
        out = np.arange(info.min, info.max + 1, dtype=np.int64).astype(dt)
    else:
        rng = np.random.default_rng(2600 + typ)
        edge = [info.min, info.max, 0, 1] + ([-1, info.min + 1] if info.min < 0 else [info.max - 1])
        out = np.concatenate([np.array(edge, dtype=dt), rng.integers(info.min, info.max, 4096, dtype=dt, endpoint=True)])
    out.setflags(write=False)
    return out


def _f64_specials():
    bits = [0x7FF8000000000000, 0xFFF0000000000001 | 0x000ABCDEF0123456]            # two NaNs with different payloads (the second: sign set)
    named = [0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072009e-308, np.finfo(np.float64).max, -np.finfo(np.float64).max,
             0.5, -0.5, 0.49999999999999994, -0.49999999999999994, 1.5, -1.5, 2.5, -2.5, 2.0**52 + 0.5, 2.0**52 - 0.5, -(2.0**52) + 0.5,
             -(2.0**52) - 0.5, 2.0**53 + 2, 1.005, 2.675, 1e22, 1e23, 1e300, -1e-300, 1.0, -1.0, 4.0, 2.0, 1e15 + 0.5, 0.125, -0.375]
    return np.concatenate([np.array(bits, dtype=np.uint64).view(np.float64), np.array(named, dtype=np.float64)])


@functools.lru_cache(maxsize=None)
def floats(typ):
    """the special values, 65,536 random bit patterns and 65,536 values j / 8 (exact ties at every d <= 0)"""
    rng = np.random.default_rng(2610 + typ)
    ties = rng.integers(-2**20, 2**20, 65536, endpoint=True).astype(np.float64) / 8.0
    if typ == R.T_F64:
        rnd = rng.integers(0, 2**64, 65536, dtype=np.uint64).view(np.float64)
        out = np.concatenate([_f64_specials(), rnd, ties])
    else:
        f32 = np.finfo(np.float32)
        with np.errstate(over="ignore", under="ignore"):
            spec = _f64_specials().astype(np.float32)
        own = np.concatenate([np.array([0x7FC00000, 0xFF800001 | 0x0012345], dtype=np.uint32).view(np.float32),
                              np.array([1e-45, -1e-45, 1.1754942e-38, f32.max, -f32.max, 0.49999997, -0.49999997, 2.0**23 + 0.5, 2.0**23 - 0.5, 2.0**24 + 2],
                                       dtype=np.float32)])
        rnd = rng.integers(0, 2**32, 65536, dtype=np.uint32).view(np.float32)
        out = np.concatenate([spec, own, rnd, ties.astype(np.float32)])
    out.setflags(write=False)
    return out


def numbers(typ):
    return floats(typ) if typ in R.FLOATS else integers(typ)


def number_calls(typ):
    """every (fn, digits) the table defines over the number type"""
    calls = []
    for fn in NUMBER_FNS:
        if R.result(fn, typ)[0] != R.OK:
            continue
        for d in (FLOAT_DIGITS if fn in (R.ROUND, R.TRUNCATE) else (0,)):
            calls.append((fn, d))
    return calls


@functools.lru_cache(maxsize=None)
def decimal_values(p):
    """0, +-1, +-(10^p - 1), +-(10^j/2 - 1, 10^j/2, 10^j/2 + 1, 10^j - 1, 10^j) for every j <= p, 4096 random values below 10^p"""
    vals = [0, 1, -1, 10**p - 1, -(10**p - 1)]
    for j in range(0, p + 1):
        for m in (10**j // 2 - 1, 10**j // 2, 10**j // 2 + 1, 10**j - 1, 10**j):
            if 0 < m <= 10**p:
                vals += [m, -m]
    rng = np.random.default_rng(2620 + p)
    digits = rng.integers(1, p, 4096, endpoint=True)
    for nd, a, b, neg in zip(digits.tolist(), rng.integers(0, 2**62, 4096).tolist(), rng.integers(0, 2**62, 4096).tolist(), rng.integers(0, 2, 4096).tolist()):
        m = ((a << 62) | b) % 10**nd
        vals.append(-m if neg else m)
    return tuple(vals)


def decimal_digits(p, s):
    """-40, s - p - 1, s - p, s - 20, s - 19, -1, 0, 1, s - 1, s, s + 1, 40: those that differ"""
    return tuple(sorted({-40, s - p - 1, s - p, s - 20, s - 19, -1, 0, 1, s - 1, s, s + 1, 40}))


def decimal_calls(p, s):
    calls = []
    for fn in DECIMAL_FNS:
        for d in (decimal_digits(p, s) if fn in (R.ROUND, R.TRUNCATE) else (0,)):
            calls.append((fn, d))
    return calls
