"""The shared case list of the conditionals (include/dbhip.h a27), for the host checker's test and the GPU test: conditions, branch
values and Kleene operands as tests/cond_ref.py's Col (unpacked bits, raw element bytes), built so that a wrong kernel shows:

  * NULL conditions whose payload bit is 1 (a chooser that ignores the validity takes the branch);
  * NULL values with non-zero payloads, non-empty views among them (the result must hold zero there);
  * rows where several conditions are TRUE (the first wins) and rows where none is;
  * branch patterns that are constant over a 64-row word (whole waves choose one branch) and ones that change every row.

Everything is seeded; nothing here touches a device."""
import numpy as np

from tests import cond_ref as R

N = 1000                                                     # the case list's rows: fifteen whole Bitmap words and a partial one
BOUNDARY_SIZES = (0, 1, 63, 64, 65, 255, 4095, 4096, 4097, 600001)
FETCH_OFFSETS = (0, 1, 63, 64, 69)                           # bit offsets of the bit fetch
COND_COUNTS = (1, 2, 3, 16)


def _rng(*key):
    return np.random.default_rng([0xC0D1] + [int(k) for k in key])


def _runs(n, rng, density, run=64):
    """bits that are constant over runs of `run` rows"""
    return np.repeat(rng.random(n // run + 1) < density, run)[:n]


def conditions(n, k, seed=0):
    """k conditions over n rows. Even ones are constant over 64-row words, odd ones change row by row. One in three cannot be NULL; the
    NULL rows of the others carry the payload bit 1 (all of them where j % 3 == 1, a random half where j % 3 == 2)."""
    out = []
    density = 1.0 / (k + 1)
    for j in range(k):
        rng = _rng(seed, n, k, j, 1)
        bits = _runs(n, rng, max(density, 0.25)) if j % 2 == 0 else rng.random(n) < density
        valid = None
        if j % 3 == 1:
            valid = rng.random(n) < 0.75
            bits = bits | ~valid
        elif j % 3 == 2:
            valid = _runs(n, rng, 0.7)
            bits = bits | (~valid & (rng.random(n) < 0.5))
        out.append(R.Col(bits, valid))
    return out


def validity(n, j, seed=0):
    """the validity of value / argument j: row by row, none, constant over words"""
    rng = _rng(seed, n, j, 2)
    if j % 3 == 0:
        return rng.random(n) < 0.6
    if j % 3 == 1:
        return None
    return _runs(n, rng, 0.5)


def raw_values(size, n, j, seed=0):
    """n elements of `size` bytes as (n, size) uint8, no byte zero: a NULL row's payload is never the zero the result must hold"""
    return _rng(seed, n, j, size, 3).integers(1, 256, (n, size), dtype=np.uint8)


def values(size, n, k, seed=0, last_valid=True):
    """k branch columns of raw elements; column j's validity is validity(n, j); last_valid: the last one (ELSE) cannot be NULL"""
    cols = [R.Col(raw_values(size, n, j, seed), validity(n, j, seed)) for j in range(k)]
    if last_valid:
        cols[-1].valid = None
    return cols


def arguments(size, n, k, seed=0):
    """k coalesce arguments of raw elements, every one nullable (row by row, or constant over words), sparse enough that some rows
    reach every argument and some stay NULL"""
    cols = []
    density = min(0.4, 2.0 / k)
    for j in range(k):
        rng = _rng(seed, n, j, 7)
        valid = rng.random(n) < density if j % 2 == 0 else _runs(n, rng, density)
        cols.append(R.Col(raw_values(size, n, j, seed), valid))
    return cols


def bool_values(n, k, seed=0):
    cols = []
    for j in range(k):
        rng = _rng(seed, n, j, 4)
        valid = validity(n, j, seed)
        bits = rng.random(n) < 0.5
        if valid is not None:
            bits = bits | (~valid & (rng.random(n) < 0.7))   # NULL rows with the payload bit set
        cols.append(R.Col(bits, valid))
    return cols


def strings(n, j, seed=0):
    """n values as bytes: empty, inline (up to 12 bytes) and long ones"""
    rng = _rng(seed, n, j, 5)
    lens = rng.choice([0, 1, 4, 11, 12, 13, 20, 40], n)
    return [bytes(rng.integers(97, 123, int(ln)).astype(np.uint8)) for ln in lens]


def kleene_operands(n, seed=0):
    """the nine forms of an operand: name -> Col. Columns hold every (payload bit, validity bit) pair; NULL scalars come with both
    payload bits."""
    rng = _rng(seed, n, 6)
    one, zero = np.array([True]), np.array([False])
    return {
        "nullable": R.Col(rng.random(n) < 0.5, rng.random(n) < 0.6),
        "plain": R.Col(rng.random(n) < 0.5, None),
        "words": R.Col(_runs(n, rng, 0.5), _runs(n, rng, 0.5)),
        "true": R.Col(one, None, True),
        "false": R.Col(zero, None, True),
        "null1": R.Col(one, zero, True),
        "null0": R.Col(zero, zero, True),
        "valid_true": R.Col(one, one, True),
        "valid_false": R.Col(zero, one, True),
    }
