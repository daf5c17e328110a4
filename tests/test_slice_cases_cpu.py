"""CPU: the bookkeeping of tests/slice_cases.py, with a stub in place of the device module — lengths and offsets of a slice, junk rows
that differ from the payload they lie over, and the bit position in a nullable scalar's Bitmap."""
import types

import numpy as np
import pytest

from tests import slice_cases as S

T_BOOL, T_NUM, T_LIST = 1, 2, 3


class Buf:
    def __init__(self, ptr, arr=None):
        self.ptr, self.arr = ptr, arr

    @classmethod
    def from_numpy(cls, arr):
        return cls(4096, np.array(arr))


class Col:
    """what Column.slice does to n, voff, boff and the data pointer, over host rows"""

    def __init__(self, values, valid, dtype, es):
        self.values, self.valid, self.dtype, self.es = values, valid, dtype, es
        self.n, self.voff, self.boff = len(values), 0, 0
        self.validity = None if valid is None else object()
        self.data = Buf(4096)
        self.is_scalar = False

    def slice(self, lo, hi):
        c = Col(self.values[lo:hi], None if self.valid is None else self.valid[lo:hi], self.dtype, self.es)
        c.validity = self.validity
        c.voff = self.voff + lo
        if self.dtype == T_BOOL:
            c.boff = self.boff + lo
        else:
            c.data = Buf(self.data.ptr + lo * self.es)
        return c

    @classmethod
    def scalar(cls, value, dtype, precision=0, scale=0):
        c = cls([value], None, dtype, 8)
        c.is_scalar = True
        return c


STUB = types.SimpleNamespace(L=types.SimpleNamespace(T_BOOL=T_BOOL), Column=Col, DeviceBuffer=Buf)


def make(values, valid):
    if isinstance(values, np.ndarray) and values.dtype == np.bool_:
        return Col(values, valid, T_BOOL, 0)
    if isinstance(values, np.ndarray):
        return Col(values, valid, T_NUM, values.dtype.itemsize)
    return Col(values, valid, T_LIST, 16)


def payloads(n):
    rng = np.random.default_rng(n)
    return [rng.integers(-100, 100, n).astype(np.int8), rng.integers(0, 2**16, n).astype(np.uint16), rng.standard_normal(n).astype(np.float32),
            rng.integers(-2**62, 2**62, n).astype(np.int64), np.full(n, np.nan), rng.integers(0, 2, n).astype(bool),
            [b"x" * int(k) for k in rng.integers(0, 20, n)], [int(x) << 40 for x in rng.integers(-2**40, 2**40, n)]]


def test_the_offsets_and_sizes_are_the_ones_the_kernels_can_trip_on():
    assert S.LOS == (1, 13, 69) and all(lo % 8 for lo in S.LOS) and 69 > 64
    assert S.SIZES == (1, 63, 257, 4099) and S.TAIL >= 77
    assert all((13 * es) % 16 for es in (1, 2, 4, 8))


@pytest.mark.parametrize("lo", S.LOS)
@pytest.mark.parametrize("n", S.SIZES)
def test_sliced_bookkeeping(lo, n):
    for values in payloads(n):
        valid = np.random.default_rng(lo + n).integers(0, 2, n).astype(bool)
        for v in (valid, None):
            col = S.sliced(STUB, make, values, v, lo)
            assert col.n == n and col.voff == lo
            assert col.boff == (lo if col.dtype == T_BOOL else 0)
            if col.dtype != T_BOOL:
                assert col.data.ptr == 4096 + lo * col.es
            # the slice holds exactly the payload
            assert len(col.values) == n
            if isinstance(values, np.ndarray):
                assert np.array_equal(col.values, values, equal_nan=values.dtype.kind == "f")
            else:
                assert list(col.values) == list(values)
            if v is not None:
                assert np.array_equal(col.valid, v)


@pytest.mark.parametrize("lo", S.LOS)
def test_junk_differs_from_the_payload_it_lies_over(lo):
    n = 257
    for values in payloads(n):
        valid = np.random.default_rng(lo).integers(0, 2, n).astype(bool)
        whole, wv = S.surround(values, valid, lo)
        assert len(whole) == lo + n + S.TAIL and len(wv) == len(whole)
        # a reader that forgets the offset takes whole[i] for payload row i: wrong in every one of the first `lo` rows
        for i in range(lo):
            a, b = whole[i], values[i]
            both_nan = isinstance(b, (float, np.floating)) and np.isnan(a) and np.isnan(b)
            assert a != b and not both_nan
            assert wv[i] != valid[i]
        # and the whole column read from bit 0 is not the payload
        assert not np.array_equal(wv[:n], valid)
        # another seed, other junk; the same seed, the same junk
        again, _ = S.surround(values, valid, lo)
        other, _ = S.surround(values, valid, lo, seed=1)
        same = lambda x, y: np.array_equal(x, y, equal_nan=True) if isinstance(x, np.ndarray) and x.dtype.kind == "f" else list(x) == list(y)
        assert same(whole, again)
        assert not same(whole[lo + n:], other[lo + n:])


def test_a_short_tail_is_refused():
    with pytest.raises(AssertionError):
        S.surround(np.arange(5), None, 13, tail=76)


@pytest.mark.parametrize("voff", [0, 5, 127])
@pytest.mark.parametrize("valid", [True, False])
def test_nullable_scalar_bit_position(voff, valid):
    col = S.nullable_scalar(STUB, 7, T_NUM, valid, voff)
    assert col.is_scalar and col.voff == voff and col.n == 1
    by = col.validity.arr
    assert by.dtype == np.uint8 and len(by) == 16
    bits = np.unpackbits(by, bitorder="little").astype(bool)
    assert bits[voff] == valid
    assert np.all(np.delete(bits, voff) == (not valid))
