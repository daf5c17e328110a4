"""Sliced columns and nullable scalars for the tests of the dbhip_col entry points (tests/test_gpu_slices.py).

A block that went through LIMIT, block splitting or Column::slice reaches the library as a VIEW: value buffers by address (aligned to
the element only), Bitmaps by bit offset. `sliced` builds such a view whose surroundings differ from the payload, so that a kernel
that reads bit `row` where it should read bit `validity_offset + row`, or a wrapper that drops the offset, gives another answer.

Plain Python: the device module is whatever the caller passes (tests/test_slice_cases_cpu.py passes a stub)."""
import numpy as np

LOS = (1, 13, 69)                 # no multiple of 8; 69 crosses a 64-bit word; 13 rows of 1, 2, 4, 8 bytes miss 16-byte alignment
SIZES = (1, 63, 257, 4099)        # the 4-row quad tail, the 64-lane wave, the 256-row chunk, more than one block
TAIL = 77                         # junk rows behind the payload, at least


def _junk_values(values, k, rng):
    """k junk rows of the kind of `values`: random, from the generator of another seed"""
    if isinstance(values, np.ndarray):
        if values.dtype == np.bool_:
            return rng.integers(0, 2, k).astype(bool)
        if values.dtype.kind in "iu":
            info = np.iinfo(values.dtype)
            return rng.integers(info.min, info.max, k, dtype=values.dtype, endpoint=True)
        return (rng.standard_normal(k) * 1e6).astype(values.dtype)
    if len(values) and isinstance(values[0], (bytes, bytearray)):
        return [bytes(rng.integers(33, 127, int(ln)).astype(np.uint8)) for ln in rng.integers(0, 24, k)]
    top = max([abs(int(v)) for v in values] + [1000])
    return [int(x) % (top + 1) * (1 if s else -1) for x, s in zip(rng.integers(0, 2**62, k), rng.integers(0, 2, k))]


def _differs(a, b):
    if isinstance(a, (float, np.floating)) and isinstance(b, (float, np.floating)) and np.isnan(a) and np.isnan(b):
        return False
    return a != b


def _other(v, rng):
    """a value of v's kind that is not v"""
    if isinstance(v, (bool, np.bool_)):
        return not v
    if isinstance(v, (bytes, bytearray)):
        return bytes(v) + b"#"
    if isinstance(v, np.floating):
        return type(v)(1.0) if (np.isnan(v) or v != 1.0) else type(v)(2.0)
    if isinstance(v, np.integer):
        return type(v)(int(v) ^ 1)
    return int(v) ^ 1


def surround(values, valid, lo, tail=TAIL, seed=0):
    """-> (whole values, whole validity | None): junk head of `lo` rows + values + junk tail of `tail` rows. Where row i of the head
    lies over payload row i (what a reader that forgets the offset would take for it), value and validity bit both differ."""
    assert tail >= TAIL
    n = len(values)
    rng = np.random.default_rng(0x51CE + 1000 * lo + seed)
    head, back = _junk_values(values, lo, rng), _junk_values(values, tail, rng)
    hv, bv = rng.integers(0, 2, lo).astype(bool), rng.integers(0, 2, tail).astype(bool)
    for i in range(min(lo, n)):
        if not _differs(head[i], values[i]):
            head[i] = _other(values[i], rng)
        if valid is not None:
            hv[i] = not valid[i]
    if isinstance(values, np.ndarray):
        whole = np.concatenate([head, values, back]).astype(values.dtype)
    else:
        whole = list(head) + list(values) + list(back)
    wv = np.concatenate([hv, np.asarray(valid, dtype=bool), bv]) if valid is not None else None
    return whole, wv


def sliced(gpu, make_col, values, valid, lo, tail=TAIL, seed=0):
    """rows [lo, lo + n) of make_col(junk_head + values + junk_tail, validity the same way) as a view. gpu: the device module (its
    T_BOOL names the Boolean type)."""
    n = len(values)
    whole_values, whole_valid = surround(values, valid, lo, tail, seed)
    whole = make_col(whole_values, whole_valid)
    assert whole.n == lo + n + tail
    col = whole.slice(lo, lo + n)
    assert col.n == n and col.voff == lo and (col.validity is None) == (valid is None)
    if col.dtype == gpu.L.T_BOOL:
        assert col.boff == lo
    elif isinstance(values, np.ndarray) and values.dtype.itemsize in (1, 2, 4, 8):
        assert col.data.ptr == whole.data.ptr + lo * values.dtype.itemsize
        if lo == 13:
            assert col.data.ptr % 16 != 0, "the slice was meant to miss 16-byte alignment"
    return col


SCALAR_BITMAP_BITS = 128          # 16 bytes, the smallest device allocation


def scalar_bitmap(valid, voff=0):
    """the Bitmap of a nullable scalar: bit `voff` is `valid`, every other bit the opposite"""
    assert 0 <= voff < SCALAR_BITMAP_BITS
    bits = np.full(SCALAR_BITMAP_BITS, not valid, dtype=bool)
    bits[voff] = bool(valid)
    return np.packbits(bits, bitorder="little")


def nullable_scalar(gpu, value, dtype, valid, voff=0, precision=0, scale=0):
    """Column.scalar with a validity Bitmap whose bit `voff` says `valid`; all other bits say the opposite, so a reader that looks at
    bit voff + row takes every row but the first for the wrong thing"""
    col = gpu.Column.scalar(value, dtype, precision, scale)
    col.validity = gpu.DeviceBuffer.from_numpy(scalar_bitmap(valid, voff))
    col.voff = voff
    return col
