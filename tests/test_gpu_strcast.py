"""GPU: dbhip_str_parse / dbhip_str_format_bytes / dbhip_str_format (include/dbhip.h a24), every row asserted exactly against
tests/strcast_ref.py (plain Python, held to Python's own operations and to negative controls by tests/test_strcast_ref_cpu.py): the
values, every bitmap word with the bits past n, the counters, the full 16 bytes of every result view and every byte of out_data.
Nothing is sampled. String columns are packed by tests/test_gpu_strfn.py's helper: the long values lie back to back in their data
buffers without padding, behind a lead of 0 to 3 bytes, so every alignment occurs and a kernel that reads outside a value reads its
neighbours' bytes. Every output is pre-filled with 0xFF and has guard bytes behind it that must stay 0xFF."""
import ctypes as C
import random

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import strcast_cases as K
from tests import strcast_ref as R
from tests.test_gpu_strfn import dirty, guarded, pack, read_guarded

pytestmark = pytest.mark.gpu

SIZE = {T.T_I8: 1, T.T_U8: 1, T.T_I16: 2, T.T_U16: 2, T.T_I32: 4, T.T_U32: 4, T.T_DATE: 4, T.T_I64: 8, T.T_U64: 8, T.T_TIMESTAMP: 8, T.T_DEC64: 8, T.T_DEC128: 16}
ROW_COUNTS = (1, 63, 64, 65, 257, 4099)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def run_parse(gpu, col, sp, is_try, n=None, bitmap=True, counters=True):
    """-> (out bytes [n * size], bitmap words (or None), error count, declined count)"""
    n = col.n if n is None else n
    size = SIZE[sp["dtype"]]
    words = (n + 63) // 64
    out = guarded(gpu, n * size)
    bm = guarded(gpu, words * 8) if bitmap else None
    cnt = gpu.DeviceBuffer(16).zero()
    cc = col.c()
    T.check(T.lib().dbhip_str_parse(C.byref(cc), C.c_int32(sp["dtype"]), C.c_uint8(sp["precision"]), C.c_uint8(sp["scale"]), C.c_int32(int(is_try)),
                                    C.c_int32(int(sp["rounding"])), C.c_int32(sp["offset_s"]), C.c_int64(n), C.c_void_p(out.ptr), C.c_void_p(bm.ptr) if bm else None,
                                    C.c_void_p(cnt.ptr) if counters else None, C.c_void_p(cnt.ptr + 8) if counters else None, None))
    raw = read_guarded(out, n * size, "out")
    bits = read_guarded(bm, words * 8, "bitmap").view(np.uint64).tolist() if bm else None
    errs, declined = (int(x) for x in cnt.to_numpy(np.uint64, 2))
    return raw.tobytes(), bits, errs, declined


def expect_parse(values, valid, sp, is_try, usable=None):
    """what dbhip_str_parse leaves for these rows (valid: None or bools; usable[i] False: a long view that points nowhere = the empty value)"""
    n = len(values)
    size = SIZE[sp["dtype"]]
    raw, errs, declined = b"", 0, 0
    words = [0 if is_try else 2**64 - 1] * ((n + 63) // 64)
    for i, v in enumerate(values):
        ok = valid is None or bool(valid[i])
        st, x = R.parse(v if usable is None or usable[i] else b"", **sp) if ok else (R.OK, 0)
        raw += (x & (256**size - 1)).to_bytes(size, "little")
        errs += st == R.ERROR and not is_try
        declined += st == R.DECLINED
        if is_try and ok and st != R.ERROR:
            words[i // 64] |= 1 << (i % 64)
        if not is_try and st == R.ERROR:
            words[i // 64] &= ~(1 << (i % 64))
    return raw, words, int(errs), int(declined)


def check_parse(gpu, values, sp, valid=None, voff=0, lead=b"", n=None, what=""):
    """both modes of one column against the reference; `voff`: the validity bitmap starts at that bit"""
    col = dirty(gpu, pack(gpu, values, lead=lead))
    if valid is not None:
        col.validity = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(np.concatenate([np.zeros(voff, dtype=bool), np.asarray(valid, dtype=bool)])))
        col.voff = voff
    n = len(values) if n is None else n
    for is_try in (False, True):
        got = run_parse(gpu, col, sp, is_try, n)
        exp = expect_parse(values[:n], None if valid is None else valid[:n], sp, is_try)
        if got != exp:
            size = SIZE[sp["dtype"]]
            rows = [i for i in range(n) if got[0][i * size:(i + 1) * size] != exp[0][i * size:(i + 1) * size]]
            assert False, (what, is_try, "rows", [(i, values[i][:50]) for i in rows[:5]], "bitmap", got[1] == exp[1], "counters", got[2:], exp[2:])


def some_nulls(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n) < 0.8


def tiled(values, n):
    return [values[i % len(values)] for i in range(n)]


def number_column(gpu, numbers, sp, valid=None):
    dt = sp["dtype"]
    if dt in (T.T_DEC64, T.T_DEC128):
        return gpu.Column.decimal([int(v) for v in numbers], sp["precision"], sp["scale"], validity=valid)
    arr = np.array([int(v) & (256**SIZE[dt] - 1) for v in numbers], dtype=np.dtype("u%d" % SIZE[dt])).view(gpu.NP_OF[dt])
    return gpu.Column.from_numpy(arr, dtype=dt, validity=valid)


def run_format(gpu, col, offset_s, n=None, short_by=0):
    """-> (views [bytes], out_data bytes, error count, the bytes dbhip_str_format_bytes reported)"""
    n = col.n if n is None else n
    cc = col.c()
    nbytes = C.c_uint64(2**64 - 1)
    T.check(T.lib().dbhip_str_format_bytes(C.byref(cc), C.c_int32(offset_s), C.c_int64(n), C.byref(nbytes), None))
    total = nbytes.value
    views = guarded(gpu, n * 16)
    data = guarded(gpu, total - short_by)          # the canary starts where out_data_bytes ends
    cnt = gpu.DeviceBuffer(8).zero()
    T.check(T.lib().dbhip_str_format(C.byref(cc), C.c_int32(offset_s), C.c_int64(n), C.c_void_p(views.ptr), C.c_void_p(data.ptr), C.c_uint64(total - short_by),
                                     C.c_void_p(cnt.ptr), None))
    v = [bytes(r) for r in read_guarded(views, n * 16, "out_views").reshape(-1, 16)]
    return v, read_guarded(data, total - short_by, "out_data").tobytes(), int(cnt.to_numpy(np.uint64, 1)[0]), total


def check_format(gpu, numbers, sp, valid=None, n=None, what=""):
    col = number_column(gpu, numbers, sp, valid)
    n = len(numbers) if n is None else n
    ok = [True] * n if valid is None else [bool(x) for x in valid[:n]]
    views, data, errs, total = run_format(gpu, col, sp["offset_s"], n)
    eviews, edata, eerrs = R.format_column(numbers[:n], ok, sp["dtype"], sp["scale"], sp["offset_s"])
    assert total == len(edata), (what, total, len(edata))
    bad = [i for i in range(n) if views[i] != eviews[i]]
    assert not bad, (what, [(i, numbers[i], views[i].hex(), eviews[i].hex()) for i in bad[:5]])
    assert data == edata and errs == eerrs, (what, errs, eerrs)


# ---- parse --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def groups():
    K.check_coverage()
    return K.parse_groups()


@pytest.mark.parametrize("kind", ["int", "decimal", "date", "timestamp"])
def test_parse_case_list(gpu, groups, kind):
    """the whole case list, every target: not nullable / nullable at bit offsets 0 and 3, and the four alignments of the data buffer"""
    k = 0
    for name, sp, values in groups:
        if not name.startswith(kind):
            continue
        k += 1
        check_parse(gpu, values, sp, lead=b"x" * (k % 4), what=name)
        check_parse(gpu, values, sp, valid=some_nulls(len(values), k), voff=(0, 3)[k % 2], lead=b"x" * ((k + 1) % 4), what=name + " nullable")
    assert k


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_parse_row_counts(gpu, groups, n):
    """word and wave edges: the bits past n, the last partial word, more than one block"""
    for name in ("int 4", "decimal(38,10) rounding", "timestamp +19800", "date"):
        sp, values = next((s, v) for g, s, v in groups if g == name)
        vals = tiled(values[::3], n)
        check_parse(gpu, vals, sp, what=(name, n))
        check_parse(gpu, vals, sp, valid=some_nulls(n, n), voff=3, lead=b"xyz", what=(name, n, "nullable"))


def test_parse_alignments_and_prefix(gpu, groups):
    """every value at each of the four byte alignments; n smaller than the column (the rows behind n are not touched)"""
    sp, values = next((s, v) for g, s, v in groups if g == "int 5")
    for lead in (b"", b"1", b"12", b"123"):
        check_parse(gpu, values, sp, lead=lead, what=("lead", lead))
    check_parse(gpu, values, sp, n=70, what="prefix")


def test_parse_scalar_and_broken_views(gpu):
    sp = K.spec(T.T_I32)
    for value, valid in ((b"  -12345678901234 ", None), (b" 0000000000000042\t", None), (b"1.5", None), (b"7", [False]), (b"", None)):
        col = pack(gpu, [value], valid=valid)
        col.is_scalar = True
        for is_try in (False, True):
            got = run_parse(gpu, col, sp, is_try, 65)
            assert got == expect_parse([value] * 65, None if valid is None else valid * 65, sp, is_try), (value, is_try)
    # long views that name a buffer the column does not have, or an entry that is NULL: the empty value, never dereferenced
    values = [b"%020d" % k for k in range(130)] + [b"7", b""]
    col = pack(gpu, values, n_buffers=1, buffer_of=lambda i: 1 if i % 3 == 0 else 0)
    usable = [len(v) <= 12 or i % 3 != 0 for i, v in enumerate(values)]
    for is_try in (False, True):
        assert run_parse(gpu, col, K.spec(T.T_U64), is_try) == expect_parse(values, None, K.spec(T.T_U64), is_try, usable)
    col = pack(gpu, values, n_buffers=2, buffer_of=lambda i: i % 2)
    col.buffers = gpu.DeviceBuffer.from_numpy(np.array([col._keep[0].ptr, 0], dtype=np.uint64))
    usable = [len(v) <= 12 or i % 2 == 0 for i, v in enumerate(values)]
    assert run_parse(gpu, col, K.spec(T.T_U64), True) == expect_parse(values, None, K.spec(T.T_U64), True, usable)
    col.buffers, col.n_buffers = None, 0
    assert run_parse(gpu, col, K.spec(T.T_U64), False) == expect_parse(values, None, K.spec(T.T_U64), False, [len(v) <= 12 for v in values])


def test_parse_optional_outputs(gpu, groups):
    """a cast without the bitmap and without the counters computes the same values"""
    sp, values = next((s, v) for g, s, v in groups if g == "decimal(15,2)")
    col = pack(gpu, values)
    full = run_parse(gpu, col, sp, False)
    assert run_parse(gpu, col, sp, False, bitmap=False)[0] == full[0]
    assert run_parse(gpu, col, sp, False, counters=False)[:2] == full[:2]


# ---- format -------------------------------------------------------------------------------------------------------------------------
def test_format_case_list(gpu):
    for k, (name, sp, numbers) in enumerate(K.format_groups()):
        check_format(gpu, numbers, sp, what=name)
        valid = some_nulls(len(numbers), k)
        col = number_column(gpu, numbers, sp)
        col.validity = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(np.concatenate([np.zeros(k % 2 * 3, dtype=bool), valid])))
        col.voff = k % 2 * 3
        views, data, errs, total = run_format(gpu, col, sp["offset_s"])
        eviews, edata, eerrs = R.format_column(numbers, valid, sp["dtype"], sp["scale"], sp["offset_s"])
        assert (views, data, errs, total) == (eviews, edata, eerrs, len(edata)), name


def mixed_numbers(sp, n, seed):
    """numbers of every length the type prints, shuffled: inline and long results alternate inside every wave"""
    rng = random.Random(seed)
    lo, hi = R.INT_RANGE.get(sp["dtype"], (-(10 ** sp["precision"]) + 1, 10 ** sp["precision"] - 1) if sp["precision"] else (R.TS_MIN, R.TS_MAX))
    out = []
    for _ in range(n):
        v = rng.randint(0, 10 ** rng.randint(0, 39)) * rng.choice((1, -1))
        out.append(min(max(v, lo), hi))
    return out


@pytest.mark.parametrize("n", ROW_COUNTS + (70000,))
def test_format_row_counts(gpu, n):
    """wave and block edges of the staging area, and at 70,000 rows more than one tile of the scan"""
    specs = [K.spec(T.T_I64), K.spec(T.T_DEC128, 38, 10), K.spec(T.T_TIMESTAMP, offset_s=19800), K.spec(T.T_U8)] if n != 70000 else [K.spec(T.T_DEC128, 38, 37)]
    for sp in specs:
        numbers = mixed_numbers(sp, n, n)
        check_format(gpu, numbers, sp, what=(sp["dtype"], n))
        if n != 70000:
            check_format(gpu, numbers, sp, valid=some_nulls(n, n + 1), what=(sp["dtype"], n, "nullable"))


def test_format_scalar_and_sliced_sources(gpu):
    for sp, v in ((K.spec(T.T_I64), -2**63), (K.spec(T.T_DEC128, 38, 38), -(10**38 - 1)), (K.spec(T.T_DATE), 19782), (K.spec(T.T_TIMESTAMP, offset_s=-3600), 1)):
        col = number_column(gpu, [v], sp)
        col.is_scalar = True
        views, data, errs, total = run_format(gpu, col, sp["offset_s"], 130)
        assert (views, data, errs) == R.format_column([v] * 130, [True] * 130, sp["dtype"], sp["scale"], sp["offset_s"]) and total == len(data)
    # a sliced column: the data base is element-aligned only, the validity starts at a bit offset
    for sp in (K.spec(T.T_I64), K.spec(T.T_I16), K.spec(T.T_I32), K.spec(T.T_DEC128, 20, 3), K.spec(T.T_DEC64, 18, 4)):
        numbers = mixed_numbers(sp, 300, 9)
        valid = some_nulls(300, 10)
        col = number_column(gpu, numbers, sp, valid).slice(1, 300)
        if sp["dtype"] != T.T_DEC128:
            assert col.data.ptr % 16
        views, data, errs, total = run_format(gpu, col, 0)
        assert (views, data, errs) == R.format_column(numbers[1:], valid[1:], sp["dtype"], sp["scale"], 0) and total == len(data)


def test_format_buffer_one_byte_short(gpu):
    """out_data_bytes one short: only the last long row is empty and counted, and the byte behind the buffer is intact"""
    for sp in (K.spec(T.T_I64), K.spec(T.T_DEC128, 38, 10), K.spec(T.T_TIMESTAMP)):
        numbers = mixed_numbers(sp, 257, 3) + [5]                   # (the last long row is not the last row)
        col = number_column(gpu, numbers, sp)
        views, data, errs, total = run_format(gpu, col, 0, short_by=1)
        eviews, edata, eerrs = R.format_column(numbers, [True] * len(numbers), sp["dtype"], sp["scale"], 0, capacity=total - 1)
        assert eerrs == 1 and len(edata) < total - 1 and sum(v == bytes(16) for v in eviews) == 1
        assert views == eviews and errs == 1
        assert data[:len(edata)] == edata and set(data[len(edata):]) == {0xFF}      # what the dropped row would have filled is untouched


# ---- both ways ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["int", "decimal", "date", "timestamp"])
def test_round_trip(gpu, name):
    """parse(format(x)) == x through the Python interface, on the extremes plus 4,099 seeded random values per type"""
    rng = random.Random(11)
    for gname, sp, numbers in K.format_groups():
        if not gname.startswith(name) or (name == "timestamp" and sp["offset_s"] not in (0, 19800)):
            continue
        lo, hi = R.INT_RANGE.get(sp["dtype"], (None, None))
        if sp["precision"]:
            lo, hi = -(10 ** sp["precision"]) + 1, 10 ** sp["precision"] - 1
        elif sp["dtype"] == T.T_DATE:
            lo, hi = R.DATE_MIN, R.DATE_MAX
        elif sp["dtype"] == T.T_TIMESTAMP:
            lo, hi = R.TS_MIN + 64800 * 10**6, R.TS_MAX - 64800 * 10**6
        vals = [v for v in numbers if lo <= v <= hi] + [lo, hi] + [rng.randint(lo, hi) for _ in range(4099)]
        col = number_column(gpu, vals, sp)
        text = gpu.to_string(col, offset_s=sp["offset_s"])
        assert int(text.str_counters.to_numpy(np.uint64, 1)[0]) == 0
        assert text.string_values() == [R.text(v, sp["dtype"], sp["scale"], sp["offset_s"]) for v in vals], gname
        back, declined = gpu.parse_strings(text, sp["dtype"], sp["precision"], sp["scale"], offset_s=sp["offset_s"])
        assert declined == 0 and (back.dtype, back.precision, back.scale) == (sp["dtype"], sp["precision"], sp["scale"])
        assert [int(x) for x in back.to_numpy()] == vals, gname


def test_python_interface_errors_and_try(gpu):
    col = gpu.Column.strings([b"12", b"x", b"1.5", b" 300 ", b"7"], validity=[True, True, True, True, False])
    with pytest.raises(T.DbhipError) as e:
        gpu.parse_strings(col, T.T_U8)
    assert e.value.code == T.ERR_ROW_ERRORS
    errors = gpu.RowErrors(5)
    res, declined = gpu.parse_strings(col, T.T_U8, errors=errors)
    assert declined == 1 and errors.num_errors() == 2 and errors.error_rows().tolist() == [1, 3] and res.to_numpy().tolist() == [12, 0, 0, 0, 0]
    assert res.validity_numpy().tolist() == [True, True, True, True, False]
    res, declined = gpu.parse_strings(col, T.T_U8, is_try=True)
    assert declined == 1 and res.validity_numpy().tolist() == [True, False, True, False, False]
    res, declined = gpu.parse_strings(col, T.T_DEC64, 5, 2, is_try=True, rounding_mode=True)
    assert declined == 0 and res.to_numpy().tolist() == [1200, 0, 150, 30000, 0] and res.validity_numpy().tolist() == [True, False, True, True, False]
    assert (res.dtype, res.precision, res.scale) == (T.T_DEC64, 5, 2)
    assert gpu.concat(gpu.to_string(gpu.Column.from_numpy(np.array([-5, 1234567890123], dtype=np.int64))), "-", gpu.Column.strings([b"a", b"b"])).string_values() == \
        [b"-5-a", b"1234567890123-b"]


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def test_argument_checks(gpu):
    L = T.lib()
    strings = pack(gpu, [b"1", b"2", b"3"])
    numbers = gpu.Column.from_numpy(np.array([1, 2, 3], dtype=np.int64))
    out = guarded(gpu, 64)
    bm = guarded(gpu, 8)
    cnt = gpu.DeviceBuffer(16).zero()

    def parse(col, dst, p=0, s=0, is_try=0, off=0, n=3, bitmap=True, o=out):
        cc = col.c()
        return L.dbhip_str_parse(C.byref(cc), C.c_int32(dst), C.c_uint8(p), C.c_uint8(s), C.c_int32(is_try), C.c_int32(0), C.c_int32(off), C.c_int64(n),
                                 C.c_void_p(o.ptr) if o else None, C.c_void_p(bm.ptr) if bitmap else None, C.c_void_p(cnt.ptr), C.c_void_p(cnt.ptr + 8), None)

    assert parse(numbers, T.T_I32) == T.ERR_INVALID                                   # the source is not a String column
    for dst in (T.T_F32, T.T_F64, T.T_BOOL, T.T_DEC256, T.T_STRING):
        assert parse(strings, dst) == T.ERR_UNSUPPORTED
    assert parse(strings, T.T_DEC64, 19, 0) == T.ERR_INVALID and parse(strings, T.T_DEC128, 18, 0) == T.ERR_INVALID     # the class of the precision
    assert parse(strings, T.T_DEC128, 39, 0) == T.ERR_INVALID and parse(strings, T.T_DEC64, 5, 6) == T.ERR_INVALID and parse(strings, T.T_DEC64, 0, 0) == T.ERR_INVALID
    assert parse(strings, T.T_I32, is_try=1, bitmap=False) == T.ERR_INVALID
    assert parse(strings, T.T_TIMESTAMP, off=64801) == T.ERR_INVALID and parse(strings, T.T_TIMESTAMP, off=-64801) == T.ERR_INVALID
    assert parse(strings, T.T_I32, n=-1) == T.ERR_INVALID and parse(strings, T.T_I32, n=2**32 - 1) == T.ERR_INVALID
    assert parse(strings, T.T_I32, o=None) == T.ERR_INVALID
    assert parse(strings, T.T_I32, n=0) == T.OK and parse(strings, T.T_DEC128, 38, 38, n=0, o=None) == T.OK
    read_guarded(out, 0, "out")                                                      # nothing of it was touched: all 0xFF
    assert (read_guarded(bm, 0, "bitmap") is not None) and cnt.to_numpy(np.uint64, 2).tolist() == [0, 0]
    assert parse(strings, T.T_TIMESTAMP, off=64800) == T.OK and parse(strings, T.T_DEC64, 18, 18) == T.OK
    assert cnt.to_numpy(np.uint64, 2).tolist() == [3, 3]          # (digits only: declined; 1 at scale 18 needs 19 digits: Decimal overflow)
    cnt.zero()

    nbytes = C.c_uint64(77)

    def fmt_bytes(col, off=0, n=3):
        cc = col.c()
        return L.dbhip_str_format_bytes(C.byref(cc), C.c_int32(off), C.c_int64(n), C.byref(nbytes), None)

    def fmt(col, off=0, n=3, views=out):
        cc = col.c()
        return L.dbhip_str_format(C.byref(cc), C.c_int32(off), C.c_int64(n), C.c_void_p(views.ptr) if views else None, None, C.c_uint64(0), C.c_void_p(cnt.ptr), None)

    views = guarded(gpu, 64)
    for col in (strings, gpu.Column.from_numpy(np.zeros(3, dtype=np.float32)), gpu.Column.from_numpy(np.zeros(3, dtype=np.float64)), gpu.Column.boolean([True] * 3),
                gpu.Column.decimal256([1, 2, 3], 40, 2)):
        assert fmt_bytes(col) == T.ERR_UNSUPPORTED and fmt(col, views=views) == T.ERR_UNSUPPORTED
    bad = gpu.Column.decimal([1, 2, 3], 18, 2)
    bad.precision = 19
    assert fmt_bytes(bad) == T.ERR_INVALID and fmt(bad, views=views) == T.ERR_INVALID
    assert fmt_bytes(numbers, off=64801) == T.ERR_INVALID and fmt(numbers, off=-64801, views=views) == T.ERR_INVALID
    assert fmt_bytes(numbers, n=2**32 - 1) == T.ERR_INVALID and fmt(numbers, n=-1, views=views) == T.ERR_INVALID and fmt(numbers, views=None) == T.ERR_INVALID
    assert nbytes.value == 77
    assert fmt_bytes(numbers, n=0) == T.OK and nbytes.value == 0 and fmt(numbers, n=0, views=None) == T.OK
    read_guarded(views, 0, "out_views")
    assert cnt.to_numpy(np.uint64, 2).tolist() == [0, 0]
    assert fmt(numbers, views=views) == T.OK                                          # inline results need no out_data at all
    assert [bytes(r[4:5]) for r in views.to_numpy(np.uint8, 48).reshape(-1, 16)] == [b"1", b"2", b"3"]
