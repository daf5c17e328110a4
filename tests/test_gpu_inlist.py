"""GPU: dbhip_inlist_create / _path / _eval / _destroy (include/dbhip.h a23). Every row is asserted exactly against tests/inlist_ref.py
(plain Python, held to Python's `in`, numpy.isin, known answers and negative controls by tests/test_inlist_ref_cpu.py); nothing is
sampled. Both output Bitmaps are pre-filled with ones, so a word the call does not write, or a bit past n it leaves set, shows. String
columns are packed back to back without padding (tests/test_gpu_like.py's pack), so a comparison that reads outside a value reads its
neighbour's bytes — which the cases choose so that it then answers wrongly. Lists whose elements collide in the table are built with
the reference's restatement of the hash (checked against the header by tests/test_inlist_host_cpu.py)."""
import ctypes as C
import random
import struct
import threading
from collections import defaultdict

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import inlist_ref as R
from tests.test_gpu_like import pack

pytestmark = pytest.mark.gpu

K = R.COMPARE_MAX
ROW_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025)
NP = {T.T_I8: np.int8, T.T_I16: np.int16, T.T_I32: np.int32, T.T_I64: np.int64, T.T_U8: np.uint8, T.T_U16: np.uint16, T.T_U32: np.uint32,
      T.T_U64: np.uint64, T.T_F32: np.float32, T.T_F64: np.float64, T.T_DATE: np.int32, T.T_TIMESTAMP: np.int64, T.T_DEC64: np.int64}
ALL_TYPES = list(NP) + [T.T_DEC128, T.T_STRING]
NAME = {T.T_I8: "i8", T.T_I16: "i16", T.T_I32: "i32", T.T_I64: "i64", T.T_U8: "u8", T.T_U16: "u16", T.T_U32: "u32", T.T_U64: "u64", T.T_F32: "f32",
        T.T_F64: "f64", T.T_DATE: "date", T.T_TIMESTAMP: "timestamp", T.T_DEC64: "dec64", T.T_DEC128: "dec128", T.T_STRING: "string"}
PS = {T.T_DEC64: (15, 2), T.T_DEC128: (38, 6)}


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def f32_of_bits(b):
    return float(np.frombuffer(np.uint32(b).tobytes(), np.float32)[0])


def f64_of_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def pool(dtype, size=2200):
    """distinct values of the type, the extreme ones first"""
    seen = {}
    for x in _pool(dtype, size):
        seen.setdefault(R.canon(dtype, x), x)
    return list(seen.values())


def _pool(dtype, size):
    rng = random.Random(int(dtype))
    if dtype == T.T_STRING:
        fixed = [b"", b"a", b"ab", b"abcd", b"abcdefghijk", b"abcdefghijkl", b"abcdefghijklm", b"abcdefghijklmnop", b"q" * 255, "né".encode(),
                 b"same" + b"-" * 35 + b"A", b"same" + b"-" * 35 + b"B"]
        more = [b"%04d" % k + b"v" * (k % 23) for k in range(size)]
        return fixed + more
    if dtype == T.T_F32:
        fixed = [f32_of_bits(0x7FC00000), 0.0, float("inf"), -float("inf"), 1.5, -1.5, f32_of_bits(1)]
        return fixed + [float(np.float32(k) / np.float32(8)) for k in range(3, size)]
    if dtype == T.T_F64:
        fixed = [f64_of_bits(0x7FF8000000000000), 0.0, float("inf"), -float("inf"), 1.5, -1.5, 5e-324]
        return fixed + [k / 8 for k in range(3, size)]
    if dtype == T.T_DEC128:
        lo, hi = -(1 << 127), (1 << 127) - 1
        fixed = [lo, hi, 0, -1, 1, 7 + (1 << 64), 7 + (2 << 64), 7 - (1 << 64), 7, (1 << 64) - 1, -(1 << 64) - 1]     # equal low words
        return fixed + sorted({rng.randint(lo, hi) for _ in range(size)})
    info = np.iinfo(NP[dtype])
    if info.max - info.min < 70000:
        fixed = list(dict.fromkeys(x for x in (info.min, info.max, 0, -1) if info.min <= x <= info.max))
        rest = [x for x in range(info.min, info.max + 1) if x not in fixed]
        rng.shuffle(rest)
        return fixed + rest
    fixed = [info.min, info.max, 0, 1, info.max - 1, info.min + 1] + ([-1] if info.min < 0 else [])
    return fixed + sorted({rng.randint(info.min, info.max) for _ in range(size)} - set(fixed))


def aliases(dtype):
    """values that equal one of the pool's under another bit pattern: NaNs of other payloads, the negative zero"""
    if dtype == T.T_F32:
        return [f32_of_bits(0x7F800001), f32_of_bits(0xFFC12345), -0.0]
    if dtype == T.T_F64:
        return [f64_of_bits(0x7FF0000000000001), f64_of_bits(0xFFF8000000012345), -0.0]
    return []


def make_rows(dtype, items, others, n, seed, null_share=0.2):
    """n rows, about half of them members, and their validity"""
    rng = random.Random(seed)
    src = [(list(items) or list(others)) + aliases(dtype), list(others) or list(items)]
    rows = [rng.choice(src[rng.random() < 0.5]) for _ in range(n)]
    valid = [rng.random() >= null_share for _ in range(n)]
    return rows, valid


def column(gpu, dtype, rows, valid=None, voff=0, seed=0):
    """`voff`: the validity Bitmap starts that many (arbitrary) bits before the first row's bit"""
    vfull = None
    if valid is not None:
        rng = random.Random(seed)
        vfull = [rng.random() < 0.5 for _ in range(voff)] + list(valid)
    if dtype == T.T_STRING:
        col = pack(gpu, rows, vfull, lead=b"\xEE")
    elif dtype == T.T_DEC128:
        col = gpu.Column.decimal128(rows, *PS[dtype], validity=vfull)
    else:
        p, s = PS.get(dtype, (0, 0))
        col = gpu.Column.from_numpy(np.array(rows, dtype=NP[dtype]), dtype, vfull, p, s)
    col.voff = voff
    return col


def make_set(gpu, dtype, items, has_null=False):
    p, s = PS.get(dtype, (0, 0))
    return gpu.InList(dtype, items, has_null, p, s)


def run(gpu, inl, col, n=None, negate=False, want_validity=True, stream=None):
    """dbhip_inlist_eval on Bitmaps pre-filled with ones: exactly ceil(n / 64) words written, the bits past n zero -> (bits, validity bits)"""
    n = col.n if n is None else n
    words = (n + 63) // 64
    outs = [gpu.DeviceBuffer.from_numpy(np.full(words * 8 + 16, 0xFF, dtype=np.uint8)) for _ in range(2 if want_validity else 1)]
    cc = col.c()
    T.check(T.lib().dbhip_inlist_eval(C.c_void_p(inl.handle), C.byref(cc), C.c_int32(T.IN_NEGATE if negate else 0), C.c_int64(n), C.c_void_p(outs[0].ptr),
                                      C.c_void_p(outs[1].ptr) if want_validity else None, stream))
    if stream is not None:
        T.check(T.lib().dbhip_stream_sync(stream))
    res = []
    for o in outs:
        raw = o.to_numpy(np.uint8)
        assert (raw[words * 8:] == 0xFF).all(), "wrote past ceil(n / 64) words"
        bits = np.unpackbits(raw[:words * 8], bitorder="little")
        assert not bits[n:].any(), "bits past n"
        res.append(bits[:n].astype(bool).tolist())
    return res[0], (res[1] if want_validity else None)


def assert_rows(got, exp, rows, what):
    if got != exp:
        bad = [i for i in range(len(exp)) if got[i] != exp[i]]
        raise AssertionError(f"{what}: {len(bad)} of {len(exp)} rows differ, first row {bad[0]} value {rows[bad[0]]!r:.90} got {got[bad[0]]} expected {exp[bad[0]]}")


def check(gpu, inl, col, dtype, rows, valid, items, has_null=False, negate=False, n=None, want_validity=True, what="", both=True, stream=None):
    n = len(rows) if n is None else n
    bits, vbits = run(gpu, inl, col, n, negate, want_validity, stream)
    eb, ev = R.evaluate(dtype, rows[:n], None if valid is None else valid[:n], items, has_null, negate)
    assert_rows(bits, eb, rows, f"{what} filter")
    if want_validity:
        assert_rows(vbits, ev, rows, f"{what} validity")
    if both:
        assert any(eb) and not all(eb), f"{what}: a case sees both answers"
    return bits


def item_lists(dtype):
    """(items, values that are no element): 0, 1, 2, the threshold, the threshold + 1 and 1024 elements, duplicates included"""
    p = pool(dtype)
    out = []
    for k in (0, 1, 2, K, K + 1, 1024):
        nd = min(k, len(p) // 2)                                   # (the one-byte types have 256 values: half of them at the most)
        distinct = p[:nd]
        if nd < k:
            items = (distinct * (k // nd + 1))[:k]
        elif 2 <= k < 1024:
            items = distinct + distinct[:2]
        else:
            items = list(distinct)
        out.append((k, items, distinct, p[nd:nd + 40]))
    return out


# ---- per type and path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_TYPES, ids=[NAME[t] for t in ALL_TYPES])
def test_every_type_item_count_and_row_count(gpu, dtype):
    paths = set()
    for k, items, distinct, others in item_lists(dtype):
        inl = make_set(gpu, dtype, items)
        paths.add(inl.path)
        exp_path = T.IN_PATH_BITS if R.WIDTH[dtype] <= 2 else (T.IN_PATH_COMPARE if len(distinct) <= K else T.IN_PATH_TABLE)
        assert inl.path == exp_path, (k, inl.path)
        rows, valid = make_rows(dtype, distinct, others, max(ROW_COUNTS), seed=k)
        col = column(gpu, dtype, rows, valid)
        for j, n in enumerate(ROW_COUNTS):
            check(gpu, inl, col, dtype, rows, valid, items, negate=bool(j & 1), n=n, what=f"{NAME[dtype]} k={k} n={n}", both=k > 0 and n >= 63)
        inl.destroy()
    assert paths == ({T.IN_PATH_BITS} if R.WIDTH[dtype] <= 2 else {T.IN_PATH_COMPARE, T.IN_PATH_TABLE})


def test_more_rows_than_one_sweep_of_the_grid(gpu):
    """the launched grid is at most 1024 workgroups of 256 lanes with 16 one-byte rows each: 4 Mi rows a sweep. One sweep, a second one
    and an odd remainder. The expected bits come from the reference's answer for each of the 256 values, valid and NULL."""
    n = 1024 * 256 * 16 + 3 * 64 * 16 + 777
    rng = np.random.default_rng(3)
    arr = rng.integers(-128, 128, n).astype(np.int8)
    valid = rng.random(n) < 0.9
    items = [-128, -1, 0, 5, 5, 77, 127]
    table = np.zeros((2, 256), dtype=bool)
    for ok in (0, 1):
        table[ok], _ = R.evaluate(T.T_I8, list(range(-128, 128)), [bool(ok)] * 256, items)
    exp = table[valid.astype(np.int64), arr.astype(np.int64) + 128]
    inl = make_set(gpu, T.T_I8, items)
    col = gpu.Column.from_numpy(arr, T.T_I8, valid)
    res = gpu.in_list(col, inl)
    got = gpu.unpack_bits(res.data.to_numpy(np.uint8, ((n + 63) // 64) * 8), n)
    assert np.array_equal(got, exp) and exp.any() and not exp.all()
    assert not np.unpackbits(res.data.to_numpy(np.uint8, ((n + 63) // 64) * 8), bitorder="little")[n:].any()
    inl.destroy()


def test_bits_all_u8_values_and_the_i16_corners(gpu):
    rows = list(range(256)) * 3
    valid = [i % 7 != 0 for i in range(len(rows))]
    inl = make_set(gpu, T.T_U8, list(range(256)))
    col = column(gpu, T.T_U8, rows, valid)
    assert check(gpu, inl, col, T.T_U8, rows, valid, list(range(256)), what="u8 all") == valid
    assert not any(check(gpu, inl, col, T.T_U8, rows, valid, list(range(256)), negate=True, what="u8 none", both=False))
    inl.destroy()
    items = [-32768, -1, 0, 32767]
    rows = items + [-32767, -2, 1, 32766, 255, 256, -256] + list(range(-40, 40))
    inl = make_set(gpu, T.T_I16, items)
    col = column(gpu, T.T_I16, rows)
    check(gpu, inl, col, T.T_I16, rows, None, items, what="i16 corners")
    check(gpu, inl, col, T.T_I16, rows, None, items, negate=True, what="i16 corners, NOT IN")
    inl.destroy()


@pytest.mark.parametrize("dtype", [T.T_I64, T.T_U64, T.T_DEC128, T.T_F32, T.T_F64], ids=["i64", "u64", "dec128", "f32", "f64"])
@pytest.mark.parametrize("table", [False, True], ids=["compare", "table"])
def test_extreme_values(gpu, dtype, table):
    """I64 / U64 at the ends of their ranges, DEC128 values that differ only in the high word, NaNs of different payloads, both zeros and
    both infinities — as elements and as rows that are none"""
    p = pool(dtype)
    special = p[:11] if dtype == T.T_DEC128 else p[:7] + aliases(dtype)
    for pick in (0, 1):
        items = special[pick::2] + (p[20:20 + 2 * K] if table else [])
        rows = special * 9 + p[100:140]
        inl = make_set(gpu, dtype, items)
        assert inl.path == (T.IN_PATH_TABLE if table else T.IN_PATH_COMPARE)
        col = column(gpu, dtype, rows)
        check(gpu, inl, col, dtype, rows, None, items, what=f"{NAME[dtype]} extremes {pick}")
        inl.destroy()


# ---- NULLs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", [(T.T_I32, 5), (T.T_I64, 40), (T.T_STRING, 7), (T.T_U8, 9)], ids=["i32", "i64-table", "string", "u8-bits"])
def test_negate_has_null_validity_and_offsets(gpu, dtype, k):
    p = pool(dtype)
    items, others = p[:k], p[k:k + 30]
    rows, valid = make_rows(dtype, items, others, 333, seed=4)
    for has_null in (False, True):
        inl = make_set(gpu, dtype, items, has_null)
        for voff in (0, 3, 69):
            col = column(gpu, dtype, rows, valid, voff, seed=voff)
            for negate in (False, True):
                for want in (True, False):
                    bits = check(gpu, inl, col, dtype, rows, valid, items, has_null, negate, want_validity=want, both=not (has_null and negate),
                                 what=f"{NAME[dtype]} has_null={has_null} negate={negate} voff={voff}")
                    if has_null and negate:
                        assert not any(bits), "x NOT IN (.., NULL) is never TRUE"
        col = column(gpu, dtype, rows)                        # no validity Bitmap at all
        check(gpu, inl, col, dtype, rows, None, items, has_null, what="no validity")
        inl.destroy()


def test_a_null_row_whose_long_view_points_nowhere(gpu):
    member = b"a long element of 27 bytes!"
    values = [member, b"short", member, b"x" * 20, member, member[:-1] + b"?"] * 11
    valid = [i % 3 != 2 for i in range(len(values))]
    col = pack(gpu, values, valid, buffer_of=lambda i: 0 if valid[i] else 5)      # the NULL rows name buffer 5 of a one-buffer column
    for items in ([member, b"short"], [member] + [b"%03d-filler-element" % j for j in range(20)]):
        inl = make_set(gpu, T.T_STRING, items)
        for negate in (False, True):
            check(gpu, inl, col, T.T_STRING, values, valid, items, negate=negate, what=f"NULL rows, {len(items)} items")
        inl.destroy()


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", [(T.T_I32, 5), (T.T_I32, 50), (T.T_I64, 5), (T.T_I64, 50), (T.T_F32, 5)], ids=["i32", "i32-table", "i64", "i64-table", "f32"])
def test_a_sliced_column_whose_base_is_not_16_byte_aligned(gpu, dtype, k):
    p = pool(dtype)
    items, others = p[:k], p[k:k + 30]
    rows, valid = make_rows(dtype, items, others, 1100, seed=8)
    full = column(gpu, dtype, rows, valid)
    inl = make_set(gpu, dtype, items)
    for lo in (1, 3):
        col = full.slice(lo, len(rows))
        assert col.data.ptr % 16 != 0
        check(gpu, inl, col, dtype, rows[lo:], valid[lo:], items, what=f"{NAME[dtype]} sliced by {lo}")
        check(gpu, inl, col, dtype, rows[lo:], valid[lo:], items, negate=True, n=70, what=f"{NAME[dtype]} sliced by {lo}, 70 rows")
    inl.destroy()


@pytest.mark.parametrize("dtype", [T.T_I16, T.T_I32, T.T_F64, T.T_DEC128, T.T_STRING], ids=["i16", "i32", "f64", "dec128", "string"])
def test_scalar_columns(gpu, dtype):
    p = pool(dtype)
    n = 130
    for k, value, ok in ((5, p[3], True), (5, p[30], True), (5, p[3], False), (20, p[3], True), (20, p[30], True), (20, p[3], False)):
        items = p[:k]
        inl = make_set(gpu, dtype, items)
        if dtype == T.T_STRING:
            col = pack(gpu, [value], lead=b"\xEE")
            col.is_scalar = True
        else:
            col = gpu.Column.scalar(value, dtype, *PS.get(dtype, (0, 0)))
        if not ok:
            col.validity = gpu.DeviceBuffer.from_numpy(gpu.pack_bits([False]))
        for negate in (False, True):
            bits, vbits = run(gpu, inl, col, n, negate)
            eb, ev = R.evaluate(dtype, [value] * n, [ok] * n, items, False, negate)
            assert (bits, vbits) == (eb, ev), (NAME[dtype], k, value, ok, negate)
        inl.destroy()


# ---- Strings ----------------------------------------------------------------------------------------------------------------------
def string_values():
    base = [b"", b"a", b"abcd", b"abcdefghijk", b"abcdefghijkl", b"abcdefghijklm", b"abcdefghijklmnop", b"q" * 255, b"q" * 256, b"q" * 4000,
            "naïve café".encode(), b"same" + b"-" * 35 + b"A", b"same" + b"-" * 35 + b"B", b"same" + b"-" * 35 + b"C"]
    out = []
    for s in base:
        out += [s, s + b"!", s[:-1], s[:-1] + bytes([(s[-1] if s else 0) ^ 1])]
    # a value whose following neighbour in the buffer would complete a match: "abcdefghijklm" + "nop" = an element
    out += [b"abcdefghijklm", b"nopqrstuvwxyz", b"abcdefghijklmnop", b"abcdefghijklmno", b"pabcdefghijklmnop"]
    return out


STRING_LISTS = {
    "inline": [b"a", b"abcd", b"abcdefghijkl", b"abcdefghijk"],
    "long": [b"abcdefghijklm", b"abcdefghijklmnop", b"q" * 255],
    "mix-empty": [b"", b"a", b"abcdefghijklmnop", b"q" * 255, "naïve café".encode()],
    "prefixes": [b"a", b"ab", b"abcd", b"abcdefghijkl", b"abcdefghijklm", b"abcdefghijklmno", b"abcdefghijklmnop"],
    "same-prefix": [b"same" + b"-" * 35 + b"A", b"same" + b"-" * 35 + b"B", b"abcdefghijklmnop"],
}


@pytest.mark.parametrize("name", list(STRING_LISTS))
@pytest.mark.parametrize("table", [False, True], ids=["compare", "table"])
def test_strings(gpu, name, table):
    values = string_values() * 2
    valid = [i % 11 != 5 for i in range(len(values))]
    items = STRING_LISTS[name] + ([b"%03d-filler" % j + b"z" * (j % 9) for j in range(K + 4)] if table else [])
    inl = make_set(gpu, T.T_STRING, items)
    assert inl.path == (T.IN_PATH_TABLE if table else T.IN_PATH_COMPARE)
    for n_buffers in (1, 3):
        col = pack(gpu, values, valid, lead=b"abc"[:n_buffers], n_buffers=n_buffers)
        for negate in (False, True):
            check(gpu, inl, col, T.T_STRING, values, valid, items, negate=negate, what=f"{name} buffers={n_buffers}")
    inl.destroy()


@pytest.mark.parametrize("table", [False, True], ids=["compare", "table"])
def test_a_long_view_with_a_bad_buffer_index_is_no_member(gpu, table):
    e1, e2 = b"an element of twenty bytes"[:20], b"another element, 33 bytes long...."[:33]
    items = [e1, e2, b"short"] + ([b"%03d-filler-element" % j for j in range(K + 2)] if table else [])
    values = [e1, e2, b"short", e1 + b"x", e2] * 13
    bad = lambda i: i % 4 == 1
    col = pack(gpu, values, None, n_buffers=2, buffer_of=lambda i: 7 if bad(i) else i % 2)
    inl = make_set(gpu, T.T_STRING, items)
    bits, vbits = run(gpu, inl, col)
    eb, ev = R.evaluate(T.T_STRING, values, None, items)
    exp = [e and not (bad(i) and len(values[i]) > 12) for i, e in enumerate(eb)]
    assert bits == exp and vbits == ev and exp != eb
    nbits, _ = run(gpu, inl, col, negate=True)
    assert nbits == [not e for e in exp]
    inl.destroy()


# ---- the table's corners -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [T.T_I32, T.T_I64, T.T_DEC128, T.T_STRING], ids=["i32", "i64", "dec128", "string"])
def test_lists_whose_elements_collide(gpu, dtype):
    slots = 64
    cand = [b"%06d" % x for x in range(60000)] if dtype == T.T_STRING else list(range(1000, 61000))
    same = R.colliding(dtype, 9, slots, 40, cand)                       # nine elements with one home slot
    wrap = R.colliding(dtype, 5, slots, slots - 1, cand)                # a run that goes on at slot 0
    fill = [c for c in cand[:200] if c not in same and c not in wrap and R.home(dtype, c, slots) not in (0, 1, 2, 3)][:8]
    items = same + wrap + fill
    assert R.inl_slots(len(items)) == slots
    rest = [c for c in cand if c not in set(items)]
    near = R.colliding(dtype, 3, slots, 40, rest) + R.colliding(dtype, 3, slots, slots - 1, rest)     # no elements, the same home slots
    rows = (items + near + cand[300:330]) * 3
    inl = make_set(gpu, dtype, items)
    assert inl.path == T.IN_PATH_TABLE
    col = column(gpu, dtype, rows)
    check(gpu, inl, col, dtype, rows, None, items, what=f"{NAME[dtype]} collisions")
    check(gpu, inl, col, dtype, rows, None, items, negate=True, what=f"{NAME[dtype]} collisions, NOT IN")
    inl.destroy()


@pytest.mark.parametrize("dtype", [T.T_I64, T.T_U64, T.T_DEC64, T.T_DEC128], ids=["i64", "u64", "dec64", "dec128"])
@pytest.mark.parametrize("k", [3, 30])
def test_the_sentinel_value_as_column_data(gpu, dtype, k):
    s = R.sentinel(dtype)
    p = [x for x in pool(dtype) if x != s]
    rows = ([s, p[0], p[1], p[k + 5], s] + p[:k + 10]) * 4
    col = column(gpu, dtype, rows)
    for items in (p[:k], p[:k] + [s]):
        inl = make_set(gpu, dtype, items)
        bits = check(gpu, inl, col, dtype, rows, None, items, what=f"{NAME[dtype]} sentinel in list: {s in items}")
        assert bits[0] == (s in items)
        inl.destroy()


# ---- composition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", [(T.T_I32, 8), (T.T_DEC128, 40), (T.T_STRING, 7)], ids=["i32-8", "dec128-40", "string-7"])
def test_equals_the_comparisons_ored_on_the_device(gpu, dtype, k):
    """the launches this call replaces: k x dbhip_cmp(EQ, col, scalar) and k - 1 x dbhip_bitmap_binary(OR) on the same column"""
    p = pool(dtype)
    items = p[:k]
    rows, _ = make_rows(dtype, items, p[k:k + 40], 1500, seed=12)
    col = column(gpu, dtype, rows)
    n = len(rows)
    acc = None
    for e in items:
        if dtype == T.T_STRING:
            sc = pack(gpu, [e])
            sc.is_scalar = True
        else:
            sc = gpu.Column.scalar(e, dtype, *PS.get(dtype, (0, 0)))
        eq = gpu.cmp(T.CMP_EQ, col, sc, n)
        if acc is None:
            acc = eq.data
        else:
            nxt = gpu.DeviceBuffer(((n + 63) // 64) * 8 + 8)
            T.check(T.lib().dbhip_bitmap_binary(1, C.c_void_p(acc.ptr), C.c_void_p(eq.data.ptr), C.c_int64(n), C.c_void_p(nxt.ptr), None))
            acc = nxt
    composed = gpu.unpack_bits(acc.to_numpy(np.uint8, (n + 7) // 8), n).tolist()
    inl = make_set(gpu, dtype, items)
    bits = check(gpu, inl, col, dtype, rows, None, items, what="composition")
    assert bits == composed
    inl.destroy()


# ---- two query shapes -------------------------------------------------------------------------------------------------------------
def test_q22_substr_in_list_filtered_group_by(gpu):
    """select substring(c_phone from 1 for 2), count(*), sum(c_acctbal) .. where substring(c_phone from 1 for 2) in (7 codes) group by 1"""
    n = 4096
    rng = np.random.default_rng(22)
    phones = [b"%02d-%03d-%03d-%04d" % (int(c), int(x), int(y), int(z)) for c, x, y, z in zip(rng.integers(10, 35, n), rng.integers(100, 1000, n),
                                                                                             rng.integers(100, 1000, n), rng.integers(1000, 10000, n))]
    bal = rng.integers(-99999, 999999, n).astype(np.int64)
    codes = [b"13", b"31", b"23", b"29", b"30", b"18", b"17"]
    key = gpu.substr(pack(gpu, phones, lead=b"7"), 1, 2)
    inl = gpu.InList(T.T_STRING, codes)
    assert inl.path == T.IN_PATH_COMPARE
    flt = gpu.in_list(key, inl)
    g = gpu.GroupBy([T.T_STRING], [(T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_I64, 0, 0, 0)])
    g.add_block([key], [None, gpu.Column.from_numpy(bal)], n, filter=flt)
    got = sorted(g.result())
    g.destroy()
    inl.destroy()
    exp = defaultdict(lambda: [0, 0])
    for p, b in zip(phones, bal):
        if p[:2] in codes:
            exp[p[:2]][0] += 1
            exp[p[:2]][1] += int(b)
    assert got == sorted((c, v[0], v[1]) for c, v in exp.items()) and len(got) == 7


def test_q16_not_in_and_not_like_then_select(gpu):
    """.. where p_size not in (8 ints) and p_type not like 'MEDIUM POLISHED%' -> the selection vector"""
    n = 4096
    rng = np.random.default_rng(16)
    size = rng.integers(1, 51, n).astype(np.int32)
    kinds = [b"MEDIUM POLISHED", b"MEDIUM BRUSHED", b"LARGE POLISHED", b"ECONOMY ANODIZED", b"SMALL"]
    metals = [b" TIN", b" COPPER", b" STEEL", b""]
    ptype = [kinds[a] + metals[b] for a, b in zip(rng.integers(0, 5, n), rng.integers(0, 4, n))]
    sizes = [49, 14, 23, 45, 19, 3, 36, 9]
    inl = gpu.InList(T.T_I32, sizes)
    f1 = gpu.in_list(gpu.Column.from_numpy(size), inl, negate=True)
    f2 = gpu.like(pack(gpu, ptype), b"MEDIUM POLISHED%", negate=True)
    both = gpu.DeviceBuffer(((n + 63) // 64) * 8 + 8)
    T.check(T.lib().dbhip_bitmap_binary(0, C.c_void_p(f1.data.ptr), C.c_void_p(f2.data.ptr), C.c_int64(n), C.c_void_p(both.ptr), None))
    sel, cnt = gpu.filter_select(gpu.Column(T.T_BOOL, n, both))
    exp = [i for i in range(n) if int(size[i]) not in sizes and not ptype[i].startswith(b"MEDIUM POLISHED")]
    assert cnt == len(exp) and sel.to_numpy(np.uint32, cnt).tolist() == exp and 0 < cnt < n
    inl.destroy()


# ---- handles ----------------------------------------------------------------------------------------------------------------------
def test_one_handle_from_four_threads_on_four_streams(gpu):
    p = pool(T.T_I64)
    items = p[:200]
    inl = make_set(gpu, T.T_I64, items, has_null=True)
    errors = []

    def worker(tid):
        try:
            stream = C.c_void_p()
            T.check(T.lib().dbhip_stream_create(C.byref(stream)))
            rows, valid = make_rows(T.T_I64, items, p[200:300], 5000 + 64 * tid + tid, seed=100 + tid)
            col = column(gpu, T.T_I64, rows, valid)
            for r in range(6):
                check(gpu, inl, col, T.T_I64, rows, valid, items, True, negate=False, what=f"thread {tid} round {r}", stream=stream)
            T.check(T.lib().dbhip_stream_destroy(stream))
        except BaseException as e:  # noqa: BLE001 — reported by the main thread
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads)
    inl.destroy()


def test_destroy_then_create_again(gpu):
    p = pool(T.T_I32)
    rows, valid = make_rows(T.T_I32, p[:40], p[40:80], 500, seed=2)
    col = column(gpu, T.T_I32, rows, valid)
    for items in (p[:40], p[:3], p[20:60]):
        inl = make_set(gpu, T.T_I32, items)
        check(gpu, inl, col, T.T_I32, rows, valid, items, what=f"{len(items)} items")
        inl.destroy()
        inl.destroy()                                             # a second destroy of the Python object is a no-op
    assert T.lib().dbhip_inlist_destroy(None) == T.OK


def test_refusals_leave_the_stream_usable(gpu):
    L = T.lib()
    h = C.c_void_p()
    vals = (C.c_int64 * 2000)(*range(2000))
    offs = (C.c_uint32 * 2000)(*range(2000))

    def create(dtype, values, offsets, n, out=h):
        return L.dbhip_inlist_create(C.c_int32(dtype), C.c_uint8(0), C.c_uint8(0), values, offsets, C.c_int32(n), C.c_int32(0), C.byref(out) if out is not None else None)

    assert create(T.T_BOOL, vals, None, 2) == T.ERR_UNSUPPORTED
    assert create(T.T_DEC256, vals, None, 2) == T.ERR_UNSUPPORTED
    assert create(T.T_I64, vals, None, T.IN_MAX_ITEMS + 1) == T.ERR_UNSUPPORTED
    assert create(T.T_I64, vals, None, T.IN_MAX_ITEMS) == T.OK and L.dbhip_inlist_destroy(h) == T.OK
    assert create(T.T_I64, None, None, 2) == T.ERR_INVALID
    assert create(T.T_I64, vals, None, -1) == T.ERR_INVALID
    assert create(0, vals, None, 2) == T.ERR_INVALID and create(99, vals, None, 2) == T.ERR_INVALID
    assert create(T.T_I64, vals, None, 2, out=None) == T.ERR_INVALID
    assert create(T.T_STRING, vals, None, 2) == T.ERR_INVALID, "a String list needs offsets"
    assert create(T.T_STRING, vals, (C.c_uint32 * 3)(0, 5, 4), 2) == T.ERR_INVALID, "descending offsets"
    assert create(T.T_STRING, vals, (C.c_uint32 * 2)(0, 256), 1) == T.ERR_UNSUPPORTED, "an element of 256 bytes"
    assert create(T.T_STRING, vals, (C.c_uint32 * 2)(0, 255), 1) == T.OK and L.dbhip_inlist_destroy(h) == T.OK
    big = (C.c_uint32 * 67)(*[250 * j for j in range(67)])         # 66 x 250 bytes of long elements: more than 16 KiB
    assert create(T.T_STRING, (C.c_uint8 * 16500)(), big, 66) == T.ERR_UNSUPPORTED
    assert create(T.T_STRING, (C.c_uint8 * 16500)(), big, 65) == T.OK and L.dbhip_inlist_destroy(h) == T.OK
    assert create(T.T_I64, None, None, 0) == T.OK and L.dbhip_inlist_path(h) == T.IN_PATH_COMPARE and L.dbhip_inlist_destroy(h) == T.OK
    del offs

    # eval
    p = pool(T.T_I32)
    rows, valid = make_rows(T.T_I32, p[:5], p[5:30], 300, seed=1)
    col = column(gpu, T.T_I32, rows, valid)
    inl = make_set(gpu, T.T_I32, p[:5])
    dec = make_set(gpu, T.T_DEC64, [1, 2, 3])
    out = gpu.DeviceBuffer(64 * 8)

    def ev(s, c, flags, n, o=out.ptr):
        cc = c.c()
        return L.dbhip_inlist_eval(C.c_void_p(s.handle) if s is not None else None, C.byref(cc), C.c_int32(flags), C.c_int64(n), C.c_void_p(o), None, None)

    assert ev(inl, col, 2, 300) == T.ERR_INVALID and ev(inl, col, -1, 300) == T.ERR_INVALID, "unknown flag bits"
    assert ev(inl, col, 0, (1 << 32) - 1) == T.ERR_INVALID and ev(inl, col, 0, -1) == T.ERR_INVALID
    assert ev(inl, column(gpu, T.T_U32, [1, 2, 3]), 0, 3) == T.ERR_INVALID, "the column's type is not the set's"
    assert ev(dec, gpu.Column.decimal([1, 2, 9], 15, 3), 0, 3) == T.ERR_INVALID, "another scale"
    assert ev(dec, gpu.Column.decimal([1, 2, 9], 15, 2), 0, 3) == T.OK
    assert ev(None, col, 0, 300) == T.ERR_INVALID
    assert ev(inl, col, 0, 300, o=out.ptr + 4) == T.ERR_INVALID, "a Bitmap that is not 8-byte aligned"
    assert ev(inl, col, 0, 0, o=None) == T.OK, "n = 0"
    assert b"DBHIP_IN" not in L.dbhip_last_error()
    check(gpu, inl, col, T.T_I32, rows, valid, p[:5], what="after the refusals")
    inl.destroy()
    dec.destroy()
