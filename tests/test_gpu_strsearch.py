"""GPU: dbhip_str_position / dbhip_str_split_part / dbhip_str_rewrite_bytes / dbhip_str_rewrite (include/dbhip.h a28), every row asserted
exactly against tests/strsearch_ref.py (plain Python, held to Python's own operations and to negative controls by
tests/test_strsearch_ref_cpu.py): every position, the full 16 bytes of every result view, every byte of every rewritten value. Nothing is
sampled. Columns are packed by tests/test_gpu_strfn.py's helper: the long values lie back to back in their data buffers without padding,
behind a lead of 1 to 3 bytes, so every alignment occurs and a kernel that reads outside a value reads its neighbours' bytes. Every
output is pre-filled with 0xFF and has guard bytes behind it that must stay 0xFF."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import str_ref as S
from tests import strfn_cases as FK
from tests import strsearch_cases as K
from tests import strsearch_ref as R
from tests.test_gpu_strfn import _host, assert_views, dirty, guarded, i64, pack, read_guarded, usable

pytestmark = pytest.mark.gpu

LEADS = [b"\xbf", b"\x80\x80", b"\xbf\x80\x80"]      # continuation bytes in front of the first long value


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def ref(col, k):
    return C.byref(k) if k is not None else None


def run_position(gpu, col, needle, start=None, unit_byte=False, n=None):
    n = col.n if n is None else n
    out = guarded(gpu, n * 8)
    cc = col.c()
    cs = i64(gpu, start, n)
    ccs = cs.c() if cs else None
    T.check(T.lib().dbhip_str_position(C.byref(cc), _host(needle), C.c_int32(len(needle)), ref(col, ccs), C.c_int32(T.STR_UNIT_BYTE if unit_byte else 0),
                                       C.c_int64(n), C.c_void_p(out.ptr), None))
    return read_guarded(out, n * 8, "out").view(np.uint64).tolist()


def run_split(gpu, col, delim, part, n=None):
    n = col.n if n is None else n
    out = guarded(gpu, n * 16)
    cc = col.c()
    cp = i64(gpu, part, n)
    ccp = cp.c()
    T.check(T.lib().dbhip_str_split_part(C.byref(cc), _host(delim), C.c_int32(len(delim)), C.byref(ccp), C.c_int64(n), C.c_void_p(out.ptr), None))
    return [bytes(r) for r in read_guarded(out, n * 16, "out_views").reshape(-1, 16)]


def run_rewrite(gpu, op, col, k=None, x=b"", y=b"", unit_byte=False, n=None, short_by=0):
    """the count call, then the rewrite into a buffer of exactly that size (less short_by) -> (views, data bytes, err, counted bytes)"""
    n = col.n if n is None else n
    cc = col.c()
    ck = i64(gpu, k, n)
    cck = ck.c() if ck else None
    flags = C.c_int32(T.STR_UNIT_BYTE if unit_byte else 0)
    nbytes = C.c_uint64(0xDEADBEEF)
    T.check(T.lib().dbhip_str_rewrite_bytes(C.c_int32(op), C.byref(cc), ref(col, cck), _host(x), C.c_int32(len(x)), _host(y), C.c_int32(len(y)), flags, C.c_int64(n),
                                            C.byref(nbytes), None))
    size = nbytes.value - short_by
    views, data = guarded(gpu, n * 16), guarded(gpu, size)
    counter = gpu.DeviceBuffer.from_numpy(np.array([0], dtype=np.uint64))
    T.check(T.lib().dbhip_str_rewrite(C.c_int32(op), C.byref(cc), ref(col, cck), _host(x), C.c_int32(len(x)), _host(y), C.c_int32(len(y)), flags, C.c_int64(n),
                                      C.c_void_p(views.ptr), C.c_void_p(data.ptr), C.c_uint64(size), C.c_void_p(counter.ptr), None))
    v = [bytes(r) for r in read_guarded(views, n * 16, "out_views").reshape(-1, 16)]
    d = read_guarded(data, size, "out_data").tobytes()
    return v, d, int(counter.to_numpy(np.uint64, 1)[0]), nbytes.value


def at(x, i):
    return x if x is None or isinstance(x, int) else x[i]


def rows_of(col, values, valid, n):
    """per row: the value, or None for a NULL row and for a long view that points nowhere"""
    n = col.n if n is None else n
    return [values[0 if col.is_scalar else i] if usable(col, 0 if col.is_scalar else i, valid) else None for i in range(n)]


def check_position(gpu, col, values, valid, needle, start=None, unit_byte=False, n=None, what=""):
    got = run_position(gpu, col, needle, start, unit_byte, n)
    exp = [0 if v is None else R.position(v, needle, 1 if start is None else at(start, i), unit_byte) for i, v in enumerate(rows_of(col, values, valid, n))]
    bad = [i for i in range(len(exp)) if got[i] != exp[i]]
    assert not bad, (what, needle[:20], unit_byte, len(bad), bad[0], got[bad[0]], exp[bad[0]], at(start, bad[0]), values[0 if col.is_scalar else bad[0]][:60])
    return exp


def check_split(gpu, col, values, valid, delim, part, n=None, what=""):
    got = run_split(gpu, col, delim, part, n)
    exp = []
    for i, v in enumerate(rows_of(col, values, valid, n)):
        rng = None if v is None else R.split_range(v, delim, at(part, i))
        _, _, idx, off = (int(x) for x in col.host_views[0 if col.is_scalar else i])
        exp.append(S.ZERO_VIEW if rng is None else S.slice_view(v, rng, idx, off))
    assert_views(got, exp, f"{what} split_part delim {delim[:16]!r}", lambda i: f"value {values[0 if col.is_scalar else i][:60]!r} part {at(part, i)}")
    return exp


def expect_rewrite(results):
    """per row the result bytes, None (NULL / unusable: the zero view) or R.TOO_LONG (the empty view, counted) -> (views, data, errors)"""
    views, data, err = [], b"", 0
    for r in results:
        if r is None or r == R.TOO_LONG:
            err += r is not None
            views.append(S.ZERO_VIEW)
            continue
        views.append(S.view(r, 0, len(data)))
        if len(r) > 12:
            data += r
    return views, data, err


def check_rewrite(gpu, op, col, values, valid, k=None, x=b"", y=b"", unit_byte=False, n=None, what=""):
    v, d, err, nbytes = run_rewrite(gpu, op, col, k, x, y, unit_byte, n)
    results = [None if val is None else R.rewrite(op, val, at(k, i) or 0, x, y, unit_byte) for i, val in enumerate(rows_of(col, values, valid, n))]
    ev, ed, eerr = expect_rewrite(results)
    label = f"{what} op {op} x {x[:16]!r} y {y[:16]!r} unit_byte {unit_byte}"
    assert nbytes == len(ed), (label, nbytes, len(ed))
    assert_views(v, ev, label, lambda i: f"value {values[0 if col.is_scalar else i][:60]!r} (len {len(values[0 if col.is_scalar else i])}) k {at(k, i)}")
    assert d == ed, (label, "out_data differs", next(i for i in range(len(ed)) if d[i] != ed[i]))
    assert err == eerr, (label, err, eerr)
    return results


def groups(rows, key, rest):
    out = {}
    for r in rows:
        out.setdefault(key(r), []).append(rest(r))
    return sorted(out.items(), key=lambda kv: repr(kv[0]))


# ---- row counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_row_counts(gpu, n):
    """the last partial wave, more than one workgroup, a nullable column over two data buffers; every entry point"""
    rng = np.random.default_rng(n)
    pool = K.pool(b"ab" + S.E3)
    values = [pool[k] for k in rng.integers(0, len(pool), n)]
    valid = rng.random(n) < 0.8
    col = pack(gpu, values, valid=valid, lead=b"\x80", n_buffers=2)
    start = [int(x) for x in rng.integers(-1, 9, n)]
    part = [int(x) for x in rng.integers(-4, 5, n)]
    ln = [int(x) for x in rng.integers(-1, 300, n)]
    for unit_byte in (False, True):
        check_position(gpu, col, values, valid, b"ab", start, unit_byte, what=f"n={n}")
        check_rewrite(gpu, R.LPAD, col, values, valid, ln, S.E3 + b"x", unit_byte=unit_byte, what=f"n={n}")
        check_rewrite(gpu, R.REVERSE, col, values, valid, unit_byte=unit_byte, what=f"n={n}")
    check_split(gpu, col, values, valid, b"a", part, what=f"n={n}")
    check_rewrite(gpu, R.REPLACE, col, values, valid, None, b"ab", b"<->", what=f"n={n}")
    check_rewrite(gpu, R.RPAD, col, values, valid, ln, b"xy", what=f"n={n}")
    check_rewrite(gpu, R.REPEAT, col, values, valid, [x % 4 for x in ln], what=f"n={n}")


# ---- the whole case list --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit_byte", [False, True])
def test_position_case_list(gpu, unit_byte):
    """every needle over the values built around it: occurrences at 0, at the end, across a 4-byte word, across byte 256; every edge of
    the start, as a column; then some starts as scalars"""
    for g, (needle, rows) in enumerate(groups(K.position_rows(unit_byte), lambda r: r[1], lambda r: (r[0], r[2]))):
        values, starts = [r[0] for r in rows], [r[1] for r in rows]
        col = pack(gpu, values, lead=LEADS[g % 3], n_buffers=2)
        exp = check_position(gpu, col, values, None, needle, starts, unit_byte, what="case list")
        assert any(exp) or not needle
    values = K.pool(b"abab")
    col = pack(gpu, values, lead=b"a", n_buffers=2)
    for needle in (b"abab", b"-", b""):
        for s in (None, 1, 2, 5, 257, 0, -1, R.INT64_MIN, R.INT64_MAX):
            check_position(gpu, col, values, None, needle, s, unit_byte, what="scalar start")


def test_split_part_case_list(gpu):
    seen = set()
    for g, (delim, rows) in enumerate(groups(K.split_rows(), lambda r: r[1], lambda r: (r[0], r[2]))):
        values, parts = [r[0] for r in rows], [r[1] for r in rows]
        col = pack(gpu, values, lead=LEADS[g % 3], n_buffers=2)
        exp = check_split(gpu, col, values, None, delim, parts, what="case list")
        seen.update(e[0] for e in exp if e[1] == 0 and e[2] == 0 and e[3] == 0)
    assert 0 in seen and any(x > 12 for x in seen)
    values = K.pool(b"aa")
    col = pack(gpu, values, lead=b"aa", n_buffers=2)
    for delim in (b"aa", b"-", b"", K.N255):
        for p in (0, 1, 2, -1, -2, 3, R.INT64_MIN, R.INT64_MAX):
            check_split(gpu, col, values, None, delim, p, what="scalar part")
    assert gpu.split_part(col, b"aa", -1).string_values() == [R.split_part(v, b"aa", -1) for v in values]


def test_rewrite_case_list(gpu):
    """replace that grows, shrinks, keeps the length and deletes; pads of one 1-byte unit, one 3-byte unit, mixed units and a stray
    continuation byte; every edge of the length and the count as a column; results of 0, 12, 13, 256 and 257 bytes from inline and long
    sources; results that are too long"""
    lens = {True: set(), False: set()}
    too_long = 0
    for g, ((op, x, y, unit_byte), rows) in enumerate(groups(K.rewrite_rows(), lambda r: (r[0], r[3], r[4], r[5]), lambda r: (r[1], r[2]))):
        values, ks = [r[0] for r in rows], [r[1] for r in rows]
        col = pack(gpu, values, lead=LEADS[g % 3], n_buffers=2)
        res = check_rewrite(gpu, op, col, values, None, ks if op in (R.LPAD, R.RPAD, R.REPEAT) else None, x, y, unit_byte, what="case list")
        for v, r in zip(values, res):
            if r == R.TOO_LONG:
                too_long += 1
            else:
                lens[len(v) <= 12].add(len(r))
    assert {0, 12, 13, 256, 257} <= lens[True] and {0, 12, 13, 256, 257} <= lens[False] and too_long >= 3


def test_scalar_length_and_count(gpu):
    values = FK.values() + K.OVERLAPS
    col = pack(gpu, values, lead=b"xy", n_buffers=2)
    for unit_byte in (False, True):
        for k in (0, 1, 5, 12, 13, 256, 257, -1, R.INT64_MIN):
            check_rewrite(gpu, R.LPAD, col, values, None, k, b"a" + S.E2, unit_byte=unit_byte, what="scalar length")
            check_rewrite(gpu, R.RPAD, col, values, None, k, b"\x80x\xbf", unit_byte=unit_byte, what="scalar length")
    for k in (0, 1, 2, -3, R.INT64_MAX):
        check_rewrite(gpu, R.REPEAT, col, values, None, k, what="scalar count")
    got = gpu.lpad(col, 20, "é")
    assert got.string_values() == [R.lpad(v, 20, S.E2) for v in values] and int(got.str_counters.to_numpy(np.uint64, 1)[0]) == 0
    assert gpu.rpad(col, 7, b"xy", unit_byte=True).string_values() == [R.rpad(v, 7, b"xy", True) for v in values]
    assert gpu.repeat(col, 2).string_values() == [v * 2 for v in values] and gpu.reverse(col).string_values() == [R.reverse(v) for v in values]
    assert gpu.replace(col, b"ab", b"").string_values() == [v.replace(b"ab", b"") for v in values]
    pos = gpu.position(col, b"ab", 2)
    assert pos.dtype == T.T_U64 and pos.to_numpy().tolist() == [R.position(v, b"ab", 2) for v in values]


# ---- neighbours, dirty views, scalar, nullable and broken columns -------------------------------------------------------------------------
def test_neighbours_in_the_buffer(gpu):
    """values packed back to back, chosen so that reading outside a value changes the answer: a value ends with the needle's first byte
    and the next one begins with the rest; a value is followed by continuation bytes that would join its last unit"""
    values = []
    for ln in (13, 14, 15, 16, 17, 300, 301):
        values += [b"x" * (ln - 1) + b"a", b"bcd" + b"y" * (ln - 4) + b"ab", b"cd" + b"z" * (ln - 3) + S.E3[:1], b"\x80\x80" + b"w" * (ln - 2), b"\xbf" * ln]
    col = pack(gpu, values, lead=b"bcd")
    for needle in (b"abcd", b"abc", b"abcdy"):
        exp = check_position(gpu, col, values, None, needle, what="neighbours")
        assert not any(exp), "no value holds the needle"
        exp = check_split(gpu, col, values, None, needle, 2, what="neighbours")
        assert all(e == S.ZERO_VIEW for e in exp)
        check_rewrite(gpu, R.REPLACE, col, values, None, None, needle, b"!", what="neighbours")
    for unit_byte in (False, True):
        check_position(gpu, col, values, None, b"", [len(v) - 1 for v in values], unit_byte, what="neighbours")
        check_position(gpu, col, values, None, S.E3[:1], 3, unit_byte, what="neighbours")
        check_rewrite(gpu, R.LPAD, col, values, None, [len(v) + 2 - (i % 5) for i, v in enumerate(values)], b"p" + S.E2, unit_byte=unit_byte, what="neighbours")
        check_rewrite(gpu, R.REVERSE, col, values, None, unit_byte=unit_byte, what="neighbours")


def test_dirty_inline_views(gpu):
    """0xFF in the bytes past every inline value: what lies there is not defined"""
    values = FK.values() + K.OVERLAPS + K.around(b"aa")[:20]
    d = dirty(gpu, pack(gpu, values, lead=b"a", n_buffers=2))
    for unit_byte in (False, True):
        check_position(gpu, d, values, None, b"aa", 2, unit_byte, what="dirty")
        check_position(gpu, d, values, None, b"", [len(v) for v in values], unit_byte, what="dirty")
        check_rewrite(gpu, R.RPAD, d, values, None, 14, b"\xffz", unit_byte=unit_byte, what="dirty")
        check_rewrite(gpu, R.REVERSE, d, values, None, unit_byte=unit_byte, what="dirty")
    check_split(gpu, d, values, None, b"a", -1, what="dirty")
    check_split(gpu, d, values, None, b"\xff", 1, what="dirty")
    check_rewrite(gpu, R.REPLACE, d, values, None, None, b"aa", b"\xff" * 5, what="dirty")
    check_rewrite(gpu, R.REPLACE, d, values, None, None, b"\xff", b"", what="dirty")
    check_rewrite(gpu, R.REPEAT, d, values, None, [i % 40 for i in range(len(values))], what="dirty")


def test_scalar_column(gpu):
    for value in (b"", b"he-llo", S.E3 * 4 + b"-x", b"ab" * 7 + S.E2 * 10 + b"-", b"x" * 300 + S.E4 * 5 + b"-ab-" + b"y" * 40):
        col = pack(gpu, [value], lead=b"\x80")
        col.is_scalar = True
        for n in (1, 64, 130):
            ks = [(i % 9) - 2 for i in range(n)]
            check_position(gpu, col, [value], None, b"-", ks, what="scalar column", n=n)
            check_split(gpu, col, [value], None, b"-", ks, what="scalar column", n=n)
            check_rewrite(gpu, R.REPEAT, col, [value], None, ks, what="scalar column", n=n)
            check_rewrite(gpu, R.LPAD, col, [value], None, [k * 40 for k in ks], b"ab", what="scalar column", n=n)
            check_rewrite(gpu, R.REPLACE, col, [value], None, None, b"-", b"", what="scalar column", n=n)
            check_rewrite(gpu, R.REVERSE, col, [value], None, what="scalar column", n=n)
    null = pack(gpu, [b"he-llo"], valid=np.array([False]))
    null.is_scalar = True
    assert run_position(gpu, null, b"-", n=70) == [0] * 70 and run_split(gpu, null, b"-", 1, n=70) == [S.ZERO_VIEW] * 70
    assert run_rewrite(gpu, R.REVERSE, null, n=70) == ([S.ZERO_VIEW] * 70, b"", 0, 0)
    space = pack(gpu, [b" "])
    space.is_scalar = True
    res = gpu.repeat(space, gpu.Column.from_numpy(np.arange(130, dtype=np.int64)))
    assert res.n == 130 and res.string_values() == [b" " * k for k in range(130)]


def test_nullable_column_with_a_validity_offset(gpu):
    rng = np.random.default_rng(5)
    pool = K.pool(b"-")
    n_all = 13 + 700 + 40
    values = [pool[k] for k in rng.integers(0, len(pool), n_all)]
    valid = rng.random(n_all) < 0.7
    whole = pack(gpu, values, valid=valid, lead=b"xyz")
    raw = whole.host_views.copy()
    raw[~valid] = [5000, 0x61616161, 77, 0xFFFFFF00]      # NULL rows are not dereferenced: their views may hold anything
    broken = gpu.Column(T.T_STRING, n_all, gpu.DeviceBuffer.from_numpy(raw), whole.validity, buffers=whole.buffers, keep=(whole,))
    broken.host_views = whole.host_views
    col = broken.slice(13, 713)
    col.host_views = whole.host_views[13:713]
    col.n_buffers = 1
    assert col.voff == 13
    v, ok = values[13:713], valid[13:713]
    for unit_byte in (False, True):
        check_position(gpu, col, v, ok, b"-", 2, unit_byte, what="nullable")
        check_rewrite(gpu, R.RPAD, col, v, ok, 15, S.E3, unit_byte=unit_byte, what="nullable")
        check_rewrite(gpu, R.REVERSE, col, v, ok, unit_byte=unit_byte, what="nullable")
    check_split(gpu, col, v, ok, b"-", -1, what="nullable")
    check_rewrite(gpu, R.REPLACE, col, v, ok, None, b"-", b"=+=", what="nullable")
    check_rewrite(gpu, R.REPEAT, col, v, ok, 2, what="nullable")
    res = gpu.split_part(col, b"-", 1)
    assert res.dtype == T.T_STRING and res.validity is col.validity and res.voff == 13 and res.n == 700 and res.buffers is col.buffers
    assert [g for g, k in zip(res.string_values(), ok) if k] == [R.split_part(x, b"-", 1) for x, k in zip(v, ok) if k]
    rep = gpu.replace(col, b"-", b"")
    assert rep.validity is col.validity and rep.voff == 13 and rep.validity_numpy().tolist() == ok.tolist()
    assert [g for g, k in zip(rep.string_values(), ok) if k] == [x.replace(b"-", b"") for x, k in zip(v, ok) if k]


def test_view_with_a_buffer_index_out_of_range(gpu):
    values = K.pool(b"aa")
    bad = {i for i in range(len(values)) if len(values[i]) > 12 and i % 3 == 0}
    assert bad
    col = pack(gpu, values, buffer_of=lambda i: 7 if i in bad else 0, lead=b"q")
    nobuf = gpu.Column(T.T_STRING, col.n, col.data, keep=(col,))      # no buffer table at all: every long view is out of range
    nobuf.host_views, nobuf.n_buffers = col.host_views, 0
    for c in (col, nobuf):
        check_position(gpu, c, values, None, b"aa", what="bad buffer index")
        check_split(gpu, c, values, None, b"aa", 2, what="bad buffer index")
        check_rewrite(gpu, R.REPLACE, c, values, None, None, b"aa", b"b", what="bad buffer index")
        check_rewrite(gpu, R.REVERSE, c, values, None, what="bad buffer index")
        check_rewrite(gpu, R.LPAD, c, values, None, 300, b"ab", what="bad buffer index")


# ---- the output buffer's end, results that are too long --------------------------------------------------------------------------------
def test_rewrite_into_a_buffer_one_byte_short(gpu):
    """out_data_bytes one less than the count call reported: exactly the last long row comes back empty, err_count is 1, nothing is
    written at or past out_data_bytes"""
    for tail in (b"y" * 20, b"y" * 150, b"y-" * 200):          # the last long row is written in the fill launch / by the wave-per-row pass
        values = [b"short", b"x-" * 20, b"", b"z" * 7, tail, b"tiny"]
        col = pack(gpu, values, lead=b"a")
        for op, k, x, y in ((R.REPEAT, 2, b"", b""), (R.REPLACE, None, b"-", b"+")):
            v, d, err, nbytes = run_rewrite(gpu, op, col, k, x, y, short_by=1)
            ev, ed, _ = expect_rewrite([R.rewrite(op, val, k or 0, x, y) for val in values])
            last = len(R.rewrite(op, tail, k or 0, x, y))
            assert nbytes == len(ed) and last > 12
            ev[4] = S.ZERO_VIEW
            assert v == ev and err == 1, (op, len(tail))
            assert d[:len(ed) - last] == ed[:len(ed) - last] and set(d[len(ed) - last:]) <= {0xFF}, "the row that does not fit writes nothing"


def test_results_that_are_too_long(gpu):
    for long_source in (False, True):
        values = [b"ab", b"x" * 400 if long_source else b"x", b"hello, world!"]
        col = pack(gpu, values, lead=b"a")
        for op, k, x in ((R.REPEAT, [1, R.INT64_MAX, 2], b""), (R.LPAD, [3, R.INT64_MAX, 14], b"ab"), (R.RPAD, [3, 1 << 32, 14], S.E3)):
            res = check_rewrite(gpu, op, col, values, None, k, x, what="too long")
            assert res[1] == R.TOO_LONG and res[0] != R.TOO_LONG and len(res[2]) > 12
    res = gpu.repeat(pack(gpu, [b"ab", b"x"]), gpu.Column.from_numpy(np.array([2, R.INT64_MAX], dtype=np.int64)))
    assert res.string_values() == [b"abab", b""] and int(res.str_counters.to_numpy(np.uint64, 1)[0]) == 1


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_usable(gpu):
    values = [b"he-llo", b"x" * 10 + b"-hello", b"", b"ab"]
    col = pack(gpu, values)
    cc = col.c()
    ints = gpu.Column.from_numpy(np.arange(4, dtype=np.int64))
    ic = ints.c()
    f64 = gpu.Column.from_numpy(np.arange(4, dtype=np.float64)).c()
    out = gpu.DeviceBuffer(256)
    L = T.lib()
    nbytes = C.c_uint64(0)
    too_many = (1 << 32) - 1

    def pos_rc(c=cc, needle=b"-", needle_len=None, start=None, flags=0, n=4, o=out.ptr):
        return L.dbhip_str_position(C.byref(c), _host(needle), C.c_int32(len(needle) if needle_len is None else needle_len), ref(col, start), C.c_int32(flags),
                                    C.c_int64(n), C.c_void_p(o), None)

    def split_rc(c=cc, delim=b"-", delim_len=None, part=ic, n=4, o=out.ptr):
        return L.dbhip_str_split_part(C.byref(c), _host(delim), C.c_int32(len(delim) if delim_len is None else delim_len), ref(col, part), C.c_int64(n), C.c_void_p(o), None)

    def rw_rc(op, c=cc, k=ic, x=b"-", x_len=None, y=b"", y_len=None, flags=0, n=4, o=out.ptr, counter=None):
        return L.dbhip_str_rewrite(C.c_int32(op), C.byref(c), ref(col, k), _host(x), C.c_int32(len(x) if x_len is None else x_len), _host(y),
                                   C.c_int32(len(y) if y_len is None else y_len), C.c_int32(flags), C.c_int64(n), C.c_void_p(o), C.c_void_p(out.ptr), C.c_uint64(0),
                                   C.c_void_p(counter), None)

    def bytes_rc(op, c=cc, k=ic, x=b"-", x_len=None, flags=0, n=4):
        return L.dbhip_str_rewrite_bytes(C.c_int32(op), C.byref(c), ref(col, k), _host(x), C.c_int32(len(x) if x_len is None else x_len), _host(b""), C.c_int32(0),
                                         C.c_int32(flags), C.c_int64(n), C.byref(nbytes), None)

    def good():
        assert run_position(gpu, col, b"l") == [4, 14, 0, 0] and [v[4:4 + v[0]] for v in run_split(gpu, col, b"-", 1)] == [b"he", b"x" * 10, b"", b"ab"]

    big = b"x" * 256
    cases = [
        (lambda: pos_rc(c=ic), T.ERR_INVALID), (lambda: split_rc(c=ic), T.ERR_INVALID), (lambda: rw_rc(R.REPLACE, c=ic), T.ERR_INVALID), (lambda: bytes_rc(R.REVERSE, c=ic), T.ERR_INVALID),
        (lambda: rw_rc(5), T.ERR_INVALID), (lambda: rw_rc(-1), T.ERR_INVALID), (lambda: bytes_rc(5), T.ERR_INVALID),
        (lambda: pos_rc(flags=2), T.ERR_INVALID), (lambda: rw_rc(R.REVERSE, flags=3), T.ERR_INVALID), (lambda: bytes_rc(R.LPAD, flags=4), T.ERR_INVALID),
        (lambda: pos_rc(needle=big), T.ERR_UNSUPPORTED), (lambda: split_rc(delim=big), T.ERR_UNSUPPORTED), (lambda: rw_rc(R.REPLACE, x=big), T.ERR_UNSUPPORTED),
        (lambda: rw_rc(R.REPLACE, y=big), T.ERR_UNSUPPORTED), (lambda: rw_rc(R.LPAD, x=big), T.ERR_UNSUPPORTED), (lambda: bytes_rc(R.RPAD, x=big), T.ERR_UNSUPPORTED),
        (lambda: pos_rc(needle_len=-1), T.ERR_INVALID), (lambda: split_rc(delim_len=-1), T.ERR_INVALID), (lambda: rw_rc(R.REPLACE, x_len=-1), T.ERR_INVALID),
        (lambda: rw_rc(R.REPLACE, y_len=-2), T.ERR_INVALID), (lambda: bytes_rc(R.LPAD, x_len=-1), T.ERR_INVALID),
        (lambda: pos_rc(n=-1), T.ERR_INVALID), (lambda: pos_rc(n=too_many), T.ERR_INVALID), (lambda: split_rc(n=-1), T.ERR_INVALID), (lambda: split_rc(n=too_many), T.ERR_INVALID),
        (lambda: rw_rc(R.REVERSE, n=-1), T.ERR_INVALID), (lambda: rw_rc(R.REVERSE, n=too_many), T.ERR_INVALID), (lambda: bytes_rc(R.REVERSE, n=-1), T.ERR_INVALID),
        (lambda: bytes_rc(R.REVERSE, n=too_many), T.ERR_INVALID),
        (lambda: rw_rc(R.LPAD, k=None), T.ERR_INVALID), (lambda: rw_rc(R.RPAD, k=f64), T.ERR_INVALID), (lambda: rw_rc(R.REPEAT, k=cc), T.ERR_INVALID),
        (lambda: bytes_rc(R.REPEAT, k=None), T.ERR_INVALID), (lambda: split_rc(part=None), T.ERR_INVALID), (lambda: split_rc(part=f64), T.ERR_INVALID), (lambda: pos_rc(start=f64), T.ERR_INVALID),
        (lambda: pos_rc(o=out.ptr + 4), T.ERR_INVALID), (lambda: split_rc(o=out.ptr + 8), T.ERR_INVALID), (lambda: rw_rc(R.REVERSE, o=out.ptr + 8), T.ERR_INVALID),
        (lambda: rw_rc(R.REVERSE, counter=out.ptr + 4), T.ERR_INVALID),
    ]
    for k, (call, code) in enumerate(cases):
        assert call() == code, k
        assert b"DBHIP_STR" not in L.dbhip_last_error()
        good()
    assert pos_rc(n=0) == T.OK and split_rc(n=0) == T.OK and rw_rc(R.REPLACE, n=0) == T.OK and bytes_rc(R.REPLACE, n=0) == T.OK and nbytes.value == 0
    # an argument an op ignores is not looked at
    assert rw_rc(R.REVERSE, k=None, x=big, n=0) == T.OK and rw_rc(R.REPEAT, x_len=-1, n=0) == T.OK
    with pytest.raises(T.DbhipError) as e:
        gpu.replace(col, big, b"")
    assert e.value.code == T.ERR_UNSUPPORTED
    good()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_split_part_as_the_string_key_of_a_group_by(gpu):
    """split_part(phone, '-', 1) as a GROUP BY key with count(*): the canonical inline result is the key, without a copy; and
    replace(phone, '-', '') fed to dbhip_str_length"""
    rng = np.random.default_rng(28)
    phones = [b"%02d-%03d-%03d-%04d" % (int(c), int(x), int(y), int(z)) for c, x, y, z in zip(rng.integers(10, 35, 1000), rng.integers(100, 1000, 1000),
                                                                                             rng.integers(100, 1000, 1000), rng.integers(1000, 10000, 1000))]
    col = pack(gpu, phones, lead=b"7")
    key = gpu.split_part(col, "-", 1)
    g = gpu.GroupBy([T.T_STRING], [(T.AGG_COUNT, 0, 0, 0, 0)])
    g.add_block([key], [None], len(phones))
    got = sorted(g.result())
    g.destroy()
    assert got == sorted(Counter(R.split_part(p, b"-", 1) for p in phones).items()) and len(got) == 25
    digits = gpu.replace(col, "-", "")
    assert gpu.str_length(digits).to_numpy().tolist() == [len(R.replace(p, b"-", b"")) for p in phones] == [12] * 1000
    assert gpu.str_length(gpu.replace(col, "-", "--")).to_numpy().tolist() == [18] * 1000
