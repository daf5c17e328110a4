"""GPU: dbhip_str_length / dbhip_str_slice / dbhip_str_build_bytes / dbhip_str_build (include/dbhip.h a22), every row asserted exactly
against tests/str_ref.py (plain Python, held to Python's own operations and to negative controls by tests/test_str_ref_cpu.py): the
full 16 bytes of every result view, and the bytes of every built value. Nothing is sampled. Columns are packed here, not by
Column.strings: the long values lie back to back in their data buffers without padding, behind a lead of 1 to 3 bytes, so every
alignment occurs and a kernel that reads outside a value reads its neighbours' bytes. Every output is pre-filled with 0xFF and has guard
bytes behind it that must stay 0xFF."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import str_ref as R
from tests import strfn_cases as K

pytestmark = pytest.mark.gpu

GUARD = 64
LONG = T.LIKE_LONG_BYTES


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def pack(gpu, values, valid=None, lead=b"", n_buffers=1, buffer_of=None):
    """a String column whose long values (> 12 bytes) are packed back to back, behind `lead`, in n_buffers data buffers (long row k goes
    to buffer k % n_buffers unless buffer_of(row) says otherwise — it may name a buffer the column does not have); no byte follows the
    last value of a buffer (tests/test_gpu_like.py's helper)"""
    n = len(values)
    lens = np.array([len(v) for v in values], dtype=np.uint32)
    views = np.zeros((n, 4), dtype=np.uint32)
    views[:, 0] = lens
    if n:
        inl = b"".join(v.ljust(12, b"\0") if len(v) <= 12 else v[:4].ljust(12, b"\0") for v in values)
        views[:, 1:4] = np.frombuffer(inl, dtype=np.uint32).reshape(n, 3)
    parts = [[lead] for _ in range(n_buffers)]
    sizes = [len(lead)] * n_buffers
    k = 0
    for i in np.nonzero(lens > 12)[0]:
        b = k % n_buffers if buffer_of is None else buffer_of(int(i))
        k += 1
        views[i, 2] = b
        if b < n_buffers:
            views[i, 3] = sizes[b]
            parts[b].append(values[i])
            sizes[b] += len(values[i])
        else:
            views[i, 3] = 0
    bufs = [gpu.DeviceBuffer.from_numpy(np.frombuffer(b"".join(p), dtype=np.uint8)) for p in parts]
    for b, size in zip(bufs, sizes):
        assert b.nbytes == size                      # the last value ends where the buffer ends
    ptrs = gpu.DeviceBuffer.from_numpy(np.array([b.ptr for b in bufs], dtype=np.uint64))
    vb = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(valid)) if valid is not None else None
    col = gpu.Column(T.T_STRING, n, gpu.DeviceBuffer.from_numpy(views), vb, buffers=ptrs, keep=tuple(bufs))
    col.n_buffers = n_buffers
    col.host_views = views
    return col


def dirty(gpu, col):
    """the same column with 0xFF in the bytes past every inline value: what lies there is not defined"""
    raw = col.host_views.copy().view(np.uint8).reshape(-1, 16)
    for r in raw:
        ln = int(r[:4].view(np.uint32)[0])
        if ln <= 12:
            r[4 + ln:] = 0xFF
    d = gpu.Column(T.T_STRING, col.n, gpu.DeviceBuffer.from_numpy(raw), col.validity, buffers=col.buffers, keep=(col,))
    d.n_buffers, d.host_views = col.n_buffers, col.host_views
    return d


def guarded(gpu, nbytes):
    return gpu.DeviceBuffer.from_numpy(np.full(nbytes + GUARD, 0xFF, dtype=np.uint8))


def read_guarded(buf, nbytes, what):
    raw = buf.to_numpy(np.uint8, nbytes + GUARD)
    assert (raw[nbytes:] == 0xFF).all(), f"{what}: wrote past its end"
    return raw[:nbytes]


def i64(gpu, x, n):
    """None / an int (a scalar column) / a list (a column)"""
    if x is None:
        return None
    if isinstance(x, int):
        return gpu.Column.scalar(x, T.T_I64)
    assert len(x) == n
    return gpu.Column.from_numpy(np.array(x, dtype=np.int64))


def _host(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")


def run_slice(gpu, op, col, a=None, b=None, pad=b"", unit_byte=False, n=None):
    n = col.n if n is None else n
    out = guarded(gpu, n * 16)
    cc = col.c()
    ca, cb = i64(gpu, a, n), i64(gpu, b, n)
    cca, ccb = (ca.c() if ca else None), (cb.c() if cb else None)
    T.check(T.lib().dbhip_str_slice(C.c_int32(op), C.byref(cc), C.byref(cca) if ca else None, C.byref(ccb) if cb else None, _host(pad), C.c_int32(len(pad)),
                                    C.c_int32(T.STR_UNIT_BYTE if unit_byte else 0), C.c_int64(n), C.c_void_p(out.ptr), None))
    return [bytes(r) for r in read_guarded(out, n * 16, "out_views").reshape(-1, 16)]


def run_length(gpu, col, unit_byte=False, n=None):
    n = col.n if n is None else n
    out = guarded(gpu, n * 8)
    cc = col.c()
    T.check(T.lib().dbhip_str_length(C.byref(cc), C.c_int32(T.STR_UNIT_BYTE if unit_byte else 0), C.c_int64(n), C.c_void_p(out.ptr), None))
    return read_guarded(out, n * 8, "out").view(np.uint64).tolist()


def usable(col, i, valid=None):
    """is row i neither NULL nor a long view that names a buffer the column does not have"""
    if valid is not None and not valid[i]:
        return False
    ln, _, idx, _ = (int(x) for x in col.host_views[i])
    return ln <= 12 or idx < col.n_buffers


def expect_slices(col, values, valid, op, a=None, b=None, pad=b"", unit_byte=False, n=None):
    n = col.n if n is None else n
    out = []
    for i in range(n):
        r = 0 if col.is_scalar else i
        if not usable(col, r, valid):
            out.append(R.ZERO_VIEW)
            continue
        ai = a if a is None or isinstance(a, int) else a[i]
        bi = b if b is None or isinstance(b, int) else b[i]
        _, _, idx, off = (int(x) for x in col.host_views[r])
        out.append(R.slice_view(values[r], R.slice_range(op, values[r], ai, bi, pad, unit_byte), idx, off))
    return out


def assert_views(got, exp, what, describe=lambda i: ""):
    if got != exp:
        bad = [i for i in range(len(exp)) if got[i] != exp[i]]
        raise AssertionError(f"{what}: {len(bad)} of {len(exp)} rows differ, first row {bad[0]} {describe(bad[0])} got {got[bad[0]].hex()} expected {exp[bad[0]].hex()}")


def check_slice(gpu, col, values, valid, op, a=None, b=None, pad=b"", unit_byte=False, what="", n=None):
    got = run_slice(gpu, op, col, a, b, pad, unit_byte, n)
    exp = expect_slices(col, values, valid, op, a, b, pad, unit_byte, n)
    assert_views(got, exp, f"{what} op {op} unit_byte {unit_byte} pad {pad[:16]!r}",
                 lambda i: f"value {values[0 if col.is_scalar else i][:60]!r} (len {len(values[0 if col.is_scalar else i])}) a {a if a is None or isinstance(a, int) else a[i]} "
                           f"b {b if b is None or isinstance(b, int) else b[i]}")
    return exp


def run_build(gpu, op, cols, n, short_by=0, nargs=None):
    """the count call, then the build call into a buffer of exactly that size (less short_by) -> (views, data bytes, live bits, err, non_ascii)"""
    arr = (T.Col * len(cols))(*[c.c() for c in cols])
    nargs = len(cols) if nargs is None else nargs
    nbytes = C.c_uint64(0xDEADBEEF)
    T.check(T.lib().dbhip_str_build_bytes(C.c_int32(op), arr, C.c_int32(nargs), C.c_int64(n), C.byref(nbytes), None))
    size = nbytes.value - short_by
    views, data, bits = guarded(gpu, n * 16), guarded(gpu, size), guarded(gpu, ((n + 63) // 64) * 8)
    counters = gpu.DeviceBuffer.from_numpy(np.array([0, 5], dtype=np.uint64))
    T.check(T.lib().dbhip_str_build(C.c_int32(op), arr, C.c_int32(nargs), C.c_int64(n), C.c_void_p(views.ptr), C.c_void_p(data.ptr), C.c_uint64(size),
                                    C.c_void_p(bits.ptr), C.c_void_p(counters.ptr), C.c_void_p(counters.ptr + 8), None))
    v = [bytes(r) for r in read_guarded(views, n * 16, "out_views").reshape(-1, 16)]
    d = read_guarded(data, size, "out_data").tobytes()
    words = read_guarded(bits, ((n + 63) // 64) * 8, "out_validity")
    live = np.unpackbits(words, bitorder="little")
    assert not live[n:].any(), "validity bits past n"
    err, high = (int(x) for x in counters.to_numpy(np.uint64, 2))
    return v, d, live[:n].astype(bool).tolist(), err, high - 5, nbytes.value


def expect_build(op, rows):
    """rows: per row the list of argument values (None: NULL) -> (views, data, live, non_ascii rows)"""
    views, data, live, high = [], b"", [], 0
    for args in rows:
        v = R.build(op, args)
        live.append(v is not None)
        if v is None:
            views.append(R.ZERO_VIEW)
            continue
        high += int(R.non_ascii(args))
        views.append(R.view(v, 0, len(data)))
        if len(v) > 12:
            data += v
    return views, data, live, high


def check_build(gpu, op, cols, rows, what):
    n = len(rows)
    v, d, live, err, high, nbytes = run_build(gpu, op, cols, n)
    ev, ed, elive, ehigh = expect_build(op, rows)
    assert nbytes == len(ed), (what, nbytes, len(ed))
    assert live == elive, what
    assert_views(v, ev, what, lambda i: f"args {[a if a is None else a[:30] for a in rows[i]]}")
    assert d == ed and err == 0 and high == ehigh, (what, err, high, ehigh)


# ---- row counts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_row_counts(gpu, n):
    """the last partial wave, the ballot words of the live bits, more than one workgroup; every entry point"""
    rng = np.random.default_rng(n)
    pool = K.values()
    values = [pool[k] for k in rng.integers(0, len(pool), n)]
    valid = rng.random(n) < 0.8
    col = pack(gpu, values, valid=valid, lead=b"\x80", n_buffers=2)
    pos = [int(x) for x in rng.integers(-6, 7, n)]
    ln = [int(x) for x in rng.integers(-1, 15, n)]
    for unit_byte in (False, True):
        check_slice(gpu, col, values, valid, R.SUBSTR, pos, ln, unit_byte=unit_byte, what=f"n={n}")
        check_slice(gpu, col, values, valid, R.RIGHT, ln, unit_byte=unit_byte, what=f"n={n}")
        assert run_length(gpu, col, unit_byte) == [R.length(v, unit_byte) if ok else 0 for v, ok in zip(values, valid)]
    check_slice(gpu, col, values, valid, R.TRIM_BOTH, pad=b"ab", what=f"n={n}")
    dash = pack(gpu, [b"-"])
    dash.is_scalar = True
    rows = [[v if ok else None, b"-", v if ok else None] for v, ok in zip(values, valid)]
    check_build(gpu, R.CONCAT, [col, dash, col], rows, f"concat n={n}")
    check_build(gpu, R.UPPER, [col], [[v if ok else None] for v, ok in zip(values, valid)], f"upper n={n}")


# ---- substr / left / right: the whole case list ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit_byte", [False, True])
def test_substr_left_right_case_list(gpu, unit_byte):
    """every value of the case list with every position / length / count of it, as columns: 0, +-1, +-(U - 1), +-U, +-(U + 1), the i64
    extremes, len <= 0, results of 12 and of 13 bytes from inline and from long sources, values up to 1000 bytes (the wave-per-row pass)"""
    groups = {}
    for v in K.values():
        for op, a, b in K.slice_args(v, unit_byte):
            g = groups.setdefault((op, b is None), ([], [], []))
            g[0].append(v)
            g[1].append(a)
            g[2].append(b)
    seen = set()
    for k, ((op, no_b), (values, a, b)) in enumerate(sorted(groups.items())):
        col = pack(gpu, values, lead=b"\xbf\x80\x80"[:1 + k % 3], n_buffers=2)
        exp = check_slice(gpu, col, values, None, op, a, None if no_b else b, unit_byte=unit_byte, what="case list")
        seen.update(e[0] for e in exp if e[1] == 0 and e[2] == 0 and e[3] == 0)
    assert {0, 12, 13} <= seen


def test_scalar_position_and_length(gpu):
    values = K.values()
    col = pack(gpu, values, lead=b"ab", n_buffers=2)
    d = dirty(gpu, col)
    for unit_byte in (False, True):
        for a, b in [(1, 2), (-4, None), (2, 12), (3, 13), (0, 5), (1, 0), (R.INT64_MIN, 1), (R.INT64_MAX, None), (-1, R.INT64_MAX), (1, R.INT64_MIN), (200, 100), (-300, 290)]:
            for c in (col, d):
                check_slice(gpu, c, values, None, R.SUBSTR, a, b, unit_byte=unit_byte, what="scalar args")
        for k in (0, 1, 12, 13, 255, 256, R.INT64_MAX, -1):
            check_slice(gpu, col, values, None, R.LEFT, k, unit_byte=unit_byte, what="left")
            check_slice(gpu, d, values, None, R.RIGHT, k, unit_byte=unit_byte, what="right")
    # a scalar position with a length column
    ln = [(i * 7) % 19 - 2 for i in range(len(values))]
    check_slice(gpu, col, values, None, R.SUBSTR, 2, ln, what="scalar pos, length column")


def test_lengths(gpu):
    values = K.values()
    for lead in (b"", b"\x80", b"\x80\x80", b"\xbf\xbf\xbf"):
        col = pack(gpu, values, lead=lead, n_buffers=2)
        assert run_length(gpu, col) == [R.length(v) for v in values]
        assert run_length(gpu, dirty(gpu, col), True) == [len(v) for v in values]
    res = gpu.str_length(col)
    assert res.dtype == T.T_U64 and res.to_numpy().tolist() == [R.length(v) for v in values]


# ---- trims ---------------------------------------------------------------------------------------------------------------------------
def test_trims(gpu):
    """pads of 1, 2 and 13 bytes, the empty pad, pads longer than the value (255 bytes), values made only of pad, every length"""
    values = K.values() + [b"ababxab", b"aba", b"aaa", b" " * 300 + b"x" + b" " * 300, b"ab" * 200, b" " * 257, b"abcdefghijklm" * 30 + b"abc"]
    cols = [pack(gpu, values, lead=b"a b"[:k], n_buffers=2) for k in (1, 2, 3)]
    empty = 0
    for k, pad in enumerate(K.PADS + [b"aa", b"a"]):
        for op in (R.TRIM_LEADING, R.TRIM_TRAILING, R.TRIM_BOTH):
            exp = check_slice(gpu, cols[k % 3], values, None, op, pad=pad, what="trim")
            empty += sum(e == R.ZERO_VIEW and len(v) > 0 for e, v in zip(exp, values))
    assert empty > 10
    got = gpu.trim(cols[0], b"ab").string_values()
    assert got[len(K.values()):len(K.values()) + 2] == [b"x", b"a"] and gpu.trim(cols[0], b"aa").string_values()[len(K.values()) + 2] == b"a"


def test_neighbours_in_the_buffer(gpu):
    """values packed back to back, chosen so that reading outside a value changes the answer: a value ends with the pad's first byte and
    the next one begins with its second; a value is followed (and preceded) by continuation bytes that would join its last unit"""
    values = []
    for ln in (13, 14, 15, 16, 17, 300, 301):
        values += [b"b" + b"x" * (ln - 2) + b"a", b"b" + b"y" * (ln - 2) + b"a", b"\x80" * ln, b"z" * (ln - 1) + b"\xe2", b"\x80\x80" + b"w" * (ln - 2)]
    col = pack(gpu, values, lead=b"a")
    for op in (R.TRIM_LEADING, R.TRIM_TRAILING, R.TRIM_BOTH):
        exp = check_slice(gpu, col, values, None, op, pad=b"ab", what="neighbours")
        assert all(e[:4] == struct_len(v) for e, v in zip(exp, values)), "no row holds a whole pad at either end"
    assert run_length(gpu, col) == [R.length(v) for v in values]
    for a, b in [(-1, None), (-2, 1), (2, None), (1, 1)]:
        check_slice(gpu, col, values, None, R.SUBSTR, a, b, what="neighbours")
    check_slice(gpu, col, values, None, R.RIGHT, 1, what="neighbours")


def struct_len(v):
    return len(v).to_bytes(4, "little")


# ---- nullable, scalar and broken columns -----------------------------------------------------------------------------------------------
def test_nullable_column_with_a_validity_offset(gpu):
    rng = np.random.default_rng(5)
    pool = K.values()
    n_all = 13 + 700 + 40
    values = [pool[k] for k in rng.integers(0, len(pool), n_all)]
    valid = rng.random(n_all) < 0.7
    whole = pack(gpu, values, valid=valid, lead=b"xyz")
    # NULL rows are not dereferenced: their views may hold anything
    raw = whole.host_views.copy()
    raw[~valid] = [5000, 0x61616161, 77, 0xFFFFFF00]
    broken = gpu.Column(T.T_STRING, n_all, gpu.DeviceBuffer.from_numpy(raw), whole.validity, buffers=whole.buffers, keep=(whole,))
    broken.host_views = whole.host_views
    col = broken.slice(13, 713)
    col.host_views = whole.host_views[13:713]
    assert col.voff == 13
    v, ok = values[13:713], valid[13:713]
    for unit_byte in (False, True):
        check_slice(gpu, col, v, ok, R.SUBSTR, -3, 2, unit_byte=unit_byte, what="nullable")
        assert run_length(gpu, col, unit_byte) == [R.length(x, unit_byte) if k else 0 for x, k in zip(v, ok)]
    check_slice(gpu, col, v, ok, R.TRIM_BOTH, pad=b" ", what="nullable")
    res = gpu.substr(col, 2, 13)
    assert res.dtype == T.T_STRING and res.validity is col.validity and res.voff == 13 and res.n == 700 and res.buffers is col.buffers
    got = res.string_values()
    assert [g for g, k in zip(got, ok) if k] == [R.substr(x, 2, 13) for x, k in zip(v, ok) if k] and res.validity_numpy().tolist() == ok.tolist()
    rows = [[x if k else None, b"|"] for x, k in zip(v, ok)]
    bar = pack(gpu, [b"|"])
    bar.is_scalar = True
    check_build(gpu, R.CONCAT, [col, bar], rows, "nullable concat")
    cat = gpu.concat(col, b"|")
    assert cat.validity_numpy().tolist() == ok.tolist() and [g for g, k in zip(cat.string_values(), ok) if k] == [x + b"|" for x, k in zip(v, ok) if k]
    assert cat.to_strings() == cat.string_values()


def test_scalar_column(gpu):
    for value in (b"", b"hello", R.E3 * 4 + b"x", b"ab" * 7 + R.E2 * 10, b"x" * 300 + R.E4 * 5 + b"  "):
        col = pack(gpu, [value], lead=b"\x80")
        col.is_scalar = True
        for n in (1, 64, 130):
            pos = [(i % 9) - 4 for i in range(n)]
            check_slice(gpu, col, [value], None, R.SUBSTR, pos, 3, what="scalar column", n=n)
            check_slice(gpu, col, [value], None, R.TRIM_TRAILING, pad=b" ", what="scalar column", n=n)
            assert run_length(gpu, col, n=n) == [R.length(value)] * n
        rows = [[value, b"-", value]] * 70
        dash = pack(gpu, [b"-"])
        dash.is_scalar = True
        check_build(gpu, R.CONCAT, [col, dash, col], rows, "all scalar")
    null = pack(gpu, [b"hello"], valid=np.array([False]))
    null.is_scalar = True
    assert run_slice(gpu, R.LEFT, null, 2, n=70) == [R.ZERO_VIEW] * 70 and run_length(gpu, null, n=70) == [0] * 70
    res = gpu.left(col, 2, n=130)
    assert res.n == 130 and res.string_values() == [b"xx"] * 130


def test_view_with_a_buffer_index_out_of_range(gpu):
    values = K.values()
    bad = {i for i in range(len(values)) if len(values[i]) > 12 and i % 3 == 0}
    assert bad
    col = pack(gpu, values, buffer_of=lambda i: 7 if i in bad else 0, lead=b"q")
    for unit_byte in (False, True):
        check_slice(gpu, col, values, None, R.SUBSTR, 2, 20, unit_byte=unit_byte, what="bad buffer index")
        assert run_length(gpu, col, unit_byte) == [R.length(v, unit_byte) if usable(col, i) else 0 for i, v in enumerate(values)]
    check_slice(gpu, col, values, None, R.TRIM_LEADING, pad=b"ab", what="bad buffer index")
    nobuf = gpu.Column(T.T_STRING, col.n, col.data, keep=(col,))      # no buffer table at all: every long view is out of range
    nobuf.host_views = col.host_views
    check_slice(gpu, nobuf, values, None, R.RIGHT, 3, what="no buffers")
    # a build row with such an argument is the empty view, and live
    v, d, live, err, high, nbytes = run_build(gpu, R.UPPER, [col], col.n)
    exp_rows = [[x if usable(col, i) else b""] for i, x in enumerate(values)]
    ev, ed, _, _ = expect_build(R.UPPER, exp_rows)
    assert v == ev and d == ed and all(live) and err == 0 and nbytes == len(ed)


# ---- builds --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nargs", [1, 2, 8])
def test_concat(gpu, nargs):
    """1, 2 and 8 arguments, columns mixed with constants; totals of 0, 12, 13, 256 and 257 bytes; one argument NULL in some rows"""
    rows = [args for op, args in K.build_rows() if op == R.CONCAT and len(args) == nargs]
    assert rows
    fixed = len(rows)
    vals = K.values()
    rows += [[vals[(7 * i + 3 * k) % len(vals)][:400] if k % 3 != 1 else b"::" for k in range(nargs)] for i in range(150)]
    nulls = np.array([i >= fixed and i % 5 == 2 for i in range(len(rows))])
    cols = []
    for k in range(nargs):
        column = [r[k] for r in rows]
        if len(set(column)) == 1 and k % 3 == 1:                   # a constant: a scalar column
            c = pack(gpu, column[:1], lead=b"\x80")
            c.is_scalar = True
        elif k == nargs - 1:                                       # the last argument is nullable, behind a bit offset
            c = pack(gpu, [b"skipped"] * 3 + column, valid=np.concatenate([[True] * 3, ~nulls]), lead=b"ab", n_buffers=2).slice(3, 3 + len(rows))
        else:
            c = pack(gpu, column, lead=b"abc"[:1 + k % 3])
        cols.append(c)
    exp_rows = [[None if (k == nargs - 1 and nulls[i]) else r[k] for k in range(nargs)] for i, r in enumerate(rows)]
    totals = {len(b"".join(r)) for r, dead in zip(rows, nulls) if not dead}
    if nargs == 2:
        assert {0, 12, 13, 256, 257} <= totals
    check_build(gpu, R.CONCAT, cols, exp_rows, f"concat of {nargs}")


def test_build_into_a_buffer_one_byte_short(gpu):
    """out_data_bytes one less than the count call reported: exactly the last long row comes back empty, err_count is 1, nothing is
    written at or past out_data_bytes"""
    for tail in (b"y" * 20, b"y" * 300):          # the last long row is copied by a lane / by a wave
        values = [b"short", b"x" * 40, b"", b"z" * 13, tail, b"tiny"]
        col = pack(gpu, values, lead=b"a")
        v, d, live, err, high, nbytes = run_build(gpu, R.CONCAT, [col, col], len(values), short_by=1)
        ev, ed, _, _ = expect_build(R.CONCAT, [[x, x] for x in values])
        assert nbytes == len(ed) == 80 + 26 + 2 * len(tail)
        ev[4] = R.ZERO_VIEW
        assert v == ev and err == 1 and all(live)
        assert d[:80 + 26] == ed[:80 + 26] and set(d[80 + 26:]) <= {0xFF}, "the row that does not fit writes nothing"


@pytest.mark.parametrize("op", [R.UPPER, R.LOWER])
def test_upper_and_lower(gpu, op):
    rows = [args for o, args in K.build_rows() if o == op] + [[v] for v in K.values()]
    col = pack(gpu, [r[0] for r in rows], lead=b"Ab", n_buffers=2)
    check_build(gpu, op, [dirty(gpu, col)], rows, "case mapping")
    assert sum(R.non_ascii(r) for r in rows) > 10
    res = (gpu.upper if op == R.UPPER else gpu.lower)(col)
    assert res.string_values() == [R.build(op, r) for r in rows]
    assert int(res.str_counters.to_numpy(np.uint64, 2)[1]) == sum(R.non_ascii(r) for r in rows)
    ascii_only = pack(gpu, [b"@AZ[`az{", b"plain ascii " * 30])
    assert run_build(gpu, op, [ascii_only], 2)[4] == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_usable(gpu):
    values = [b"hello", b"x" * 20 + b"hello", b"", b"ab"]
    col = pack(gpu, values)
    cc = col.c()
    ints = gpu.Column.from_numpy(np.arange(4, dtype=np.int64))
    ic = ints.c()
    out = gpu.DeviceBuffer(256)
    L = T.lib()
    one = gpu.Column.scalar(1, T.T_I64).c()
    nbytes = C.c_uint64(0)
    args9 = (T.Col * 9)(*[cc] * 9)

    def slice_rc(op, c, a=one, pad=b"", pad_len=None, flags=0, n=4):
        return L.dbhip_str_slice(C.c_int32(op), C.byref(c), C.byref(a) if a is not None else None, None, _host(pad), C.c_int32(len(pad) if pad_len is None else pad_len),
                                 C.c_int32(flags), C.c_int64(n), C.c_void_p(out.ptr), None)

    def build_rc(op, nargs, n=4, arr=args9):
        return L.dbhip_str_build(C.c_int32(op), arr, C.c_int32(nargs), C.c_int64(n), C.c_void_p(out.ptr), C.c_void_p(out.ptr), C.c_uint64(0), None, None, None, None)

    def bytes_rc(op, nargs, n=4, arr=args9):
        return L.dbhip_str_build_bytes(C.c_int32(op), arr, C.c_int32(nargs), C.c_int64(n), C.byref(nbytes), None)

    def good():
        assert [v[4:4 + v[0]] for v in run_slice(gpu, R.LEFT, col, 2)] == [b"he", b"xx", b"", b"ab"]

    too_many = (1 << 32) - 1
    cases = [
        (lambda: slice_rc(R.SUBSTR, ic), T.ERR_INVALID), (lambda: slice_rc(6, cc), T.ERR_INVALID), (lambda: slice_rc(-1, cc), T.ERR_INVALID),
        (lambda: slice_rc(R.TRIM_BOTH, cc, pad=b"x" * 256), T.ERR_UNSUPPORTED), (lambda: slice_rc(R.TRIM_BOTH, cc, pad=b"x", pad_len=-1), T.ERR_INVALID),
        (lambda: slice_rc(R.LEFT, cc, n=too_many), T.ERR_INVALID), (lambda: slice_rc(R.LEFT, cc, n=-1), T.ERR_INVALID), (lambda: slice_rc(R.LEFT, cc, flags=2), T.ERR_INVALID),
        (lambda: slice_rc(R.LEFT, cc, a=cc), T.ERR_INVALID), (lambda: slice_rc(R.LEFT, cc, a=None), T.ERR_INVALID),
        (lambda: L.dbhip_str_length(C.byref(ic), C.c_int32(0), C.c_int64(4), C.c_void_p(out.ptr), None), T.ERR_INVALID),
        (lambda: L.dbhip_str_length(C.byref(cc), C.c_int32(0), C.c_int64(too_many), C.c_void_p(out.ptr), None), T.ERR_INVALID),
        (lambda: L.dbhip_str_length(C.byref(cc), C.c_int32(4), C.c_int64(4), C.c_void_p(out.ptr), None), T.ERR_INVALID),
        (lambda: build_rc(R.CONCAT, 0), T.ERR_INVALID), (lambda: build_rc(R.CONCAT, 9), T.ERR_INVALID), (lambda: build_rc(R.UPPER, 2), T.ERR_INVALID),
        (lambda: build_rc(3, 1), T.ERR_INVALID), (lambda: build_rc(R.CONCAT, 1, n=too_many), T.ERR_INVALID), (lambda: build_rc(R.CONCAT, 2, arr=(T.Col * 2)(cc, ic)), T.ERR_INVALID),
        (lambda: bytes_rc(R.CONCAT, 0), T.ERR_INVALID), (lambda: bytes_rc(R.CONCAT, 9), T.ERR_INVALID), (lambda: bytes_rc(R.LOWER, 2), T.ERR_INVALID),
        (lambda: bytes_rc(R.CONCAT, 1, n=too_many), T.ERR_INVALID), (lambda: bytes_rc(R.CONCAT, 1, arr=(T.Col * 1)(ic)), T.ERR_INVALID),
    ]
    for k, (call, code) in enumerate(cases):
        assert call() == code, k
        assert b"DBHIP_STR" not in L.dbhip_last_error()
        good()
    assert slice_rc(R.LEFT, cc, n=0) == T.OK and build_rc(R.CONCAT, 2, n=0) == T.OK and bytes_rc(R.CONCAT, 2, n=0) == T.OK and nbytes.value == 0
    assert L.dbhip_str_length(C.byref(cc), C.c_int32(0), C.c_int64(0), C.c_void_p(out.ptr), None) == T.OK
    with pytest.raises(T.DbhipError) as e:
        gpu.trim(col, b"x" * 256)
    assert e.value.code == T.ERR_UNSUPPORTED
    good()


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_substr_as_the_string_key_of_a_group_by(gpu):
    """TPC-H Q22's substring(c_phone from 1 for 2) as a GROUP BY key with count(*): the canonical inline result is the key, without a copy"""
    rng = np.random.default_rng(22)
    phones = [b"%02d-%03d-%03d-%04d" % (int(c), int(x), int(y), int(z)) for c, x, y, z in zip(rng.integers(10, 35, 1000), rng.integers(100, 1000, 1000),
                                                                                             rng.integers(100, 1000, 1000), rng.integers(1000, 10000, 1000))]
    col = pack(gpu, phones, lead=b"7")
    key = gpu.substr(col, 1, 2)
    g = gpu.GroupBy([T.T_STRING], [(T.AGG_COUNT, 0, 0, 0, 0)])
    g.add_block([key], [None], len(phones))
    got = sorted(g.result())
    g.destroy()
    assert got == sorted(Counter(p[:2] for p in phones).items()) and len(got) == 25
