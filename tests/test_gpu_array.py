"""GPU: dbhip_array_length / _get / _find / _find_str / _reduce_result / _reduce / _unnest_sel (include/dbhip.h a29), every row asserted
against tests/array_ref.py (plain Python, held to Python's own operations and to negative controls by tests/test_array_ref_cpu.py) over
the case list the host checker runs (tests/array_cases.py). Nothing is sampled. Every output is pre-filled with 0xFF and has guard
bytes behind it that must stay 0xFF. Floats: MIN, MAX and find are compared with float_ref.same_value / of_cmp, SUM with
float_ref.sum_ok, the any-order bound gamma(n - 1) * sum|x|."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import array_cases as K
from tests import array_ref as R
from tests import float_ref as F
from tests.test_gpu_strfn import _host, dirty, guarded, pack, read_guarded

pytestmark = pytest.mark.gpu

FULL = ("i64", "f32", "u8", "dec128")        # every shape; the other types share these kernels and run the edge lengths
assert (T.ARRAY_LONG_LEN, T.ARRAY_STAGE_BYTES, T.ARRAY_MAX_NEEDLE) == (K.T, K.STAGE_BYTES, 255)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
class Arr:
    """a device Array column built from rows: `first` filler elements lie in front of the first run (offsets[0] = first) and `tail`
    behind the last; the child's validity Bitmap starts at bit `voff`; under every NULL element lies a value of the pool"""

    def __init__(self, gpu, tname, rows, first=0, voff=0, tail=0, seed=1, strings=None):
        rng = np.random.default_rng(seed)
        self.tname, self.rows, self.n = tname, rows, len(rows)
        self.off = K.offsets_of(rows, first)
        elems = K.values(tname, rng, first) + K.flat(rows) + K.values(tname, rng, tail)
        valid = [e is not None for e in elems]
        under = K.values(tname, rng, len(elems))
        stored = [e if e is not None else u for e, u in zip(elems, under)]
        self.stored, self.n_elems = stored, len(elems)
        bits = None if all(valid) and not voff else [bool(x) for x in rng.integers(0, 2, voff)] + valid
        if tname == "string":
            self.child = strings(stored) if strings else pack(gpu, stored, lead=b"\x80")
            self.child.validity = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(bits)) if bits is not None else None
        else:
            raw = np.frombuffer(b"".join(K.encode(tname, e) for e in stored) + bytes(16), dtype=np.uint8)
            vb = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(bits)) if bits is not None else None
            self.child = gpu.Column(K.TYPES[tname][0], len(elems), gpu.DeviceBuffer.from_numpy(raw), vb, 20 if tname == "dec128" else (10 if tname == "dec64" else 0), 3 if tname.startswith("dec") else 0)
        self.child.voff = voff
        self.offsets = gpu.DeviceBuffer.from_numpy(np.array(self.off, dtype=np.uint64))

    def args(self):
        self.cc = self.child.c()
        return C.byref(self.cc), C.c_void_p(self.offsets.ptr), C.c_int64(self.n), C.c_uint64(self.n_elems)


def words(n):
    return ((n + 63) // 64) * 8


def bits_of(raw, n):
    return np.unpackbits(np.asarray(raw, dtype=np.uint8), bitorder="little")[:n].astype(bool).tolist()


def whole_words(raw, n):
    """the Bitmap's bits past n, inside its last word, are written as zero"""
    return not np.unpackbits(np.asarray(raw, dtype=np.uint8), bitorder="little")[n:].any()


def run_length(gpu, a):
    out, bad = guarded(gpu, a.n * 8), gpu.DeviceBuffer.from_numpy(np.zeros(1, np.uint64))
    T.check(T.lib().dbhip_array_length(C.c_void_p(a.offsets.ptr), C.c_int64(a.n), C.c_uint64(a.n_elems), C.c_void_p(out.ptr), C.c_void_p(bad.ptr), None))
    return read_guarded(out, a.n * 8, "out").view(np.uint64).tolist(), int(bad.to_numpy(np.uint64, 1)[0])


def run_get(gpu, a, index):
    es = K.TYPES[a.tname][2]
    out, vb = guarded(gpu, a.n * es), guarded(gpu, words(a.n))
    ci = gpu.Column.scalar(index, T.T_I64) if isinstance(index, int) else gpu.Column.from_numpy(np.array(index, dtype=np.int64))
    cci = ci.c()
    T.check(T.lib().dbhip_array_get(*a.args(), C.byref(cci), C.c_void_p(out.ptr), C.c_void_p(vb.ptr), None))
    raw, v = read_guarded(out, a.n * es, "out_values"), read_guarded(vb, words(a.n), "out_validity")
    assert whole_words(v, a.n)
    return [bytes(raw[r * es:(r + 1) * es]) for r in range(a.n)], bits_of(v, a.n)


def needle_column(gpu, tname, needle, n):
    """a Python value / None (a scalar) or a list (a column, None = a NULL needle row)"""
    code = K.TYPES[tname][0]
    p, s = (20, 3) if tname == "dec128" else ((10, 3) if tname == "dec64" else (0, 0))
    vals = needle if isinstance(needle, list) else [needle]
    raw = np.frombuffer(b"".join(K.encode(tname, 0 if v is None else v) for v in vals) + bytes(16), dtype=np.uint8)
    valid = [v is not None for v in vals]
    vb = None if all(valid) else gpu.DeviceBuffer.from_numpy(gpu.pack_bits(valid))
    return gpu.Column(code, len(vals), gpu.DeviceBuffer.from_numpy(raw), vb, p, s, is_scalar=not isinstance(needle, list))


def read_find(gpu, op, out, n):
    if op == R.CONTAINS:
        raw = read_guarded(out, words(n), "out")
        assert whole_words(raw, n)
        return bits_of(raw, n)
    return read_guarded(out, n * 8, "out").view(np.uint64).tolist()


def run_find(gpu, op, a, needle):
    out = guarded(gpu, words(a.n) if op == R.CONTAINS else a.n * 8)
    cn = needle_column(gpu, a.tname, needle, a.n)
    ccn = cn.c()
    T.check(T.lib().dbhip_array_find(C.c_int32(op), *a.args(), C.byref(ccn), C.c_void_p(out.ptr), None))
    return read_find(gpu, op, out, a.n)


def run_find_str(gpu, op, a, needle):
    out = guarded(gpu, words(a.n) if op == R.CONTAINS else a.n * 8)
    T.check(T.lib().dbhip_array_find_str(C.c_int32(op), *a.args(), _host(needle), C.c_int32(len(needle)), C.c_void_p(out.ptr), None))
    return read_find(gpu, op, out, a.n)


def run_reduce(gpu, kind, a):
    rt = K.result_type(kind, a.tname)
    es = K.TYPES[rt][2]
    out, vb = guarded(gpu, a.n * es), guarded(gpu, words(a.n))
    err = gpu.DeviceBuffer.from_numpy(np.zeros(1, np.uint64))
    T.check(T.lib().dbhip_array_reduce(C.c_int32(kind), *a.args(), C.c_void_p(out.ptr), C.c_void_p(vb.ptr), C.c_void_p(err.ptr), None))
    raw, v = read_guarded(out, a.n * es, "out"), read_guarded(vb, words(a.n), "out_validity")
    assert whole_words(v, a.n)
    return [K.decode(rt, raw[r * es:(r + 1) * es]) for r in range(a.n)], bits_of(v, a.n), int(err.to_numpy(np.uint64, 1)[0])


def run_unnest(gpu, offsets_dev, n, n_elems, num_out):
    out = guarded(gpu, num_out * 4)
    T.check(T.lib().dbhip_array_unnest_sel(C.c_void_p(offsets_dev.ptr), C.c_int64(n), C.c_uint64(n_elems), C.c_void_p(out.ptr), C.c_int64(num_out), None))
    return read_guarded(out, num_out * 4, "out_sel").view(np.uint32).tolist()


def shapes(tname, for_sum=False):
    """(name, rows, first, voff): every column of the case list; two of them sliced (offsets[0] > 0) with a validity offset that is no
    multiple of 8"""
    out = []
    for name, rows in K.columns(tname, for_sum, full=tname in FULL or tname == "string"):
        out.append((name, rows, 0, 0))
        if name in ("edges", "n65"):
            out.append((name + " sliced", rows, 5, 3))
    return out


def check_reduce(tname, kind, rows, got):
    vals, valid, err = got
    bad, overflows = [], 0
    for r, row in enumerate(rows):
        exp = R.reduce(kind, row, tname)
        if exp is None or exp == R.OVERFLOW:
            overflows += exp is not None
            ok = not valid[r] and vals[r] == 0
        elif not valid[r]:
            ok = False
        elif K.is_float(tname) and kind == R.SUM:
            ok = F.sum_ok(vals[r], exp)
        elif K.is_float(tname) and kind != R.COUNT:
            ok = F.same_value(vals[r], exp, K.TYPES[tname][1], F.one_signed_zero([float(e) for e in row if e is not None]))
        else:
            ok = vals[r] == exp
        if not ok:
            bad.append((r, len(row), vals[r], valid[r], exp))
    assert not bad, (tname, kind, len(bad), bad[0])
    assert err == overflows


# ---- length -----------------------------------------------------------------------------------------------------------------------
def test_length_every_shape(gpu):
    for name, rows, first, voff in shapes("i64"):
        a = Arr(gpu, "i64", rows, first, voff)
        got, bad = run_length(gpu, a)
        assert got == [len(r) for r in rows] and bad == 0, name


def test_n_zero_returns_before_any_launch(gpu):
    a = Arr(gpu, "i64", [])
    lib = T.lib()
    assert lib.dbhip_array_length(None, C.c_int64(0), C.c_uint64(0), None, None, None) == T.OK
    ci = gpu.Column.scalar(1, T.T_I64).c()
    assert lib.dbhip_array_get(*a.args(), C.byref(ci), None, None, None) == T.OK
    cn = needle_column(gpu, "i64", 1, 0).c()
    assert lib.dbhip_array_find(0, *a.args(), C.byref(cn), None, None) == T.OK
    assert lib.dbhip_array_reduce(R.SUM, *a.args(), None, None, None, None) == T.OK
    assert lib.dbhip_array_unnest_sel(None, C.c_int64(0), C.c_uint64(0), None, C.c_int64(0), None) == T.OK
    s = Arr(gpu, "string", [])
    assert lib.dbhip_array_find_str(0, *s.args(), _host(b"x"), C.c_int32(1), None, None) == T.OK
    assert lib.dbhip_array_length(None, C.c_int64(2 ** 32 - 1), C.c_uint64(0), None, None, None) == T.ERR_INVALID


# ---- get ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", list(K.TYPES))
def test_get(gpu, tname):
    es = K.TYPES[tname][2]
    for name, rows, first, voff in shapes(tname):
        a = Arr(gpu, tname, rows, first, voff)
        views = a.child.to_numpy().reshape(-1, 16) if tname == "string" else None

        def expect(r, i):
            n = len(rows[r])
            if not (1 <= i <= n or -n <= i <= -1):
                return bytes(es), False
            e = a.off[r] + (i - 1 if i > 0 else n + i)
            raw = bytes(views[e]) if tname == "string" else K.encode(tname, a.stored[e])     # moved uninterpreted, whatever lies under a NULL
            return raw, rows[r][i - 1 if i > 0 else n + i] is not None

        per_row = K.get_indexes(rows)
        asks = list(K.GET_INDEXES) + [[per_row[r][(r + k) % len(per_row[r])] for r in range(a.n)] for k in range(4)]
        for index in asks:
            vals, valid = run_get(gpu, a, index)
            exp = [expect(r, index if isinstance(index, int) else index[r]) for r in range(a.n)]
            bad = [r for r in range(a.n) if (vals[r], valid[r]) != exp[r]]
            assert not bad, (name, tname, index if isinstance(index, int) else index[bad[0]], len(rows[bad[0]]), vals[bad[0]], valid[bad[0]], exp[bad[0]])


# ---- find ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", K.NUMBERS)
def test_find(gpu, tname):
    isf = K.is_float(tname)
    hits = 0
    for name, rows, first, voff in shapes(tname):
        a = Arr(gpu, tname, rows, first, voff)
        col = K.needles(tname, rows, 5)
        scalars = [col[0], None] + [x for x in col if x is not None][:2]
        for needle in [col] + scalars:
            exp = [R.indexof(row, needle[r] if isinstance(needle, list) else needle, isf) for r, row in enumerate(rows)]
            assert run_find(gpu, R.INDEXOF, a, needle) == exp, (name, tname)
            assert run_find(gpu, R.CONTAINS, a, needle) == [e != 0 for e in exp], (name, tname)
            hits += sum(1 for e in exp if e > 1)
    assert hits > 5


def test_indexof_first_match_in_lane_63_and_in_lane_0_of_the_second_step(gpu):
    rows, x, want = K.indexof_lane_rows()
    a = Arr(gpu, "i64", rows, first=3)
    assert run_find(gpu, R.INDEXOF, a, x) == want
    assert run_find(gpu, R.CONTAINS, a, x) == [w != 0 for w in want]


def test_float_find_is_ordered_float(gpu):
    for tname, nan, zero in (("f32", F.NAN32, F.ZERO32), ("f64", F.NAN64, F.ZERO64)):
        dt = K.TYPES[tname][1]
        long_row = [dt(k) for k in range(1, K.LONG_ROW)] + [nan[1]]
        rows = [[dt(1), nan[1], nan[0]], [dt(1), zero[1], zero[0]], [nan[2]], [dt(np.inf)], long_row, [None, zero[1]]]
        a = Arr(gpu, tname, rows)
        for needle in (nan[3], zero[0], zero[1], dt(np.inf)):
            assert run_find(gpu, R.INDEXOF, a, needle) == [R.indexof(row, needle, True) for row in rows]
        assert run_find(gpu, R.INDEXOF, a, nan[3]) == [2, 0, 1, 0, K.LONG_ROW, 0]


def string_columns(gpu):
    """the String child inline, long at every alignment of a packed buffer, with dirty inline views"""
    return {"packed": None, "lead2": lambda vals: pack(gpu, vals, lead=b"\x80\x80"), "two buffers": lambda vals: pack(gpu, vals, lead=b"\x80\x80\x80", n_buffers=2),
            "dirty": lambda vals: dirty(gpu, pack(gpu, vals))}


def test_find_str(gpu):
    hits = 0
    needles = K.STR_NEEDLES + [b"abcdXfghijklm", b"abcdefghijklmno", bytes(range(1, 255)) + b"\x01", b"zz", b"abc"]
    for how, strings in string_columns(gpu).items():
        for name, rows, first, voff in shapes("string"):
            if how != "packed" and not name.startswith("edges"):
                continue
            a = Arr(gpu, "string", rows, first, voff, strings=strings)
            for nd in needles:
                exp = [R.indexof(row, nd) for row in rows]
                assert run_find_str(gpu, R.INDEXOF, a, nd) == exp, (how, name, nd[:20])
                assert run_find_str(gpu, R.CONTAINS, a, nd) == [e != 0 for e in exp], (how, name, nd[:20])
                hits += sum(1 for e in exp if e > 1)
    assert hits > 50


def test_find_str_view_that_names_a_missing_buffer(gpu):
    long = b"abcd" + b"x" * 16
    for n_long in (3, K.LONG_ROW):                           # the lane's search and the wave's
        vals = [long] * n_long + [b"ab", long]
        rows = [vals]
        miss = {0, 1, 2} if n_long == 3 else set(range(n_long))
        a = Arr(gpu, "string", rows, strings=lambda v: pack(gpu, v, buffer_of=lambda i: 7 if i in miss else 0))
        assert run_find_str(gpu, R.INDEXOF, a, long) == [n_long + 2]
        assert run_find_str(gpu, R.INDEXOF, a, b"ab") == [n_long + 1]


# ---- reduce -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", K.NUMBERS)
def test_reduce(gpu, tname):
    for for_sum in ((False, True) if K.is_float(tname) else (False,)):
        for name, rows, first, voff in shapes(tname, for_sum):
            a = Arr(gpu, tname, rows, first, voff)
            for kind in (R.COUNT, R.SUM, R.MIN, R.MAX):
                if K.result_type(kind, tname) is None or (K.is_float(tname) and (kind == R.SUM) != for_sum and kind != R.COUNT):
                    continue
                check_reduce(tname, kind, rows, run_reduce(gpu, kind, a))
            if R.SUM_CLASS[tname] is None:
                out = gpu.DeviceBuffer(64)
                assert T.lib().dbhip_array_reduce(R.SUM, *a.args(), C.c_void_p(out.ptr), C.c_void_p(out.ptr), None, None) == T.ERR_INVALID


def test_dec128_sum_overflows_in_its_own_row_only(gpu):
    rows = K.dec128_overflow_rows()
    a = Arr(gpu, "dec128", rows)
    vals, valid, err = run_reduce(gpu, R.SUM, a)
    assert valid == [False, True, False, True, False, False, True, True] and err == 4
    assert vals == [0, R.DEC128_MAX, 0, 5, 0, 0, 0, 7]
    check_reduce("dec128", R.SUM, rows, (vals, valid, err))


def test_reduce_result_agrees_with_groupby_result_type(gpu):
    lib = T.lib()
    for tname, (code, _, _) in K.TYPES.items():
        for kind in (R.COUNT, R.SUM, R.MIN, R.MAX):
            t, p, s = C.c_int32(-1), C.c_uint8(99), C.c_uint8(99)
            rc = lib.dbhip_array_reduce_result(kind, code, 20, 3, C.byref(t), C.byref(p), C.byref(s))
            if tname == "string" or K.result_type(kind, tname) is None:
                assert rc == T.ERR_INVALID
                continue
            d = T.AggDesc()
            d.kind, d.arg_type, d.arg_precision, d.arg_scale, d.arg_nullable = kind, code, 20, 3, 1
            gt, gp, gs = C.c_int32(-1), C.c_uint8(99), C.c_uint8(99)
            T.check(lib.dbhip_groupby_result_type(C.byref(d), C.byref(gt), C.byref(gp), C.byref(gs)))
            assert rc == T.OK and (t.value, p.value, s.value) == (gt.value, gp.value, gs.value), (tname, kind)
            assert t.value == K.TYPES[K.result_type(kind, tname)][0]
    for code in (T.T_BOOL, T.T_DEC256):
        t = C.c_int32(-1)
        assert lib.dbhip_array_reduce_result(R.MIN, code, 0, 0, C.byref(t), None, None) == T.ERR_UNSUPPORTED


# ---- unnest -------------------------------------------------------------------------------------------------------------------------
def test_unnest_sel(gpu):
    for name, rows, first, voff in shapes("i64"):
        a = Arr(gpu, "i64", rows, first, voff, tail=4)
        exp = [r for r, row in enumerate(rows) for _ in row]
        assert run_unnest(gpu, a.offsets, a.n, a.n_elems, len(exp)) == exp, name
        if len(exp) > 70:                                    # a num_out below the real one: nothing behind it is written
            assert run_unnest(gpu, a.offsets, a.n, a.n_elems, len(exp) - 67) == exp[:-67], name


def test_unnest_takes_a_sibling_column(gpu):
    rows = K.column("i32", K.small_lengths(300, 4), 9)
    arr = gpu.ArrayColumn.from_lists(rows, T.T_I32)
    sibling = gpu.Column.from_numpy(np.arange(1000, 1300, dtype=np.int64))
    sel, k, values = gpu.unnest(arr)
    taken = gpu.take(sibling, sel, k).to_numpy().tolist()
    assert taken == [1000 + r for r, row in enumerate(rows) for _ in row] and k == sum(len(r) for r in rows)
    flat = K.flat(rows)
    assert [v if ok else None for v, ok in zip(values.to_numpy().tolist(), values.validity_numpy())] == flat


# ---- refusals and malformed offsets -------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    lib = T.lib()
    a = Arr(gpu, "string", [[b"a", b"b"], []])
    out = gpu.DeviceBuffer(256)
    o = C.c_void_p(out.ptr)
    assert lib.dbhip_array_find_str(0, *a.args(), _host(b"x" * 256), C.c_int32(256), o, None) == T.ERR_UNSUPPORTED
    assert lib.dbhip_array_find_str(0, *a.args(), _host(b"x"), C.c_int32(-1), o, None) == T.ERR_INVALID
    assert lib.dbhip_array_find_str(0, *a.args(), None, C.c_int32(3), o, None) == T.ERR_INVALID
    assert lib.dbhip_array_find_str(2, *a.args(), _host(b"x"), C.c_int32(1), o, None) == T.ERR_INVALID
    d = Arr(gpu, "dec128", [[1, 2], [3]])
    other_scale = gpu.Column.scalar(1, T.T_DEC128, 20, 4).c()
    other_type = gpu.Column.scalar(1, T.T_I64).c()
    assert lib.dbhip_array_find(0, *d.args(), C.byref(other_scale), o, None) == T.ERR_INVALID
    assert lib.dbhip_array_find(0, *d.args(), C.byref(other_type), o, None) == T.ERR_INVALID
    ci = gpu.Column.scalar(1, T.T_I64).c()
    for code in (T.T_BOOL, T.T_DEC256):
        bad = gpu.Column(code, 4, gpu.DeviceBuffer(256)).c()
        ref, args = C.byref(bad), (C.c_void_p(d.offsets.ptr), C.c_int64(2), C.c_uint64(3))
        assert lib.dbhip_array_get(ref, *args, C.byref(ci), o, o, None) == T.ERR_UNSUPPORTED
        assert lib.dbhip_array_find(0, ref, *args, C.byref(bad), o, None) == T.ERR_UNSUPPORTED
        assert lib.dbhip_array_find_str(0, ref, *args, _host(b"x"), C.c_int32(1), o, None) == T.ERR_UNSUPPORTED
        assert lib.dbhip_array_reduce(R.COUNT, ref, *args, o, o, None, None) == T.ERR_UNSUPPORTED
    scalar = gpu.Column.scalar(5, T.T_I64).c()
    args = (C.c_void_p(d.offsets.ptr), C.c_int64(2), C.c_uint64(3))
    assert lib.dbhip_array_get(C.byref(scalar), *args, C.byref(ci), o, o, None) == T.ERR_INVALID
    assert lib.dbhip_array_reduce(R.SUM, C.byref(scalar), *args, o, o, None, None) == T.ERR_INVALID
    assert lib.dbhip_array_find(0, C.byref(scalar), *args, C.byref(scalar), o, None) == T.ERR_INVALID
    not_i64 = gpu.Column.scalar(1, T.T_I32).c()
    assert lib.dbhip_array_get(*d.args(), C.byref(not_i64), o, o, None) == T.ERR_INVALID
    # the stream is usable after every refusal
    assert run_reduce(gpu, R.SUM, d)[0] == [3, 3]


def test_malformed_offsets_are_empty_rows(gpu):
    """a decreasing pair and an end past n_elems among good rows (a short one and one for the wave pass): every function treats the bad
    rows as empty and reads nothing through them. The child's allocation is far larger than n_elems says, so an implementation that
    followed the offsets would read allocated bytes (and give a wrong answer), not fault."""
    n_elems = 400
    rng = np.random.default_rng(8)
    data = rng.integers(1, 100, 4096).astype(np.int64)
    off = [0, 3, 2, 5, 4000, 10, 10, 330, 401, 390, 400, 2 ** 63, 2 ** 64 - 1, 7]
    n = len(off) - 1
    runs = R.row_runs(off, n_elems)
    rows = [data[s:s + ln].tolist() for s, ln, _ in runs]
    nbad = sum(1 for r in runs if r[2])
    assert nbad == 8 and max(len(r) for r in rows) > K.T
    child = gpu.Column.from_numpy(data)
    offsets = gpu.DeviceBuffer.from_numpy(np.array(off, dtype=np.uint64))
    a = Arr(gpu, "i64", [])
    a.child, a.offsets, a.n, a.n_elems, a.rows = child, offsets, n, n_elems, rows
    got, bad = run_length(gpu, a)
    assert got == [len(r) for r in rows] and bad == nbad
    for kind in (R.COUNT, R.SUM, R.MIN, R.MAX):
        check_reduce("i64", kind, rows, run_reduce(gpu, kind, a))
    needle = [row[-1] if row else 5 for row in rows]
    assert run_find(gpu, R.INDEXOF, a, needle) == [R.indexof(row, x) for row, x in zip(rows, needle)]
    for i in (1, -1, 3):
        vals, valid = run_get(gpu, a, i)
        assert [K.decode("i64", v) if ok else None for v, ok in zip(vals, valid)] == [R.get(row, i) for row in rows]
    num_out = 500
    got = run_unnest(gpu, offsets, n, n_elems, num_out)
    exp = R.unnest_sel(off, n_elems)
    assert set(exp) == {k for k in range(num_out) if any(s <= k < s + ln for s, ln, _ in runs)}
    overlapped = {k for k in range(num_out) if sum(1 for s, ln, _ in runs if s <= k < s + ln) > 1}
    for k in range(num_out):
        owners = [r for r, (s, ln, _) in enumerate(runs) if s <= k < s + ln]
        assert (got[k] in owners) if owners else got[k] == 0xFFFFFFFF, (k, got[k], owners)
    assert overlapped


def test_n_elems_zero(gpu):
    a = Arr(gpu, "i64", [[]] * 70)
    assert a.n_elems == 0
    assert run_length(gpu, a) == ([0] * 70, 0)
    assert run_reduce(gpu, R.SUM, a) == ([0] * 70, [False] * 70, 0)
    assert run_reduce(gpu, R.COUNT, a) == ([0] * 70, [True] * 70, 0)
    assert run_find(gpu, R.CONTAINS, a, 0) == [False] * 70
    assert run_get(gpu, a, 1) == ([bytes(8)] * 70, [False] * 70)


# ---- the Python layer and the scan --------------------------------------------------------------------------------------------------
def test_array_column_functions(gpu):
    rows = [[1, 2, None, 4], None, [], [None], [7, 7, 3], list(range(300))]
    arr = gpu.ArrayColumn.from_lists(rows, T.T_I64)
    assert arr.to_lists() == [r if r is not None else None for r in rows]
    runs = [r or [] for r in rows]
    live = [r is not None for r in rows]

    def values(col):
        v, ok = col.to_numpy().tolist(), col.validity_numpy().tolist()
        return [x if o else None for x, o in zip(v, ok)]

    def lifted(fn):
        return [fn(run) if ok else None for run, ok in zip(runs, live)]

    assert values(gpu.array_length(arr)) == lifted(len)
    assert values(gpu.array_get(arr, -1)) == lifted(lambda r: R.get(r, -1))
    assert values(gpu.array_contains(arr, 7)) == lifted(lambda r: R.contains(r, 7))
    assert values(gpu.array_indexof(arr, 7)) == lifted(lambda r: R.indexof(r, 7))
    assert values(gpu.array_count(arr)) == lifted(lambda r: R.reduce(R.COUNT, r, "i64"))
    for fn, kind in ((gpu.array_sum, R.SUM), (gpu.array_min, R.MIN), (gpu.array_max, R.MAX)):
        assert values(fn(arr)) == lifted(lambda r: R.reduce(kind, r, "i64"))
    avg = values(gpu.array_avg(arr))
    exp = lifted(lambda r: (sum(e for e in r if e is not None) / len([e for e in r if e is not None])) if any(e is not None for e in r) else None)
    assert avg == exp
    part = arr.slice(3, 6)
    assert part.to_lists() == rows[3:6] and values(gpu.array_sum(part)) == [None, 17, sum(range(300))]
    sel, k, vals = gpu.unnest(part)
    assert sel.to_numpy(np.uint32, k).tolist() == [0] + [1] * 3 + [2] * 300 and vals.n == k
    s = gpu.ArrayColumn.from_lists([[b"a", b"long enough to leave the view", None], [b"b"]], T.T_STRING)
    assert values(gpu.array_contains(s, b"long enough to leave the view")) == [True, False]
    assert gpu.array_get(s, 2).string_values()[0] == b"long enough to leave the view"


def test_decoded_list_chunk_through_array_sum_and_length(gpu):
    import pyarrow as pa
    from tests import parquet_nested_util as NU
    rng = np.random.default_rng(2)
    rows = [[None if rng.random() < 0.2 else int(rng.integers(-10 ** 12, 10 ** 12)) for _ in range(int(rng.integers(0, 6)))] for _ in range(3000)]
    rows[17] = [int(x) for x in rng.integers(-10 ** 12, 10 ** 12, K.LONG_ROW)]
    typ = pa.list_(pa.field("item", pa.int64(), nullable=True))
    table = pa.Table.from_arrays([pa.array(rows, type=typ)], schema=pa.schema([pa.field("c", typ, nullable=False)]))
    ch = NU.write_table(table, "none", False, False)[0][0]
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], NU.LEAF_KINDS["i64"], ch["type_length"], codec=ch["codec"], list_of=(0, 1))
    offs, lv, col = pc.decode_list()
    assert lv is None and pc.rows == len(rows)
    arr = gpu.ArrayColumn(pc.offsets_dev, pc.rows, col)
    assert gpu.array_length(arr).to_numpy().tolist() == [len(r) for r in rows]
    s = gpu.array_sum(arr)
    got = [v if ok else None for v, ok in zip(s.to_numpy().tolist(), s.validity_numpy())]
    assert got == [R.reduce(R.SUM, r, "i64") for r in rows]
    pc.close()
