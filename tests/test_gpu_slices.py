"""GPU: every dbhip_col entry point of the older core on SLICED columns (validity bit offsets that are no multiple of 8, value pointers
aligned to the element only: tests/slice_cases.py) and on nullable scalars. Each result is compared bit for bit with a reference
computed on the host rows (the oracle where the parity tests use it, numpy / Python ints otherwise) and with the same entry point on a
freshly uploaded copy of the same rows: values, result validity (through validity_numpy(), at the result's own offset), error
bitmaps and error counts."""
import ctypes as C
import math

import numpy as np
import pytest

from databend_amd import _lib as T
from databend_amd.device import make_views_general
from tests import datetime_ref as DR
from tests import dec256_ref as R256
from tests import oracle_lib as O
from tests import slice_cases as S
from tests.test_cast_cpu import CODE, NP, oracle_cast
from tests.test_gpu_parity import NUMS, dec_cases, norm, oracle_groupby, oracle_rows, rand_col, rand_dec, same_bits
from tests.test_serializer import oracle_serialize
from tests.test_siphash_cpu import orc_hash

pytestmark = pytest.mark.gpu

NPD = dict(NUMS)
FIVE = [T.T_I8, T.T_I32, T.T_I64, T.T_F32, T.T_F64]
OTHER_LO = {1: 13, 13: 69, 69: 1}


# ---- columns: device (sliced / fresh) and host -------------------------------------------------------------------------------------------
def maker(gpu, t, p=0, s=0):
    if t == T.T_STRING:
        return lambda v, valid: gpu.Column.strings(v, validity=valid)
    if t == T.T_BOOL:
        return lambda v, valid: gpu.Column.boolean(v, validity=valid)
    if t == T.T_DEC128:
        return lambda v, valid: gpu.Column.decimal128(v, p, s, validity=valid)
    if t == T.T_DEC256:
        return lambda v, valid: gpu.Column.decimal256(v, p, s, validity=valid)
    return lambda v, valid: gpu.Column.from_numpy(v, t, validity=valid, precision=p, scale=s)


def host(t, v, valid=None, p=0, s=0, is_scalar=False):
    if t == T.T_STRING:
        views, buf = make_views_general(v)
        return O.HostCol(t, views, valid, buffers=[buf])
    if t == T.T_BOOL:
        return O.HostCol(t, np.concatenate([np.packbits(np.asarray(v, dtype=bool), bitorder="little"), np.zeros(8, np.uint8)]), valid)
    if t == T.T_DEC128:
        return O.HostCol(t, O.i128_array(v), valid, p, s, is_scalar=is_scalar)
    return O.HostCol(t, v, valid, p, s, is_scalar=is_scalar)


def both(gpu, t, v, valid, lo, p=0, s=0, seed=0):
    """-> (the rows as a slice at `lo`, the same rows freshly uploaded)"""
    mk = maker(gpu, t, p, s)
    return S.sliced(gpu, mk, v, valid, lo, seed=seed), mk(v, valid)


def ones(v, n):
    return np.ones(n, dtype=bool) if v is None else np.asarray(v, dtype=bool)


def errs_of(e):
    return e.error_rows().tolist(), e.num_errors()


def bits_to_bool(raw, n):
    return np.unpackbits(np.asarray(raw, np.uint8), bitorder="little")[:n].astype(bool)


def oracle_arith(oracle, op, ha, hb, n):
    ot = oracle.orc_arith_result_type(op, ha.dtype, hb.dtype)
    exp = np.zeros(max(n, 1), dtype=NPD[ot])
    eb = np.zeros(((n + 31) // 32) * 4 + 8, np.uint8)
    ec = C.c_uint64(0)
    ca, cb = ha.c(), hb.c()
    assert oracle.orc_arith(op, C.byref(ca), C.byref(cb), C.c_int64(n), ot, exp.ctypes.data_as(C.c_void_p), eb.ctypes.data_as(C.c_void_p), C.byref(ec)) == 0
    return ot, exp[:n], np.nonzero(~bits_to_bool(eb, n))[0].tolist(), ec.value


def zero_rows(b, n, lo):
    """division-by-zero rows where the junk rows' validity differs from the payload's (the first `lo` rows) and a few behind them"""
    b[:min(n, lo + 3)] = 0
    if n > 200:
        b[190:200] = 0
    return b


def check_arith(gpu, oracle, op, lhs, rhs, n, what):
    """dbhip_arith on the sliced pair == the oracle on the host rows == dbhip_arith on the fresh pair; lhs / rhs = (sliced, fresh, host
    column, validity rows | None)"""
    (ca, fa, ha, va), (cb, fb, hb, vb) = lhs, rhs
    ot, exp, exp_rows, exp_cnt = oracle_arith(oracle, op, ha, hb, n)
    e1, e2 = gpu.RowErrors(n), gpu.RowErrors(n)
    got, fresh = gpu.arith(op, ca, cb, n, errors=e1), gpu.arith(op, fa, fb, n, errors=e2)
    assert got.dtype == ot
    assert same_bits(got.to_numpy()[:n], exp), (what, got.to_numpy()[:8], exp[:8])
    assert same_bits(got.to_numpy()[:n], fresh.to_numpy()[:n]), what
    assert errs_of(e1) == (exp_rows, exp_cnt) == errs_of(e2), (what, errs_of(e1)[1], exp_cnt)
    assert np.array_equal(got.validity_numpy(), ones(va, n) & ones(vb, n)), what
    assert np.array_equal(fresh.validity_numpy(), ones(va, n) & ones(vb, n)), what


# ---- arith -------------------------------------------------------------------------------------------------------------------------------
def test_arith_every_type_pair_on_two_slices(gpu, oracle):
    """all 10 x 10 pairs x 6 operators: lhs a slice at 13, rhs a slice at 69; both nullable (the merged validity is realigned) or the
    rhs plain (the result carries the lhs Bitmap at its offset)"""
    n = 1029
    rng = np.random.default_rng(1301)
    for i, (ta, da) in enumerate(NUMS):
        for j, (tb, db) in enumerate(NUMS):
            a, b = rand_col(rng, ta, da, n), zero_rows(rand_col(rng, tb, db, n), n, 69)
            va = rng.integers(0, 2, n).astype(bool)
            vb = rng.integers(0, 3, n).astype(bool) if (i + j) % 2 else None
            ca, fa = both(gpu, ta, a, va, 13)
            cb, fb = both(gpu, tb, b, vb, 69, seed=1)
            for op in range(6):
                check_arith(gpu, oracle, op, (ca, fa, host(ta, a, va), va), (cb, fb, host(tb, b, vb), vb), n, (op, ta, tb))
            if vb is None:
                res = gpu.arith(T.OP_PLUS, ca, cb, n)
                assert res.validity is ca.validity and res.voff == 13


@pytest.mark.parametrize("n", S.SIZES)
@pytest.mark.parametrize("lo", S.LOS)
def test_arith_offsets_and_sizes(gpu, oracle, lo, n):
    """every (lo, n): two slices at different offsets, a slice with a scalar on either side"""
    rng = np.random.default_rng(100 * lo + n)
    for ta in FIVE:
        for tb in FIVE:
            a, b = rand_col(rng, ta, NPD[ta], n, edge=False), zero_rows(rand_col(rng, tb, NPD[tb], n, edge=False), n, lo)
            va, vb = rng.integers(0, 2, n).astype(bool), rng.integers(0, 4, n) > 0
            ca, fa = both(gpu, ta, a, va, lo)
            cb, fb = both(gpu, tb, b, vb, OTHER_LO[lo], seed=1)
            for op in range(6):
                check_arith(gpu, oracle, op, (ca, fa, host(ta, a, va), va), (cb, fb, host(tb, b, vb), vb), n, (op, ta, tb, "cols"))
            for value in (0, 3):
                sc = np.array([value], dtype=NPD[tb])
                gs, hs = gpu.Column.scalar(sc[0], tb), O.HostCol(tb, sc, is_scalar=True)
                for op in (T.OP_PLUS, T.OP_DIVIDE, T.OP_MODULO):
                    check_arith(gpu, oracle, op, (ca, fa, host(ta, a, va), va), (gs, gs, hs, None), n, (op, ta, tb, "col op scalar", value))
                    check_arith(gpu, oracle, op, (gs, gs, hs, None), (cb, fb, host(tb, b, vb), vb), n, (op, tb, tb, "scalar op col", value))


# ---- nullable scalars --------------------------------------------------------------------------------------------------------------------
SCALAR_CASES = [(True, 0), (True, 5), (False, 0), (False, 5)]      # (valid, voff)


@pytest.mark.parametrize("n", [100, 4099])
@pytest.mark.parametrize("valid,voff", SCALAR_CASES)
def test_nullable_scalar_in_arith(gpu, oracle, valid, voff, n):
    """a scalar has ONE validity bit: a valid zero divisor raises in exactly the rows where the other side is valid, a NULL one never"""
    rng = np.random.default_rng(n + voff)
    a = rng.integers(-1000, 1000, n).astype(np.int32)
    va = rng.integers(0, 3, n) > 0
    ca, fa = both(gpu, T.T_I32, a, va, 13)
    b = rng.integers(-2, 3, n).astype(np.int32)
    cb, fb = both(gpu, T.T_I32, b, va, 69, seed=1)
    for op in (T.OP_DIVIDE, T.OP_INTDIV, T.OP_MODULO, T.OP_DIVNULL):
        for value in (0, 7):
            for left in (False, True):
                sc = S.nullable_scalar(gpu, value, T.T_I32, valid, voff)
                hs = O.HostCol(T.T_I32, np.array([value], np.int32), np.array([valid]), is_scalar=True)
                e1, e2 = gpu.RowErrors(n), gpu.RowErrors(n)
                if left:     # scalar op column: the column holds the zeros
                    got, fresh = gpu.arith(op, sc, cb, n, errors=e1), gpu.arith(op, sc, fb, n, errors=e2)
                    raising = (b == 0) & va & valid
                    hx, hy = hs, host(T.T_I32, b, va)
                else:
                    got, fresh = gpu.arith(op, ca, sc, n, errors=e1), gpu.arith(op, fa, sc, n, errors=e2)
                    raising = va & bool(valid and value == 0)
                    hx, hy = host(T.T_I32, a, va), hs
                exp_rows = np.nonzero(raising)[0].tolist()
                assert errs_of(e1) == (exp_rows, len(exp_rows)), (op, value, left, errs_of(e1)[1], len(exp_rows))
                assert errs_of(e2) == (exp_rows, len(exp_rows))
                if op != T.OP_DIVNULL:
                    _, exp, orows, ocnt = oracle_arith(oracle, op, hx, hy, n)
                    assert (orows, ocnt) == (exp_rows, len(exp_rows))
                    assert same_bits(got.to_numpy()[:n], exp) and same_bits(fresh.to_numpy()[:n], exp)
                assert np.array_equal(got.validity_numpy(), va & valid) and np.array_equal(fresh.validity_numpy(), va & valid)


@pytest.mark.parametrize("n", [100, 4099])
@pytest.mark.parametrize("valid,voff", SCALAR_CASES)
def test_nullable_scalar_in_decimal_arith(gpu, oracle, valid, voff, n):
    rng = np.random.default_rng(n + voff + 1)
    a = rng.integers(-10**9, 10**9, n).astype(np.int64)
    va = rng.integers(0, 3, n) > 0
    ca, fa = both(gpu, T.T_DEC64, a, va, 13, 15, 2)
    for value in (0, 700):
        sc = S.nullable_scalar(gpu, value, T.T_DEC64, valid, voff, 15, 2)
        e1, e2 = gpu.RowErrors(n), gpu.RowErrors(n)
        got, fresh = gpu.decimal_arith(T.OP_DIVIDE, ca, sc, n, errors=e1), gpu.decimal_arith(T.OP_DIVIDE, fa, sc, n, errors=e2)
        exp_rows = np.nonzero(va & bool(valid and value == 0))[0].tolist()
        assert errs_of(e1) == (exp_rows, len(exp_rows)) == errs_of(e2), (value, errs_of(e1)[1], len(exp_rows))
        assert np.array_equal(got.validity_numpy(), va & valid)
        assert np.array_equal(got.data.to_numpy(np.uint64, n), fresh.data.to_numpy(np.uint64, n))
        if value:       # the values: the oracle with a plain scalar (what a scalar's NULL does to the errors is stated above, not asked of it)
            exp = np.zeros(n * (2 if got.dtype == T.T_DEC128 else 1), dtype=np.uint64)
            xa, xs = host(T.T_DEC64, a, None, 15, 2).c(), O.HostCol(T.T_DEC64, np.array([value], np.int64), None, 15, 2, is_scalar=True).c()
            assert oracle.orc_decimal_arith(T.OP_DIVIDE, C.byref(xa), C.byref(xs), C.c_int64(n), got.dtype, got.precision, got.scale, exp.ctypes.data_as(C.c_void_p),
                                            None, None) == 0
            assert np.array_equal(got.data.to_numpy(np.uint64, exp.size), exp)


@pytest.mark.parametrize("n", [100, 4099])
@pytest.mark.parametrize("valid,voff", SCALAR_CASES)
def test_nullable_scalar_in_cmp_select_and_dt_add(gpu, valid, voff, n):
    rng = np.random.default_rng(n + voff + 2)
    a = rng.integers(-50, 50, n).astype(np.int64)
    va = rng.integers(0, 3, n) > 0
    ca, fa = both(gpu, T.T_I64, a, va, 13)
    sc = S.nullable_scalar(gpu, 3, T.T_I64, valid, voff)
    for col in (ca, fa):
        res = gpu.cmp(T.CMP_LT, col, sc, n)
        assert np.array_equal(res.to_numpy()[:n], a < 3)
        assert np.array_equal(res.validity_numpy(), va & valid)
        t, k, f = gpu.select_cmp(T.CMP_LT, col, sc, n=n, want_false=True)
        passed = (a < 3) & va & valid
        assert k == int(passed.sum())
        assert np.array_equal(t.to_numpy(np.uint32, k), np.nonzero(passed)[0]) and np.array_equal(f.to_numpy(np.uint32, n - k), np.nonzero(~passed)[0])
    # dt_add: a delta that leaves the range raises where the date is valid — and only under a valid scalar
    dates = rng.integers(-1000, 1000, n).astype(np.int32)
    cd, fd = both(gpu, T.T_DATE, dates, va, 16)
    for delta in (5, 10**9):
        sd = S.nullable_scalar(gpu, delta, T.T_I64, valid, voff)
        exp, bad = DR.add(DR.U_DAY, dates, np.full(n, delta), DR.SRC_DATE)
        for col in (cd, fd):
            e = gpu.RowErrors(n)
            res = gpu.dt_add(DR.U_DAY, col, sd, n=n, errors=e)
            exp_rows = np.nonzero(bad & va & valid)[0].tolist()
            assert errs_of(e) == (exp_rows, len(exp_rows)), (delta, errs_of(e)[1], len(exp_rows))
            keep = va & valid & ~bad
            assert np.array_equal(res.to_numpy()[:n][keep].astype(np.int64), np.asarray(exp)[keep])
            assert np.array_equal(res.validity_numpy(), va & valid)


# ---- decimals ----------------------------------------------------------------------------------------------------------------------------
def test_decimal_arith_on_slices(gpu, oracle):
    """the dec_cases() of the parity test, lhs a slice at 13, rhs a slice at 69, both nullable; a zero divisor in the rows whose junk
    validity differs"""
    n = 257
    rng = np.random.default_rng(1302)
    props = {T.T_I8: (3, 0), T.T_U8: (3, 0), T.T_I16: (5, 0), T.T_U16: (5, 0), T.T_I32: (10, 0), T.T_U32: (10, 0), T.T_I64: (19, 0), T.T_U64: (20, 0)}
    checked = 0
    for lhs, rhs, op in dec_cases():
        av, _ = rand_dec(rng, lhs, n, True)
        bv, _ = rand_dec(rng, rhs, n, True)
        if op == T.OP_DIVIDE:
            for r in (0, 5, 12, 200):
                bv[r] = 0
        va, vb = rng.integers(0, 2, n).astype(bool), rng.integers(0, 4, n) > 0
        ap = lhs[1:] if lhs[0] in (T.T_DEC64, T.T_DEC128) else props[lhs[0]]
        bp = rhs[1:] if rhs[0] in (T.T_DEC64, T.T_DEC128) else props[rhs[0]]
        p, s = C.c_int(), C.c_int()
        if oracle.orc_decimal_result_size(op, ap[0], ap[1], bp[0], bp[1], C.byref(p), C.byref(s)) != 0:
            continue
        ot = T.T_DEC64 if p.value <= 18 else T.T_DEC128
        exp = np.zeros(n * (2 if ot == T.T_DEC128 else 1), dtype=np.uint64)
        eb = np.zeros(((n + 31) // 32) * 4 + 8, np.uint8)
        ec = C.c_uint64(0)
        ha, hb = host(lhs[0], av, None, lhs[1], lhs[2]), host(rhs[0], bv, None, rhs[1], rhs[2])     # every row computed; only valid rows raise
        xa, xb = ha.c(), hb.c()
        assert oracle.orc_decimal_arith(op, C.byref(xa), C.byref(xb), C.c_int64(n), ot, p.value, s.value, exp.ctypes.data_as(C.c_void_p),
                                        eb.ctypes.data_as(C.c_void_p), C.byref(ec)) == 0
        raw_rows = np.nonzero(~bits_to_bool(eb, n))[0]
        assert ec.value == len(raw_rows)
        exp_rows = [int(r) for r in raw_rows if va[r] and vb[r]]
        ca, fa = both(gpu, lhs[0], av, va, 13, lhs[1], lhs[2])
        cb, fb = both(gpu, rhs[0], bv, vb, 69, rhs[1], rhs[2], seed=1)
        e1, e2 = gpu.RowErrors(n), gpu.RowErrors(n)
        got, fresh = gpu.decimal_arith(op, ca, cb, n, errors=e1), gpu.decimal_arith(op, fa, fb, n, errors=e2)
        ok = np.ones(n, bool)
        ok[raw_rows] = False
        rows = np.repeat(ok, 2) if ot == T.T_DEC128 else ok          # (error rows hold T::one() on the device, the oracle's choice is its own)
        g, f = got.data.to_numpy(np.uint64, exp.size), fresh.data.to_numpy(np.uint64, exp.size)
        assert np.array_equal(g[rows], exp[rows]) and np.array_equal(g, f), (lhs, rhs, op)
        assert errs_of(e1) == (exp_rows, len(exp_rows)) == errs_of(e2), (lhs, rhs, op)
        assert np.array_equal(got.validity_numpy(), va & vb) and np.array_equal(fresh.validity_numpy(), va & vb)
        checked += 1
    assert checked >= 30


def test_decimal_neg_cast_and_decimal256_on_slices(gpu):
    n, lo = 257, 13
    rng = np.random.default_rng(1303)
    valid = rng.integers(0, 2, n).astype(bool)
    for bits, p in ((64, 18), (128, 38), (256, 76)):
        t = {64: T.T_DEC64, 128: T.T_DEC128, 256: T.T_DEC256}[bits]
        vals = [int(x) * 10 ** (p - 18) + int(y) for x, y in zip(rng.integers(-10**17, 10**17, n), rng.integers(0, 1000, n))]
        arr = np.array(vals, dtype=np.int64) if bits == 64 else vals
        col, fresh = both(gpu, t, arr, valid, lo, p, 2)
        # unary minus: the source's validity at its offset
        for c in (col, fresh):
            out = gpu.decimal_neg(c)
            assert [int(v) for v in out.to_numpy()[:n]] == [R256.negate(v, bits) for v in vals]
            assert np.array_equal(out.validity_numpy(), valid)
        assert gpu.decimal_neg(col).voff == lo and gpu.decimal_neg(col).validity is col.validity
        # decimal -> decimal casts, CAST and TRY_CAST
        for dst in ((p, 4), (max(p - 10, 5), 1)):
            exp, okrows = [], []
            for v in vals:
                try:
                    exp.append(R256.cast_decimal(v, bits, (p, 2), dst, rounding_mode=True))
                    okrows.append(True)
                except R256.RowError:
                    exp.append(None)
                    okrows.append(False)
            okrows = np.array(okrows)
            for is_try in (False, True):
                outs = [gpu.decimal_cast(c, dst[0], dst[1], is_try=is_try, rounding_mode=True) for c in (col, fresh)]
                for out, ok, cnt in outs:
                    got = out.to_numpy()[:n]
                    assert all(int(g) == e for g, e, v in zip(got, exp, valid) if e is not None and v), (bits, dst, is_try)
                    if is_try:
                        assert np.array_equal(ok, okrows & valid) and np.array_equal(out.validity_numpy(), okrows & valid)
                    else:
                        assert np.array_equal(ok, okrows | ~valid) and cnt == int((~okrows & valid).sum())
                        assert np.array_equal(out.validity_numpy(), valid)
                assert [int(x) for x in outs[0][0].to_numpy()[:n]] == [int(x) for x in outs[1][0].to_numpy()[:n]]
    # Decimal256 arithmetic and comparisons, two slices
    xs = [int(x) * 10**40 + int(y) for x, y in zip(rng.integers(-10**15, 10**15, n), rng.integers(0, 10**9, n))]
    ys = [int(x) * 10**20 + 1 for x in rng.integers(-10**9, 10**9, n)]
    for r in (0, 7, 12, 100):
        ys[r] = 0
    for r in (3, 50):
        ys[r] = xs[r]
    vx, vy = rng.integers(0, 2, n).astype(bool), rng.integers(0, 3, n) > 0
    cx, fx = both(gpu, T.T_DEC256, xs, vx, 13, 60, 4)
    cy, fy = both(gpu, T.T_DEC256, ys, vy, 69, 60, 4, seed=1)
    for op, rop in ((T.OP_PLUS, R256.OP_PLUS), (T.OP_MULTIPLY, R256.OP_MULTIPLY), (T.OP_DIVIDE, R256.OP_DIVIDE)):
        exp = []
        for x, y in zip(xs, ys):
            try:
                exp.append(R256.binary(rop, x, "dec", (60, 4), y, "dec", (60, 4))[0])
            except R256.RowError:
                exp.append(None)
        exp_rows = [i for i, e in enumerate(exp) if e is None and vx[i] and vy[i]]
        for a, b in ((cx, cy), (fx, fy)):
            e = gpu.RowErrors(n)
            out = gpu.decimal_arith(op, a, b, n, errors=e)
            assert errs_of(e) == (exp_rows, len(exp_rows)), (op, errs_of(e)[1], len(exp_rows))
            assert all(int(g) == x for g, x, v in zip(out.to_numpy()[:n], exp, vx & vy) if x is not None and v), op
            assert np.array_equal(out.validity_numpy(), vx & vy)
    for op, f in ((T.CMP_EQ, lambda x, y: x == y), (T.CMP_LT, lambda x, y: x < y), (T.CMP_GTE, lambda x, y: x >= y)):
        for a, b in ((cx, cy), (fx, fy)):
            res = gpu.cmp(op, a, b, n)
            assert res.to_numpy()[:n].tolist() == [f(x, y) for x, y in zip(xs, ys)]
            assert np.array_equal(res.validity_numpy(), vx & vy)


# ---- cast --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_try", [False, True])
def test_cast_every_number_pair_on_a_slice(gpu, is_try):
    L = O.load()
    n, lo = 1029, 13
    rng = np.random.default_rng(1304)
    for src in NP:
        arr = rand_col(rng, CODE[src], NP[src], n)
        valid = rng.integers(0, 3, n) > 0
        col, fresh = both(gpu, CODE[src], arr, valid, lo)
        for dst in NP:
            with np.errstate(all="ignore"):
                eout, eok, enerr = oracle_cast(L, arr, src, dst, is_try, True, validity=valid)
            (c1, ok1, n1), (c2, ok2, n2) = (gpu.cast(c, CODE[dst], is_try=is_try, rounding_mode=True) for c in (col, fresh))
            for c, ok, nerr in ((c1, ok1, n1), (c2, ok2, n2)):
                assert np.array_equal(c.to_numpy()[:n].view(np.uint8), eout.view(np.uint8)), (src, dst)
                assert np.array_equal(ok, eok), (src, dst)
                assert np.array_equal(c.validity_numpy(), eok if is_try else valid), (src, dst)
                if not is_try:
                    assert nerr == enerr
            if not is_try:
                assert c1.validity is col.validity and c1.voff == lo


# ---- column_sum --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SIZES)
@pytest.mark.parametrize("lo", S.LOS)
def test_column_sum_on_a_slice(gpu, lo, n):
    rng = np.random.default_rng(lo * 7 + n)
    valid = rng.integers(0, 3, n) > 0
    for t, npd in NUMS:
        a = rand_col(rng, t, npd, n, edge=False)
        for v in (valid, None):
            col, fresh = both(gpu, t, a, v, lo)
            got, again = gpu.column_sum(col), gpu.column_sum(fresh)
            rows = a[ones(v, n)]
            if npd in (np.float32, np.float64):
                x = [float(y) for y in rows]
                exp = math.fsum(x)
                tol = n * np.finfo(np.float64).eps * math.fsum(abs(y) for y in x)
                assert abs(got - exp) <= tol, (t, got, exp, tol)
                assert got == again          # the same rows in the same fixed tree
            else:
                exp = sum(int(y) for y in rows) & (2**64 - 1)
                if np.issubdtype(npd, np.signedinteger) and exp >> 63:
                    exp -= 2**64
                assert got == exp == again, (t, v is None)


# ---- cmp ---------------------------------------------------------------------------------------------------------------------------------
def oracle_cmp(oracle, op, ha, hb, n):
    exp = np.zeros((n + 7) // 8 + 8, np.uint8)
    ca, cb = ha.c(), hb.c()
    oracle.orc_cmp(op, C.byref(ca), C.byref(cb), C.c_int64(n), exp.ctypes.data_as(C.c_void_p))
    return bits_to_bool(exp, n)


@pytest.mark.parametrize("n", S.SIZES)
@pytest.mark.parametrize("lo", S.LOS)
def test_cmp_numbers_on_slices(gpu, oracle, lo, n):
    """every number type; at lo = 13 neither operand is 16-byte aligned and the narrow types take the 4-rows-per-lane kernel (whose
    loads fall back to the element path), also against a scalar"""
    rng = np.random.default_rng(lo * 11 + n)
    for t, npd in NUMS:
        a, b = rand_col(rng, t, npd, n), rand_col(rng, t, npd, n)
        b[::3] = a[::3]
        va, vb = rng.integers(0, 2, n).astype(bool), rng.integers(0, 4, n) > 0
        ca, fa = both(gpu, t, a, va, lo)
        cb, fb = both(gpu, t, b, vb, lo, seed=1)
        if lo == 13:
            assert ca.data.ptr % 16 and cb.data.ptr % 16
        gs, hs = gpu.Column.scalar(a[0], t), O.HostCol(t, a[:1], is_scalar=True)
        for op in range(6):
            exp = oracle_cmp(oracle, op, host(t, a), host(t, b), n)
            for x, y in ((ca, cb), (fa, fb)):
                res = gpu.cmp(op, x, y, n)
                assert np.array_equal(res.to_numpy()[:n], exp), (t, op)
                assert np.array_equal(res.validity_numpy(), va & vb)
            exp = oracle_cmp(oracle, op, host(t, a), hs, n)
            for x in (ca, fa):
                res = gpu.cmp(op, x, gs, n)
                assert np.array_equal(res.to_numpy()[:n], exp), (t, op, "scalar")
                assert np.array_equal(res.validity_numpy(), va)


STRS = [b"", b"a", b"ab", b"abc", b"abd", b"a" * 12, b"a" * 13, b"a" * 13 + b"b", b"zzzzzzzzzzzzzzzzzzzzzz", b"b", b"a value of more than twelve bytes"]


def test_cmp_strings_decimal128_and_boolean_on_slices(gpu):
    n = 257
    rng = np.random.default_rng(1305)
    va, vb = rng.integers(0, 2, n).astype(bool), rng.integers(0, 4, n) > 0
    ops = ((T.CMP_EQ, lambda x, y: x == y), (T.CMP_NOTEQ, lambda x, y: x != y), (T.CMP_LT, lambda x, y: x < y), (T.CMP_GTE, lambda x, y: x >= y))
    A = [STRS[i] for i in rng.integers(0, len(STRS), n)]
    B = [STRS[i] for i in rng.integers(0, len(STRS), n)]
    d1 = [int(x) * 10**12 for x in rng.integers(-10**17, 10**17, n)]
    d2 = [d1[i] if i % 3 == 0 else int(x) * 10**12 for i, x in enumerate(rng.integers(-10**17, 10**17, n))]
    b1, b2 = rng.integers(0, 2, n).astype(bool), rng.integers(0, 2, n).astype(bool)
    for t, x, y, p in ((T.T_STRING, A, B, 0), (T.T_DEC128, d1, d2, 38), (T.T_BOOL, b1, b2, 0)):
        for lo in S.LOS:
            ca, fa = both(gpu, t, x, va, lo, p, 0)
            cb, fb = both(gpu, t, y, vb, OTHER_LO[lo], p, 0, seed=1)
            for op, f in ops:
                exp = [bool(f(u, v)) for u, v in zip(x, y)]
                for u, v in ((ca, cb), (fa, fb), (ca, fb)):
                    res = gpu.cmp(op, u, v, n)
                    assert res.to_numpy()[:n].tolist() == exp, (t, lo, op)
                    assert np.array_equal(res.validity_numpy(), va & vb)


# ---- selections --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SIZES)
@pytest.mark.parametrize("lo", S.LOS)
def test_select_cmp_and_select_bool_on_slices(gpu, oracle, lo, n):
    rng = np.random.default_rng(lo * 13 + n)
    va, vb = rng.integers(0, 2, n).astype(bool), rng.integers(0, 4, n) > 0
    picked = np.nonzero(rng.integers(0, 3, n) > 0)[0].astype(np.uint32)
    if len(picked) == 0:
        picked = np.array([0], np.uint32)
    dsel = gpu.DeviceBuffer.from_numpy(picked)

    def lists(passed, sel):
        rows = np.arange(n) if sel is None else sel
        return rows[passed[rows]], rows[~passed[rows]]

    for t in (T.T_I8, T.T_I32, T.T_I64, T.T_F32, T.T_F64):
        a, b = rand_col(rng, t, NPD[t], n), rand_col(rng, t, NPD[t], n)
        b[::2] = a[::2]
        ca, fa = both(gpu, t, a, va, lo)
        cb, fb = both(gpu, t, b, vb, OTHER_LO[lo], seed=1)
        for op in (T.CMP_EQ, T.CMP_LT, T.CMP_GTE):
            passed = oracle_cmp(oracle, op, host(t, a), host(t, b), n) & va & vb
            for x, y in ((ca, cb), (fa, fb)):
                for sel, hs in ((None, None), (dsel, picked)):
                    k_in = n if sel is None else len(picked)
                    tl, k, fl = gpu.select_cmp(op, x, y, sel, k_in, want_false=True)
                    et, ef = lists(passed, hs)
                    assert k == len(et)
                    assert np.array_equal(tl.to_numpy(np.uint32, k), et) and np.array_equal(fl.to_numpy(np.uint32, k_in - k), ef), (t, op)
                    tl2, k2, none = gpu.select_cmp(op, x, y, sel, k_in)
                    assert none is None and k2 == k and np.array_equal(tl2.to_numpy(np.uint32, k), et)
    bools = rng.integers(0, 2, n).astype(bool)
    cp, fp = both(gpu, T.T_BOOL, bools, va, lo)
    passed = bools & va
    for pred in (cp, fp):
        for sel, hs in ((None, None), (dsel, picked)):
            k_in = n if sel is None else len(picked)
            tl, k, fl = gpu.select_bool(pred, sel, k_in, want_false=True)
            et, ef = lists(passed, hs)
            assert k == len(et) and np.array_equal(tl.to_numpy(np.uint32, k), et) and np.array_equal(fl.to_numpy(np.uint32, k_in - k), ef)


@pytest.mark.parametrize("n", S.SIZES)
@pytest.mark.parametrize("lo", S.LOS)
def test_filter_select_and_bitmap_count_on_a_sliced_predicate(gpu, lo, n):
    bools = np.random.default_rng(lo * 17 + n).integers(0, 2, n).astype(bool)
    for pred in both(gpu, T.T_BOOL, bools, None, lo):
        sel, k = gpu.filter_select(pred)
        assert k == int(bools.sum()) and np.array_equal(sel.to_numpy(np.uint32, k), np.nonzero(bools)[0])
        assert gpu.bitmap_count(pred, n) == int(bools.sum())


# ---- take --------------------------------------------------------------------------------------------------------------------------------
def take_sources(rng, n):
    return [(T.T_U8, rng.integers(0, 255, n).astype(np.uint8), 0), (T.T_I16, rng.integers(-2**15, 2**15, n).astype(np.int16), 0),
            (T.T_I32, rng.integers(-2**31, 2**31, n).astype(np.int32), 0), (T.T_I64, rng.integers(-2**62, 2**62, n).astype(np.int64), 0),
            (T.T_F64, rng.standard_normal(n), 0), (T.T_DEC128, [int(x) << 50 for x in rng.integers(-2**60, 2**60, n)], 38),
            (T.T_BOOL, rng.integers(0, 2, n).astype(bool), 0)]


@pytest.mark.parametrize("density", ["dense", "tenth", "unordered"])
@pytest.mark.parametrize("lo", S.LOS)
def test_take_and_take_block_from_sliced_sources(gpu, lo, density):
    """the shapes the windowed take distinguishes (plain gather / LDS window / gather again), every element size, Boolean values and
    validities at a bit offset"""
    n = 4099
    rng = np.random.default_rng(lo + len(density))
    if density == "dense":
        sel = np.nonzero(rng.random(n) < 0.9)[0]
    elif density == "tenth":
        sel = np.nonzero(rng.random(n) < 0.12)[0]
    else:
        sel = rng.integers(0, n, 1500)
    sel = sel.astype(np.uint32)
    k = len(sel)
    dsel = gpu.DeviceBuffer.from_numpy(sel)
    valid = rng.integers(0, 3, n) > 0
    srcs = take_sources(rng, n)
    pairs = [both(gpu, t, v, valid if i % 2 == 0 else None, lo, p, 0) for i, (t, v, p) in enumerate(srcs)]

    def check(out, i, v):
        got = out.to_numpy()[:k]
        exp = [v[j] for j in sel] if isinstance(v, list) else v[sel]
        assert (got == exp) if isinstance(v, list) else np.array_equal(got, exp), (i, density)
        assert np.array_equal(out.validity_numpy(), valid[sel] if i % 2 == 0 else np.ones(k, bool)), (i, density)

    for which in (0, 1):
        cols = [p[which] for p in pairs]
        for i, (c, (t, v, p)) in enumerate(zip(cols, srcs)):
            check(gpu.take(c, dsel, k), i, v)
        for i, (out, (t, v, p)) in enumerate(zip(gpu.take_block(cols, dsel, k), srcs)):
            check(out, i, v)


@pytest.mark.parametrize("lo", S.LOS)
def test_take_outer_and_take_bitmap_from_sliced_sources(gpu, lo):
    n, k = 1029, 700
    rng = np.random.default_rng(lo + 40)
    idx = rng.integers(0, n, k).astype(np.uint32)
    idx[::7] = 0xFFFFFFFF
    didx = gpu.DeviceBuffer.from_numpy(idx)
    valid = rng.integers(0, 2, n).astype(bool)
    hit = idx != 0xFFFFFFFF
    safe = np.where(hit, idx, 0)
    for t, v, p in take_sources(rng, n)[:6]:
        for col in both(gpu, t, v, valid, lo, p, 0):
            es = gpu.ELEM_SIZE[t]
            data, vbuf = gpu.DeviceBuffer(k * es + 64), gpu.DeviceBuffer(((k + 63) // 64) * 8 + 8)
            T.check(T.lib().dbhip_take_outer(C.c_void_p(col.data.ptr), C.c_void_p(col.validity.ptr), C.c_int64(col.voff), es, C.c_void_p(didx.ptr), C.c_int64(k),
                                             C.c_void_p(data.ptr), C.c_void_p(vbuf.ptr), None))
            out = gpu.Column(t, k, data, vbuf, p, 0)
            got = out.to_numpy()
            if isinstance(v, list):
                assert [int(g) for g in got] == [v[j] if h else 0 for j, h in zip(safe, hit)]
            else:
                assert np.array_equal(got, np.where(hit, v[safe], 0).astype(v.dtype))
            assert np.array_equal(out.validity_numpy(), hit & valid[safe])
    # dbhip_take_bitmap at a bit offset, ascending selection
    sel = np.nonzero(rng.integers(0, 2, n))[0].astype(np.uint32)
    dsel = gpu.DeviceBuffer.from_numpy(sel)
    for col in both(gpu, T.T_BOOL, valid, None, lo):
        out = gpu.DeviceBuffer(((len(sel) + 63) // 64) * 8 + 8)
        T.check(T.lib().dbhip_take_bitmap(C.c_void_p(col.data.ptr), C.c_int64(col.boff), C.c_void_p(dsel.ptr), C.c_int64(len(sel)), C.c_void_p(out.ptr), None))
        assert np.array_equal(gpu.unpack_bits(out.to_numpy(np.uint8, (len(sel) + 7) // 8), len(sel)), valid[sel])


# ---- keys --------------------------------------------------------------------------------------------------------------------------------
def key_sets(rng, n):
    """the six column sets of test_pack_keys_matches_oracle"""
    v1, v2 = rng.integers(0, 4, n) > 0, rng.integers(0, 3, n) > 0
    i64 = rng.integers(-2**62, 2**62, n).astype(np.int64)
    i32 = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    u8 = rng.integers(0, 256, n).astype(np.uint8)
    i16 = rng.integers(-2**15, 2**15 - 1, n).astype(np.int16)
    f32 = rng.standard_normal(n).astype(np.float32)
    d128 = [int(x) * 10**7 for x in rng.integers(-10**17, 10**17, n)]
    d128s = [int(x) for x in rng.integers(-10**9, 10**9, n)]
    return [
        [(T.T_I64, i64, None, 0, 0)],
        [(T.T_I32, i32, v1, 0, 0), (T.T_U8, u8, None, 0, 0), (T.T_I16, i16, v2, 0, 0)],
        [(T.T_I64, i64, v1, 0, 0), (T.T_DATE, i32, None, 0, 0), (T.T_F32, f32, None, 0, 0)],
        [(T.T_DEC128, d128, v2, 30, 4), (T.T_I16, i16, None, 0, 0)],
        [(T.T_DEC128, d128s, None, 12, 2), (T.T_DEC64, i64, None, 15, 2), (T.T_U8, u8, v1, 0, 0)],
        [(T.T_I64, i64, None, 0, 0), (T.T_TIMESTAMP, i64[::-1].copy(), None, 0, 0), (T.T_DEC128, d128, None, 38, 0)],
    ]


@pytest.mark.parametrize("n", [63, 257, 4099])
def test_pack_keys_and_keys_method_on_slices(gpu, oracle, n):
    rng = np.random.default_rng(n + 50)
    for spec in key_sets(rng, n):
        hcols = [host(t, arr, v, p, s) for t, arr, v, p, s in spec]
        pairs = [both(gpu, t, arr, v, S.LOS[i % 3], p, s, seed=i) for i, (t, arr, v, p, s) in enumerate(spec)]
        kb = oracle.orc_keys_method(O.cols(hcols), len(hcols))
        exp = np.zeros(n * kb, np.uint8)
        assert oracle.orc_pack_keys(O.cols(hcols), len(hcols), C.c_int64(n), kb, exp.ctypes.data_as(C.c_void_p)) == 0
        allv = np.ones(n, bool)
        for _, _, v, _, _ in spec:
            allv &= ones(v, n)
        for which in (0, 1):
            gcols = [p[which] for p in pairs]
            assert gpu.keys_method(gcols) == kb and kb > 0
            pk = gpu.pack_keys(gcols)
            assert pk.key_bytes == kb and np.array_equal(pk.to_numpy().reshape(-1), exp)
            assert np.array_equal(gpu.unpack_bits(pk.validity.to_numpy(np.uint8, (n + 7) // 8), n), allv)


def serializer_columns(rng, n):
    pool = [b"", b"k", b"Customer#000000001", b"Customer#000000002", b"x" * 40, b"x" * 39 + b"y", b"abcdefghijkl", b"abcdefghijklm"]
    return [(T.T_I32, rng.integers(-5, 5, n).astype(np.int32), rng.integers(0, 6, n) > 0, 0, 0),
            (T.T_STRING, [pool[i] for i in rng.integers(0, len(pool), n)], rng.integers(0, 8, n) > 0, 0, 0),
            (T.T_DEC128, [int(x) * 10**20 for x in rng.integers(-3, 3, n)], None, 30, 2),
            (T.T_BOOL, rng.integers(0, 2, n).astype(bool), rng.integers(0, 5, n) > 0, 0, 0),
            (T.T_I64, rng.integers(-2**62, 2**62, n).astype(np.int64), None, 0, 0)]


@pytest.mark.parametrize("n", [63, 257, 4099])
def test_serialize_keys_on_slices(gpu, n):
    spec = serializer_columns(np.random.default_rng(n + 60), n)
    off_o, data_o = oracle_serialize([host(t, v, val, p, s) for t, v, val, p, s in spec], n)
    allv = np.ones(n, bool)
    for _, _, val, _, _ in spec:
        allv &= ones(val, n)
    pairs = [both(gpu, t, v, val, S.LOS[i % 3], p, s, seed=i) for i, (t, v, val, p, s) in enumerate(spec)]
    for which in (0, 1):
        off, data, av, total = gpu.serialize_keys([p[which] for p in pairs], n)
        assert total == len(data_o)
        assert np.array_equal(off.to_numpy(np.uint64, n + 1), off_o) and np.array_equal(data.to_numpy(np.uint8, total), data_o)
        assert np.array_equal(gpu.unpack_bits(av.to_numpy(np.uint8, (n + 7) // 8), n), allv)


@pytest.mark.parametrize("n", [63, 257, 4099])
def test_siphash64_and_scatter_indices_on_slices(gpu, oracle, n):
    rng = np.random.default_rng(n + 70)
    spec = serializer_columns(rng, n) + [(T.T_F64, rng.standard_normal(n), rng.integers(0, 3, n) > 0, 0, 0), (T.T_U16, rng.integers(0, 2**16, n).astype(np.uint16), None, 0, 0)]
    pairs = [both(gpu, t, v, val, S.LOS[i % 3], p, s, seed=i) for i, (t, v, val, p, s) in enumerate(spec)]
    hcols = [host(t, v, val, p, s) for t, v, val, p, s in spec]
    for (col, fresh), h in zip(pairs, hcols):
        exp = orc_hash(h, n)
        assert np.array_equal(gpu.siphash64(col), exp) and np.array_equal(gpu.siphash64(fresh), exp), h.dtype
    m = 7
    for idxs, default in (([0], 3), ([4], 0), ([0, 1], 0), ([4, 0, 1], 0)):
        eidx, ecnt = np.zeros(n, np.uint32), np.zeros(m, np.uint64)
        assert oracle.orc_scatter_indices(O.cols([hcols[i] for i in idxs]), len(idxs), C.c_int64(n), C.c_uint64(m), C.c_uint64(default),
                                          eidx.ctypes.data_as(C.c_void_p), ecnt.ctypes.data_as(C.c_void_p)) == 0
        for which in (0, 1):
            idx, counts = gpu.scatter_indices([pairs[i][which] for i in idxs], m, default)
            assert np.array_equal(idx.to_numpy(np.uint32, n), eidx) and np.array_equal(counts, ecnt), (idxs, which)


# ---- expressions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.SIZES)
def test_expression_program_over_three_sliced_nullable_inputs(gpu, n):
    """if(and_filters(a < b, cast(a) > c), a + b, c): arith, cmp, cast, if_ and and_filters in one program"""
    rng = np.random.default_rng(n + 80)
    a, b = rng.integers(-100, 100, n).astype(np.int32), rng.integers(-100, 100, n).astype(np.int32)
    c = rng.integers(-100, 100, n).astype(np.int64)
    va, vb, vc = (rng.integers(0, 4, n) > 0 for _ in range(3))
    trios = [both(gpu, T.T_I32, a, va, 1), both(gpu, T.T_I32, b, vb, 13, seed=1), both(gpu, T.T_I64, c, vc, 69, seed=2)]
    outs = []
    for which in (0, 1):
        p = gpu.ExprProgram([t[which] for t in trios])
        la, lb, lc = p.load(0), p.load(1), p.load(2)
        c1 = p.cmp(T.EX_LT, la, lb, keep=(la, lb))
        s = p.arith(T.EX_PLUS, la, lb, keep=(la,))
        c2 = p.cmp(T.EX_GT, p.cast(la, T.T_I64), lc, keep=(lc,))
        r = p.if_(p.and_filters(c1, c2), s, lc)
        outs.append(p.run(r, n))
    cond = (va & vb & (a < b)) & (va & vc & (a.astype(np.int64) > c))
    exp = np.where(cond, a.astype(np.int64) + b, c)
    allv = va & vb & vc
    for out in outs:
        assert out["type"] == T.T_I64
        assert np.array_equal(out["values"][allv], exp[allv])
        assert out["validity"][allv].all()
    assert np.array_equal(outs[0]["values"], outs[1]["values"]) and np.array_equal(outs[0]["validity"], outs[1]["validity"])


# ---- group by ----------------------------------------------------------------------------------------------------------------------------
def test_groupby_sliced_keys_and_arguments(gpu, oracle):
    """add_block and add_block with a sliced nullable filter column over about 40 groups, add_block_program over four (the fused kernel
    takes at most 8 distinct groups per workgroup, by contract): sorted row sets against the oracle"""
    n, card = 4099, 40
    rng = np.random.default_rng(1310)
    k_i64 = rng.integers(0, card, n).astype(np.int64) - card // 2
    strs = [b"s%d" % (x % 7) for x in rng.integers(0, card, n)]
    kvalid = rng.integers(0, 8, n) > 0
    a_i32 = rng.integers(-2**31, 2**31 - 1, n).astype(np.int32)
    a_i64 = rng.integers(-2**40, 2**40, n).astype(np.int64)
    avalid = rng.integers(0, 4, n) > 0
    fbits, fvalid = rng.integers(0, 3, n) > 0, rng.integers(0, 5, n) > 0
    key_types, key_nullable = [T.T_I64, T.T_STRING], [1, 0]
    aggs = [(T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_I32, 0, 0, 1), (T.AGG_MAX, T.T_I64, 0, 0, 0), (T.AGG_COUNT, T.T_I32, 0, 0, 1)]

    k_few = np.abs(k_i64) % 3

    def expected(rows, few=False):
        v, buf = make_views_general([strs[i] for i in rows])
        hkeys = [O.HostCol(T.T_I64, (k_few if few else k_i64)[rows], kvalid[rows]), O.HostCol(T.T_STRING, v, buffers=[buf])][:1 if few else 2]
        hargs = [None, O.HostCol(T.T_I32, a_i32[rows], avalid[rows]), O.HostCol(T.T_I64, a_i64[rows]), O.HostCol(T.T_I32, a_i32[rows], avalid[rows])]
        kt, kn = (key_types[:1], key_nullable[:1]) if few else (key_types, key_nullable)
        h = oracle_groupby(oracle, kt, kn, aggs, hkeys, hargs, len(rows))
        exp = oracle_rows(oracle, h, kt, aggs)
        oracle.orc_hashagg_destroy(h)
        return exp

    everything, kept = np.arange(n), np.nonzero(fbits & fvalid)[0]
    for which in (0, 1):
        keys = [both(gpu, T.T_I64, k_i64, kvalid, 13)[which], both(gpu, T.T_STRING, strs, None, 69, seed=1)[which]]
        arg32, arg64 = both(gpu, T.T_I32, a_i32, avalid, 1, seed=2)[which], both(gpu, T.T_I64, a_i64, None, 13, seed=3)[which]
        flt = both(gpu, T.T_BOOL, fbits, fvalid, 69, seed=4)[which]
        g = gpu.GroupBy(key_types, aggs, key_nullable)
        g.add_block(keys, [None, arg32, arg64, arg32], n)
        assert norm(g.result()) == norm(expected(everything)), which
        g = gpu.GroupBy(key_types, aggs, key_nullable)
        g.add_block(keys, [None, arg32, arg64, arg32], n, filter=flt)
        assert norm(g.result()) == norm(expected(kept)), which
        g = gpu.GroupBy(key_types[:1], aggs, key_nullable[:1])
        g.add_block_program([both(gpu, T.T_I64, k_few, kvalid, 69, seed=5)[which]], gpu.ExprProgram([arg32, arg64]), [None, ("input", 0), ("input", 1), ("input", 0)], n)
        assert norm(g.result()) == norm(expected(everything, few=True)), which


# ---- joins -------------------------------------------------------------------------------------------------------------------------------
def dict_join(bk, bok, pk, pok):
    table = {}
    for r, (k, ok) in enumerate(zip(bk, bok)):
        if ok:
            table.setdefault(k, []).append(r)
    return [(i, r) for i, (k, ok) in enumerate(zip(pk, pok)) if ok for r in table.get(k, [])]


def test_hash_join_on_sliced_keys_and_payloads(gpu):
    nb, np_ = 1000, 4099
    rng = np.random.default_rng(1311)
    bk = rng.integers(0, 300, nb).astype(np.uint64) * np.uint64(2654435761)
    pk = rng.integers(0, 450, np_).astype(np.uint64) * np.uint64(2654435761)
    bvalid, pvalid = rng.integers(0, 4, nb) > 0, rng.integers(0, 4, np_) > 0
    bpay, ppay = rng.integers(-2**62, 2**62, nb).astype(np.int64), rng.integers(-2**31, 2**31, np_).astype(np.int32)
    bpv, ppv = rng.integers(0, 3, nb) > 0, rng.integers(0, 3, np_) > 0
    exp = dict_join(bk.tolist(), bvalid, pk.tolist(), pvalid)
    assert len(exp) > 1000
    ep, eb = np.array([p for p, _ in exp], np.uint32), np.array([b for _, b in exp], np.uint32)
    marks = np.zeros(np_, bool)
    marks[ep] = True
    unmatched = np.nonzero(~marks)[0]
    for which in (0, 1):
        j = gpu.HashJoin(nb)
        for lo, hi, off in ((0, 400, 13), (400, nb, 69)):       # two build blocks, each a slice
            j.add_block(both(gpu, T.T_U64, bk[lo:hi], bvalid[lo:hi], off)[which])
        j.final_build()
        probe = both(gpu, T.T_U64, pk, pvalid, 13, seed=1)[which]
        gp, gb = j.probe_block(probe)
        assert np.array_equal(gp, ep) and np.array_equal(gb, eb)
        assert np.array_equal(j.probe_mark(probe), marks)
        pcol, bcol = both(gpu, T.T_I32, ppay, ppv, 69, seed=2)[which], both(gpu, T.T_I64, bpay, bpv, 1, seed=3)[which]
        outp, outb, rows = j.join("left", probe, [pcol], [bcol])
        assert rows == len(exp) + len(unmatched)
        prow = np.concatenate([ep, unmatched]).astype(np.int64)
        assert np.array_equal(outp[0].to_numpy()[:rows], ppay[prow]) and np.array_equal(outp[0].validity_numpy(), ppv[prow])
        assert np.array_equal(outb[0].to_numpy()[:len(exp)], bpay[eb])
        assert np.array_equal(outb[0].validity_numpy(), np.concatenate([bpv[eb], np.zeros(len(unmatched), bool)]))
        outp, outb, rows = j.join("inner", probe, [pcol], [bcol])
        assert rows == len(exp) and np.array_equal(outb[0].validity_numpy(), bpv[eb]) and np.array_equal(outp[0].validity_numpy(), ppv[ep])


def test_binary_hash_join_on_sliced_key_columns(gpu):
    nb, np_ = 300, 1029
    rng = np.random.default_rng(1312)
    pool = [b"", b"k", b"Customer#000000001", b"Customer#000000002", b"x" * 40, b"abcdefghijklm"]

    def side(n):
        return (rng.integers(-3, 3, n).astype(np.int32), rng.integers(0, 6, n) > 0, [pool[i] for i in rng.integers(0, len(pool), n)], rng.integers(0, 8, n) > 0)

    bi, bv1, bs, bv2 = side(nb)
    pi, pv1, ps, pv2 = side(np_)
    exp = sorted(dict_join(list(zip(bi.tolist(), bs)), bv1 & bv2, list(zip(pi.tolist(), ps)), pv1 & pv2))
    assert len(exp) > 100
    for which in (0, 1):
        j = gpu.BinaryHashJoin(nb)
        j.add_block([both(gpu, T.T_I32, bi, bv1, 13)[which], both(gpu, T.T_STRING, bs, bv2, 69, seed=1)[which]], nb)
        j.final_build()
        gi, gb, matched = j.probe_block([both(gpu, T.T_I32, pi, pv1, 69, seed=2)[which], both(gpu, T.T_STRING, ps, pv2, 1, seed=3)[which]], np_)
        assert list(zip(gi.tolist(), gb.tolist())) == exp
        assert np.array_equal(matched, np.isin(np.arange(np_), [p for p, _ in exp]))


# ---- entry points that reject unaligned data by contract ------------------------------------------------------------------------------------
def test_alignment_contract_of_the_datetime_functions_and_the_fused_sum(gpu):
    """dbhip_dt_* and dbhip_sum_a_plus_b_mul_c_i64 want 16-byte aligned data: a slice at row 13 is refused with that
    message, a slice at row 16 — aligned, Bitmap offset 16 — gives the reference result"""
    n = 1029
    rng = np.random.default_rng(1313)
    dates = rng.integers(DR.DATE_MIN, DR.DATE_MAX + 1, n).astype(np.int32)
    other = rng.integers(DR.DATE_MIN, DR.DATE_MAX + 1, n).astype(np.int32)
    delta = rng.integers(-500, 500, n).astype(np.int64)
    valid, dvalid = rng.integers(0, 3, n) > 0, rng.integers(0, 4, n) > 0
    calls = {
        "dt_part": lambda c, d, o: gpu.dt_part(DR.YEAR, c),
        "dt_trunc": lambda c, d, o: gpu.dt_trunc(DR.U_MONTH, c),
        "dt_add": lambda c, d, o: gpu.dt_add(DR.U_MONTH, c, d, errors=gpu.RowErrors(n)),
        "dt_diff": lambda c, d, o: gpu.dt_diff(DR.U_DAY, c, o),
    }
    bad = [both(gpu, T.T_DATE, dates, valid, 13)[0], both(gpu, T.T_I64, delta, dvalid, 13, seed=1)[0], both(gpu, T.T_DATE, other, None, 13, seed=2)[0]]
    for name, call in calls.items():
        with pytest.raises(T.DbhipError, match="16-byte aligned"):
            call(*bad)
    good = [both(gpu, T.T_DATE, dates, valid, 16), both(gpu, T.T_I64, delta, dvalid, 16, seed=1), both(gpu, T.T_DATE, other, None, 16, seed=2)]
    added, raised = DR.add(DR.U_MONTH, dates, delta, DR.SRC_DATE)
    refs = {"dt_part": (DR.part(DR.YEAR, dates, DR.SRC_DATE), valid), "dt_trunc": (DR.trunc(DR.U_MONTH, 0, dates, DR.SRC_DATE, DR.SRC_DATE), valid),
            "dt_add": (added, valid & dvalid), "dt_diff": (DR.diff(DR.U_DAY, dates, other, DR.SRC_DATE), valid)}
    for name, call in calls.items():
        for which in (0, 1):
            res = call(*[g[which] for g in good])
            exp, ev = refs[name]
            keep = ev & (~raised if name == "dt_add" else True)          # (a NULL row and a row that raised hold no result)
            assert np.array_equal(res.to_numpy()[:n].astype(np.int64)[keep], np.asarray(exp, dtype=np.int64)[keep]), name
            assert np.array_equal(res.validity_numpy(), ev), name
    assert gpu.dt_part(DR.YEAR, good[0][0]).voff == 16
    a, b, c = (rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64) for _ in range(3))
    with pytest.raises(T.DbhipError, match="16-byte aligned"):
        gpu.sum_a_plus_b_mul_c(*(both(gpu, T.T_I64, x, None, 13, seed=i)[0] for i, x in enumerate((a, b, c))))
    exp = int((a.astype(np.uint64) + b.astype(np.uint64) * c.astype(np.uint64)).sum(dtype=np.uint64).astype(np.int64))
    for which in (0, 1):
        assert gpu.sum_a_plus_b_mul_c(*(both(gpu, T.T_I64, x, None, 16, seed=i)[which] for i, x in enumerate((a, b, c)))) == exp
