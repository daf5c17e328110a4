"""GPU: the fused expression interpreter (csrc/dev_expr.h behind dbhip_expr_eval, and behind the fused aggregation of k_fagg.hip)
against tests/expr_ref.py — never against another kernel. Every launch here writes into buffers fenced by 64 bytes of 0xA5 on both
sides (values at exactly n * elem bytes, both Bitmaps at ceil(n/64) * 8, the error Bitmap at ceil(n/32) * 4): the fences must survive,
the bits past n of the value / validity Bitmaps must be zero, every bit of the error Bitmap that is not a raising row must still be
one, and a refused program must leave every byte as it was."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import expr_cases as EC
from tests import expr_ref as R
from tests import float_ref as FR
from tests import slice_cases as SC

pytestmark = pytest.mark.gpu

FENCE, FILL = 64, 0xA5


def elem_bytes(t):
    return 16 if t == T.T_DEC128 else np.dtype(R.NP[t]).itemsize


class Fenced:
    """a device buffer of exactly `nbytes` with FENCE bytes of FILL on either side, the payload FILLed too"""

    def __init__(self, gpu, nbytes):
        self.nbytes = nbytes
        self.buf = gpu.DeviceBuffer.from_numpy(np.full(nbytes + 2 * FENCE, FILL, np.uint8))
        self.ptr = self.buf.ptr + FENCE

    def read(self):
        raw = self.buf.to_numpy(np.uint8, self.nbytes + 2 * FENCE)
        assert (raw[:FENCE] == FILL).all() and (raw[FENCE + self.nbytes:] == FILL).all(), "the kernel wrote outside its buffer"
        return raw[FENCE:FENCE + self.nbytes]

    def untouched(self):
        return bool((self.read() == FILL).all())


def device_column(gpu, c, lo=0):
    """expr_ref.Input -> device Column (lo > 0: rows [lo, lo + n) of a longer column, the validity at a bit offset)"""
    p, s = c.precision, c.scale
    if c.is_scalar:
        valid = None if c.validity is None else bool(c.validity[0])
        if c.dtype == T.T_BOOL:
            col = gpu.Column.boolean(c.values)
            col.is_scalar = True
            if valid is not None:
                col.validity, col.voff = gpu.DeviceBuffer.from_numpy(SC.scalar_bitmap(valid, 5)), 5
            return col
        v = c.values[0]
        return gpu.Column.scalar(v, c.dtype, p, s) if valid is None else SC.nullable_scalar(gpu, v, c.dtype, valid, 5, p, s)
    if c.dtype == T.T_DEC128:
        make = lambda v, m: gpu.Column.decimal128(v, p, s, validity=m)         # noqa: E731
    elif c.dtype == T.T_BOOL:
        make = lambda v, m: gpu.Column.boolean(v, validity=m)                  # noqa: E731
    else:
        make = lambda v, m: gpu.Column.from_numpy(v, c.dtype, validity=m, precision=p, scale=s)   # noqa: E731
    return SC.sliced(gpu, make, c.values, c.validity, lo) if lo else make(c.values, c.validity)


def c_program(ins):
    prog = (T.ExprIns * max(len(ins), 1))()
    for k, (op, dst, a, b, typ, imm, size) in enumerate(ins):
        prog[k].op, prog[k].dst, prog[k].a, prog[k].b, prog[k].type, prog[k].imm = op, dst, a, b, typ, imm
        prog[k].precision, prog[k].scale = size
    return prog


def launch(gpu, ins, inputs, n, out, out_type, want_sum=False, lo=0):
    """dbhip_expr_eval into fenced buffers -> dict(rc, values, validity, raising, err_count, sum) (values .. sum: None when refused)"""
    from databend_amd.device import _cols, bytes_to_i128
    cols = [device_column(gpu, c, lo) for c in inputs]
    words = (n + 63) // 64
    vals = Fenced(gpu, words * 8 if out_type == T.T_BOOL else n * elem_bytes(out_type))
    valid, err = Fenced(gpu, words * 8), Fenced(gpu, ((n + 31) // 32) * 4)
    cnt, sm = gpu.DeviceBuffer(8).zero(), gpu.DeviceBuffer(8).zero()
    rc = T.lib().dbhip_expr_eval(c_program(ins), len(ins), _cols(cols), len(cols), C.c_int64(n), out, C.c_void_p(vals.ptr), C.c_void_p(valid.ptr),
                                 C.c_void_p(err.ptr), C.c_void_p(cnt.ptr), C.c_void_p(sm.ptr) if want_sum else None, None)
    res = dict(rc=rc, values=None, validity=None, raising=None, err_count=None, sum=None)
    if rc != T.OK:
        assert vals.untouched() and valid.untouched() and err.untouched(), "a refused program wrote to its outputs"
        assert int(cnt.to_numpy(np.uint64, 1)[0]) == 0
        return res
    raw = vals.read()
    if out_type == T.T_BOOL:
        bits = np.unpackbits(raw, bitorder="little")
        assert not bits[n:].any(), "value bits past n"
        res["values"] = bits[:n].astype(bool)
    elif out_type == T.T_DEC128:
        res["values"] = bytes_to_i128(raw)
    else:
        res["values"] = raw.view(R.NP[out_type]).copy()
    vbits = np.unpackbits(valid.read(), bitorder="little")
    assert not vbits[n:].any(), "validity bits past n"
    res["validity"] = vbits[:n].astype(bool)
    ebits = np.unpackbits(err.read(), bitorder="little").astype(bool)
    assert ebits[n:].all(), "error bits past n were cleared"
    res["raising"] = np.flatnonzero(~ebits[:n])
    res["err_count"] = int(cnt.to_numpy(np.uint64, 1)[0])
    if want_sum:
        res["sum"] = sm.to_numpy(np.float64 if R.INFO[out_type][1] == "f" else (np.int64 if R.INFO[out_type][1] == "s" else np.uint64), 1)[0]
    return res


def check(gpu, oracle, ins, inputs, n, out, want_sum=False, lo=0, use_numpy=True, tag=None):
    """run the program on the device and through the reference; values (on the valid rows), validity, raising rows, err_count"""
    exp = R.run(ins, inputs, n, out, oracle, use_numpy=use_numpy)
    got = launch(gpu, ins, inputs, n, out, exp.type, want_sum=want_sum, lo=lo)
    assert got["rc"] == T.OK, (tag, got["rc"], T.lib().dbhip_last_error())
    ev = np.ones(n, bool) if exp.validity is None else exp.validity
    assert np.array_equal(got["validity"], ev), (tag, "validity")
    assert np.array_equal(got["raising"], exp.raising) and got["err_count"] == exp.raise_events, (tag, "raising rows", got["raising"][:8], exp.raising[:8], got["err_count"], exp.raise_events)
    if exp.type == T.T_DEC128:
        bad = [i for i in np.flatnonzero(ev).tolist() if got["values"][i] != exp.values[i]]
    else:
        g, e = np.asarray(got["values"])[ev], np.asarray(exp.values)[ev]
        bad = [] if R.same(g, e) else np.flatnonzero(ev)[[not R.same(g[i:i + 1], e[i:i + 1]) for i in range(len(g))]].tolist()
    assert not bad, (tag, "values", bad[:5], [got["values"][i] for i in bad[:5]], [exp.values[i] for i in bad[:5]])
    if want_sum:
        if R.INFO[exp.type][1] == "f":
            assert FR.sum_ok(got["sum"], FR.sum_expected(np.asarray(exp.values)[ev].astype(np.float64))), (tag, "sum", got["sum"])
        else:
            assert int(got["sum"]) == R.wrapping_sum(exp.values, ev, exp.type), (tag, "sum")
    return exp, got


def column(rng, t, n, size=(0, 0), nullable=False, for_sum=False, tame=False):
    v = EC.fill(rng, t, n, size, tame=tame)
    if for_sum and t in (T.T_F32, T.T_F64):
        v = FR.mixed(rng, n, R.NP[t], for_sum=True)
    if n > 1 and not isinstance(v, list):
        v = v[rng.permutation(n)]                                  # pool values meet pool values of the other operand at random
    return R.Input(t, v, (rng.random(n) < 0.75) if nullable else None, False, *size)


def scalar(rng, t, size=(0, 0), valid=None):
    p = EC.pool(t, size)
    return R.Input(t, [p[int(rng.integers(0, len(p)))]], None if valid is None else [valid], True, *size)


def ld(reg, c, t, size=(0, 0)):
    return (T.EX_LOAD, reg, c, 0, t, 0, size)


# ---- arithmetic --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ta", R.NUMBERS)
def test_arithmetic_on_every_type_pair(gpu, oracle, ta):
    """(lhs, rhs) x + - * / as one node (nullable lhs) and as a chain whose second operand has a third type; a scalar on either side
    (a nullable one too). Two of the SIZES per pair, all of them per lhs type."""
    i = R.NUMBERS.index(ta)
    for j, tb in enumerate(R.NUMBERS):
        tc = R.NUMBERS[(i + 3 * j + 1) % 10]
        for n in (EC.SIZES[(10 * i + j) % 15], EC.SIZES[(10 * i + j + 7) % 15]):
            rng = np.random.default_rng([i, j, n])
            a, b, c = column(rng, ta, n, nullable=True), column(rng, tb, n), column(rng, tc, n, nullable=j % 2 == 0)
            for k, op in enumerate(R.ARITH):
                t1 = R.arith_result_type(op, ta, tb)
                check(gpu, oracle, [ld(0, 0, ta), ld(1, 1, tb), (op, 2, 0, 1, t1, 0, (0, 0))], [a, b], n, 2, tag=(op, ta, tb, n))
                op2 = R.ARITH[(k + j) % 4]
                t2 = R.arith_result_type(op2, t1, tc)
                check(gpu, oracle, [ld(0, 0, ta), ld(1, 1, tb), (op, 0, 0, 1, t1, 0, (0, 0)), ld(1, 2, tc), (op2, 0, 0, 1, t2, 0, (0, 0))], [a, b, c], n, 0,
                      tag=("chain", op, op2, ta, tb, tc, n))
            op = R.ARITH[(i + j) % 4]
            t1 = R.arith_result_type(op, ta, tb)
            sb = scalar(rng, tb, valid=None if j % 3 else bool(j % 2))
            check(gpu, oracle, [ld(0, 0, ta), ld(1, 1, tb), (op, 2, 0, 1, t1, 0, (0, 0))], [a, sb], n, 2, tag=("scalar rhs", op, ta, tb, n))
            sa = scalar(rng, ta, valid=None if i % 3 else bool(j % 2))
            check(gpu, oracle, [ld(0, 0, ta), ld(1, 1, tb), (op, 2, 0, 1, t1, 0, (0, 0))], [sa, b], n, 2, tag=("scalar lhs", op, ta, tb, n))
    # a zero divisor of every kind: 0, -0.0 raise, NaN does not; under a NULL nothing raises
    n = 257
    rng = np.random.default_rng(i)
    a = column(rng, ta, n, nullable=True)
    z = np.zeros(n, np.float64)
    z[1::3], z[2::3] = -0.0, np.nan
    exp, got = check(gpu, oracle, [ld(0, 0, ta), ld(1, 1, T.T_F64), (T.EX_DIVIDE, 2, 0, 1, T.T_F64, 0, (0, 0))], [a, R.Input(T.T_F64, z)], n, 2)
    assert np.array_equal(exp.raising, np.flatnonzero(a.validity & (np.arange(n) % 3 != 2)))


# ---- comparisons -------------------------------------------------------------------------------------------------------------------
SIZE_OF = {T.T_DEC64: (15, 2), T.T_DEC128: (30, 4)}


def const_ins(reg, t, value, size=(0, 0)):
    """instructions that leave a constant of type t in `reg` (Decimal128: a Decimal64 constant widened by CAST)"""
    if t == T.T_DEC128:
        return [(T.EX_CONST, reg, 0, 0, T.T_DEC64, EC.const_imm(T.T_DEC64, value), (18, size[1])), (T.EX_CAST, reg, reg, 0, T.T_DEC128, 0, size)]
    return [(T.EX_CONST, reg, 0, 0, t, EC.const_imm(t, int(value) if t == T.T_BOOL else value), size)]


@pytest.mark.parametrize("t", EC.ALL_TYPES)
def test_comparisons_at_the_class_edges(gpu, oracle, t):
    """every comparison on every operand type, column-column (the pool against itself: UInt64 around 2^63, NaN and signed zeros,
    Decimal64 negatives, Decimal128 values that differ in the high word only, Boolean, Date, Timestamp) and column-constant"""
    size = SIZE_OF.get(t, (0, 0))
    pool = list(EC.pool(t, size))
    k = EC.ALL_TYPES.index(t)
    for n in (1025, EC.SIZES[k]):
        rng = np.random.default_rng([k, n])
        a, b = column(rng, t, n, size, nullable=True), column(rng, t, n, size)
        va, vb = (list(a.values), list(b.values)) if t == T.T_DEC128 else (a.values, b.values)
        m = 0
        for x in pool:                                            # the pool against itself, as far as n allows
            for y in pool:
                if m < n:
                    va[m], vb[m] = x, y
                    m += 1
        a, b = R.Input(t, va, a.validity, False, *size), R.Input(t, vb, None, False, *size)
        for op in R.CMPS:
            check(gpu, oracle, [ld(0, 0, t, size), ld(1, 1, t, size), (op, 2, 0, 1, T.T_BOOL, 0, (0, 0))], [a, b], n, 2, use_numpy=n > 300, tag=(op, t, n))
        consts = [pool[0], pool[len(pool) // 2], pool[-1]]
        if t == T.T_DEC128:
            consts = [7, -7, 10 ** 17]                             # (a Decimal128 constant is a widened Decimal64 one)
        for ci, cv in enumerate(consts):
            op = R.CMPS[(ci + k) % 6]
            check(gpu, oracle, [ld(0, 0, t, size)] + const_ins(1, t, cv, size) + [(op, 2, 0, 1, T.T_BOOL, 0, (0, 0))], [a], n, 2, tag=("const", op, t, cv))
            check(gpu, oracle, [ld(0, 0, t, size)] + const_ins(1, t, cv, size) + [(R.CMPS[5 - (ci + k) % 6], 2, 1, 0, T.T_BOOL, 0, (0, 0))], [a], n, 2,
                  tag=("const lhs", t, cv))


# ---- CAST --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", R.NUMBERS + (T.T_DEC64,))
def test_cast_matrix(gpu, oracle, src):
    """the whole 10 x 10 matrix and Decimal64 -> Decimal128: a lossless pair equals the reference, alone and feeding a later +
    (the only way a Float32 register comes to be); every other pair is DBHIP_ERR_UNSUPPORTED and writes nothing"""
    size = (15, 2) if src == T.T_DEC64 else (0, 0)
    for j, dst in enumerate(R.NUMBERS + (T.T_DEC128,)):
        if (src == T.T_DEC64) != (dst == T.T_DEC128):
            if src == T.T_DEC64 or dst == T.T_DEC128:             # number <-> decimal: refused (checked below for two pairs)
                if dst not in (T.T_I64, T.T_DEC128):
                    continue
        n = EC.SIZES[(3 * EC.ALL_TYPES.index(src) + j) % 15]
        rng = np.random.default_rng([src, dst])
        a = column(rng, src, n, size, nullable=True)
        dsize = (38, 2) if dst == T.T_DEC128 else (0, 0)
        prog = [ld(0, 0, src, size), (T.EX_CAST, 1, 0, 0, dst, 0, dsize)]
        if not R.lossless_cast(src, dst):
            with pytest.raises(R.Refused):
                R.run(prog, [a], n, 1, oracle)
            assert launch(gpu, prog, [a], n, 1, dst)["rc"] == T.ERR_UNSUPPORTED, (src, dst)
            continue
        check(gpu, oracle, prog, [a], n, 1, tag=("cast", src, dst, n))
        tb = T.T_DEC64 if dst == T.T_DEC128 else R.NUMBERS[(j + 5) % 10]
        bsize = (9, 0) if tb == T.T_DEC64 else (0, 0)
        b = column(rng, tb, n, bsize, tame=True)
        if dst == T.T_DEC128:
            ot, p, s = R.decimal_result(oracle, T.EX_PLUS, R.Val(dst, None, size=dsize), R.Val(tb, None, size=bsize))
        else:
            ot, p, s = R.arith_result_type(T.EX_PLUS, dst, tb), 0, 0
        check(gpu, oracle, prog + [ld(2, 1, tb, bsize), (T.EX_PLUS, 0, 1, 2, ot, 0, (p, s))], [a, b], n, 0, tag=("cast then +", src, dst, tb, n))


# ---- IF ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", EC.ALL_TYPES)
def test_if_over_every_value_class(gpu, oracle, t):
    """if(cond, then, else) with column, scalar and constant branches; the result's validity is then | else"""
    size = SIZE_OF.get(t, (0, 0))
    k = EC.ALL_TYPES.index(t)
    for n in (EC.SIZES[k], EC.SIZES[(k + 8) % 15]):
        rng = np.random.default_rng([k, n, 7])
        cond = R.Input(T.T_BOOL, rng.integers(0, 2, n).astype(bool))
        x, y = column(rng, t, n, size, nullable=True), column(rng, t, n, size, nullable=True)
        cv = 7 if t in R.DECIMALS else EC.pool(t, size)[1]
        head = [ld(0, 0, T.T_BOOL), ld(1, 1, t, size)]
        check(gpu, oracle, head + [ld(2, 2, t, size), (T.EX_IF, 3, 0, 1, t, 2, size)], [cond, x, y], n, 3, tag=("if col col", t, n))
        check(gpu, oracle, head + [ld(2, 2, t, size), (T.EX_IF, 3, 0, 1, t, 2, size)], [cond, x, scalar(rng, t, size, valid=bool(k % 2))], n, 3, tag=("if col scalar", t, n))
        check(gpu, oracle, head + const_ins(2, t, cv, size) + [(T.EX_IF, 3, 0, 2, t, 1, size)], [cond, x], n, 3, tag=("if const col", t, n))
        check(gpu, oracle, [ld(0, 0, T.T_BOOL)] + const_ins(1, t, cv, size) + const_ins(2, t, 0, size) + [(T.EX_IF, 1, 0, 1, t, 2, size)], [cond], n, 1,
              tag=("if const const", t, n))
        # the condition computed in the program, over a nullable operand, decoded by IS_TRUE
        check(gpu, oracle, head + [ld(2, 2, t, size), (T.EX_LT, 3, 1, 2, T.T_BOOL, 0, (0, 0)), (T.EX_IS_TRUE, 3, 3, 0, T.T_BOOL, 0, (0, 0)),
                                   (T.EX_IF, 1, 3, 1, t, 2, size)], [cond, x, y], n, 1, tag=("if computed", t, n))


# ---- want_sum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", R.NUMBERS + (T.T_DATE, T.T_TIMESTAMP, T.T_DEC64))
def test_sum_of_every_result_class(gpu, oracle, t):
    """integer results: the wrapping sum of the valid rows, exactly; float results: inside float_ref.sum_ok of the valid rows' terms"""
    size = SIZE_OF.get(t, (0, 0))
    k = EC.ALL_TYPES.index(t)
    for n in (EC.SIZES[(k + 3) % 15], 4099):
        rng = np.random.default_rng([k, n, 11])
        cond = R.Input(T.T_BOOL, rng.integers(0, 2, n).astype(bool))
        x, y = column(rng, t, n, size, nullable=True, for_sum=True), column(rng, t, n, size, for_sum=True)
        check(gpu, oracle, [ld(0, 0, T.T_BOOL), ld(1, 1, t, size), ld(2, 2, t, size), (T.EX_IF, 3, 0, 1, t, 2, size)], [cond, x, y], n, 3, want_sum=True, tag=("sum if", t, n))
        check(gpu, oracle, [ld(0, 0, t, size)], [x], n, 0, want_sum=True, tag=("sum input", t, n))
        if t in R.NUMBERS and R.INFO[t][1] != "f":
            ot = R.arith_result_type(T.EX_MULTIPLY, t, t)
            check(gpu, oracle, [ld(0, 0, t), ld(1, 1, t), (T.EX_MULTIPLY, 2, 0, 1, ot, 0, (0, 0))], [x, y], n, 2, want_sum=True, tag=("sum product", t, n))


# ---- random programs ---------------------------------------------------------------------------------------------------------------
SLICED = EC.Klass(4, False, False, False)


@pytest.mark.parametrize("ci", range(len(EC.seed_list())))
def test_generated_programs(gpu, oracle, ci):
    """every committed seed at two of the SIZES; the seeds of one class on sliced inputs (row offset 13, validity at a bit offset).
    A program the library refuses is a failure: the generator stays inside the documented limits (tests/test_expr_ref_cpu.py)."""
    case = EC.cases(oracle)[ci]
    for n in (EC.SIZES[ci % 15], EC.SIZES[(ci + 6) % 15]):
        check(gpu, oracle, case.ins, EC.make_inputs(case, n), n, case.root, lo=13 if case.klass == SLICED else 0, tag=(case.seed, case.klass, n),
              want_sum=case.root_type in R.NUMBERS + (T.T_DATE, T.T_TIMESTAMP, T.T_DEC64) and ci % 4 == 0 and case.root_type not in (T.T_F32, T.T_F64))


# ---- the second trip of the grid-stride loop ---------------------------------------------------------------------------------------
def big_inputs(types, n, seed, sizes=None):
    rng = np.random.default_rng(seed)
    out = []
    for i, t in enumerate(types):
        size = sizes[i] if sizes else (0, 0)
        if t == T.T_F64:
            v = rng.standard_normal(n) * 10.0 ** rng.integers(-20, 20, n)
        elif t == T.T_DEC64:
            v = rng.integers(-10 ** 9, 10 ** 9, n)
            v[rng.random(n) < 0.01] = 0
        else:
            v = rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64)
        out.append(R.Input(t, v, (rng.random(n) < 0.9) if i == 0 else None, False, *size))
    return out


def test_second_grid_trip_four_rows_per_lane(gpu, oracle):
    """n = 1 048 576 + 257: with at most 8 live slots a wave covers 256 rows and the grid 1024 x 4 waves, so the first waves come round
    a second time and reuse their LDS register file"""
    n = 1_048_576 + 257
    ins = [ld(0, 0, T.T_I64), ld(1, 1, T.T_I64), ld(2, 2, T.T_F64), (T.EX_MULTIPLY, 3, 1, 1, T.T_I64, 0, (0, 0)), (T.EX_PLUS, 3, 0, 3, T.T_I64, 0, (0, 0)),
           (T.EX_MULTIPLY, 3, 3, 2, T.T_F64, 0, (0, 0)), (T.EX_LT, 4, 3, 2, T.T_BOOL, 0, (0, 0)), (T.EX_IS_TRUE, 4, 4, 0, T.T_BOOL, 0, (0, 0)),
           (T.EX_IF, 0, 4, 3, T.T_F64, 2, (0, 0))]
    specs = [EC.Spec(t, False, False, (0, 0)) for t in (T.T_I64, T.T_I64, T.T_F64)]
    assert EC.live_width(ins, specs, 0) <= 8
    check(gpu, oracle, ins, big_inputs((T.T_I64, T.T_I64, T.T_F64), n, 1), n, 0, tag="rows 4")


def test_second_grid_trip_two_rows_per_lane(gpu, oracle):
    """n = 524 288 + 129 with more than 8 live slots (2 rows per lane: a wave covers 128 rows)"""
    n = 524_288 + 129
    types = (T.T_I64, T.T_F64, T.T_I64, T.T_F64, T.T_I64, T.T_I64, T.T_F64, T.T_I64)
    ins = [ld(c, c, t) for c, t in enumerate(types)]
    ins += [(T.EX_PLUS, 8, 0, 2, T.T_I64, 0, (0, 0)), (T.EX_MULTIPLY, 9, 1, 3, T.T_F64, 0, (0, 0)), (T.EX_MINUS, 10, 4, 5, T.T_I64, 0, (0, 0)),
            (T.EX_MULTIPLY, 8, 8, 10, T.T_I64, 0, (0, 0)), (T.EX_PLUS, 9, 9, 6, T.T_F64, 0, (0, 0)), (T.EX_MINUS, 8, 8, 7, T.T_I64, 0, (0, 0)),
            (T.EX_PLUS, 8, 8, 0, T.T_I64, 0, (0, 0)), (T.EX_MINUS, 8, 8, 2, T.T_I64, 0, (0, 0)), (T.EX_MULTIPLY, 8, 8, 9, T.T_F64, 0, (0, 0)), (T.EX_MINUS, 8, 8, 1, T.T_F64, 0, (0, 0))]
    specs = [EC.Spec(t, False, False, (0, 0)) for t in types]
    assert EC.live_width(ins, specs, 8) >= 9
    check(gpu, oracle, ins, big_inputs(types, n, 2), n, 8, tag="rows 2")


def test_second_grid_trip_dividing_kernel(gpu, oracle):
    """n = 524 288 + 129 through the instantiation with the long divisions: a rounding Decimal(15,8) multiply, then a divide"""
    n = 524_288 + 129
    sz = (15, 8)
    ins = [ld(0, 0, T.T_DEC64, sz), ld(1, 1, T.T_DEC64, sz), ld(2, 2, T.T_I64)]
    x = R.Val(T.T_DEC64, None, size=sz)
    t1, p1, s1 = R.decimal_result(oracle, T.EX_MULTIPLY, x, x)
    t2, p2, s2 = R.decimal_result(oracle, T.EX_DIVIDE, R.Val(t1, None, size=(p1, s1)), x)
    ins += [(T.EX_MULTIPLY, 3, 0, 1, t1, 0, (p1, s1)), (T.EX_DIVIDE, 3, 3, 1, t2, 0, (p2, s2)), (T.EX_PLUS, 4, 2, 2, T.T_I64, 0, (0, 0))]
    assert s1 == 12
    inputs = big_inputs((T.T_DEC64, T.T_DEC64, T.T_I64), n, 3, sizes=[sz, sz, (0, 0)])
    inputs[1].values[n - 3], inputs[0].validity[n - 3] = 0, True          # a zero divisor on the second trip
    exp, got = check(gpu, oracle, ins, inputs, n, 3, tag="div")
    assert len(exp.raising) > 100 and exp.raising[-1] == n - 3


# ---- canaries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [T.T_BOOL, T.T_U8, T.T_I16, T.T_I32, T.T_I64, T.T_F32, T.T_DEC128])
def test_outputs_end_where_they_should(gpu, oracle, t):
    """one result per output kind (Bitmap, 1 / 2 / 4 / 8 bytes, Float32, Decimal128) with a raising divide beside it, at sizes around
    the 32- and 64-row words: launch() fences values, validity and the error Bitmap and checks the fences and the bits past n"""
    size = SIZE_OF.get(t, (0, 0))
    for n in (1, 31, 33, 63, 65, 257):
        rng = np.random.default_rng([t, n])
        x, d = column(rng, t, n, size, nullable=True), column(rng, T.T_I8, n)
        check(gpu, oracle, [ld(0, 0, t, size)], [x], n, 0, tag=("canary", t, n))
        exp, _ = check(gpu, oracle, [ld(0, 0, T.T_I8), (T.EX_DIVIDE, 1, 0, 0, T.T_F64, 0, (0, 0))], [d], n, 1, tag=("canary raise", n))
        assert n < 33 or len(exp.raising)


# ---- documented refusals -----------------------------------------------------------------------------------------------------------
def test_documented_refusals_return_their_code_and_write_nothing(gpu, oracle):
    n = 257
    rng = np.random.default_rng(0)
    i64 = column(rng, T.T_I64, n)
    nul = column(rng, T.T_I64, n, nullable=True)
    d128 = column(rng, T.T_DEC128, n, (30, 4), tame=True)
    d64 = column(rng, T.T_DEC64, n, (9, 0), tame=True)
    plus = lambda dst, a, b: (T.EX_PLUS, dst, a, b, T.T_I64, 0, (0, 0))              # noqa: E731

    def refused(ins, inputs, out, out_type=T.T_I64):
        return launch(gpu, ins, inputs, n, out, out_type)["rc"]

    assert refused([ld(0, 0, T.T_I64), plus(16, 0, 0)], [i64], 0) == T.ERR_INVALID                       # register out of range
    assert refused([ld(0, 0, T.T_I64), plus(1, 0, 5)], [i64], 1) == T.ERR_INVALID                        # read of an unset register
    chain = [ld(0, 0, T.T_I64)] + [plus(1 + k % 2, k % 2 if k else 0, 0) for k in range(25)]
    assert refused(chain[:25], [i64], 1) == T.OK                                                          # 24 instructions are fine
    assert refused(chain, [i64], 1) == T.ERR_UNSUPPORTED                                                  # 25 after LOAD elimination
    assert refused([ld(0, 0, T.T_I64)], [i64] * 9, 0) == T.ERR_INVALID                                   # 9 inputs
    three = [ld(c, c, T.T_DEC128, (30, 4)) for c in range(3)]
    assert refused(three, [d128] * 3, 0, T.T_DEC128) == T.ERR_UNSUPPORTED                                 # three Decimal128 inputs
    dec = [ld(0, 0, T.T_DEC64, (9, 0))]
    p = 9
    for k in range(7):
        p += 1
        dec.append((T.EX_PLUS, 1, 1 if k else 0, 0, T.T_DEC64, 0, (p, 0)))
    assert refused(dec[:7], [d64], 1, T.T_DEC64) == T.OK                                                  # six decimal nodes are fine
    assert refused(dec, [d64], 1, T.T_DEC64) == T.ERR_UNSUPPORTED                                         # seven decimal nodes
    assert refused([(T.EX_CONST, 0, 0, 0, T.T_DEC128, 5, (30, 4))], [i64], 0, T.T_DEC128) == T.ERR_INVALID   # CONST of Decimal128
    raising = [ld(0, 0, T.T_I64), (T.EX_DIVIDE, 1, 0, 0, T.T_F64, 0, (0, 0)), (T.EX_CONST, 2, 0, 0, T.T_F64, 0, (0, 0)),
               (T.EX_GT, 3, 0, 0, T.T_BOOL, 0, (0, 0)), (T.EX_IF, 4, 3, 1, T.T_F64, 2, (0, 0))]
    assert refused(raising, [i64], 4, T.T_F64) == T.ERR_UNSUPPORTED                                       # IF with a raising branch
    with pytest.raises(R.Refused):
        R.run(raising, [i64], n, 4, oracle)
    nullable_cond = [ld(0, 0, T.T_I64), ld(1, 1, T.T_I64), (T.EX_GT, 2, 0, 1, T.T_BOOL, 0, (0, 0)), (T.EX_IF, 3, 2, 0, T.T_I64, 1, (0, 0))]
    assert refused(nullable_cond, [nul, i64], 3) == T.ERR_UNSUPPORTED                                     # IF on a nullable condition
    with pytest.raises(R.Refused):
        R.run(nullable_cond, [nul, i64], n, 3, oracle)
    # more live slots than the register file holds: k Decimal128 copies of one column (2 slots each) alive at once, then folded by IF
    def copies(k):
        ins = [ld(0, 0, T.T_DEC64, (9, 0))] + [(T.EX_CAST, c, 0, 0, T.T_DEC128, 0, (38, 0)) for c in range(1, k + 1)]
        ins.append((T.EX_CONST, 13, 0, 0, T.T_BOOL, 1, (0, 0)))
        return ins + [(T.EX_IF, c - 1, 13, c - 1, T.T_DEC128, c, (38, 0)) for c in range(k, 1, -1)]
    assert len(copies(12)) - 1 == 24 and EC.live_width(copies(12), [EC.Spec(T.T_DEC64, False, False, (9, 0))], 1) == 25
    assert refused(copies(12), [d64], 1, T.T_DEC128) == T.ERR_UNSUPPORTED
    check(gpu, oracle, copies(7), [d64], n, 1, tag="15 live slots")


# ---- the same programs through the fused aggregation -------------------------------------------------------------------------------
FA_ROOTS = (T.T_DEC128, T.T_DEC64, T.T_F64, T.T_F64, T.T_F64, T.T_I32)      # the root types of the six shapes (arithmetic ends in Float64 or a decimal)
FA_SIZES = (129, 4099)
FA_PREPARED = (1,)          # the shape that also goes through prepare_program: a compile each (this one 2 s; the Decimal128 shape 10 s, two Float64 shapes 23 s and 40 s)
F_REG = 15                                                                   # the filter's register; 13 and 14 are its temporaries


def fagg_filter(case):
    """and_filters(in_a <op> const, in_b <op> const) over the first two narrow inputs of the case, as LEADING instructions"""
    cols = [c for c, s in enumerate(case.specs) if s.dtype != T.T_DEC128][:2]
    ins = []
    for j, c in enumerate(cols):
        s, r = case.specs[c], 13 + j
        cv = 0 if s.dtype in R.DECIMALS + (T.T_DATE, T.T_TIMESTAMP, T.T_BOOL) + R.NUMBERS[8:] else R.value_range(s.dtype)[1] // 3
        ins += [ld(r, c, s.dtype, s.size)] + const_ins(F_REG, s.dtype, cv, s.size)
        ins += [((T.EX_GTE, T.EX_LTE)[j], r, r, F_REG, T.T_BOOL, 0, (0, 0)), (T.EX_IS_TRUE, r, r, 0, T.T_BOOL, 0, (0, 0))]
    if len(cols) == 1:
        return ins + [(T.EX_IS_TRUE, F_REG, 13, 0, T.T_BOOL, 0, (0, 0))]
    return ins + [(T.EX_AND, F_REG, 13, 14, T.T_BOOL, 0, (0, 0))]


def fagg_shapes(oracle):
    """six generated programs with the root types of FA_ROOTS that leave room for the filter (registers 13..15, 7 instructions,
    one slot) and raise on no row of the data used here — the raising rows have a test of their own below"""
    out = []
    for want in FA_ROOTS:
        for case in EC.cases(oracle):
            body = [i for i in case.ins if i[0] != T.EX_LOAD]
            if case.root_type != want or case in out or max(i[1] for i in case.ins) > 12 or len(body) > 15 or case.live > 8 or not body:
                continue
            if any(s.dtype == T.T_DEC128 for s in case.specs[:1]) and len(case.specs) == 1:
                continue
            runs = [R.run(case.ins, EC.make_inputs(case, n), n, case.root, oracle, use_numpy=True) for n in FA_SIZES]
            tame = case.root_type != T.T_F64 or all(np.all(np.abs(r.values[np.isfinite(r.values)]) <= FR.MAX_SUM_ABS) for r in runs)   # float_ref.sum_ok's domain
            if all(len(r.raising) == 0 for r in runs) and tame and (want == T.T_I32 or len(set(np.asarray(runs[-1].values, dtype=object).tolist())) >= 8):   # not a constant (the narrow integer roots are if()s over constants)
                out.append(case)
                break
    assert [c.root_type for c in out] == list(FA_ROOTS), "the seed list no longer holds a shape for every root type"
    return out


def fagg_aggs(case, nullable):
    t, (p, s) = case.root_type, case.root_size
    kinds = (T.AGG_SUM, T.AGG_COUNT) if t == T.T_DEC128 else (T.AGG_SUM, T.AGG_MIN, T.AGG_MAX, T.AGG_COUNT)   # (min / max over Decimal128 stay on the row path)
    return [(k, t, p, s, int(nullable)) for k in kinds] + [(T.AGG_COUNT, 0, 0, 0, 0)]


def fagg_expected(case, ins, inputs, n, key, kv, oracle):
    val = R.run(ins, inputs, n, case.root, oracle, use_numpy=True)
    flt = R.run(ins, inputs, n, F_REG, oracle, use_numpy=True)
    assert flt.validity is None and flt.type == T.T_BOOL
    keep = flt.values
    assert not len(np.intersect1d(val.raising, np.flatnonzero(keep)))
    arg = val.values if isinstance(val.values, list) else np.asarray(val.values)
    nargs = 2 if case.root_type == T.T_DEC128 else 4
    exp = FR.agg_expected([key], [kv], [arg] * nargs + [None], [val.validity] * nargs + [None], keep)
    cls = R.INFO[case.root_type][1]
    for per_group in exp.values():
        d = per_group[0]
        if d["sum"] is not None and cls in ("s", "u"):
            d["sum"] = R.wrap_py(d["sum"], 64, cls == "s")              # integer and Decimal64 sums wrap at 64 bits
    return exp, val, keep


@pytest.mark.parametrize("si", range(len(FA_ROOTS)))
def test_generated_programs_through_the_fused_aggregation(gpu, oracle, si):
    """filter (and_filters over two inputs) and aggregate argument as roots of ONE program in add_block_program: sum / min / max /
    count / count(*) by a nullable UInt8 key with three values, against expr_ref and plain Python grouping over the rows whose
    filter is TRUE; for the shape of FA_PREPARED then a fresh table after prepare_program (the run-time specialised kernel)"""
    case = fagg_shapes(oracle)[si]
    ins = fagg_filter(case) + list(case.ins)
    dt = None if case.root_type in R.DECIMALS else R.NP[case.root_type]
    for n in FA_SIZES:
        inputs = EC.make_inputs(case, n)
        rng = np.random.default_rng([si, n])
        key, kv = rng.integers(0, 3, n).astype(np.uint8), rng.random(n) < 0.8
        exp, val, keep = fagg_expected(case, ins, inputs, n, key, kv, oracle)
        assert 0 < keep.sum() < n or n < 200
        aggs = fagg_aggs(case, val.validity is not None)
        kinds = [("count" if a[0] == T.AGG_COUNT else ("sum", "min", "max")[a[0] - 1], dt if a[1] else None) for a in aggs]
        for prepare in (False, True):
            p = gpu.ExprProgram([device_column(gpu, c) for c in inputs])
            p.ins = list(ins)
            keys = [gpu.Column.from_numpy(key, validity=kv)]
            g = gpu.GroupBy([T.T_U8], aggs, key_nullable=[1])
            regs = [case.root] * (len(aggs) - 1) + [None]
            if prepare and si not in FA_PREPARED:
                continue
            if prepare:
                g.prepare_program(keys, p, regs, filter_reg=F_REG)
            g.add_block_program(keys, p, regs, n, filter_reg=F_REG)
            assert FR.mismatches(g.result(), exp, [np.uint8], kinds) == [], (case.seed, n, prepare)


def test_fused_aggregation_raises_only_for_rows_the_filter_keeps(gpu, oracle):
    """a / b with zero divisors: on rows the filter drops nothing is raised; on a row it keeps the block fails with
    DBHIP_ERR_ROW_ERRORS and the table is unchanged"""
    n = 4099
    rng = np.random.default_rng(9)
    a, b = rng.integers(-1000, 1000, n).astype(np.int64), rng.integers(1, 50, n).astype(np.int64)
    flag = (rng.random(n) < 0.5).astype(np.int64)
    flag[[5, 1000, 4098]] = (0, 0, 1)
    b[flag == 0] = 0                                               # every dropped row would divide by zero
    key = rng.integers(0, 3, n).astype(np.uint8)
    ins = [ld(0, 2, T.T_I64)] + const_ins(1, T.T_I64, 1) + [(T.EX_EQ, F_REG, 0, 1, T.T_BOOL, 0, (0, 0)), ld(0, 0, T.T_I64), ld(1, 1, T.T_I64),
                                                            (T.EX_DIVIDE, 2, 0, 1, T.T_F64, 0, (0, 0))]
    aggs = [(T.AGG_SUM, T.T_F64, 0, 0, 0), (T.AGG_COUNT, 0, 0, 0, 0)]

    def add(g, bcol):
        p = gpu.ExprProgram([gpu.Column.from_numpy(a), gpu.Column.from_numpy(bcol), gpu.Column.from_numpy(flag)])
        p.ins = list(ins)
        g.add_block_program([gpu.Column.from_numpy(key)], p, [2, None], n, filter_reg=F_REG)

    inputs = [R.Input(T.T_I64, a), R.Input(T.T_I64, b), R.Input(T.T_I64, flag)]
    val = R.run(ins, inputs, n, 2, oracle, use_numpy=True)
    assert len(val.raising) == int((flag == 0).sum()) > 1000       # the reference alone, without the filter, raises on every dropped row
    exp = FR.agg_expected([key], [None], [val.values, None], [None, None], flag == 1)
    g = gpu.GroupBy([T.T_U8], aggs)
    add(g, b)
    rows = g.result()
    assert FR.mismatches(rows, exp, [np.uint8], [("sum", np.float64), ("count", None)]) == []
    b2 = b.copy()
    b2[4098] = 0                                                   # a kept row divides by zero
    with pytest.raises(T.DbhipError) as e:
        add(g, b2)
    assert e.value.code == T.ERR_ROW_ERRORS
    assert sorted(g.result()) == sorted(rows)
