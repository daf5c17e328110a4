"""GPU: Decimal64 / Decimal128 arithmetic (dev_decimal.h: dec_row, dec_row_nodiv; the division helpers of dev_common.h) at its branch
edges — the directed cases of tests/dec_edge_cases.py, which tests/test_dec_edges_cpu.py pins on the Python statement, through the
column kernel (dbhip_decimal_arith: column x column at several lengths, scalars on either side, nullable operands) and through the fused
expression interpreter (dbhip_expr_eval: one node, and a rounding multiply feeding a divide). Exact integers throughout: values, the
raising rows, the error count, the value 1 on raised rows, result type and size."""
import numpy as np
import pytest

from databend_amd import _lib as T
from tests import dec256_cases as K
from tests import dec256_ref as R
from tests import dec_edge_cases as E

pytestmark = pytest.mark.gpu

EX = {R.OP_PLUS: T.EX_PLUS, R.OP_MINUS: T.EX_MINUS, R.OP_MULTIPLY: T.EX_MULTIPLY, R.OP_DIVIDE: T.EX_DIVIDE}
PREFIXES = (1, 3, 5, 257)   # the four-rows-per-lane loop of decimal_kernel clamps the rows past n to n - 1


def cases_of(t):
    return [c for c in E.cases() if c["label"][1] == t]


def dev_col(D, side, n, validity=None):
    kind, typ, size, values = side
    if kind == "dec":
        return D.Column.decimal(values[:n], size[0], size[1], None if validity is None else validity[:n], bits=typ)
    code, npd = K.INTS[kind]
    return D.Column.from_numpy(np.array(values[:n], dtype=npd), code, None if validity is None else validity[:n])


def scalar_col(D, side, value):
    kind, typ, size, _ = side
    if kind == "dec":
        return D.Column.scalar(value, K.DEC_TYPE[typ], size[0], size[1])
    return D.Column.scalar(value, K.INTS[kind][0])


def expect(case, xv, yv):
    (xk, _, xs, _), (yk, _, ys, _) = case["x"], case["y"]
    out = []
    for x, y in zip(xv, yv):
        try:
            out.append(R.binary(case["op"], x, xk, xs, y, yk, ys)[0])
        except R.RowError:
            out.append(None)
    return out


def check_rows(case, what, vals, err_rows, err_count, expected, live=None):
    """values on the rows that compute, the raising rows (live ones only), their count and the 1 they hold"""
    n = len(expected)
    live = [True] * n if live is None else live
    bad = [i for i in range(n) if expected[i] is None and live[i]]
    assert list(err_rows) == bad, (what, E.OPNAME[case["op"]], case["x"][:3], case["y"][:3], sorted(set(err_rows) ^ set(bad))[:5])
    assert err_count == len(bad), (what, err_count, len(bad))
    wrong = [i for i in range(n) if live[i] and vals[i] != (1 if expected[i] is None else expected[i])]
    assert not wrong, (what, E.OPNAME[case["op"]], case["x"][:3], case["y"][:3], case["ret"], len(wrong),
                       [(i, case["x"][3][i], case["y"][3][i], vals[i], expected[i], sorted(case["labels"][i])) for i in wrong[:4]])


def column_run(D, case, a, b, n):
    err = D.RowErrors(n)
    out = D.decimal_arith(case["op"], a, b, n, errors=err)
    ret = tuple(case["ret"])
    assert D.decimal_result_size(case["op"], a, b) == ret
    assert (out.precision, out.scale) == ret and out.dtype == K.DEC_TYPE[R.storage_bits(ret[0])]
    return [int(v) for v in out.to_numpy()], err.error_rows().tolist(), err.num_errors(), out


def fused_run(D, case, cols, n, build=None):
    p = D.ExprProgram(cols)
    reg = build(p) if build else p.arith(EX[case["op"]], p.load(0), p.load(1))
    err = D.RowErrors(n)
    res = p.run(reg, n, errors=err)
    return res, [int(v) for v in res["values"]], err.error_rows().tolist(), err.num_errors()


@pytest.mark.parametrize("t", [64, 128])
def test_column_kernel_on_every_case_and_prefix(gpu, t):
    """gpu.decimal_arith, column x column: the whole case, and its prefixes of 1, 3, 5 and 257 rows"""
    seen = 0
    for case in cases_of(t):
        full = len(case["expected"])
        assert full >= max(PREFIXES)
        for n in (full,) + PREFIXES:
            vals, rows, cnt, _ = column_run(gpu, case, dev_col(gpu, case["x"], n), dev_col(gpu, case["y"], n), n)
            check_rows(case, f"column n={n}", vals, rows, cnt, case["expected"][:n])
            seen += len(vals)
    assert seen > 10_000   # (about twenty cases of at least 260 rows, and their prefixes)


def edge_picks(case, side, k=4):
    """a handful of operand values of one side taken from the rows that carry a divisor class, a tie or a range edge"""
    vals, out = case[side][3], []
    for v, labels in zip(vals, case["labels"]):
        if v not in out and any(lab.startswith(("D:2^", "D:10^", "tie:exact", "range:", "raise:div0", "wrap:")) for lab in labels):
            out.append(v)
    step = max(1, len(out) // k)
    out = out[::step][:k]
    for v in vals[::max(1, len(vals) // k)]:              # cases without such rows (plain pass-through sizes): ordinary values
        if len(out) < k and v not in out:
            out.append(v)
    return out


@pytest.mark.parametrize("t", [64, 128])
def test_scalar_operands_on_either_side(gpu, t):
    """one operand a constant (a scalar column has one value and one validity bit): edge divisors against every left operand of the
    case, edge left operands against every right operand"""
    for case in cases_of(t):
        n = len(case["expected"])
        xv, yv = case["x"][3], case["y"][3]
        assert len(edge_picks(case, "x")) >= 3 and len(edge_picks(case, "y")) >= 3
        for y in edge_picks(case, "y"):
            vals, rows, cnt, _ = column_run(gpu, case, dev_col(gpu, case["x"], n), scalar_col(gpu, case["y"], y), n)
            check_rows(case, f"scalar y={y}", vals, rows, cnt, expect(case, xv, [y] * n))
        for x in edge_picks(case, "x"):
            vals, rows, cnt, _ = column_run(gpu, case, scalar_col(gpu, case["x"], x), dev_col(gpu, case["y"], n), n)
            check_rows(case, f"scalar x={x}", vals, rows, cnt, expect(case, [x] * n, yv))


def null_masks(case, ci):
    """about a quarter of the rows NULL, every other raising row among them; which side is nullable rotates with the case"""
    n = len(case["expected"])
    valid = np.arange(n) % 4 != (ci % 4)
    raising = [i for i, e in enumerate(case["expected"]) if e is None]
    valid[np.array(raising[::2], dtype=np.int64)] = False
    xvalid = valid if ci % 3 != 1 else None
    yvalid = (np.arange(n) % 5 != 2) & (valid if ci % 3 == 1 else True) if ci % 3 != 0 else None
    live = np.ones(n, bool)
    for m in (xvalid, yvalid):
        if m is not None:
            live &= m
    return xvalid, yvalid, live


@pytest.mark.parametrize("t", [64, 128])
def test_null_rows_never_raise_and_are_not_counted(gpu, t):
    for ci, case in enumerate(cases_of(t)):
        n = len(case["expected"])
        xvalid, yvalid, live = null_masks(case, ci)
        vals, rows, cnt, out = column_run(gpu, case, dev_col(gpu, case["x"], n, xvalid), dev_col(gpu, case["y"], n, yvalid), n)
        check_rows(case, "nullable", vals, rows, cnt, case["expected"], live.tolist())
        assert np.array_equal(out.validity_numpy()[:n], live)
        # the same through the fused interpreter
        res, fvals, frows, fcnt = fused_run(gpu, case, [dev_col(gpu, case["x"], n, xvalid), dev_col(gpu, case["y"], n, yvalid)], n)
        check_rows(case, "fused nullable", fvals, frows, fcnt, case["expected"], live.tolist())
        assert np.array_equal(res["validity"], live)


@pytest.mark.parametrize("t", [64, 128])
def test_fused_interpreter_on_every_case(gpu, t):
    """one decimal node inside dbhip_expr_eval: dec_row_nodiv (or the inline form of a trivial node) where nothing divides, the full
    dec_row for the rounding multiply and the divide"""
    seen = 0
    for case in cases_of(t):
        for n in (len(case["expected"]), 5):
            res, vals, rows, cnt = fused_run(gpu, case, [dev_col(gpu, case["x"], n), dev_col(gpu, case["y"], n)], n)
            ret = tuple(case["ret"])
            assert res["type"] == K.DEC_TYPE[R.storage_bits(ret[0])] and res["size"] == ret
            check_rows(case, f"fused n={n}", vals, rows, cnt, case["expected"][:n])
            seen += len(vals)
    assert seen > 5_000


TWO_NODE = {   # T -> (sizes of a and b: a checked rounding multiply; the divisor's size: a shift-0 divide at the maximum precision)
    64: (((12, 8), (10, 8)), (3, 0), [1, -1, 3, -3, 7, 999, -999, 2, 0]),
    128: (((38, 10), (18, 10)), (6, 0), [1, -1, 3, -7, 999999, -999999, 2 ** 16 + 1, 10 ** 5, 0]),
}


@pytest.mark.parametrize("t", [64, 128])
def test_fused_rounding_multiply_feeding_a_divide(gpu, t):
    """(a * b) / c as one program: the expected value is the reference statement applied twice; a row raises if either node does
    (a raised product holds the value 1, which the divide then sees, like the reference builders; zero divisors sit on rows whose
    product computes, so that no row is counted twice)"""
    (sa, sb), sc, divisors = TWO_NODE[t]
    case = next(c for c in E.cases() if c["op"] == R.OP_MULTIPLY and c["x"][2] == sa and c["y"][2] == sb)
    n = len(case["expected"])
    mid = R.result_size(R.OP_MULTIPLY, sa, sb)[2]
    ret = R.result_size(R.OP_DIVIDE, mid, sc)[2]
    assert R.storage_bits(mid[0]) == t and R.storage_bits(ret[0]) == t and None in case["expected"]
    cv, exp, held = [], [], []
    for i, e in enumerate(case["expected"]):
        c = divisors[i % len(divisors)]
        if e is None and c == 0:
            c = 1
        cv.append(c)
        try:   # the divide sees the 1 a raised product holds, as the reference's second pass over the column would
            q = R.binary(R.OP_DIVIDE, 1 if e is None else e, "dec", mid, c, "dec", sc)[0]
        except R.RowError:
            q = None
        exp.append(None if e is None else q)
        held.append(1 if q is None else q)
    assert sum(e is None for e in exp) > sum(e is None for e in case["expected"])   # both nodes raise somewhere
    cols = [dev_col(gpu, case["x"], n), dev_col(gpu, case["y"], n), gpu.Column.decimal(cv, sc[0], sc[1])]

    def build(p):
        prod = p.arith(T.EX_MULTIPLY, p.load(0), p.load(1))
        return p.arith(T.EX_DIVIDE, prod, p.load(2))
    res, vals, rows, cnt = fused_run(gpu, case, cols, n, build)
    assert res["type"] == K.DEC_TYPE[t] and res["size"] == ret
    bad = [i for i, e in enumerate(exp) if e is None]
    assert rows == bad and cnt == len(bad)
    wrong = [(i, case["x"][3][i], case["y"][3][i], cv[i], vals[i], held[i]) for i in range(n) if vals[i] != held[i]]
    assert not wrong, (len(wrong), wrong[:4])
