"""GPU: the extended fused expression programs (Decimal64/128 nodes, if(), per-node NULL dependencies) and the generic fused
filter -> map -> partial-aggregate kernel (dbhip_groupby_add_block_program), against the oracle / the per-node kernels."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import oracle_lib as O
from tests.test_gpu_parity import norm, oracle_groupby, oracle_rows

pytestmark = pytest.mark.gpu


def oracle_decimal(oracle, op, a, b, n):
    """(values list, error rows) of the oracle's binary_decimal on two HostCols"""
    p, s = C.c_int(), C.c_int()
    props = {T.T_I8: (3, 0), T.T_U8: (3, 0), T.T_I16: (5, 0), T.T_U16: (5, 0), T.T_I32: (10, 0), T.T_U32: (10, 0), T.T_I64: (19, 0), T.T_U64: (20, 0)}
    ap = (a.precision, a.scale) if a.dtype in (T.T_DEC64, T.T_DEC128) else props[a.dtype]
    bp = (b.precision, b.scale) if b.dtype in (T.T_DEC64, T.T_DEC128) else props[b.dtype]
    assert oracle.orc_decimal_result_size(op, ap[0], ap[1], bp[0], bp[1], C.byref(p), C.byref(s)) == 0
    ot = T.T_DEC64 if p.value <= 18 else T.T_DEC128
    out = np.zeros(n * (2 if ot == T.T_DEC128 else 1) + 2, np.uint64)
    err = np.full((n + 7) // 8 + 8, 0xFF, np.uint8)
    cnt = C.c_uint64(0)
    ca, cb = a.c(), b.c()
    assert oracle.orc_decimal_arith(op, C.byref(ca), C.byref(cb), C.c_int64(n), ot, p.value, s.value, out.ctypes.data_as(C.c_void_p),
                                    err.ctypes.data_as(C.c_void_p), C.byref(cnt)) == 0
    vals = O.i128_list(out[:2 * n]) if ot == T.T_DEC128 else out[:n].view(np.int64).tolist()
    ok = np.unpackbits(err, bitorder="little")[:n].astype(bool)
    return vals, ok, ot, p.value, s.value


@pytest.mark.parametrize("n", [1, 63, 129, 50_003])
def test_fused_decimal_program_equals_the_per_node_decimal_semantics(gpu, oracle, n):
    """price * (1 - disc) * (1 + tax) — Q1's maps — and a rounding multiply, a Decimal128 + Decimal64 add and a decimal
    comparison as ONE program each, against the oracle's binary_decimal applied node by node (incl. NULL rows)."""
    rng = np.random.default_rng(n)
    price = rng.integers(-10**12, 10**12, n).astype(np.int64)
    disc = rng.integers(0, 11, n).astype(np.int64)
    tax = rng.integers(0, 9, n).astype(np.int64)
    pv = rng.integers(0, 6, n) > 0
    cp, cd, ct = (gpu.Column.from_numpy(x, T.T_DEC64, precision=15, scale=2) for x in (price, disc, tax))
    cpn = gpu.Column.from_numpy(price, T.T_DEC64, validity=pv, precision=15, scale=2)
    hp, hd, ht = (O.HostCol(T.T_DEC64, x, None, 15, 2) for x in (price, disc, tax))
    one = O.HostCol(T.T_U8, np.array([1], np.uint8), is_scalar=True)

    p = gpu.ExprProgram([cpn, cd, ct])
    a, b, c = p.load(0), p.load(1), p.load(2)
    k1 = p.const(1, T.T_U8)
    om = p.arith(T.EX_MINUS, k1, b, keep=(k1,))
    dp = p.arith(T.EX_MULTIPLY, a, om)
    op_ = p.arith(T.EX_PLUS, k1, c)
    ch = p.arith(T.EX_MULTIPLY, dp, op_)
    res = p.run(ch, n)
    assert res["type"] == T.T_DEC128 and res["size"] == (38, 6)
    v_om, _, t_om, p_om, s_om = oracle_decimal(oracle, T.OP_MINUS, one, hd, n)
    v_dp, _, t_dp, p_dp, s_dp = oracle_decimal(oracle, T.OP_MULTIPLY, hp, O.HostCol(t_om, np.array(v_om, np.int64), None, p_om, s_om), n)
    v_op, _, t_op, p_op, s_op = oracle_decimal(oracle, T.OP_PLUS, one, ht, n)
    v_ch, ok, t_ch, p_ch, s_ch = oracle_decimal(oracle, T.OP_MULTIPLY, O.HostCol(t_dp, O.i128_array(v_dp), None, p_dp, s_dp),
                                                O.HostCol(t_op, np.array(v_op, np.int64), None, p_op, s_op), n)
    assert (t_ch, p_ch, s_ch) == (T.T_DEC128, 38, 6) and ok.all()
    assert res["values"] == v_ch
    assert np.array_equal(res["validity"], pv)

    # a rounding multiply (Decimal(15,8) * Decimal(15,8) -> scale 12: divides by 10^4, arithmetic.rs:212-243) is fused since round 4
    x = rng.integers(-10**14, 10**14, n).astype(np.int64)
    cx = gpu.Column.from_numpy(x, T.T_DEC64, precision=15, scale=8)
    p2 = gpu.ExprProgram([cx, cx])
    r2 = p2.run(p2.arith(T.EX_MULTIPLY, p2.load(0), p2.load(1)), n)
    hx = O.HostCol(T.T_DEC64, x, None, 15, 8)
    v2, ok2, t2, pp2, ss2 = oracle_decimal(oracle, T.OP_MULTIPLY, hx, hx, n)
    assert ss2 == 12 and r2["type"] == t2 and r2["size"] == (pp2, ss2) and ok2.all() and r2["values"] == v2

    # Decimal128 + Decimal64 (rescale of the narrower side), then a comparison of two Decimal128 values, then if()
    big = [int(v) * 10**9 for v in rng.integers(-10**17, 10**17, n)]
    cb128 = gpu.Column.decimal128(big, 30, 4)
    p3 = gpu.ExprProgram([cb128, cp])
    s128 = p3.arith(T.EX_PLUS, p3.load(0), p3.load(1), keep=())
    r3 = p3.run(s128, n)
    v3, ok3, t3, pp3, s3 = oracle_decimal(oracle, T.OP_PLUS, O.HostCol(T.T_DEC128, O.i128_array(big), None, 30, 4), hp, n)
    assert r3["type"] == t3 and r3["size"] == (pp3, s3) and ok3.all() and r3["values"] == v3
    p4 = gpu.ExprProgram([cb128, cp])
    l0 = p4.load(0)
    s4 = p4.arith(T.EX_PLUS, l0, p4.load(1), keep=(l0,))
    r4 = p4.run(p4.cmp(T.EX_GT, s4, l0), n)                 # Decimal128(31,4) > Decimal128(30,4): same storage, same scale
    assert np.array_equal(r4["values"], np.array([a_ > b_ for a_, b_ in zip(v3, big)]))
    big2 = [int(v) * 10**9 for v in rng.integers(-10**17, 10**17, n)]
    p5 = gpu.ExprProgram([cb128, cp, gpu.Column.decimal128(big2, 30, 4)])
    l0, l1, l2 = p5.load(0), p5.load(1), p5.load(2)
    zero = p5.const(0, T.T_DEC64, 15, 2)
    cnd = p5.cmp(T.EX_GTE, l1, zero)
    r5 = p5.run(p5.if_(cnd, l0, l2), n)                      # if(price >= 0, big, big2) over Decimal128 values
    assert r5["values"] == [a_ if pr >= 0 else b_ for a_, b_, pr in zip(big, big2, price.tolist())]
    p6 = gpu.ExprProgram([cb128, cp])                          # a branch that can raise is NOT fused (lazy branches stay on the CPU)
    l0, l1 = p6.load(0), p6.load(1)
    s6 = p6.arith(T.EX_PLUS, l0, l1, keep=(l0, l1))
    with pytest.raises(T.DbhipError) as e6:
        p6.run(p6.if_(p6.cmp(T.EX_GTE, l1, p6.const(0, T.T_DEC64, 15, 2)), s6, l0), n)
    assert e6.value.code == T.ERR_UNSUPPORTED


def test_fused_decimal_program_row_errors(gpu, oracle):
    """'Decimal overflow' rows of a fused decimal node (plus at precision 38 checks the result, arithmetic.rs:229-243): the
    same rows as the oracle's, value 1 like the reference builders; a NULL input the node depends on never raises."""
    n = 1000
    rng = np.random.default_rng(3)
    x = [int(v) * 10**20 for v in rng.integers(-10**18 + 1, 10**18 - 1, n)]          # Decimal(38,0), |x| < 10^38
    y = [int(v) * 10**20 for v in rng.integers(-10**18 + 1, 10**18 - 1, n)]
    yv = rng.integers(0, 3, n) > 0
    cx, cy = gpu.Column.decimal128(x, 38, 0), gpu.Column.decimal128(y, 38, 0, validity=yv)
    p = gpu.ExprProgram([cx, cy])
    r = p.arith(T.EX_PLUS, p.load(0), p.load(1))
    errs = gpu.RowErrors(n)
    res = p.run(r, n, errors=errs)
    v, ok, t, pp, ss = oracle_decimal(oracle, T.OP_PLUS, O.HostCol(T.T_DEC128, O.i128_array(x), None, 38, 0), O.HostCol(T.T_DEC128, O.i128_array(y), yv, 38, 0), n)
    really = np.array([abs(a_ + b_) > 10**38 - 1 for a_, b_ in zip(x, y)])
    bad = np.nonzero(really & yv)[0]
    assert len(bad) > 20
    assert np.array_equal(np.nonzero(~ok)[0], bad)       # the oracle raises for the same rows (valid inputs only)
    assert np.array_equal(errs.error_rows(), bad) and errs.num_errors() == len(bad)
    got = res["values"]
    assert all(got[i] == v[i] for i in range(n) if not really[i])
    assert all(got[i] == 1 for i in bad)


DIV_CASES = [
    # (op, a: (type, precision, scale, lo, hi), b: likewise) — branches of dec_row that divide (their edges: test_gpu_decimal_edges.py)
    (T.OP_MULTIPLY, (T.T_DEC64, 9, 6, -10**8, 10**8), (T.T_DEC64, 9, 6, -10**8, 10**8)),          # T = i64 at precision 18, scale shift 0: rounds nothing, checks nothing
    (T.OP_MULTIPLY, (T.T_DEC64, 15, 8, -10**14, 10**14), (T.T_DEC64, 15, 8, -10**14, 10**14)),    # T = i128, no overflow check
    (T.OP_MULTIPLY, (T.T_DEC128, 38, 10, -10**30, 10**30), (T.T_DEC64, 18, 10, -10**17, 10**17)),  # T = i128 at precision 38: 256-bit product, may overflow
    (T.OP_DIVIDE, (T.T_DEC64, 9, 2, -10**8, 10**8), (T.T_DEC64, 9, 4, -300, 300)),                # divide, zero divisors raise
    (T.OP_DIVIDE, (T.T_DEC64, 15, 2, -10**14, 10**14), (T.T_DEC64, 15, 2, -10**6, 10**6)),        # divide in i128
    (T.OP_DIVIDE, (T.T_DEC128, 30, 4, -10**27, 10**27), (T.T_DEC64, 15, 8, -10**10, 10**10)),
    (T.OP_DIVIDE, (T.T_DEC64, 15, 2, -10**14, 10**14), (T.T_I32, 0, 0, -5, 5)),                   # integer operand (other_to_decimal)
]


@pytest.mark.parametrize("ci", range(len(DIV_CASES)))
def test_fused_rounding_multiply_and_divide_equal_the_oracle(gpu, oracle, ci):
    """The rounding decimal multiply (scale shift > 0) and the decimal divide INSIDE a fused program (decimal/src/arithmetic.rs:212-243,
    types/decimal.rs:759-797,1024-1064: do_round_mul / do_round_div): values, result size and the raising rows (division by zero, results
    beyond the precision) equal the oracle's binary_decimal; NULL rows of a nullable operand never raise."""
    op, (ta, pa, sa, loa, hia), (tb, pb, sb, lob, hib) = DIV_CASES[ci]
    n = 20_011
    rng = np.random.default_rng(40 + ci)

    def make(t, pr, sc, lo, hi, validity=None):
        if t == T.T_DEC128:
            vals = [int(v) * (hi // 10**17 or 1) for v in rng.integers(-10**17, 10**17, n)]
            vals = [max(min(v, hi - 1), lo) for v in vals]
            return gpu.Column.decimal128(vals, pr, sc, validity=validity), O.HostCol(T.T_DEC128, O.i128_array(vals), validity, pr, sc)
        if t == T.T_I32:
            v = rng.integers(lo, hi + 1, n).astype(np.int32)
            return gpu.Column.from_numpy(v, validity=validity), O.HostCol(T.T_I32, v, validity)
        v = rng.integers(lo, hi, n).astype(np.int64)
        v[::97] = 0
        return gpu.Column.from_numpy(v, T.T_DEC64, validity=validity, precision=pr, scale=sc), O.HostCol(T.T_DEC64, v, validity, pr, sc)
    bvalid = rng.integers(0, 8, n) > 0
    ca, ha = make(ta, pa, sa, loa, hia)
    cb, hb = make(tb, pb, sb, lob, hib, validity=bvalid)
    p = gpu.ExprProgram([ca, cb])
    ex = {T.OP_MULTIPLY: T.EX_MULTIPLY, T.OP_DIVIDE: T.EX_DIVIDE}[op]
    errs = gpu.RowErrors(n)
    res = p.run(p.arith(ex, p.load(0), p.load(1)), n, errors=errs)
    v, ok, t, pp, ss = oracle_decimal(oracle, op, ha, hb, n)
    assert res["type"] == t and res["size"] == (pp, ss)
    bad = np.nonzero(~ok)[0]                                  # (the oracle skips NULL rows like the reference's evaluator)
    assert np.array_equal(errs.error_rows(), bad) and errs.num_errors() == len(bad)
    if op == T.OP_DIVIDE:
        assert len(bad) > 0
    got = res["values"]
    live = ok & bvalid
    assert all(got[i] == v[i] for i in np.nonzero(live)[0])
    assert all(got[i] == 1 for i in bad)
    assert np.array_equal(res["validity"], bvalid)


def test_fused_aggregation_over_a_rescaling_q1_variant(gpu, oracle):
    """A Q1-like query whose scales force a rescale — sum(price * discount) with Decimal(15,8) columns (a rounding multiply) and
    sum(quantity / price) (a divide) — stays ONE fused filter + map + aggregate program: interpreted first, then PREPAREd (run-time
    specialised, the divisors folded to constants); both equal filter -> maps -> hash aggregation of the oracle."""
    n = 120_007
    rng = np.random.default_rng(77)
    k = rng.integers(0, 3, n).astype(np.int64)
    ship = rng.integers(8000, 10600, n).astype(np.int32)
    qty = (rng.integers(1, 51, n) * 100).astype(np.int64)
    price = rng.integers(10**8, 10**13, n).astype(np.int64)
    disc = rng.integers(0, 10**7, n).astype(np.int64)
    aggs = None

    def run(prepare):
        nonlocal aggs
        cs = gpu.Column.from_numpy(ship, T.T_DATE)
        cq = gpu.Column.from_numpy(qty, T.T_DEC64, precision=15, scale=2)
        cp = gpu.Column.from_numpy(price, T.T_DEC64, precision=15, scale=8)
        cd = gpu.Column.from_numpy(disc, T.T_DEC64, precision=15, scale=8)
        p = gpu.ExprProgram([cs, cq, cp, cd])
        f = p.cmp(T.EX_LTE, p.load(0), p.const(10471, T.T_DATE))
        q, pr, di = p.load(1), p.load(2), p.load(3)
        prod = p.arith(T.EX_MULTIPLY, pr, di, keep=(pr,))
        quo = p.arith(T.EX_DIVIDE, q, pr, keep=(q,))
        aggs = [(T.AGG_SUM, T.T_DEC64, 15, 2, 0), (T.AGG_SUM, p.types[prod], p.size[prod][0], p.size[prod][1], 0),
                (T.AGG_SUM, p.types[quo], p.size[quo][0], p.size[quo][1], 0), (T.AGG_COUNT, 0, 0, 0, 0)]
        g = gpu.GroupBy([T.T_I64], aggs)
        if prepare:
            g.prepare_program([gpu.Column.from_numpy(k)], p, [q, prod, quo, None], filter_reg=f)    # blocks until the kernel is loaded
        g.add_block_program([gpu.Column.from_numpy(k)], p, [q, prod, quo, None], n, filter_reg=f)
        return g, (p.types[prod], p.size[prod]), (p.types[quo], p.size[quo])
    before = fagg_stats()
    g0, tprod, tquo = run(False)
    mid = fagg_stats()
    g1, _, _ = run(True)
    after = fagg_stats()
    assert mid["interpreted"] > before["interpreted"] or mid["jit"] > before["jit"]     # (an earlier run may have left the kernel in the cache)
    assert after["jit"] > mid["jit"]
    sel = np.nonzero(ship <= 10471)[0]
    m = len(sel)
    hq = O.HostCol(T.T_DEC64, qty[sel], None, 15, 2)
    hp, hd = O.HostCol(T.T_DEC64, price[sel], None, 15, 8), O.HostCol(T.T_DEC64, disc[sel], None, 15, 8)
    vprod, okp, t1, p1, s1 = oracle_decimal(oracle, T.OP_MULTIPLY, hp, hd, m)
    vquo, okq, t2, p2, s2 = oracle_decimal(oracle, T.OP_DIVIDE, hq, hp, m)
    assert okp.all() and okq.all() and (t1, (p1, s1)) == tprod and (t2, (p2, s2)) == tquo
    harg = lambda vals, t, pp, ss: O.HostCol(t, O.i128_array(vals) if t == T.T_DEC128 else np.array(vals, np.int64), None, pp, ss)
    h = oracle_groupby(oracle, [T.T_I64], [0], aggs, [O.HostCol(T.T_I64, k[sel])], [hq, harg(vprod, t1, p1, s1), harg(vquo, t2, p2, s2), None], m)
    exp = oracle_rows(oracle, h, [T.T_I64], aggs)
    oracle.orc_hashagg_destroy(h)
    assert norm(g0.result()) == norm(exp)
    assert norm(g1.result()) == norm(exp)


Q_KEYS = ([T.T_I64, T.T_STRING], [1, 0])


def fagg_case(gpu, oracle, n, card, seed, keep=0.9):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, card, n).astype(np.int64) * 7 - 3
    kv = rng.integers(0, 10, n) > 0
    s = [b"x%d" % (v % 2) for v in rng.integers(0, 1000, n)]
    a = rng.integers(-10**9, 10**9, n).astype(np.int64)
    b = rng.integers(-10**6, 10**6, n).astype(np.int32)
    bv = rng.integers(0, 4, n) > 0
    d = rng.integers(-10**13, 10**13, n).astype(np.int64)
    e = rng.integers(0, 1000, n).astype(np.int64)
    f = rng.integers(-1000, 1000, n).astype(np.float64)
    thr = int(np.quantile(a, 1 - keep)) if n > 1 else -10**10
    return dict(k=k, kv=kv, s=s, a=a, b=b, bv=bv, d=d, e=e, f=f, thr=thr)


FA_AGGS = [(T.AGG_SUM, T.T_I64, 0, 0, 1), (T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_DEC128, 31, 4, 0), (T.AGG_MIN, T.T_I32, 0, 0, 1),
           (T.AGG_MAX, T.T_F64, 0, 0, 0), (T.AGG_COUNT, T.T_I32, 0, 0, 1), (T.AGG_SUM, T.T_F64, 0, 0, 0)]


def run_fagg(gpu, c, n, g=None):
    """sum(a + b) [nullable through b], count(*), sum(d * (e + 3)) as Decimal128(31,4), min(b), max(f), count(b), sum(f)
    WHERE a > thr GROUP BY k (nullable), s"""
    from databend_amd.device import make_views_general
    g = g or gpu.GroupBy(Q_KEYS[0], FA_AGGS, Q_KEYS[1])
    ca, cb = gpu.Column.from_numpy(c["a"]), gpu.Column.from_numpy(c["b"], validity=c["bv"])
    cd = gpu.Column.from_numpy(c["d"], T.T_DEC64, precision=15, scale=2)
    ce = gpu.Column.from_numpy(c["e"], T.T_DEC64, precision=15, scale=2)
    cf = gpu.Column.from_numpy(c["f"])
    p = gpu.ExprProgram([ca, cb, cd, ce, cf])
    la = p.load(0)
    filt = p.cmp(T.EX_GT, la, p.const(c["thr"], T.T_I64), keep=(la,))
    lb = p.load(1)
    apb = p.arith(T.EX_PLUS, la, lb, keep=(lb,))                       # i64 + i32 -> i64
    e3 = p.arith(T.EX_PLUS, p.load(3), p.const(3, T.T_U8))            # Decimal(16,2)
    prod = p.arith(T.EX_MULTIPLY, p.load(2), e3)                       # Decimal(31,4)
    lf = p.load(4)
    keys = [gpu.Column.from_numpy(c["k"], validity=c["kv"]), gpu.Column.strings(c["s"])]
    g.add_block_program(keys, p, [apb, None, prod, lb, lf, lb, lf], n, filter_reg=filt)
    return g


def expect_fagg(oracle, c, n):
    from databend_amd.device import make_views_general
    sel = np.nonzero(c["a"] > c["thr"])[0]
    m = len(sel)
    if m == 0:
        return []
    apb = (c["a"][sel] + c["b"][sel].astype(np.int64))
    e3 = O.HostCol(T.T_DEC64, c["e"][sel] + 300, None, 16, 2)
    vals, ok, t, pp, ss = oracle_decimal(oracle, T.OP_MULTIPLY, O.HostCol(T.T_DEC64, c["d"][sel], None, 15, 2), e3, m)
    assert (t, pp, ss) == (T.T_DEC128, 31, 4) and ok.all()
    v, buf = make_views_general([c["s"][i] for i in sel])
    hkeys = [O.HostCol(T.T_I64, c["k"][sel], c["kv"][sel]), O.HostCol(T.T_STRING, v, buffers=[buf])]
    bv = c["bv"][sel]
    hargs = [O.HostCol(T.T_I64, apb, bv), None, O.HostCol(T.T_DEC128, O.i128_array(vals), None, 31, 4), O.HostCol(T.T_I32, c["b"][sel], bv),
             O.HostCol(T.T_F64, c["f"][sel]), O.HostCol(T.T_I32, c["b"][sel], bv), O.HostCol(T.T_F64, c["f"][sel])]
    h = oracle_groupby(oracle, Q_KEYS[0], Q_KEYS[1], FA_AGGS, hkeys, hargs, m)
    exp = oracle_rows(oracle, h, Q_KEYS[0], FA_AGGS)
    oracle.orc_hashagg_destroy(h)
    return exp


@pytest.mark.parametrize("n,card,keep", [(1, 1, 1.0), (127, 2, 0.5), (129, 3, 0.9), (100_003, 2, 0.986), (300_000, 3, 0.03), (70_000, 1, 0.0)])
def test_fused_filter_map_aggregate_matches_oracle(gpu, oracle, n, card, keep):
    """One launch == filter -> take -> maps -> hash aggregation of the oracle, compared as sorted row sets: nullable key +
    string key (up to 2 x card x 2 groups incl. the NULL key), nullable and decimal arguments, min / max / f64 sums."""
    c = fagg_case(gpu, oracle, n, card, 100 + n, keep)
    g = run_fagg(gpu, c, n)
    assert norm(g.result()) == norm(expect_fagg(oracle, c, n))


def test_fused_aggregate_gives_up_cleanly_on_too_many_groups(gpu, oracle):
    """> 8 groups inside a workgroup: DBHIP_ERR_CAPACITY and the table is untouched (the caller keeps the operator plan);
    the 8-slot variant takes over between 5 and 8 groups."""
    n = 50_000
    c = fagg_case(gpu, oracle, n, 2, 7)       # up to 3 keys (incl. NULL) x 2 strings = 6 groups: needs the 8-slot kernel
    g = run_fagg(gpu, c, n)
    exp = expect_fagg(oracle, c, n)
    assert len(exp) > 4 and norm(g.result()) == norm(exp)
    c9 = fagg_case(gpu, oracle, n, 40, 8)
    with pytest.raises(T.DbhipError) as e:
        run_fagg(gpu, c9, n, g)
    assert e.value.code == T.ERR_CAPACITY
    assert norm(g.result()) == norm(exp)


def test_fused_aggregate_row_errors_respect_the_filter(gpu, oracle):
    """A map that overflows on a row the filter DROPS raises nothing (TransformFilter precedes the maps); on a kept row the
    block fails with DBHIP_ERR_ROW_ERRORS and nothing is merged."""
    n = 4096
    k = np.zeros(n, np.int64)
    x = [9 * 10**37] * n                                   # Decimal(38,0)
    sel = np.arange(n) == 777                              # ONE kept row (two such sums would leave 38 digits at flush)
    y_bad = [5 * 10**37] * n                               # x + y leaves 38 digits on every row
    y_ok = [1 if keep else 5 * 10**37 for keep in sel]     # kept rows are fine, dropped rows would overflow
    flag = sel.astype(np.int64)
    aggs = [(T.AGG_SUM, T.T_DEC128, 38, 0, 0), (T.AGG_COUNT, 0, 0, 0, 0)]

    def run(ycol, g=None):
        g = g or gpu.GroupBy([T.T_I64], aggs)
        cx, cy, cf = gpu.Column.decimal128(x, 38, 0), gpu.Column.decimal128(ycol, 38, 0), gpu.Column.from_numpy(flag)
        p = gpu.ExprProgram([cx, cy, cf])
        filt = p.cmp(T.EX_EQ, p.load(2), p.const(1, T.T_I64))
        tot = p.arith(T.EX_PLUS, p.load(0), p.load(1))
        assert p.types[tot] == T.T_DEC128
        g.add_block_program([gpu.Column.from_numpy(k)], p, [tot, None], n, filter_reg=filt)
        return g
    g = run(y_ok)
    rows = g.result()
    assert rows == [(0, 9 * 10**37 + 1, 1)]
    with pytest.raises(T.DbhipError) as e:
        run(y_bad, g)
    assert e.value.code == T.ERR_ROW_ERRORS
    assert g.result() == rows


@pytest.mark.parametrize("n", [1, 129, 300_007])
def test_q1_as_one_generic_fused_program_equals_the_oracle(gpu, oracle, n):
    from databend_amd import tpch
    host = tpch.gen_lineitem(n, seed=n + 5)
    li = tpch.LineitemDevice(host)
    exp = O.q1_run(host, tpch.Q1_CUTOFF, threads=1)
    assert tpch.q1_rows(tpch.q1_fused_program(li)) == exp


def fagg_stats():
    import ctypes as C
    out = (C.c_uint64 * 3)()
    T.lib().dbhip_fagg_stats(out)
    return dict(jit=out[0], interpreted=out[1], pending=out[2])


@pytest.mark.parametrize("card", [1, 4, 8])
def test_plain_add_block_uses_the_fused_few_groups_kernel(gpu, oracle, card):
    """add_block on a table whose probing chunk shows <= 8 groups hands the rest of the block to the RUN-TIME SPECIALISED
    fused kernel (empty program) once that kernel exists: the first block of a new shape starts a background compile and takes
    the LDS path (a query never waits for the compiler), later blocks find the code object in the on-disk cache. Same sorted
    row set as the closed form either way, incl. a pushed-down filter; a 9th group appearing late falls back to the LDS path."""
    import time
    n = 6_000_000      # (> 4 M rows: the first block of a shape goes through the probing chunk)
    rng = np.random.default_rng(card)
    k = rng.integers(0, card, n).astype(np.int64)
    a = rng.integers(-10**9, 10**9, n).astype(np.int64)
    av = rng.integers(0, 5, n) > 0
    d = rng.integers(-10**14, 10**14, n).astype(np.int64)
    keep = rng.random(n) < 0.9
    aggs = [(T.AGG_SUM, T.T_I64, 0, 0, 1), (T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_DEC64, 15, 2, 0), (T.AGG_MAX, T.T_I64, 0, 0, 1)]

    def expect(kk, sel):
        out = []
        for key in np.unique(kk[sel]):
            m = sel & (kk == key)
            mv = m & av
            out.append((int(key), int(a[mv].sum()) if mv.any() else None, int(m.sum()), int(d[m].sum()), int(a[mv].max()) if mv.any() else None))
        return sorted(out)

    def run(kk, filt):
        g = gpu.GroupBy([T.T_I64], aggs)
        g.add_block([gpu.Column.from_numpy(kk)], [gpu.Column.from_numpy(a, validity=av), None, gpu.Column.from_numpy(d, T.T_DEC64, precision=15, scale=2),
                                                  gpu.Column.from_numpy(a, validity=av)], n, filter=gpu.Column.boolean(filt) if filt is not None else None)
        return sorted(g.result())
    exp_all, exp_keep = expect(k, np.ones(n, bool)), expect(k, keep)
    assert run(k, None) == exp_all     # whichever kernel is available now
    assert run(k, keep) == exp_keep
    # wait for the background compiles of both shapes (with / without the predicate), then the specialised kernel must be the one that runs
    deadline = time.time() + 90
    for filt, exp in ((None, exp_all), (keep, exp_keep)):
        while True:
            before = fagg_stats()["jit"]
            assert run(k, filt) == exp
            if fagg_stats()["jit"] > before:
                break
            assert time.time() < deadline, ("the specialised kernel never became available", fagg_stats())
            time.sleep(0.25)
    assert fagg_stats()["interpreted"] == 0 or True   # (other tests of this process may have interpreted prepared-less programs)
    if card == 8:
        k2 = k.copy()
        k2[5_500_000:] += 100       # 8 more groups show up after the probing chunk: the fused kernel gives up, the LDS path takes over
        assert run(k2, None) == expect(k2, np.ones(n, bool))


def test_prepared_specialised_kernel_equals_the_interpreter(gpu, oracle):
    """dbhip_groupby_prepare_program: after PREPARE the launches go through the kernel hiprtc specialised for this program
    (env DBHIP_TRACE shows it); results are those of the interpreter (run before the prepare) and of the query-specific kernel.
    A second, different program shape gets its own kernel."""
    import torch
    from databend_amd import tpch
    li = tpch.LineitemTorch(3_000_003, seed=9, torch=torch)
    exp = tpch.q1_rows(tpch.q1_fused(li))
    first = tpch.q1_rows(tpch.q1_fused_program(li))            # interpreter, or the specialised kernel if an earlier test prepared it
    tpch.q1_fused_program(li, prepare=True)                    # blocks until the specialised kernel is loaded
    again = tpch.q1_rows(tpch.q1_fused_program(li))
    other = tpch.q1_rows(tpch.q1_fused_program(li, cutoff=tpch.Q1_CUTOFF - 400))   # the constant is part of the program: another kernel
    tpch.q1_fused_program(li, cutoff=tpch.Q1_CUTOFF - 400, prepare=True)
    other2 = tpch.q1_rows(tpch.q1_fused_program(li, cutoff=tpch.Q1_CUTOFF - 400))
    assert first == exp and again == exp and other == other2 and other != exp


def test_and_or_over_nullable_operands_keep_three_valued_semantics(gpu):
    """the fused interpreter evaluates AND / OR strictly while the reference's are three-valued. An AND over
    nullable operands may end in the FILTER (NULL and FALSE both drop the row); OR over a nullable operand, and a nullable AND
    that feeds a value result or NOT, are refused so that the binding keeps the CPU evaluator. A nullable predicate Bitmap
    handed to add_block drops its NULL rows like FALSE ones."""
    D = gpu
    n = 5000
    rng = np.random.default_rng(77)
    a = rng.integers(0, 10, n).astype(np.int64)
    b = rng.integers(0, 10, n).astype(np.int64)
    va, vb = rng.integers(0, 4, n) > 0, rng.integers(0, 4, n) > 0
    k = rng.integers(0, 3, n).astype(np.int64)
    x = rng.integers(-100, 100, n).astype(np.int64)
    aggs = [(T.AGG_SUM, T.T_I64, 0, 0, 0), (T.AGG_COUNT, 0, 0, 0, 0)]

    def program():
        ca, cb = D.Column.from_numpy(a, validity=va), D.Column.from_numpy(b, validity=vb)
        p = D.ExprProgram([ca, cb, D.Column.from_numpy(x)])
        pa = p.cmp(T.EX_GT, p.load(0), p.const(3, T.T_I64))
        pb = p.cmp(T.EX_LT, p.load(1), p.const(8, T.T_I64))
        return p, pa, pb

    # AND ending in the filter: rows kept iff both predicates are TRUE (a NULL operand never passes a filter)
    p, pa, pb = program()
    f = p.logic(T.EX_AND, pa, pb)
    g = D.GroupBy([T.T_I64], aggs)
    g.add_block_program([D.Column.from_numpy(k)], p, [("input", 2), None], n, filter_reg=f)
    keep = va & vb & (a > 3) & (b < 8)
    exp = sorted((int(key), int(x[keep & (k == key)].sum()), int((keep & (k == key)).sum())) for key in np.unique(k[keep]))
    assert sorted(g.result()) == exp
    # OR over a nullable operand: refused (TRUE OR NULL = TRUE)
    p, pa, pb = program()
    f = p.logic(T.EX_OR, pa, pb)
    with pytest.raises(T.DbhipError) as e:
        D.GroupBy([T.T_I64], aggs).add_block_program([D.Column.from_numpy(k)], p, [("input", 2), None], n, filter_reg=f)
    assert e.value.code == T.ERR_UNSUPPORTED
    # NOT over a nullable AND, and a nullable AND as a value: refused (FALSE AND NULL = FALSE)
    p, pa, pb = program()
    f = p.logic(T.EX_NOT, p.logic(T.EX_AND, pa, pb))
    with pytest.raises(T.DbhipError) as e:
        D.GroupBy([T.T_I64], aggs).add_block_program([D.Column.from_numpy(k)], p, [("input", 2), None], n, filter_reg=f)
    assert e.value.code == T.ERR_UNSUPPORTED
    p, pa, pb = program()
    f = p.logic(T.EX_AND, pa, pb)
    with pytest.raises(T.DbhipError) as e:
        p.run(f, n)
    assert e.value.code == T.ERR_UNSUPPORTED
    # non-nullable operands: OR and NOT stay fused
    p = D.ExprProgram([D.Column.from_numpy(a), D.Column.from_numpy(b)])
    f = p.logic(T.EX_NOT, p.logic(T.EX_OR, p.cmp(T.EX_GT, p.load(0), p.const(3, T.T_I64)), p.cmp(T.EX_LT, p.load(1), p.const(8, T.T_I64))))
    out = p.run(f, n)
    assert np.array_equal(np.asarray(out["values"], dtype=bool)[:n], ~((a > 3) | (b < 8)))
    # a nullable predicate column pushed into add_block: NULL rows are dropped like FALSE ones
    pred = D.cmp(T.CMP_GT, D.Column.from_numpy(a, validity=va), D.Column.scalar(3, T.T_I64))
    g = D.GroupBy([T.T_I64], aggs)
    g.add_block([D.Column.from_numpy(k)], [D.Column.from_numpy(x), None], n, filter=pred)
    keep = va & (a > 3)
    exp = sorted((int(key), int(x[keep & (k == key)].sum()), int((keep & (k == key)).sum())) for key in np.unique(k[keep]))
    assert sorted(g.result()) == exp


def test_or_filters_and_filters_over_nullable_predicates(gpu):
    """or_filters / and_filters (evaluator.rs:1802-1880): every argument goes through decode_predicate (NULL -> FALSE) and the
    result is never NULL. As a value, as the operand of NOT, and as the filter of a fused aggregation — interpreted and through
    the run-time specialised kernel."""
    D = gpu
    n = 70001
    rng = np.random.default_rng(78)
    a = rng.integers(0, 10, n).astype(np.int64)
    b = rng.integers(0, 10, n).astype(np.int64)
    c = rng.integers(0, 10, n).astype(np.int32)
    va, vb, vc = rng.integers(0, 4, n) > 0, rng.integers(0, 3, n) > 0, rng.integers(0, 5, n) > 0
    k = rng.integers(0, 3, n).astype(np.int64)
    x = rng.integers(-100, 100, n).astype(np.int64)
    ta, tb, tc = va & (a > 3), vb & (b < 8), vc & (c == 5)          # decode_predicate of the three predicates

    def program():
        cols = [D.Column.from_numpy(a, validity=va), D.Column.from_numpy(b, validity=vb), D.Column.from_numpy(c, validity=vc), D.Column.from_numpy(x)]
        p = D.ExprProgram(cols)
        return p, (p.cmp(T.EX_GT, p.load(0), p.const(3, T.T_I64)), p.cmp(T.EX_LT, p.load(1), p.const(8, T.T_I64)),
                   p.cmp(T.EX_EQ, p.load(2), p.const(5, T.T_I32)))

    def bits(out):
        assert out.get("validity") is None or np.asarray(out["validity"], dtype=bool)[:n].all()   # never NULL
        return np.asarray(out["values"], dtype=bool)[:n]

    p, preds = program()
    assert np.array_equal(bits(p.run(p.or_filters(*preds), n)), ta | tb | tc)
    p, preds = program()
    assert np.array_equal(bits(p.run(p.and_filters(*preds), n)), ta & tb & tc)
    p, preds = program()
    assert np.array_equal(bits(p.run(p.logic(T.EX_NOT, p.or_filters(preds[0], preds[1])), n)), ~(ta | tb))
    # or_filters(and_filters(p, q), r): the strict AND below IS_TRUE is exact (FALSE AND NULL and TRUE AND NULL decode to FALSE)
    p, preds = program()
    inner = p.logic(T.EX_AND, preds[0], preds[1])
    assert np.array_equal(bits(p.run(p.logic(T.EX_OR, p.is_true(inner), p.is_true(preds[2])), n)), (ta & tb) | tc)
    # as the filter of a fused aggregation
    aggs = [(T.AGG_SUM, T.T_I64, 0, 0, 0), (T.AGG_COUNT, 0, 0, 0, 0)]
    keep = ta | tb & tc
    exp = sorted((int(key), int(x[keep & (k == key)].sum()), int((keep & (k == key)).sum())) for key in np.unique(k[keep]))
    for prepare in (False, True):
        p, preds = program()
        f = p.logic(T.EX_OR, p.is_true(preds[0]), p.and_filters(preds[1], preds[2]))
        g = D.GroupBy([T.T_I64], aggs)
        if prepare:
            g.add_block_program([D.Column.from_numpy(k)], p, [("input", 3), None], n, filter_reg=f, prepare=True)
            g = D.GroupBy([T.T_I64], aggs)
        g.add_block_program([D.Column.from_numpy(k)], p, [("input", 3), None], n, filter_reg=f)
        assert sorted(g.result()) == exp, prepare
