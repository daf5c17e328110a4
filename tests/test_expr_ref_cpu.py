"""CPU: the reference of the fused expression interpreter (tests/expr_ref.py) against the oracle's per-node functions, its two integer
evaluators against each other, the NULL rule on hand-written programs, and the generator of tests/expr_cases.py against the documented
limits of dbhip_expr_eval and the coverage tests/test_gpu_expr.py claims."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import expr_cases as EC
from tests import expr_ref as R
from tests import oracle_lib as O
from tests.test_cast_cpu import NAME, interesting, oracle_cast

OPS = ((T.EX_PLUS, T.OP_PLUS), (T.EX_MINUS, T.OP_MINUS), (T.EX_MULTIPLY, T.OP_MULTIPLY), (T.EX_DIVIDE, T.OP_DIVIDE))


@pytest.fixture(scope="module")
def L():
    return O.load()


def pool_column(t, n, seed):
    return EC.fill(np.random.default_rng(seed), t, n)


def one_node(op, ta, tb, typ):
    return [(T.EX_LOAD, 0, 0, 0, ta, 0, (0, 0)), (T.EX_LOAD, 1, 1, 0, tb, 0, (0, 0)), (op, 2, 0, 1, typ, 0, (0, 0))]


def test_result_type_table_equals_the_oracle(L):
    for ta in R.NUMBERS:
        for tb in R.NUMBERS:
            for ex, op in OPS:
                assert R.arith_result_type(ex, ta, tb) == L.orc_arith_result_type(op, ta, tb), (ex, ta, tb)


@pytest.mark.parametrize("use_numpy", [False, True])
def test_one_node_arithmetic_equals_orc_arith_on_every_type_pair(L, use_numpy):
    n = 96
    for ta in R.NUMBERS:
        for tb in R.NUMBERS:
            a, b = pool_column(ta, n, ta), pool_column(tb, n, 100 + tb)
            va = np.random.default_rng(ta * 31 + tb).random(n) < 0.7
            ha, hb = O.HostCol(ta, a, va), O.HostCol(tb, b)          # (kept alive: c() hands out their addresses)
            ca, cb = ha.c(), hb.c()
            for ex, op in OPS:
                ot = R.arith_result_type(ex, ta, tb)
                exp = np.zeros(n, dtype=R.NP[ot])
                eb = np.zeros(((n + 31) // 32) * 4 + 8, np.uint8)
                ec = C.c_uint64(0)
                assert L.orc_arith(op, C.byref(ca), C.byref(cb), C.c_int64(n), ot, exp.ctypes.data_as(C.c_void_p), eb.ctypes.data_as(C.c_void_p), C.byref(ec)) == 0
                got = R.run(one_node(ex, ta, tb, ot), [R.Input(ta, a, va), R.Input(tb, b)], n, 2, L, use_numpy=use_numpy)
                assert got.type == ot and R.same(got.values, exp), (ex, ta, tb)
                assert np.array_equal(got.validity, va)
                bad = np.flatnonzero(~np.unpackbits(eb, bitorder="little")[:n].astype(bool))
                assert np.array_equal(got.raising, bad) and ec.value == len(bad) == got.raise_events, (ex, ta, tb)
                if ex == T.EX_DIVIDE and len(bad):
                    assert not np.asarray(got.values)[bad].any()


@pytest.mark.parametrize("use_numpy", [False, True])
def test_one_node_comparison_equals_orc_cmp(L, use_numpy):
    n = 128
    for t in R.NUMBERS:
        a, b = pool_column(t, n, t), pool_column(t, n, 50 + t)
        b[n // 2:] = a[:n - n // 2][::-1]             # pool values against each other, incl. equal ones
        ha, hb = O.HostCol(t, a), O.HostCol(t, b)
        ca, cb = ha.c(), hb.c()
        for k, ex in enumerate(R.CMPS):
            exp = np.zeros((n + 7) // 8 + 8, np.uint8)
            assert L.orc_cmp(k, C.byref(ca), C.byref(cb), C.c_int64(n), exp.ctypes.data_as(C.c_void_p)) == 0
            got = R.run(one_node(ex, t, t, T.T_BOOL), [R.Input(t, a), R.Input(t, b)], n, 2, L, use_numpy=use_numpy)
            assert np.array_equal(got.values, np.unpackbits(exp, bitorder="little")[:n].astype(bool)), (t, ex)


def exact(v):
    v = v.item() if hasattr(v, "item") else v
    return v if isinstance(v, int) or v != v or v in (float("inf"), float("-inf")) else Fraction(v)


def test_cast_matrix_equals_the_oracle_and_its_refusals_are_the_lossy_pairs(L):
    rng = np.random.default_rng(5)
    for src in R.NUMBERS:
        arr = interesting(NAME[src], rng)
        for dst in R.NUMBERS:
            with np.errstate(all="ignore"):
                out, ok, nerr = oracle_cast(L, arr, NAME[src], NAME[dst], False, False)
            keeps = nerr == 0 and all(exact(x) == exact(y) or (x != x and y != y) for x, y in zip(arr, out))
            assert R.lossless_cast(src, dst) == keeps, (src, dst)       # lossless: no value of the column is refused or changed
            prog = [(T.EX_LOAD, 0, 0, 0, src, 0, (0, 0)), (T.EX_CAST, 1, 0, 0, dst, 0, (0, 0))]
            if not keeps:
                with pytest.raises(R.Refused):
                    R.run(prog, [R.Input(src, arr)], len(arr), 1, L)
                continue
            got = R.run(prog, [R.Input(src, arr)], len(arr), 1, L)
            assert got.type == dst and R.same(got.values, out), (src, dst)
    d = R.run([(T.EX_LOAD, 0, 0, 0, T.T_DEC64, 0, (15, 2)), (T.EX_CAST, 1, 0, 0, T.T_DEC128, 0, (38, 2))],
              [R.Input(T.T_DEC64, [-5, 0, 10 ** 15 - 1], None, False, 15, 2)], 3, 1, L)
    assert d.values == [-5, 0, 10 ** 15 - 1] and d.size == (38, 2)
    for src, dst in ((T.T_DEC128, T.T_DEC64), (T.T_DEC64, T.T_I64), (T.T_I64, T.T_DEC64), (T.T_DEC128, T.T_F64)):
        assert not R.lossless_cast(src, dst)


def test_python_integer_and_numpy_evaluators_agree_on_every_generated_program(L):
    n = 257
    for case in EC.cases(L):
        inputs = EC.make_inputs(case, n)
        a = R.run(case.ins, inputs, n, case.root, L)
        b = R.run(case.ins, inputs, n, case.root, L, use_numpy=True)
        assert a.type == b.type == case.root_type and a.size == b.size
        assert a.values == b.values if a.type == T.T_DEC128 else R.same(a.values, b.values), case.seed
        assert np.array_equal(a.raising, b.raising) and a.raise_events == b.raise_events and (a.validity is None) == (b.validity is None)
        assert a.validity is None or np.array_equal(a.validity, b.validity)


def test_the_null_rule_on_hand_written_programs(L):
    n = 6
    a = np.array([1, 2, 3, 4, 5, 6], np.int64)
    z = np.array([0, 0, 1, 0, 2, 0], np.int64)
    va = np.array([1, 0, 1, 1, 0, 1], bool)
    vz = np.array([1, 1, 1, 0, 1, 0], bool)
    load2 = [(T.EX_LOAD, 0, 0, 0, T.T_I64, 0, (0, 0)), (T.EX_LOAD, 1, 1, 0, T.T_I64, 0, (0, 0))]
    # a divide by zero under a NULL (of either operand) does not raise; a raising row holds 0
    r = R.run(load2 + [(T.EX_DIVIDE, 2, 0, 1, T.T_F64, 0, (0, 0))], [R.Input(T.T_I64, a, va), R.Input(T.T_I64, z, vz)], n, 2, L)
    assert r.raising.tolist() == [0] and np.array_equal(r.validity, va & vz) and r.values[0] == 0.0 and r.values[2] == 3.0
    # IS_TRUE clears the dependency: the result is never NULL, and FALSE where the operand was NULL
    prog = load2 + [(T.EX_GT, 2, 0, 1, T.T_BOOL, 0, (0, 0)), (T.EX_IS_TRUE, 3, 2, 0, T.T_BOOL, 0, (0, 0))]
    r = R.run(prog, [R.Input(T.T_I64, a, va), R.Input(T.T_I64, z, vz)], n, 3, L)
    assert r.validity is None and r.values.tolist() == [True, False, True, False, False, False]
    # IF depends on then | else, not on what the (IS_TRUE'd) condition was computed from
    b = np.array([10, 20, 30, 40, 50, 60], np.int64)
    vb = np.array([1, 1, 0, 1, 1, 1], bool)
    prog = load2 + [(T.EX_LOAD, 2, 2, 0, T.T_I64, 0, (0, 0)), (T.EX_GT, 3, 1, 1, T.T_BOOL, 0, (0, 0)), (T.EX_IS_TRUE, 3, 3, 0, T.T_BOOL, 0, (0, 0)),
                    (T.EX_IF, 4, 3, 0, T.T_I64, 2, (0, 0))]
    r = R.run(prog, [R.Input(T.T_I64, a, va), R.Input(T.T_I64, z, vz), R.Input(T.T_I64, b, vb)], n, 4, L)
    assert np.array_equal(r.validity, va & vb) and r.values.tolist() == b.tolist()      # z > z is never TRUE: always the else branch
    with pytest.raises(R.Refused):                                                        # a nullable condition is not fused
        R.run(load2 + [(T.EX_GT, 2, 1, 1, T.T_BOOL, 0, (0, 0)), (T.EX_IF, 3, 2, 0, T.T_I64, 0, (0, 0))],
              [R.Input(T.T_I64, a), R.Input(T.T_I64, z, vz)], n, 3, L)
    with pytest.raises(R.Refused):                                                        # a branch that can raise is not fused
        R.run(load2 + [(T.EX_DIVIDE, 2, 0, 1, T.T_F64, 0, (0, 0)), (T.EX_GT, 3, 0, 1, T.T_BOOL, 0, (0, 0)), (T.EX_IF, 4, 3, 2, T.T_F64, 2, (0, 0))],
              [R.Input(T.T_I64, a), R.Input(T.T_I64, z)], n, 4, L)
    # a scalar has ONE validity bit: bit 0 clear makes every row NULL and nothing raises
    for bit in (False, True):
        r = R.run(load2 + [(T.EX_DIVIDE, 2, 0, 1, T.T_F64, 0, (0, 0))],
                  [R.Input(T.T_I64, a), R.Input(T.T_I64, np.array([0], np.int64), np.array([bit]), is_scalar=True)], n, 2, L)
        assert r.validity.tolist() == [bit] * n and r.raising.tolist() == (list(range(n)) if bit else [])


def test_generated_programs_stay_inside_the_limits_and_cover_what_the_gpu_test_claims(L):
    cs = EC.cases(L)
    assert len(cs) == len(EC.seed_list()) and len({tuple(c.ins) for c in cs}) > len(cs) - 3
    for c in cs:
        assert EC.within_limits(c) and EC.in_class(c), c.seed
        assert len([i for i in c.ins if i[0] != T.EX_LOAD]) <= EC.MAX_INS and c.live <= EC.MAX_LIVE
        for n in (1, 257):                             # well-typed: the reference accepts it (it raises Refused otherwise)
            r = R.run(c.ins, EC.make_inputs(c, n), n, c.root, L, use_numpy=True)
            assert r.type == c.root_type
    s = EC.census(cs)
    print({k: (dict(v) if hasattr(v, "items") else v) for k, v in s.items()})
    assert all(s["op"][name] >= 3 for name in EC.OP_NAMES), s["op"]
    assert all(s["root_type"][t] >= 3 and s["node_type"][t] >= 3 for t in EC.ALL_TYPES), (s["root_type"], s["node_type"])
    assert all(s["klass"][k] >= 3 for k in EC.KLASSES) and len(EC.KLASSES) == 15
    assert s["wide_if"] >= 3 and s["wide_cast"] >= 3 and s["live9"] >= 3
    assert s["scalar_inputs"] >= 3 and s["nullable_inputs"] >= 3 and s["x_op_x"] >= 3 and s["root_is_input"] >= 3
    # the generated data makes the programs do something: rows raise in some, stay valid in most
    raised = sum(len(R.run(c.ins, EC.make_inputs(c, 257), 257, c.root, L, use_numpy=True).raising) > 0 for c in cs)
    assert raised >= 10
