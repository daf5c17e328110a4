"""CPU: tests/float_ref.py — the reference the GPU module tests/test_gpu_float_edges.py asserts against — checked against the C oracle on
the same inputs (two independent statements of OrderedFloat's compare and of COUNT / SUM / MIN / MAX per group agree), and the checker
itself checked with four deliberately wrong aggregators that it must reject."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import float_ref as R
from tests import oracle_lib as O
from tests.test_gpu_parity import oracle_groupby, oracle_rows

FT = {np.dtype(np.float32): T.T_F32, np.dtype(np.float64): T.T_F64}
DTYPES = [np.float32, np.float64]


def case_aggs(dtype, nullable):
    """the device / oracle aggregate descriptors of float_ref.CASE_AGGS"""
    t, nul = FT[np.dtype(dtype)], 1 if nullable else 0
    return [(T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_I64, 0, 0, 0), (T.AGG_SUM, t, 0, 0, nul), (T.AGG_MIN, t, 0, 0, nul), (T.AGG_MAX, t, 0, 0, nul)]


def check_aggs(dtype):
    return [("count", None), ("sum", np.int64), ("sum", dtype), ("min", dtype), ("max", dtype)]


def oracle_case_rows(oracle, c):
    """the C oracle's AggregateHashTable over the rows of the case that pass the filter"""
    idx = np.arange(c["n"]) if c["keep"] is None else np.flatnonzero(c["keep"])
    t = FT[c["dtype"]]
    v = None if c["valid"] is None else c["valid"][idx]
    aggs = case_aggs(c["dtype"], v is not None)
    hargs = [None, O.HostCol(T.T_I64, c["i"][idx]), O.HostCol(t, c["fs"][idx], v), O.HostCol(t, c["fm"][idx], v), O.HostCol(t, c["fm"][idx], v)]
    h = oracle_groupby(oracle, [T.T_I64], [0], aggs, [O.HostCol(T.T_I64, c["key"][idx])], hargs, len(idx))
    rows = oracle_rows(oracle, h, [T.T_I64], aggs)
    oracle.orc_hashagg_destroy(h)
    return rows


def test_the_pool_holds_what_it_says():
    for p, dt, ut in ((R.POOL32, np.float32, np.uint32), (R.POOL64, np.float64, np.uint64)):
        assert p.dtype == dt and len(set(R.bits_of(p).tolist())) == len(p)
        fi = np.finfo(dt)
        nan = p[np.isnan(p)]
        assert len(nan) >= 4 and len(set(np.signbit(nan).tolist())) == 2
        for v in (np.inf, -np.inf, fi.max, -fi.max, fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal, np.nextafter(dt(1), dt(2)), np.nextafter(dt(1), dt(0)),
                  dt(0.1), dt(1) / dt(3)):
            assert np.any(p == dt(v)), v
        assert {0, 1 << (8 * p.itemsize - 1)} <= set(R.bits_of(p).tolist())           # +0.0 and -0.0
        assert np.any(p == np.nextafter(fi.tiny, dt(0))) and np.any(p == -np.nextafter(fi.tiny, dt(0)))     # largest subnormals
    assert 2.0 ** 24 + 1 in R.POOL64 and float(np.float32(2.0 ** 24 + 1)) != 2.0 ** 24 + 1
    assert not np.any(np.abs(R.SUM_POOL64[np.isfinite(R.SUM_POOL64)]) > R.MAX_SUM_ABS)


def test_of_cmp_is_the_total_order_the_definition_states():
    nan, pinf = R.NAN64, np.inf
    assert all(R.of_cmp(a, b) == 0 for a in nan for b in nan)
    assert all(R.of_cmp(a, x) == 1 and R.of_cmp(x, a) == -1 for a in nan for x in (pinf, -pinf, 0.0, 1e308))
    assert R.of_cmp(-0.0, 0.0) == 0 and R.of_cmp(0.0, -0.0) == 0
    assert R.of_cmp(-pinf, pinf) == -1 and R.of_cmp(5e-324, 0.0) == 1 and R.of_cmp(-5e-324, -0.0) == -1
    for p in (R.POOL32, R.POOL64):            # antisymmetric and transitive over the pool
        for a in p:
            for b in p:
                assert R.of_cmp(a, b) == -R.of_cmp(b, a)
        s = sorted(p.tolist(), key=lambda v: (v != v, v if v == v else 0.0))
        assert all(R.of_cmp(s[i], s[j]) <= 0 for i in range(len(s)) for j in range(i, len(s)))


def cross(p):
    """every ordered pair of the pool as two columns"""
    return np.repeat(p, len(p)), np.tile(p, len(p))


@pytest.mark.parametrize("dtype", DTYPES)
def test_of_cmp_equals_the_oracle_on_every_ordered_pair_of_the_pool(oracle, dtype):
    a, b = cross(R.pool(dtype))
    n, t = len(a), FT[np.dtype(dtype)]
    differs_from_ieee = 0
    for op, name in enumerate(R.CMP_OPS):
        exp = np.zeros((n + 7) // 8 + 8, np.uint8)
        ca, cb = O.HostCol(t, a).c(), O.HostCol(t, b).c()
        oracle.orc_cmp(op, C.byref(ca), C.byref(cb), C.c_int64(n), exp.ctypes.data_as(C.c_void_p))
        orc = np.unpackbits(exp, bitorder="little")[:n].astype(bool)
        assert np.array_equal(orc, R.cmp_expected(name, a, b)), name
        # negative control (d): the IEEE compare in place of of_cmp is rejected on these inputs, for every operator
        ieee = np.array([R.cmp_holds(name, R.ieee_cmp(x, y)) for x, y in zip(a, b)])
        assert not np.array_equal(orc, ieee), name
        differs_from_ieee += int((orc != ieee).sum())
    assert differs_from_ieee > 6 * len(R.pool(dtype))


CASES = [(n, card, dtype, nullable, filtered) for n, card in ((40, 12), (5000, 37), (20_000, 2500)) for dtype in DTYPES
         for nullable in (False, True) for filtered in (False, True)]


@pytest.mark.parametrize("n,card,dtype,nullable,filtered", CASES)
def test_agg_reference_equals_the_oracle(oracle, n, card, dtype, nullable, filtered):
    """float_ref.agg_expected against the oracle's hash aggregation (a sequential sum: inside the any-order bound) on the aggregation
    cases of the GPU module at small n: every planned group kind is there, every group is compared"""
    c = R.agg_case(np.random.default_rng(n + card), n, card, dtype, nullable, filtered)
    exp = R.case_expected(c)
    for kind, j in c["plan"].items():
        e = exp[(j,)]
        assert e[0]["count"] == 1 if kind == "single" else e[0]["count"] >= 3
        if kind == "all_null" and nullable:
            assert e[2]["count"] == 0 and e[3]["min"] is None
    assert R.mismatches(oracle_case_rows(oracle, c), exp, [np.int64], check_aggs(dtype)) == []


@pytest.mark.parametrize("dtype", DTYPES)
def test_sum_bound_holds_for_the_oracle_on_same_binade_values(oracle, dtype):
    c = R.binade_case(np.random.default_rng(5), dtype=dtype)
    assert R.mismatches(oracle_case_rows(oracle, c), R.case_expected(c), [np.int64], check_aggs(dtype)) == []


@pytest.mark.parametrize("second_key", [False, True])
@pytest.mark.parametrize("few", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_float_keys_group_by_bit_pattern_in_the_oracle(oracle, dtype, few, second_key):
    """-0.0 and 0.0 are two groups, two NaN payloads are two groups (row_match compares the stored bytes)"""
    c = R.key_case(np.random.default_rng(9), 3000, dtype, few, second_key)
    kt = [FT[np.dtype(dtype)]] + ([T.T_I64] if second_key else [])
    aggs = [(T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_I64, 0, 0, 0)]
    h = oracle_groupby(oracle, kt, [0] * len(kt), aggs, [O.HostCol(t, k) for t, k in zip(kt, c["keys"])], [None, O.HostCol(T.T_I64, c["i"])], c["n"])
    rows = oracle_rows(oracle, h, kt, aggs)
    oracle.orc_hashagg_destroy(h)
    assert len(rows) == len(c["exp"]) >= len(R.key_values(dtype, few))
    assert R.mismatches(rows, c["exp"], [dtype] + ([np.int64] if second_key else []), [("count", None), ("sum", np.int64)]) == []


# ---- negative controls: the checker must be able to fail ------------------------------------------------------------------------
def host_rows(c, wrong=None):
    """a host-side aggregator over an agg_case in the result-row format of the tables; wrong = None (right), 'f32' (SUM accumulated in
    float32), 'fminmax' (MIN / MAX with fmin / fmax semantics: NaN ignored), 'mask' (NULL and filtered rows multiplied by 0 instead of
    being left out)"""
    n, key, dt = c["n"], c["key"], c["dtype"]
    keep = np.ones(n, bool) if c["keep"] is None else c["keep"]
    valid = np.ones(n, bool) if c["valid"] is None else c["valid"]
    rows = []
    with np.errstate(all="ignore"):
        for k in np.unique(key[keep]):
            m = keep & (key == k)
            if wrong == "mask":
                g = key == k
                w = (keep & valid)[g]
                xs, xm, has = c["fs"][g].astype(np.float64) * w, c["fm"][g] * w.astype(dt), bool(w.any())
            else:
                xs, xm = c["fs"][m & valid].astype(np.float64), c["fm"][m & valid]
                has = len(xs) > 0
            if not has:
                rows.append((int(k), int(m.sum()), int(c["i"][m].sum()), None, None, None))
                continue
            s = float(np.cumsum(xs.astype(np.float32), dtype=np.float32)[-1]) if wrong == "f32" else float(np.cumsum(xs)[-1])     # sequential
            if wrong == "fminmax":
                mn, mx = np.fmin.reduce(xm), np.fmax.reduce(xm)
            else:
                nn = xm[~np.isnan(xm)]
                mn = nn.min() if len(nn) else np.nan
                mx = np.nan if len(nn) < len(xm) else nn.max()
            rows.append((int(k), int(m.sum()), int(c["i"][m].sum()), s, float(mn), float(mx)))
    return rows


@pytest.mark.parametrize("n,card,dtype,nullable,filtered", [c for c in CASES if c[0] == 5000])
def test_negative_controls_are_rejected(n, card, dtype, nullable, filtered):
    c = R.agg_case(np.random.default_rng(n + card), n, card, dtype, nullable, filtered)
    exp, aggs = R.case_expected(c), check_aggs(dtype)
    assert R.mismatches(host_rows(c), exp, [np.int64], aggs) == []                       # the right aggregator passes
    bad = R.mismatches(host_rows(c, "f32"), exp, [np.int64], aggs)                       # (a)
    assert bad and all(b[2] == "sum" for b in bad)
    bad = R.mismatches(host_rows(c, "fminmax"), exp, [np.int64], aggs)                   # (b): at least the one-NaN group's MAX
    assert bad and all(b[2] in ("min", "max") for b in bad) and any(b[0] == (c["plan"]["one_nan"],) and b[2] == "max" for b in bad)
    if nullable or filtered:                                                              # (c): 0 * NaN, 0 * Inf
        assert R.mismatches(host_rows(c, "mask"), exp, [np.int64], aggs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_float32_accumulation_is_rejected_on_same_binade_values(dtype):
    """negative control (a) where it is hardest to see: no overflow, no special value, 20 000 values of one magnitude per group"""
    c = R.binade_case(np.random.default_rng(5), dtype=dtype)
    exp, aggs = R.case_expected(c), check_aggs(dtype)
    assert R.mismatches(host_rows(c), exp, [np.int64], aggs) == []
    bad = R.mismatches(host_rows(c, "f32"), exp, [np.int64], aggs)
    assert len(bad) == len(exp) and all(b[2] == "sum" for b in bad)                      # every group's SUM


def test_same_value_and_sum_ok_reject_what_they_should():
    f32, f64 = np.float32, np.float64
    assert R.same_value(R.NAN64[0], R.NAN64[3], f64) and R.same_value(-0.0, 0.0, f64) and not R.same_value(-0.0, 0.0, f64, strict_zero=True)
    assert not R.same_value(np.nan, np.inf, f64) and not R.same_value(0.0, R.SUB64[0], f64) and not R.same_value(0.0, float(R.SUB32[0]), f32)   # a flushed subnormal
    assert not R.same_value(float(f32(0.1)), 0.1, f64) and R.same_value(0.1, float(f32(0.1)), f32) and not R.same_value(1.0, float(np.nextafter(f32(1), f32(2))), f32)
    assert R.same_value(None, None, f64) and not R.same_value(None, 0.0, f64) and not R.same_value(np.nan, None, f64)
    assert R.sum_ok(0.1 + 0.2, R.sum_expected([0.1, 0.2])) and not R.sum_ok(0.3 + 2 ** -50, R.sum_expected([0.1, 0.2]))
    assert R.sum_ok(1.5, R.sum_expected([1.5])) and not R.sum_ok(np.nextafter(1.5, 2), R.sum_expected([1.5]))           # one term: exact
    assert not R.sum_ok(0.0, R.sum_expected([R.SUB64[0]] * 3)) and R.sum_ok(3 * R.SUB64[0], R.sum_expected([R.SUB64[0]] * 3))
    for xs, cls in (([1.0, np.nan], "nan"), ([np.inf, -np.inf], "nan"), ([np.inf, 1.0], "+inf"), ([-np.inf, 1.0], "-inf")):
        e = R.sum_expected(xs)
        assert e[0] == cls
        for got in (np.nan, np.inf, -np.inf, 1.0):
            assert R.sum_ok(got, e) == ({"nan": np.isnan(got), "+inf": got == np.inf, "-inf": got == -np.inf}[cls])
    with pytest.raises(AssertionError):
        R.sum_ok(0.0, R.sum_expected([R.MAX64[0], 1.0]))
