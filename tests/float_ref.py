"""The reference for floats at their edges (NaN, +-Inf, signed zeros, subnormals, +-MAX, non-integers) in the hash aggregation and
the comparisons: plain Python / numpy on float64 and math.fsum, independent of the C oracle and of the device code.

* POOL32 / POOL64         the adversarial values (built from bit patterns, so payloads and signs are what they say)
* of_cmp / cmp_holds      OrderedFloat's three-way compare, stated from its definition (types/number.rs: NaN == NaN, NaN largest)
* agg_expected            COUNT / MIN / MAX / SUM per group; the group of a float KEY is its stored bit pattern
* same_value / sum_ok     the two equivalences the tests assert: exact (up to the NaN payload and, among both zeros, the sign) for
                          MIN / MAX and stored values; the any-order error bound of n - 1 IEEE double additions for SUM
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53            # unit roundoff of IEEE double
MAX_SUM_ABS = 1e290       # |x| of a finite SUM input: with <= 2^20 rows per group no partial sum overflows in any order
MAX_SUM_ROWS = 1 << 20


# ---- the pool -------------------------------------------------------------------------------------------------------------------
def _f32(*bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def _f64(*bits):
    return np.array(bits, dtype=np.uint64).view(np.float64)


NAN32 = _f32(0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFD2345F)            # quiet NaNs: both signs, two payloads each
NAN64 = _f64(0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0xFFFA5A5A12345678)
INF32, INF64 = _f32(0x7F800000, 0xFF800000), _f64(0x7FF0000000000000, 0xFFF0000000000000)
ZERO32, ZERO64 = _f32(0x00000000, 0x80000000), _f64(0x0000000000000000, 0x8000000000000000)
SUB32 = _f32(0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF)            # smallest / largest subnormal, both signs
SUB64 = _f64(0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF)
MAX32, MAX64 = _f32(0x7F7FFFFF, 0xFF7FFFFF), _f64(0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF)
_ORD32 = np.concatenate([_f32(0x00800000, 0x3F800001, 0x3F7FFFFF),      # smallest normal, 1 + ulp, 1 - ulp
                         np.array([0.1, 1.0 / 3.0, 1.0, -1.0, 5.0, -2.5, 16777216.0], dtype=np.float32)])
_ORD64 = np.concatenate([_f64(0x0010000000000000, 0x3FF0000000000001, 0x3FEFFFFFFFFFFFFF),
                         np.array([0.1, 1.0 / 3.0, 1.0, -1.0, 5.0, -2.5, 2.0 ** 24 + 1], dtype=np.float64)])   # 2^24 + 1 is not an f32

SUM_POOL32 = np.concatenate([NAN32, INF32, ZERO32, SUB32, MAX32, _ORD32])     # +-FLT_MAX is far below MAX_SUM_ABS in a double sum
SUM_POOL64 = np.concatenate([NAN64, INF64, ZERO64, SUB64, _ORD64])            # +-DBL_MAX: MIN / MAX / compare only
POOL32 = SUM_POOL32
POOL64 = np.concatenate([SUM_POOL64, MAX64])


def pool(dtype, for_sum=False):
    if np.dtype(dtype) == np.float32:
        return SUM_POOL32 if for_sum else POOL32
    return SUM_POOL64 if for_sum else POOL64


def draws(rng, n, dtype):
    """real-valued draws over many binades, |x| <= MAX_SUM_ABS"""
    lo, hi = (-30, 30) if np.dtype(dtype) == np.float32 else (-280, 280)
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(lo, hi, n)).astype(dtype)
    assert np.all(np.abs(x.astype(np.float64)) <= MAX_SUM_ABS)
    return x


def mixed(rng, n, dtype, for_sum=False, p_pool=0.2):
    """n values: a pool value with probability p_pool per row, a real-valued draw otherwise"""
    x = draws(rng, n, dtype)
    p = pool(dtype, for_sum)
    pick = rng.random(n) < p_pool
    x[pick] = p[rng.integers(0, len(p), int(pick.sum()))]
    return x


def bits_of(a):
    """the stored bit patterns of a float (or integer) array as unsigned integers of the same width"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- OrderedFloat ---------------------------------------------------------------------------------------------------------------
def of_cmp(a, b):
    """-1 / 0 / +1. NaN equals NaN whatever its sign or payload; NaN is greater than everything else, +Inf included; -0.0 equals
    0.0; everything else in the IEEE order."""
    a, b = float(a), float(b)          # f32 -> f64 is exact and keeps the order
    if math.isnan(a) and math.isnan(b):
        return 0
    if math.isnan(a):
        return 1
    if math.isnan(b):
        return -1
    if a == 0.0 and b == 0.0:
        return 0
    return -1 if a < b else (1 if a > b else 0)


CMP_OPS = ("eq", "noteq", "lt", "lte", "gt", "gte")       # in the order of DBHIP_CMP_EQ .. DBHIP_CMP_GTE


def cmp_holds(op, c):
    return {"eq": c == 0, "noteq": c != 0, "lt": c < 0, "lte": c <= 0, "gt": c > 0, "gte": c >= 0}[op]


def cmp_expected(op, a, b):
    """bool array: a[i] op b[i] under of_cmp (a or b may have length 1: a scalar operand)"""
    n = max(len(a), len(b))
    return np.array([cmp_holds(op, of_cmp(a[i if len(a) > 1 else 0], b[i if len(b) > 1 else 0])) for i in range(n)], dtype=bool)


def cmp3_array(a, b):
    """of_cmp per row as an int8 array (a or b may have length 1: a scalar operand)"""
    n = max(len(a), len(b))
    return np.array([of_cmp(a[i if len(a) > 1 else 0], b[i if len(b) > 1 else 0]) for i in range(n)], dtype=np.int8)


def holds_array(op, c3):
    return {"eq": c3 == 0, "noteq": c3 != 0, "lt": c3 < 0, "lte": c3 <= 0, "gt": c3 > 0, "gte": c3 >= 0}[op]


def ieee_cmp(a, b):
    """the WRONG compare (hardware semantics: every ordered test on a NaN is false) — negative controls only"""
    a, b = float(a), float(b)
    return -1 if a < b else (1 if a > b else 0)


# ---- the checks -----------------------------------------------------------------------------------------------------------------
def same_value(got, exp, dtype, strict_zero=False):
    """MIN / MAX results and stored values: both NaN, or both zero (either sign; strict_zero: the same sign), or bit-identical in the
    result's own type (so a flushed subnormal or a double rounding of an f32 fails)."""
    if got is None or exp is None:
        return got is None and exp is None
    g, e = np.array([got]).astype(dtype), np.array([exp]).astype(dtype)
    if np.isnan(g[0]) or np.isnan(e[0]):
        return bool(np.isnan(g[0]) and np.isnan(e[0]))
    if g[0] == 0 and e[0] == 0 and not strict_zero:
        return True
    return bool(bits_of(g)[0] == bits_of(e)[0])


def gamma(k):
    return k * U / (1 - k * U)


def sum_expected(x):
    """(class, fsum of the finite terms, fsum of their absolute values, number of terms) of the float values x (an f32 widens exactly);
    class: 'nan' (a NaN term, or both infinities) | '+inf' | '-inf' | 'finite'"""
    x = [float(v) for v in x]
    fin = [v for v in x if math.isfinite(v)]
    if len(x) > MAX_SUM_ROWS or any(abs(v) > MAX_SUM_ABS for v in fin):
        return ("out of bounds", 0.0, 0.0, len(x))         # a MIN / MAX column (+-DBL_MAX): sum_ok refuses to judge a SUM over it
    pinf, ninf = math.inf in x, -math.inf in x
    cls = "nan" if any(v != v for v in x) or (pinf and ninf) else "+inf" if pinf else "-inf" if ninf else "finite"
    return (cls, math.fsum(fin), math.fsum(abs(v) for v in fin), len(x))


def sum_ok(got, exp):
    """class exactly; a finite sum within gamma(n - 1) * sum|x| of the exact one — the bound for ANY order and ANY tree of n - 1 IEEE
    double additions (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), evaluated in exact rational arithmetic"""
    if got is None or exp is None:
        return got is None and exp is None
    cls, s, sabs, n = exp
    assert cls != "out of bounds", "a SUM input outside |x| <= MAX_SUM_ABS, n <= MAX_SUM_ROWS: gamma is no bound there"
    got = float(got)
    if cls == "nan":
        return math.isnan(got)
    if cls == "+inf":
        return got == math.inf
    if cls == "-inf":
        return got == -math.inf
    if not math.isfinite(got):
        return False
    return abs(Fraction(got) - Fraction(s)) <= Fraction(gamma(max(n - 1, 0))) * Fraction(sabs)


# ---- aggregation ----------------------------------------------------------------------------------------------------------------
def key_ids(col, valid=None):
    """group identity of one key column per row: the stored bit pattern of a float (-0.0 and 0.0 are two groups, two NaN payloads are
    two groups: the reference's row_match compares the stored bytes), the value of an integer, None for NULL"""
    col = np.asarray(col)
    ids = (bits_of(col) if col.dtype.kind == "f" else col).tolist()
    if valid is not None:
        ids = [i if v else None for i, v in zip(ids, valid)]
    return ids


def extreme(vals, want_max):
    """MIN / MAX of a non-empty list of floats by of_cmp, as a value: NaN is the largest, so MAX is a NaN as soon as one is there and
    MIN is one only when nothing else is. Among equals (NaNs; -0.0 and 0.0) the reference's choice depends on the row order, so any of
    them is right: same_value says so."""
    nn = [v for v in vals if v == v]
    if want_max:
        return math.nan if len(nn) < len(vals) else max(nn)
    return min(nn) if nn else math.nan


def one_signed_zero(vals):
    """every value is a zero of ONE sign: that sign must come back from MIN / MAX (same_value's strict_zero)"""
    return all(v == 0 for v in vals) and len({math.copysign(1.0, v) for v in vals}) == 1


def agg_expected(keys, valid_keys, args, valid_args, keep=None):
    """keys: key columns (numpy), valid_keys: their validity (bool arrays or None); args: argument columns (float32 / float64 / integer
    numpy arrays, Python-int lists, or None = count(*)), valid_args likewise; keep: the rows that pass the filter (None: all).
    -> {group id tuple: [per argument dict(count, min, max, sum, strict_zero)]}
    count = rows of the group whose argument is not NULL; min / max / sum are None when that is 0; sum of a float argument is the
    sum_expected tuple, of an integer argument the exact Python int."""
    n = len(keys[0])
    rows = range(n) if keep is None else np.flatnonzero(keep).tolist()
    ids = [key_ids(k, v) for k, v in zip(keys, valid_keys)]
    groups = {}
    for r in rows:
        groups.setdefault(tuple(i[r] for i in ids), []).append(r)
    isf = [a is not None and not isinstance(a, list) and a.dtype.kind == "f" for a in args]
    cols = [a if a is None or isinstance(a, list) else a.tolist() for a in args]        # Python floats / ints (f32 -> f64: exact)
    vas = [None if v is None else np.asarray(v).tolist() for v in valid_args]
    out = {}
    for gid, rr in groups.items():
        res = []
        for a, va, f in zip(cols, vas, isf):
            if a is None:
                res.append(dict(count=len(rr), min=None, max=None, sum=None, strict_zero=False))
                continue
            vals = [a[i] for i in rr] if va is None else [a[i] for i in rr if va[i]]
            d = dict(count=len(vals), min=None, max=None, sum=None, strict_zero=False)
            if vals and f:
                d.update(min=extreme(vals, False), max=extreme(vals, True), sum=sum_expected(vals), strict_zero=one_signed_zero(vals))
            elif vals:
                d.update(min=min(vals), max=max(vals), sum=sum(vals))
            res.append(d)
        out[gid] = res
    return out


# ---- the aggregation cases (shared by the CPU and the GPU module) ---------------------------------------------------------------
KINDS = ("all_nan", "one_nan", "pos_inf", "both_inf", "neg_zero", "both_zero", "subnormal", "all_null", "single")


def agg_case(rng, n, card, dtype, nullable, filtered, kinds=KINDS):
    """One aggregation input: an int64 key column with `card` groups of which the first len(kinds) follow a plan (KINDS: what the
    rows that reach the aggregate hold in that group), a SUM column `fs` (and a second one, `fy`, for maps) and a MIN / MAX column `fm` of `dtype` (pool value with
    probability 0.2, real-valued otherwise; the non-finite ones in every fourth group only; +-DBL_MAX only in fm), an int64 column, a validity (nullable) and a filter Bitmap
    (filtered) — with NaN / +-Inf under every NULL and every dropped row. 'all_null' needs nullable; without it the group is ordinary."""
    dtype = np.dtype(dtype)
    P = len(kinds)
    assert n >= 3 * P and card >= 1
    key = rng.integers(0, max(card, P), n).astype(np.int64)
    forced = []                                       # (row, group): three rows per planned group, ONE for 'single'
    for j, kind in enumerate(kinds):
        forced += [(len(forced) + t, j) for t in range(1 if kind == "single" else 3)]
    if "single" in kinds:
        j = kinds.index("single")
        key[key == j] = (j + 1) % max(card, P) if max(card, P) > 1 else j
    rows = rng.permutation(n)[:len(forced)]           # spread over the blocks of a multi-block run
    for r, (_, j) in zip(rows, forced):
        key[r] = j
    valid = rng.random(n) > 0.25 if nullable else None
    keep = rng.random(n) < 0.7 if filtered else None
    for v in (valid, keep):
        if v is not None:
            v[rows] = True
    fs, fm, fy = mixed(rng, n, dtype, for_sum=True), mixed(rng, n, dtype), mixed(rng, n, dtype, for_sum=True)
    for x, for_sum in ((fs, True), (fm, False), (fy, True)):      # NaN / +-Inf only in every fourth group: the others keep a finite SUM and a numeric MAX
        p = pool(dtype, for_sum)
        p = p[np.isfinite(p)]
        idx = np.flatnonzero((key % 4 != 0) & ~np.isfinite(x))
        x[idx] = p[rng.integers(0, len(p), len(idx))]
    nan, inf, zero, sub = (NAN32, INF32, ZERO32, SUB32) if dtype == np.float32 else (NAN64, INF64, ZERO64, SUB64)
    eff = np.ones(n, bool)
    if valid is not None:
        eff &= valid
    if keep is not None:
        eff &= keep
    for j, kind in enumerate(kinds):
        idx = np.flatnonzero((key == j) & eff)
        m = len(idx)
        cyc = lambda vals: vals[np.arange(m) % len(vals)]     # noqa: E731
        if kind == "all_nan":
            v = cyc(nan)
        elif kind == "one_nan":
            v = draws(rng, m, dtype)
            v[m // 2] = nan[3]
        elif kind == "pos_inf":
            v = cyc(inf[:1])
        elif kind == "both_inf":
            v = cyc(inf)
        elif kind == "neg_zero":
            v = cyc(zero[1:])
        elif kind == "both_zero":
            v = cyc(zero)
        elif kind == "subnormal":
            v = cyc(sub)
        elif kind == "all_null":
            if valid is not None:
                valid[key == j] = False
                eff[key == j] = False
            continue
        else:
            v = draws(rng, m, dtype)
        fs[idx], fm[idx], fy[idx] = v, v, v[::-1]
    hidden = np.flatnonzero(~eff)                      # NULL or dropped: what lies under them must not reach any state
    bad = np.concatenate([nan, inf])
    fs[hidden] = bad[rng.integers(0, len(bad), len(hidden))]
    fm[hidden] = bad[rng.integers(0, len(bad), len(hidden))]
    fy[hidden] = bad[rng.integers(0, len(bad), len(hidden))]
    i64 = rng.integers(-10**9, 10**9, n).astype(np.int64)
    return dict(n=n, key=key, fs=fs, fm=fm, fy=fy, i=i64, valid=valid, keep=keep, dtype=dtype, plan={k: j for j, k in enumerate(kinds)})


# the aggregates every case runs, in this order: COUNT(*), SUM(i64), SUM(fs), MIN(fm), MAX(fm) — (kind, column of the case)
CASE_AGGS = (("count", None), ("sum", "i"), ("sum", "fs"), ("min", "fm"), ("max", "fm"))


def case_expected(c, extra_keys=(), extra_args=(), sum_col=None):
    """agg_expected of an agg_case (extra_keys: more key columns in front of `key`; extra_args: [(kind, column, validity)] behind;
    sum_col: a float column computed from fs / fy that takes the place of fs under SUM and of fm under MIN)"""
    args = [None if col is None else c[col] for _, col in CASE_AGGS] + [a[1] for a in extra_args]
    if sum_col is not None:
        args[2], args[3] = sum_col, sum_col
    va = [c["valid"] if col in ("fs", "fm") else None for _, col in CASE_AGGS] + [a[2] for a in extra_args]
    keys = list(extra_keys) + [c["key"]]
    return agg_expected(keys, [None] * len(keys), args, va, c["keep"])


def mismatches(rows, exp, key_dtypes, aggs):
    """rows: result rows (key values..., aggregate values...; NULL = None) of a table; exp: agg_expected's dict; key_dtypes: numpy
    dtype per key; aggs: [(kind, numpy dtype of the ARGUMENT or None)] per aggregate -> the list of disagreements (empty = equal).
    Every group of `exp` is looked at, none is left out; float results are compared with same_value / sum_ok only."""
    bad = []
    nk = len(key_dtypes)
    seen = set()
    for r in rows:
        gid = tuple(None if v is None else int(bits_of(np.array([v], dtype=dt))[0]) if np.dtype(dt).kind == "f" else int(v)
                    for v, dt in zip(r[:nk], key_dtypes))
        if gid in seen or gid not in exp:
            bad.append(("unexpected or repeated group", gid))
            continue
        seen.add(gid)
        for a, ((kind, dt), got, e) in enumerate(zip(aggs, r[nk:], exp[gid])):
            isf = dt is not None and np.dtype(dt).kind == "f"
            if kind == "count":
                ok = got == e["count"]
            elif kind == "sum":
                ok = sum_ok(got, e["sum"]) if isf else got == e["sum"]
            else:
                ok = same_value(got, e[kind], dt, e["strict_zero"]) if isf else got == e[kind]
            if not ok:
                bad.append((gid, a, kind, got, e[kind if kind != "count" else "count"]))
    bad += [("missing group", gid) for gid in exp if gid not in seen]
    return bad


def binade_case(rng, n=60_000, groups=3, dtype=np.float64):
    """the SUM case that keeps the float32-accumulation control decisive: <= 20 000 rows per group, every value N(0, 1000^2) (one or
    two binades), no pool value — the any-order bound is ~n * 2^-53 * sum|x| there, an f32 running sum misses it by orders of magnitude"""
    key = (np.arange(n) % groups).astype(np.int64)
    f = (rng.standard_normal(n) * 1000).astype(dtype)
    return dict(n=n, key=key, fs=f, fm=f.copy(), fy=f.copy(), i=rng.integers(-10**9, 10**9, n).astype(np.int64), valid=None, keep=None, dtype=np.dtype(dtype), plan={})


def key_values(dtype, few=False):
    """float GROUP BY keys: both zeros, two NaN payloads (and, in the long form, both signs of each), +-Inf, subnormals, ordinary values"""
    nan, inf, zero, sub = (NAN32, INF32, ZERO32, SUB32) if np.dtype(dtype) == np.float32 else (NAN64, INF64, ZERO64, SUB64)
    if few:
        return np.concatenate([zero, nan[[0, 2]], inf[:1], sub[:1], np.array([1.5, -2.5], dtype=dtype)])       # 8 keys
    return np.concatenate([zero, nan, inf, sub, np.array([1.5, -2.5, 0.1, 1.0 / 3.0, 1e30, -1e-30], dtype=dtype)])


def key_case(rng, n, dtype, few=False, second_key=False):
    """rows whose float key is drawn from key_values (every value at least once); COUNT(*) and SUM(i64) are what is aggregated"""
    kv = key_values(dtype, few)
    pick = rng.integers(0, len(kv), n)
    pick[:len(kv)] = np.arange(len(kv))
    fk = kv[rng.permutation(pick)]
    k2 = rng.integers(0, 3 if not few else 1, n).astype(np.int64)
    i64 = rng.integers(-10**9, 10**9, n).astype(np.int64)
    keys = [fk, k2] if second_key else [fk]
    return dict(n=n, keys=keys, i=i64, exp=agg_expected(keys, [None] * len(keys), [None, i64], [None, None]))
