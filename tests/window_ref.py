"""What the window calls promise (include/dbhip.h, a19), stated in plain Python over plain values, and nothing about how the device gets
there: partition and peer boundaries from `sort_ref.compare_rows(...) == 0` on neighbouring rows, the frame rule, the rank family,
lag / lead, first / last / nth value and COUNT / SUM / MIN / MAX over a frame, all by loops.

Two statements of it: the loops (`boundaries`, `frame_of`, `rank`, `shift`, `value`, `aggregate`) and the numpy twins (`*_fast`) for the
sizes at which the loops are too slow. tests/test_window_ref_cpu.py proves the twins equal to the loops and the loops equal to sqlite3's
window functions, and shows that the shared cases reject six wrong implementations.

Values travel as (values, valid): values = a numpy array or a list, valid = None or a bool array. Results are lists with None for NULL;
a float SUM is the tuple of `float_ref.sum_expected` over the frame's own valid terms (compare with `float_ref.sum_ok`).

The rest is the seeded case builder and the case lists that the CPU and the GPU module share."""
import math
from fractions import Fraction

import numpy as np

from tests import float_ref as F
from tests import sort_ref as R

ROWS, RANGE = 0, 1
UNBOUNDED_PRECEDING, PRECEDING, CURRENT_ROW, FOLLOWING, UNBOUNDED_FOLLOWING = range(5)
ROW_NUMBER, RANK, DENSE_RANK, PERCENT_RANK, CUME_DIST, NTILE = range(6)
FIRST_VALUE, LAST_VALUE, NTH_VALUE = range(3)
COUNT, SUM, MIN, MAX = range(4)
OK, INVALID, UNSUPPORTED = 0, 1, 7          # DBHIP_OK, DBHIP_ERR_INVALID, DBHIP_ERR_UNSUPPORTED


class Frame:
    """units, (start kind, offset), (end kind, offset)"""

    def __init__(self, units, start, end):
        self.units = units
        self.sk, self.so = start if isinstance(start, tuple) else (start, 0)
        self.ek, self.eo = end if isinstance(end, tuple) else (end, 0)

    def sql(self):
        def bound(k, o):
            return ["UNBOUNDED PRECEDING", f"{o} PRECEDING", "CURRENT ROW", f"{o} FOLLOWING", "UNBOUNDED FOLLOWING"][k]
        return f"{'ROWS' if self.units == ROWS else 'RANGE'} BETWEEN {bound(self.sk, self.so)} AND {bound(self.ek, self.eo)}"

    def __repr__(self):
        return self.sql().replace(" ", "_")


def frame_status(f):
    """OK, INVALID or UNSUPPORTED, as the contract lists them"""
    s_off, e_off = f.sk in (PRECEDING, FOLLOWING), f.ek in (PRECEDING, FOLLOWING)
    if f.units not in (ROWS, RANGE) or not 0 <= f.sk <= 4 or not 0 <= f.ek <= 4:
        return INVALID
    if (s_off and f.so < 0) or (e_off and f.eo < 0):
        return INVALID
    if f.sk == UNBOUNDED_FOLLOWING or f.ek == UNBOUNDED_PRECEDING or f.sk > f.ek:
        return INVALID
    if f.sk == f.ek == PRECEDING and f.so < f.eo:
        return INVALID
    if f.sk == f.ek == FOLLOWING and f.so > f.eo:
        return INVALID
    if f.units == RANGE and (s_off or e_off):
        return UNSUPPORTED
    return OK


# ---- the loops ------------------------------------------------------------------------------------------------------------------
def boundaries(part_cols, order_cols, n):
    """-> part_start, part_end, peer_start, peer_end (lists). part_cols / order_cols: lists of sort_ref.KeyCol"""
    zp, zo = [0] * len(part_cols), [0] * len(order_cols)
    ps, qs = [0] * n, [0] * n
    for i in range(n):
        same_part = i > 0 and R.compare_rows(part_cols, i - 1, part_cols, i, zp, zp) == 0
        same_peer = same_part and R.compare_rows(order_cols, i - 1, order_cols, i, zo, zo) == 0
        ps[i] = ps[i - 1] if same_part else i
        qs[i] = qs[i - 1] if same_peer else i
    pe, qe = [n] * n, [n] * n
    for i in range(n - 2, -1, -1):
        pe[i] = pe[i + 1] if ps[i + 1] == ps[i] else i + 1
        qe[i] = qe[i + 1] if qs[i + 1] == qs[i] else i + 1
    return ps, pe, qs, qe


def clamp(x, lo, hi):
    return lo if x < lo else hi if x > hi else x


def frame_of(f, i, ps, pe, qs, qe):
    """[lo, hi) of row i; hi <= lo is an empty frame"""
    assert frame_status(f) == OK
    if f.sk == UNBOUNDED_PRECEDING:
        lo = ps
    elif f.sk == CURRENT_ROW:
        lo = qs if f.units == RANGE else i
    else:
        lo = i - f.so if f.sk == PRECEDING else i + f.so
    if f.ek == UNBOUNDED_FOLLOWING:
        hi = pe
    elif f.ek == CURRENT_ROW:
        hi = qe if f.units == RANGE else i + 1
    else:
        hi = i - f.eo + 1 if f.ek == PRECEDING else i + f.eo + 1
    return clamp(lo, ps, pe), clamp(hi, ps, pe)


def rank(kind, b, buckets=0):
    ps, pe, qs, qe = b
    n = len(ps)
    out = []
    dense = 0
    for i in range(n):
        rows, k = pe[i] - ps[i], i - ps[i]
        if kind == ROW_NUMBER:
            out.append(k + 1)
        elif kind == RANK:
            out.append(qs[i] - ps[i] + 1)
        elif kind == DENSE_RANK:
            dense = 1 if ps[i] == i else dense + (1 if qs[i] == i else 0)
            out.append(dense)
        elif kind == PERCENT_RANK:
            out.append(0.0 if rows == 1 else (qs[i] - ps[i]) / (rows - 1))
        elif kind == CUME_DIST:
            out.append((qe[i] - ps[i]) / rows)
        else:
            q, r = divmod(rows, buckets)
            out.append(k // (q + 1) + 1 if k < r * (q + 1) else (k - r * (q + 1)) // q + r + 1)
    return out


def _get(vals, valid, i):
    return vals[i] if valid is None or valid[i] else None


def shift(b, vals, valid, offset, default=None):
    """default: None (NULL) | ('scalar', value or None) | ('column', values, valid)"""
    ps, pe, _, _ = b
    out = []
    for i in range(len(ps)):
        j = i + offset
        if ps[i] <= j < pe[i]:
            out.append(_get(vals, valid, j))
        elif default is None:
            out.append(None)
        elif default[0] == "scalar":
            out.append(default[1])
        else:
            out.append(_get(default[1], default[2], i))
    return out


def value(kind, b, vals, valid, f, nth=1):
    ps, pe, qs, qe = b
    out = []
    for i in range(len(ps)):
        lo, hi = frame_of(f, i, ps[i], pe[i], qs[i], qe[i])
        j = lo if kind == FIRST_VALUE else hi - 1 if kind == LAST_VALUE else lo + nth - 1
        out.append(_get(vals, valid, j) if hi > lo and lo <= j < hi else None)
    return out


def wrap(x, bits, signed):
    x &= (1 << bits) - 1
    return x - (1 << bits) if signed and x >> (bits - 1) else x


def sum_mode(kind):
    """how a SUM over a column of `kind` accumulates: ('int', bits, signed) or 'float'"""
    if kind in R.FLOAT_KINDS:
        return "float"
    if kind == "dec128":
        return ("int", 128, True)
    return ("int", 64, not kind.startswith("u"))


def aggregate(agg, b, vals, valid, f, kind="i64"):
    """vals = None: count(*). kind = the sort_ref kind of the argument (decides wrapping and the float rules)"""
    ps, pe, qs, qe = b
    out = []
    mode = sum_mode(kind)
    for i in range(len(ps)):
        lo, hi = frame_of(f, i, ps[i], pe[i], qs[i], qe[i])
        if vals is None:
            out.append(max(hi - lo, 0))
            continue
        terms = [vals[j] for j in range(lo, hi) if valid is None or valid[j]]        # the value under a NULL is never read
        if agg == COUNT:
            out.append(len(terms))
        elif not terms:
            out.append(None)
        elif agg == SUM:
            out.append(F.sum_expected(terms) if mode == "float" else wrap(sum(int(t) for t in terms), mode[1], mode[2]))
        elif mode == "float":
            out.append(F.extreme([float(t) for t in terms], agg == MAX))
        else:
            out.append(max(terms) if agg == MAX else min(terms))
    return out


# ---- the numpy twins ------------------------------------------------------------------------------------------------------------
def boundaries_fast(part_cols, order_cols, n):
    def heads(cols, base):
        h = base.copy()
        if cols:
            ranks = R.rank_keys(cols, [0] * len(cols), [0] * len(cols))
            h[1:] |= np.any(ranks[:, 1:] != ranks[:, :-1], axis=0)
        return h
    first = np.zeros(n, bool)
    if n:
        first[0] = True
    ph = heads(part_cols, first)
    qh = heads(order_cols, ph)
    idx = np.arange(n, dtype=np.int64)

    def spans(h):
        start = np.maximum.accumulate(np.where(h, idx, 0))
        nxt = np.where(h, idx, n)
        after = np.concatenate([nxt[1:], np.array([n], np.int64)])
        end = np.minimum.accumulate(after[::-1])[::-1]
        return start, end
    ps, pe = spans(ph)
    qs, qe = spans(qh)
    return ps, pe, qs, qe


def frames_fast(f, b):
    ps, pe, qs, qe = (np.asarray(x, dtype=object if max(f.so, f.eo) >= 2**62 else np.int64) for x in b)
    i = np.arange(len(ps), dtype=ps.dtype)
    lo = ps if f.sk == UNBOUNDED_PRECEDING else (qs if f.units == RANGE else i) if f.sk == CURRENT_ROW else i - f.so if f.sk == PRECEDING else i + f.so
    hi = pe if f.ek == UNBOUNDED_FOLLOWING else (qe if f.units == RANGE else i + 1) if f.ek == CURRENT_ROW else i - f.eo + 1 if f.ek == PRECEDING else i + f.eo + 1
    lo = np.minimum(np.maximum(lo, ps), pe).astype(np.int64)
    hi = np.minimum(np.maximum(hi, ps), pe).astype(np.int64)
    return lo, hi


def rank_fast(kind, b, buckets=0):
    ps, pe, qs, qe = (np.asarray(x, dtype=np.int64) for x in b)
    n = len(ps)
    i = np.arange(n, dtype=np.int64)
    rows, k = pe - ps, i - ps
    if kind == ROW_NUMBER:
        return (k + 1).astype(np.uint64)
    if kind == RANK:
        return (qs - ps + 1).astype(np.uint64)
    if kind == DENSE_RANK:
        h = np.cumsum(qs == i)
        return (h - h[ps] + 1).astype(np.uint64) if n else np.zeros(0, np.uint64)
    if kind == PERCENT_RANK:
        return np.where(rows == 1, 0.0, (qs - ps).astype(np.float64) / np.maximum(rows - 1, 1).astype(np.float64))
    if kind == CUME_DIST:
        return (qe - ps).astype(np.float64) / rows.astype(np.float64)
    q, r = rows // buckets, rows % buckets
    return np.where(k < r * (q + 1), k // (q + 1) + 1, (k - r * (q + 1)) // np.maximum(q, 1) + r + 1).astype(np.uint64)


def _objects(vals):
    out = np.empty(len(vals), dtype=object)
    out[:] = vals.tolist() if isinstance(vals, np.ndarray) else list(vals)
    return out


def _nullable(vals, valid):
    """object array with None under NULLs"""
    out = _objects(vals)
    if valid is not None:
        out[~np.asarray(valid, bool)] = None
    return out


def shift_fast(b, vals, valid, offset, default=None):
    ps, pe = np.asarray(b[0], np.int64), np.asarray(b[1], np.int64)
    n = len(ps)
    src = np.arange(n, dtype=np.int64) + offset
    inside = (src >= ps) & (src < pe)
    v = _nullable(vals, valid)
    if default is None:
        d = np.full(n, None, dtype=object)
    elif default[0] == "scalar":
        d = np.empty(n, dtype=object)
        d[:] = [default[1]] * n
    else:
        d = _nullable(default[1], default[2])
    out = d.copy()
    out[inside] = v[src[inside]]
    return out.tolist()


def value_fast(kind, b, vals, valid, f, nth=1):
    lo, hi = frames_fast(f, b)
    j = lo if kind == FIRST_VALUE else hi - 1 if kind == LAST_VALUE else lo + nth - 1
    ok = (hi > lo) & (j >= lo) & (j < hi)
    v = _nullable(vals, valid)
    out = np.full(len(lo), None, dtype=object)
    out[ok] = v[j[ok]]
    return out.tolist()


def _sparse_extreme(key, lo, hi, want_max):
    """position of the extreme key in [lo, hi) for every row with hi > lo (sparse table over int64 keys; ties: any)"""
    n = len(key)
    pick = np.maximum if want_max else np.minimum
    levels = [key]
    w = 1
    while 2 * w <= n:
        prev = levels[-1]
        levels.append(pick(prev[:-w], prev[w:]))
        w *= 2
    ln = np.maximum(hi - lo, 1)
    lev = np.floor(np.log2(ln)).astype(np.int64)
    out = np.zeros(len(lo), np.int64)
    for k in range(len(levels)):
        m = (lev == k) & (hi > lo)
        if m.any():
            out[m] = pick(levels[k][lo[m]], levels[k][hi[m] - (1 << k)])
    return out


def _exact_prefix(x):
    """prefix sums of the finite doubles x as exact integers in units of 2^-1074"""
    out = [0] * (len(x) + 1)
    acc = 0
    for i, v in enumerate(x):
        if v != 0.0 and math.isfinite(v):
            num, den = v.as_integer_ratio()          # den is a power of two, at most 2^1074
            acc += num * ((1 << 1074) // den)
        out[i + 1] = acc
    return out


def aggregate_fast(agg, b, vals, valid, f, kind="i64"):
    lo, hi = frames_fast(f, b)
    n = len(lo)
    some = hi > lo
    if vals is None:
        return np.maximum(hi - lo, 0).tolist()
    ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
    cnt0 = np.concatenate([[0], np.cumsum(ok)])
    cnt = np.where(some, cnt0[hi] - cnt0[lo], 0)
    if agg == COUNT:
        return cnt.tolist()
    mode = sum_mode(kind)
    out = [None] * n
    if agg == SUM and mode != "float":
        pre = [0] * (n + 1)
        acc = 0
        vl = vals.tolist() if isinstance(vals, np.ndarray) else list(vals)
        for i in range(n):
            if ok[i]:
                acc += int(vl[i])
            pre[i + 1] = acc
        for i in np.nonzero(cnt > 0)[0].tolist():
            out[i] = wrap(pre[hi[i]] - pre[lo[i]], mode[1], mode[2])
        return out
    if agg == SUM:
        with np.errstate(invalid="ignore"):
            x = np.asarray(vals).astype(np.float64)
        x = np.where(ok, x, 0.0)            # a NULL contributes nothing, whatever lies under it
        nan0 = np.concatenate([[0], np.cumsum(np.isnan(x))])
        pin0 = np.concatenate([[0], np.cumsum(x == np.inf)])
        nin0 = np.concatenate([[0], np.cumsum(x == -np.inf)])
        xl = x.tolist()
        assert all(abs(v) <= F.MAX_SUM_ABS for v in xl if math.isfinite(v))
        pre, pre_abs = _exact_prefix(xl), _exact_prefix([abs(v) for v in xl])
        unit = Fraction(1, 1 << 1074)
        for i in np.nonzero(cnt > 0)[0].tolist():
            l, h = int(lo[i]), int(hi[i])
            nan, pinf, ninf = nan0[h] - nan0[l], pin0[h] - pin0[l], nin0[h] - nin0[l]
            cls = "nan" if nan or (pinf and ninf) else "+inf" if pinf else "-inf" if ninf else "finite"
            out[i] = (cls, float((pre[h] - pre[l]) * unit), float((pre_abs[h] - pre_abs[l]) * unit), int(cnt[i]))
        return out
    # MIN / MAX: the extreme of the values' dense ranks under the type's own order, then a value of that rank
    col = R.KeyCol(kind, vals)
    rank_of, nd = R._dense_rank(col)
    key = np.where(ok, rank_of, -1 if agg == MAX else nd + 1).astype(np.int64)
    best = _sparse_extreme(key, lo, hi, agg == MAX)
    rep = {}
    vl = col.py()
    for i in np.nonzero(ok)[0].tolist():
        rep.setdefault(int(rank_of[i]), vl[i])
    for i in np.nonzero(cnt > 0)[0].tolist():
        v = rep[int(best[i])]
        out[i] = float(v) if mode == "float" else v
    return out


# ---- comparing ------------------------------------------------------------------------------------------------------------------
def same_results(got, exp, kind="i64", agg=None):
    """'' or the first difference. got / exp: lists with None for NULL. Float MIN / MAX compare with float_ref.same_value, a float SUM
    (exp = the sum_expected tuple) with float_ref.sum_ok, everything else exactly."""
    if len(got) != len(exp):
        return f"{len(got)} rows for {len(exp)}"
    flt = kind in R.FLOAT_KINDS
    for i, (g, e) in enumerate(zip(got, exp)):
        if (g is None) != (e is None):
            return f"row {i}: {g!r} for {e!r}"
        if g is None:
            continue
        if flt and agg == SUM:
            good = F.sum_ok(g, e) if not isinstance(g, tuple) else g[0] == e[0] and g[3] == e[3] and g[1] == e[1]
        elif flt and agg in (MIN, MAX):
            good = F.same_value(g, e, R.FLOAT_KINDS[kind])
        elif flt:
            good = F.same_value(g, e, R.FLOAT_KINDS[kind], strict_zero=True)
        else:
            good = g == e
        if not good:
            return f"row {i}: {g!r} for {e!r}"
    return ""


# ---- the shared cases -----------------------------------------------------------------------------------------------------------
TILE = 1024                                   # rows per workgroup of the device scan: the shapes put heads on and around its multiples
SHAPES = ("one", "each", "tile_heads", "long", "mixed")
BOUNDS = [UNBOUNDED_PRECEDING, (PRECEDING, 0), (PRECEDING, 3), (PRECEDING, 400), CURRENT_ROW, (FOLLOWING, 2), (FOLLOWING, 400), UNBOUNDED_FOLLOWING]


def legal_frames():
    """all legal ROWS / RANGE frames over BOUNDS: 34 + 4"""
    out = []
    for units in (ROWS, RANGE):
        for s in BOUNDS:
            for e in BOUNDS:
                f = Frame(units, s, e)
                if frame_status(f) == OK:
                    out.append(f)
    return out


FRAMES = legal_frames()
HUGE = 2 ** 62
HUGE_FRAMES = [Frame(ROWS, (PRECEDING, HUGE), (FOLLOWING, HUGE)), Frame(ROWS, (PRECEDING, HUGE), (PRECEDING, 1)), Frame(ROWS, (FOLLOWING, 1), (FOLLOWING, HUGE)),
               Frame(ROWS, (FOLLOWING, HUGE), (FOLLOWING, HUGE)), Frame(ROWS, (PRECEDING, HUGE), (PRECEDING, HUGE)), Frame(ROWS, (PRECEDING, 2 ** 63 - 1), CURRENT_ROW)]
REFUSED_FRAMES = [(Frame(ROWS, (PRECEDING, -1), CURRENT_ROW), INVALID), (Frame(ROWS, CURRENT_ROW, (FOLLOWING, -5)), INVALID),
                  (Frame(ROWS, UNBOUNDED_FOLLOWING, UNBOUNDED_FOLLOWING), INVALID), (Frame(ROWS, UNBOUNDED_PRECEDING, UNBOUNDED_PRECEDING), INVALID),
                  (Frame(ROWS, CURRENT_ROW, (PRECEDING, 1)), INVALID), (Frame(ROWS, (FOLLOWING, 1), CURRENT_ROW), INVALID),
                  (Frame(ROWS, (PRECEDING, 1), (PRECEDING, 2)), INVALID), (Frame(ROWS, (FOLLOWING, 3), (FOLLOWING, 2)), INVALID),
                  (Frame(RANGE, UNBOUNDED_FOLLOWING, UNBOUNDED_FOLLOWING), INVALID), (Frame(RANGE, (PRECEDING, 1), CURRENT_ROW), UNSUPPORTED),
                  (Frame(RANGE, CURRENT_ROW, (FOLLOWING, 0)), UNSUPPORTED), (Frame(RANGE, (PRECEDING, 2), (FOLLOWING, 2)), UNSUPPORTED)]


def partition_sizes(rng, n, shape):
    if shape == "one":
        return [n]
    if shape == "each":
        return [1] * n
    if shape == "tile_heads":                 # every partition begins on a tile's first row; some span two and three tiles
        out, left, k = [], n, 0
        while left > 0:
            s = min(left, TILE * (1 + (k % 5 == 2) + 2 * (k % 7 == 3)))
            out.append(s)
            left -= s
            k += 1
        return out
    if shape == "long":                       # one partition over many tiles between small ones
        if n < 8:
            return [n]
        a, c = max(1, min(5, n // 4)), max(1, min(15, n // 4))
        return [a, n - a - c, c]
    out, left = [], n
    while left > 0:
        pick = rng.random()
        s = 1 if pick < 0.2 else int(rng.integers(2, 40)) if pick < 0.7 else int(rng.integers(40, 3 * TILE + 7))
        s = min(s, left)
        out.append(s)
        left -= s
    return out


def layout(seed, n, shape):
    """-> (partition key i64, order key i64) of n sorted rows: partitions of the shape's sizes, order keys ascending with ties"""
    rng = np.random.default_rng([seed, n, SHAPES.index(shape)])
    sizes = partition_sizes(rng, n, shape)
    assert sum(sizes) == n
    p = np.repeat(np.arange(len(sizes), dtype=np.int64) * 3 - 7, sizes)
    step = (rng.random(n) < 0.4).astype(np.int64)
    o = np.cumsum(step)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if n else np.zeros(0, np.int64)
    o = o - np.repeat(o[starts] if n else o, sizes)           # every partition begins at 0
    return R.KeyCol("i64", p), R.KeyCol("i64", o.astype(np.int64))


def sorted_keys(seed, n, keys):
    """seeded key columns (sort_ref.make_cols) put into their own sort order: what a window receives"""
    cols = R.make_cols(seed, n, keys)
    order = R.sort_perm_fast(cols, [0] * len(cols), [0] * len(cols))
    return [c.take(order) for c in cols]


def int_values(rng, n, kind="i64", nullable=True, small=False):
    dt = R.INT_KINDS[kind]
    vals = rng.integers(-50, 50, n).astype(dt) if small and np.iinfo(dt).min < 0 else rng.integers(0, 100, n).astype(dt) if small else R._ints(rng, n, dt, "pool")
    valid = None
    if nullable:
        valid = rng.random(n) < 0.7
        if small is False and n:
            vals = np.where(valid, vals, np.iinfo(dt).max).astype(dt)        # something loud under every NULL
    return vals, valid


def float_values(rng, n, dtype, for_sum, nullable=True):
    """float_ref.mixed with NaN / Inf / a huge value under the NULLs; SUM inputs stay inside float_ref's bound"""
    vals = F.mixed(rng, n, dtype, for_sum=for_sum)
    valid = None
    if nullable:
        valid = rng.random(n) < 0.7
        loud = np.array([np.nan, np.inf, -np.inf, 3e38 if np.dtype(dtype) == np.float32 else 1e308], dtype=dtype)
        vals = np.where(valid, vals, loud[rng.integers(0, 4, n)]).astype(dtype)
    if for_sum:
        with np.errstate(invalid="ignore"):
            live = vals.astype(np.float64)[valid if valid is not None else np.ones(n, bool)]
        assert np.all(np.abs(live[np.isfinite(live)]) <= F.MAX_SUM_ABS)
    return vals, valid


def poison_case():
    """one partition: a NaN and a 1e200 early, small terms after them. A prefix difference is NaN (without the NaN: 0.0) where the frame holds 1.5 + 2.5"""
    n = 40
    vals = np.array([1.0, np.nan, 1e200] + [1.5 + k for k in range(n - 3)], dtype=np.float64)
    p, o = R.KeyCol("i64", np.zeros(n, np.int64)), R.KeyCol("i64", np.arange(n, dtype=np.int64))
    return p, o, vals, Frame(ROWS, (PRECEDING, 1), CURRENT_ROW)
