"""The plain reference of the vector kernels (k_vector.hip): numpy float64, no GPU and no oracle.

distances()        the four metrics of dbhip_vec_distance as a [nq, n] float64 matrix
row_distances()    the same row by row (dbhip_vec_distance_rows), plus the norm
eps()              the project's f32 tolerance: 1e-5 * max(1, |d|, s) + 2e-7, s = sum |q_k b_k| for dot and 0 otherwise
check_topk()       what "an exact top-k" means when distances are only known to eps — states it from d_ref alone
check_topk_strict  the same for inputs whose arithmetic is exact in any order: the one possible list
band()             how many rows lie within eps of the k-th best: the rows check_topk cannot tell apart
merge_expected()   dbhip_vec_topk_merge: a plain sort by (distance with NaN -> +inf, id), fillers excluded

Order everywhere: ascending distance, NaN counts as +inf, equal distances by the lower row id; missing entries are (+inf, 0xFFFFFFFF).
tests/test_vec_ref_cpu.py checks this file against the C oracle and shows that the checkers reject wrong answers."""
import numpy as np

COSINE, L2, DOT, L1, NORM = 0, 1, 2, 3, 4
FILL = 0xFFFFFFFF


def distances(metric, base, queries):
    """float64 [nq, n]; cosine = 1 - q.b / (|q| |b|) (0/0 = NaN), l2 = sqrt(sum (q-b)^2) in the difference form, dot = sum q b,
    l1 = sum |q-b|"""
    b = np.asarray(base, dtype=np.float64)
    q = np.asarray(queries, dtype=np.float64)
    n, dim = b.shape
    nq = q.shape[0]
    with np.errstate(all="ignore"):
        if metric == DOT:
            return q @ b.T
        if metric == COSINE:
            return 1.0 - (q @ b.T) / np.outer(np.sqrt((q * q).sum(1)), np.sqrt((b * b).sum(1)))
        out = np.zeros((nq, n), dtype=np.float64)
        step = max(1, (1 << 23) // max(1, n * dim))
        for lo in range(0, nq, step):
            diff = q[lo:lo + step, None, :] - b[None, :, :]
            if metric == L2:
                out[lo:lo + step] = np.sqrt(np.einsum("ijk,ijk->ij", diff, diff))
            else:
                out[lo:lo + step] = np.abs(diff, out=diff).sum(-1)
        return out


def row_distances(metric, lhs, rhs):
    """float64 [n]: distance(lhs[i], rhs[i]) (a 1-d side stands for every row); metric NORM = |lhs[i]|"""
    a = np.atleast_2d(np.asarray(lhs, dtype=np.float64))
    with np.errstate(all="ignore"):
        if metric == NORM:
            return np.sqrt((a * a).sum(1))
        b = np.atleast_2d(np.asarray(rhs, dtype=np.float64))
        if metric == DOT:
            return (a * b).sum(1)
        if metric == COSINE:
            return 1.0 - (a * b).sum(1) / (np.sqrt((a * a).sum(1)) * np.sqrt((b * b).sum(1)))
        if metric == L2:
            return np.sqrt(((a - b) ** 2).sum(1))
        return np.abs(a - b).sum(1)


def dot_scale(base, queries):
    """s = sum_k |q_k b_k|, the natural scale of a dot product's rounding"""
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(queries, np.float64)) @ np.abs(np.asarray(base, np.float64)).T


def eps(metric, d_ref, base=None, queries=None):
    """1e-5 * max(1, |d|, s) + 2e-7 per element; 0 where that is not a number (a NaN / infinite reference distance): such a row
    is at +inf (or -inf) exactly, ties only with its equals, and may not stand before a finite row"""
    with np.errstate(all="ignore"):
        m = np.maximum(1.0, np.abs(np.asarray(d_ref, np.float64)))
        if metric == DOT:
            m = np.maximum(m, dot_scale(base, queries))
        e = 1e-5 * m + 2e-7
    return np.where(np.isfinite(e), e, 0.0)


def _clean(d_ref):
    d = np.asarray(d_ref, dtype=np.float64)
    return np.where(np.isnan(d), np.inf, d)


def kth(d_ref, k):
    """t = the min(k, n)-th smallest reference distance (NaN as +inf)"""
    d = _clean(d_ref)
    kk = min(k, d.shape[0])
    return np.partition(d, kk - 1)[kk - 1]


def band(d_ref, e, k):
    """per query: rows with |d_ref - t| <= eps (equal infinities tie; an infinite row is in the band of an infinite t only)"""
    D, E = np.atleast_2d(d_ref), np.atleast_2d(e)
    out = np.zeros(D.shape[0], dtype=np.int64)
    for q in range(D.shape[0]):
        d = _clean(D[q])
        t = kth(d, k)
        with np.errstate(all="ignore"):
            diff = np.abs(d - t)
            out[q] = int(((np.isfinite(diff) & (diff <= E[q])) | (d == t)).sum())
    return out


def check_topk(d_ref, e, idx, dist, k, n):
    """one query: d_ref, e [n]; idx, dist [k] as returned. Raises AssertionError naming the broken statement."""
    d_raw = np.asarray(d_ref, dtype=np.float64)
    d = _clean(d_raw)
    e = np.asarray(e, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    dist = np.asarray(dist, dtype=np.float64)
    assert idx.shape == (k,) and dist.shape == (k,) and d.shape == (n,)
    kk = min(k, n)
    assert (idx[kk:] == FILL).all(), ("filler ids", idx[kk:])
    assert np.isposinf(dist[kk:]).all(), ("filler distances", dist[kk:])
    if kk == 0:
        return
    got = idx[:kk]
    assert (got < n).all() and (got >= 0).all(), ("row id out of range", got)
    assert len(set(got.tolist())) == kk, ("duplicate row id", got)
    t = kth(d, k)
    dg, eg = d[got], e[got]
    # (a <= b + e is written (a <= b) | (a - b <= e): equal infinities compare, and inf - inf = NaN decides nothing)
    with np.errstate(all="ignore"):
        late = got[~((dg <= t) | (dg - t <= eg))]
        assert late.size == 0, ("returned rows beyond the k-th best", late, d[late], t)
        must = np.flatnonzero((d < t) & (t - d > e))
        lost = np.setdiff1d(must, got)
        assert lost.size == 0, ("rows before the k-th best are missing", lost, d[lost], t)
        asc = (dg[:, None] <= dg[None, :]) | (dg[:, None] - dg[None, :] <= np.maximum(eg[:, None], eg[None, :]))
        bad = np.argwhere(np.triu(~asc, 1))
        assert bad.size == 0, ("not ascending", bad[0].tolist(), dg[bad[0]])
        r = d_raw[got]
        fin = np.isfinite(r) & (np.abs(r) < 1e30)
        off = fin & ~(np.abs(dist[:kk] - r) <= eg)
        assert not off.any(), ("distance", np.flatnonzero(off), got[off], dist[:kk][off], r[off], eg[off])
        wild = ~np.isfinite(r) & np.isfinite(dist[:kk])
        assert not wild.any(), ("distance of a NaN / infinite row", np.flatnonzero(wild), got[wild], dist[:kk][wild], r[wild])


def strict_order(d_ref, k):
    d = _clean(d_ref)
    return np.lexsort((np.arange(d.shape[0]), d))[:min(k, d.shape[0])]


def check_topk_strict(d_ref, idx, k, n):
    """one query whose distances are exact in any arithmetic: idx[:kk] is lexsort((row id, d_ref))[:kk], fillers behind"""
    idx = np.asarray(idx).astype(np.int64)
    assert idx.shape == (k,)
    kk = min(k, n)
    exp = strict_order(d_ref, k)
    assert np.array_equal(idx[:kk], exp), ("strict order", idx[:kk], exp)
    assert (idx[kk:] == FILL).all(), ("filler ids", idx[kk:])


def check_all(D, E, idx, dist, k, strict=False, tag=None):
    """every query of a batch; the failing query is named"""
    nq, n = D.shape
    assert idx.shape == (nq, k) and dist.shape == (nq, k), (idx.shape, dist.shape)
    for q in range(nq):
        try:
            if strict:
                check_topk_strict(D[q], idx[q], k, n)
                kk = min(k, n)
                assert np.isposinf(np.asarray(dist[q, kk:], np.float64)).all(), ("filler distances", dist[q, kk:])
            else:
                check_topk(D[q], E[q], idx[q], dist[q], k, n)
        except AssertionError as err:
            raise AssertionError((tag, "query", q) + tuple(err.args)) from None


def merge_expected(dists, ids, k):
    """dbhip_vec_topk_merge of one row of candidates: (ids [k], dists [k]) by a plain sort"""
    real = np.asarray(ids) != FILL
    d, i = _clean(np.asarray(dists)[real]), np.asarray(ids)[real].astype(np.int64)
    order = np.lexsort((i, d))[:k]
    pad = k - order.shape[0]
    return (np.concatenate([i[order], np.full(pad, FILL, np.int64)]).astype(np.uint32),
            np.concatenate([d[order], np.full(pad, np.inf)]).astype(np.float32))
