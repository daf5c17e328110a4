"""CPU: the reference and the case tables of the vector edge suite can carry the weight put on them. tests/vec_ref.py agrees with the
C oracle on the metric definitions; every leg that check_topk judges has at most BAND_CAP rows within eps of its k-th best (or is
named in vec_cases.WEAK with the statement it is judged by); the checkers reject each kind of wrong answer; the grid class is exact
in f32 in any summation order; the collapsed block has one bf16 image; the tables sit on both sides of every dispatch rule."""
import ctypes as C

import numpy as np
import pytest

from tests import vec_cases as V
from tests import vec_ref as R


def orc(oracle, metric, base, q):
    out = np.zeros((q.shape[0], base.shape[0]), np.float32)
    oracle.orc_vec_distance(metric, base.ctypes.data_as(C.c_void_p), C.c_int64(base.shape[0]), base.shape[1], q.ctypes.data_as(C.c_void_p), q.shape[0],
                            out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("cls", ["normal", "grid", "collapsed", "offset"])
def test_reference_agrees_with_oracle(oracle, cls):
    """pins the metric definitions and the sign of dot (ascending: the most negative inner product is the nearest)"""
    base, q = {"normal": lambda: V.normal(50, 33, 7, 1), "grid": lambda: V.grid(60, 36, 5, 2), "collapsed": lambda: V.collapsed(64, 4, 3),
               "offset": lambda: V.offset(100, 17, 5, 4)}[cls]()
    for metric in V.ALL4:
        D = R.distances(metric, base, q)
        E = R.eps(metric, D, base, q)
        got = orc(oracle, metric, base, q).astype(np.float64)
        assert np.array_equal(np.isnan(D), np.isnan(got)), metric
        ok = np.isnan(D) | (np.abs(got - D) <= E)
        assert ok.all(), (metric, np.abs(got - D)[~ok].max())
        if cls == "grid":
            assert np.isnan(D).any() == (metric == V.COSINE)
    assert R.distances(V.DOT, np.array([[1.0, 2.0]]), np.array([[3.0, -5.0]]))[0, 0] == -7.0
    assert R.distances(V.L1, np.array([[1.0, 2.0]]), np.array([[3.0, -5.0]]))[0, 0] == 9.0
    # row by row = the diagonal
    for metric in V.ALL4:
        b2, q2 = base[:4], q[:4]
        assert np.allclose(R.row_distances(metric, q2, b2), np.diag(R.distances(metric, b2, q2)), rtol=1e-14, atol=0, equal_nan=True)
    assert np.allclose(R.row_distances(V.NORM, base[:5], None), np.linalg.norm(base[:5].astype(np.float64), axis=1), rtol=1e-15)


JUDGED = [(kind, name) for kind, table in (("topk", V.TOPK_CASES), ("index", V.INDEX_CASES)) for name, c in table.items() if c.n > 0 and c.nq > 0]


@pytest.mark.parametrize("kind,name", JUDGED)
def test_band_cap(oracle, kind, name):
    """at most BAND_CAP rows within eps of the k-th best in every leg check_topk judges, the named weak legs / queries aside"""
    c = (V.TOPK_CASES if kind == "topk" else V.INDEX_CASES)[name]
    base, q = V.make(c)
    assert base.shape == (c.n, c.dim) and q.shape == (c.nq, c.dim) and base.dtype == np.float32
    for metric in c.metrics:
        weak = V.weak_queries(c, metric)
        if V.strict(c, metric) or weak == "all":
            continue
        D, E = V.reference(c, metric, base, q, oracle)
        b = R.band(D, E, c.k)
        if weak:
            b[list(weak)] = 0
        assert b.max() <= V.BAND_CAP, (V.METRIC_NAMES[metric], int(b.argmax()), int(b.max()))


def test_weak_list_is_only_what_it_may_be():
    for w in V.WEAK:
        assert w["cls"] in ("collapsed", "special", "dupes", "dupes_normal") and w["reason"] and w["judged_by"]
        assert not (w["cls"] == "collapsed" and w["metric"] in (None, V.L2))
    c = V.INDEX_CASES["collapsed_n11192_dim64_nq20_k10_f128"]
    assert V.weak_queries(c, V.L2) is None and V.weak_queries(c, V.COSINE) == "all"
    for table in (V.TOPK_CASES, V.INDEX_CASES):
        for c in table.values():
            if c.cls in ("normal", "grid", "offset", "placed"):
                assert all(V.weak_queries(c, m) is None for m in c.metrics), c.name


def test_collapsed_block_has_one_bf16_image_and_holds_every_neighbour():
    lo, hi = V.COLLAPSED_BLOCK
    for dim in (64, 128):
        base, q = V.collapsed(dim, 20, 5)
        img = V.bf16_image(base[lo:hi])
        assert len(np.unique(img, axis=0)) == 1
        assert len(np.unique(base[lo:hi], axis=0)) == hi - lo
        assert len(np.unique(V.bf16_image(q[:10]), axis=0)) == 1 and np.array_equal(V.bf16_image(q[10:])[0], -img[0])
        D = R.distances(V.L2, base, q[:10])
        assert ((np.argsort(D, axis=1)[:, :hi - lo] >= lo) & (np.argsort(D, axis=1)[:, :hi - lo] < hi)).all()
        Dd = R.distances(V.DOT, base, q[10:])
        assert ((np.argsort(Dd, axis=1)[:, :hi - lo] >= lo) & (np.argsort(Dd, axis=1)[:, :hi - lo] < hi)).all()
        # aligned: one image again, part of it before S0, and for every query true neighbours behind S0 that the filter must let through
        abase, aq = V.collapsed(dim, 20, 5, aligned=True)
        (slo, shi), (alo, ahi) = V.COLLAPSED_ALIGNED_ROWS
        assert shi <= V.S0 < alo
        assert len(np.unique(V.bf16_image(np.concatenate([abase[slo:shi], abase[alo:ahi]])), axis=0)) == 1
        best = np.argsort(R.distances(V.L2, abase, aq[:10]), axis=1)[:, :10]
        assert (best >= alo).any(axis=1).all() and ((best >= slo) & (best < ahi)).all()
        # ... and the low parts meet Cauchy-Schwarz almost with equality: |c . delta| > 0.9 |c| |delta| for most rows
        cimg = V.bf16_image(abase[alo:ahi]).astype(np.float64)
        delta = abase[alo:ahi].astype(np.float64) - cimg
        cs = np.abs((cimg * delta).sum(1)) / (np.linalg.norm(cimg, axis=1) * np.linalg.norm(delta, axis=1))
        assert np.median(cs) > 0.9


def test_far_tail_leaves_the_filter_nothing_to_keep():
    """every row behind S0 is worse than the k-th best of the rows before it by a margin no error bound reaches (the filter's
    slack is ~1e-3 of |q| |b|): the case takes the maxc == 0 return by construction, and its answer lies wholly before S0"""
    for c in V.INDEX_CASES.values():
        if c.cls != "far_tail":
            continue
        base, q = V.make(c)
        for metric in c.metrics:
            D = R.distances(metric, base, q)
            t = np.sort(D[:, :V.S0], axis=1)[:, c.k - 1]
            scale = np.linalg.norm(q.astype(np.float64), axis=1) * np.linalg.norm(base[V.S0:].astype(np.float64), axis=1).max()
            margin = {V.COSINE: 0.5, V.L2: 0.5 * np.sqrt(c.dim), V.DOT: 0.05 * scale}[metric]
            assert (D[:, V.S0:].min(axis=1) > t + margin).all(), (c.name, metric)


def test_grid_is_exact_in_f32_in_any_order():
    base, q = V.grid(200, 128, 6, 9)
    prod = q[:, None, :] * base[None, :, :]
    diff = q[:, None, :] - base[None, :, :]
    for terms in (prod, diff * diff, np.abs(diff)):
        assert terms.dtype == np.float32
        fwd = np.zeros(terms.shape[:2], np.float32)
        rev = np.zeros(terms.shape[:2], np.float32)
        for k in range(terms.shape[2]):
            fwd = fwd + terms[:, :, k]
            rev = rev + terms[:, :, terms.shape[2] - 1 - k]
        pair = terms.sum(-1, dtype=np.float32)                        # numpy's pairwise order
        exact = terms.astype(np.float64).sum(-1)
        assert fwd.dtype == np.float32 and fwd.tobytes() == rev.tobytes() == pair.tobytes()
        assert np.array_equal(fwd.astype(np.float64), exact)
    assert np.array_equal(V.bf16_image(base), base) and np.array_equal(V.bf16_image(q), q)


def _answer(D, k):
    idx = np.stack([np.concatenate([R.strict_order(D[qi], k), np.full(k - min(k, D.shape[1]), R.FILL)]) for qi in range(D.shape[0])]).astype(np.uint32)
    dist = np.full(idx.shape, np.inf, np.float32)
    for qi in range(D.shape[0]):
        kk = min(k, D.shape[1])
        dist[qi, :kk] = np.nan_to_num(D[qi, idx[qi, :kk].astype(np.int64)], nan=np.inf)
    return idx, dist


def _rejects(fn, *args):
    try:
        fn(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("metric", [V.COSINE, V.L2, V.DOT, V.L1])
def test_checkers_reject_wrong_answers(metric):
    n, k = 500, 10
    base, q = V.normal(n, 16, 4, 11)
    D = R.distances(metric, base, q)
    E = R.eps(metric, D, base, q)
    idx, dist = _answer(D, k)
    R.check_all(D, E, idx, dist, k)
    R.check_all(D, E, idx, dist, k, strict=True)
    for qi in range(4):
        d, e, order = D[qi], E[qi], R.strict_order(D[qi], n)

        def mutated(f):
            i2, d2 = idx[qi].copy(), dist[qi].copy()
            f(i2, d2)
            return i2, d2

        def kth_replaced(i2, d2):
            assert d[order[k + 4]] > d[order[k - 1]] + e[order[k + 4]]
            i2[k - 1], d2[k - 1] = order[k + 4], d[order[k + 4]]

        gaps = [j for j in range(k - 1) if d[order[j + 1]] - d[order[j]] > 2 * max(e[order[j]], e[order[j + 1]])]
        assert gaps

        def swapped(i2, d2):
            j = gaps[0]
            i2[[j, j + 1]] = i2[[j + 1, j]]
            d2[[j, j + 1]] = d2[[j + 1, j]]

        def duplicated(i2, d2):
            i2[3], d2[3] = i2[2], d2[2]

        def distance_off(i2, d2):
            d2[5] = np.float32(d[order[5]] + 3 * e[order[5]])

        def filler_inside(i2, d2):
            i2[4], d2[4] = R.FILL, np.inf

        for f in (kth_replaced, swapped, duplicated, distance_off, filler_inside):
            i2, d2 = mutated(f)
            assert _rejects(R.check_topk, d, e, i2, d2, k, n), f.__name__
            if f is not distance_off:
                assert _rejects(R.check_topk_strict, d, i2, k, n), f.__name__
    # k above n: the tail must be fillers
    D5, E5 = D[:, :5], E[:, :5]
    idx5, dist5 = _answer(D5, k)
    R.check_all(D5, E5, idx5, dist5, k)
    bad = idx5.copy()
    bad[0, 7] = 2
    assert _rejects(R.check_all, D5, E5, bad, dist5, k) and _rejects(R.check_all, D5, E5, bad, dist5, k, True)
    badd = dist5.copy()
    badd[0, 9] = 1.0
    assert _rejects(R.check_all, D5, E5, idx5, badd, k) and _rejects(R.check_all, D5, E5, idx5, badd, k, True)


@pytest.mark.parametrize("metric", [V.COSINE, V.L2, V.DOT, V.L1])
def test_checker_rejects_a_nan_or_inf_row_ranked_before_finite_rows(metric):
    """NaN counts as +inf: a row whose reference distance is NaN or infinite has no tolerance to hide in (eps = 0), so it may
    neither replace the k-th best nor stand at rank 0 with distance +inf — the answer a selection that mishandles NaN would give"""
    n, k = 500, 10
    base, q = V.normal(n, 16, 2, 3)
    base[100, 3] = np.nan
    base[200, 5] = np.inf
    D = R.distances(metric, base, q)
    E = R.eps(metric, D, base, q)
    assert not np.isfinite(D[:, [100, 200]]).any() and (E[:, [100, 200]] == 0).all() and (R.band(D, E, k) <= 2).all()
    idx, dist = _answer(D, k)
    R.check_all(D, E, idx, dist, k)
    for qi in range(2):
        for row in (100, 200):
            i2, d2 = idx[qi].copy(), dist[qi].copy()
            i2[1:], d2[1:] = idx[qi][:-1], dist[qi][:-1]             # the k-th best is dropped ...
            i2[0], d2[0] = row, np.inf                               # ... for the NaN / Inf row at rank 0
            assert _rejects(R.check_topk, D[qi], E[qi], i2, d2, k, n), (qi, row)
            assert _rejects(R.check_topk_strict, D[qi], i2, k, n)
            i3, d3 = idx[qi].copy(), dist[qi].copy()
            i3[k - 1], d3[k - 1] = row, np.inf                       # in the k-th place: still before finite rows that are left out
            assert _rejects(R.check_topk, D[qi], E[qi], i3, d3, k, n), (qi, row)
    # where fewer than k rows are finite the NaN / Inf rows belong in the answer, behind the finite ones, tied among themselves
    if metric == V.DOT:          # (the Inf row's inner product is -inf or +inf by the sign of q_5: no tie with the NaN row)
        return
    few = np.array([100, 200, 7, 8, 9])
    Df, Ef = D[:, few], E[:, few]
    idxf, distf = _answer(Df, 4)
    assert (idxf[:, 3] == 0).all() and np.isposinf(distf[:, 3]).all()
    R.check_all(Df, Ef, idxf, distf, 4)
    other = idxf.copy()
    other[:, 3] = 1
    R.check_all(Df, Ef, other, distf, 4)                             # equal infinities tie
    assert _rejects(R.check_all, Df, Ef, other, distf, 4, True)      # ... strictly, by the lower id
    assert _rejects(R.check_all, Df, Ef, idxf[:, [3, 0, 1, 2]], distf[:, [3, 0, 1, 2]], 4)


def test_strict_checker_rejects_a_tie_resolved_to_the_higher_id():
    base, q = V.grid(400, 8, 4, 12)
    k = 16
    for metric in V.STRICT_GRID:
        D = R.distances(metric, base, q)
        E = R.eps(metric, D, base, q)
        idx, dist = _answer(D, k)
        R.check_all(D, E, idx, dist, k, strict=True)
        R.check_all(D, E, idx, dist, k)
        done = 0
        for qi in range(4):
            got = idx[qi].astype(np.int64)
            ties = [j for j in range(k - 1) if D[qi, got[j]] == D[qi, got[j + 1]]]
            if not ties:
                continue
            i2 = idx[qi].copy()
            j = ties[0]
            i2[[j, j + 1]] = i2[[j + 1, j]]
            assert _rejects(R.check_topk_strict, D[qi], i2, k, 400)
            R.check_topk(D[qi], E[qi], i2, dist[qi], k, 400)          # the tolerant checker cannot see it: why grid is judged strictly
            # a tie across the k-th place resolved to a higher id
            t = D[qi, got[k - 1]]
            later = [r for r in np.flatnonzero(D[qi] == t) if r > got[k - 1]]
            if later:
                i3 = idx[qi].copy()
                i3[k - 1] = later[0]
                assert _rejects(R.check_topk_strict, D[qi], i3, k, 400)
            done += 1
        assert done >= 2
    # NaN counts as +inf and ties with it
    d = np.array([np.nan, 1.0, np.inf, 0.5])
    R.check_topk_strict(d, np.array([3, 1, 0, 2, R.FILL]), 5, 4)
    R.check_topk(d, R.eps(V.L2, d), np.array([3, 1, 2, 0, R.FILL]), np.array([0.5, 1.0, np.inf, np.nan, np.inf]), 5, 4)
    assert _rejects(R.check_topk, d, R.eps(V.L2, d), np.array([3, 1, 2, 0, R.FILL]), np.array([0.5, 1.0, np.inf, 7.0, np.inf]), 5, 4)
    assert R.band(d, R.eps(V.L2, d), 3)[0] == 2


def test_merge_reference_and_lists():
    d = np.array([2.0, np.nan, 1.0, 1.0, np.inf, np.inf, 0.5], np.float32)
    i = np.array([9, 4, 0xFFFFFFFE, 7, R.FILL, 3, 8], np.uint32)
    ei, ed = R.merge_expected(d, i, 6)
    assert ei.tolist() == [8, 7, 0xFFFFFFFE, 9, 3, 4] and ed.tolist() == [0.5, 1.0, 1.0, 2.0, np.inf, np.inf]
    ei, ed = R.merge_expected(d, i, 8)
    assert ei.tolist()[6:] == [R.FILL, R.FILL] and np.isposinf(ed[6:]).all()
    for name, (m, nq, k) in V.MERGE_CASES.items():
        if m > 200_000:
            continue
        dd, ii = V.merge_lists(m, nq, k)
        for r in range(nq):
            real = ii[r][ii[r] != R.FILL]
            assert len(set(real.tolist())) == len(real), name                     # the expected order is total
            assert np.isposinf(dd[r][ii[r] == R.FILL]).all()
        if m >= 8192:
            assert np.isnan(dd).any() and (ii == R.FILL).any() and (ii > 0xF0000000).any()
    assert {V.merge_stages(m, k) for m, _, k in V.MERGE_CASES.values()} == {1, 2, 3}


def test_tables_sit_on_both_sides_of_every_dispatch_rule():
    dist = list(V.DISTANCE_CASES.values())
    assert {V.dot_tile(c.nq, c.dim, c.aligned) for c in dist} == {"t32x256", "t64x256", "t128x128", "scalar128x128"}
    assert any(not c.aligned and c.dim % 4 == 0 for c in dist)
    for axis, want in (("n", V.DISTANCE_N), ("nq", V.DISTANCE_NQ), ("dim", V.DISTANCE_DIM)):
        assert set(want) <= {getattr(c, axis) for c in dist}
    topk = list(V.TOPK_CASES.values())
    assert {1, 2, 15, 16} <= {c.k for c in topk} and {1, 33, 65, 2048, 2049} <= {c.nq for c in topk}
    assert {0, 1, 8191, 8192, 8193, 16_385, 65_536, 65_537, 65_836, V.EXACT_MAX + V.CAND_CAP, V.EXACT_MAX + V.CAND_CAP + 1} <= {c.n for c in topk}
    index = list(V.INDEX_CASES.values())
    assert {V.S0 + r for r in (0, 1, 127, 128, 129, 255, 256, 257)} | {0, 5, 8191, 65_836} <= {c.n for c in index}
    assert {1, 127, 128, 129, 255, 256, 257, 2049} <= {c.nq for c in index}
    assert {1, 3, 63, 64, 65, 96, 128, 129, 192, 256} <= {c.dim for c in index} and {1, 16} <= {c.k for c in index}
    for cls in ("normal", "grid", "dupes", "collapsed", "offset", "special"):
        paths = {V.index_path(c.n, c.dim, c.nq) for c in index if c.cls == cls}
        assert {"f256x8phase", "f128"} <= paths, (cls, paths)
    assert {"ftall", "exact_only"} <= {V.index_path(c.n, c.dim, c.nq) for c in index}
    assert any(V.index_path(c.n, c.dim, c.nq).startswith("two_levels") for c in index)
    assert V.filter_kernel(255, 96, 129) == "ftall" and V.filter_kernel(256, 96, 129) == "f256x8phase" and V.filter_kernel(300, 192, 130) == "ftall"
    assert {V.rows_group(d) for d, _ in V.ROWS_CASES.values()} == {1, 2, 4, 8, 16, 32, 64}
    assert [V.rows_group(d) for d in (4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)] == [1, 2, 2, 4, 4, 8, 8, 16, 16, 32, 32, 64]
    u8 = list(V.SCORE_U8_CASES.values())
    assert {1, 15, 16, 17, 100, 16_384, 16_400} <= {d for d, _, _ in u8} and {0, 1, 3, 4, 5, 257} <= {n for _, n, _ in u8}
    assert any(off == 1 and d % 16 == 0 for d, _, off in u8)
