"""GPU: vector distance, top-k and the bf16 index (k_vector.hip) at the edges of their kernels — tile borders of dot_tile_kernel and
diff_valu_kernel on all three axes, the scalar-staging shape, one / two / three stages of the selection with its carry slot, the exact /
sample + filter threshold of dbhip_vec_topk, the candidate list exactly full and one over, every filter kernel of the index with ragged
tiles on both sides, zero-padded dims, two filter levels, query batches, and data the filter's error bound has no margin on.
Every result is judged against tests/vec_ref.py (numpy float64, never another device path) on the case tables of tests/vec_cases.py:
check_topk states an exact top-k from the reference alone, check_topk_strict demands the one possible list where the arithmetic is exact.
tests/test_vec_ref_cpu.py checks that reference and shows that the checkers reject wrong answers."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import vec_cases as V
from tests import vec_ref as R

pytestmark = pytest.mark.gpu


def shifted(gpu, arr, off):
    """a device copy of `arr` that starts `off` bytes into its allocation -> (buffer to keep alive, pointer)"""
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = gpu.DeviceBuffer.from_numpy(np.concatenate([np.zeros(off, np.uint8), raw, np.zeros(32, np.uint8)]))
    return buf, buf.ptr + off


def exact_f32(c, metric):
    return c.cls in ("grid", "placed") and metric in V.STRICT_GRID


def judge(c, metric, D, E, idx, dist, tag):
    if V.strict(c, metric):
        R.check_all(D, E, idx, dist, c.k, strict=True, tag=tag)
    R.check_all(D, E, idx, dist, c.k, tag=tag)
    if exact_f32(c, metric) and c.n:            # exact arithmetic: the distances are the reference's, bit for bit
        kk = min(c.k, c.n)
        want = np.take_along_axis(D, idx[:, :kk].astype(np.int64), axis=1).astype(np.float32)
        assert np.array_equal(dist[:, :kk], want), tag


# ---- dbhip_vec_distance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.DISTANCE_CASES))
def test_vec_distance_edges(gpu, name):
    c = V.DISTANCE_CASES[name]
    base, q = V.make(c)
    if c.aligned:
        gb, gq = gpu.VectorColumn(base), gpu.VectorColumn(q)
    else:
        keep_b, pb = shifted(gpu, base, 4)
        keep_q, pq = shifted(gpu, q, 4)
        assert pb % 16 == 4 and pq % 16 == 4
    for metric in c.metrics:
        if c.aligned:
            got = gpu.vec_distance(metric, gb, gq)
        else:
            out = gpu.DeviceBuffer(c.n * c.nq * 4)
            T.check(T.lib().dbhip_vec_distance(metric, C.c_void_p(pb), C.c_int64(c.n), c.dim, C.c_void_p(pq), c.nq, C.c_void_p(out.ptr), None))
            got = out.to_numpy(np.float32, c.n * c.nq).reshape(c.nq, c.n)
        D = R.distances(metric, base, q)
        E = R.eps(metric, D, base, q)
        tag = (name, V.METRIC_NAMES[metric])
        assert np.array_equal(np.isnan(got), np.isnan(D)), tag
        ok = np.isnan(D) | (np.abs(got.astype(np.float64) - D) <= E)
        assert ok.all(), tag + (np.argwhere(~ok)[:4].tolist(), float(np.abs(got - D)[~ok].max()))
        if exact_f32(c, metric):
            assert np.array_equal(got, D.astype(np.float32)), tag
        if c.cls == "grid" and metric == V.COSINE:
            assert np.isnan(D).any()


# ---- dbhip_vec_topk -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.TOPK_CASES))
def test_vec_topk_edges(gpu, oracle, name):
    c = V.TOPK_CASES[name]
    base, q = V.make(c)
    gb, gq = gpu.VectorColumn(base), gpu.VectorColumn(q)
    for metric in c.metrics:
        idx, dist = gpu.vec_topk(metric, gb, gq, c.k)
        assert idx.shape == (c.nq, c.k) and dist.shape == (c.nq, c.k)
        if c.nq == 0:
            continue
        D, E = V.reference(c, metric, base, q, oracle)
        judge(c, metric, D, E, idx, dist, (name, V.METRIC_NAMES[metric], V.topk_path(c.n, metric)))
        if c.cls == "dupes":
            assert np.array_equal(idx, np.tile(np.arange(c.k, dtype=np.uint32), (c.nq, 1)))


def test_vec_topk_k_out_of_range_raises(gpu):
    base, q = V.normal(40, 8, 2, 1)
    gb, gq = gpu.VectorColumn(base), gpu.VectorColumn(q)
    for k, msg in ((0, "bad shape"), (V.KMAX + 1, "k=17 > 16")):
        with pytest.raises(T.DbhipError, match=msg):
            gpu.vec_topk(V.L2, gb, gq, k)
        with pytest.raises(T.DbhipError, match=msg):
            gpu.vec_topk_merge(np.zeros((2, 40), np.float32), np.tile(np.arange(40, dtype=np.uint32), (2, 1)), k)
        ix = gpu.VectorIndex(V.L2, gb)
        try:
            with pytest.raises(T.DbhipError, match="bad argument" if k == 0 else msg):
                ix.search(gq, k)
        finally:
            ix.destroy()
    idx, dist = gpu.vec_topk(V.L2, gb, gq, V.KMAX)
    D = R.distances(V.L2, base, q)
    R.check_all(D, R.eps(V.L2, D), idx, dist, V.KMAX)


# ---- dbhip_vec_index_* --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.INDEX_CASES))
def test_vec_index_edges(gpu, oracle, name):
    """the index returns an exact top-k by the reference's own statement, and so does the scan; where the two differ, the rows that
    differ lie inside the reference's band (or the query is named weak)"""
    c = V.INDEX_CASES[name]
    base, q = V.make(c)
    gb, gq = gpu.VectorColumn(base), gpu.VectorColumn(q)
    for metric in c.metrics:
        tag = (name, V.METRIC_NAMES[metric])
        ix = gpu.VectorIndex(metric, gb)
        try:
            idx, dist = ix.search(gq, c.k)
        finally:
            ix.destroy()
        eidx, edist = gpu.vec_topk(metric, gb, gq, c.k)
        D, E = V.reference(c, metric, base, q, oracle)
        judge(c, metric, D, E, idx, dist, tag + ("index",))
        judge(c, metric, D, E, eidx, edist, tag + ("scan",))
        if c.n == 0:
            continue
        if V.strict(c, metric):
            assert np.array_equal(idx, eidx), tag
            continue
        weak = V.weak_queries(c, metric)
        if weak == "all":
            continue
        for qi in range(c.nq):
            if (weak and qi in weak) or np.array_equal(idx[qi], eidx[qi]):
                continue
            t = R.kth(D[qi], c.k)
            moved = np.concatenate([idx[qi][idx[qi] != eidx[qi]], eidx[qi][idx[qi] != eidx[qi]]]).astype(np.int64)
            d = np.where(np.isnan(D[qi, moved]), np.inf, D[qi, moved])
            with np.errstate(all="ignore"):
                inside = (np.abs(d - t) <= E[qi, moved]) | (d == t)
            assert inside.all(), tag + ("index and scan differ outside the band", qi, moved[~inside].tolist())


def test_vec_index_has_no_l1(gpu):
    base, _ = V.normal(40, 8, 2, 1)
    with pytest.raises(T.DbhipError, match="no bf16 pre-filter"):
        gpu.VectorIndex(V.L1, gpu.VectorColumn(base))


# ---- dbhip_vec_topk_merge -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.MERGE_CASES))
def test_vec_topk_merge_edges(gpu, name):
    m, nq, k = V.MERGE_CASES[name]
    d, ids = V.merge_lists(m, nq, k)
    gi, gd = gpu.vec_topk_merge(d, ids, k)
    for r in range(nq):
        ei, ed = R.merge_expected(d[r], ids[r], k)
        assert np.array_equal(gi[r], ei), (name, r, gi[r], ei)
        assert np.array_equal(gd[r], ed), (name, r, gd[r], ed)


# ---- dbhip_score_u8 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(V.SCORE_U8_CASES))
def test_score_u8_edges(gpu, oracle, name):
    dim, n, off = V.SCORE_U8_CASES[name]
    q, base = V.score_u8_data(dim, n)
    if off:
        keep_b, pb = shifted(gpu, base, off)
        keep_q = gpu.DeviceBuffer.from_numpy(q)
    for is_l1 in (0, 1):
        exp = np.zeros(n, np.float32)
        if n:
            oracle.orc_score_u8(is_l1, q.ctypes.data_as(C.c_void_p), base.ctypes.data_as(C.c_void_p), C.c_int64(n), dim, exp.ctypes.data_as(C.c_void_p))
        if off:
            out = gpu.DeviceBuffer(n * 4)
            T.check(T.lib().dbhip_score_u8(is_l1, C.c_void_p(keep_q.ptr), C.c_void_p(pb), C.c_int64(n), dim, C.c_void_p(out.ptr), None))
            got = out.to_numpy(np.float32, n)
        else:
            got = gpu.score_u8(is_l1, q, base)
        assert got.shape == (n,) and np.array_equal(got, exp), (name, is_l1)
        if dim == 16_384 and not is_l1:
            assert exp[-1] == np.float32(127 * 127 * 16_384)       # the all-127 row against the all-127 query


# ---- dbhip_vec_distance_rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", ["f32", "f64", "i8"])
@pytest.mark.parametrize("name", list(V.ROWS_CASES))
def test_vec_distance_rows_edges(gpu, name, elem):
    dim, n = V.ROWS_CASES[name]
    a, b = V.rows_data(dim, n, elem)
    et = {"f32": T.T_F32, "f64": T.T_F64, "i8": T.T_I8}[elem]
    assert n == 1 or not np.array_equal(a[-1], a[0])
    for metric in (V.COSINE, V.L2, V.DOT, V.L1, V.NORM):
        sides = [(a, b, False, False)] if metric == V.NORM else [(a, b, False, False), (a[0], b, True, False), (a, b[0], False, True)]
        for lhs, rhs, ls, rs in sides:
            got = gpu.vec_distance_rows(metric, lhs, None if metric == V.NORM else rhs, n, dim, elem=et, lhs_scalar=ls, rhs_scalar=rs)
            ref = R.row_distances(metric, lhs, rhs)
            ref = np.broadcast_to(ref, (n,))
            assert got.shape == (n,) and got.dtype == (np.float64 if elem == "f64" else np.float32)
            scale = np.maximum(1.0, np.abs(ref))
            if metric == V.DOT:
                scale = np.maximum(scale, (np.abs(np.atleast_2d(lhs).astype(np.float64)) * np.abs(np.atleast_2d(rhs).astype(np.float64))).sum(1))
            tol = 1e-12 * scale if elem == "f64" else 1e-5 * scale + 2e-7
            bad = ~((np.isnan(got) & np.isnan(ref)) | (np.abs(got.astype(np.float64) - ref) <= tol))   # (an i8 zero vector: cosine NaN)
            assert not bad.any(), (name, elem, V.METRIC_NAMES[metric], ls, rs, np.flatnonzero(bad)[:4].tolist(), got[bad][:4], ref[bad][:4])
