"""Case tables of the vector edge suites (tests/test_gpu_vector_edges.py on the device, tests/test_vec_ref_cpu.py for the tables
themselves): seeded data classes and, per entry point of k_vector.hip, shapes on both sides of every threshold in the code. A case
is named by the branch it takes; the helpers below restate the dispatch rules of k_vector.hip so that the names are computed.

Data classes
  normal     standard_normal f32
  grid       integers in [-3, 3] (dim <= 128): exact in bf16, and every dot, squared difference and l1 sum is exact in f32 in any
             order — every path must return the one list, its many genuine ties by the lower row id. A few zero rows and a zero
             query (cosine NaN; cosine itself is rounded, so grid is judged strictly under dot, l2 and l1 only)
  dupes      every base row is the same grid-valued vector: all rows tie with tau, the candidate list fills / overflows; answer
             ids 0..k-1 on every path. dupes_normal: the same with a normal-valued vector, judged to eps only
  collapsed  2,000 rows c + delta with |delta_k| below a quarter bf16 ulp of c_k among normal rows: ONE bf16 image, only the low
             parts the filter cannot see decide the top-k. Queries c + delta' and -c + delta'. collapsed_aligned: the low
             parts all along c and part of the block before S0 — tau is a block distance and no term of the bound has slack
  offset     normal * 1e-2 + 100: |b|^2 ~ 1e4 dim against distances ~0.1 — the expanded l2 form of the filter cancels, the
             re-scored answer must not. l2 only: under dot and cosine every row lies within eps of every other
  far_tail   behind S0 only rows that no query can want: the filter keeps no candidate at all (maxc == 0)
  special    zero rows, NaN / Inf components, rows * 1e18, 1e-18, 1e20 (squares overflow f32), f32 denormals, components that
             round to bf16 infinity; the zero query and a query * 1e15. Judged against orc_vec_distance (f32: overflow is part of
             the semantics)
"""
from types import SimpleNamespace

import numpy as np

from tests import vec_ref as R

COSINE, L2, DOT, L1, NORM = R.COSINE, R.L2, R.DOT, R.L1, R.NORM
METRIC_NAMES = {COSINE: "cosine", L2: "l2", DOT: "dot", L1: "l1", NORM: "norm"}

# the constants of k_vector.hip the shapes straddle
KMAX = 16
SEL_SEG = 8192        # scores per workgroup of select_stage_kernel; more than one segment -> a second stage
SEL_LIST = 512        # LDS list of select_stage_kernel
EXACT_MAX = 65536     # topk_batch / sample_rows: up to here everything is scored exactly
CAND_CAP = 4096       # candidates kept per query by a filter pass; one more falls back to the exact scan
S0 = 8192             # index_search_batch: rows scored exactly before the bf16 filter starts
QB = 2048             # queries per batch of dbhip_vec_topk / dbhip_vec_index_search
HBK = 64              # bf16 k-tile: dpad = dim rounded up to it

COLLAPSED_N = S0 + 3000
COLLAPSED_BLOCK = (S0 + 500, S0 + 2500)


# ---- the dispatch rules, restated ----------------------------------------------------------------------------------------------------
def dot_tile(nq, dim, aligned=True):
    """launch_dot: the tile shape of dot_tile_kernel"""
    if dim % 4 != 0 or dim < 4 or not aligned:
        return "scalar128x128"
    return "t32x256" if nq <= 32 else ("t64x256" if nq <= 64 else "t128x128")


def filter_kernel(rows, dim, nq):
    """index_search_batch::filter_range over `rows` base rows"""
    dpad = -(-dim // HBK) * HBK
    if nq <= 128:
        return "f128"
    if (dpad // HBK) % 2 == 0 and dpad >= 128 and rows >= 256:
        return "f256x8phase"
    return "ftall"


def index_path(n, dim, nq):
    nqb = min(nq, QB)
    if n <= S0:
        return "exact_only"
    if n > EXACT_MAX:
        return "two_levels_" + filter_kernel(EXACT_MAX - S0, dim, nqb) + "_" + filter_kernel(n - EXACT_MAX, dim, nqb)
    return filter_kernel(n - S0, dim, nqb)


def topk_path(n, metric):
    if n > EXACT_MAX and metric in (COSINE, DOT):
        return "sample_filter"
    return "exact_%dseg" % max(1, -(-n // SEL_SEG))


def rows_group(dim):
    """dbhip_vec_distance_rows: lanes per row"""
    g = 0
    while g < 6 and (4 << g) < dim:
        g += 1
    return 1 << g


# ---- data classes -------------------------------------------------------------------------------------------------------------------
def bf16_image(x):
    """f32 -> the f32 value of its bf16 rounding (nearest even); finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def normal(n, dim, nq, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((nq, dim)).astype(np.float32)


def grid(n, dim, nq, seed, zero_query=True):
    assert dim <= 128
    rng = np.random.default_rng(seed)
    base = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    q = rng.integers(-3, 4, (nq, dim)).astype(np.float32)
    for r in (3, n // 2, n - 1):
        if 0 <= r < n and n > 4:
            base[r] = 0.0
    if zero_query and nq > 1:
        q[nq // 2] = 0.0
    return base, q


def dupes(n, dim, nq, seed, exact=True):
    """exact: grid-valued row and queries — every kernel gives every row the same float, so ids 0..k-1 is the one answer. Otherwise
    normal-valued: the same row scores an ulp apart in kernels that sum in different orders (dot_tile_kernel before S0,
    rescore_kernel behind it), so only the tolerant statement holds"""
    rng = np.random.default_rng(seed)
    if exact:
        row, q = rng.integers(-3, 4, dim).astype(np.float32), rng.integers(-3, 4, (nq, dim)).astype(np.float32)
        row[0], q[:, 0] = 1.0, 2.0          # no zero vector
    else:
        row, q = rng.standard_normal(dim).astype(np.float32), rng.standard_normal((nq, dim)).astype(np.float32)
    return np.tile(row, (n, 1)), q


COLLAPSED_ALIGNED_ROWS = ((4000, 4100), (S0 + 500, S0 + 1100))   # 100 rows in the exactly scored part, 600 behind S0


def collapsed(dim, nq, seed, aligned=False):
    """n = COLLAPSED_N; queries [0, nq/2) are c + delta', [nq/2, nq) are -c + delta'.
    aligned: the bound's worst case. The low parts all point along c (delta = s u, u_k = 0.24 ulp(c_k) sign(c_k), s in [-0.9, 0.9] per
    row and per query, plus a jitter), so Cauchy-Schwarz is met almost with equality in every term and no term's slack covers for
    another; and 100 rows of the block lie before S0, so tau is itself a block distance: the rows behind S0 that beat it survive
    the filter only if the bound holds every term. (With random deltas |c . delta| is far below |c| |delta|, and with the block
    behind S0 only, tau comes from normal rows far away: a bound that lost a term would still pass the block.)"""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((COLLAPSED_N, dim)).astype(np.float32)
    c = bf16_image((rng.uniform(2.0, 7.5, dim) * rng.choice([-1.0, 1.0], dim)).astype(np.float32))
    ulp = 2.0 ** (np.floor(np.log2(np.abs(c.astype(np.float64)))) - 7)
    sign = np.where(np.arange(nq) < (nq + 1) // 2, 1.0, -1.0)[:, None]
    if not aligned:
        lo, hi = COLLAPSED_BLOCK
        base[lo:hi] = (c + rng.uniform(-0.24, 0.24, (hi - lo, dim)) * ulp).astype(np.float32)
        q = (sign * c + rng.uniform(-0.24, 0.24, (nq, dim)) * ulp).astype(np.float32)
        return base, q
    u = 0.24 * ulp * np.sign(c)

    def low(m):
        return rng.uniform(-0.9, 0.9, (m, 1)) * u + rng.uniform(-0.02, 0.02, (m, dim)) * ulp
    for lo, hi in COLLAPSED_ALIGNED_ROWS:
        base[lo:hi] = (c + low(hi - lo)).astype(np.float32)
    q = (sign * (c + low(nq))).astype(np.float32)
    return base, q


def offset(n, dim, nq, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((n, dim)) * 1e-2 + 100).astype(np.float32),
            (rng.standard_normal((nq, dim)) * 1e-2 + 100).astype(np.float32))


SPECIAL_WEAK_QUERIES = (0, 1)   # the zero query (cosine NaN, dot 0 everywhere) and the query * 1e15 (l2: every row at one f32 distance)


def special(n, dim, nq, seed):
    """every special row behind S0, where the bf16 filter meets it; the huge and non-finite ones before S0 as well, where they
    shape tau. (The zero, * 1e-18 and denormal rows are one l2 distance from any query: one of each, so the tie stays under the cap.)"""
    assert n >= S0 + 257 and dim >= 8 and nq >= 3
    base, q = normal(n, dim, nq, seed)
    for at in (7, S0 + 3):
        base[at + 4] *= 1e18
        base[at + 12, 3] = np.nan
        base[at + 16, 5] = np.inf
        base[at + 20] *= 1e20               # squares overflow f32
        base[at + 28, 2] = 3.39e38          # rounds to bf16 infinity (one component: what overflows does so in any summation order)
    base[S0 + 3] = 0.0                      # a zero row
    base[S0 + 11] *= 1e-18
    base[S0 + 27] = 1e-40                   # f32 denormals
    q[0] = 0.0
    q[1] *= 1e15
    return base, q


def far_tail(n, dim, nq, seed, side):
    """queries near the all-ones vector, normal rows before S0, and behind S0 only rows no query can want: near -4 * ones
    (side = -1: cosine distance ~2, l2 ~5 sqrt(dim)) or near +4 * ones (side = +1: the largest inner products, last under dot).
    Their lower bounds lie far above tau, so no query keeps a candidate: the maxc == 0 return of index_search_batch"""
    assert n > S0
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((n, dim)).astype(np.float32)
    base[S0:] = (side * 4.0 + 0.3 * rng.standard_normal((n - S0, dim))).astype(np.float32)
    return base, (1.0 + 0.3 * rng.standard_normal((nq, dim))).astype(np.float32)


def make(c):
    """(base, queries) f32 of a case"""
    if c.cls == "far_tail":
        return far_tail(c.n, c.dim, c.nq, c.seed, c.side)
    if c.cls == "normal":
        return normal(c.n, c.dim, c.nq, c.seed)
    if c.cls == "grid":
        return grid(c.n, c.dim, c.nq, c.seed, zero_query=getattr(c, "zero_query", True))
    if c.cls in ("dupes", "dupes_normal"):
        return dupes(c.n, c.dim, c.nq, c.seed, exact=c.cls == "dupes")
    if c.cls in ("collapsed", "collapsed_aligned"):
        assert c.n == COLLAPSED_N
        return collapsed(c.dim, c.nq, c.seed, aligned=c.cls == "collapsed_aligned")
    if c.cls == "offset":
        return offset(c.n, c.dim, c.nq, c.seed)
    if c.cls == "special":
        return special(c.n, c.dim, c.nq, c.seed)
    if c.cls == "placed":
        return c.build()
    raise KeyError(c.cls)


def reference(c, metric, base, q, oracle=None):
    """(D, E): reference distances [nq, n] and their tolerance. `special` is judged in the oracle's f32, everything else in float64;
    dupes needs one column only."""
    if c.cls == "special":
        import ctypes as C
        D32 = np.zeros((q.shape[0], base.shape[0]), np.float32)
        oracle.orc_vec_distance(metric, base.ctypes.data_as(C.c_void_p), C.c_int64(base.shape[0]), base.shape[1], q.ctypes.data_as(C.c_void_p),
                                q.shape[0], D32.ctypes.data_as(C.c_void_p))
        D = D32.astype(np.float64)
        return D, R.eps(metric, D, base, q)
    if c.cls in ("dupes", "dupes_normal"):
        D1 = R.distances(metric, base[:1], q)
        return np.repeat(D1, base.shape[0], axis=1), np.repeat(R.eps(metric, D1, base[:1], q), base.shape[0], axis=1)
    D = R.distances(metric, base, q)
    return D, R.eps(metric, D, base, q)


# grid is run under dot, l2 and l1 in the top-k tables and under dot and l2 in the index tables, never under cosine: a cosine
# distance divides by rounded norms, so it is not exact, and its values on a grid lie closer than eps to one another in their
# thousands — check_topk_strict does not apply and check_topk would be a weak leg, which no grid leg may be. The zero rows and
# the zero query of the class give cosine NaN in DISTANCE_CASES (whole matrices, judged element by element); through top-k and
# the index, cosine NaN comes from `special` (a zero row behind S0, the zero query), judged with eps = 0 on every NaN row.
# offset is l2 only for the reason in the header: its dot products and cosine distances all lie within eps of one another.
STRICT_GRID = (DOT, L2, L1)


def strict(c, metric):
    """judged by check_topk_strict: inputs whose arithmetic is exact in any order"""
    return c.cls == "dupes" or (c.cls in ("grid", "placed") and metric in STRICT_GRID)


# Legs that cannot meet the band cap (tests/test_vec_ref_cpu.py: at most 4 rows within eps of the k-th best), by name, with the
# statement they are judged by instead. No normal, grid, offset or collapsed-l2 leg is here.
WEAK = [
    dict(cls="collapsed", metric=COSINE, queries=None,
         reason="the 2,000 block rows lie within 1e-7 of one another, far inside eps",
         judged_by="check_topk: every returned row is within eps of the k-th best, which only block rows are — fails if the filter drops the block"),
    dict(cls="collapsed", metric=DOT, queries=None,
         reason="eps = 1e-5 sum|q_k b_k| ~ 6e-4 |c|^2 is wider than the spacing of the block's dot products near the k-th best",
         judged_by="check_topk as above: for the -c queries only block rows are within eps of the k-th best"),
    dict(cls="special", metric=None, queries=SPECIAL_WEAK_QUERIES,
         reason="zero query: cosine NaN and dot 0 on every row; query * 1e15: one f32 l2 distance for every finite row",
         judged_by="check_topk: equal infinities tie, distances of NaN / infinite rows are not finite, fillers and distinct ids hold"),
    dict(cls="dupes", metric=None, queries=None,
         reason="every row has the same distance (grid-valued: the same float in every kernel)",
         judged_by="check_topk_strict: ids 0..k-1"),
    dict(cls="dupes_normal", metric=None, queries=None,
         reason="every row has the same distance, an ulp apart between kernels that sum in different orders",
         judged_by="check_topk: k distinct rows, distances within eps of the one reference distance, fillers"),
]


def weak_queries(c, metric):
    """None: no query of this leg is weak; 'all'; or the tuple of weak query numbers"""
    for w in WEAK:
        if w["cls"] == c.cls.replace("_aligned", "") and w["metric"] in (None, metric):
            return "all" if w["queries"] is None else w["queries"]
    return None


BAND_CAP = 4   # the k-th row itself plus three


def _case(name, cls, n, dim, nq, k=None, metrics=None, **kw):
    seed = (n * 1_000_003 + dim * 10_007 + nq * 101 + (k or 0)) % (1 << 31)
    return SimpleNamespace(name=name, cls=cls, n=n, dim=dim, nq=nq, k=k, metrics=metrics, seed=seed, **kw)


def _named(cases):
    out = {}
    for c in cases:
        assert c.name not in out, c.name
        out[c.name] = c
    return out


# ---- dbhip_vec_distance: one sweep per axis, the other two small -------------------------------------------------------------------------
ALL4 = (COSINE, L2, DOT, L1)


def _dist(cls, n, nq, dim, aligned=True):
    name = "%s_n%d_nq%d_dim%d_%s%s" % (cls, n, nq, dim, dot_tile(nq, dim, aligned), "" if aligned else "_off4bytes")
    return _case(name, cls, n, dim, nq, metrics=ALL4, aligned=aligned)


DISTANCE_N = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2049)   # 64: diff_valu tile; 128 / 256: dot tiles; 2049: 9 -> 16 i-tile slots
DISTANCE_NQ = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
DISTANCE_DIM = (1, 2, 3, 4, 5, 31, 32, 33, 36, 63, 64, 65)        # 4: VEC4 from here; 32: one k-tile; 36 / 65: the k tail of load4
DISTANCE_CASES = _named(
    [_dist("normal", n, 3, 8) for n in DISTANCE_N] +
    [_dist("normal", n, 65, 8) for n in (127, 128, 129)] +
    [_dist("normal", 70, nq, 8) for nq in DISTANCE_NQ] +
    [_dist("normal", 70, 5, dim) for dim in DISTANCE_DIM] +
    [_dist("normal", 257, 129, 33), _dist("grid", 129, 65, 36), _dist("grid", 300, 33, 7), _dist("offset", 2049, 33, 5),
     # base and queries 4 bytes off 16-byte alignment at dim % 4 == 0: scalar staging; nq <= 64 in a 128 x 128 tile, heavy clamping
     _dist("normal", 129, 33, 8, aligned=False)])


# ---- dbhip_vec_topk ---------------------------------------------------------------------------------------------------------------------
def _topk(cls, n, dim, nq, k, metrics=None, tag="", **kw):
    if metrics is None:
        metrics = {"grid": STRICT_GRID, "dupes": (COSINE, DOT, L2)}.get(cls, ALL4)
    name = "%s_n%d_dim%d_nq%d_k%d_%s%s" % (cls, n, dim, nq, k, topk_path(n, COSINE), tag)
    return _case(name, cls, n, dim, nq, k=k, metrics=metrics, **kw)


def _placed(kind):
    """grid-valued rows placed so that the small l2 / l1 distances to the zero query sit at chosen (segment, thread) positions of
    select_stage_kernel (element p of a segment belongs to thread p % 256)"""
    def build():
        n = SEL_SEG if kind == "densest" else 2 * SEL_SEG
        base = np.full((n, 4), 3.0, np.float32)                       # far
        if kind == "densest":
            # threads 0..14 hold 32 scores each below the 16th thread minimum (thread 15's): 15 * 32 + 1 = 481 list entries, the
            # most a segment can pass at k = 16 (the thread whose minimum IS the threshold passes only that one score)
            p = np.arange(n)
            base[p % 256 < 15] = (1.0, 0.0, 0.0, 0.0)
            base[15] = (1.0, 1.0, 0.0, 0.0)
        else:
            base[:16] = (1.0, 0.0, 0.0, 0.0)                          # segment 0: its 16 best in 16 threads' strides
            for j in range(16):                                       # segment 1: its 16 best all in thread 7's stride
                base[SEL_SEG + 256 * j + 7] = (0.0, 0.0, 0.0, 0.0) if j % 2 == 0 else (0.0, 1.0, 0.0, 0.0)
        q = np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, -1, 0, 0]], np.float32)
        return base, q
    n = SEL_SEG if kind == "densest" else 2 * SEL_SEG
    name = {"densest": "placed_sel_list_densest_481_of_512_k16", "spread": "placed_16_threads_vs_one_thread_k16"}[kind]
    return _case(name, "placed", n, 4, 3, k=16, metrics=(L2, L1), build=build)


TOPK_CASES = _named(
    [_topk("normal", 300, 8, 3, k) for k in (1, 2, 15, 16)] +
    [_topk("normal", 5, 8, 3, 16, tag="_k_above_n"), _topk("normal", 0, 8, 3, 3, tag="_no_rows"), _topk("normal", 300, 8, 0, 3, tag="_no_queries"),
     _topk("grid", 300, 8, 5, 16)] +
    # 8192: one / two segments (a second select stage); 65536: exact / sample + filter with tau; + 300: a ragged filter tile
    [_topk("normal", n, 4 if n % 2 else 8, 5, 10) for n in (1, 8191, 8192, 8193, 16_385, 65_536, 65_537, 65_836)] +
    [_topk("grid", 8193, 8, 5, 16), _topk("grid", 65_836, 8, 5, 16)] +
    # the filter's tile shapes (nq <= 32, <= 64, above), and the QB = 2048 query batches
    [_topk("normal", 65_836, 8, nq, 10, metrics=(COSINE, DOT)) for nq in (1, 33, 65)] +
    [_topk("normal", 8449, 8, 2048, 10, metrics=(COSINE,), tag="_one_batch"), _topk("normal", 8449, 8, 2049, 10, metrics=(COSINE, L2, DOT), tag="_two_batches"),
     # every row ties with tau: CAND_CAP candidates are kept, CAND_CAP + 1 fall back to the exact scan with the carry slot
     _topk("dupes", EXACT_MAX + CAND_CAP, 8, 3, 16, tag="_cand_list_full"), _topk("dupes", EXACT_MAX + CAND_CAP + 1, 8, 3, 16, tag="_cand_overflow_fallback"),
     _placed("densest"), _placed("spread")])


# ---- dbhip_vec_index_* ------------------------------------------------------------------------------------------------------------------
IDX3 = (COSINE, DOT, L2)


def _index(cls, n, dim, nq, k, metrics=None, tag="", **kw):
    if metrics is None:
        metrics = {"grid": (DOT, L2), "offset": (L2,)}.get(cls, IDX3)
    name = "%s_n%d_dim%d_nq%d_k%d_%s%s" % (cls, n, dim, nq, k, index_path(n, dim, nq), tag)
    return _case(name, cls, n, dim, nq, k=k, metrics=metrics, **kw)


INDEX_CASES = _named(
    # rows behind S0: 128 = one base tile of the 128-row kernels, 256 = the least the 8-phase kernel takes and its tile
    [_index("normal", S0 + r, 96, 129, 10) for r in (0, 1, 127, 128, 129, 255, 256, 257)] +
    [_index("normal", S0 + r, 64, 5, 16) for r in (1, 129)] +
    [_index("normal", 0, 8, 3, 3), _index("normal", 5, 8, 3, 16), _index("normal", 8191, 8, 3, 1),
     _index("normal", EXACT_MAX + 300, 8, 33, 16), _index("grid", EXACT_MAX + 300, 8, 5, 16, zero_query=False)] +
    # queries: 128 = the 256-query tiles begin; 256 = a second query tile; nq_pad zero rows behind the queries
    [_index("normal", S0 + 257, 128, nq, 16 if nq % 2 else 1) for nq in (1, 127, 128, 129, 255, 256, 257)] +
    [_index("normal", S0 + 257, 8, 2049, 10, metrics=(COSINE, L2), tag="_two_batches")] +
    # dpad: 65 / 129 zero padding; 96 / 128 -> dpad 128 and 256 -> four k-tiles: 8-phase; 192 -> three k-tiles: the plain tall kernel
    # (at dim = 1 a cosine distance is 0 or 2: no top-k to speak of, dot and l2 only)
    [_index("normal", S0 + 300, dim, 130, 16 if dim % 2 else 1, metrics=(DOT, L2) if dim == 1 else None) for dim in (1, 3, 63, 64, 65, 96, 128, 129, 192, 256)] +
    # every class through the 8-phase kernel and through bf16_filter_kernel<., 128>
    [_index("grid", S0 + 300, 128, 130, 16), _index("grid", S0 + 300, 100, 9, 16),
     # the candidate list exactly full (kept) and one over (fallback to the exact scan with the carry slot)
     _index("dupes", S0 + CAND_CAP, 128, 129, 16, tag="_cand_list_full"), _index("dupes", S0 + CAND_CAP + 1, 128, 129, 16, tag="_cand_overflow_fallback"),
     _index("dupes", S0 + CAND_CAP, 64, 3, 16, tag="_cand_list_full"), _index("dupes", S0 + CAND_CAP + 1, 64, 3, 16, tag="_cand_overflow_fallback"),
     _index("dupes_normal", S0 + CAND_CAP, 128, 129, 16, tag="_cand_list_full"), _index("dupes_normal", S0 + CAND_CAP, 64, 3, 16, tag="_cand_list_full"),
     _index("collapsed", COLLAPSED_N, 128, 130, 10), _index("collapsed", COLLAPSED_N, 64, 20, 10),
     _index("collapsed_aligned", COLLAPSED_N, 128, 130, 10), _index("collapsed_aligned", COLLAPSED_N, 64, 20, 10),
     _index("offset", S0 + 257, 128, 129, 10), _index("offset", S0 + 257, 64, 9, 10),
     _index("special", S0 + 257, 128, 129, 10), _index("special", S0 + 257, 36, 9, 10),
     # no row behind S0 survives the filter: maxc == 0, the sample's answer stands
     _index("far_tail", S0 + 300, 128, 129, 10, metrics=(COSINE, L2), tag="_no_candidates", side=-1),
     _index("far_tail", S0 + 300, 128, 129, 10, metrics=(DOT,), tag="_no_candidates_dot", side=1),
     _index("far_tail", S0 + 300, 64, 5, 16, metrics=(COSINE, L2), tag="_no_candidates", side=-1),
     _index("far_tail", S0 + 300, 64, 5, 16, metrics=(DOT,), tag="_no_candidates_dot", side=1)])


# ---- dbhip_vec_topk_merge: (m, nq, k) ---------------------------------------------------------------------------------------------------
# A stage turns every segment of 8192 entries into k: one stage up to 8192 entries, two up to 8192 * (8192 / k) (8192 * 16 + 1 makes
# 17 lists of 16 = 272 entries, still one more stage), three from 8192 * 512 + 1 at k = 16.
def merge_stages(m, k):
    stages, n = 1, m
    while n > SEL_SEG:
        n = -(-n // SEL_SEG) * k
        stages += 1
    return stages


MERGE_CASES = {"m%d_nq%d_k%d_%dstage" % (m, nq, k, merge_stages(m, k)): (m, nq, k)
               for m, nq, k in [(1, 1, 16), (15, 3, 16), (16, 3, 16), (8192, 3, 16), (8193, 3, 16), (8192 * 16 + 1, 1, 16), (8192 * 16 + 1, 3, 16),
                                (8192 * 512 + 1, 1, 16), (8193, 1, 1), (9, 3, 10)]}


def merge_lists(m, nq, k):
    """candidate lists with fillers, NaN distances, duplicate distances under different ids and ids near 2^32 - 2"""
    rng = np.random.default_rng(m * 31 + nq)
    d = rng.integers(0, max(2, m // 3), (nq, m)).astype(np.float32) * 0.25       # many duplicate distances
    ids = np.stack([rng.permutation(m) for _ in range(nq)]).astype(np.uint32)
    big = rng.random((nq, m)) < 0.2
    ids[big] = np.uint32(0xFFFFFFFE) - ids[big]                                   # still distinct within a row
    d[rng.random((nq, m)) < 0.1] = np.nan
    d[rng.random((nq, m)) < 0.05] = np.inf                                        # a real row at +inf sorts before the fillers
    fill = rng.random((nq, m)) < 0.15
    d[fill] = np.inf
    ids[fill] = R.FILL
    if m > 4 and nq > 1:
        d[-1, max(0, k - 3):] = np.inf                                            # a row with fewer than k real entries
        ids[-1, max(0, k - 3):] = R.FILL
    return d, ids


# ---- dbhip_score_u8: (dim, n, base offset in bytes) ----------------------------------------------------------------------------------------
def _u8_path(dim, off):
    return "quarter_wave" if dim % 16 == 0 and off % 16 == 0 and dim <= 16384 else "wave_per_row"


SCORE_U8_CASES = {"dim%d_n%d_off%d_%s" % (dim, n, off, _u8_path(dim, off)): (dim, n, off)
                  for dim, n, off in [(d, 5, 0) for d in (1, 15, 16, 17, 100, 16_384, 16_400)] +
                  [(16, n, 0) for n in (0, 1, 3, 4, 257)] + [(17, n, 0) for n in (1, 4, 257)] + [(16, 5, 1), (64, 257, 1)]}


def score_u8_data(dim, n):
    rng = np.random.default_rng(dim * 7 + n)
    base = rng.integers(0, 128, (n, dim)).astype(np.uint8)
    q = rng.integers(0, 128, dim).astype(np.uint8)
    if dim == 16_384 and n:
        base[n - 1] = 127
        q[:] = 127                      # 127^2 * 16384 < 2^32: the u32 accumulator's largest sum
    return q, base


# ---- dbhip_vec_distance_rows: G lanes per row doubles at dim 5, 9, 17, 33, 65, 129 ---------------------------------------------------------
ROWS_DIM = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257)
ROWS_N = (1, 2, 63, 64, 65, 257)
ROWS_CASES = {"dim%d_n%d_G%d" % (dim, n, rows_group(dim)): (dim, n) for dim, n in [(d, 65) for d in ROWS_DIM] + [(17, n) for n in ROWS_N] + [(5, 257), (129, 5)]}


def rows_data(dim, n, elem):
    """elem: 'f32', 'f64', 'i8'; the last row differs from row 0 (dead rows of the last block are redirected to row 0)"""
    rng = np.random.default_rng(dim * 13 + n)
    if elem == "i8":
        a, b = rng.integers(-128, 128, (n, dim)).astype(np.int8), rng.integers(-128, 128, (n, dim)).astype(np.int8)
    else:
        dt = np.float32 if elem == "f32" else np.float64
        a, b = rng.standard_normal((n, dim)).astype(dt), rng.standard_normal((n, dim)).astype(dt)
    if n > 1:
        a[-1] = a[0] + (a[0] == a[0]).astype(a.dtype)   # row 0 shifted by one: never equal to it
    return a, b
