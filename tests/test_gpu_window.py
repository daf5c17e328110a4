"""GPU: the five window calls (include/dbhip.h a19) through device.Window, every result asserted row by row against tests/window_ref.py
(plain Python / numpy; tests/test_window_ref_cpu.py holds that reference to its own loops, to sqlite3 and to six negative controls).
Everything is bit-exact except a float SUM, which must lie inside float_ref.sum_ok's any-order bound over the frame's OWN terms, and
a float MIN / MAX, compared with float_ref.same_value. Nothing is sampled."""
import sqlite3

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import float_ref as F
from tests import sort_ref as R
from tests import window_ref as W

pytestmark = pytest.mark.gpu

TYPE_OF = {"bool": T.T_BOOL, "i8": T.T_I8, "i16": T.T_I16, "i32": T.T_I32, "i64": T.T_I64, "u8": T.T_U8, "u16": T.T_U16, "u32": T.T_U32,
           "u64": T.T_U64, "f32": T.T_F32, "f64": T.T_F64, "date": T.T_DATE, "ts": T.T_TIMESTAMP, "dec64": T.T_DEC64, "dec128": T.T_DEC128,
           "str": T.T_STRING, "lstr": T.T_STRING}
BIG = 3_000_001
RUNNING = W.Frame(W.ROWS, W.UNBOUNDED_PRECEDING, W.CURRENT_ROW)


def to_gpu(gpu, c):
    if c.kind == "bool":
        return gpu.Column.boolean(c.values, validity=c.valid)
    if c.kind == "dec128":
        return gpu.Column.decimal128(c.values, 38, 0, validity=c.valid)
    if c.kind == "dec256":
        return gpu.Column.decimal256(c.values, 76, 0, validity=c.valid)
    if c.kind in R.STRING_KINDS:
        return gpu.Column.strings(c.values, validity=c.valid)
    return gpu.Column.from_numpy(c.values, TYPE_OF[c.kind], validity=c.valid, precision=18 if c.kind == "dec64" else 0)


def to_gpu_sliced(gpu, c, seed):
    """the column as rows [13, 13 + n) of a column of n + 77 rows: value buffers by address, the validity Bitmap by bit offset"""
    rng = np.random.default_rng(seed)
    head, tail = R.make_col(rng, 13, c.kind, c.valid is not None), R.make_col(rng, 64, c.kind, c.valid is not None)
    s = to_gpu(gpu, R.concat(R.concat(head, c), tail)).slice(13, 13 + c.n)
    assert s.voff == 13
    return s


def gframe(gpu, f):
    return gpu.WindowFrame(f.units, (f.sk, f.so), (f.ek, f.eo))


def as_list(x):
    return x.tolist() if isinstance(x, np.ndarray) else list(x)


def nullable_list(vals, valid):
    return [v if ok else None for v, ok in zip(as_list(vals), as_list(valid))]


def check(got, exp, kind="i64", agg=None, what=""):
    if got == exp:
        return
    why = W.same_results(got, exp, kind, agg)
    assert why == "", (what, why)


def reference_bounds(parts, orders, n):
    return (W.boundaries if n <= 65 else W.boundaries_fast)(parts, orders, n)


def check_bounds(gpu, parts, orders, gparts, gorders, n, what=""):
    w = gpu.Window(gparts, gorders, n=n)
    got = w.bounds()
    exp = reference_bounds(parts, orders, n)
    for name, g, e in zip(("part_start", "part_end", "peer_start", "peer_end"), got, exp):
        e = np.asarray(e, dtype=np.uint32)
        bad = np.nonzero(g != e)[0]
        assert len(bad) == 0, (what, name, int(bad[0]), int(g[bad[0]]), int(e[bad[0]]))
    return w, tuple(np.asarray(e, dtype=np.int64) for e in exp)


# ---- boundaries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("kind", R.ALL_KINDS)
def test_bounds_every_key_kind(gpu, kind, nullable):
    """every key type as the partition key and as the order key, at the sizes around the wave and the scan tiles"""
    for n in R.SIZES:
        cols = W.sorted_keys(41, n, [("u8", False, "low"), (kind, nullable, "low" if kind != "bool" else "pool"), (kind, nullable, "pool")])
        g = [to_gpu(gpu, c) for c in cols]
        check_bounds(gpu, [cols[1]], [cols[2]], [g[1]], [g[2]], n, (kind, n, "partition key"))
        check_bounds(gpu, [cols[0]], [cols[1]], [g[0]], [g[1]], n, (kind, n, "order key"))


@pytest.mark.parametrize("n", R.SIZES + [BIG])
@pytest.mark.parametrize("shape", W.SHAPES)
def test_bounds_and_rank_family_on_partition_shapes(gpu, shape, n):
    """one partition, every row its own, heads on tile starts, one partition over many tiles, mixed; then the rank family and ntile"""
    p, o = W.layout(3, n, shape)
    w, b = check_bounds(gpu, [p], [o], [to_gpu(gpu, p)], [to_gpu(gpu, o)], n, (shape, n))
    for kind in (W.ROW_NUMBER, W.RANK, W.DENSE_RANK):
        assert np.array_equal(w.rank(kind), W.rank_fast(kind, b)), (shape, n, kind)
    for kind in (W.PERCENT_RANK, W.CUME_DIST):
        got, exp = w.rank(kind), W.rank_fast(kind, b)
        assert np.array_equal(got.view(np.uint64), exp.view(np.uint64)), (shape, n, kind)      # bit for bit
    rows = int((b[1] - b[0]).max())
    for buckets in (1, 3, rows, rows + 1):
        assert np.array_equal(w.rank(W.NTILE, buckets), W.rank_fast(W.NTILE, b, buckets)), (shape, n, buckets)
    if n <= 65:
        for kind in (W.ROW_NUMBER, W.RANK, W.DENSE_RANK, W.PERCENT_RANK, W.CUME_DIST):
            assert as_list(w.rank(kind)) == W.rank(kind, tuple(as_list(x) for x in b)), (shape, n, kind)


@pytest.mark.parametrize("n", [1, 65, 4097, 100_003])
def test_bounds_sliced_columns(gpu, n):
    """validity bit offset 13, value buffers by address (dbhip_col carries no bit offset for Boolean VALUES, so a sliced Boolean column is no
    key here, as for dbhip_sort_perm: the binding materialises it first)"""
    for kind in (k for k in R.ALL_KINDS if k != "bool"):
        cols = W.sorted_keys(43, n, [(kind, True, "low"), (kind, True, "pool")])
        g = [to_gpu_sliced(gpu, c, 7 + k) for k, c in enumerate(cols)]
        check_bounds(gpu, [cols[0]], [cols[1]], [g[0]], [g[1]], n, (kind, n))


@pytest.mark.parametrize("n", [2, 65, 4097, 100_003])
def test_bounds_multi_key(gpu, n):
    """3 partition keys + 2 order keys, NULLs and floats among them; no partition key; no order key"""
    keys = [("u8", True, "low"), ("f32", True, "low"), ("str", True, "low"), ("i16", True, "low"), ("f64", True, "pool")]
    cols = W.sorted_keys(44, n, keys)
    g = [to_gpu(gpu, c) for c in cols]
    check_bounds(gpu, cols[:3], cols[3:], g[:3], g[3:], n, "3 + 2")
    check_bounds(gpu, [], cols[:2], [], g[:2], n, "0 + 2")
    check_bounds(gpu, cols[:2], [], g[:2], [], n, "2 + 0")
    check_bounds(gpu, [], [], [], [], n, "0 + 0")


def test_bounds_eight_plus_eight_keys_and_no_rows(gpu):
    n = 20_011
    cols = W.sorted_keys(45, n, [(k, i % 2 == 0, "low") for i, k in enumerate(R.MIXED8)] + [(k, i % 2 == 1, "low" if i < 6 else "pool") for i, k in enumerate(R.MIXED8[::-1])])
    g = [to_gpu(gpu, c) for c in cols]
    check_bounds(gpu, cols[:8], cols[8:], g[:8], g[8:], n, "8 + 8")
    w = gpu.Window([], [], n=0)
    assert all(len(x) == 0 for x in w.bounds()) and len(w.rank(W.RANK)) == 0


# ---- shift ----------------------------------------------------------------------------------------------------------------------
def value_column(rng, n, kind, nullable=True):
    if kind == "dec256":
        vals = [int(x) * (10 ** 40 + 7) for x in rng.integers(-10 ** 9, 10 ** 9, n)]
        return R.KeyCol("dec256", vals, rng.random(n) < 0.75 if nullable else None)
    return R.make_col(rng, n, kind, nullable)


def host_values(gpu, col, res):
    """the device result `res` (a Column) as a list with None for NULL; strings through the source column's data buffer"""
    valid = res.validity_numpy()
    if col.dtype == T.T_STRING:
        buf0 = next(k for k in col._keep if isinstance(k, gpu.DeviceBuffer))
        vals = gpu.view_strings(res.to_numpy(), buf0.to_numpy(np.uint8, buf0.nbytes))
    else:
        vals = res.to_numpy()
    return nullable_list(vals, valid)


SHIFT_KINDS = ["u8", "i16", "f32", "i64", "f64", "dec128", "dec256", "bool", "str", "lstr"]      # 1, 2, 4, 8, 16 and 32 bytes, bits, views


@pytest.mark.parametrize("kind", SHIFT_KINDS)
def test_shift(gpu, kind):
    """lag / lead by 0, 1, 2 and 70,000 rows with no default, a scalar default, a NULL scalar default and a column default"""
    strings = kind in R.STRING_KINDS
    for shape, n in (("mixed", 4097), ("long", 100_003)):
        p, o = W.layout(4, n, shape)
        w = gpu.Window([to_gpu(gpu, p)], [to_gpu(gpu, o)])
        b = W.boundaries_fast([p], [o], n)
        rng = np.random.default_rng([51, n])
        c, d = value_column(rng, n, kind), value_column(rng, n, kind)
        gc, gd = to_gpu(gpu, c), to_gpu(gpu, d)
        one = d.py()[0] if kind != "dec256" else d.values[0]
        for off in (0, 1, -1, 2, -2, 70_000, -70_000):
            got = host_values(gpu, gc, w.shift(gc, off, device=True))
            check(got, W.shift_fast(b, c.values, c.valid, off), kind, None, (kind, n, off, "no default"))
            if strings:
                continue
            if kind == "bool":
                sc = gpu.Column.boolean([bool(one)])
                sc.is_scalar = True
            else:
                sc = gpu.Column.scalar(one, gc.dtype, gc.precision, gc.scale)
            got = host_values(gpu, gc, w.shift(gc, off, default=sc, device=True))
            check(got, W.shift_fast(b, c.values, c.valid, off, ("scalar", one)), kind, None, (kind, n, off, "scalar default"))
            got = host_values(gpu, gc, w.shift(gc, off, default=gd, device=True))
            check(got, W.shift_fast(b, c.values, c.valid, off, ("column", d.values, d.valid)), kind, None, (kind, n, off, "column default"))
        if not strings:
            null_scalar = gpu.Column.scalar(one, gc.dtype, gc.precision, gc.scale) if kind != "bool" else gpu.Column.boolean([True])
            null_scalar.is_scalar = True
            null_scalar.validity = gpu.DeviceBuffer.from_numpy(gpu.pack_bits([False]))
            got = host_values(gpu, gc, w.shift(gc, -1, default=null_scalar, device=True))
            check(got, W.shift_fast(b, c.values, c.valid, -1, ("scalar", None)), kind, None, (kind, n, "NULL scalar default"))


# ---- value and aggregate ----------------------------------------------------------------------------------------------------------
def window_of(gpu, seed, n, shape):
    p, o = W.layout(seed, n, shape)
    return gpu.Window([to_gpu(gpu, p)], [to_gpu(gpu, o)]), W.boundaries_fast([p], [o], n)


def check_aggregates(gpu, w, b, c, gc, frames, aggs, what):
    for f in frames:
        gf = gframe(gpu, f)
        for agg in aggs:
            vals, valid = w.aggregate(agg, gc, gf)
            if agg == W.COUNT:
                assert valid.all(), (what, f)
            got = nullable_list(vals, valid)
            check(got, W.aggregate_fast(agg, b, c.values, c.valid, f, c.kind), c.kind, agg, (what, c.kind, f, agg))
            zeros = [v for v, ok in zip(as_list(vals), as_list(valid)) if not ok]
            assert all(v == 0 for v in zeros), (what, f, agg, "a NULL result carries the value 0")


@pytest.mark.parametrize("shape,n", [("mixed", 100_003), ("long", 100_003), ("tile_heads", 20_011), ("one", 4097), ("each", 4097), ("mixed", 65), ("one", 1)])
def test_aggregate_i64_over_every_frame(gpu, shape, n):
    """COUNT(*), COUNT(col), SUM, MIN, MAX of a nullable i64 over the 38 legal frames and offsets of 2^62"""
    w, b = window_of(gpu, 5, n, shape)
    vals, valid = W.int_values(np.random.default_rng(53), n, "i64", nullable=True)
    c = R.KeyCol("i64", vals, valid)
    gc = to_gpu(gpu, c)
    check_aggregates(gpu, w, b, c, gc, W.FRAMES + W.HUGE_FRAMES, (W.COUNT, W.SUM, W.MIN, W.MAX), shape)
    for f in W.FRAMES + W.HUGE_FRAMES:
        vals_, valid_ = w.aggregate(W.COUNT, None, gframe(gpu, f))
        assert valid_.all() and as_list(vals_) == W.aggregate_fast(W.COUNT, b, None, None, f), (shape, f, "count(*)")


@pytest.mark.parametrize("kind", ["i8", "i16", "i32", "u8", "u16", "u32", "u64", "date", "ts", "dec64"])
def test_aggregate_other_integer_types(gpu, kind):
    n = 20_011
    w, b = window_of(gpu, 6, n, "mixed")
    rng = np.random.default_rng(57)
    for nullable in (True, False):
        vals, valid = W.int_values(rng, n, kind, nullable=nullable)
        c = R.KeyCol(kind, vals, valid)
        aggs = (W.COUNT, W.MIN, W.MAX) if kind in ("date", "ts") else (W.COUNT, W.SUM, W.MIN, W.MAX)
        check_aggregates(gpu, w, b, c, to_gpu(gpu, c), W.FRAMES[::4] + W.HUGE_FRAMES[:2], aggs, nullable)


@pytest.mark.parametrize("kind", ["i64", "u8", "f64", "dec128", "dec256", "bool", "str", "lstr"])
def test_first_last_nth_value(gpu, kind):
    for shape, n in (("mixed", 20_011), ("long", 4097)):
        w, b = window_of(gpu, 7, n, shape)
        c = value_column(np.random.default_rng([59, n]), n, kind)
        gc = to_gpu(gpu, c)
        for f in (W.FRAMES if kind == "i64" else W.FRAMES[::6]) + W.HUGE_FRAMES[:3]:
            for vk, nth in ((W.FIRST_VALUE, 1), (W.LAST_VALUE, 1), (W.NTH_VALUE, 1), (W.NTH_VALUE, 3), (W.NTH_VALUE, 401), (W.NTH_VALUE, 2 ** 62)):
                got = host_values(gpu, gc, w.value(vk, gc, gframe(gpu, f), nth, device=True))
                check(got, W.value_fast(vk, b, c.values, c.valid, f, nth), kind, None, (kind, n, f, vk, nth))


# ---- floats ---------------------------------------------------------------------------------------------------------------------
FLOAT_FRAMES = [f for k, f in enumerate(W.FRAMES) if k % 3 == 0 or f.units == W.RANGE] + W.HUGE_FRAMES[:2] + [W.Frame(W.ROWS, (W.PRECEDING, 1), W.CURRENT_ROW)]


def float_sum_case(seed, n, shape, dtype, nullable=True):
    p, o = W.layout(seed, n, shape)
    b = W.boundaries_fast([p], [o], n)
    assert int((b[1] - b[0]).max()) <= F.MAX_SUM_ROWS
    vals, valid = W.float_values(np.random.default_rng([61, n]), n, R.FLOAT_KINDS[dtype], for_sum=True, nullable=nullable)
    with np.errstate(invalid="ignore"):
        live = vals.astype(np.float64)[valid if valid is not None else np.ones(n, bool)]
    assert np.all(np.abs(live[np.isfinite(live)]) <= F.MAX_SUM_ABS)
    return p, o, b, R.KeyCol(dtype, vals, valid)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape,n", [("mixed", 8193), ("long", 4097), ("tile_heads", 4096), ("one", 1100)])
def test_float_sum_is_the_sum_of_the_frames_own_terms(gpu, dtype, shape, n):
    """float_ref.mixed inputs with NaN / Inf / 1e308 under the NULLs: every row's SUM inside the any-order bound of ITS frame's terms, with the exact class for
    NaN / +-Inf — a NaN or an Inf before the frame must not reach it"""
    for nullable in (True, False):
        p, o, b, c = float_sum_case(8, n, shape, dtype, nullable)
        w = gpu.Window([to_gpu(gpu, p)], [to_gpu(gpu, o)])
        check_aggregates(gpu, w, b, c, to_gpu(gpu, c), FLOAT_FRAMES, (W.SUM, W.COUNT), (shape, nullable))


def test_float_sum_after_a_nan_and_a_huge_term(gpu):
    p, o, vals, f = W.poison_case()
    n = len(vals)
    w = gpu.Window([to_gpu(gpu, p)], [to_gpu(gpu, o)])
    b = W.boundaries([p], [o], n)
    c = R.KeyCol("f64", vals)
    got, valid = w.aggregate(W.SUM, to_gpu(gpu, c), gframe(gpu, f))
    check(nullable_list(got, valid), W.aggregate(W.SUM, b, vals, None, f, "f64"), "f64", W.SUM, "poison")
    assert as_list(got[4:8]) == [4.0, 6.0, 8.0, 10.0]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_float_min_max(gpu, dtype):
    """OrderedFloat: a NaN is the largest value, -0.0 equals +0.0; +-DBL_MAX, subnormals and both infinities among the inputs"""
    for shape, n in (("mixed", 20_011), ("long", 4097), ("each", 65)):
        w, b = window_of(gpu, 9, n, shape)
        vals, valid = W.float_values(np.random.default_rng([63, n]), n, R.FLOAT_KINDS[dtype], for_sum=False)
        c = R.KeyCol(dtype, vals, valid)
        check_aggregates(gpu, w, b, c, to_gpu(gpu, c), FLOAT_FRAMES, (W.MIN, W.MAX), shape)


# ---- one long partition: the walk's two levels of partials and a scan whose carry kernel owns several tiles per thread -------------
# Frames whose start moves and whose end is far away. Row i's frame [i, n) is folded from single rows up to the next multiple of 256,
# per-256-row partials up to the next multiple of 65,536, per-65,536-row partials, and the same again downwards.
MOVING_START_FAR_END = [W.Frame(W.ROWS, W.CURRENT_ROW, W.UNBOUNDED_FOLLOWING), W.Frame(W.ROWS, (W.FOLLOWING, 1), (W.FOLLOWING, W.HUGE)),
                        W.Frame(W.RANGE, W.CURRENT_ROW, W.UNBOUNDED_FOLLOWING)]
PEAK, VALLEY = 100_000, 165_000       # inside the second and the third run of 65,536 rows


def long_partition(gpu, n):
    """no partition key: n rows are one partition; an order key with ties for the RANGE frame"""
    o = R.KeyCol("i64", np.cumsum(np.random.default_rng([81, n]).random(n) < 0.4).astype(np.int64))
    return gpu.Window([], [to_gpu(gpu, o)], n=n), W.boundaries_fast([], [o], n)


def peak_and_valley(n, kind):
    """the only MAX of the rows after PEAK's run begins is at PEAK and the only MIN at VALLEY, so every frame that starts before their
    runs of 65,536 rows has its answer in a second-level partial and nowhere else; NULLs with something loud under them"""
    assert n > VALLEY + 20_000
    i = np.arange(n, dtype=np.int64)
    v = -np.abs(i - PEAK) - 100 * np.maximum(0, 20_000 - np.abs(i - VALLEY))
    valid = np.random.default_rng([83, n]).random(n) < 0.7
    valid[[PEAK, VALLEY]] = True
    if kind == "i64":
        loud = np.where(i % 2 == 0, np.iinfo(np.int64).max, np.iinfo(np.int64).min)
        return R.KeyCol("i64", np.where(valid, v, loud), valid)
    loud = np.array([np.nan, np.inf, -np.inf, 1e308])[i % 4]
    return R.KeyCol("f64", np.where(valid, v.astype(np.float64), loud), valid)


@pytest.mark.parametrize("frame", range(len(MOVING_START_FAR_END)))
@pytest.mark.parametrize("kind", ["i64", "f64"])
def test_long_partition_min_max_reads_the_second_level_partials(gpu, kind, frame):
    n = 200_003
    w, b = long_partition(gpu, n)
    c = peak_and_valley(n, kind)
    check_aggregates(gpu, w, b, c, to_gpu(gpu, c), [MOVING_START_FAR_END[frame]], (W.MIN, W.MAX), ("long partition", n))


@pytest.mark.parametrize("frame", range(len(MOVING_START_FAR_END)))
def test_long_partition_float_sum_reads_the_second_level_partials(gpu, frame):
    """terms of one magnitude, so that one term lost or taken twice anywhere in a frame leaves float_ref.sum_ok's bound by orders of magnitude;
    a NaN and an Inf before almost every frame, NaN / Inf / 1e308 under the NULLs"""
    n = 140_001
    assert n <= F.MAX_SUM_ROWS
    w, b = long_partition(gpu, n)
    rng = np.random.default_rng([85, n])
    vals, valid = rng.uniform(-1.0, 1.0, n), rng.random(n) < 0.7
    vals[5], vals[20] = np.nan, np.inf
    valid[[5, 20]] = True
    vals = np.where(valid, vals, np.array([np.nan, np.inf, -np.inf, 1e308])[np.arange(n) % 4])
    c = R.KeyCol("f64", vals, valid)
    check_aggregates(gpu, w, b, c, to_gpu(gpu, c), [MOVING_START_FAR_END[frame]], (W.SUM,), ("long partition", n))


def test_partition_of_more_than_a_million_rows(gpu):
    """more than 1024 tiles of 1024 rows: the one workgroup that carries the tile folds of a MIN / MAX scan owns two tiles per thread,
    and PEAK / VALLEY have to reach every later tile; the walk reads 16 second-level partials"""
    n = 1_100_003
    w, b = long_partition(gpu, n)
    c = peak_and_valley(n, "i64")
    check_aggregates(gpu, w, b, c, to_gpu(gpu, c), [RUNNING, MOVING_START_FAR_END[0]], (W.MIN, W.MAX), ("long partition", n))


# ---- Decimal128 -----------------------------------------------------------------------------------------------------------------
def test_dec128_inside_and_outside_the_gate(gpu):
    n = 20_011
    w, b = window_of(gpu, 10, n, "mixed")
    rng = np.random.default_rng(67)
    vals = [int(x) * (10 ** 21 + 3) for x in rng.integers(-10 ** 12, 10 ** 12, n)]          # |x| < 10^34: 3079 rows of a partition stay below 10^38
    c = R.KeyCol("dec128", vals, rng.random(n) < 0.7)
    assert int((b[1] - b[0]).max()) * 10 ** 34 < 10 ** 38
    gc = to_gpu(gpu, c)
    check_aggregates(gpu, w, b, c, gc, W.FRAMES[::3] + W.HUGE_FRAMES[:2], (W.COUNT, W.SUM, W.MIN, W.MAX), "dec128")
    # two terms of 9 * 10^37 in one partition: sum |x| leaves 10^38 - 1, although every frame of one row would fit
    big = list(vals)
    at = int(np.nonzero((b[1] - b[0]) >= 2)[0][0])
    big[at], big[at + 1] = 9 * 10 ** 37, -9 * 10 ** 37
    gbig = gpu.Column.decimal128(big, 38, 0)
    with pytest.raises(T.DbhipError) as e:
        w.aggregate(W.SUM, gbig, gframe(gpu, W.Frame(W.ROWS, W.CURRENT_ROW, W.CURRENT_ROW)))
    assert e.value.code == T.ERR_UNSUPPORTED
    # ... MIN / MAX have no gate, and the next SUM on the stream works
    cb = R.KeyCol("dec128", big)
    check_aggregates(gpu, w, b, cb, gbig, [RUNNING], (W.MIN, W.MAX), "dec128 extremes")
    check_aggregates(gpu, w, b, c, gc, [RUNNING], (W.SUM,), "dec128 after a refusal")
    # precision <= 18 in the wide storage class: no gate is needed
    small = gpu.Column.decimal128([v % 1000 for v in vals], 18, 0)
    got, valid = w.aggregate(W.SUM, small, gframe(gpu, RUNNING))
    check(nullable_list(got, valid), W.aggregate_fast(W.SUM, b, [v % 1000 for v in vals], None, RUNNING, "dec128"), "dec128", W.SUM)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def refused(code, fn, *args, **kw):
    with pytest.raises(T.DbhipError) as e:
        fn(*args, **kw)
    assert e.value.code == code, (e.value.code, code, args)


def test_refusals_leave_the_stream_usable(gpu):
    n = 4097
    p, o = W.layout(11, n, "mixed")
    gp, go = to_gpu(gpu, p), to_gpu(gpu, o)
    w = gpu.Window([gp], [go])
    b = W.boundaries_fast([p], [o], n)
    c = R.KeyCol("i64", *W.int_values(np.random.default_rng(71), n, "i64"))
    gc = to_gpu(gpu, c)

    def still_works():
        assert np.array_equal(w.rank(W.DENSE_RANK), W.rank_fast(W.DENSE_RANK, b))
        check_aggregates(gpu, w, b, c, gc, [RUNNING], (W.SUM,), "after a refusal")

    for f, code in W.REFUSED_FRAMES:
        refused(code, w.aggregate, W.SUM, gc, gframe(gpu, f))
        refused(code, w.aggregate, W.COUNT, None, gframe(gpu, f))
        refused(code, w.value, W.FIRST_VALUE, gc, gframe(gpu, f))
        still_works()
    ok = gframe(gpu, RUNNING)
    refused(T.ERR_INVALID, w.value, W.NTH_VALUE, gc, ok, 0)
    refused(T.ERR_INVALID, w.value, W.NTH_VALUE, gc, ok, -3)
    refused(T.ERR_INVALID, w.value, 3, gc, ok)
    refused(T.ERR_INVALID, w.rank, W.NTILE, 0)
    refused(T.ERR_INVALID, w.rank, 6)
    still_works()
    rng = np.random.default_rng(73)
    d256, bools, strs = to_gpu(gpu, value_column(rng, n, "dec256")), to_gpu(gpu, R.make_col(rng, n, "bool", True)), to_gpu(gpu, R.make_col(rng, n, "lstr", True))
    refused(T.ERR_UNSUPPORTED, w.aggregate, W.SUM, d256, ok)
    for col in (d256, bools, strs):
        refused(T.ERR_UNSUPPORTED, w.aggregate, W.MIN, col, ok)
        refused(T.ERR_UNSUPPORTED, w.aggregate, W.MAX, col, ok)
    refused(T.ERR_UNSUPPORTED, w.shift, strs, 1, strs)                      # a String default
    refused(T.ERR_INVALID, w.shift, gc, 1, bools)                           # a default of another type
    still_works()
    refused(T.ERR_UNSUPPORTED, gpu.Window, [d256], [go])                     # not a sort key type
    refused(T.ERR_INVALID, gpu.Window, [gp] * 9, [go])
    rows = T.WindowRows()
    rows.n, rows.part_start, rows.part_end, rows.peer_start, rows.peer_end = 0, *([w.rows.part_start] * 4)
    import ctypes as C
    rc = T.lib().dbhip_window_bounds(None, 0, None, 0, C.c_int64(2 ** 32 - 1), C.byref(rows), None)
    assert rc == T.ERR_INVALID
    rows.n = 2 ** 32 - 1
    out = gpu.DeviceBuffer(64)
    assert T.lib().dbhip_window_rank(C.byref(rows), W.RANK, C.c_uint64(0), C.c_void_p(out.ptr), None) == T.ERR_INVALID
    still_works()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_sort_then_window_against_sqlite(gpu):
    """200,000 unsorted rows -> dbhip_sort_perm + dbhip_take_block -> Window: rank, a running SUM(i64) and lag(1) equal sqlite3's answer
    for the same SQL (ORDER BY o, id makes the row order total; sqlite puts NULLs first in ascending order)"""
    n = 200_000
    rng = np.random.default_rng(79)
    pv, pvalid = rng.integers(0, 300, n).astype(np.int64), rng.random(n) < 0.97
    ov, ovalid = rng.integers(0, 50, n).astype(np.int64), rng.random(n) < 0.9
    ids = rng.permutation(n).astype(np.int64)
    vv, vvalid = rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64), rng.random(n) < 0.8
    cols = [gpu.Column.from_numpy(pv, validity=pvalid), gpu.Column.from_numpy(ov, validity=ovalid), gpu.Column.from_numpy(ids), gpu.Column.from_numpy(vv, validity=vvalid)]
    perm, m = gpu.sort_perm_device(cols[:3], nulls_first=[1, 1, 1])
    assert m == n
    sp, so, sid, sv = gpu.take_block(cols, perm, n)
    w = gpu.Window([sp], [so, sid])
    rank = w.rank(W.RANK)
    run, run_valid = w.aggregate(W.SUM, sv, gframe(gpu, RUNNING))
    lag, lag_valid = w.shift(sv, -1)
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (id INTEGER, p INTEGER, o INTEGER, v INTEGER)")
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?)", zip(ids.tolist(), nullable_list(pv, pvalid), nullable_list(ov, ovalid), nullable_list(vv, vvalid)))
    exp = con.execute("SELECT id, rank() OVER w, sum(v) OVER (w ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW), lag(v, 1) OVER w FROM t "
                      "WINDOW w AS (PARTITION BY p ORDER BY o, id) ORDER BY p, o, id").fetchall()
    e_id, e_rank, e_run, e_lag = (list(x) for x in zip(*exp))
    assert sid.to_numpy().tolist() == e_id
    assert rank.tolist() == e_rank
    assert nullable_list(run, run_valid) == e_run
    assert nullable_list(lag, lag_valid) == e_lag


# ---- the bytes past an inline value, and long values in a second buffer (tests/strview_cases.py) --------------------------------------
def test_string_keys_ignore_the_bytes_past_an_inline_value(gpu):
    """the shared String column, sorted, as partition key and as order key, with clean and with 0xFF padding: the reference's four
    arrays both times (equal long values lie in different buffers)"""
    from tests import strview_cases as S
    vals = sorted(S.values())
    p = S.build(gpu, vals)
    half = [v[:len(v) // 2] for v in vals]             # a coarser partition key: partitions of several peer groups
    q = S.build(gpu, half)
    exp = W.boundaries([R.KeyCol("lstr", half)], [R.KeyCol("lstr", vals)], S.N)
    assert len(set(exp[0])) > 1 and len(set(exp[2])) > len(set(exp[0])) and len(set(exp[2])) < S.N
    for (name, part), (_, order) in zip(q.both(), p.both()):
        got = gpu.Window([part], [order]).bounds()
        for g, e in zip(got, exp):
            assert g.tolist() == list(e), name
