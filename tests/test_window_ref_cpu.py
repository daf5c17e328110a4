"""CPU: tests/window_ref.py — the reference the GPU window tests assert against — is held to three things here. Its loops equal its
numpy twins on the shared cases; its loops equal sqlite3's window functions on nullable integer data (all 38 legal frames x COUNT / SUM /
MIN / MAX, the rank family, ntile with 1 .. 1000 buckets, lag / lead with and without a default, first / last / nth value); and the
shared cases reject six wrong implementations (negative controls, as in tests/test_sort_ref_cpu.py). One test checks that the five
window symbols are declared, exported and bound."""
import math
import os
import re
import sqlite3
import subprocess

import numpy as np
import pytest

from tests import float_ref as F
from tests import sort_ref as R
from tests import window_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_SYMBOLS = ["dbhip_window_bounds", "dbhip_window_rank", "dbhip_window_shift", "dbhip_window_value", "dbhip_window_aggregate"]


def test_window_symbols_are_exported():
    from databend_amd import _lib
    header = open(os.path.join(ROOT, "include", "dbhip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name in WINDOW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert re.search(r"\bT " + name + r"$", exported, flags=re.M), name
        assert name in _lib.SYMBOLS, name
    assert _lib.WindowRows and _lib.WindowFrame
    from databend_amd import device
    assert device.Window and device.WindowFrame


# ---- the hand-written case ------------------------------------------------------------------------------------------------------
def hand_case():
    nan2 = np.array([0xFFF8000000000123], dtype=np.uint64).view(np.float64)[0]
    pk = R.KeyCol("f64", np.array([-0.0, 0.0, 0.0, 1.5, 1.5, np.nan, nan2, np.nan, 1.0, 2.0, np.nan, -0.0]), np.array([1] * 8 + [0] * 4, bool))
    ok = R.KeyCol("i32", np.array([1, 1, 2, 7, 7, 3, 3, 99, 4, 4, 5, 9], dtype=np.int32), np.array([1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0], bool))
    v = np.arange(1, 13, dtype=np.int64)
    valid = np.array([1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1], bool)
    return pk, ok, v, valid


def test_hand_written_expectations():
    """12 rows: -0.0 and +0.0 are one partition, the three NaNs (two payloads) one, the four NULL keys one whatever lies under them;
    NULL order keys are peers of each other"""
    pk, ok, v, valid = hand_case()
    for bounds in (W.boundaries, W.boundaries_fast):
        b = tuple(list(map(int, x)) for x in bounds([pk], [ok], 12))
        assert b[0] == [0, 0, 0, 3, 3, 5, 5, 5, 8, 8, 8, 8]
        assert b[1] == [3, 3, 3, 5, 5, 8, 8, 8, 12, 12, 12, 12]
        assert b[2] == [0, 0, 2, 3, 3, 5, 5, 7, 8, 8, 10, 10]
        assert b[3] == [2, 2, 3, 5, 5, 7, 7, 8, 10, 10, 12, 12]
    assert W.rank(W.RANK, b) == [1, 1, 3, 1, 1, 1, 1, 3, 1, 1, 3, 3]
    assert W.rank(W.DENSE_RANK, b) == [1, 1, 2, 1, 1, 1, 1, 2, 1, 1, 2, 2]
    assert W.rank(W.ROW_NUMBER, b) == [1, 2, 3, 1, 2, 1, 2, 3, 1, 2, 3, 4]
    assert W.rank(W.CUME_DIST, b) == [2 / 3, 2 / 3, 1.0, 1.0, 1.0, 2 / 3, 2 / 3, 1.0, 0.5, 0.5, 1.0, 1.0]
    assert W.rank(W.PERCENT_RANK, b) == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 2 / 3, 2 / 3]
    assert W.rank(W.NTILE, b, 2) == [1, 1, 2, 1, 2, 1, 1, 2, 1, 1, 2, 2]
    running = W.Frame(W.ROWS, W.UNBOUNDED_PRECEDING, W.CURRENT_ROW)
    assert W.aggregate(W.SUM, b, v, valid, running) == [1, 3, 6, 4, 4, 6, 13, 21, None, 10, 21, 33]
    assert W.aggregate(W.SUM, b, v, valid, W.Frame(W.RANGE, W.UNBOUNDED_PRECEDING, W.CURRENT_ROW)) == [3, 3, 6, 4, 4, 13, 13, 21, 10, 10, 33, 33]
    assert W.aggregate(W.COUNT, b, v, valid, running) == [1, 2, 3, 1, 1, 1, 2, 3, 0, 1, 2, 3]
    assert W.aggregate(W.COUNT, b, None, None, W.Frame(W.ROWS, (W.PRECEDING, 1), (W.FOLLOWING, 1))) == [2, 3, 2, 2, 2, 2, 3, 2, 2, 3, 3, 2]
    assert W.aggregate(W.MAX, b, v, valid, W.Frame(W.ROWS, (W.FOLLOWING, 1), W.UNBOUNDED_FOLLOWING)) == [3, 3, None, None, None, 8, 8, None, 12, 12, 12, None]
    assert W.shift(b, v, valid, -1) == [None, 1, 2, None, 4, None, 6, 7, None, None, 10, 11]
    assert W.shift(b, v, valid, 2, ("scalar", -1)) == [3, -1, -1, -1, -1, 8, -1, -1, 11, 12, -1, -1]
    assert W.value(W.LAST_VALUE, b, v, valid, running) == [1, 2, 3, 4, None, 6, 7, 8, None, 10, 11, 12]
    assert W.value(W.NTH_VALUE, b, v, valid, W.Frame(W.ROWS, W.UNBOUNDED_PRECEDING, W.UNBOUNDED_FOLLOWING), 2) == [2, 2, 2, None, None, 7, 7, 7, 10, 10, 10, 10]


def test_frame_statuses():
    assert len(W.FRAMES) == 38 and sum(f.units == W.ROWS for f in W.FRAMES) == 34
    for f, code in W.REFUSED_FRAMES:
        assert W.frame_status(f) == code, f
    for f in W.FRAMES + W.HUGE_FRAMES:
        assert W.frame_status(f) == W.OK, f


# ---- loops == twins -------------------------------------------------------------------------------------------------------------
def as_list(x):
    return x.tolist() if isinstance(x, np.ndarray) else list(x)


@pytest.mark.parametrize("shape", W.SHAPES)
@pytest.mark.parametrize("n", [1, 2, 65, 1100, 2500])
def test_twin_boundaries_and_ranks(shape, n):
    p, o = W.layout(3, n, shape)
    b = W.boundaries([p], [o], n)
    bf = W.boundaries_fast([p], [o], n)
    assert [as_list(x) for x in bf] == [as_list(x) for x in b]
    rows = max(b[1][i] - b[0][i] for i in range(n))
    for kind in (W.ROW_NUMBER, W.RANK, W.DENSE_RANK, W.PERCENT_RANK, W.CUME_DIST):
        assert as_list(W.rank_fast(kind, b)) == W.rank(kind, b), kind
    for buckets in (1, 3, rows, rows + 1):
        assert as_list(W.rank_fast(W.NTILE, b, buckets)) == W.rank(W.NTILE, b, buckets), buckets


@pytest.mark.parametrize("kind", R.ALL_KINDS)
@pytest.mark.parametrize("nullable", [False, True])
def test_twin_boundaries_every_key_kind(kind, nullable):
    for n in (1, 2, 65, 700):
        cols = W.sorted_keys(40, n, [("u8", False, "low"), (kind, nullable, "low" if kind != "bool" else "pool"), (kind, nullable, "pool")])
        for parts, orders in (([cols[1]], [cols[2]]), ([cols[0]], [cols[1]]), ([cols[0], cols[1]], [cols[2]]), ([], [cols[1]]), ([cols[1]], [])):
            b, bf = W.boundaries(parts, orders, n), W.boundaries_fast(parts, orders, n)
            assert [as_list(x) for x in bf] == [as_list(x) for x in b]


def check_twin_aggregates(b, vals, valid, kind, frames, aggs=(W.COUNT, W.SUM, W.MIN, W.MAX)):
    for f in frames:
        for agg in aggs:
            why = W.same_results(W.aggregate_fast(agg, b, vals, valid, f, kind), W.aggregate(agg, b, vals, valid, f, kind), kind, agg)
            assert why == "", (f, agg, kind, why)
        assert W.aggregate_fast(W.COUNT, b, None, None, f) == W.aggregate(W.COUNT, b, None, None, f), f
        for vk, nth in ((W.FIRST_VALUE, 1), (W.LAST_VALUE, 1), (W.NTH_VALUE, 1), (W.NTH_VALUE, 3), (W.NTH_VALUE, 500)):
            assert W.same_results(W.value_fast(vk, b, vals, valid, f, nth), W.value(vk, b, as_list(vals), valid, f, nth), kind) == "", (f, vk, nth)


@pytest.mark.parametrize("shape", W.SHAPES)
def test_twin_aggregates_integers(shape):
    n = 600
    p, o = W.layout(5, n, shape)
    b = W.boundaries([p], [o], n)
    rng = np.random.default_rng(17)
    vals, valid = W.int_values(rng, n, "i64", nullable=True)
    check_twin_aggregates(b, vals, valid, "i64", W.FRAMES + W.HUGE_FRAMES)
    for kind in ("i8", "u16", "u64", "date", "dec64"):
        vals, valid = W.int_values(rng, n, kind, nullable=kind != "u64")
        check_twin_aggregates(b, vals, valid, kind, W.FRAMES[::5] + W.HUGE_FRAMES[:2])
    d128 = R.make_col(rng, n, "dec128", True)
    check_twin_aggregates(b, d128.values, d128.valid, "dec128", W.FRAMES[::7])


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_twin_aggregates_floats(dtype):
    n = 500
    p, o = W.layout(6, n, "mixed")
    b = W.boundaries([p], [o], n)
    rng = np.random.default_rng(19)
    vals, valid = W.float_values(rng, n, R.FLOAT_KINDS[dtype], for_sum=True)
    check_twin_aggregates(b, vals, valid, dtype, W.FRAMES[::3] + W.HUGE_FRAMES[:1])
    vals, valid = W.float_values(rng, n, R.FLOAT_KINDS[dtype], for_sum=False)
    check_twin_aggregates(b, vals, valid, dtype, W.FRAMES[1::4], aggs=(W.MIN, W.MAX))


def test_twin_shift():
    n = 900
    p, o = W.layout(7, n, "mixed")
    b = W.boundaries([p], [o], n)
    rng = np.random.default_rng(23)
    vals, valid = W.int_values(rng, n, "i32", nullable=True)
    dv, dvalid = W.int_values(rng, n, "i32", nullable=True)
    for off in (0, 1, -1, 2, -2, 70_000, -70_000, 5, -37):
        for d in (None, ("scalar", 77), ("scalar", None), ("column", dv, dvalid)):
            dl = d if d is None or d[0] == "scalar" else ("column", as_list(dv), dvalid)
            assert W.shift_fast(b, vals, valid, off, d) == W.shift(b, as_list(vals), valid, off, dl), (off, d and d[0])


# ---- loops == sqlite3 -----------------------------------------------------------------------------------------------------------
def sqlite_case(seed, n):
    """nullable integer data already in (p, o, id) order with NULLs first, the way sqlite orders ascending keys"""
    rng = np.random.default_rng(seed)
    sizes = [450, 1, 2, 3] + [int(x) for x in rng.integers(1, 30, 40)]
    p, o = [], []
    for k, s in enumerate(sizes):
        if len(p) >= n:
            break
        s = min(s, n - len(p))
        p += [None if k == 0 else k] * s
        oo = sorted(rng.integers(0, max(2, s // 3), s).tolist())
        nulls = int(rng.integers(0, 3)) if s > 2 else 0
        o += [None] * nulls + oo[nulls:]
    n = len(p)
    v = rng.integers(-40, 40, n).tolist()
    valid = rng.random(n) < 0.75
    v = [x if ok else None for x, ok in zip(v, valid)]
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (id INTEGER, p INTEGER, o INTEGER, v INTEGER)")
    rows = [(i, p[i], o[i], v[i]) for i in range(n)]
    con.executemany("INSERT INTO t VALUES (?, ?, ?, ?)", [rows[i] for i in rng.permutation(n).tolist()])

    def key(values):
        return R.KeyCol("i64", np.array([0 if x is None else x for x in values], dtype=np.int64), np.array([x is not None for x in values], bool))
    ids = R.KeyCol("i64", np.arange(n, dtype=np.int64))
    vals = np.array([0 if x is None else x for x in v], dtype=np.int64)
    return con, n, key(p), key(o), ids, vals, valid


@pytest.fixture(scope="module")
def sq():
    return sqlite_case(11, 700)


def query(con, sql):
    return [list(col) for col in zip(*con.execute(sql).fetchall())]


def test_sqlite_aggregates_over_every_legal_frame(sq):
    con, n, p, o, ids, vals, valid = sq
    peers = W.boundaries([p], [o], n)              # ORDER BY o: peer groups (RANGE frames do not depend on the order inside one)
    total = W.boundaries([p], [o, ids], n)         # ORDER BY o, id: a total order (ROWS frames need one)
    checked = 0
    for f in W.FRAMES:
        b = peers if f.units == W.RANGE else total
        order = "o" if f.units == W.RANGE else "o, id"
        got = query(con, f"SELECT count(v) OVER w, sum(v) OVER w, min(v) OVER w, max(v) OVER w, count(*) OVER w FROM t "
                         f"WINDOW w AS (PARTITION BY p ORDER BY {order} {f.sql()}) ORDER BY id")
        for k, agg in enumerate((W.COUNT, W.SUM, W.MIN, W.MAX)):
            assert W.aggregate(agg, b, vals, valid, f) == got[k], (f, agg)
            checked += 1
        assert W.aggregate(W.COUNT, b, None, None, f) == got[4], f
    assert checked == 152


def test_sqlite_rank_family_and_ntile(sq):
    con, n, p, o, ids, vals, valid = sq
    peers, total = W.boundaries([p], [o], n), W.boundaries([p], [o, ids], n)
    got = query(con, "SELECT rank() OVER w, dense_rank() OVER w, percent_rank() OVER w, cume_dist() OVER w FROM t WINDOW w AS (PARTITION BY p ORDER BY o) ORDER BY id")
    for k, kind in enumerate((W.RANK, W.DENSE_RANK, W.PERCENT_RANK, W.CUME_DIST)):
        assert W.rank(kind, peers) == got[k], kind              # (the two REAL columns bit for bit: one double division each)
    assert W.rank(W.ROW_NUMBER, total) == query(con, "SELECT row_number() OVER (PARTITION BY p ORDER BY o, id) FROM t ORDER BY id")[0]
    for buckets in range(1, 1001):
        assert W.rank(W.NTILE, total, buckets) == query(con, f"SELECT ntile({buckets}) OVER (PARTITION BY p ORDER BY o, id) FROM t ORDER BY id")[0], buckets


def test_sqlite_lag_lead_and_values(sq):
    con, n, p, o, ids, vals, valid = sq
    b = W.boundaries([p], [o, ids], n)
    vl = vals.tolist()
    for k in (0, 1, 2, 7, 449, 450, 70_000):
        for fn, off in (("lag", -k), ("lead", k)):
            w = "OVER (PARTITION BY p ORDER BY o, id)"
            assert W.shift(b, vl, valid, off) == query(con, f"SELECT {fn}(v, {k}) {w} FROM t ORDER BY id")[0], (fn, k)
            assert W.shift(b, vl, valid, off, ("scalar", -99)) == query(con, f"SELECT {fn}(v, {k}, -99) {w} FROM t ORDER BY id")[0], (fn, k)
            assert W.shift(b, vl, valid, off, ("column", [2 * x for x in vl], valid)) == query(con, f"SELECT {fn}(v, {k}, 2 * v) {w} FROM t ORDER BY id")[0], (fn, k)
    for f in W.FRAMES:
        if f.units == W.RANGE:
            continue                                    # (first / last over peers would depend on the order inside a peer group)
        got = query(con, f"SELECT first_value(v) OVER w, last_value(v) OVER w, nth_value(v, 1) OVER w, nth_value(v, 3) OVER w, nth_value(v, 401) OVER w FROM t "
                         f"WINDOW w AS (PARTITION BY p ORDER BY o, id {f.sql()}) ORDER BY id")
        for k, (vk, nth) in enumerate(((W.FIRST_VALUE, 1), (W.LAST_VALUE, 1), (W.NTH_VALUE, 1), (W.NTH_VALUE, 3), (W.NTH_VALUE, 401))):
            assert W.value(vk, b, vl, valid, f, nth) == got[k], (f, vk, nth)


# ---- negative controls: the shared cases reject wrong implementations -------------------------------------------------------------
RUNNING = W.Frame(W.ROWS, W.UNBOUNDED_PRECEDING, W.CURRENT_ROW)
CONTROL_N = 8 * W.TILE + 1


def tiled_running_sum(vals, valid, ps, tile, bug=None):
    """a running SUM the way a device computes it: folds per tile, a carry per tile, then the rows of a tile. `bug`: 'no_reset_at_tile_start' (the
    carry is added to a tile whose first row begins a partition) | 'carry_lost' (a tile inherits from the tile before it only)"""
    n = len(vals)
    nt = (n + tile - 1) // tile
    fold, has_head = [0] * nt, [False] * nt
    for t in range(nt):
        for i in range(t * tile, min(n, (t + 1) * tile)):
            if ps[i] == i:
                fold[t], has_head[t] = 0, True
            if valid[i]:
                fold[t] += int(vals[i])
    carry = [0] * nt
    for t in range(1, nt):
        carry[t] = fold[t - 1] if has_head[t - 1] or bug == "carry_lost" else carry[t - 1] + fold[t - 1]
    out, cnt = [], 0
    for t in range(nt):
        run = carry[t]
        for i in range(t * tile, min(n, (t + 1) * tile)):
            if ps[i] == i:
                cnt = 0
                if not (bug == "no_reset_at_tile_start" and i == t * tile):
                    run = 0
            if valid[i]:
                run += int(vals[i])
                cnt += 1
            out.append(run if cnt else None)
    return out


def control_inputs(shape):
    p, o = W.layout(9, CONTROL_N, shape)
    b = W.boundaries_fast([p], [o], CONTROL_N)
    vals, valid = W.int_values(np.random.default_rng(29), CONTROL_N, "i64", nullable=True, small=True)
    return b, vals, valid


def rejecting_shapes(wrong):
    """the shapes on which `wrong(b, vals, valid)` differs from the reference's running SUM"""
    out = []
    for shape in W.SHAPES:
        b, vals, valid = control_inputs(shape)
        exp = W.aggregate_fast(W.SUM, b, vals, valid, RUNNING)
        assert tiled_running_sum(vals, valid, b[0], W.TILE) == exp, shape          # the tiled scan itself is right
        if wrong(b, vals, valid) != exp:
            out.append(shape)
    return out


def test_control_scan_that_does_not_reset_at_a_head_on_a_tile_start():
    assert "tile_heads" in rejecting_shapes(lambda b, vals, valid: tiled_running_sum(vals, valid, b[0], W.TILE, "no_reset_at_tile_start"))


def test_control_carry_lost_over_more_than_two_tiles():
    got = rejecting_shapes(lambda b, vals, valid: tiled_running_sum(vals, valid, b[0], W.TILE, "carry_lost"))
    assert "one" in got and "long" in got and "tile_heads" in got


def test_control_rank_computed_as_dense_rank():
    rejected = 0
    for shape in W.SHAPES:
        p, o = W.layout(3, 2500, shape)
        b = W.boundaries_fast([p], [o], 2500)
        rejected += as_list(W.rank_fast(W.DENSE_RANK, b)) != as_list(W.rank_fast(W.RANK, b))
    assert rejected >= 3


def test_control_range_frame_resolved_as_rows():
    b, vals, valid = control_inputs("mixed")
    for f in W.FRAMES:
        if f.units == W.RANGE and W.CURRENT_ROW in (f.sk, f.ek):
            as_rows = W.Frame(W.ROWS, (f.sk, f.so), (f.ek, f.eo))
            assert W.aggregate_fast(W.SUM, b, vals, valid, as_rows) != W.aggregate_fast(W.SUM, b, vals, valid, f), f


def test_control_float_sum_by_prefix_difference():
    p, o, vals, f = W.poison_case()
    n = len(vals)
    b = W.boundaries([p], [o], n)
    exp = W.aggregate(W.SUM, b, vals, None, f, "f64")
    own = [sum(float(vals[j]) for j in range(*W.frame_of(f, i, b[0][i], b[1][i], b[2][i], b[3][i]))) for i in range(n)]
    assert W.same_results(own, exp, "f64", W.SUM) == ""
    prefix = np.concatenate([[0.0], np.cumsum(vals)])
    diff = [float(prefix[hi] - prefix[lo]) for lo, hi in (W.frame_of(f, i, b[0][i], b[1][i], b[2][i], b[3][i]) for i in range(n))]
    assert all(math.isnan(d) for d in diff[3:]) and W.same_results(diff, exp, "f64", W.SUM) != ""
    # without the NaN the 1e200 still cancels the small terms away
    vals2 = vals.copy()
    vals2[1] = 2.0
    exp2 = W.aggregate(W.SUM, b, vals2, None, f, "f64")
    prefix2 = np.concatenate([[0.0], np.cumsum(vals2)])
    diff2 = [float(prefix2[min(i + 1, n)] - prefix2[max(i - 1, 0)]) for i in range(n)]
    assert W.same_results(diff2, exp2, "f64", W.SUM) != ""


def test_control_reading_the_value_under_a_null():
    b, vals, valid = control_inputs("mixed")
    loud = np.where(valid, vals, 10**6)
    for agg in (W.SUM, W.MIN, W.MAX):
        for f in (RUNNING, W.Frame(W.ROWS, (W.PRECEDING, 3), W.CURRENT_ROW)):
            assert W.aggregate_fast(agg, b, loud, None, f) != W.aggregate_fast(agg, b, loud, valid, f), (agg, f)
            assert W.aggregate_fast(agg, b, loud, valid, f) == W.aggregate_fast(agg, b, vals, valid, f), (agg, f)
    rng = np.random.default_rng(31)
    fv, fvalid = W.float_values(rng, len(vals), np.float64, for_sum=True)
    assert np.isnan(fv[~fvalid]).any() and np.isinf(fv[~fvalid]).any()
    got = W.aggregate_fast(W.SUM, b, fv, fvalid, RUNNING, "f64")
    quiet = np.where(fvalid, fv, 0.0)
    assert W.same_results(got, W.aggregate_fast(W.SUM, b, quiet, fvalid, RUNNING, "f64"), "f64", W.SUM) == ""
