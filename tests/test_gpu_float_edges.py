"""GPU: NaN, +-Inf, signed zeros, subnormals, +-MAX and real-valued floats through the hash aggregation (every path: row / generic
kernels, compact LDS tables, radix-partitioned, many groups, the fused few-groups kernel interpreted and run-time specialised, pushed-down
filters, the pipelined table, state transport), as GROUP BY keys, through dbhip_sum, and through the three float comparisons (dbhip_cmp,
dbhip_select_cmp, the expression interpreter and the kernels specialised from it). Every result is asserted against tests/float_ref.py —
never against another device path — under its two equivalences: same_value (exact up to the NaN payload and the sign among both zeros)
and sum_ok (the any-order bound gamma(n - 1) * sum|x| of n - 1 double additions). tests/test_float_edges_cpu.py checks that reference
against the C oracle and shows that the checker rejects float32 accumulation, fmin / fmax, masking by multiplication and the IEEE compare."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import float_ref as R

pytestmark = pytest.mark.gpu

FT = {np.dtype(np.float32): T.T_F32, np.dtype(np.float64): T.T_F64}
DTYPES = [np.float32, np.float64]
NULL_FILTER = [(False, False), (True, False), (True, True)]          # (nullable arguments, pushed-down filter)
IDS_NF = ["plain", "nullable", "nullable+filter"]


def fagg_stats():
    out = (C.c_uint64 * 3)()
    T.check(T.lib().dbhip_fagg_stats(out))
    return dict(jit=out[0], interpreted=out[1], pending=out[2])


def case_aggs(dtype, nullable):
    """float_ref.CASE_AGGS as aggregate descriptors: COUNT(*), SUM(i64), SUM(f), MIN(f), MAX(f)"""
    t, nul = FT[np.dtype(dtype)], 1 if nullable else 0
    return [(T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_I64, 0, 0, 0), (T.AGG_SUM, t, 0, 0, nul), (T.AGG_MIN, t, 0, 0, nul), (T.AGG_MAX, t, 0, 0, nul)]


def check_aggs(dtype):
    return [("count", None), ("sum", np.int64), ("sum", dtype), ("min", dtype), ("max", dtype)]


def assert_rows(rows, exp, key_dtypes, aggs):
    bad = R.mismatches(rows, exp, key_dtypes, aggs)
    assert bad == [], (len(bad), bad[:6])


def run_case(gpu, c, compact=True, pbits=None, blocks=1, dec128=False):
    """the case through plain add_block (with the case's filter Bitmap, if it has one) -> result rows"""
    dt = c["dtype"]
    t = FT[dt]
    aggs = case_aggs(dt, c["valid"] is not None) + ([(T.AGG_MIN, T.T_DEC128, 38, 0, 0)] if dec128 else [])
    g = gpu.GroupBy([T.T_I64], aggs, [0])
    T.check(T.lib().dbhip_groupby_debug_set_compact(g.h, C.c_int32(1 if compact else 0)))
    if pbits is not None:
        g.debug_set_partition_bits(pbits)
    n = c["n"]
    cuts = [n * b // blocks for b in range(blocks + 1)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v = None if c["valid"] is None else c["valid"][lo:hi]
        fcol = lambda name: gpu.Column.from_numpy(c[name][lo:hi], t, validity=v)     # noqa: E731
        args = [None, gpu.Column.from_numpy(c["i"][lo:hi]), fcol("fs"), fcol("fm"), fcol("fm")]
        if dec128:
            args.append(gpu.Column.decimal128(c["dec"][lo:hi], 38, 0))
        g.add_block([gpu.Column.from_numpy(c["key"][lo:hi])], args, hi - lo, filter=None if c["keep"] is None else gpu.Column.boolean(c["keep"][lo:hi]))
    rows = g.result()
    assert g.num_groups() == len(rows)
    g.destroy()
    return rows


def make_case(seed, n, card, dtype, nullable, filtered, kinds=R.KINDS):
    return R.agg_case(np.random.default_rng(seed), n, card, dtype, nullable, filtered, kinds)


def assert_planned_groups(c, exp):
    """every kind of group the plan promises is in the expected result, with what it promises"""
    for kind, j in c["plan"].items():
        e = exp[(j,)]
        assert e[0]["count"] == 1 if kind == "single" else e[0]["count"] >= 3, kind
        if kind == "all_null" and c["valid"] is not None:
            assert e[2]["count"] == 0
        if kind == "all_nan":
            assert e[3]["min"] != e[3]["min"] and e[2]["sum"][0] == "nan"
        if kind == "one_nan":
            assert e[3]["min"] == e[3]["min"] and e[4]["max"] != e[4]["max"]
        if kind == "both_inf":
            assert e[2]["sum"][0] == "nan" and e[3]["min"] == -np.inf and e[4]["max"] == np.inf
        if kind == "neg_zero":
            assert e[3]["strict_zero"]


# ---- aggregation: plain add_block through every kernel family ---------------------------------------------------------------------------
@pytest.mark.parametrize("nullable,filtered", NULL_FILTER, ids=IDS_NF)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dec128", [False, True], ids=["generic", "row path (Decimal128 MIN)"])
def test_row_path_and_generic_kernels(gpu, dtype, nullable, filtered, dec128):
    """compact kernels off, never partitioned; with a Decimal128 MIN beside the float aggregates the table aggregates on the row path only"""
    c = make_case(11, 20_000, 300, dtype, nullable, filtered)
    extra = ()
    if dec128:
        c["dec"] = [int(x) * 10**20 - 7 for x in np.random.default_rng(3).integers(-10**17, 10**17, c["n"])]
        extra = [("min", c["dec"], None)]
    exp = R.case_expected(c, extra_args=extra)
    assert_planned_groups(c, exp)
    rows = run_case(gpu, c, compact=False, pbits=-1, dec128=dec128, blocks=2)
    assert_rows(rows, exp, [np.int64], check_aggs(dtype) + ([("min", None)] if dec128 else []))


@pytest.mark.parametrize("nullable,filtered", NULL_FILTER, ids=IDS_NF)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,card", [(5000, 37), (60_000, 300), (120_000, 2500)])
def test_compact_lds_tables(gpu, dtype, nullable, filtered, n, card):
    c = make_case(n + card, n, card, dtype, nullable, filtered)
    exp = R.case_expected(c)
    assert_planned_groups(c, exp)
    assert_rows(run_case(gpu, c, blocks=2), exp, [np.int64], check_aggs(dtype))


@pytest.mark.parametrize("nullable,filtered", NULL_FILTER, ids=IDS_NF)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("compact", [True, False], ids=["compact", "generic"])
@pytest.mark.parametrize("pbits", [4, 11])
def test_radix_partitioned(gpu, dtype, nullable, filtered, pbits, compact):
    """16 and 2048 partitions forced, three blocks so that the states of later blocks merge into existing ones"""
    c = make_case(pbits, 90_000, 5000, dtype, nullable, filtered)
    exp = R.case_expected(c)
    assert_rows(run_case(gpu, c, compact=compact, pbits=pbits, blocks=3), exp, [np.int64], check_aggs(dtype))


@pytest.mark.parametrize("nullable,filtered", [(False, False), (True, True)], ids=["plain", "nullable+filter"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_many_groups(gpu, dtype, nullable, filtered):
    """about one group per row: 200 000 rows, 150 000 key values"""
    c = make_case(77, 200_000, 150_000, dtype, nullable, filtered)
    exp = R.case_expected(c)
    assert len(exp) > 60_000
    assert_rows(run_case(gpu, c), exp, [np.int64], check_aggs(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sums_of_one_magnitude_stay_inside_the_bound(gpu, monkeypatch, tmp_path, dtype):
    """20 000 values N(0, 1000^2) per group: the case on which float32 accumulation misses the bound by orders of magnitude (CPU module)"""
    monkeypatch.setenv("DBHIP_JIT_CACHE_DIR", str(tmp_path))
    c = R.binade_case(np.random.default_rng(5), dtype=dtype)
    exp = R.case_expected(c)
    for compact, pbits in ((True, None), (False, -1), (True, 4)):
        assert_rows(run_case(gpu, c, compact=compact, pbits=pbits), exp, [np.int64], check_aggs(dtype))
    rows, _ = run_fused(gpu, c, "empty", False)
    assert_rows(rows, exp, [np.int64], check_aggs(dtype))


# ---- aggregation: the fused few-groups kernel -------------------------------------------------------------------------------------------
FEW_A = ("all_nan", "one_nan", "pos_inf", "both_inf", "neg_zero", "both_zero")          # + 2 ordinary groups = 8
FEW_B = ("subnormal", "all_null", "single", "one_nan", "all_nan")                       # + 3 ordinary groups = 8


def map_column(c):
    """x * 0.5 + y as the reference's evaluator computes it: a Float64 column whatever the width of x and y (Float32 * Float32 and
    Float32 + Float32 are Float64 there, arithmetics_type.rs), one rounding per node — no fused multiply-add"""
    with np.errstate(all="ignore"):
        return c["fs"].astype(np.float64) * 0.5 + c["fy"].astype(np.float64)


def map_check_aggs(dtype):
    return [("count", None), ("sum", np.int64), ("sum", np.float64), ("min", np.float64), ("max", dtype)]


def run_fused(gpu, c, program, prepare, filter_mode=None, rotate=False, pipelined_blocks=0, seed_rows=0):
    """the case through add_block_program -> (result rows in CASE_AGGS order, the register types); program: 'empty' (the arguments are
    input columns as they are) | 'map' (SUM and MIN over x * 0.5 + y); filter_mode: None | 'bitmap' | 'reg' (keep == 1 inside the program);
    rotate: COUNT(*) last (another table layout, hence another kernel shape); pipelined_blocks: that many add_block_program calls on a
    pipelined table, one checkpoint; seed_rows: the first rows go through plain add_block — PREPARE compiles the 8-slot variant of the
    kernel only for a table that already holds more than four groups, and an eight-group block makes the 4-slot variant give up"""
    dt, n = c["dtype"], c["n"]
    t = FT[dt]
    aggs = case_aggs(dt, c["valid"] is not None)
    if program == "map":
        aggs[2], aggs[3] = (T.AGG_SUM, T.T_F64) + aggs[2][2:], (T.AGG_MIN, T.T_F64) + aggs[3][2:]
    order = [1, 2, 3, 4, 0] if rotate else [0, 1, 2, 3, 4]
    g = gpu.GroupBy([T.T_I64], [aggs[o] for o in order], [0])
    if seed_rows:
        v = None if c["valid"] is None else c["valid"][:seed_rows]
        fcol = lambda name: gpu.Column.from_numpy(c[name][:seed_rows], t, validity=v)     # noqa: E731
        assert program == "empty"
        args = [None, gpu.Column.from_numpy(c["i"][:seed_rows]), fcol("fs"), fcol("fm"), fcol("fm")]
        g.add_block([gpu.Column.from_numpy(c["key"][:seed_rows])], [args[o] for o in order], seed_rows,
                    filter=gpu.Column.boolean(c["keep"][:seed_rows]) if filter_mode else None)
        assert g.num_groups() > 4
    if pipelined_blocks:
        g.set_pipelined(True)
    nb = max(pipelined_blocks, 1)
    cuts = [seed_rows + (n - seed_rows) * b // nb for b in range(nb + 1)]
    held = []

    def block(lo, hi):
        v = None if c["valid"] is None else c["valid"][lo:hi]
        cols = [gpu.Column.from_numpy(c["i"][lo:hi]), gpu.Column.from_numpy(c["fs"][lo:hi], t, validity=v), gpu.Column.from_numpy(c["fm"][lo:hi], t, validity=v),
                gpu.Column.from_numpy(c["fy"][lo:hi], t, validity=v)]
        if filter_mode == "reg":
            cols.append(gpu.Column.from_numpy(c["keep"][lo:hi].astype(np.int64)))
        p = gpu.ExprProgram(cols)
        freg = -1
        if filter_mode == "reg":
            freg = p.cmp(T.EX_EQ, p.load(4), p.const(1, T.T_I64))
        if program == "map":
            m = p.arith(T.EX_PLUS, p.arith(T.EX_MULTIPLY, p.load(1), p.const(0.5, t)), p.load(3))
            assert p.types[m] == T.T_F64
            regs = [None, ("input", 0), m, m, ("input", 2)]
        else:
            regs = [None, ("input", 0), ("input", 1), ("input", 2), ("input", 2)]
        keys = [gpu.Column.from_numpy(c["key"][lo:hi])]
        fb = gpu.Column.boolean(c["keep"][lo:hi]) if filter_mode == "bitmap" else None
        return keys, p, [regs[o] for o in order], freg, fb

    if prepare:
        assert filter_mode != "bitmap"                  # PREPARE has no Bitmap argument: that shape is compiled in the background only
        keys, p, regs, freg, fb = block(0, min(n, 64))
        g.prepare_program(keys, p, regs, filter_reg=freg)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        keys, p, regs, freg, fb = block(lo, hi)
        g.add_block_program(keys, p, regs, hi - lo, filter_reg=freg, filter=fb)
        held.append((keys, p, fb))                      # a pipelined table reads the blocks until the checkpoint
    if pipelined_blocks:
        assert g.checkpoint() == pipelined_blocks
    rows = g.result()
    g.destroy()
    back = [order.index(a) for a in range(5)]
    return [r[:1] + tuple(r[1 + b] for b in back) for r in rows], None


@pytest.mark.parametrize("nullable,filter_mode", [(False, None), (True, None), (True, "bitmap"), (True, "reg")], ids=["plain", "nullable", "nullable+filter", "nullable+filter_reg"])
@pytest.mark.parametrize("program", ["empty", "map"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_few_groups_kernel_interpreted_and_specialised(gpu, monkeypatch, tmp_path, dtype, program, nullable, filter_mode):
    """<= 8 groups through dbhip_groupby_add_block_program: first un-PREPAREd (the interpreting kernel: the code-object cache is an empty
    directory of this test, so nothing specialised can be found), then PREPAREd (the run-time specialised kernel), both against float_ref.
    Two group plans (no case holds nine kinds in eight groups); the second one runs on a rotated aggregate layout — a kernel shape of its
    own, so that its un-PREPAREd launch cannot find what the first one's background compile may have published meanwhile."""
    monkeypatch.setenv("DBHIP_JIT_CACHE_DIR", str(tmp_path))
    for kinds, rotate in ((FEW_A, False), (FEW_B, True)):
        c = make_case(len(kinds), 60_000, 8, dtype, nullable, filter_mode is not None, kinds)
        exp = R.case_expected(c, sum_col=map_column(c) if program == "map" else None)
        assert len(exp) == 8
        assert_planned_groups(c, exp) if program == "empty" else None
        s0 = fagg_stats()
        rows, _ = run_fused(gpu, c, program, False, filter_mode, rotate)
        s1 = fagg_stats()
        assert s1["interpreted"] > s0["interpreted"] and s1["jit"] == s0["jit"]
        assert_rows(rows, exp, [np.int64], map_check_aggs(dtype) if program == "map" else check_aggs(dtype))
        if filter_mode == "bitmap" or program == "map":
            continue
        rows, _ = run_fused(gpu, c, program, True, filter_mode, rotate, seed_rows=3000)
        s2 = fagg_stats()
        assert s2["jit"] > s1["jit"] and s2["interpreted"] == s1["interpreted"]
        assert_rows(rows, exp, [np.int64], check_aggs(dtype))


@pytest.mark.parametrize("nullable,filter_mode", [(False, None), (True, "reg")], ids=["plain", "nullable+filter_reg"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_float_map_specialised(gpu, monkeypatch, tmp_path, dtype, nullable, filter_mode):
    """SUM and MIN over x * 0.5 + y, PREPAREd: four groups (the 4-slot variant PREPARE compiles for an empty table), the kinds on which a
    fused multiply-add or a flushed subnormal would show (x * 0.5 is inexact exactly on odd subnormals)"""
    monkeypatch.setenv("DBHIP_JIT_CACHE_DIR", str(tmp_path))
    c = make_case(4, 40_000, 4, dtype, nullable, filter_mode is not None, ("subnormal", "one_nan", "both_inf", "neg_zero"))
    exp = R.case_expected(c, sum_col=map_column(c))
    assert len(exp) == 4
    s0 = fagg_stats()
    rows, _ = run_fused(gpu, c, "map", True, filter_mode)
    s1 = fagg_stats()
    assert s1["jit"] > s0["jit"] and s1["interpreted"] == s0["interpreted"]
    assert_rows(rows, exp, [np.int64], map_check_aggs(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pipelined_table(gpu, monkeypatch, tmp_path, dtype):
    """16 blocks of 65 536 rows queued on a pipelined table (PREPAREd: the blocks go several to a launch), one checkpoint; nullable
    arguments, the filter inside the program"""
    monkeypatch.setenv("DBHIP_JIT_CACHE_DIR", str(tmp_path))
    c = make_case(16, 16 * 65_536 + 4096, 8, dtype, True, True, FEW_A)
    exp = R.case_expected(c)
    s0 = fagg_stats()
    rows, _ = run_fused(gpu, c, "empty", True, "reg", pipelined_blocks=16, seed_rows=4096)
    assert fagg_stats()["jit"] > s0["jit"]
    assert_rows(rows, exp, [np.int64], check_aggs(dtype))


# ---- aggregation: state transport -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [False, True], ids=["plain", "nullable"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_state_transport_keeps_the_float_states(gpu, dtype, nullable):
    """two partial tables -> flush_state_block -> merge_state_block into a fresh table, and -> flush_serialized -> merge_serialized into
    another: the final tables under the same checks (an all-NaN MIN, whose encoded state equals the identity of an encoded MIN, survives;
    an all-NULL group stays NULL)"""
    c = make_case(21, 30_000, 300, dtype, nullable, False)
    exp = R.case_expected(c)
    assert_planned_groups(c, exp)
    t, n = FT[c["dtype"]], c["n"]
    aggs = case_aggs(dtype, nullable)

    def partial(lo, hi):
        g = gpu.GroupBy([T.T_I64], aggs, [0])
        v = None if c["valid"] is None else c["valid"][lo:hi]
        fcol = lambda name: gpu.Column.from_numpy(c[name][lo:hi], t, validity=v)     # noqa: E731
        g.add_block([gpu.Column.from_numpy(c["key"][lo:hi])], [None, gpu.Column.from_numpy(c["i"][lo:hi]), fcol("fs"), fcol("fm"), fcol("fm")], hi - lo)
        return g

    by_block, by_rows = gpu.GroupBy([T.T_I64], aggs, [0]), gpu.GroupBy([T.T_I64], aggs, [0])
    for lo, hi in ((0, n // 3), (n // 3, n)):
        p = partial(lo, hi)
        keys, states = p.flush_state_block()
        by_block.merge_state_block(keys, states, keys[0].n)
        by_rows.merge_serialized(p.flush_serialized())
    assert_rows(by_block.result(), exp, [np.int64], check_aggs(dtype))
    assert_rows(by_rows.result(), exp, [np.int64], check_aggs(dtype))


# ---- float GROUP BY keys ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second_key", [False, True], ids=["alone", "with an i64 key"])
@pytest.mark.parametrize("path", ["row", "compact", "partitioned", "few groups", "few groups specialised"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_float_keys_group_by_their_bit_pattern(gpu, monkeypatch, tmp_path, dtype, path, second_key):
    """+-0.0, two NaN payloads, +-Inf, subnormals and ordinary values as GROUP BY keys: the groups are the stored bit patterns (the oracle's
    row_match compares bytes; tests/test_float_edges_cpu.py holds that statement) — number of groups, key bits, COUNT(*), SUM(i64)"""
    monkeypatch.setenv("DBHIP_JIT_CACHE_DIR", str(tmp_path))
    few = path.startswith("few")
    c = R.key_case(np.random.default_rng(4), 40_000, dtype, few, second_key)
    kt = [FT[np.dtype(dtype)]] + ([T.T_I64] if second_key else [])
    g = gpu.GroupBy(kt, [(T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_I64, 0, 0, 0)], [0] * len(kt))
    keys = [gpu.Column.from_numpy(k, t) for k, t in zip(c["keys"], kt)]
    if few:
        p = gpu.ExprProgram([gpu.Column.from_numpy(c["i"])])
        s0 = fagg_stats()
        lo = 0
        if path.endswith("specialised"):      # (PREPARE compiles the 8-slot variant for a table that holds more than four groups)
            lo = 2000
            g.add_block([gpu.Column.from_numpy(k[:lo], t) for k, t in zip(c["keys"], kt)], [None, gpu.Column.from_numpy(c["i"][:lo])], lo)
            keys = [gpu.Column.from_numpy(k[lo:], t) for k, t in zip(c["keys"], kt)]
            p = gpu.ExprProgram([gpu.Column.from_numpy(c["i"][lo:])])
            g.prepare_program(keys, p, [None, ("input", 0)])
        g.add_block_program(keys, p, [None, ("input", 0)], c["n"] - lo)
        s1 = fagg_stats()
        if path.endswith("specialised"):
            assert s1["jit"] > s0["jit"] and s1["interpreted"] == s0["interpreted"]
        else:
            assert s1["interpreted"] > s0["interpreted"] and s1["jit"] == s0["jit"]
    else:
        T.check(T.lib().dbhip_groupby_debug_set_compact(g.h, C.c_int32(0 if path == "row" else 1)))
        g.debug_set_partition_bits({"row": -1, "compact": -1, "partitioned": 4}[path])
        half = c["n"] // 2
        for lo, hi in ((0, half), (half, c["n"])):
            g.add_block([gpu.Column.from_numpy(k[lo:hi], t) for k, t in zip(c["keys"], kt)], [None, gpu.Column.from_numpy(c["i"][lo:hi])], hi - lo)
    rows = g.result()
    assert len(rows) == len(c["exp"]) >= len(R.key_values(dtype, few))
    assert_rows(rows, c["exp"], [dtype] + ([np.int64] if second_key else []), [("count", None), ("sum", np.int64)])


# ---- dbhip_sum --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 100_003])
@pytest.mark.parametrize("dtype", DTYPES)
def test_column_sum_of_floats(gpu, dtype, n):
    """dbhip_sum's float branch (it honours the column's validity Bitmap: NULL rows add nothing, whatever lies under them): finite mixes
    inside the bound, the class of the sum with NaN / +Inf / -Inf / both infinities in the column, the same under NULL rows only"""
    rng = np.random.default_rng(n + 1)
    nan, inf = (R.NAN32, R.INF32) if dtype == np.float32 else (R.NAN64, R.INF64)
    fin = R.pool(dtype, True)
    fin = fin[np.isfinite(fin)]
    base = R.draws(rng, n, dtype)
    pick = rng.random(n) < 0.2
    base[pick] = fin[rng.integers(0, len(fin), int(pick.sum()))]
    for special in ([], [nan[1]], [inf[0]], [inf[1]], [inf[0], inf[1]], [nan[3], inf[0]]):
        for nullable in (False, True):
            x = base.copy()
            valid = rng.random(n) > 0.3 if nullable else np.ones(n, bool)
            pos = rng.permutation(n)[:len(special)]
            x[pos] = special[:len(pos)]
            valid[pos] = True
            hidden = np.flatnonzero(~valid)
            x[hidden] = np.concatenate([nan, inf])[rng.integers(0, 6, len(hidden))]
            got = gpu.column_sum(gpu.Column.from_numpy(x, FT[np.dtype(dtype)], validity=valid if nullable else None))
            exp = R.sum_expected(x[valid])
            assert R.sum_ok(got, exp), (special, nullable, got, exp, x[:4], valid[:4])
            if n >= 63:        # (the inputs are what they claim: one class per mix)
                want = "finite" if not special else "nan" if len(special) > 1 or special[0] != special[0] else "+inf" if special[0] > 0 else "-inf"
                assert exp[0] == want


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def cmp_operands(rng, dtype, n):
    """the cross product pool x pool as two columns (every special meets every other, in both operand positions) in a random order, cut or
    padded with mixed draws to n rows"""
    p = R.pool(dtype)
    a, b = np.repeat(p, len(p)), np.tile(p, len(p))
    order = rng.permutation(len(a))
    a, b = a[order][:n], b[order][:n]
    if n > len(a):
        a = np.concatenate([a, R.mixed(rng, n - len(a), dtype)])
        b = np.concatenate([b, R.mixed(rng, n - len(b), dtype)])
    return a, b


def bitmap_of(col, n):
    return np.unpackbits(col.data.to_numpy(np.uint8, (n + 7) // 8), bitorder="little")[:n].astype(bool)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 729, 4097])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cmp_every_special_against_every_other(gpu, dtype, n):
    """dbhip_cmp, all six operators: column - column (plain and with nullable operands: specials under the NULL rows, the result's validity
    the AND of the operands'), column - scalar and scalar - column with every pool value as the scalar; the Bitmap from of_cmp, bit for bit"""
    rng = np.random.default_rng(n)
    t = FT[np.dtype(dtype)]
    a, b = cmp_operands(rng, dtype, n)
    ga, gb = gpu.Column.from_numpy(a, t), gpu.Column.from_numpy(b, t)
    va, vb = rng.random(n) > 0.3, rng.random(n) > 0.3
    na, nb = gpu.Column.from_numpy(a, t, validity=va), gpu.Column.from_numpy(b, t, validity=vb)
    c3 = R.cmp3_array(a, b)
    for op, name in enumerate(R.CMP_OPS):
        exp = R.holds_array(name, c3)
        assert np.array_equal(bitmap_of(gpu.cmp(op, ga, gb, n), n), exp), name
        out = gpu.cmp(op, na, nb, n)
        assert np.array_equal(bitmap_of(out, n), exp) and np.array_equal(out.validity_numpy(), va & vb), name
    for s in R.pool(dtype):
        gs = gpu.Column.scalar(s, t)
        assert R.bits_of(gs.data.to_numpy(dtype, 1))[0] == R.bits_of(np.array([s]))[0]
        cs, sc = R.cmp3_array(a, [s]), R.cmp3_array([s], b)
        for op, name in enumerate(R.CMP_OPS):
            assert np.array_equal(bitmap_of(gpu.cmp(op, ga, gs, n), n), R.holds_array(name, cs)), (name, s)
            assert np.array_equal(bitmap_of(gpu.cmp(op, gs, gb, n), n), R.holds_array(name, sc)), (name, s)


@pytest.mark.parametrize("n", [1, 65, 4097])
@pytest.mark.parametrize("dtype", DTYPES)
def test_select_cmp_true_and_false_lists(gpu, dtype, n):
    """dbhip_select_cmp: the same operands over all rows and over an input selection, true list and false list, a scalar on either side,
    nullable operands (a NULL row does not pass: it is on the false list)"""
    rng = np.random.default_rng(n + 7)
    t = FT[np.dtype(dtype)]
    a, b = cmp_operands(rng, dtype, n)
    va = rng.random(n) > 0.3
    sel = np.flatnonzero(rng.random(n) < 0.6).astype(np.uint32)
    sel_dev = gpu.DeviceBuffer.from_numpy(np.concatenate([sel, np.zeros(16, np.uint32)]))
    ga, gb, na = gpu.Column.from_numpy(a, t), gpu.Column.from_numpy(b, t), gpu.Column.from_numpy(a, t, validity=va)
    p = R.pool(dtype)
    scalars = p[rng.permutation(len(p))[:6]] if n > 1 else p
    pairs = [(ga, gb, R.cmp3_array(a, b), None), (na, gb, R.cmp3_array(a, b), va)]
    for s in scalars:
        gs = gpu.Column.scalar(s, t)
        pairs += [(ga, gs, R.cmp3_array(a, [s]), None), (gs, gb, R.cmp3_array([s], b), None)]
    for x, y, c3, valid in pairs:
        for op, name in enumerate(R.CMP_OPS):
            exp = R.holds_array(name, c3) & (valid if valid is not None else True)
            for rows, dev, cnt in ((np.arange(n, dtype=np.uint32), None, n), (sel, sel_dev, len(sel))):
                if cnt == 0:
                    continue
                tl, k, fl = gpu.select_cmp(op, x, y, dev, cnt, want_false=True)
                assert k == int(exp[rows].sum()), name
                assert np.array_equal(tl.to_numpy(np.uint32, k), rows[exp[rows]]) and np.array_equal(fl.to_numpy(np.uint32, cnt - k), rows[~exp[rows]]), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_expression_compare_and_if(gpu, dtype):
    """ExprProgram.cmp through the interpreter: x > 5.0, x >= y, x == x, x != y over the pool's cross product, and IF on such a predicate
    (the chosen side comes out as stored: NaN stays NaN, the sign of a zero is kept)"""
    rng = np.random.default_rng(8)
    t, n = FT[np.dtype(dtype)], 4097
    x, y = cmp_operands(rng, dtype, n)
    cols = [gpu.Column.from_numpy(x, t), gpu.Column.from_numpy(y, t)]
    preds = predicates(x, y)
    for name, (build, exp) in preds.items():
        p = gpu.ExprProgram(cols)
        got = p.run(build(p, t), n=n)
        assert np.array_equal(got["values"], exp), name
        p = gpu.ExprProgram(cols)
        lx, ly = p.load(0), p.load(1)
        r = p.if_(build(p, t), lx, ly)
        out = p.run(r, n=n)["values"]
        want = np.where(exp, x, y)
        assert out.dtype == want.dtype and np.array_equal(np.isnan(out), np.isnan(want)), name
        ok = ~np.isnan(want)
        assert np.array_equal(R.bits_of(out[ok]), R.bits_of(want[ok])), name


def predicates(x, y):
    """name -> (builder of the predicate register in a program over [x, y, ...], the rows of_cmp admits)"""
    five = np.array([5.0], dtype=x.dtype)

    def gt5(p, t):
        return p.cmp(T.EX_GT, p.load(0), p.const(5.0, t))

    def gte(p, t):
        return p.cmp(T.EX_GTE, p.load(0), p.load(1))

    def eq_self(p, t):
        lx = p.load(0)
        return p.cmp(T.EX_EQ, lx, lx)

    def noteq(p, t):
        return p.cmp(T.EX_NOTEQ, p.load(0), p.load(1))

    return {"x > 5.0": (gt5, R.holds_array("gt", R.cmp3_array(x, five))), "x >= y": (gte, R.holds_array("gte", R.cmp3_array(x, y))),
            "x == x": (eq_self, R.holds_array("eq", R.cmp3_array(x, x))), "x != y": (noteq, R.holds_array("noteq", R.cmp3_array(x, y)))}


@pytest.mark.parametrize("pred", ["x > 5.0", "x >= y", "x == x", "x != y"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_float_predicate_as_the_filter_of_a_fused_aggregation(gpu, monkeypatch, tmp_path, dtype, pred):
    """the predicate as filter_reg of dbhip_groupby_add_block_program, interpreted and PREPAREd (the kernel specialised from the same
    text): the rows that reach the aggregate are exactly those of_cmp admits — COUNT(*) and SUM(i64) per group against float_ref"""
    monkeypatch.setenv("DBHIP_JIT_CACHE_DIR", str(tmp_path))
    rng = np.random.default_rng(12)
    t, n = FT[np.dtype(dtype)], 50_000
    x, y = cmp_operands(rng, dtype, n)
    key = rng.integers(0, 4, n).astype(np.int64)          # (four groups: the variant of the kernel PREPARE compiles for an empty table)
    i64 = rng.integers(-10**9, 10**9, n).astype(np.int64)
    build, keep = predicates(x, y)[pred]
    assert 0 < keep.sum() < n or pred == "x == x"
    exp = R.agg_expected([key], [None], [None, i64], [None, None], keep)
    aggs = [(T.AGG_COUNT, 0, 0, 0, 0), (T.AGG_SUM, T.T_I64, 0, 0, 0)]
    for prepare in (False, True):
        g = gpu.GroupBy([T.T_I64], aggs, [0])
        p = gpu.ExprProgram([gpu.Column.from_numpy(x, t), gpu.Column.from_numpy(y, t), gpu.Column.from_numpy(i64)])
        f = build(p, t)
        keys = [gpu.Column.from_numpy(key)]
        s0 = fagg_stats()
        if prepare:
            g.prepare_program(keys, p, [None, ("input", 2)], filter_reg=f)
        g.add_block_program(keys, p, [None, ("input", 2)], n, filter_reg=f)
        s1 = fagg_stats()
        assert (s1["jit"] > s0["jit"] and s1["interpreted"] == s0["interpreted"]) if prepare else (s1["interpreted"] > s0["interpreted"] and s1["jit"] == s0["jit"])
        assert_rows(g.result(), exp, [np.int64], [("count", None), ("sum", np.int64)])
        g.destroy()


@pytest.mark.parametrize("dtype", DTYPES)
def test_filter_select_and_take_do_not_canonicalise(gpu, dtype):
    """filter_select + take of a float column holding the pool: payloads and zero signs come out as they went in"""
    rng = np.random.default_rng(2)
    n = 10_007
    x = R.mixed(rng, n, dtype, p_pool=0.6)
    x[:len(R.pool(dtype))] = R.pool(dtype)
    keep = rng.random(n) < 0.5
    keep[:len(R.pool(dtype))] = True
    sel, k = gpu.filter_select(gpu.Column.boolean(keep))
    assert k == int(keep.sum())
    got = gpu.take(gpu.Column.from_numpy(x, FT[np.dtype(dtype)]), sel, k).to_numpy()
    assert got.dtype == x.dtype and np.array_equal(R.bits_of(got), R.bits_of(x[keep]))
