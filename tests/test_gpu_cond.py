"""GPU: the conditionals (include/dbhip.h a27: dbhip_case / dbhip_coalesce / dbhip_bool_logic through device.case_when, coalesce,
bool_logic and their wrappers) against tests/cond_ref.py, everything compared for equality — bits, bytes and views: the shared case list
(tests/cond_cases.py) for every one of the seventeen types; word and lane boundaries with guarded outputs; sixteen conditions and the
refusal of a seventeenth; scalars, NULL scalars without data, nullable scalars; sliced conditions, values and outputs
(tests/slice_cases.py); out_branch and the lazy-branch recipe; parity with ExprProgram.if_; Kleene logic against the truth tables and
against the dbhip_bitmap_binary composition; nullif / is_null; a plan of Q14's shape; the refusals."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import cond_cases as K
from tests import cond_ref as R
from tests import slice_cases as S

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SIZES_OF = {t: R.SIZE[t] for t in R.TYPES}
DEC = {T.T_DEC64: (15, 2), T.T_DEC128: (30, 4), T.T_DEC256: (60, 6)}
TABLES = (1, 2, 0)                                        # buffers per String argument, in turn


# ---- columns ----------------------------------------------------------------------------------------------------------------------------
def bitmap(gpu, bits, voff=0):
    """(DeviceBuffer, voff): the bits behind `voff` junk bits"""
    head = np.random.default_rng(voff).integers(0, 2, voff).astype(bool)
    return gpu.DeviceBuffer.from_numpy(gpu.pack_bits(np.concatenate([head, np.asarray(bits, dtype=bool)])))


def bool_col(gpu, rc, voff=0):
    col = gpu.Column.boolean(np.asarray(rc.values, dtype=bool))
    col.is_scalar = rc.scalar
    if rc.valid is not None:
        col.validity, col.voff = bitmap(gpu, rc.valid, voff), voff
    return col


def raw_col(gpu, typ, rc, voff=0, n_buffers=0):
    """a column of `typ` whose elements are rc.values' raw bytes ((rows, size) uint8). A String column gets a table of n_buffers made-up
    entries: the kernel copies tables and never reads a value byte."""
    p, s = DEC.get(typ, (0, 0))
    col = gpu.Column(typ, len(rc.values), gpu.DeviceBuffer.from_numpy(np.ascontiguousarray(rc.values).reshape(-1)), None, p, s, is_scalar=rc.scalar)
    if rc.valid is not None:
        col.validity, col.voff = bitmap(gpu, rc.valid, voff), voff
    if n_buffers:
        col.buffers = gpu.DeviceBuffer.from_numpy(np.arange(1, n_buffers + 1, dtype=np.uint64) * 0x1000 + len(rc.values))
        col.n_buffers = n_buffers
    return col


def as_views(raw):
    """random (n, 16) bytes shaped into views: lengths on both sides of 12, buffer indices 0 or 1 for the long ones"""
    v = np.ascontiguousarray(raw).view(np.uint32).reshape(-1, 4).copy()
    v[:, 0] = v[:, 0] % 25
    v[:, 2] = np.where(v[:, 0] > 12, v[:, 2] % 2, v[:, 2])
    return v.view(np.uint8).reshape(-1, 16)


def guarded(gpu, nbytes, lead=16):
    whole = gpu.DeviceBuffer.from_numpy(np.full(lead + nbytes + 64, GUARD, dtype=np.uint8))
    return whole, gpu.BorrowedBuffer(whole.ptr + lead, nbytes, keep=whole)


def guards_intact(whole, nbytes, lead=16):
    back = whole.to_numpy(np.uint8, lead + nbytes + 64)
    return (back[:lead] == GUARD).all() and (back[lead + nbytes:] == GUARD).all(), back[lead:lead + nbytes]


def run_select(gpu, typ, conds, vals, n, what, voffs=K.FETCH_OFFSETS, lead=16):
    """conds: Boolean Cols or None (a coalesce); vals: Cols of raw elements (Boolean Cols for T_BOOL). Runs the call with guarded
    outputs of its own and compares values, validity, branch and (Strings) the table with the reference."""
    size = SIZES_OF[typ]
    string = typ == T.T_STRING
    nbufs = [TABLES[j % 3] if string else 0 for j in range(len(vals))]
    if string:
        vals = [R.Col(as_views(v.values), v.valid, v.scalar) for v in vals]
    dconds = [bool_col(gpu, c, voffs[j % 5]) for j, c in enumerate(conds)] if conds is not None else None
    if typ == T.T_BOOL:
        dvals = [bool_col(gpu, v, voffs[(j + 1) % 5]) for j, v in enumerate(vals)]
    else:
        dvals = [raw_col(gpu, typ, v, voffs[(j + 3) % 5], nbufs[j]) for j, v in enumerate(vals)]
    words = (n + 63) // 64
    nd = n * size if size else words * 8
    w_out, out = guarded(gpu, nd, lead)
    w_val, val = guarded(gpu, words * 8)
    w_br, br = guarded(gpu, n, lead=13)
    if conds is not None:
        res = gpu.case_when(dconds, dvals, n, out=out, out_validity=val, out_branch=br)
        exp_branch = R.choose_case(conds, n)
    else:
        res = gpu.coalesce(*dvals, n=n, out=out, out_validity=val, out_branch=br)
        exp_branch = R.choose_coalesce(vals, n)
    ok1, data = guards_intact(w_out, nd, lead)
    ok2, vbytes = guards_intact(w_val, words * 8)
    ok3, branch = guards_intact(w_br, n, lead=13)
    assert ok1 and ok2 and ok3, (what, "a guard byte was written")
    assert (branch == exp_branch).all(), (what, "branch", np.nonzero(branch != exp_branch)[0][:5])
    vbits = np.unpackbits(vbytes, bitorder="little")
    if typ == T.T_BOOL:
        exp, exp_valid = R.select(vals, exp_branch, False)
        bits = np.unpackbits(data, bitorder="little")
        assert not bits[n:].any() and (bits[:n].astype(bool) == exp).all(), (what, "bits")
    elif string:
        exp_valid = R.select(vals, exp_branch, 0)[1]
        exp = R.select_views([v.values for v in vals], [v.valid for v in vals], [v.scalar for v in vals], nbufs, exp_branch)
        assert data.tobytes() == exp, (what, "views")
        table = np.concatenate([d.buffers.to_numpy(np.uint64, d.n_buffers) for d in dvals if d.n_buffers] or [np.zeros(0, np.uint64)])
        assert res.n_buffers == sum(nbufs) and (res.buffers.to_numpy(np.uint64, res.n_buffers) == table).all(), (what, "table")
    else:
        exp, exp_valid = R.select(vals, exp_branch, 0)
        assert data.tobytes() == exp.tobytes(), (what, "values", np.nonzero((data.reshape(n, size) != exp).any(axis=1))[0][:5])
    assert not vbits[n:].any() and (vbits[:n].astype(bool) == exp_valid).all(), (what, "validity")
    assert (res.dtype, res.n) == (typ, n) and (res.precision, res.scale) == DEC.get(typ, (0, 0))
    return exp_branch


# ---- every type, the case list ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", R.TYPES)
def test_every_type(gpu, typ):
    n = K.N
    size = SIZES_OF[typ]
    conds = K.conditions(n, 2)
    vals = K.bool_values(n, 3) if typ == T.T_BOOL else K.values(size, n, 3, last_valid=False)
    branch = run_select(gpu, typ, conds, vals, n, ("case", typ))
    assert set(branch) == {0, 1, 2}
    args = K.bool_values(n, 3, seed=1) if typ == T.T_BOOL else K.arguments(size, n, 3)
    if typ == T.T_BOOL:
        args[1].valid = K.validity(n, 0, seed=9)
    branch = run_select(gpu, typ, None, args, n, ("coalesce", typ))
    assert set(branch) == {0, 1, 2, 3}


def test_strings_by_value(gpu):
    """real Strings, inline and long, tables of 1, 2 and 0 buffers: the result's values read through ITS table"""
    n = K.N
    strs = [K.strings(n, j) for j in range(3)]
    strs[2] = [s[:12] for s in strs[2]]
    valid = [K.validity(n, 0), K.validity(n, 2), None]
    a = gpu.Column.strings(strs[0], valid[0])
    # two buffers: long values alternate between them
    views, bufs = np.zeros((n, 4), np.uint32), [bytearray(), bytearray()]
    for i, s in enumerate(strs[1]):
        views[i, 0] = len(s)
        if len(s) <= 12:
            views[i, 1:4] = np.frombuffer(s.ljust(12, b"\0"), np.uint32)
        else:
            views[i, 1:4] = (int.from_bytes(s[:4], "little"), i % 2, len(bufs[i % 2]))
            bufs[i % 2] += s
    dbufs = [gpu.DeviceBuffer.from_numpy(np.frombuffer(bytes(x) + bytes(16), np.uint8)) for x in bufs]
    b = gpu.Column(T.T_STRING, n, gpu.DeviceBuffer.from_numpy(views.view(np.uint8)), bitmap(gpu, valid[1]),
                   buffers=gpu.DeviceBuffer.from_numpy(np.array([x.ptr for x in dbufs], dtype=np.uint64)), keep=tuple(dbufs))
    b.n_buffers = 2
    c = gpu.Column.from_views(gpu.make_views(strs[2]))
    conds = K.conditions(n, 2)
    res = gpu.case_when([bool_col(gpu, x, 5) for x in conds], [a, b, c], n, want_branch=True)
    exp, exp_valid, exp_branch = R.case_when(conds, [R.Col(strs[j], valid[j]) for j in range(3)], n, b"")
    assert res.n_buffers == 3 and res.string_values() == exp
    assert (res.validity_numpy() == exp_valid).all() and (res.branch.to_numpy() == exp_branch).all()
    assert sum(1 for i in range(n) if len(exp[i]) > 12 and exp_branch[i] == 1) > 20
    # a scalar String that is long, with its own table, as ELSE
    long_ = gpu.Column.strings([b"a constant of more than twelve bytes"])
    long_.is_scalar = True
    res = gpu.case_when([bool_col(gpu, conds[1], 1)], [a, long_], n)
    exp, exp_valid, _ = R.case_when([conds[1]], [R.Col(strs[0], valid[0]), R.Col([b"a constant of more than twelve bytes"], None, True)], n, b"")
    assert res.n_buffers == 2 and res.string_values() == exp and (res.validity_numpy() == exp_valid).all()


# ---- word and lane boundaries ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", (T.T_I8, T.T_I64, T.T_DEC128, T.T_STRING))
def test_boundaries(gpu, typ):
    size = SIZES_OF[typ]
    for n in K.BOUNDARY_SIZES:
        if n == 0:
            empty = R.Col(np.zeros((0, size), np.uint8), None)
            res = gpu.case_when([bool_col(gpu, R.Col(np.zeros(0, bool), None))], [raw_col(gpu, typ, empty), raw_col(gpu, typ, empty)], 0)
            assert res.n == 0
            continue
        run_select(gpu, typ, K.conditions(n, 2), K.values(size, n, 3, last_valid=False), n, ("case", typ, n))
        run_select(gpu, typ, None, K.arguments(size, n, 2), n, ("coalesce", typ, n))


def test_sixteen_conditions(gpu):
    n = 6000
    conds, vals = K.conditions(n, 16), K.values(4, n, 17)
    branch = run_select(gpu, T.T_I32, conds, vals, n, "sixteen")
    assert set(branch) == set(range(17)), "every branch is reached"
    dconds = [bool_col(gpu, c) for c in K.conditions(n, 17)]
    dvals = [raw_col(gpu, T.T_I32, v) for v in K.values(4, n, 18)]
    w_out, out = guarded(gpu, 4 * n)
    with pytest.raises(T.DbhipError) as e:
        gpu.case_when(dconds, dvals, n, out=out)
    assert e.value.code == T.ERR_UNSUPPORTED and "dbhip_case" in str(e.value)
    ok, _ = guards_intact(w_out, 0)
    assert ok and (w_out.to_numpy(np.uint8, 4 * n + 80) == GUARD).all(), "a refused call wrote"
    run_select(gpu, T.T_I32, conds[:1], vals[:2], n, "the stream is still usable")


# ---- scalars ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("typ", (T.T_U8, T.T_I16, T.T_F32, T.T_TIMESTAMP, T.T_DEC128, T.T_DEC256, T.T_STRING, T.T_BOOL))
def test_scalars(gpu, typ):
    n = 777
    size = SIZES_OF[typ]
    one, zero = np.array([True]), np.array([False])
    if typ == T.T_BOOL:
        col, const = K.bool_values(n, 1)[0], [R.Col(one, None, True), R.Col(one, zero, True)]
    else:
        col = K.values(size, n, 1, last_valid=False)[0]
        const = [R.Col(K.raw_values(size, 1, 7), None, True), R.Col(K.raw_values(size, 1, 8), zero, True)]
    cond = K.conditions(n, 2)[1]
    for c in (cond, R.Col(one, None, True), R.Col(zero, None, True), R.Col(one, zero, True), R.Col(one, one, True)):
        for then, other in ((col, const[0]), (const[0], col), (const[0], const[1]), (const[1], col)):
            run_select(gpu, typ, [c], [then, other], n, ("scalars", typ))
    run_select(gpu, typ, None, [col, const[1], const[0]], n, ("coalesce(x, NULL, c)", typ))


def test_null_scalar_without_data_and_nullable_scalars(gpu):
    n = 1000
    rng = np.random.default_rng(5)
    x = rng.integers(-10**9, 10**9, n).astype(np.int32)
    vx = rng.random(n) < 0.7
    conds = K.conditions(n, 2)
    c = bool_col(gpu, conds[1], 69)
    res = gpu.case_when([c], [gpu.Column.from_numpy(x, validity=vx), gpu.null_scalar(T.T_I32)], n, want_branch=True)   # CASE without ELSE
    exp, exp_valid, exp_branch = R.case_when([conds[1]], [R.Col(x, vx), R.Col(np.array([0], np.int32), np.array([False]), True)], n, 0)
    assert (res.to_numpy() == exp).all() and (res.validity_numpy() == exp_valid).all() and (res.branch.to_numpy() == exp_branch).all()
    for voff in (0, 5):
        for valid in (True, False):
            s = S.nullable_scalar(gpu, 42, T.T_I32, valid, voff)
            rs = R.Col(np.array([42], np.int32), np.array([valid]), True)
            res = gpu.coalesce(gpu.Column.from_numpy(x, validity=vx), s, n=n)
            exp, exp_valid, _ = R.coalesce([R.Col(x, vx), rs], n, 0)
            assert (res.to_numpy() == exp).all() and (res.validity_numpy() == exp_valid).all(), (voff, valid)
            sc = gpu.Column.boolean([True])
            sc.is_scalar, sc.validity, sc.voff = True, gpu.DeviceBuffer.from_numpy(S.scalar_bitmap(valid, voff)), voff
            res = gpu.if_(sc, gpu.Column.from_numpy(x, validity=vx), s, n=n)
            exp, exp_valid, _ = R.case_when([R.Col(np.array([True]), np.array([valid]), True)], [R.Col(x, vx), rs], n, 0)
            assert (res.to_numpy() == exp).all() and (res.validity_numpy() == exp_valid).all(), (voff, valid)
            t = gpu.bool_and(sc, c, n)
            et, ev = R.bool_logic(R.AND, R.Col(np.array([True]), np.array([valid]), True), conds[1], n)
            assert (t.to_numpy() == et).all() and (t.validity_numpy() == ev).all(), (voff, valid)


# ---- slices -----------------------------------------------------------------------------------------------------------------------------------
def slice_maker(gpu, typ):
    if typ == T.T_DEC128:
        return lambda v, valid: gpu.Column.decimal128(v, 30, 4, validity=valid)
    if typ == T.T_STRING:
        return lambda v, valid: gpu.Column.strings(v, validity=valid)
    if typ == T.T_BOOL:
        return lambda v, valid: gpu.Column.boolean(v, validity=valid)
    return lambda v, valid: gpu.Column.from_numpy(v, typ, validity=valid)


def typed_values(typ, n, j):
    rng = np.random.default_rng([typ, n, j])
    if typ == T.T_I8:
        return rng.integers(1, 127, n).astype(np.int8)
    if typ == T.T_I64:
        return rng.integers(1, 2**62, n).astype(np.int64)
    if typ == T.T_DEC128:
        return [int(x) * 2**64 + int(y) + 1 for x, y in zip(rng.integers(-2**62, 2**62, n), rng.integers(0, 2**62, n))]
    return K.strings(n, j, seed=n)


def values_of(res):
    if res.dtype == T.T_STRING:
        return res.string_values()
    got = res.to_numpy()
    return list(got) if isinstance(got, list) else got


@pytest.mark.parametrize("typ", (T.T_I8, T.T_I64, T.T_DEC128, T.T_STRING))
def test_slices(gpu, typ):
    zero = b"" if typ == T.T_STRING else 0
    es = gpu.ELEM_SIZE[typ]
    for lo in S.LOS:
        for n in S.SIZES:
            conds = K.conditions(n, 2, seed=lo)
            dconds = [S.sliced(gpu, slice_maker(gpu, T.T_BOOL), np.asarray(c.values), c.valid, lo, seed=j) for j, c in enumerate(conds)]
            vals = [R.Col(typed_values(typ, n, j), K.validity(n, j, seed=lo)) for j in range(3)]
            dvals = [S.sliced(gpu, slice_maker(gpu, typ), v.values, v.valid, lo, seed=j) for j, v in enumerate(vals)]
            exp, exp_valid, exp_branch = R.case_when(conds, vals, n, zero)
            # the output a slice too: element-aligned, not 16-byte aligned (views stay 16-byte aligned), guard bytes on both sides
            lead = 16 if typ == T.T_STRING else (8 if typ == T.T_DEC128 else 13 * es)
            whole, out = guarded(gpu, n * es, lead)
            assert typ == T.T_STRING or out.ptr % 16 != 0
            res = gpu.case_when(dconds, dvals, n, want_branch=True, out=out)
            ok, _ = guards_intact(whole, n * es, lead)
            assert ok, (typ, lo, n, "guard")
            got = values_of(res)
            assert (list(got) == list(exp)) and (res.validity_numpy() == exp_valid).all(), (typ, lo, n)
            assert (res.branch.to_numpy() == exp_branch).all(), (typ, lo, n)
            res = gpu.coalesce(*dvals, n=n)
            exp, exp_valid, _ = R.coalesce(vals, n, zero)
            assert (list(values_of(res)) == list(exp)) and (res.validity_numpy() == exp_valid).all(), (typ, lo, n, "coalesce")


# ---- out_branch and the lazy branches -----------------------------------------------------------------------------------------------------------
def test_lazy_division(gpu):
    """if(b != 0, a / b, 0): the division raises on the rows where b = 0, and none of those errors is left once they are masked with
    out_branch == 0 (dbhip_cmp + dbhip_bitmap_binary), because those rows took the other branch"""
    n = 5003
    rng = np.random.default_rng(14)
    a = rng.integers(-10**12, 10**12, n).astype(np.int64)
    b = rng.integers(-3, 4, n).astype(np.int64)
    ca, cb = gpu.Column.from_numpy(a), gpu.Column.from_numpy(b)
    cond = gpu.cmp(T.CMP_NOTEQ, cb, gpu.Column.scalar(0, T.T_I64))
    errors = gpu.RowErrors(n)
    q = gpu.arith(T.OP_DIVIDE, ca, cb, errors=errors)
    assert q.dtype == T.T_F64 and errors.num_errors() == int((b == 0).sum()) > 100
    res = gpu.if_(cond, q, gpu.Column.scalar(0.0, T.T_F64), want_branch=True)
    took = gpu.cmp(T.CMP_EQ, res.branch, gpu.Column.scalar(0, T.T_U8))             # the rows that took the division
    left = gpu.DeviceBuffer(((n + 63) // 64) * 8)                                  # took AND NOT ok: the errors that count
    T.check(T.lib().dbhip_bitmap_binary(2, C.c_void_p(took.data.ptr), C.c_void_p(errors.bitmap.ptr), C.c_int64(n), C.c_void_p(left.ptr), None))
    assert gpu.bitmap_count(gpu.Column(T.T_BOOL, n, left), n) == 0
    assert (res.branch.to_numpy() == (b == 0)).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        exp = np.where(b != 0, a.astype(np.float64) / b.astype(np.float64), 0.0)
    assert res.to_numpy().tobytes() == exp.tobytes()


@pytest.mark.parametrize("typ", (T.T_I64, T.T_F64))
def test_parity_with_the_expression_program(gpu, typ):
    n = 70_001
    rng = np.random.default_rng(typ)
    if typ == T.T_I64:
        x, y = rng.integers(-2**62, 2**62, n), rng.integers(-2**62, 2**62, n)
    else:
        x, y = rng.standard_normal(n), rng.standard_normal(n)
        x[::97], y[::89] = np.nan, -0.0
    cx, cy = gpu.Column.from_numpy(x, typ), gpu.Column.from_numpy(y, typ)
    p = gpu.ExprProgram([cx, cy])
    lx, ly = p.load(0), p.load(1)
    old = p.run(p.if_(p.cmp(T.EX_LT, lx, ly, keep=(lx, ly)), lx, ly), n=n)["values"]
    new = gpu.if_(gpu.cmp(T.CMP_LT, cx, cy), cx, cy)
    assert new.validity is None and new.to_numpy().tobytes() == old.tobytes()


# ---- Kleene logic ---------------------------------------------------------------------------------------------------------------------------------
def logic_matches(gpu, op, a, b, n, da, db, what):
    w_t, t = guarded(gpu, ((n + 63) // 64) * 8)
    w_v, v = guarded(gpu, ((n + 63) // 64) * 8)
    gpu.bool_logic(op, da, db if op != R.NOT else None, n, out=t, out_validity=v)
    et, ev = R.bool_logic(op, a, b, n)
    for whole, exp, name in ((w_t, et, "true"), (w_v, ev, "valid")):
        ok, raw = guards_intact(whole, ((n + 63) // 64) * 8)
        bits = np.unpackbits(raw, bitorder="little")
        assert ok and not bits[n:].any() and (bits[:n].astype(bool) == exp).all(), (what, R.NAMES[op], name, n)


@pytest.mark.parametrize("op", (R.AND, R.OR, R.NOT, R.XOR))
def test_kleene_boundaries(gpu, op):
    for n in K.BOUNDARY_SIZES[1:]:
        f = K.kleene_operands(n)
        a, b = f["nullable"], f["words"]
        logic_matches(gpu, op, a, b, n, bool_col(gpu, a, 69), bool_col(gpu, b, 1), "columns")


@pytest.mark.parametrize("op", (R.AND, R.OR, R.NOT, R.XOR))
def test_kleene_every_pair_of_forms(gpu, op):
    n = 333
    forms = K.kleene_operands(n)
    dev = {k: bool_col(gpu, c, K.FETCH_OFFSETS[i % 5]) for i, (k, c) in enumerate(forms.items())}
    for na, a in forms.items():
        for nb, b in forms.items():
            if op == R.NOT and nb != "plain":
                continue
            logic_matches(gpu, op, a, b, n, dev[na], dev[nb], (na, nb))


def test_kleene_slices_and_the_composition(gpu):
    for lo in S.LOS:
        for n in S.SIZES:
            f = K.kleene_operands(n, seed=lo)
            a, b = f["nullable"], f["words"]
            da = S.sliced(gpu, slice_maker(gpu, T.T_BOOL), np.asarray(a.values), a.valid, lo)
            db = S.sliced(gpu, slice_maker(gpu, T.T_BOOL), np.asarray(b.values), b.valid, lo, seed=1)
            for op in (R.AND, R.OR, R.NOT, R.XOR):
                logic_matches(gpu, op, a, b, n, da, db, ("sliced", lo))
            # OR as a binding had to spell it before: five dbhip_bitmap_binary launches over Bitmaps at bit 0
            A, VA, B, VB = da.bits(), gpu._validity_at_zero(da), db.bits(), gpu._validity_at_zero(db)
            ta, tb = gpu._bitmap_op(0, A, VA, n), gpu._bitmap_op(0, B, VB, n)
            true = gpu._bitmap_op(1, ta, tb, n)
            valid = gpu._bitmap_op(1, gpu._bitmap_op(0, VA, VB, n), true, n)
            res = gpu.bool_or(da, db, n)
            # (the composition leaves whatever its inputs held past n; the new call writes zeros there: compare the n rows)
            nbytes = (n + 7) // 8
            for got, exp in ((res.data, true), (res.validity, valid)):
                assert (gpu.unpack_bits(got.to_numpy(np.uint8, nbytes), n) == gpu.unpack_bits(exp.to_numpy(np.uint8, nbytes), n)).all(), (lo, n)


def test_nullif_and_is_null(gpu):
    n = 4099
    rng = np.random.default_rng(33)
    x, y = rng.integers(0, 4, n).astype(np.int64), rng.integers(0, 4, n).astype(np.int64)
    vx, vy = rng.random(n) < 0.7, rng.random(n) < 0.7
    for va, vb in ((vx, vy), (None, vy), (vx, None), (None, None)):
        a, b = gpu.Column.from_numpy(x, validity=va), gpu.Column.from_numpy(y, validity=vb)
        res = gpu.nullif(a, b)
        assert (res.to_numpy() == x).all() and (res.validity_numpy() == R.nullif(R.Col(x, va), R.Col(y, vb), n)).all()
    sl = S.sliced(gpu, slice_maker(gpu, T.T_I64), x, vx, 69)
    res = gpu.nullif(sl, gpu.Column.scalar(2, T.T_I64))
    assert (res.validity_numpy() == R.nullif(R.Col(x, vx), R.Col(np.array([2]), None, True), n)).all() and (res.to_numpy() == x).all()
    for col, valid in ((sl, vx), (gpu.Column.from_numpy(x), np.ones(n, bool)), (S.nullable_scalar(gpu, 1, T.T_I64, False, 5), np.zeros(n, bool))):
        assert (gpu.is_null(col, n).to_numpy() == ~valid).all() and (gpu.is_not_null(col, n).to_numpy() == valid).all()


# ---- one composed plan ------------------------------------------------------------------------------------------------------------------------------
def test_promo_revenue_plan(gpu):
    """sum(CASE WHEN p_type LIKE 'PROMO%' THEN price * (1 - disc) ELSE 0 END) group by k: dbhip_like gives the condition,
    dbhip_decimal_arith the branch, a Decimal constant the ELSE, then the group-by — against Python ints"""
    n = 10_007
    rng = np.random.default_rng(1400)
    kinds = [b"PROMO BRUSHED COPPER", b"STANDARD PLATED TIN", b"PROMO ANODIZED", b"ECONOMY POLISHED STEEL", b"PROMOTION", b"PROM"]
    p_type = [kinds[i] for i in rng.integers(0, len(kinds), n)]
    key = rng.integers(0, 23, n).astype(np.int64)
    price = rng.integers(1, 10**9, n).astype(np.int64)                      # Decimal(15, 2)
    one_minus_disc = rng.integers(85, 101, n).astype(np.int64)              # Decimal(15, 2)
    cond = gpu.like(gpu.Column.strings(p_type), b"PROMO%")
    prod = gpu.decimal_arith(T.OP_MULTIPLY, gpu.Column.from_numpy(price, T.T_DEC64, precision=15, scale=2),
                             gpu.Column.from_numpy(one_minus_disc, T.T_DEC64, precision=15, scale=2))
    assert (prod.dtype, prod.precision, prod.scale) == (T.T_DEC128, 30, 4)
    promo = gpu.case_when([cond], [prod, gpu.Column.scalar(0, T.T_DEC128, 30, 4)], n)
    assert (promo.dtype, promo.precision, promo.scale, promo.validity) == (T.T_DEC128, 30, 4, None)
    g = gpu.GroupBy([T.T_I64], [(T.AGG_SUM, T.T_DEC128, 30, 4, 0), (T.AGG_COUNT, 0, 0, 0, 0)])
    g.add_block([gpu.Column.from_numpy(key)], [promo, None], n)
    exp = {}
    for k, t, a, b in zip(key.tolist(), p_type, price.tolist(), one_minus_disc.tolist()):
        tot, cnt = exp.get(k, (0, 0))
        exp[k] = (tot + (a * b if t.startswith(b"PROMO") else 0), cnt + 1)
    assert sorted(tuple(r) for r in g.result()) == sorted((k, tot, cnt) for k, (tot, cnt) in exp.items())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_call_and_leave_the_stream_usable(gpu):
    n = 300
    x = gpu.Column.from_numpy(np.arange(n, dtype=np.int32))
    y = gpu.Column.from_numpy(np.arange(n, dtype=np.int64))
    c = gpu.Column.boolean(np.arange(n) % 2 == 0)
    d1 = gpu.Column.from_numpy(np.arange(n, dtype=np.int64), T.T_DEC64, precision=15, scale=2)
    d2 = gpu.Column.from_numpy(np.arange(n, dtype=np.int64), T.T_DEC64, precision=15, scale=3)
    for call, name in ((lambda: gpu.case_when([c], [x, y], n), "dbhip_case"), (lambda: gpu.coalesce(d1, d2, n=n), "dbhip_coalesce"),
                       (lambda: gpu.case_when([x], [x, x], n), "dbhip_case"), (lambda: gpu.case_when([], [x], n), "dbhip_case"),
                       (lambda: gpu.coalesce(x, y, n=n), "dbhip_coalesce"), (lambda: gpu.bool_and(c, x, n), "dbhip_bool_logic")):
        with pytest.raises(T.DbhipError) as e:
            call()
        assert e.value.code == T.ERR_INVALID and name in str(e.value), (name, str(e.value))
    out = gpu.DeviceBuffer(4 * n)
    assert T.lib().dbhip_coalesce(None, 2, C.c_int64(n), C.c_void_p(out.ptr), None, None, None, None, None) == T.ERR_INVALID
    assert b"dbhip_coalesce" in T.lib().dbhip_last_error()
    res = gpu.if_(c, x, gpu.Column.scalar(-1, T.T_I32))
    assert (res.to_numpy() == np.where(np.arange(n) % 2 == 0, np.arange(n), -1)).all()
