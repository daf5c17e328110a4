"""GPU decode of nested Parquet leaves (dbhip_pq_chunk_open_device_nested / _decode_device_nested): every node of a leaf's path — offsets,
validity bits, item and NULL counts — and the leaf bytes, compared bit for bit with what pyarrow (the independent reader) reads from the
same file. Also: a 20 M-entry chunk, the one-LIST path against decode_device_list, the reference-held fixtures, hand-built malformed
levels, bit flips inside the level streams, and edge cases."""
import ctypes as C
import struct

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import parquet_nested_util as NU
from tests import parquet_ref as PR
from tests import parquet_util as PU

pytestmark = pytest.mark.gpu

SHAPES = NU.shapes()
LV_LDS = 40960    # k_parquet_dev.hip: level streams up to this size are walked from LDS, longer ones in place


def _decode(gpu, ch, path, ln, out_type):
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], out_type, ch["type_length"], codec=ch["codec"], nested=path, leaf_nullable=ln)
    res, col = pc.decode_nested()
    return pc, res, col


# ---- 1. shapes against pyarrow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(NU.VARIANTS))
@pytest.mark.parametrize("codec", NU.CODECS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_equal_pyarrow(gpu, shape, codec, variant):
    v2, dictionary = NU.VARIANTS[variant]
    spec = SHAPES[shape]
    chunks, back = NU.write_shape(spec, 2500, seed=len(shape) * 7 + len(codec), codec=codec, v2=v2, dictionary=dictionary)
    for ch, (path, ln, kind) in zip(chunks, NU.leaves(spec)):
        ot = NU.LEAF_KINDS[kind]
        pc, res, col = _decode(gpu, ch, NU.node_tuples(path), ln, ot)
        assert pc.rows == len(back)
        NU.check_decoded(res, col, back, path, ln, ot)
        pc.close()


# ---- 2. larger inputs ---------------------------------------------------------------------------------------------------------
def _big_list_list(seed):
    """List<List<Int64>> (all nullable) of >= 20 M level entries, from numpy offsets and masks. The first rows are [[v]] — their level
    streams are RLE runs, so those pages are walked from LDS — the rest are random, whose level streams exceed LV_LDS."""
    import pyarrow as pa
    rng = np.random.default_rng(seed)
    n_rows = 6_000_000
    n_plain = 1_000_000
    # outer lists: lengths 0..4, 10 % NULL (empty span)
    olen = rng.integers(0, 5, n_rows)
    olen[:n_plain] = 1
    onull = rng.random(n_rows) < 0.1
    onull[:n_plain] = False
    olen[onull] = 0
    ooff = np.zeros(n_rows + 1, np.int32)
    np.cumsum(olen, out=ooff[1:])
    n_mid = int(ooff[-1])
    ilen = rng.integers(0, 6, n_mid)
    ilen[:n_plain] = 1
    inull = rng.random(n_mid) < 0.1
    inull[:n_plain] = False
    ilen[inull] = 0
    ioff = np.zeros(n_mid + 1, np.int32)
    np.cumsum(ilen, out=ioff[1:])
    n_val = int(ioff[-1])
    vals = rng.integers(-2**62, 2**62, n_val)
    vnull = rng.random(n_val) < 0.1
    vnull[:n_plain] = False
    leaf = pa.array(vals, pa.int64(), mask=vnull)
    inner = pa.ListArray.from_arrays(pa.array(ioff), leaf, mask=pa.array(inull))
    outer = pa.ListArray.from_arrays(pa.array(ooff), inner, mask=pa.array(onull))
    table = pa.Table.from_arrays([outer], names=["c"])
    return table


@pytest.mark.parametrize("codec", ["zstd", "none"])
def test_large_list_list_chunk(gpu, codec):
    table = _big_list_list(21)
    chunks, back = NU.write_table(table, codec, True, False, page_size=1 << 20)
    ch = chunks[0]
    assert ch["num_values"] >= 20_000_000
    # both walks of the level streams run: v2 headers carry the level byte lengths
    lev = [pg["header"][8][5] + pg["header"][8][6] for pg in NU.pages(ch["chunk"]) if pg["type"] == 3]
    assert min(lev) + 8 <= LV_LDS - 16 and max(lev) > LV_LDS, (min(lev), max(lev))
    path = [("list", 1, None), ("list", 1, None)]
    pc, res, col = _decode(gpu, ch, NU.node_tuples(path), 1, T.T_I64)
    assert pc.rows == len(back)
    NU.check_decoded(res, col, back, path, 1, T.T_I64)
    pc.close()


# ---- 3. the one-LIST path equals decode_device_list ---------------------------------------------------------------------------------
def _list_array(rng, n, ln, en, kind):
    import pyarrow as pa
    from decimal import Decimal
    rows = []
    for _ in range(n):
        if ln and rng.random() < 0.15:
            rows.append(None)
            continue
        row = []
        for _ in range(int(rng.integers(0, 4))):
            if en and rng.random() < 0.15:
                row.append(None)
            elif kind == "i64":
                row.append(int(rng.integers(-2**62, 2**62)))
            elif kind == "str":
                row.append("s%d-" % int(rng.integers(0, 10**6)) + "y" * int(rng.integers(0, 18)))
            elif kind == "bool":
                row.append(bool(rng.integers(0, 2)))
            else:
                row.append(Decimal(int(rng.integers(-10**15, 10**15))).scaleb(-6))
        rows.append(row)
    et = {"i64": pa.int64(), "str": pa.string(), "bool": pa.bool_(), "dec": pa.decimal128(38, 6)}[kind]
    typ = pa.list_(pa.field("item", et, nullable=bool(en)))
    return pa.Table.from_arrays([pa.array(rows, type=typ)], schema=pa.schema([pa.field("c", typ, nullable=bool(ln))]))


@pytest.mark.parametrize("kind", ["i64", "str", "bool", "dec"])
@pytest.mark.parametrize("ln,en", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_one_list_path_equals_decode_list(gpu, ln, en, kind):
    rng = np.random.default_rng(ln * 2 + en + 10 * len(kind))
    table = _list_array(rng, 6000, ln, en, kind)
    ot = NU.LEAF_KINDS[kind]
    for codec, v2, dictionary in (("none", False, False), ("zstd", True, True)):
        ch = NU.write_table(table, codec, v2, dictionary)[0][0]
        a = gpu.ParquetChunk(ch["chunk"], ch["physical"], ot, ch["type_length"], codec=ch["codec"], list_of=(ln, en))
        offs, lv, acol = a.decode_list()
        b = gpu.ParquetChunk(ch["chunk"], ch["physical"], ot, ch["type_length"], codec=ch["codec"], nested=[("list", ln)], leaf_nullable=en)
        res, bcol = b.decode_nested()
        (boffs, blv, brows, bnulls), = res
        assert b.rows == a.rows == brows and np.array_equal(boffs, offs)
        if ln:
            assert np.array_equal(blv, lv) and bnulls == a.null_lists
        else:
            assert blv is None and bnulls == 0
        assert bcol.n == acol.n == a.elems
        nbytes = (acol.n + 7) // 8 if kind == "bool" else acol.n * PU.ESIZE[ot]
        assert np.array_equal(bcol.data.to_numpy(np.uint8, nbytes), acol.data.to_numpy(np.uint8, nbytes))
        if en:
            vb = (acol.n + 7) // 8
            assert np.array_equal(bcol.validity.to_numpy(np.uint8, vb), acol.validity.to_numpy(np.uint8, vb))
        a.close()
        b.close()


# ---- 4. reference-held fixtures through the new entry point ---------------------------------------------------------------------------
def _rows_of(res, col, ln_path):
    """a List leaf (path [LIST ln]) -> python list of lists (None for a NULL list / element)"""
    (offs, lv, rows, _), = res
    ev = col.validity_numpy()
    vals = col.to_strings() if col.dtype == T.T_STRING else col.to_numpy().tolist()
    return [None if (lv is not None and not lv[r]) else [vals[x] if ev[x] else None for x in range(int(offs[r]), int(offs[r + 1]))] for r in range(rows)]


def test_reference_fixtures_through_decode_nested(gpu):
    def decode_list(ch, ln, en, ot):
        pc, res, col = _decode(gpu, ch, [("list", ln)], en, ot)
        out = _rows_of(res, col, ln)
        pc.close()
        return out

    assert PR.check_lists(decode_list) == 4

    def decode_map_leaf(ch, ln, en, ot):
        # a Map leaf: [LIST 1, STRUCT 0] + the key / value leaf (the required STRUCT adds no level)
        assert ln == 1
        pc, res, col = _decode(gpu, ch, [("list", 1), ("struct", 0)], en, ot)
        (offs, lv, rows, _), (so, sv, sitems, snulls) = res
        assert so is None and sv is None and sitems == int(offs[-1]) and snulls == 0
        out = _rows_of(res[:1], col, 1)
        pc.close()
        return out

    assert PR.check_map(decode_map_leaf) == 1

    def decode_flat(ch, ot):
        pc, res, col = _decode(gpu, ch, [("struct", 0)], 0, ot)
        (so, sv, items, nulls), = res
        assert so is None and sv is None and items == pc.rows == col.n
        vals = col.to_strings() if ot == T.T_STRING else col.to_numpy().tolist()
        pc.close()
        return vals, np.ones(len(vals), bool)

    assert PR.check_tuple(decode_flat) == 3


# ---- 5. malformed input ----------------------------------------------------------------------------------------------------------
def _decode_rc(gpu, data, path, ln, ot=T.T_I64, physical=2):
    pc = gpu.ParquetChunk(data, physical, ot, 0, codec=0, nested=path, leaf_nullable=ln)
    try:
        res, col = pc.decode_nested()
        return 0, pc, res, col
    except T.DbhipError as e:
        pc.close()
        return e.code, None, None, None


@pytest.mark.parametrize("case", ["first_entry_repeats", "repeat_without_element", "def_above_max", "rep_above_R"])
def test_malformed_levels_are_invalid(gpu, case):
    # List<List<Int64>> all required: R = 2, max_def = 2, Ê_1 = 1, Ê_2 = 2
    path = [("list", 0), ("list", 0)]
    ln = 0
    if case == "first_entry_repeats":
        reps, defs = [1, 0], [2, 2]
    elif case == "repeat_without_element":
        reps, defs = [0, 2, 0], [2, 1, 2]
    elif case == "def_above_max":
        reps, defs = [0, 0], [2, 3]
    else:
        # a List<List> page opened with a one-LIST path (max_def 2 with a nullable leaf): r = 2 > R = 1
        reps, defs = [0, 2, 1], [2, 2, 2]
        path, ln = [("list", 0)], 1
    page = NU.v1_levels_page(reps, defs, [7] * sum(1 for d in defs if d == 2))
    rc, _, _, _ = _decode_rc(gpu, page, path, ln)
    assert rc == T.ERR_INVALID, case
    # (a well-formed page of the same shape decodes)
    ok = NU.v1_levels_page([0, 2, 1, 0], [2, 2, 2, 1], [5, 6, 7])
    rc, pc, res, col = _decode_rc(gpu, ok, [("list", 0), ("list", 0)], 0)
    assert rc == 0
    assert res[0][0].tolist() == [0, 2, 3] and res[1][0].tolist() == [0, 2, 3, 3] and col.to_numpy().tolist() == [5, 6, 7]
    pc.close()


def test_bit_flips_in_the_level_streams_never_fault(gpu):
    chunks, _ = NU.write_shape(SHAPES["list_list_i64_111"], 20_000, seed=17, codec="none", v2=False, dictionary=False)
    ch = chunks[0]
    ranges = NU.v1_level_ranges(ch["chunk"])
    path = [("list", 1), ("list", 1)]
    rng = np.random.default_rng(60)
    outcomes = {"refused": 0, "decoded": 0}
    for k in range(60):
        a, b = ranges[int(rng.integers(0, len(ranges)))]
        pos = int(rng.integers(a, b))
        m = bytearray(ch["chunk"])
        m[pos] ^= 1 << int(rng.integers(0, 8))
        rc, _ = NU.open_nested(ch, path, 1, T.T_I64, data=bytes(m))
        assert rc == T.OK, (k, pos)         # open reads headers only: a refusal means the flip missed the level streams
        rc, pc, res, col = _decode_rc(gpu, bytes(m), path, 1)
        if rc:
            assert rc in (T.ERR_INVALID, T.ERR_UNSUPPORTED), rc
            outcomes["refused"] += 1
            continue
        entries = pc.info.num_values
        (o0, _, rows, _), (o1, _, mids, _) = res
        assert np.all(np.diff(o0.astype(np.int64)) >= 0) and np.all(np.diff(o1.astype(np.int64)) >= 0)
        assert int(o0[-1]) == mids and int(o1[-1]) == col.n
        assert rows <= entries and mids <= entries and col.n <= entries
        outcomes["decoded"] += 1
        pc.close()
    assert sum(outcomes.values()) == 60


# ---- 6. edge cases ---------------------------------------------------------------------------------------------------------------
def test_empty_chunk(gpu):
    import pyarrow as pa
    typ = NU.arrow_type(SHAPES["list_list_i64_111"])
    table = pa.table({"c": pa.array([], type=typ)})
    ch = NU.write_table(table, "none", False, False)[0][0]
    pc, res, col = _decode(gpu, ch, [("list", 1), ("list", 1)], 1, T.T_I64)
    assert pc.rows == 0 and col.n == 0
    assert [r[2] for r in res] == [0, 0] and res[0][0].tolist() == [0] and res[1][0].tolist() == [0]


@pytest.mark.parametrize("shape", ["list_list_i64_111", "tuple_list"])
def test_only_null_rows(gpu, shape):
    import pyarrow as pa
    spec = SHAPES[shape]
    typ = NU.arrow_type(spec)
    table = pa.Table.from_arrays([pa.array([None] * 3000, type=typ)], schema=pa.schema([pa.field("c", typ, nullable=True)]))
    for codec, v2, dictionary in (("none", False, False), ("snappy", True, True)):
        chunks, back = NU.write_table(table, codec, v2, dictionary)
        for ch, (path, ln, kind) in zip(chunks, NU.leaves(spec)):
            pc, res, col = _decode(gpu, ch, NU.node_tuples(path), ln, NU.LEAF_KINDS[kind])
            assert pc.rows == 3000 and res[0][3] == 3000
            NU.check_decoded(res, col, back, path, ln, NU.LEAF_KINDS[kind])
            pc.close()


def test_delta_byte_array_strings_with_arena(gpu):
    spec = NU.L(1, NU.L(1, NU.leaf(1, "str")))
    chunks, back = NU.write_shape(spec, 4000, seed=9, codec="zstd", v2=True, dictionary=False, encoding={"c.list.element.list.element": "DELTA_BYTE_ARRAY"})
    ch = chunks[0]
    assert "DELTA_BYTE_ARRAY" in ch["encodings"], ch["encodings"]
    path = [("list", 1, None), ("list", 1, None)]
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], T.T_STRING, 0, codec=ch["codec"], nested=NU.node_tuples(path), leaf_nullable=1)
    res, col = pc.decode_nested()
    assert col.n_buffers == 2           # buffer 1: the arena take_arena handed over
    assert pc.take_arena() is None      # (taken once)
    NU.check_decoded(res, col, back, path, 1, T.T_STRING)
    pc.close()


def test_batched_decode_refuses_a_nested_handle(gpu):
    ch = NU.write_shape(SHAPES["list_list_i64_111"], 500, seed=2, codec="none", v2=False, dictionary=False)[0][0]
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], T.T_I64, 0, codec=0, nested=[("list", 1), ("list", 1)], leaf_nullable=1)
    with pytest.raises(T.DbhipError) as e:
        gpu.ParquetChunk.decode_many([pc])
    assert e.value.code == T.ERR_INVALID
    with pytest.raises(T.DbhipError) as e:
        pc.decode()
    assert e.value.code == T.ERR_INVALID
    pc.close()
