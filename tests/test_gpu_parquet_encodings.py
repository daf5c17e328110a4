"""GPU decode of DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY and BYTE_STREAM_SPLIT data pages (device mode of the scan side), every column
compared with what pyarrow (the independent reader) reads from the same file. DELTA_BYTE_ARRAY values are materialised into the chunk's
arena, buffer 1 of a String column (dbhip_pq_chunk_take_arena)."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import parquet_util as PU

pytestmark = pytest.mark.gpu

CODECS = ["none", "snappy", "lz4", "zstd"]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _write(table, encoding, codec="none", v2=False, page_size=64 * 1024, dictionary=False, col="c"):
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    kw = dict(compression=codec, use_dictionary=dictionary, write_statistics=False, data_page_version="2.0" if v2 else "1.0",
              row_group_size=max(table.num_rows, 1), store_schema=False, data_page_size=page_size)
    if encoding is not None:
        kw["column_encoding"] = {col: encoding}
    pq.write_table(table, buf, **kw)
    return PU.column_chunks(buf.getvalue())


def _resolve_strings(views, valid, bufs):
    """16-byte views -> bytes (None where not valid); bufs: host copies of the column's buffers, by buffer index"""
    out = []
    w = views.view(np.uint32).reshape(-1, 4)
    for r in range(len(views)):
        if not valid[r]:
            assert not views[r].any(), r            # a NULL row decodes to an all-zero view
            out.append(None)
            continue
        ln = int(w[r, 0])
        if ln <= 12:
            out.append(views[r, 4:4 + ln].tobytes())
        else:
            b, off = int(w[r, 2]), int(w[r, 3])
            s = bufs[b][off:off + ln].tobytes()
            assert s[:4] == views[r, 4:8].tobytes(), r
            out.append(s)
    return out


def _col_values(col, ot, n, valid):
    if ot == T.T_STRING:
        bufs = [k.to_numpy(np.uint8, k.nbytes) for k in col._keep]
        assert col.n_buffers == len(bufs)
        ptrs = col.buffers.to_numpy(np.uint64, col.n_buffers)
        assert [int(p) for p in ptrs] == [k.ptr for k in col._keep]
        return _resolve_strings(col.data.to_numpy(np.uint8, 16 * n).reshape(-1, 16), valid, bufs)
    raw = col.data.to_numpy(np.uint8, n * PU.ESIZE[ot]).tobytes()
    return PU.decoded_to_python(raw, valid, ot, n)


def _valid_of(col, i):
    n = i.num_values
    if not i.has_validity:
        return np.ones(n, dtype=bool)
    bits = np.unpackbits(col.validity.to_numpy(np.uint8, i.validity_bytes), bitorder="little")
    return bits[:n].astype(bool)


def _decode(gpu, ch, ot, precision=0, scale=0):
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], ot, ch["type_length"], ch["max_def"], 0, ch["codec"], precision=precision, scale=scale,
                          device=True)
    col = pc.decode()
    valid = _valid_of(col, pc.info)
    got = _col_values(col, ot, pc.info.num_values, valid)
    pc.close()
    return got, valid


def _check(gpu, ch, back, ot, what):
    exp, exp_valid = PU.expected_of(back.column(0), ot)
    got, valid = _decode(gpu, ch, ot)
    assert np.array_equal(valid, exp_valid), what
    assert got == exp, what


def _gen(name, n, frac, rng):
    import pyarrow as pa
    from decimal import Decimal
    mask = rng.random(n) < frac if frac else None
    if name == "str":
        base = ["", "a", "abc", "http://example.com/", "http://example.com/path/to/some/resource?id=", "key-0000000"]
        vals = [base[int(x) % len(base)] + str(int(x)) * int(x % 4) for x in rng.integers(0, 10**6, n)]
        vals.sort()
        return pa.array(vals, pa.string(), mask=mask), T.T_STRING
    if name == "dec15_2":
        return pa.array([Decimal(int(x)).scaleb(-2) for x in rng.integers(-10**13, 10**13, n)], pa.decimal128(15, 2), mask=mask), T.T_DEC128
    if name == "dec38_6":
        return pa.array([Decimal(int(x) * 10**12 + 7).scaleb(-6) for x in rng.integers(-10**18, 10**18, n)], pa.decimal128(38, 6), mask=mask), T.T_DEC128
    if name == "f32":
        a = rng.standard_normal(n).astype(np.float32)
        a[::97] = np.nan
        a[5::101] = -0.0
        return pa.array(a, pa.float32(), mask=mask), T.T_F32
    if name == "f64":
        a = rng.standard_normal(n)
        a[::89] = np.nan
        a[3::103] = -0.0
        a[7::107] = np.inf
        return pa.array(a, pa.float64(), mask=mask), T.T_F64
    if name == "i32":
        return pa.array(rng.integers(-2**31, 2**31, n), pa.int32(), mask=mask), T.T_I32
    return pa.array(rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64), pa.int64(), mask=mask), T.T_I64


GRID = [("DELTA_LENGTH_BYTE_ARRAY", "str"), ("DELTA_BYTE_ARRAY", "str"), ("DELTA_BYTE_ARRAY", "dec15_2"), ("DELTA_BYTE_ARRAY", "dec38_6"),
        ("BYTE_STREAM_SPLIT", "f32"), ("BYTE_STREAM_SPLIT", "f64"), ("BYTE_STREAM_SPLIT", "i32"), ("BYTE_STREAM_SPLIT", "i64"),
        ("BYTE_STREAM_SPLIT", "dec15_2"), ("BYTE_STREAM_SPLIT", "dec38_6")]


# ---- coverage grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("v2", [False, True])
def test_encoding_grid_matches_pyarrow(gpu, codec, v2):
    import pyarrow as pa
    rng = np.random.default_rng(17)
    for enc, name in GRID:
        for frac in (0.0, 0.07, 1.0):
            for n in (1, 129, 70_000):
                arr, ot = _gen(name, n, frac, rng)
                chunks, back = _write(pa.table({"c": arr}), enc, codec, v2, page_size=32 * 1024)
                ch = chunks[0]
                if frac < 1.0:
                    assert enc in ch["encodings"], (enc, ch["encodings"])
                _check(gpu, ch, back, ot, (enc, name, codec, v2, frac, n))


# ---- strings ---------------------------------------------------------------------------------------------------------------------
def _string_cases(rng):
    long_a = "x" * 20_000 + "tail-a"
    long_b = "x" * 20_000 + "tail-b" + "y" * 5000             # longer than the replay's LDS ring, sharing a 20 000-byte prefix
    urls = sorted(f"https://www.example.org/catalog/category-{int(c):03d}/item/{int(i):09d}.html" for c, i in zip(rng.integers(0, 50, 3000),
                                                                                                       rng.integers(0, 10**9, 3000)))
    keys = sorted(f"customer#{int(x):012d}" for x in rng.integers(0, 10**12, 5000))
    return {
        "empty_only": [""] * 300,
        "empty_first": ["", "", "a", "", "abcdefghijklmnop", "abcdefghijklmnop", ""],
        "short_long_mix": ["ab", "abcdefghijklm", "abcdefghijkl", "abcdefghijklmnopqrstuvwxyz", "abc", "", "zz" * 40, "zz" * 6],
        "prefix_of_previous": ["hello world, hello world", "hello world", "hello", "h", "", "hello world, again"],
        "sorted_keys": keys,
        "urls": urls,
        "longer_than_ring": [long_a, long_b, long_a, long_b[:20_003], long_b, "", long_a],
    }


@pytest.mark.parametrize("codec", ["none", "zstd"])
@pytest.mark.parametrize("enc", ["DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"])
def test_string_shapes(gpu, codec, enc):
    import pyarrow as pa
    rng = np.random.default_rng(2)
    for name, vals in _string_cases(rng).items():
        for v2 in (False, True):
            for nullable in (False, True):
                mask = (rng.random(len(vals)) < 0.2) if nullable else None
                chunks, back = _write(pa.table({"c": pa.array(vals, pa.string(), mask=mask)}), enc, codec, v2, page_size=8 * 1024)
                _check(gpu, chunks[0], back, T.T_STRING, (name, v2, nullable))


# ---- a chunk that mixes encodings, read by an operator ---------------------------------------------------------------------------
def _concat_chunk(dict_ch, dba_ch):
    ch = dict(dict_ch)
    ch["chunk"] = dict_ch["chunk"] + dba_ch["chunk"]
    return ch


@pytest.mark.parametrize("codec", ["none", "zstd"])
def test_dictionary_then_delta_byte_array_pages_feed_an_operator(gpu, codec):
    """what a format-2 writer's dictionary fallback produces: a dictionary page and RLE_DICTIONARY pages, then DELTA_BYTE_ARRAY pages"""
    import pyarrow as pa
    rng = np.random.default_rng(9)
    a = [f"city-{int(x) % 40:02d}" + ("/district-with-a-long-name" if x % 3 == 0 else "") for x in rng.integers(0, 10**6, 20_000)]
    b = sorted(f"https://host.example/{int(x):010d}/resource" for x in rng.integers(0, 10**10, 30_000))
    ma, mb = rng.random(len(a)) < 0.05, rng.random(len(b)) < 0.05
    ca, back_a = _write(pa.table({"c": pa.array(a, pa.string(), mask=ma)}), None, codec, v2=True, dictionary=True, page_size=16 * 1024)
    cb, back_b = _write(pa.table({"c": pa.array(b, pa.string(), mask=mb)}), "DELTA_BYTE_ARRAY", codec, v2=True, page_size=16 * 1024)
    assert "RLE_DICTIONARY" in ca[0]["encodings"] and "DELTA_BYTE_ARRAY" in cb[0]["encodings"]
    ch = _concat_chunk(ca[0], cb[0])
    exp = PU.expected_of(back_a.column(0), T.T_STRING)[0] + PU.expected_of(back_b.column(0), T.T_STRING)[0]
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], T.T_STRING, 0, ch["max_def"], 0, ch["codec"], device=True)
    col = pc.decode()
    valid = _valid_of(col, pc.info)
    got = _col_values(col, T.T_STRING, pc.info.num_values, valid)
    assert got == exp
    assert col.n_buffers == 2
    w = col.data.to_numpy(np.uint32, 4 * len(exp)).reshape(-1, 4)
    assert set(int(x) for x in w[w[:, 0] > 12, 2]) == {0, 1}      # long views into the chunk (buffer 0) and into the arena (buffer 1)
    # an operator that resolves views through the column's buffer table: equality against the same strings built on the host
    ref = gpu.Column.strings([v if v is not None else b"" for v in exp], validity=np.array([v is not None for v in exp]))
    eq = gpu.cmp(T.CMP_EQ, col, ref).to_numpy()
    assert eq[valid].all()
    other = gpu.Column.strings([(v or b"") + b"!" for v in exp])
    assert not gpu.cmp(T.CMP_EQ, col, other).to_numpy()[valid].any()
    pc.close()


# ---- List<String> ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc", ["DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"])
@pytest.mark.parametrize("codec", ["none", "snappy"])
def test_list_of_strings(gpu, enc, codec):
    import pyarrow as pa
    rng = np.random.default_rng(4)
    rows = [None if rng.random() < 0.1 else
            [None if rng.random() < 0.1 else "prefix/shared/" + "z" * int(x % 20) + str(int(x)) for x in rng.integers(0, 1000, int(rng.integers(0, 6)))]
            for _ in range(5000)]
    chunks, back = _write(pa.table({"c": pa.array(rows, pa.list_(pa.string()))}), enc, codec, page_size=8 * 1024, col="c.list.element")
    ch = chunks[0]
    assert enc in ch["encodings"]
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], T.T_STRING, 0, codec=ch["codec"], device=True, list_of=(True, True))
    offs, lval, col = pc.decode_list()
    ev = np.unpackbits(col.validity.to_numpy(np.uint8, (pc.elems + 7) // 8), bitorder="little")[:pc.elems].astype(bool)
    vals = _col_values(col, T.T_STRING, pc.elems, ev)
    got = [None if not lval[r] else vals[int(offs[r]):int(offs[r + 1])] for r in range(pc.rows)]
    exp = [None if r is None else [None if v is None else v.encode() for v in r] for r in back.column(0).to_pylist()]
    assert got == exp
    pc.close()


# ---- one batch over several chunks -------------------------------------------------------------------------------------------------
def test_batch_of_mixed_chunks(gpu):
    import pyarrow as pa
    rng = np.random.default_rng(6)
    cases = []
    s = sorted(f"item-{int(x):08d}-" + "q" * int(x % 17) for x in rng.integers(0, 10**8, 40_000))
    for enc in ("DELTA_BYTE_ARRAY", "PLAIN", "DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"):
        chunks, back = _write(pa.table({"c": pa.array(s, pa.string(), mask=rng.random(len(s)) < 0.03)}), enc if enc != "PLAIN" else None, "zstd",
                              page_size=16 * 1024)
        cases.append((chunks[0], back, T.T_STRING))
    f = rng.standard_normal(50_000)
    chunks, back = _write(pa.table({"c": pa.array(f)}), "BYTE_STREAM_SPLIT", "lz4")
    cases.append((chunks[0], back, T.T_F64))
    chunks, back = _write(pa.table({"c": pa.array(rng.integers(0, 1000, 30_000))}), None, "zstd", dictionary=True)
    cases.append((chunks[0], back, T.T_I64))
    pcs = [gpu.ParquetChunk(ch["chunk"], ch["physical"], ot, ch["type_length"], ch["max_def"], 0, ch["codec"], device=True) for ch, _, ot in cases]
    st = []
    cols = gpu.ParquetChunk.decode_many(pcs, statuses=st)
    assert st == [0] * len(cases)
    for (ch, back, ot), pc, col in zip(cases, pcs, cols):
        exp, exp_valid = PU.expected_of(back.column(0), ot)
        valid = _valid_of(col, pc.info)
        assert np.array_equal(valid, exp_valid)
        assert _col_values(col, ot, pc.info.num_values, valid) == exp
    assert [c.n_buffers for c in cols[:4]] == [2, 1, 1, 2]
    for pc in pcs:
        pc.close()


# ---- the arena changes hands ---------------------------------------------------------------------------------------------------------
def test_arena_hand_over(gpu):
    import pyarrow as pa
    rng = np.random.default_rng(8)
    vals = sorted(f"/data/warehouse/table-{int(x):06d}/part-{int(x) % 97:05d}.parquet" for x in rng.integers(0, 10**6, 20_000))
    chunks, back = _write(pa.table({"c": pa.array(vals, pa.string())}), "DELTA_BYTE_ARRAY", "snappy")
    ch = chunks[0]
    exp = PU.expected_of(back.column(0), T.T_STRING)[0]
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], T.T_STRING, 0, ch["max_def"], 0, ch["codec"], device=True)
    lib = T.lib()
    info = pc.info
    out = gpu.DeviceBuffer(info.out_bytes + 16)
    img = pc.image_dev = gpu.DeviceBuffer(info.image_bytes)
    chunk_dev = pc.upload()

    val = gpu.DeviceBuffer(info.validity_bytes + 8)

    def decode_raw():
        nulls = C.c_int64()
        T.check(lib.dbhip_pq_chunk_decode_device(pc.h, C.c_void_p(chunk_dev.ptr), C.c_void_p(img.ptr), C.c_void_p(out.ptr),
                                                 C.c_void_p(val.ptr) if info.has_validity else None, C.byref(nulls), None))
        return out.to_numpy(np.uint8, 16 * info.num_values).reshape(-1, 16)

    def take():
        p, nb = C.c_void_p(), C.c_int64()
        T.check(lib.dbhip_pq_chunk_take_arena(pc.h, C.byref(p), C.byref(nb)))
        return p.value, nb.value

    views = decode_raw()
    p1, n1 = take()
    assert p1 and n1 == sum(len(v) for v in exp)
    assert take() == (None, 0)                       # a second take: nothing
    # a second decode without a take makes a new arena (the old one now belongs to the caller); its views point into the new one
    views2 = decode_raw()
    assert np.array_equal(views, views2)
    pc2_arena = gpu.DeviceBuffer.adopt(*take())
    assert pc2_arena.ptr and pc2_arena.ptr != p1
    a1 = gpu.DeviceBuffer.adopt(p1, n1)
    img_host = img.to_numpy(np.uint8, info.image_bytes)
    assert _resolve_strings(views, np.ones(len(exp), bool), [img_host, a1.to_numpy(np.uint8, n1)]) == exp
    assert _resolve_strings(views2, np.ones(len(exp), bool), [img_host, pc2_arena.to_numpy(np.uint8, n1)]) == exp
    # decode through the binding, take, close the handle: the column still reads back
    col = pc.decode()
    pc.close()
    assert _col_values(col, T.T_STRING, len(exp), np.ones(len(exp), bool)) == exp
    a1.free()
    pc2_arena.free()


# ---- malformed pages: every device-side check ------------------------------------------------------------------------------------
def _dbp(vals):
    """DELTA_BINARY_PACKED (Encodings.md) of python ints: block 128, 4 miniblocks of 32"""
    def uv(v):
        return PU._varint(v)

    def zz(v):
        return PU._varint((v << 1) ^ (v >> 63) if v < 0 else v << 1)
    out = bytearray(uv(128) + uv(4) + uv(len(vals)) + zz(vals[0] if vals else 0))
    deltas = [vals[i] - vals[i - 1] for i in range(1, len(vals))]
    for b0 in range(0, len(deltas), 128):
        blk = deltas[b0:b0 + 128]
        md = min(blk)
        out += zz(md)
        minis = [blk[m * 32:(m + 1) * 32] for m in range(4)]
        widths = [max((d - md).bit_length() for d in mb) if mb else 0 for mb in minis]
        out += bytes(widths)
        for mb, w in zip(minis, widths):
            if not mb:
                break
            acc, nbits = 0, 0
            for k in range(32):
                acc |= ((mb[k] - md) if k < len(mb) else 0) << nbits
                nbits += w
            out += acc.to_bytes((32 * w) // 8, "little")
    return bytes(out)


def _dba_page(prefix, suffix_bytes, suffix_lens=None):
    sl = [len(s) for s in suffix_bytes] if suffix_lens is None else suffix_lens
    return _dbp(prefix) + _dbp(sl) + b"".join(suffix_bytes)


def _raw(payload, n, enc, phys, tl=0):
    return dict(chunk=PU.raw_page_chunk(payload, len(payload), n, encoding=enc), codec=0, physical=phys, type_length=tl, max_def=0)


def _status(gpu, ch, ot):
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], ot, ch["type_length"], 0, 0, 0, device=True)
    st = []
    cols = gpu.ParquetChunk.decode_many([pc], statuses=st)
    vals = _col_values(cols[0], ot, pc.info.num_values, np.ones(pc.info.num_values, bool)) if st[0] == 0 else None
    pc.close()
    return st[0], vals


def test_malformed_pages_are_invalid(gpu):
    BA, FL = PU.PHYS["BYTE_ARRAY"], PU.PHYS["FIXED_LEN_BYTE_ARRAY"]
    words = [b"apple", b"applesauce", b"apricot", b"banana", b"band", b""]
    good_prefix = [0, 5, 2, 0, 3, 0]
    good_suffix = [b"apple", b"sauce", b"ricot", b"banana", b"d", b""]
    ok = _raw(_dba_page(good_prefix, good_suffix), 6, 7, BA)
    assert _status(gpu, ok, T.T_STRING) == (0, words)
    bad = {
        "prefix[0] > 0": _raw(_dba_page([1, 5, 2, 0, 3, 0], [b"pple", b"sauce", b"ricot", b"banana", b"d", b""]), 6, 7, BA),
        "prefix longer than the previous value": _raw(_dba_page([0, 6, 2, 0, 3, 0], good_suffix), 6, 7, BA),
        "negative length": _raw(_dba_page([0, 5, 2, 0, 3, 0], good_suffix, [5, 5, 5, -1, 1, 0]), 6, 7, BA),
        "suffix section short": _raw(_dba_page(good_prefix, good_suffix)[:-3], 6, 7, BA),
        "prefix stream count": _raw(_dbp(good_prefix[:5]) + _dbp([len(s) for s in good_suffix]) + b"".join(good_suffix), 6, 7, BA),
        "suffix stream count": _raw(_dbp(good_prefix) + _dbp([len(s) for s in good_suffix] + [0]) + b"".join(good_suffix), 6, 7, BA),
        "DLBA negative length": _raw(_dbp([3, -2]) + b"abc", 2, 6, BA),
        "DLBA bytes short": _raw(_dbp([3, 20]) + b"abcdefgh", 2, 6, BA),
        "DLBA count": _raw(_dbp([3, 2, 1]) + b"abcdef", 2, 6, BA),
    }
    for what, ch in bad.items():
        assert _status(gpu, ch, T.T_STRING)[0] == T.ERR_INVALID, what
    # FIXED_LEN_BYTE_ARRAY(4): a value whose length is not type_length
    fl_ok = _raw(_dba_page([0, 2, 4], [b"\x00\x00\x01\x02", b"\x03\x04", b""]), 3, 7, FL, 4)
    assert _status(gpu, fl_ok, T.T_DEC64) == (0, [0x0102, 0x0304, 0x0304])
    fl_bad = _raw(_dba_page([0, 2, 4], [b"\x00\x00\x01\x02", b"\x03", b""]), 3, 7, FL, 4)
    assert _status(gpu, fl_bad, T.T_DEC64)[0] == T.ERR_INVALID
    # BYTE_STREAM_SPLIT page shorter than n * w
    bss = _raw(struct.pack("<4i", 1, 2, 3, 4)[:15], 4, 9, PU.PHYS["INT32"])
    assert _status(gpu, bss, T.T_I32)[0] == T.ERR_INVALID
    bss_ok = _raw(bytes([1, 2, 0, 0, 0, 0, 0, 0]), 2, 9, PU.PHYS["INT32"])
    assert _status(gpu, bss_ok, T.T_I32) == (0, [1, 2])
    # after all of them, a valid decode still succeeds
    assert _status(gpu, ok, T.T_STRING) == (0, words)


# ---- size --------------------------------------------------------------------------------------------------------------------------
def test_20m_row_delta_byte_array_zstd(gpu):
    import pyarrow as pa
    import pyarrow.compute as pc_
    n = 20_000_000
    ids = pa.array(np.arange(n, dtype=np.int64) * 7919 % 10**9).cast(pa.string())
    arr = pc_.binary_join_element_wise("https://warehouse.example/orders/", ids, "")
    arr = pc_.if_else(pa.array(np.arange(n) % 11 == 0), pa.scalar("k"), arr)        # short values between the long ones
    chunks, back = _write(pa.table({"c": arr}), "DELTA_BYTE_ARRAY", "zstd", v2=True, page_size=1024 * 1024)
    ch = chunks[0]
    pc = gpu.ParquetChunk(ch["chunk"], ch["physical"], T.T_STRING, 0, ch["max_def"], 0, ch["codec"], device=True)
    col = pc.decode()
    assert col.n_buffers == 2
    views = col.data.to_numpy(np.uint32, 4 * n).reshape(-1, 4)
    exp = back.column(0).combine_chunks()
    eoff = np.frombuffer(exp.buffers()[1], dtype=np.int32)[:n + 1].astype(np.int64)
    edata = np.frombuffer(exp.buffers()[2], dtype=np.uint8)
    lens = views[:, 0].astype(np.int64)
    assert np.array_equal(lens, np.diff(eoff))
    arena = col._keep[1].to_numpy(np.uint8, col._keep[1].nbytes)
    long_ = lens > 12
    assert (views[long_, 2] == 1).all()
    # every long value: its bytes in the arena equal pyarrow's (a million rows at a time)
    for r0 in range(0, n, 1_000_000):
        sel = np.nonzero(long_[r0:r0 + 1_000_000])[0] + r0
        L = lens[sel]
        starts = np.cumsum(L) - L
        idx = np.repeat(views[sel, 3].astype(np.int64) - starts, L) + np.arange(int(L.sum()))
        eidx = np.repeat(eoff[sel] - starts, L) + np.arange(int(L.sum()))
        assert np.array_equal(arena[idx], edata[eidx]), r0
    # inline values: the 12 bytes of the view
    short = np.nonzero(~long_)[0]
    inl = views[short, 1:4].copy().view(np.uint8).reshape(-1, 12)
    for j in range(12):
        has = lens[short] > j
        assert np.array_equal(inl[has, j], edata[eoff[short[has]] + j])
        assert not inl[~has, j].any()
    pc.close()
