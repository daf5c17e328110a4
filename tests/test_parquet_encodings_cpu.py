"""DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY and BYTE_STREAM_SPLIT data pages at dbhip_pq_chunk_open_device / _open_device_list (no device
needed: open reads the thrift page headers only). pyarrow writes the chunks (the independent writer); the pairs the device decodes are
accepted, every other (encoding, physical type) pair and the host-mode open keep refusing."""
import ctypes as C
import io

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import parquet_util as PU

CODECS = ["none", "snappy", "lz4", "zstd"]


def _columns():
    """(name, pyarrow array builder(n, rng, nullable), out_type, encodings that apply)"""
    import pyarrow as pa
    from decimal import Decimal

    def strs(n, rng, mask):
        return pa.array([f"key-{int(x):08d}-{'x' * int(x % 23)}" for x in rng.integers(0, 10**6, n)], pa.string(), mask=mask)

    def dec(p, s):
        def mk(n, rng, mask):
            v = [Decimal(int(x)).scaleb(-s) for x in rng.integers(-10**12, 10**12, n)]
            return pa.array(v, pa.decimal128(p, s), mask=mask)
        return mk

    return [
        ("string", strs, T.T_STRING, ("DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY")),
        ("dec15_2", dec(15, 2), T.T_DEC128, ("DELTA_BYTE_ARRAY", "BYTE_STREAM_SPLIT")),
        ("dec38_6", dec(38, 6), T.T_DEC128, ("DELTA_BYTE_ARRAY", "BYTE_STREAM_SPLIT")),
        ("f32", lambda n, rng, m: pa.array(rng.standard_normal(n).astype(np.float32), pa.float32(), mask=m), T.T_F32, ("BYTE_STREAM_SPLIT",)),
        ("f64", lambda n, rng, m: pa.array(rng.standard_normal(n), pa.float64(), mask=m), T.T_F64, ("BYTE_STREAM_SPLIT",)),
        ("i32", lambda n, rng, m: pa.array(rng.integers(-2**31, 2**31, n), pa.int32(), mask=m), T.T_I32, ("BYTE_STREAM_SPLIT",)),
        ("i64", lambda n, rng, m: pa.array(rng.integers(-2**62, 2**62, n), pa.int64(), mask=m), T.T_I64, ("BYTE_STREAM_SPLIT",)),
    ]


def _write(arr, encoding, codec, v2, page_size=4096):
    import pyarrow as pa
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    kw = dict(compression=codec, use_dictionary=False, write_statistics=False, data_page_version="2.0" if v2 else "1.0",
              row_group_size=max(len(arr), 1), store_schema=False, data_page_size=page_size)
    if encoding != "PLAIN":
        kw["column_encoding"] = {"c": encoding}
    pq.write_table(pa.table({"c": arr}), buf, **kw)
    chunks, _ = PU.column_chunks(buf.getvalue())
    return chunks[0]


def _open(ch, out_type, device=True, max_def=None):
    data = ch["chunk"]
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    h, info = C.c_void_p(), T.PqInfo()
    fn = T.lib().dbhip_pq_chunk_open_device if device else T.lib().dbhip_pq_chunk_open
    rc = fn(buf, C.c_int64(len(data)), ch["codec"], ch["physical"], ch["type_length"], ch["max_def"] if max_def is None else max_def, 0, out_type,
            C.byref(h), C.byref(info))
    if rc == 0:
        T.lib().dbhip_pq_chunk_close(h)
    return rc, info


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("v2", [False, True])
@pytest.mark.parametrize("nullable", [False, True])
def test_open_device_accepts_the_new_encodings(codec, v2, nullable):
    rng = np.random.default_rng(11)
    n = 3000
    for name, mk, ot, encs in _columns():
        mask = (rng.random(n) < 0.1) if nullable else None
        arr = mk(n, rng, mask)
        plain = _write(arr, "PLAIN", codec, v2)
        rc_p, info_p = _open(plain, ot)
        assert rc_p == T.OK, (name, T.lib().dbhip_last_error())
        for enc in encs:
            ch = _write(arr, enc, codec, v2)
            assert enc in ch["encodings"], (name, enc, ch["encodings"])
            rc, info = _open(ch, ot)
            assert rc == T.OK, (name, enc, T.lib().dbhip_last_error())
            assert info.num_values == info_p.num_values == n
            assert info.n_pages >= 1 and info.out_bytes == info_p.out_bytes and info.has_validity == info_p.has_validity
            assert (info.image_bytes == 0) == (codec == "none")
            if enc == "BYTE_STREAM_SPLIT":    # the same bytes per value as PLAIN: the same pages
                assert info.n_pages == info_p.n_pages and info.image_bytes == info_p.image_bytes, (name, codec)
            # the host-mode open keeps refusing every such chunk
            rc_h, _ = _open(ch, ot, device=False)
            assert rc_h == T.ERR_UNSUPPORTED, (name, enc)


@pytest.mark.parametrize("enc", ["DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"])
@pytest.mark.parametrize("codec", CODECS)
def test_open_device_list_accepts_string_leaves(enc, codec):
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(3)
    rows = [None if rng.random() < 0.1 else [None if rng.random() < 0.1 else f"v{int(x)}" * int(x % 5) for x in rng.integers(0, 100, int(rng.integers(0, 5)))]
            for _ in range(2000)]
    t = pa.table({"c": pa.array(rows, pa.list_(pa.string()))})
    buf = io.BytesIO()
    pq.write_table(t, buf, compression=codec, use_dictionary=False, write_statistics=False, column_encoding={"c.list.element": enc}, data_page_size=4096,
                   store_schema=False)
    chunks, _ = PU.column_chunks(buf.getvalue())
    ch = chunks[0]
    assert enc in ch["encodings"]
    data = ch["chunk"]
    cbuf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    h, info = C.c_void_p(), T.PqInfo()
    rc = T.lib().dbhip_pq_chunk_open_device_list(cbuf, C.c_int64(len(data)), C.c_int32(ch["codec"]), C.c_int32(ch["physical"]), C.c_int32(0),
                                                 C.c_int32(1), C.c_int32(1), C.c_int32(T.T_STRING), C.byref(h), C.byref(info))
    assert rc == T.OK, T.lib().dbhip_last_error()
    assert info.num_values == ch["num_values"]
    T.lib().dbhip_pq_chunk_close(h)


def test_illegal_pairs_still_refused():
    payload = bytes(64)
    for phys, ot, tl, enc in ((PU.PHYS["INT32"], T.T_I32, 0, 7),            # DELTA_BYTE_ARRAY on INT32
                              (PU.PHYS["INT64"], T.T_I64, 0, 6),            # DELTA_LENGTH_BYTE_ARRAY on INT64
                              (PU.PHYS["FIXED_LEN_BYTE_ARRAY"], T.T_DEC128, 16, 6),
                              (PU.PHYS["BOOLEAN"], T.T_BOOL, 0, 9),         # BYTE_STREAM_SPLIT on BOOLEAN
                              (PU.PHYS["BYTE_ARRAY"], T.T_STRING, 0, 9),    # ... and on BYTE_ARRAY
                              (PU.PHYS["INT32"], T.T_I32, 0, 4),            # BIT_PACKED values
                              (PU.PHYS["BYTE_ARRAY"], T.T_STRING, 0, 5)):   # DELTA_BINARY_PACKED on BYTE_ARRAY
        ch = dict(chunk=PU.raw_page_chunk(payload, len(payload), 4, encoding=enc), codec=0, physical=phys, type_length=tl, max_def=0)
        rc, _ = _open(ch, ot)
        assert rc == T.ERR_UNSUPPORTED, (phys, enc)
    # the legal pairs in the same hand-built form pass open (the payload is only looked at on the device)
    for phys, ot, tl, enc in ((PU.PHYS["INT32"], T.T_I32, 0, 9), (PU.PHYS["BYTE_ARRAY"], T.T_STRING, 0, 7), (PU.PHYS["BYTE_ARRAY"], T.T_STRING, 0, 6),
                              (PU.PHYS["FIXED_LEN_BYTE_ARRAY"], T.T_DEC128, 16, 7), (PU.PHYS["DOUBLE"], T.T_F64, 0, 9)):
        ch = dict(chunk=PU.raw_page_chunk(payload, len(payload), 4, encoding=enc), codec=0, physical=phys, type_length=tl, max_def=0)
        rc, _ = _open(ch, ot)
        assert rc == T.OK, (phys, enc, T.lib().dbhip_last_error())
        rc_h, _ = _open(ch, ot, device=False)
        assert rc_h == T.ERR_UNSUPPORTED


def test_take_arena_is_declared_and_empty_after_open():
    """dbhip_pq_chunk_take_arena: exported, and NULL / 0 on a handle no decode has materialised anything for"""
    assert "dbhip_pq_chunk_take_arena" in T.SYMBOLS
    ch = dict(chunk=PU.raw_page_chunk(bytes(64), 64, 4, encoding=7), codec=0, physical=PU.PHYS["BYTE_ARRAY"], type_length=0, max_def=0)
    data = ch["chunk"]
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    h, info = C.c_void_p(), T.PqInfo()
    T.check(T.lib().dbhip_pq_chunk_open_device(buf, C.c_int64(len(data)), 0, ch["physical"], 0, 0, 0, T.T_STRING, C.byref(h), C.byref(info)))
    p, nb = C.c_void_p(123), C.c_int64(7)
    T.check(T.lib().dbhip_pq_chunk_take_arena(h, C.byref(p), C.byref(nb)))
    assert not p.value and nb.value == 0
    T.lib().dbhip_pq_chunk_close(h)
