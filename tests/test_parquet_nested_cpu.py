"""Nested Parquet leaves at dbhip_pq_chunk_open_device_nested (no device needed: open reads the thrift page headers only). pyarrow writes
the chunks (the independent writer). Open accepts every shape the GPU suite decodes, refuses descriptors beyond the limits and malformed
ones, and the host-mode open keeps refusing nested leaves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import parquet_nested_util as NU
from tests import parquet_util as PU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = NU.shapes()


@pytest.mark.parametrize("variant", sorted(NU.VARIANTS))
@pytest.mark.parametrize("codec", NU.CODECS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_open_accepts_every_shape(shape, codec, variant):
    v2, dictionary = NU.VARIANTS[variant]
    spec = SHAPES[shape]
    chunks, _ = NU.write_shape(spec, 600, seed=len(shape), codec=codec, v2=v2, dictionary=dictionary)
    lv = NU.leaves(spec)
    assert len(chunks) == len(lv)
    for ch, (path, ln, kind) in zip(chunks, lv):
        R = sum(1 for k, _, _ in path if k == "list")
        assert ch["max_rep"] == R and ch["max_def"] == sum(n for _, n, _ in path) + R + ln, (ch["name"], path)
        rc, info = NU.open_nested(ch, NU.node_tuples(path), ln, NU.LEAF_KINDS[kind])
        assert rc == T.OK, (ch["name"], T.lib().dbhip_last_error())
        assert info.num_values == ch["num_values"]          # level entries
        assert info.has_validity == ln
        es = 1 if kind == "bool" else PU.ESIZE[NU.LEAF_KINDS[kind]]
        if kind == "bool":
            assert info.out_bytes == (ch["num_values"] + 63) // 64 * 8
        else:
            assert info.out_bytes == ch["num_values"] * es
        assert info.validity_bytes == (ch["num_values"] + 63) // 64 * 8


def _list_list_chunk(codec="none"):
    chunks, _ = NU.write_shape(SHAPES["list_list_i64_111"], 300, seed=3, codec=codec, v2=False, dictionary=False)
    return chunks[0]


@pytest.mark.parametrize("path,code", [
    ([], T.ERR_UNSUPPORTED),
    ([("struct", 0)] * 9, T.ERR_UNSUPPORTED),
    ([("list", 1)] * 5, T.ERR_UNSUPPORTED),
    ([("list", 1), (0, 1)], T.ERR_INVALID),
    ([("list", 1), (3, 1)], T.ERR_INVALID),
    ([("list", 2), ("list", 1)], T.ERR_INVALID),
])
def test_open_refuses_bad_descriptors(path, code):
    ch = _list_list_chunk()
    rc, _ = NU.open_nested(ch, path, 1, T.T_I64)
    assert rc == code, T.lib().dbhip_last_error()


def test_open_refuses_a_null_path():
    ch = _list_list_chunk()
    data = ch["chunk"]
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    h, info = C.c_void_p(), T.PqInfo()
    rc = T.lib().dbhip_pq_chunk_open_device_nested(buf, C.c_int64(len(data)), 0, ch["physical"], 0, None, 2, 1, T.T_I64, C.byref(h), C.byref(info))
    assert rc == T.ERR_INVALID


@pytest.mark.parametrize("def_enc,rep_enc", [(4, 3), (3, 4), (4, 4)])
def test_open_refuses_v1_levels_that_are_not_rle(def_enc, rep_enc):
    page = NU.v1_levels_page([0, 2, 1], [4, 4, 4], [1, 2, 3], def_enc=def_enc, rep_enc=rep_enc)
    ch = dict(chunk=page, codec=0, physical=2, type_length=0)
    rc, _ = NU.open_nested(ch, [("list", 1), ("list", 1)], 1, T.T_I64)
    assert rc == T.ERR_UNSUPPORTED
    rc, _ = NU.open_nested(ch, [("list", 1), ("list", 1)], 1, T.T_I64, data=NU.v1_levels_page([0, 2, 1], [4, 4, 4], [1, 2, 3]))
    assert rc == T.OK       # (the same page with RLE levels)


def test_open_refuses_what_the_flat_open_refuses():
    import pyarrow as pa
    rng = np.random.default_rng(5)
    rows = [[[int(x) for x in rng.integers(0, 100, 2)]] for _ in range(200)]
    typ = NU.arrow_type(SHAPES["list_list_i64_111"])
    table = pa.table({"c": pa.array(rows, type=typ)})
    path = [("list", 1), ("list", 1)]
    # an (encoding, physical) pair the flat open refuses: BYTE_STREAM_SPLIT is fine for INT64, DELTA_LENGTH_BYTE_ARRAY is not written for it,
    # so the refused pair is built from an accepted chunk opened as a type it cannot become
    chunks, _ = NU.write_table(table, "none", False, False)
    ch = chunks[0]
    for ot in (T.T_STRING, T.T_BOOL, T.T_F64, T.T_I32):
        rc, _ = NU.open_nested(ch, path, 1, ot)
        assert rc == T.ERR_UNSUPPORTED, ot
    # GZIP pages
    chunks, _ = NU.write_table(table, "gzip", False, False)
    rc, _ = NU.open_nested(chunks[0], path, 1, T.T_I64)
    assert rc == T.ERR_UNSUPPORTED
    # a value encoding the device does not decode (DELTA_BINARY_PACKED on a BYTE_ARRAY page, by hand: encoding 5 in the page header)
    payload = b"\x02\x00\x00\x00\x02\x00" + b"\x02\x00\x00\x00\x02\x01" + b"\x00" * 8
    ch2 = dict(chunk=NU.v1_page(1, payload, encoding=5), codec=0, physical=6, type_length=0)
    rc, _ = NU.open_nested(ch2, [("list", 0)], 0, T.T_STRING)
    assert rc == T.ERR_UNSUPPORTED
    # the same page as PLAIN is accepted
    ch2 = dict(chunk=NU.v1_page(1, payload, encoding=0), codec=0, physical=6, type_length=0)
    rc, _ = NU.open_nested(ch2, [("list", 0)], 0, T.T_STRING)
    assert rc == T.OK


def test_host_mode_open_refuses_a_rep_2_leaf():
    ch = _list_list_chunk()
    data = ch["chunk"]
    buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    h, info = C.c_void_p(), T.PqInfo()
    rc = T.lib().dbhip_pq_chunk_open(buf, C.c_int64(len(data)), 0, ch["physical"], 0, ch["max_def"], ch["max_rep"], T.T_I64, C.byref(h), C.byref(info))
    assert rc == T.ERR_UNSUPPORTED
    # and the flat device open likewise
    rc = T.lib().dbhip_pq_chunk_open_device(buf, C.c_int64(len(data)), 0, ch["physical"], 0, ch["max_def"], ch["max_rep"], T.T_I64, C.byref(h), C.byref(info))
    assert rc == T.ERR_UNSUPPORTED


def test_bit_flip_targets_are_accepted_by_open():
    """the malformed-input test of the GPU suite flips bits inside the level streams of a v1 List<List<Int64>> chunk; open reads page
    headers only, so every such mutant must still open (a refusal would mean the flip missed the level streams)"""
    import pyarrow as pa
    chunks, _ = NU.write_shape(SHAPES["list_list_i64_111"], 20_000, seed=17, codec="none", v2=False, dictionary=False)
    ch = chunks[0]
    ranges = NU.v1_level_ranges(ch["chunk"])
    assert len(ranges) >= 2 * 10
    rng = np.random.default_rng(60)
    for k in range(60):
        a, b = ranges[int(rng.integers(0, len(ranges)))]
        pos = int(rng.integers(a, b))
        m = bytearray(ch["chunk"])
        m[pos] ^= 1 << int(rng.integers(0, 8))
        rc, _ = NU.open_nested(ch, [("list", 1), ("list", 1)], 1, T.T_I64, data=bytes(m))
        assert rc == T.OK, (k, pos)


def _rust_fields(name):
    text = open(os.path.join(ROOT, "bindings", "dbhip_sys.rs")).read()
    m = re.search(r"pub struct " + name + r" \{(.*?)\}", text, flags=re.S)
    return [(f, t.strip()) for f, t in re.findall(r"pub (\w+): ([^,]+),", m.group(1))]


def test_rust_node_structs_match_the_ctypes_mirrors():
    rust_of = {C.c_int32: "i32", C.c_int64: "i64"}
    for rname, py in (("dbhip_pq_node", T.PqNode), ("dbhip_pq_node_out", T.PqNodeOut)):
        rf = _rust_fields(rname)
        assert [f for f, _ in rf] == [f for f, _ in py._fields_], rname
        for (f, rt), (_, ct) in zip(rf, py._fields_):
            if ct is C.c_void_p:
                assert rt.startswith("*mut "), (rname, f, rt)
            else:
                assert rust_of[ct] == rt, (rname, f, rt)
    assert C.sizeof(T.PqNode) == 8 and C.sizeof(T.PqNodeOut) == 32
