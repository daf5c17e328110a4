"""Test plumbing for nested Parquet leaves (dbhip_pq_chunk_open_device_nested / _decode_device_nested): the shapes the tests write with
pyarrow (the independent writer and reader), the path of each leaf, what pyarrow's own reading of the file says every node of that path
holds, a hand-written v1 page builder and a reader of the thrift page headers (to find the level streams of a chunk)."""
import io
import struct

import numpy as np

from databend_amd import _lib as T
from tests import parquet_util as PU

CODECS = ["none", "snappy", "lz4", "zstd"]
# (v2, dictionary): v1 + PLAIN and v2 + dictionary
VARIANTS = {"v1_plain": (False, False), "v2_dict": (True, True)}


# ---- shapes: a small type language -> pyarrow type, random rows, and the leaves with their paths ---------------------------------
# ("list", nullable, child) | ("struct", nullable, [(name, child), ..]) | ("map", nullable, key, value) | ("leaf", nullable, kind)
LEAF_KINDS = {"i64": T.T_I64, "i32": T.T_I32, "i16": T.T_I16, "str": T.T_STRING, "bool": T.T_BOOL, "dec": T.T_DEC128}


def arrow_type(spec):
    import pyarrow as pa
    k = spec[0]
    if k == "leaf":
        return {"i64": pa.int64(), "i32": pa.int32(), "i16": pa.int16(), "str": pa.string(), "bool": pa.bool_(), "dec": pa.decimal128(38, 6)}[spec[2]]
    if k == "list":
        return pa.list_(pa.field("item", arrow_type(spec[2]), nullable=bool(spec[2][1])))
    if k == "struct":
        return pa.struct([pa.field(n, arrow_type(c), nullable=bool(c[1])) for n, c in spec[2]])
    assert k == "map"
    return pa.map_(arrow_type(spec[2]), pa.field("value", arrow_type(spec[3]), nullable=bool(spec[3][1])))


def gen_value(rng, spec, p_null=0.15, max_len=3):
    from decimal import Decimal
    if spec[1] and rng.random() < p_null:
        return None
    k = spec[0]
    if k == "leaf":
        kind = spec[2]
        if kind == "i64":
            return int(rng.integers(-2**62, 2**62))
        if kind == "i32":
            return int(rng.integers(-2**31, 2**31))
        if kind == "i16":
            return int(rng.integers(-2**15, 2**15))
        if kind == "bool":
            return bool(rng.integers(0, 2))
        if kind == "str":
            return "v%06d-" % int(rng.integers(0, 10**6)) + "x" * int(rng.integers(0, 20))   # 8 .. 27 bytes: inline and long views
        return Decimal(int(rng.integers(-10**15, 10**15))).scaleb(-6)
    if k == "list":
        return [gen_value(rng, spec[2], p_null, max_len) for _ in range(int(rng.integers(0, max_len + 1)))]
    if k == "struct":
        return {n: gen_value(rng, c, p_null, max_len) for n, c in spec[2]}
    return [(gen_value(rng, spec[2], p_null, max_len), gen_value(rng, spec[3], p_null, max_len)) for _ in range(int(rng.integers(0, max_len + 1)))]


def leaves(spec, path=()):
    """-> [(path [(kind, nullable, member)], leaf_nullable, leaf kind)] in the column order of the Parquet schema"""
    k = spec[0]
    if k == "leaf":
        return [(list(path), int(spec[1]), spec[2])]
    if k == "list":
        return leaves(spec[2], path + (("list", int(spec[1]), None),))
    if k == "struct":
        out = []
        for n, c in spec[2]:
            out += leaves(c, path + (("struct", int(spec[1]), n),))
        return out
    base = path + (("list", int(spec[1]), None),)
    return leaves(spec[2], base + (("struct", 0, "key"),)) + leaves(spec[3], base + (("struct", 0, "value"),))


def L(n, c):
    return ("list", n, c)


def leaf(n, kind):
    return ("leaf", n, kind)


def shapes():
    """name -> (spec of the column, the column's own nullability is spec[1])"""
    out = {}
    for ln in (0, 1):
        for mn in (0, 1):
            for en in (0, 1):
                out[f"list_list_i64_{ln}{mn}{en}"] = L(ln, L(mn, leaf(en, "i64")))
    out["list3_i32"] = L(1, L(1, L(0, leaf(1, "i32"))))
    out["list4_i16"] = L(1, L(0, L(1, L(1, leaf(1, "i16")))))
    out["tuple5"] = ("struct", 1, [("a", leaf(1, "i64")), ("b", leaf(1, "str")), ("c", leaf(1, "bool")), ("d", leaf(1, "dec")), ("e", leaf(0, "i32"))])
    out["tuple_tuple"] = ("struct", 1, [("inner", ("struct", 1, [("x", leaf(1, "i64")), ("y", leaf(0, "i32"))]))])
    out["list_tuple"] = L(1, ("struct", 1, [("a", leaf(1, "i64")), ("b", leaf(1, "str"))]))
    out["tuple_list"] = ("struct", 1, [("l", L(1, leaf(1, "i64")))])
    out["map_str_list_i64"] = ("map", 1, leaf(0, "str"), L(1, leaf(1, "i64")))
    return out


def write_shape(spec, n_rows, seed, codec, v2, dictionary, page_size=4096, encoding=None):
    """-> (column chunks of row group 0, pyarrow's reading of the column as one array)"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    rng = np.random.default_rng(seed)
    rows = [gen_value(rng, spec) for _ in range(n_rows)]
    typ = arrow_type(spec)
    table = pa.Table.from_arrays([pa.array(rows, type=typ)], schema=pa.schema([pa.field("c", typ, nullable=bool(spec[1]))]))
    return write_table(table, codec, v2, dictionary, page_size, encoding)


def write_table(table, codec, v2, dictionary, page_size=4096, encoding=None):
    import pyarrow.parquet as pq
    buf = io.BytesIO()
    kw = dict(compression=codec, use_dictionary=dictionary, write_statistics=False, data_page_version="2.0" if v2 else "1.0",
              row_group_size=max(table.num_rows, 1), store_schema=False, data_page_size=page_size)
    if encoding:
        kw["column_encoding"] = encoding
    pq.write_table(table, buf, **kw)
    data = buf.getvalue()
    chunks, _ = PU.column_chunks(data)
    back = pq.read_table(io.BytesIO(data)).column(0).combine_chunks()
    return chunks, back


def node_tuples(path):
    """path as decode_nested takes it"""
    return [(k, n) for k, n, _ in path]


# ---- what pyarrow's reading says every node holds -----------------------------------------------------------------------------
# The VALUE of a required member in a slot under a NULL STRUCT ancestor (in the same index space) is not defined in Arrow's format:
# pyarrow's reader leaves there whatever its buffer held (values of other rows). Those values are compared with the decode's contract,
# zero bytes; everything else — offsets, every validity bit, every other value — with pyarrow, bit for bit.
def expected_nodes(arr, path):
    """-> ([(offsets u64 or None, validity bool or None, items, undefined bool)] per node, the leaf's pyarrow array, the leaf's undefined
    mask); undefined: the slot has a NULL STRUCT ancestor in its own index space"""
    nodes = []
    cur = arr
    under_null = np.zeros(len(arr), dtype=bool)
    for kind, nullable, member in path:
        n = len(cur)
        valid = np.asarray(cur.is_valid().to_numpy(zero_copy_only=False), dtype=bool) if nullable else None
        if kind == "list":
            offs = np.asarray(cur.offsets.to_numpy(zero_copy_only=False), dtype=np.int64)
            base = int(offs[0])
            nodes.append(((offs - base).astype(np.uint64), valid, n, under_null))
            cur = cur.values.slice(base, int(offs[-1]) - base)
            under_null = np.zeros(len(cur), dtype=bool)
        else:
            nodes.append((None, valid, n, under_null))
            cur = cur.field(member)
            assert len(cur) == n
            if valid is not None:
                under_null = under_null | ~valid
    return nodes, cur, under_null


def expected_leaf(arr, out_type):
    """pyarrow leaf array -> (values: numpy array / list of bytes, with NULL as 0 / None, validity bool)"""
    valid = np.asarray(arr.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
    if out_type == T.T_STRING:
        return [None if v is None else v.encode() for v in arr.to_pylist()], valid
    if out_type == T.T_DEC128:
        return [0 if v is None else int(v.scaleb(6)) for v in arr.to_pylist()], valid
    if out_type == T.T_BOOL:
        return np.asarray(arr.fill_null(False).to_numpy(zero_copy_only=False), dtype=bool), valid
    return np.asarray(arr.fill_null(0).to_numpy(zero_copy_only=False)).astype(PU.NP_OF[out_type]), valid


def resolve_views(views, bufs):
    """16-byte views (n, 16) u8 -> bytes, through the column's buffers (host copies, by buffer index)"""
    w = views.view(np.uint32).reshape(-1, 4)
    out = []
    for r in range(len(views)):
        ln = int(w[r, 0])
        if ln <= 12:
            assert not views[r, 4 + ln:].any(), r
            out.append(views[r, 4:4 + ln].tobytes())
        else:
            s = bufs[int(w[r, 2])][int(w[r, 3]):int(w[r, 3]) + ln].tobytes()
            assert s[:4] == views[r, 4:8].tobytes(), r
            out.append(s)
    return out


def check_decoded(res, col, arr, path, leaf_nullable, out_type, bufs=None):
    """decode_nested's output against pyarrow's reading, node by node and bit for bit; NULL and absent slots must be zero"""
    nodes, leaf_arr, leaf_undef = expected_nodes(arr, path)
    assert len(res) == len(nodes)
    for j, ((offs, valid, n, _), (goffs, gvalid, gitems, gnulls)) in enumerate(zip(nodes, res)):
        assert gitems == n, (j, gitems, n)
        if offs is not None:
            assert np.array_equal(goffs, offs), (j, goffs[:20], offs[:20])
        else:
            assert goffs is None
        if valid is not None:
            assert np.array_equal(gvalid, valid), j
            assert gnulls == int((~valid).sum()), j
        else:
            assert gvalid is None and gnulls == 0
    vals, valid = expected_leaf(leaf_arr, out_type)
    n = len(leaf_arr)
    assert col.n == n
    if leaf_nullable:
        assert np.array_equal(col.validity_numpy(), valid)
    # what the decode must hold: pyarrow's value where the leaf is valid, zero bytes in a NULL slot and in a required member's slot under
    # a NULL STRUCT
    zero = ~valid | leaf_undef
    if out_type == T.T_BOOL:
        exp = np.where(zero, False, vals)
        assert np.array_equal(col.to_numpy(), exp)
    elif out_type == T.T_STRING:
        views = col.to_numpy()
        if bufs is None:
            bufs = [k.to_numpy(np.uint8, k.nbytes) for k in col._keep]
        for r in np.nonzero(zero)[0]:
            assert not views[r].any(), r
        got = resolve_views(views, bufs)
        assert [None if z else g for g, z in zip(got, zero)] == [None if z else v for v, z in zip(vals, zero)]
    elif out_type == T.T_DEC128:
        assert col.to_numpy() == [0 if z else v for v, z in zip(vals, zero)]
    else:
        exp = np.where(zero, 0, vals).astype(vals.dtype)
        assert np.array_equal(col.to_numpy(), exp)


# ---- hand-built pages and the page headers of a chunk ------------------------------------------------------------------------
def rle_runs(levels):
    """RLE / bit-packed hybrid stream of `levels`, one RLE run per level (bit width <= 8: one value byte)"""
    out = bytearray()
    for v in levels:
        out += PU._varint(2) + bytes([v])
    return bytes(out)


def v1_page(num_values, payload, def_enc=3, rep_enc=3, encoding=0):
    """thrift compact PageHeader of an uncompressed v1 DATA_PAGE + the payload"""
    zz = PU._zz32
    hdr = (b"\x15" + zz(0) + b"\x15" + zz(len(payload)) + b"\x15" + zz(len(payload)) +
           b"\x2c" + b"\x15" + zz(num_values) + b"\x15" + zz(encoding) + b"\x15" + zz(def_enc) + b"\x15" + zz(rep_enc) + b"\x00" + b"\x00")
    return hdr + payload


def v1_levels_page(reps, defs, values, def_enc=3, rep_enc=3):
    """an uncompressed v1 data page of an INT64 leaf: <len><repetition runs><len><definition runs><PLAIN values>"""
    rs, ds = rle_runs(reps), rle_runs(defs)
    payload = struct.pack("<I", len(rs)) + rs + struct.pack("<I", len(ds)) + ds + np.asarray(values, np.int64).tobytes()
    return v1_page(len(defs), payload, def_enc, rep_enc)


class _Thrift:
    def __init__(self, b, p):
        self.b, self.p = b, p

    def varint(self):
        v = s = 0
        while True:
            x = self.b[self.p]
            self.p += 1
            v |= (x & 0x7F) << s
            s += 7
            if not x & 0x80:
                return v

    def zz(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def struct_(self):
        """-> {field id: value} (nested structs as dicts; lists / binaries skipped)"""
        out, last = {}, 0
        while True:
            h = self.b[self.p]
            self.p += 1
            if h == 0:
                return out
            t = h & 0x0F
            fid = last + (h >> 4) if h >> 4 else self.zz()
            last = fid
            if t in (1, 2):
                out[fid] = t == 1
            elif t in (3, 4, 5, 6):
                out[fid] = self.zz() if t != 3 else self.b[self.p]
                if t == 3:
                    self.p += 1
            elif t == 7:
                self.p += 8
            elif t == 8:
                self.p += self.varint()
            elif t == 12:
                out[fid] = self.struct_()
            elif t in (9, 10):
                x = self.b[self.p]
                self.p += 1
                n = x >> 4 if x >> 4 != 15 else self.varint()
                et = x & 0x0F
                for _ in range(n):
                    if et == 12:
                        self.struct_()
                    elif et in (5, 6):
                        self.zz()
                    elif et == 8:
                        self.p += self.varint()
                    else:
                        raise ValueError(et)
            else:
                raise ValueError(t)


def pages(chunk):
    """-> [dict(type, payload_at, payload_len, header)] of a column chunk (payload_at: offset in the chunk)"""
    out, p = [], 0
    while p < len(chunk):
        r = _Thrift(chunk, p)
        h = r.struct_()
        out.append(dict(type=h[1], payload_at=r.p, payload_len=h[3], header=h))
        p = r.p + h[3]
    return out


def v1_level_ranges(chunk):
    """uncompressed v1 chunk with repetition levels -> [(start, end)] of the repetition and definition level runs of every data page"""
    out = []
    for pg in pages(chunk):
        if pg["type"] != 0:
            continue
        a = pg["payload_at"]
        rl = struct.unpack_from("<I", chunk, a)[0]
        out.append((a + 4, a + 4 + rl))
        dl = struct.unpack_from("<I", chunk, a + 4 + rl)[0]
        out.append((a + 8 + rl, a + 8 + rl + dl))
    return out


def open_nested(ch, path, leaf_nullable, out_type, data=None):
    """dbhip_pq_chunk_open_device_nested through ctypes -> (rc, info); the handle is closed"""
    import ctypes as C
    data = ch["chunk"] if data is None else data
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data if data else b"\0")
    nodes = (T.PqNode * max(len(path), 1))(*[T.PqNode(KIND.get(k, k), n) for k, n in path])
    h, info = C.c_void_p(), T.PqInfo()
    rc = T.lib().dbhip_pq_chunk_open_device_nested(buf, C.c_int64(len(data)), ch["codec"], ch["physical"], ch["type_length"], nodes, len(path),
                                                   leaf_nullable, out_type, C.byref(h), C.byref(info))
    if rc == 0:
        T.lib().dbhip_pq_chunk_close(h)
    return rc, info


KIND = {"list": T.PQ_LIST, "struct": T.PQ_STRUCT}
