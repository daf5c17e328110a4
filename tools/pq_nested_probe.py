"""Decodes one nested column chunk through the device mode of the scan side, for timings and rocprofv3 runs:
    python tools/pq_nested_probe.py list_list [entries] [codec]           List<List<Int64>>, every level nullable, through decode_device_nested
    python tools/pq_nested_probe.py list [rows] [codec] [nested|list]     List<Int64> (the chunk of tools/probes/pq_list_rate.py: lists of 0..7
                                                                          elements, 8 % NULL lists, 10 % NULL elements) through decode_device_nested
                                                                          with the path [LIST 1] or through decode_device_list
V1 pages, PLAIN, 1 MiB pages (the reference writer's settings without a dictionary). The chunk is resident in HBM and the output buffers are
allocated before the clock starts; each decode is one ABI call, which synchronises its stream. Prints one JSON line: shape, rows, level entries,
codec, chunk bytes, output bytes, and ms per decode (5 runs after a warm-up decode). The first 20 000 rows are checked against pyarrow."""
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402
from tests import parquet_util as PU        # noqa: E402


def list_i64(rows, rng):
    import pyarrow as pa
    lens = rng.integers(0, 8, rows).astype(np.int32)
    null_list = rng.random(rows) < 0.08
    lens[null_list] = 0
    offsets = np.zeros(rows + 1, np.int32)
    np.cumsum(lens, out=offsets[1:])
    m = int(offsets[-1])
    vals = rng.integers(-10**12, 10**12, m)
    return pa.ListArray.from_arrays(pa.array(offsets, pa.int32()), pa.array(vals, pa.int64(), mask=rng.random(m) < 0.1), mask=pa.array(null_list))


def list_list_i64(entries, rng):
    """about `entries` level entries: lists of 0..4 lists of 0..5 Int64, 10 % NULL at every level"""
    import pyarrow as pa
    rows = int(entries / 4.7)
    olen = rng.integers(0, 5, rows)
    onull = rng.random(rows) < 0.1
    olen[onull] = 0
    ooff = np.zeros(rows + 1, np.int32)
    np.cumsum(olen, out=ooff[1:])
    mids = int(ooff[-1])
    ilen = rng.integers(0, 6, mids)
    inull = rng.random(mids) < 0.1
    ilen[inull] = 0
    ioff = np.zeros(mids + 1, np.int32)
    np.cumsum(ilen, out=ioff[1:])
    n = int(ioff[-1])
    leaf = pa.array(rng.integers(-2**62, 2**62, n), pa.int64(), mask=rng.random(n) < 0.1)
    inner = pa.ListArray.from_arrays(pa.array(ioff), leaf, mask=pa.array(inull))
    return pa.ListArray.from_arrays(pa.array(ooff), inner, mask=pa.array(onull))


def main():
    import pyarrow as pa
    import pyarrow.parquet as pq
    shape = sys.argv[1] if len(sys.argv) > 1 else "list_list"
    size = int(sys.argv[2]) if len(sys.argv) > 2 else (20_000_000 if shape == "list_list" else 6_000_000)
    codec = sys.argv[3] if len(sys.argv) > 3 else "none"
    via = sys.argv[4] if len(sys.argv) > 4 else "nested"
    rng = np.random.default_rng(21)
    arr = list_i64(size, rng) if shape == "list" else list_list_i64(size, rng)
    path = [("list", 1)] if shape == "list" else [("list", 1), ("list", 1)]
    data = PU.write_parquet(pa.Table.from_arrays([arr], names=["c"]), dictionary=False, v2=False, compression=codec, page_size=1 << 20)
    ch = PU.column_chunks(data)[0][0]
    D.init(0)
    L = T.lib()
    if via == "list":
        pc = D.ParquetChunk(ch["chunk"], ch["physical"], T.T_I64, 0, codec=ch["codec"], list_of=(1, 1))
        offs, lv, col = pc.decode_list()                 # warm-up + the check
        vals, ev = col.to_numpy(), col.validity_numpy()
        got_rows = [None if not lv[r] else [int(vals[k]) if ev[k] else None for k in range(int(offs[r]), int(offs[r + 1]))]
                    for r in range(min(20_000, pc.rows))]
    else:
        pc = D.ParquetChunk(ch["chunk"], ch["physical"], T.T_I64, 0, codec=ch["codec"], nested=path, leaf_nullable=1)
        res, col = pc.decode_nested()
        vals, ev = col.to_numpy(), col.validity_numpy()

        def build(level, lo, hi):
            if level == len(res):
                return [int(vals[k]) if ev[k] else None for k in range(lo, hi)]
            o, v = res[level][0], res[level][1]
            return [None if not v[k] else build(level + 1, int(o[k]), int(o[k + 1])) for k in range(lo, hi)]
        got_rows = build(0, 0, min(20_000, pc.rows))
    back = pq.read_table(io.BytesIO(data)).column(0).slice(0, 20_000).to_pylist()
    assert got_rows == back, shape
    i = pc.info
    ent = int(i.num_values)
    bufs = [D.DeviceBuffer((ent + 1) * 8 + 16) for _ in path] + [D.DeviceBuffer(i.validity_bytes + 8) for _ in range(len(path) + 1)]
    out = D.DeviceBuffer(i.out_bytes + 16)
    img = C.c_void_p(pc.image_dev.ptr) if pc.image_dev else None
    rows, elems, nl = C.c_int64(), C.c_int64(), C.c_int64()
    if via != "list":        # (via list: also runs against a build of the library from before the nested entry points)
        nodes = (T.PqNodeOut * (len(path) + 1))()
        for j in range(len(path)):
            nodes[j].offsets_dev, nodes[j].validity_dev = bufs[j].ptr, bufs[len(path) + j].ptr
        nodes[len(path)].validity_dev = bufs[-1].ptr

    def once():
        if via == "list":
            T.check(L.dbhip_pq_chunk_decode_device_list(pc.h, C.c_void_p(pc.chunk_dev.ptr), img, C.c_void_p(bufs[0].ptr), C.c_void_p(bufs[1].ptr),
                                                        C.c_void_p(out.ptr), C.c_void_p(bufs[2].ptr), C.byref(rows), C.byref(elems), C.byref(nl), None))
        else:
            T.check(L.dbhip_pq_chunk_decode_device_nested(pc.h, C.c_void_p(pc.chunk_dev.ptr), img, nodes, C.c_void_p(out.ptr), C.byref(rows), None))
    once()                                               # warm-up of the timed call
    ms = []
    for _ in range(5):
        T.check(L.dbhip_stream_sync(None))
        t0 = time.perf_counter()
        once()
        ms.append((time.perf_counter() - t0) * 1e3)
    # bytes written: offsets and validity of every node, the leaf values and validity
    items = [nodes[j].items for j in range(len(path) + 1)] if via != "list" else [rows.value, elems.value]
    out_bytes = sum((n + 1) * 8 + (n + 7) // 8 for n in items[:-1]) + items[-1] * 8 + (items[-1] + 7) // 8
    print(json.dumps(dict(shape=shape, via=via, rows=int(rows.value), entries=ent, codec=codec, pages=int(i.n_pages), chunk_bytes=len(ch["chunk"]),
                          out_bytes=int(out_bytes), ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3),
                          entries_per_s=round(ent / (float(np.median(ms)) / 1e3)))))
    pc.close()


if __name__ == "__main__":
    main()
