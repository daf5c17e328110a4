"""Decodes one column of `rows` values written in a given encoding through the device mode of the scan side a few times, for rocprofv3 runs
(kernel time per encoding, next to PLAIN of the same values):
    python tools/pq_encoding_probe.py [plain|bss|dlba|dba] [f64|i64|dec|str] [rows] [codec]
BYTE_STREAM_SPLIT (bss) takes the fixed-width kinds, DELTA_LENGTH_BYTE_ARRAY (dlba) strings, DELTA_BYTE_ARRAY (dba) strings and decimals
(FIXED_LEN_BYTE_ARRAY). Prints one JSON line: chunk bytes in, column bytes out, ms per decode (host clock around a synchronised decode)."""
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

ENC = {"plain": None, "bss": "BYTE_STREAM_SPLIT", "dlba": "DELTA_LENGTH_BYTE_ARRAY", "dba": "DELTA_BYTE_ARRAY"}


def values(kind, n, rng):
    """the same values for every encoding: (pyarrow array, out type)"""
    import pyarrow as pa
    import pyarrow.compute as pc
    if kind == "f64":
        return pa.array(rng.standard_normal(n)), T.T_F64
    if kind == "i64":
        return pa.array(rng.integers(-2**40, 2**40, n)), T.T_I64
    if kind == "dec":
        v = rng.integers(-10**12, 10**12, n)
        words = np.stack([v, v >> 63], axis=1)   # unscaled values as 16-byte little-endian two's complement
        return pa.Array.from_buffers(pa.decimal128(15, 2), n, [None, pa.py_buffer(words.tobytes())]), T.T_DEC128
    # strings of 10-30 bytes, sorted (the shape a format-2 writer's DELTA_BYTE_ARRAY fallback sees: keys with shared prefixes)
    ids = pa.array(np.sort(rng.integers(0, 10**12, n))).cast(pa.string())
    return pc.binary_join_element_wise("key-", ids, ""), T.T_STRING


def main():
    import pyarrow as pa
    import pyarrow.parquet as pq
    enc = sys.argv[1] if len(sys.argv) > 1 else "plain"
    kind = sys.argv[2] if len(sys.argv) > 2 else "str"
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 20_000_000
    codec = sys.argv[4] if len(sys.argv) > 4 else "none"
    rng = np.random.default_rng(4)
    arr, ot = values(kind, n, rng)
    buf = io.BytesIO()
    kw = dict(compression=codec, use_dictionary=False, write_statistics=False, data_page_version="2.0", row_group_size=n, store_schema=False,
              data_page_size=1024 * 1024)
    if ENC[enc]:
        kw["column_encoding"] = {"c": ENC[enc]}
    pq.write_table(pa.table({"c": pa.array(arr)}), buf, **kw)
    chunks, back = PU.column_chunks(buf.getvalue())
    ch = chunks[0]
    assert ENC[enc] is None or ENC[enc] in ch["encodings"], ch["encodings"]
    D.init(0)
    pc = D.ParquetChunk(ch["chunk"], ch["physical"], ot, ch["type_length"], ch["max_def"], 0, ch["codec"], precision=15, scale=2, device=True)
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        col = pc.decode()
        ms.append((time.perf_counter() - t0) * 1e3)
    exp = back.column(0).combine_chunks()
    if ot == T.T_STRING:
        lens = col.data.to_numpy(np.uint32, 4 * n).reshape(-1, 4)[:, 0]
        assert np.array_equal(lens, np.diff(np.frombuffer(exp.buffers()[1], np.int32)[:n + 1]))
        out_bytes = 16 * n + (col._keep[1].nbytes if len(col._keep) > 1 else 0)
    else:
        got = col.data.to_numpy(np.uint8, n * PU.ESIZE[ot])
        if ot == T.T_DEC128:
            ref = np.frombuffer(exp.buffers()[1], np.uint8)[:16 * n]
        else:
            ref = np.frombuffer(exp.buffers()[1], np.uint8)[:n * PU.ESIZE[ot]]
        assert np.array_equal(got, ref)
        out_bytes = n * PU.ESIZE[ot]
    print(json.dumps(dict(encoding=enc, kind=kind, rows=n, codec=codec, pages=pc.info.n_pages, chunk_bytes=len(ch["chunk"]), out_bytes=out_bytes,
                          ms=[round(x, 3) for x in ms])))


if __name__ == "__main__":
    main()
