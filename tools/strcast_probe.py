"""Times the String casts (include/dbhip.h a24) on columns resident in HBM:
    python tools/strcast_probe.py [rows] [out.jsonl]
defaults: 16 Mi rows. For every supported type — I8 .. U64, Decimal(15,2) as DEC64, Decimal(38,10) as DEC128, Date, Timestamp — a column
of seeded random values over the type's whole range (the decimals: every digit count up to the precision equally often) is
  formatted   dbhip_str_format_bytes + dbhip_str_format into a buffer sized once (the count call is part of the timed shape), beside
              the yardstick a22 and a23 used: dbhip_take with the type's element size and the identity selection on the same column;
  parsed      dbhip_str_parse over the String column the format call has just produced, beside dbhip_take with elem_size 16 over
              that column's views.
Each shape runs once as a warm-up and then 5 times between two device events on the synchronised stream. Prints (and appends to
out.jsonl) one JSON line per type: per shape the 5 times, their median, rows/s, the bytes touched (a model, below) per second as a
share of the 8.0 TB/s HBM peak, the spread (max - min) / median, and the two ratios to the yardstick. Every figure is guarded: the
outputs are filled with 0xFF before the timed runs, and afterwards the parsed column must equal the source bit for bit with no row
raised or declined — a call that did nothing, or printed something else, is not timed."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402
from like_probe import HBM_PEAK, timed      # noqa: E402

TYPES = [("int8", T.T_I8, 0, 0), ("int16", T.T_I16, 0, 0), ("int32", T.T_I32, 0, 0), ("int64", T.T_I64, 0, 0), ("uint8", T.T_U8, 0, 0), ("uint16", T.T_U16, 0, 0),
         ("uint32", T.T_U32, 0, 0), ("uint64", T.T_U64, 0, 0), ("decimal(15,2)", T.T_DEC64, 15, 2), ("decimal(38,10)", T.T_DEC128, 38, 10), ("date", T.T_DATE, 0, 0),
         ("timestamp", T.T_TIMESTAMP, 0, 0)]
OFFSET_S = 19800


def random_column(rng, n, dtype, precision):
    """-> raw little-endian bytes of n values as a numpy array"""
    if dtype == T.T_DATE:
        return rng.integers(-719162, 2932897, n, dtype=np.int64).astype(np.int32)
    if dtype == T.T_TIMESTAMP:
        return rng.integers(-62135596800000000 + 64800 * 10**6, 253402300799999999 - 64800 * 10**6, n, dtype=np.int64)
    if dtype in D.NP_OF and dtype != T.T_DEC64:
        info = np.iinfo(D.NP_OF[dtype])
        return rng.integers(info.min, info.max, n, dtype=D.NP_OF[dtype], endpoint=True)
    # decimals: a digit count, then digits; as two u64 limbs, sign applied in two's complement
    digits = rng.integers(1, precision + 1, n)
    lo_digits = np.minimum(digits, 19)
    lo = (rng.random(n) * 10.0 ** lo_digits).astype(np.uint64) % np.uint64(10**19)
    hi_part = np.where(digits > 19, (rng.random(n) * 10.0 ** np.maximum(digits - 19, 0)).astype(np.uint64), np.uint64(0))
    if dtype == T.T_DEC64:
        mag = lo % np.uint64(10**precision)
        return np.where(rng.random(n) < 0.5, mag.astype(np.int64), -mag.astype(np.int64))
    # mag = hi_part * 10^19 + lo in 128 bits, by 32-bit pieces of the constant
    c = 10**19
    c_lo, c_hi = np.uint64(c & 0xFFFFFFFF), np.uint64(c >> 32)
    a_lo, a_hi = hi_part & np.uint64(0xFFFFFFFF), hi_part >> np.uint64(32)
    p0, p1, p2, p3 = a_lo * c_lo, a_lo * c_hi, a_hi * c_lo, a_hi * c_hi
    mid = (p0 >> np.uint64(32)) + (p1 & np.uint64(0xFFFFFFFF)) + (p2 & np.uint64(0xFFFFFFFF))
    low = (p0 & np.uint64(0xFFFFFFFF)) | (mid << np.uint64(32))
    high = p3 + (p1 >> np.uint64(32)) + (p2 >> np.uint64(32)) + (mid >> np.uint64(32))
    s = low + lo
    high = high + (s < low).astype(np.uint64)
    low = s
    neg = rng.random(n) < 0.5
    nlow = (~low) + np.uint64(1)
    nhigh = (~high) + (low == 0).astype(np.uint64)
    out = np.empty((n, 2), dtype=np.uint64)
    out[:, 0] = np.where(neg, nlow, low)
    out[:, 1] = np.where(neg, nhigh, high)
    return out.reshape(-1)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    D.init(0)
    rng = np.random.default_rng(24)
    L = T.lib()
    sel = D.DeviceBuffer.from_numpy(np.arange(n, dtype=np.uint32))
    views = D.DeviceBuffer(n * 16)
    moved = D.DeviceBuffer(n * 16)
    counters = D.DeviceBuffer(24)
    lines = []
    for name, dtype, precision, scale in TYPES:
        size = D.ELEM_SIZE[dtype]
        host = random_column(rng, n, dtype, precision)
        col = D.Column(dtype, n, D.DeviceBuffer.from_numpy(host), None, precision, scale)
        cc = col.c()
        res = dict(type=name, rows=n, offset_s=OFFSET_S, hbm_peak_bytes_per_s=HBM_PEAK, shapes={})

        def record(label, fn, nbytes):
            ms = timed(fn)
            med = float(np.median(ms))
            res["shapes"][label] = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4), rows_per_s=round(n / (med / 1e3)),
                                        touched_bytes=int(nbytes), bytes_per_row=round(nbytes / n, 2), share_of_hbm_peak=round(nbytes / (med / 1e3) / HBM_PEAK, 4))
            return med

        nbytes = C.c_uint64(0)
        T.check(L.dbhip_str_format_bytes(C.byref(cc), C.c_int32(OFFSET_S), C.c_int64(n), C.byref(nbytes), None))
        data = D.DeviceBuffer(nbytes.value)
        for buf in (views, moved, data):
            T.check(L.dbhip_memset(C.c_void_p(buf.ptr), 0xFF, C.c_size_t(max(buf.nbytes, 1)), None))
        counters.zero()

        def format_call():
            T.check(L.dbhip_str_format_bytes(C.byref(cc), C.c_int32(OFFSET_S), C.c_int64(n), C.byref(nbytes), None))
            T.check(L.dbhip_str_format(C.byref(cc), C.c_int32(OFFSET_S), C.c_int64(n), C.c_void_p(views.ptr), C.c_void_p(data.ptr), C.c_uint64(nbytes.value),
                                       C.c_void_p(counters.ptr), None))

        take_src = record("dbhip_take %d B identity" % size, lambda: T.check(L.dbhip_take(C.c_void_p(col.data.ptr), size, C.c_void_p(sel.ptr), C.c_int64(n),
                                                                                            C.c_void_p(moved.ptr), None)), (2 * size + 4) * n)
        # count: the value in; fill: the value in again, 4 B counts out and in (twice: the scan), 8 B offsets out and in, the view and the text out
        fmt = record("format", format_call, (3 * size + 3 * 4 + 2 * 8 + 16) * n + nbytes.value)
        res["shapes"]["format"]["out_data_bytes"] = nbytes.value
        res["format_over_take"] = round(fmt / take_src, 2)

        ptrs = D.DeviceBuffer.from_numpy(np.array([data.ptr], dtype=np.uint64))
        text = D.Column(T.T_STRING, n, views, None, buffers=ptrs)
        ct = text.c()
        out = D.DeviceBuffer(n * size)
        bitmap = D.DeviceBuffer(((n + 63) // 64) * 8)
        T.check(L.dbhip_memset(C.c_void_p(out.ptr), 0xFF, C.c_size_t(out.nbytes), None))
        take_views = record("dbhip_take 16 B identity", lambda: T.check(L.dbhip_take(C.c_void_p(views.ptr), 16, C.c_void_p(sel.ptr), C.c_int64(n), C.c_void_p(moved.ptr),
                                                                                       None)), 36 * n)
        # the view in, the text's words in (one more for a value that starts off a boundary), the value and the row's bit out
        parse = record("parse", lambda: T.check(L.dbhip_str_parse(C.byref(ct), C.c_int32(dtype), C.c_uint8(precision), C.c_uint8(scale), 0, 0, C.c_int32(OFFSET_S),
                                                                   C.c_int64(n), C.c_void_p(out.ptr), C.c_void_p(bitmap.ptr), C.c_void_p(counters.ptr + 8),
                                                                   C.c_void_p(counters.ptr + 16), None)), (16 + size) * n + n // 8 + nbytes.value + 4 * n)
        res["parse_over_take"] = round(parse / take_views, 2)
        # the guard: what came back is the source, and no row was dropped, raised or declined in any of the runs
        back = out.to_numpy(np.uint8, n * size)
        assert np.array_equal(back, np.ascontiguousarray(host).view(np.uint8).reshape(-1)), name
        assert counters.to_numpy(np.uint64, 3).tolist() == [0, 0, 0], name
        assert (bitmap.to_numpy(np.uint64, n // 64) == np.uint64(2**64 - 1)).all(), name
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del col, text, data, out, bitmap
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
