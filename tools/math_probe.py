"""Times the math functions (include/dbhip.h a26) on columns resident in HBM:
    python tools/math_probe.py [rows] [out.jsonl]
defaults: 64 Mi rows. Six calls — round(Float64, 2), abs(Int32), ceil(Int8), round(Decimal(15,4) as DEC64, 2), round(Decimal(38,10) as
DEC128, 2) and round(Decimal(38,30), 2), which takes the two-step division — each BESIDE an existing call that moves the same bytes, in
the same run: dbhip_cast for the number maps (Float64 -> Int64, Int32 -> UInt32, Int8 -> Float64), dbhip_decimal_cast to the same target
scale with rounding_mode = 1 for the decimal ones. No row of a yardstick should raise (its error count over all calls is read back and printed): the
Int32 -> UInt32 cast runs over the same column with the sign bits cleared, since a cast that counts an overflow in every second row
times its counter and not its bytes. The column is a seeded block of 4 Mi random rows repeated on the device. Each pair runs 3 times
as a warm-up and then 9 times, the two calls ALTERNATING, each between two device events on the synchronised stream. Prints
(and appends to out.jsonl) one JSON line per call: per side the times, their median, the spread (max - min) / median, rows/s and the
algorithmic bytes (value in + value out; the yardsticks also write one validity bit per row) per second as a share of the 8.0 TB/s HBM
peak, and the ratio of the two medians. Every figure is guarded: the outputs are filled with 0xFF before the timed runs, and afterwards
the first and the last 4,096 rows of the math result must equal tests/math_ref.py bit for bit."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402
from tests import math_ref as R             # noqa: E402

HBM_PEAK = 8.0e12
BLOCK = 4 << 20
REPS = 9
WARMUPS = 3


def random_block(rng, n, dtype, precision):
    """-> n seeded values as a numpy array (Decimal128: (n, 2) u64 words, two's complement), magnitudes below 10^precision"""
    if dtype == T.T_F64:
        return rng.standard_normal(n) * 1e6
    if dtype in (T.T_I32, T.T_I8):
        info = np.iinfo(D.NP_OF[dtype])
        return rng.integers(info.min, info.max, n, dtype=D.NP_OF[dtype], endpoint=True)
    neg = rng.random(n) < 0.5
    if dtype == T.T_DEC64:
        mag = rng.integers(0, 10**precision, n, dtype=np.int64)
        return np.where(neg, -mag, mag)
    hi = rng.integers(0, 10**precision >> 64, n, dtype=np.uint64)
    lo = rng.integers(0, 2**64, n, dtype=np.uint64)
    out = np.empty((n, 2), dtype=np.uint64)
    out[:, 0] = np.where(neg, ~lo + np.uint64(1), lo)
    out[:, 1] = np.where(neg, ~hi + (lo == 0).astype(np.uint64), hi)
    return out


def as_ints(block):
    return [(int(h) << 64 | int(l)) - ((int(h) >> 63) << 128) for l, h in block.tolist()]


def reference(fn, dtype, p, s, digits, rows):
    """tests/math_ref.py over a few rows -> raw bytes of the result"""
    if dtype in (T.T_DEC64, T.T_DEC128):
        vals = rows.tolist() if dtype == T.T_DEC64 else as_ints(rows)
        out = R.decimal(fn, vals, p, s, digits)
        if dtype == T.T_DEC64:
            return np.array(out, dtype=np.int64).tobytes()
        return b"".join((v & (2**128 - 1)).to_bytes(16, "little") for v in out)
    return R.number(fn, rows, digits).tobytes()


def event_pair():
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        T.check(T.lib().dbhip_event_create(C.byref(e)))
    return ev


def time_once(ev, fn):
    L = T.lib()
    T.check(L.dbhip_stream_sync(None))
    T.check(L.dbhip_event_record(ev[0], None))
    fn()
    T.check(L.dbhip_event_record(ev[1], None))
    T.check(L.dbhip_stream_sync(None))
    out = C.c_float()
    T.check(L.dbhip_event_elapsed_ms(ev[0], ev[1], C.byref(out)))
    return out.value


def side(ms, n, nbytes):
    med = float(np.median(ms))
    return dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4), rows_per_s=round(n / (med / 1e3)),
                bytes_per_row=round(nbytes / n, 3), share_of_hbm_peak=round(nbytes / (med / 1e3) / HBM_PEAK, 4))


# (name, fn, digits, source type, p, s, the yardstick: ("cast", dst type) | ("decimal_cast", p, s))
CALLS = [("round(float64, 2)", R.ROUND, 2, T.T_F64, 0, 0, ("cast", T.T_I64)),
         ("abs(int32)", R.ABS, 0, T.T_I32, 0, 0, ("cast", T.T_U32)),
         ("ceil(int8)", R.CEIL, 0, T.T_I8, 0, 0, ("cast", T.T_F64)),
         ("round(decimal(15,4), 2)", R.ROUND, 2, T.T_DEC64, 15, 4, ("decimal_cast", 15, 2)),
         ("round(decimal(38,10), 2)", R.ROUND, 2, T.T_DEC128, 38, 10, ("decimal_cast", 38, 2)),
         ("round(decimal(38,30), 2)", R.ROUND, 2, T.T_DEC128, 38, 30, ("decimal_cast", 38, 2))]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    D.init(0)
    L = T.lib()
    rng = np.random.default_rng(26)
    ev = event_pair()
    bitmap = D.DeviceBuffer(((n + 63) // 64) * 8 + 8)
    count = D.DeviceBuffer(8).zero()
    lines = []
    for name, fn, digits, dtype, p, s, yard in CALLS:
        size = D.ELEM_SIZE[dtype]
        block = random_block(rng, min(BLOCK, n), dtype, p)
        rows = len(block)
        one = D.DeviceBuffer.from_numpy(block)
        data = D.DeviceBuffer(n * size)
        for at in range(0, n, rows):
            k = min(rows, n - at)
            T.check(L.dbhip_memcpy_d2d(C.c_void_p(data.ptr + at * size), C.c_void_p(one.ptr), C.c_size_t(k * size), None))
        col = D.Column(dtype, n, data, None, p, s)
        cc = col.c()
        yard_cc = cc
        if name == "abs(int32)":          # the yardstick's source: the same rows without their sign bits, so that no row overflows UInt32
            one_pos = D.DeviceBuffer.from_numpy(block & np.int32(0x7FFFFFFF))
            yard_data = D.DeviceBuffer(n * size)
            for at in range(0, n, rows):
                k = min(rows, n - at)
                T.check(L.dbhip_memcpy_d2d(C.c_void_p(yard_data.ptr + at * size), C.c_void_p(one_pos.ptr), C.c_size_t(k * size), None))
            yard_col = D.Column(dtype, n, yard_data, None, p, s)
            yard_cc = yard_col.c()
        out_t, out_p, out_s = D.math_result(fn, col, digits)
        out_size = D.ELEM_SIZE[out_t]
        out = D.DeviceBuffer(n * out_size)
        yard_t = yard[1] if yard[0] == "cast" else dtype
        yard_out = D.DeviceBuffer(n * D.ELEM_SIZE[yard_t])
        assert D.ELEM_SIZE[yard_t] == out_size, name
        for buf in (out, yard_out):
            T.check(L.dbhip_memset(C.c_void_p(buf.ptr), 0xFF, C.c_size_t(buf.nbytes), None))

        def math_call():
            T.check(L.dbhip_math(fn, C.byref(cc), digits, C.c_int64(n), C.c_void_p(out.ptr), None))

        def yard_call():
            if yard[0] == "cast":
                T.check(L.dbhip_cast(C.byref(yard_cc), yard[1], 0, 1, C.c_int64(n), C.c_void_p(yard_out.ptr), C.c_void_p(bitmap.ptr), C.c_void_p(count.ptr), None))
            else:
                T.check(L.dbhip_decimal_cast(C.byref(yard_cc), dtype, yard[1], yard[2], 0, 1, C.c_int64(n), C.c_void_p(yard_out.ptr), C.c_void_p(bitmap.ptr),
                                             C.c_void_p(count.ptr), None))

        count.zero()
        for _ in range(WARMUPS):
            math_call()
            yard_call()
        ms_math, ms_yard = [], []
        for _ in range(REPS):
            ms_math.append(time_once(ev, math_call))
            ms_yard.append(time_once(ev, yard_call))
        # the guard: the first and the last rows are the reference's
        k = min(4096, n)
        tail_at = n - k
        head_rows, tail_rows = block[:k], np.concatenate([block] * 2)[(tail_at % rows):(tail_at % rows) + k]
        got_head = D.BorrowedBuffer(out.ptr, k * out_size).to_numpy(np.uint8, k * out_size).tobytes()
        got_tail = D.BorrowedBuffer(out.ptr + tail_at * out_size, k * out_size).to_numpy(np.uint8, k * out_size).tobytes()
        assert got_head == reference(fn, dtype, p, s, digits, head_rows), name
        assert got_tail == reference(fn, dtype, p, s, digits, tail_rows), name
        raised = int(count.to_numpy(np.uint64, 1)[0])
        nbytes = (size + out_size) * n
        res = dict(call=name, rows=n, hbm_peak_bytes_per_s=HBM_PEAK, math=side(ms_math, n, nbytes),
                   yardstick=dict(call="dbhip_%s -> type %d" % (yard[0], yard_t), raised_rows_in_all_calls=raised, **side(ms_yard, n, nbytes + n / 8)))
        res["math_over_yardstick"] = round(res["math"]["median_ms"] / res["yardstick"]["median_ms"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del col, data, out, yard_out, one
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
