"""Times the conditionals (include/dbhip.h a27) on columns resident in HBM:
    python tools/cond_probe.py [rows] [out.jsonl]
defaults: 64 Mi rows (a multiple of the 4 Mi block). Six calls, each BESIDE the existing call a binding had for the shape, in the same
run:
  if(cond, a, b) over Int64, the condition mixed within every wave    beside ExprProgram.if_ (dbhip_expr_eval), the same result
  the same with a condition that is constant over 4,096-row runs      beside the same program: the branch nobody chose is not read
  coalesce(x, 0) over a nullable Int64 with 10 % NULLs                beside dbhip_cast Int64 -> UInt64, one column in, one out
  a 4-condition CASE with constant String results, some long          beside dbhip_take of 16-byte elements, identity selection
  if(cond, a, b) over Int8, the narrow stores                         beside dbhip_cast Int8 -> UInt8
  bool_or over two nullable Boolean columns                           beside the five dbhip_bitmap_binary launches
The columns are a seeded block of 4 Mi random rows repeated on the device (Bitmaps too). Each pair runs 3 times as a warm-up and then
9 times, the two calls ALTERNATING, each between two device events on the synchronised stream. Prints (and appends to out.jsonl) one
JSON line per call: per side the times, their median, the spread (max - min) / median, rows/s and the algorithmic bytes per second as a
share of the 8.0 TB/s HBM peak, and the ratio of the two medians. The byte model of the new call counts what the call has to move:
every Bitmap it reads, the output, and of each branch column only the rows' share that some wave chose. Every figure is guarded: the
outputs are filled with 0xFF before the timed runs, and afterwards the first and the last 4,096 rows must equal tests/cond_ref.py."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402
from tests import cond_ref as R             # noqa: E402

HBM_PEAK = 8.0e12
BLOCK = 4 << 20
REPS = 9
WARMUPS = 3
GUARD_ROWS = 4096


def repeated(block_bytes, total_bytes):
    """a device buffer of total_bytes: the block's bytes again and again"""
    one = D.DeviceBuffer.from_numpy(block_bytes)
    buf = D.DeviceBuffer(total_bytes)
    for at in range(0, total_bytes, len(block_bytes)):
        k = min(len(block_bytes), total_bytes - at)
        T.check(T.lib().dbhip_memcpy_d2d(C.c_void_p(buf.ptr + at), C.c_void_p(one.ptr), C.c_size_t(k), None))
    return buf


def column(values, n, dtype, valid=None):
    """the block `values` (numpy, one row per element) repeated to n rows -> Column"""
    raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
    size = len(raw) // len(values)
    col = D.Column(dtype, n, repeated(raw, n * size))
    if valid is not None:
        col.validity = repeated(np.packbits(valid, bitorder="little"), n // 8)
    return col


def bool_column(bits, n, valid=None):
    col = D.Column(T.T_BOOL, n, repeated(np.packbits(bits, bitorder="little"), n // 8))
    if valid is not None:
        col.validity = repeated(np.packbits(valid, bitorder="little"), n // 8)
    return col


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


def ends(buf, n, size):
    """the first and the last GUARD_ROWS elements of a device buffer as bytes"""
    k = min(GUARD_ROWS, n)
    return (D.BorrowedBuffer(buf.ptr, k * size).to_numpy(np.uint8, k * size).tobytes(),
            D.BorrowedBuffer(buf.ptr + (n - k) * size, k * size).to_numpy(np.uint8, k * size).tobytes())


def ref_ends(fn, rows):
    """fn(slice) -> bytes over the first and the last GUARD_ROWS rows of the block (n is a whole number of blocks)"""
    k = min(GUARD_ROWS, rows)
    return fn(slice(0, k)), fn(slice(rows - k, rows))


def select_call(conds, vals, n, out):
    carr = D._cols(conds) if conds else None
    varr = D._cols(vals)
    keep = (carr, varr)
    if conds:
        return keep, lambda: T.check(T.lib().dbhip_case(carr, len(conds), varr, C.c_int64(n), C.c_void_p(out.ptr), None, None, None, None, None))
    return keep, lambda: T.check(T.lib().dbhip_coalesce(varr, len(vals), C.c_int64(n), C.c_void_p(out.ptr), None, None, None, None, None))


def chosen_share(branch, k, run):
    """the share of the rows of branch column k that lie in a run of `run` rows (what a wave covers) where some row chose k"""
    b = np.asarray(branch)
    b = b[:len(b) // run * run].reshape(-1, run)
    return float((b == k).any(axis=1).mean())


def if_case(name, n, rng, rows, dtype, runs):
    np_t = D.NP_OF[dtype]
    size = np.dtype(np_t).itemsize
    info = np.iinfo(np_t)
    a = rng.integers(1, info.max, rows, dtype=np_t)
    b = rng.integers(1, info.max, rows, dtype=np_t)
    bits = np.repeat(rng.random(rows // 4096) < 0.5, 4096) if runs else rng.random(rows) < 0.5
    ca, cb, cc = column(a, n, dtype), column(b, n, dtype), bool_column(bits, n)
    out, yard_out = D.DeviceBuffer(n * size), D.DeviceBuffer(n * size)
    keep, new = select_call([cc], [ca, cb], n, out)
    exp = np.where(bits, a, b)
    wave_rows = 64 * max(16 // size, 1)
    share = sum(chosen_share(np.where(bits, 0, 1), k, wave_rows) for k in (0, 1))
    nbytes = n * (1 / 8 + size * share + size)
    if dtype == T.T_I64:
        p = D.ExprProgram([cc, ca, cb])
        reg = p.if_(p.load(0), p.load(1), p.load(2))
        prog, inputs = p.c_program(), D._cols(p.inputs)

        def yard():
            T.check(T.lib().dbhip_expr_eval(prog, len(p.ins), inputs, 3, C.c_int64(n), reg, C.c_void_p(yard_out.ptr), None, None, None, None, None))
        yard_name, yard_bytes, yard_check = "dbhip_expr_eval: load, load, load, if", n * (1 / 8 + 3 * size), True
    else:
        bitmap, count = D.DeviceBuffer(n // 8 + 8), D.DeviceBuffer(8).zero()
        src = ca.c()

        def yard():
            T.check(T.lib().dbhip_cast(C.byref(src), T.T_U8, 0, 1, C.c_int64(n), C.c_void_p(yard_out.ptr), C.c_void_p(bitmap.ptr), C.c_void_p(count.ptr), None))
        yard_name, yard_bytes, yard_check = "dbhip_cast Int8 -> UInt8", n * (2 * size + 1 / 8), False
    return dict(name=name, new=new, yard=yard, yard_name=yard_name, out=out, yard_out=yard_out if yard_check else None, size=size,
                ref=lambda s: exp[s].tobytes(), nbytes=nbytes, yard_bytes=yard_bytes, keep=(keep, ca, cb, cc), model="chosen share of the two branches %.3f of 2" % share)


def coalesce_case(n, rng, rows):
    x = rng.integers(1, 2**62, rows, dtype=np.int64)
    valid = rng.random(rows) >= 0.1
    cx, zero = column(x, n, T.T_I64, valid), D.Column.scalar(0, T.T_I64)
    out, yard_out = D.DeviceBuffer(n * 8), D.DeviceBuffer(n * 8)
    keep, new = select_call(None, [cx, zero], n, out)
    bitmap, count = D.DeviceBuffer(n // 8 + 8), D.DeviceBuffer(8).zero()
    src = cx.c()

    def yard():
        T.check(T.lib().dbhip_cast(C.byref(src), T.T_U64, 0, 1, C.c_int64(n), C.c_void_p(yard_out.ptr), C.c_void_p(bitmap.ptr), C.c_void_p(count.ptr), None))
    exp = np.where(valid, x, 0)
    return dict(name="coalesce(x, 0), nullable int64, 10% NULL", new=new, yard=yard, yard_name="dbhip_cast Int64 -> UInt64", out=out, yard_out=None, size=8,
                ref=lambda s: exp[s].tobytes(), nbytes=n * (8 + 1 / 8 + 8), yard_bytes=n * (16 + 1 / 8), keep=(keep, cx, zero), model="x, its validity, out")


def string_case(n, rng, rows):
    texts = [b"1-URGENT", b"a priority that is longer than twelve bytes", b"3-MEDIUM", b"another long constant, in its own buffer", b"5-LOW"]
    consts = []
    for t in texts:
        c = D.Column.strings([t])
        c.is_scalar = True
        consts.append(c)
    bits = [rng.random(rows) < 0.25 for _ in range(4)]
    conds = [bool_column(b, n) for b in bits]
    out, yard_out = D.DeviceBuffer(n * 16), D.DeviceBuffer(n * 16)
    table = D.DeviceBuffer(8 * 5)
    carr, varr, nbuf = D._cols(conds), D._cols(consts), C.c_int32()

    def new():
        T.check(T.lib().dbhip_case(carr, 4, varr, C.c_int64(n), C.c_void_p(out.ptr), None, None, C.c_void_p(table.ptr), C.byref(nbuf), None))
    src = repeated(rng.integers(0, 256, rows * 16, dtype=np.uint8), n * 16)
    sel = D.DeviceBuffer.from_numpy(np.arange(n, dtype=np.uint32))

    def yard():
        T.check(T.lib().dbhip_take(C.c_void_p(src.ptr), 16, C.c_void_p(sel.ptr), C.c_int64(n), C.c_void_p(yard_out.ptr), None))
    views = [c.to_numpy() for c in consts]
    branch = R.choose_case([R.Col(b, None) for b in bits], rows)

    def ref(s):
        return R.select_views(views, [None] * 5, [True] * 5, [1] * 5, branch[s])
    return dict(name="CASE, 4 conditions, constant String results", new=new, yard=yard, yard_name="dbhip_take, 16-byte elements, identity selection",
                out=out, yard_out=None, size=16, ref=ref, nbytes=n * (4 / 8 + 16), yard_bytes=n * (16 + 4 + 16), keep=(conds, consts, table, src, sel),
                model="four condition Bitmaps, out")


def or_case(n, rng, rows):
    cols = [(rng.random(rows) < 0.5, rng.random(rows) < 0.8) for _ in range(2)]
    a, b = (bool_column(bits, n, valid) for bits, valid in cols)
    words = n // 8
    t, v = D.DeviceBuffer(words), D.DeviceBuffer(words)
    tmp = [D.DeviceBuffer(words) for _ in range(3)]
    yt, yv = D.DeviceBuffer(words), D.DeviceBuffer(words)
    ca, cb = a.c(), b.c()

    def new():
        T.check(T.lib().dbhip_bool_logic(T.BOOL_OR, C.byref(ca), C.byref(cb), C.c_int64(n), C.c_void_p(t.ptr), C.c_void_p(v.ptr), None))

    def op(mode, x, y, o):
        T.check(T.lib().dbhip_bitmap_binary(mode, C.c_void_p(x.ptr), C.c_void_p(y.ptr), C.c_int64(n), C.c_void_p(o.ptr), None))

    def yard():
        op(0, a.data, a.validity, tmp[0])
        op(0, b.data, b.validity, tmp[1])
        op(1, tmp[0], tmp[1], yt)
        op(0, a.validity, b.validity, tmp[2])
        op(1, tmp[2], yt, yv)
    et, ev = R.bool_logic(R.OR, R.Col(cols[0][0], cols[0][1]), R.Col(cols[1][0], cols[1][1]), rows)
    return dict(name="bool_or, two nullable Boolean columns", new=new, yard=yard, yard_name="five dbhip_bitmap_binary launches", out=t, yard_out=yt, size=1 / 8,
                ref=lambda s: np.packbits(et[s], bitorder="little").tobytes(), nbytes=n * 6 / 8, yard_bytes=n * 15 / 8, keep=(a, b, v, tmp, yv),
                model="four Bitmaps in, two out", extra=(v, lambda s: np.packbits(ev[s], bitorder="little").tobytes()))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    rows = min(BLOCK, n)
    assert n % rows == 0 and rows % 4096 == 0, "rows: a whole number of 4 Mi blocks, or a multiple of 4096 below that"
    D.init(0)
    L = T.lib()
    rng = np.random.default_rng(27)
    ev = event_pair()
    lines = []
    makers = [lambda: if_case("if(cond, a, b), int64, mixed in every wave", n, rng, rows, T.T_I64, False),
              lambda: if_case("if(cond, a, b), int64, condition constant over 4096 rows", n, rng, rows, T.T_I64, True),
              lambda: coalesce_case(n, rng, rows), lambda: string_case(n, rng, rows),
              lambda: if_case("if(cond, a, b), int8, mixed in every wave", n, rng, rows, T.T_I8, False), lambda: or_case(n, rng, rows)]
    for make in makers:
        c = make()
        bufs = [c["out"]] + ([c["yard_out"]] if c["yard_out"] is not None else []) + ([c["extra"][0]] if "extra" in c else [])
        for buf in bufs:
            T.check(L.dbhip_memset(C.c_void_p(buf.ptr), 0xFF, C.c_size_t(buf.nbytes), None))
        for _ in range(WARMUPS):
            c["new"]()
            c["yard"]()
        ms_new, ms_yard = [], []
        for _ in range(REPS):
            ms_new.append(time_once(ev, c["new"]))
            ms_yard.append(time_once(ev, c["yard"]))
        # the guard: the first and the last rows are the reference's (and the call beside it gives the same, where it computes the same)
        checks = [(c["out"], c["ref"])] + ([(c["yard_out"], c["ref"])] if c["yard_out"] is not None else []) + ([c["extra"]] if "extra" in c else [])
        for buf, ref in checks:
            if c["size"] < 1:
                k = min(GUARD_ROWS, n) // 8
                got = (D.BorrowedBuffer(buf.ptr, k).to_numpy(np.uint8, k).tobytes(), D.BorrowedBuffer(buf.ptr + n // 8 - k, k).to_numpy(np.uint8, k).tobytes())
            else:
                got = ends(buf, n, c["size"])
            assert got == ref_ends(ref, rows), c["name"]
        res = dict(call=c["name"], rows=n, hbm_peak_bytes_per_s=HBM_PEAK, byte_model=c["model"], new=side(ms_new, n, c["nbytes"]),
                   beside=dict(call=c["yard_name"], **side(ms_yard, n, c["yard_bytes"])))
        res["new_over_beside"] = round(res["new"]["median_ms"] / res["beside"]["median_ms"], 3)
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
        del c, bufs, checks
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
