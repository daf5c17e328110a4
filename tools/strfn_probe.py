"""Times the String functions (include/dbhip.h a22) on the three synthetic String columns of tools/like_probe.py, resident in HBM:
    python tools/strfn_probe.py [rows] [out.jsonl]
defaults: 16 Mi rows; p_type (inline-only), p_name (mixed), o_comment (all-long). Shapes: dbhip_str_length in both modes, substr(1, 2)
and substr(-4) in unit mode and in byte mode, trim(' '), concat(col, '-', col) and upper(col) (each the count call plus the build call
into a buffer sized once), and in the same run the yardstick: dbhip_take with elem_size 16 and the identity selection on the same
column — the existing entry point that moves 16-byte views: 16 B in, 16 B out and 4 B of selection per row. Each shape runs once as a
warm-up and then 5 times between two device events on the synchronised stream. Prints (and appends to out.jsonl) one JSON line per
column: per shape the 5 times, their median, rows/s, the bytes touched (a model, below) per second as a share of the 8.0 TB/s HBM
peak and the spread (max - min) / median. Every figure is guarded by a checksum: the output is filled with 0xFF before the timed runs
and the sum of the result lengths afterwards must be the one computed on the host from the column's pool of values — a call that did
nothing is not timed."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402
from like_probe import HBM_PEAK, TILE, build_column, columns, timed     # noqa: E402


def words_of(lens, nbytes):
    """the aligned 4-byte words that hold `nbytes` bytes of each long value, one word more for a value that starts off a boundary"""
    return int(((np.minimum(lens, nbytes).astype(np.int64) + 3) // 4 * 4 + 4).sum())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    D.init(0)
    rng = np.random.default_rng(7)
    L = T.lib()
    views_out = D.DeviceBuffer(n * 16)
    len_out = D.DeviceBuffer(n * 8)
    sel = D.DeviceBuffer.from_numpy(np.arange(n, dtype=np.uint32))
    one, two, minus4 = (D.Column.scalar(x, T.T_I64) for x in (1, 2, -4))
    c1, c2, cm4 = one.c(), two.c(), minus4.c()
    dash = D.Column.strings([b"-"])
    dash.is_scalar = True
    space = (C.c_uint8 * 1)(0x20)
    lines = []
    for name, pool in columns(n, rng):
        pick = rng.integers(0, len(pool), TILE)
        col, lens, _ = build_column(pool, pick, n)
        cc = col.c()
        long_lens = lens[lens > 12]
        rows_of = np.bincount(np.tile(pick, (n + TILE - 1) // TILE)[:n], minlength=len(pool))      # rows per pool value

        def expect(f):
            return int(sum(int(k) * f(v) for v, k in zip(pool, rows_of)))

        res = dict(column=name, rows=n, long_rows=int(len(long_lens)), long_bytes=int(long_lens.astype(np.int64).sum()), hbm_peak_bytes_per_s=HBM_PEAK, shapes={})

        def record(label, fn, nbytes, out, checksum, want):
            T.check(L.dbhip_memset(C.c_void_p(out.ptr), 0xFF, C.c_size_t(out.nbytes), None))
            ms = timed(fn)
            got = checksum()
            assert got == want, (name, label, got, want)
            med = float(np.median(ms))
            res["shapes"][label] = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4),
                                        rows_per_s=round(n / (med / 1e3)), touched_bytes=int(nbytes), bytes_per_row=round(nbytes / n, 2),
                                        share_of_hbm_peak=round(nbytes / (med / 1e3) / HBM_PEAK, 4), checksum=got)

        def view_lens():
            return int(views_out.to_numpy(np.uint32, n * 4)[0::4].astype(np.int64).sum())

        def lengths():
            return int(len_out.to_numpy(np.uint64, n).sum())

        def slice_call(op, a, b, pad, pad_len, flags):
            return lambda: T.check(L.dbhip_str_slice(C.c_int32(op), C.byref(cc), a, b, pad, C.c_int32(pad_len), C.c_int32(flags), C.c_int64(n),
                                                     C.c_void_p(views_out.ptr), None))

        # the yardstick first: 16 B in, 16 B out, 4 B of selection
        record("dbhip_take 16 B identity", lambda: T.check(L.dbhip_take(C.c_void_p(col.data.ptr), 16, C.c_void_p(sel.ptr), C.c_int64(n), C.c_void_p(views_out.ptr), None)),
               36 * n, views_out, view_lens, expect(len))
        for label, flags in (("str_length unit", 0), ("str_length byte", T.STR_UNIT_BYTE)):
            record(label, lambda: T.check(L.dbhip_str_length(C.byref(cc), C.c_int32(flags), C.c_int64(n), C.c_void_p(len_out.ptr), None)),
                   24 * n + (0 if flags else words_of(long_lens, 1 << 30)), len_out, lengths, expect(len))
        for mode, flags in (("unit", 0), ("byte", T.STR_UNIT_BYTE)):
            # substr(1, 2): two bytes of the view's own prefix word; the unit walk looks at the first three bytes of a long value
            record(f"substr(1, 2) {mode}", slice_call(T.STR_SUBSTR, C.byref(c1), C.byref(c2), None, 0, flags),
                   32 * n + (0 if flags else words_of(long_lens, 3)), views_out, view_lens, expect(lambda v: len(v[:2])))
            # substr(-4): the last four bytes of a long value (its words), which the unit walk reads as well
            record(f"substr(-4) {mode}", slice_call(T.STR_SUBSTR, C.byref(cm4), None, None, 0, flags),
                   32 * n + words_of(long_lens, 4), views_out, view_lens, expect(lambda v: 4 if len(v) >= 4 else 0))
        # trim(' '): the first and the last byte of a long value
        record("trim ' '", slice_call(T.STR_TRIM_BOTH, None, None, space, 1, 0), 32 * n + 2 * words_of(long_lens, 1), views_out, view_lens,
               expect(lambda v: len(v.strip(b" "))))

        # builds: the count call (views in), then count + scan + fill (+ copy): views in twice, 4 B counts out and in twice, 8 B offsets out
        # and in, the view out, the arguments' bytes in and the result's bytes out
        def build_shape(label, op, args, result_len):
            arr = (T.Col * len(args))(*[a.c() for a in args])
            nbytes = C.c_uint64(0)
            T.check(L.dbhip_str_build_bytes(C.c_int32(op), arr, C.c_int32(len(args)), C.c_int64(n), C.byref(nbytes), None))
            data = D.DeviceBuffer(nbytes.value)

            def call():
                T.check(L.dbhip_str_build_bytes(C.c_int32(op), arr, C.c_int32(len(args)), C.c_int64(n), C.byref(nbytes), None))
                T.check(L.dbhip_str_build(C.c_int32(op), arr, C.c_int32(len(args)), C.c_int64(n), C.c_void_p(views_out.ptr), C.c_void_p(data.ptr), C.c_uint64(nbytes.value),
                                          None, None, None, None))
            n_cols = sum(1 for a in args if not a.is_scalar)
            record(label, call, (3 * 16 + 4 + 4 + 4 + 8 + 8 + 16) * n + n_cols * words_of(long_lens, 1 << 30) + nbytes.value, views_out, view_lens, expect(result_len))
            res["shapes"][label]["out_data_bytes"] = nbytes.value

        build_shape("concat(col, '-', col)", T.STR_CONCAT, [col, dash, col], lambda v: 2 * len(v) + 1)
        build_shape("upper(col)", T.STR_UPPER, [col], len)
        line = json.dumps(res)
        print(line)
        lines.append(line)
        del col
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
