"""Times String search and rewrite (include/dbhip.h a28) on the three synthetic String columns of tools/like_probe.py, resident in HBM:
    python tools/strsearch_probe.py [rows] [out.jsonl]
defaults: 16 Mi rows; p_type (inline-only), p_name (mixed), o_comment (all-long). Every shape stands beside a yardstick taken in the
same run on the same column:
    dbhip_str_match(CONTAINS, needle)               beside  position(needle)             the same bytes in; 8 B out per row instead of one bit
    dbhip_str_slice(TRIM_BOTH ' ')                  beside  split_part(col, ' ', 2)      a view out either way
    dbhip_str_build_bytes + dbhip_str_build(UPPER)  beside  replace(' ', '_'), replace(' ', ''), reverse (units and bytes) and
                                                            lpad(col, 20, '*'), each the count call plus the rewrite call
Each shape runs once as a warm-up and then 5 times between two device events on the synchronised stream. Prints (and appends to
out.jsonl) one JSON line per column: per shape the 5 times, their median, rows/s, the bytes touched (a model, below), the spread
(max - min) / median, and beside its yardstick the ratio of the medians and the ratio of the models: the second is the expectation for
the first. Every figure is guarded by a checksum: the output is filled with 0xFF before the timed runs and the sum of the results
(positions, matching rows, result lengths) afterwards must be the one computed on the host from the column's pool of values — a call
that did nothing is not timed."""
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

NEEDLE = {"p_type_inline": b"BRASS", "p_name_mixed": b"green", "o_comment_long": b"special"}


def words(nbytes):
    """the aligned 4-byte words that hold nbytes[i] bytes of each long value, one word more for a value that starts off a boundary"""
    return int(((nbytes.astype(np.int64) + 3) // 4 * 4 + 4).sum())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    D.init(0)
    rng = np.random.default_rng(7)
    L = T.lib()
    views_out = D.DeviceBuffer(n * 16)
    pos_out = D.DeviceBuffer(n * 8)
    bits_out = D.DeviceBuffer(((n + 63) // 64) * 8 + 8)
    two, twenty = D.Column.scalar(2, T.T_I64), D.Column.scalar(20, T.T_I64)
    c2, c20 = two.c(), twenty.c()
    space, under, star = (C.c_uint8 * 1)(0x20), (C.c_uint8 * 1)(0x5F), (C.c_uint8 * 1)(0x2A)
    lines = []
    for name, pool in columns(n, rng):
        pick = rng.integers(0, len(pool), TILE)
        col, lens, _ = build_column(pool, pick, n)
        cc = col.c()
        rows_pool = np.tile(pick, (n + TILE - 1) // TILE)[:n]             # the pool value of every row
        is_long = lens > 12
        long_lens = lens[is_long]
        rows_of = np.bincount(rows_pool, minlength=len(pool))
        needle = NEEDLE[name]
        nbuf = (C.c_uint8 * len(needle)).from_buffer_copy(needle)

        def expect(f):
            return int(sum(int(k) * f(v) for v, k in zip(pool, rows_of)))

        def per_long_row(f):
            """f(value) for every long row, as an array"""
            return np.array([f(v) for v in pool], dtype=np.int64)[rows_pool][is_long]

        res = dict(column=name, rows=n, long_rows=int(len(long_lens)), long_bytes=int(long_lens.astype(np.int64).sum()), hbm_peak_bytes_per_s=HBM_PEAK,
                   needle=needle.decode(), shapes={})

        def record(label, fn, nbytes, out, checksum, want, yardstick=None):
            T.check(L.dbhip_memset(C.c_void_p(out.ptr), 0xFF, C.c_size_t(out.nbytes), None))
            ms = timed(fn)
            got = checksum()
            assert got == want, (name, label, got, want)
            med = float(np.median(ms))
            s = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4), rows_per_s=round(n / (med / 1e3)),
                     touched_bytes=int(nbytes), bytes_per_row=round(nbytes / n, 2), share_of_hbm_peak=round(nbytes / (med / 1e3) / HBM_PEAK, 4), checksum=got)
            if yardstick:
                y = res["shapes"][yardstick]
                s.update(yardstick=yardstick, ratio_to_yardstick=round(med / y["median_ms"], 3), model_ratio=round(nbytes / y["touched_bytes"], 3))
            res["shapes"][label] = s

        def view_lens():
            return int(views_out.to_numpy(np.uint32, n * 4)[0::4].astype(np.int64).sum())

        # ---- position beside CONTAINS: the views, the whole of every long value that does not hold the needle, up to the match's end otherwise
        searched = words(per_long_row(lambda v: (v.find(needle) + len(needle)) if needle in v else len(v)))
        contains = "str_match CONTAINS"
        record(contains, lambda: T.check(L.dbhip_str_match(T.LIKE_CONTAINS, C.byref(cc), nbuf, C.c_int32(len(needle)), C.c_int32(0), C.c_int64(n), C.c_void_p(bits_out.ptr), None)),
               16 * n + n // 8 + searched, bits_out, lambda: D.bitmap_count(D.Column(T.T_BOOL, n, bits_out), n), expect(lambda v: int(needle in v)))
        for mode, flags in (("unit", 0), ("byte", T.STR_UNIT_BYTE)):
            record(f"position {mode}", lambda: T.check(L.dbhip_str_position(C.byref(cc), nbuf, C.c_int32(len(needle)), None, C.c_int32(flags), C.c_int64(n), C.c_void_p(pos_out.ptr), None)),
                   24 * n + searched, pos_out, lambda: int(pos_out.to_numpy(np.uint64, n).sum()), expect(lambda v: v.find(needle) + 1), contains)

        # ---- split_part beside trim: 16 B in and 16 B out; trim looks at the ends of a long value, split_part(' ', 2) up to the second space
        trim = "str_slice TRIM_BOTH ' '"
        record(trim, lambda: T.check(L.dbhip_str_slice(T.STR_TRIM_BOTH, C.byref(cc), None, None, space, C.c_int32(1), C.c_int32(0), C.c_int64(n), C.c_void_p(views_out.ptr), None)),
               32 * n + 2 * words(np.minimum(long_lens, 1)), views_out, view_lens, expect(lambda v: len(v.strip(b" "))))

        def second_space(v):
            cut = v.split(b" ", 2)
            return len(v) if len(cut) < 3 else len(cut[0]) + len(cut[1]) + 2
        record("split_part(col, ' ', 2)", lambda: T.check(L.dbhip_str_split_part(C.byref(cc), space, C.c_int32(1), C.byref(c2), C.c_int64(n), C.c_void_p(views_out.ptr), None)),
               32 * n + words(per_long_row(second_space)), views_out, view_lens, expect(lambda v: len(v.split(b" ")[1]) if v.count(b" ") else 0), trim)

        # ---- rewrites beside upper: the count call (views in), then count + scan + fill (+ the wave-per-row pass): views in three times,
        # 4 B counts out and in twice, 8 B offsets out and in, the view out, the result's bytes out; value bytes in once per pass that looks
        fixed = (3 * 16 + 4 + 4 + 4 + 8 + 8 + 16) * n
        whole = words(long_lens)
        upper = "str_build UPPER"
        arr = (T.Col * 1)(cc)
        nbytes = C.c_uint64(0)
        T.check(L.dbhip_str_build_bytes(T.STR_UPPER, arr, C.c_int32(1), C.c_int64(n), C.byref(nbytes), None))
        data = D.DeviceBuffer(max(nbytes.value, 2 * int(lens.astype(np.int64).sum())) + 20 * n)      # room for every shape below

        def upper_call():
            T.check(L.dbhip_str_build_bytes(T.STR_UPPER, arr, C.c_int32(1), C.c_int64(n), C.byref(nbytes), None))
            T.check(L.dbhip_str_build(T.STR_UPPER, arr, C.c_int32(1), C.c_int64(n), C.c_void_p(views_out.ptr), C.c_void_p(data.ptr), C.c_uint64(nbytes.value), None, None, None, None))
        record(upper, upper_call, fixed + whole + nbytes.value, views_out, view_lens, expect(len))

        def rewrite_shape(label, op, k, x, x_len, y, y_len, flags, passes, result):
            """passes: how many of the three passes read the long values' bytes"""
            kp = C.byref(k) if k is not None else None
            got = C.c_uint64(0)

            def call():
                T.check(L.dbhip_str_rewrite_bytes(op, C.byref(cc), kp, x, C.c_int32(x_len), y, C.c_int32(y_len), C.c_int32(flags), C.c_int64(n), C.byref(got), None))
                T.check(L.dbhip_str_rewrite(op, C.byref(cc), kp, x, C.c_int32(x_len), y, C.c_int32(y_len), C.c_int32(flags), C.c_int64(n), C.c_void_p(views_out.ptr),
                                            C.c_void_p(data.ptr), C.c_uint64(got.value), None, None))
            out_bytes = expect(lambda v: len(result(v)) if len(result(v)) > 12 else 0)
            record(label, call, fixed + passes * whole + out_bytes, views_out, view_lens, expect(lambda v: len(result(v))), upper)
            assert got.value == out_bytes, (name, label, got.value, out_bytes)
            res["shapes"][label]["out_data_bytes"] = out_bytes

        rewrite_shape("replace(' ', '_')", T.STRW_REPLACE, None, space, 1, under, 1, 0, 3, lambda v: v.replace(b" ", b"_"))
        rewrite_shape("replace(' ', '')", T.STRW_REPLACE, None, space, 1, None, 0, 0, 3, lambda v: v.replace(b" ", b""))
        rewrite_shape("reverse unit", T.STRW_REVERSE, None, None, 0, None, 0, 0, 1, lambda v: v[::-1])
        rewrite_shape("reverse byte", T.STRW_REVERSE, None, None, 0, None, 0, T.STR_UNIT_BYTE, 1, lambda v: v[::-1])
        rewrite_shape("lpad(col, 20, '*') unit", T.STRW_LPAD, c20, star, 1, None, 0, 0, 3, lambda v: v.rjust(20, b"*")[:20] if len(v) < 20 else v[:20])
        line = json.dumps(res)
        print(line)
        lines.append(line)
        del col, data
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
