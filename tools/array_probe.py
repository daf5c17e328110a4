"""Times the Array functions (include/dbhip.h a29) on synthetic Array columns resident in HBM:
    python tools/array_probe.py [elements] [out.jsonl]
defaults: about 32 Mi elements per column; three row shapes — short (0 .. 8 elements a row), medium (64 .. 256) and long (a few
thousand rows of 4,096 .. 12,288 elements) — for Int64 and Float32 children without NULLs. Every shape stands beside a yardstick taken
in the same run on the same buffers:
    dbhip_sum over the child                        beside  array_sum            the same elements in; one value out per row instead of one
    dbhip_take of n elements (each row's first)     beside  array_get(arr, 1)    the same gather; get reads the offsets instead of a selection
    dbhip_cmp(EQ, child, scalar)                    beside  array_contains       the same elements in; one bit out per row instead of per element
    dbhip_take of num_out u32 (a shuffled iota)     beside  unnest_sel           the same u32 out; unnest reads the offsets instead of a selection
Each shape runs once as a warm-up and then 5 times between two device events on the synchronised stream. Prints (and appends to
out.jsonl) one JSON line per column: per shape the 5 times, their median, elements/s, the bytes touched (a model, below), the spread
(max - min) / median, and beside its yardstick the ratio of the medians and the ratio of the models: the second is the expectation for
the first. Every figure is guarded by a checksum: the output is filled with 0xFF before the timed runs and the sum of the results
afterwards must be the one computed on the host from the column — a call that did nothing is not timed."""
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

NEEDLE = 5000                               # the elements are 0 .. 999; the needle is the last element of every tenth row that has one
SHAPES = {"short 0..8": (0, 9), "medium 64..256": (64, 257), "long 4096..12288": (4096, 12289)}


def main():
    target = int(sys.argv[1]) if len(sys.argv) > 1 else 32 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    D.init(0)
    L = T.lib()
    lines = []
    for shape, (lo, hi) in SHAPES.items():
        rng = np.random.default_rng(lo + 3)
        n = max(int(target // ((lo + hi - 1) / 2)), 1)
        lens = rng.integers(lo, hi, n).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ne = int(off[-1])
        ints = rng.integers(0, 1000, ne).astype(np.int64)
        has = (np.arange(n) % 10 == 0) & (lens > 0)
        ints[(off[1:][has] - 1).astype(np.int64)] = NEEDLE
        first = np.where(lens > 0, off[:-1], 0).astype(np.uint32)            # the selection of the take beside get
        offsets = D.DeviceBuffer.from_numpy(off)
        sel_first = D.DeviceBuffer.from_numpy(first)
        shuffled = D.DeviceBuffer.from_numpy(rng.permutation(ne).astype(np.uint32))
        iota = D.DeviceBuffer.from_numpy(np.arange(ne, dtype=np.uint32))
        for tname, dt, code, es in (("i64", np.int64, T.T_I64, 8), ("f32", np.float32, T.T_F32, 4)):
            vals = ints.astype(dt)
            child = D.Column.from_numpy(vals)
            cc = child.c()
            needle = D.Column.scalar(NEEDLE, code)
            cn = needle.c()
            one = D.Column.scalar(1, T.T_I64)
            c1 = one.c()
            out_rows = D.DeviceBuffer(n * 8 + 64)
            out_valid = D.DeviceBuffer(((n + 63) // 64) * 8 + 8)
            out_elems = D.DeviceBuffer(ne * 4 + 64)
            out_bits = D.DeviceBuffer(((ne + 63) // 64) * 8 + 8)
            out_sum = D.DeviceBuffer(64)
            args = (C.byref(cc), C.c_void_p(offsets.ptr), C.c_int64(n), C.c_uint64(ne))
            res = dict(column=f"{shape} {tname}", rows=n, elements=ne, elem_bytes=es, hbm_peak_bytes_per_s=HBM_PEAK, long_len=T.ARRAY_LONG_LEN,
                       stage_bytes=T.ARRAY_STAGE_BYTES, shapes={})

            def record(label, fn, nbytes, out, checksum, want, yardstick=None):
                T.check(L.dbhip_memset(C.c_void_p(out.ptr), 0xFF, C.c_size_t(out.nbytes), None))
                ms = timed(fn)
                got = checksum()
                assert got == want, (shape, tname, label, got, want)
                med = float(np.median(ms))
                s = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4), elements_per_s=round(ne / (med / 1e3)),
                         touched_bytes=int(nbytes), share_of_hbm_peak=round(nbytes / (med / 1e3) / HBM_PEAK, 4), checksum=got)
                if yardstick:
                    y = res["shapes"][yardstick]
                    s.update(yardstick=yardstick, ratio_to_yardstick=round(med / y["median_ms"], 3), model_ratio=round(nbytes / y["touched_bytes"], 3))
                res["shapes"][label] = s

            def as_num(buf, count, dtype):
                return int(buf.to_numpy(dtype, count).astype(np.float64 if np.dtype(dtype).kind == "f" else np.uint64).sum())

            total = int(ints.sum())
            rdt = np.float64 if tname == "f32" else np.int64

            # ---- sum: the child in; the offsets in and 8 B + a bit out per row
            def child_sum():
                T.check(L.dbhip_memset(C.c_void_p(out_sum.ptr), 0, C.c_size_t(8), None))     # (it is accumulated into)
                T.check(L.dbhip_sum(C.byref(cc), C.c_int64(ne), C.c_void_p(out_sum.ptr), None))
            record("dbhip_sum child", child_sum, ne * es, out_sum, lambda: as_num(out_sum, 1, rdt), total)
            record("array_sum", lambda: T.check(L.dbhip_array_reduce(T.ARR_SUM, *args, C.c_void_p(out_rows.ptr), C.c_void_p(out_valid.ptr), None, None)),
                   ne * es + (n + 1) * 8 + n * 8 + n // 8, out_rows, lambda: as_num(out_rows, n, rdt), total, "dbhip_sum child")

            # ---- get: a gather of one element per row
            firsts = int(ints[first.astype(np.int64)][lens > 0].sum()) if ne else 0
            want_take = int(ints[first.astype(np.int64)].sum()) if ne else 0
            record("dbhip_take first", lambda: T.check(L.dbhip_take(C.c_void_p(child.data.ptr), es, C.c_void_p(sel_first.ptr), C.c_int64(n), C.c_void_p(out_rows.ptr), None)),
                   n * 4 + 2 * n * es, out_rows, lambda: as_num(out_rows, n, dt), want_take)
            record("array_get(arr, 1)", lambda: T.check(L.dbhip_array_get(*args, C.byref(c1), C.c_void_p(out_rows.ptr), C.c_void_p(out_valid.ptr), None)),
                   (n + 1) * 8 + 2 * n * es + n // 8, out_rows, lambda: as_num(out_rows, n, dt), firsts, "dbhip_take first")

            # ---- contains: every element compared (the needle is a row's last element or absent)
            record("dbhip_cmp EQ child", lambda: T.check(L.dbhip_cmp(T.CMP_EQ, C.byref(cc), C.byref(cn), C.c_int64(ne), C.c_void_p(out_bits.ptr), None)),
                   ne * es + ne // 8, out_bits, lambda: D.bitmap_count(D.Column(T.T_BOOL, ne, out_bits), ne), int(has.sum()))
            record("array_contains", lambda: T.check(L.dbhip_array_find(T.ARR_CONTAINS, *args, C.byref(cn), C.c_void_p(out_valid.ptr), None)),
                   ne * es + (n + 1) * 8 + n // 8, out_valid, lambda: D.bitmap_count(D.Column(T.T_BOOL, n, out_valid), n), int(has.sum()), "dbhip_cmp EQ child")

            # ---- unnest_sel: num_out u32 out
            if tname == "i64":
                record("dbhip_take u32", lambda: T.check(L.dbhip_take(C.c_void_p(iota.ptr), 4, C.c_void_p(shuffled.ptr), C.c_int64(ne), C.c_void_p(out_elems.ptr), None)),
                       3 * ne * 4, out_elems, lambda: as_num(out_elems, ne, np.uint32), ne * (ne - 1) // 2)
                record("unnest_sel", lambda: T.check(L.dbhip_array_unnest_sel(C.c_void_p(offsets.ptr), C.c_int64(n), C.c_uint64(ne), C.c_void_p(out_elems.ptr), C.c_int64(ne), None)),
                       (n + 1) * 8 + ne * 4, out_elems, lambda: as_num(out_elems, ne, np.uint32), int((np.arange(n, dtype=np.int64) * lens).sum()), "dbhip_take u32")
            line = json.dumps(res)
            print(line)
            lines.append(line)
            del child, out_rows, out_valid, out_elems, out_bits
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
