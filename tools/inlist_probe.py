"""Times constant IN-list membership (include/dbhip.h a23) on columns resident in HBM:
    python tools/inlist_probe.py [rows] [out.jsonl] [build label] [--sweep]
defaults: 16 Mi rows; the label (which build of the library ran, for the sweep) goes into every line as `build`. Cases: I32 with 8 elements (TPC-H Q16's p_size), I64 with 8, 64 and 1024, an inline-only String column with 4
(Q19's p_container) and 7 elements (Q22's two-byte phone codes), a String column of 40-byte values with 4 long elements, and the I32
and the Q22 case again in calls of 65,536 rows (the reference's block size). --sweep instead times I64 and the 40-byte String column
with 8, 16, 32 and 64 elements: run against two builds of the library it gives the two rows of numbers behind the COMPARE / TABLE
threshold.
Each case is timed beside what it replaces on the same buffers — k x dbhip_cmp(EQ, col, scalar) + (k - 1) x dbhip_bitmap_binary(OR) —
and beside ONE dbhip_cmp(EQ, col, scalar) of that column, the one-pass floor. Each shape runs once as a warm-up and then 5 times
between two device events on the synchronised stream. Prints (and appends to out.jsonl) one JSON line per case: the 5 times of each
of the three, their medians and spreads, the two ratios, and the call's bytes (the column and the result Bitmap, once) per second as a
share of the 8.0 TB/s HBM peak. Every figure is guarded: the result Bitmap is filled with 0xFF before the timed runs, afterwards it must
equal the composition's Bitmap byte for byte and hold the number of members numpy counts on the host."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402
from like_probe import HBM_PEAK, TILE, build_column, timed     # noqa: E402

PATHS = {T.IN_PATH_BITS: "BITS", T.IN_PATH_COMPARE: "COMPARE", T.IN_PATH_TABLE: "TABLE"}


def stats(ms):
    med = float(np.median(ms))
    return dict(ms=[round(x, 4) for x in ms], median_ms=round(med, 4), spread=round((max(ms) - min(ms)) / med, 4))


def scalar_of(dtype, e):
    if dtype == T.T_STRING:
        c = D.Column.strings([e])
        c.is_scalar = True
        return c
    return D.Column.scalar(e, dtype)


def run_case(label, dtype, col, n, items, members, col_bytes):
    """col: the Column (n rows), items: the list's elements, members: how many rows are members (counted on the host)"""
    L = T.lib()
    words = (n + 63) // 64
    out, acc, tmp = (D.DeviceBuffer(words * 8 + 8) for _ in range(3))
    inl = D.InList(dtype, items)
    cc = col.c()
    scalars = [scalar_of(dtype, e) for e in items]
    cs = [s.c() for s in scalars]

    def in_list():
        T.check(L.dbhip_inlist_eval(C.c_void_p(inl.handle), C.byref(cc), 0, C.c_int64(n), C.c_void_p(out.ptr), None, None))

    def composition():
        T.check(L.dbhip_cmp(T.CMP_EQ, C.byref(cc), C.byref(cs[0]), C.c_int64(n), C.c_void_p(acc.ptr), None))
        for s in cs[1:]:
            T.check(L.dbhip_cmp(T.CMP_EQ, C.byref(cc), C.byref(s), C.c_int64(n), C.c_void_p(tmp.ptr), None))
            T.check(L.dbhip_bitmap_binary(1, C.c_void_p(acc.ptr), C.c_void_p(tmp.ptr), C.c_int64(n), C.c_void_p(acc.ptr), None))

    def single_cmp():
        T.check(L.dbhip_cmp(T.CMP_EQ, C.byref(cc), C.byref(cs[0]), C.c_int64(n), C.c_void_p(tmp.ptr), None))

    T.check(L.dbhip_memset(C.c_void_p(out.ptr), 0xFF, C.c_size_t(out.nbytes), None))
    t_in = timed(in_list)
    t_comp = timed(composition)
    t_one = timed(single_cmp)
    got = out.to_numpy(np.uint8, words * 8)
    nbytes = (n + 7) // 8
    assert np.array_equal(got[:nbytes], acc.to_numpy(np.uint8, nbytes)), (label, "differs from the composition")
    count = int(np.unpackbits(got, bitorder="little").sum())
    assert count == members, (label, count, members)
    touched = col_bytes + words * 8
    a, b, c = stats(t_in), stats(t_comp), stats(t_one)
    res = dict(case=label, rows=n, items=len(items), path=PATHS[inl.path], members=count, in_list=a, composition=dict(b, launches=2 * len(items) - 1), single_cmp=c,
               composition_over_in_list=round(b["median_ms"] / a["median_ms"], 2), in_list_over_single_cmp=round(a["median_ms"] / c["median_ms"], 2),
               touched_bytes=int(touched), share_of_hbm_peak=round(touched / (a["median_ms"] / 1e3) / HBM_PEAK, 4), hbm_peak_bytes_per_s=HBM_PEAK)
    inl.destroy()
    return res


def int_case(label, np_type, dtype, n, k, rng, domain):
    """k elements out of `domain` distinct values, uniformly distributed rows"""
    base = 1 + np.arange(domain, dtype=np.int64) * ((1 << 40) + 7919 if np_type == np.int64 else 1)
    values = rng.permutation(base).astype(np_type)
    arr = values[rng.integers(0, domain, n)]
    items = [int(x) for x in values[:k]]
    members = int(np.isin(arr, values[:k]).sum())
    return run_case(label, dtype, D.Column.from_numpy(arr), n, items, members, arr.nbytes)


def string_case(label, pool, n, items, rng):
    pick = rng.integers(0, len(pool), TILE)
    col, lens, _ = build_column(pool, pick, n)
    rows_of = np.bincount(np.tile(pick, (n + TILE - 1) // TILE)[:n], minlength=len(pool))
    members = int(sum(int(c) for v, c in zip(pool, rows_of) if v in items))
    long_bytes = int(lens[lens > 12].astype(np.int64).sum())
    return run_case(label, T.T_STRING, col, n, items, members, 16 * n + long_bytes)


CONTAINERS = [a + b" " + b for a in (b"SM", b"LG", b"MED", b"JUMBO", b"WRAP") for b in (b"CASE", b"BOX", b"BAG", b"JAR", b"PKG", b"PACK", b"CAN", b"DRUM")]
CODES = [b"%02d" % c for c in range(10, 35)]
LONG40 = [b"%04d" % k + b"-forty-byte-value-of-a-string-column" for k in range(64)]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    sweep = "--sweep" in sys.argv
    n = int(args[0]) if args else 16 << 20
    out_path = args[1] if len(args) > 1 else None
    build = args[2] if len(args) > 2 else None
    D.init(0)
    rng = np.random.default_rng(7)
    small = min(n, 65536)
    if sweep:
        cases = [lambda k=k: int_case(f"sweep i64 k={k}", np.int64, T.T_I64, n, k, rng, 2048) for k in (8, 16, 32, 64)]
        cases += [lambda k=k: string_case(f"sweep string40 k={k}", LONG40, n, LONG40[:k], rng) for k in (8, 16, 32, 64)]
    else:
        cases = [
            lambda: int_case("q16 i32 p_size", np.int32, T.T_I32, n, 8, rng, 50),
            lambda: int_case("i64 k=8", np.int64, T.T_I64, n, 8, rng, 2048),
            lambda: int_case("i64 k=64", np.int64, T.T_I64, n, 64, rng, 2048),
            lambda: int_case("i64 k=1024", np.int64, T.T_I64, n, 1024, rng, 2048),
            lambda: string_case("q19 p_container inline", CONTAINERS, n, [b"SM CASE", b"SM BOX", b"SM PACK", b"SM PKG"], rng),
            lambda: string_case("q22 phone codes inline", CODES, n, [b"13", b"31", b"23", b"29", b"30", b"18", b"17"], rng),
            lambda: string_case("string40 long", LONG40, n, LONG40[:4], rng),
            lambda: int_case("q16 i32 p_size, 65,536-row call", np.int32, T.T_I32, small, 8, rng, 50),
            lambda: string_case("q22 phone codes, 65,536-row call", CODES, small, [b"13", b"31", b"23", b"29", b"30", b"18", b"17"], rng),
        ]
    lines = []
    for case in cases:
        res = case()
        if build:
            res["build"] = build
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
