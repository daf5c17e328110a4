"""Times dbhip_like (include/dbhip.h a20) for the constant LIKE patterns of six TPC-H queries (seven patterns) on synthetic String columns resident in HBM:
    python tools/like_probe.py [rows] [out.jsonl]
defaults: 16 Mi rows. Three columns, built from the TPC-H word lists with numpy (no dbgen):
    p_type     inline-only   "<size> <finish> <metal>" cut to 12 bytes (every value sits in its view)
    p_name     mixed         five colour words; about a third of the values are <= 12 bytes after a seeded cut, the others long
    o_comment  all-long      19 .. 78 bytes of comment words, "special ... requests" / "Customer ... Complaints" planted in ~1 %
Every pattern runs on every column. Each shape runs once as a warm-up and then 5 times between two device events on the synchronised
stream. Beside it: dbhip_cmp EQ against a scalar String on the same column, the one string predicate the library had before, in the
same run. Prints (and appends to out.jsonl) one JSON line per column: per pattern the 5 times, their median, rows/s, the bytes touched
(touched_bytes below: a model) per second as a share of the 8.0 TB/s HBM peak, the spread (max - min) / median of the five repetitions,
and the number of matching rows (a guard against timing a call that did nothing)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402

HBM_PEAK = 8.0e12
PATTERNS = [("Q2", b"%BRASS"), ("Q9", b"%green%"), ("Q13", b"%special%requests%"), ("Q14", b"PROMO%"), ("Q16a", b"MEDIUM POLISHED%"),
            ("Q16b", b"%Customer%Complaints%"), ("Q20", b"forest%")]
SIZES = [b"STANDARD", b"SMALL", b"MEDIUM", b"LARGE", b"ECONOMY", b"PROMO"]
FINISH = [b"ANODIZED", b"BURNISHED", b"PLATED", b"POLISHED", b"BRUSHED"]
METAL = [b"TIN", b"NICKEL", b"BRASS", b"STEEL", b"COPPER"]
COLOURS = [b"almond", b"antique", b"aquamarine", b"azure", b"beige", b"bisque", b"black", b"blanched", b"blue", b"blush", b"brown", b"burlywood",
           b"chartreuse", b"chiffon", b"coral", b"cornflower", b"cyan", b"dark", b"dim", b"dodger", b"drab", b"firebrick", b"floral", b"forest",
           b"frosted", b"ghost", b"goldenrod", b"green", b"grey", b"honeydew", b"hot", b"indian", b"ivory", b"khaki", b"lace", b"lavender"]
WORDS = [b"furiously", b"sly", b"careful", b"blithe", b"quick", b"fluffy", b"slow", b"quiet", b"ruthless", b"thin", b"close", b"dogged", b"packages",
         b"requests", b"accounts", b"deposits", b"foxes", b"ideas", b"theodolites", b"pinto beans", b"instructions", b"special", b"Customer",
         b"Complaints", b"regular", b"express", b"even", b"final", b"unusual", b"ironic", b"pending", b"bold"]


def timed(fn):
    L = T.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        T.check(L.dbhip_event_create(C.byref(e)))
    fn()                                     # warm-up
    ms = []
    for _ in range(5):
        T.check(L.dbhip_stream_sync(None))
        T.check(L.dbhip_event_record(ev[0], None))
        fn()
        T.check(L.dbhip_event_record(ev[1], None))
        T.check(L.dbhip_stream_sync(None))
        out = C.c_float()
        T.check(L.dbhip_event_elapsed_ms(ev[0], ev[1], C.byref(out)))
        ms.append(out.value)
    for e in ev:
        L.dbhip_event_destroy(e)
    return ms


TILE = 1 << 16


def build_column(pool, pick, n):
    """pool: distinct values; pick: one pool index per row of a tile of TILE rows, which the column repeats -> (Column, lens, first words).
    Every long row has its own bytes in the data buffer, back to back without padding (the tiles' images follow each other)."""
    lens_pool = np.array([len(v) for v in pool], dtype=np.uint32)
    inl_pool = np.frombuffer(b"".join(v.ljust(12, b"\0") if len(v) <= 12 else v[:4].ljust(12, b"\0") for v in pool), dtype=np.uint32).reshape(-1, 3)
    tile = np.zeros((TILE, 4), dtype=np.uint32)
    tile[:, 0] = lens_pool[pick]
    tile[:, 1:4] = inl_pool[pick]
    long_rows = np.nonzero(tile[:, 0] > 12)[0]
    tile_bytes = b"".join(pool[k] for k in pick[long_rows])
    offs = np.concatenate([[0], np.cumsum(tile[long_rows, 0].astype(np.int64))])
    tile[long_rows, 2] = 0
    tile[long_rows, 3] = offs[:-1].astype(np.uint32)
    reps = (n + TILE - 1) // TILE
    assert reps * len(tile_bytes) < 2**32
    views = np.tile(tile, (reps, 1))
    is_long = views[:, 0] > 12
    views[:, 3] += np.where(is_long, np.repeat(np.arange(reps, dtype=np.uint32) * np.uint32(len(tile_bytes)), TILE), np.uint32(0))
    views = views[:n]
    dbuf = D.DeviceBuffer.from_numpy(np.tile(np.frombuffer(tile_bytes, dtype=np.uint8), reps))
    ptrs = D.DeviceBuffer.from_numpy(np.array([dbuf.ptr], dtype=np.uint64))
    return D.Column(T.T_STRING, n, D.DeviceBuffer.from_numpy(views), None, buffers=ptrs, keep=(dbuf,)), views[:, 0].copy(), views[:, 1].copy()


def columns(n, rng):
    ptype = [(a + b" " + b + b" " + c)[:12] for a in SIZES for b in FINISH for c in METAL] + [b"PROMO BRASS", b"TIN BRASS", b"MEDIUM BRASS"]
    pname = []
    for _ in range(4000):
        v = b" ".join(COLOURS[k] for k in rng.integers(0, len(COLOURS), 5))
        pname.append(v[:int(rng.integers(5, 13))] if rng.random() < 0.33 else v)
    comment = []
    for k in range(4000):
        v = b" ".join(WORDS[j] for j in rng.integers(0, len(WORDS), 12))
        if k % 100 == 0:
            v = b"the special packages of requests " + v
        if k % 100 == 1:
            v = b"a Customer with Complaints " + v
        comment.append(v[:int(rng.integers(19, 79))])
    return [("p_type_inline", ptype), ("p_name_mixed", pname), ("o_comment_long", comment)]


def touched_bytes(kind, needle, lens, first_words):
    """a model, not a counter: 16 bytes per view and one result bit per row, plus the 4-byte words of the long values the kind has to
    read (a value that does not start on a word boundary spans one word more): the whole value for CONTAINS / SEGMENTS, the needle's
    words at the tail for SUFFIX, the needle's words behind the first four bytes for PREFIX / EQUALS where the view's prefix word agrees"""
    n, m = len(lens), len(needle)
    is_long = lens > 12
    if kind in (T.LIKE_CONTAINS, T.LIKE_SEGMENTS):
        extra = int(((lens[is_long].astype(np.int64) + 3) // 4 * 4 + 4).sum())
    elif kind == T.LIKE_SUFFIX:
        extra = int((is_long & (lens >= m)).sum()) * ((m + 3) // 4 * 4 + 4)
    elif m <= 4:
        extra = 0
    else:
        w0 = int.from_bytes(needle[:4], "little")
        fits = (lens >= m) if kind == T.LIKE_PREFIX else (lens == m)
        extra = int((is_long & fits & (first_words == w0)).sum()) * ((m - 4 + 3) // 4 * 4 + 4)
    return 16 * n + n // 8 + extra


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    D.init(0)
    rng = np.random.default_rng(7)
    L = T.lib()
    out = D.DeviceBuffer(((n + 63) // 64) * 8 + 8)
    lines = []
    for name, pool in columns(n, rng):
        col, lens, first_words = build_column(pool, rng.integers(0, len(pool), TILE), n)
        cc = col.c()
        res = dict(column=name, rows=n, long_rows=int((lens > 12).sum()), long_bytes=int(lens[lens > 12].astype(np.int64).sum()),
                   hbm_peak_bytes_per_s=HBM_PEAK, shapes={})

        def record(label, fn, nbytes, extra):
            ms = timed(fn)
            med = float(np.median(ms))
            hits = D.bitmap_count(D.Column(T.T_BOOL, n, out), n)
            res["shapes"][label] = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4),
                                        rows_per_s=round(n / (med / 1e3)), touched_bytes=int(nbytes),
                                        share_of_hbm_peak=round(nbytes / (med / 1e3) / HBM_PEAK, 4), matches=hits, **extra)

        for q, pattern in PATTERNS:
            kind = D.like_kind(pattern)
            buf = (C.c_uint8 * len(pattern)).from_buffer_copy(pattern)
            record(f"{q} {pattern.decode()}",
                   lambda: T.check(L.dbhip_like(C.byref(cc), buf, C.c_int32(len(pattern)), C.c_int32(0x5C), C.c_int32(0), C.c_int64(n), C.c_void_p(out.ptr), None)),
                   touched_bytes(kind, pattern.replace(b"%", b""), lens, first_words), dict(kind=kind))
        # the yardstick: dbhip_cmp EQ against a scalar String (a value of the column's own pool) on the same column, and the same
        # comparison through dbhip_str_match
        eq = pool[0]
        scalar = D.Column.strings([eq])
        scalar.is_scalar = True
        sc = scalar.c()
        eq_bytes = touched_bytes(T.LIKE_EQUALS, eq, lens, first_words)
        record("dbhip_cmp EQ scalar", lambda: T.check(L.dbhip_cmp(T.CMP_EQ, C.byref(cc), C.byref(sc), C.c_int64(n), C.c_void_p(out.ptr), None)),
               eq_bytes, dict(value_len=len(eq)))
        ebuf = (C.c_uint8 * len(eq)).from_buffer_copy(eq)
        record("dbhip_str_match EQUALS same value",
               lambda: T.check(L.dbhip_str_match(T.LIKE_EQUALS, C.byref(cc), ebuf, C.c_int32(len(eq)), C.c_int32(0), C.c_int64(n), C.c_void_p(out.ptr), None)),
               eq_bytes, dict(value_len=len(eq)))
        pre = eq[:5]
        pbuf = (C.c_uint8 * len(pre)).from_buffer_copy(pre)
        record("dbhip_str_match PREFIX first 5 bytes",
               lambda: T.check(L.dbhip_str_match(T.LIKE_PREFIX, C.byref(cc), pbuf, C.c_int32(len(pre)), C.c_int32(0), C.c_int64(n), C.c_void_p(out.ptr), None)),
               touched_bytes(T.LIKE_PREFIX, pre, lens, first_words), dict(value_len=len(pre)))
        line = json.dumps(res)
        print(line)
        lines.append(line)
        del col
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
