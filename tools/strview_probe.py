"""Times the String paths that read views through databend_amd/csrc/dev_strview.h, for same-box A/B runs of two builds of the library
(DBHIP_LIBRARY names the build, databend_amd/_lib.py):
    python tools/strview_probe.py <label> <out.jsonl>
4 Mi rows, HIP events, two warm-ups and five repetitions per shape: dbhip_cmp EQ / LT column against column, dbhip_group_hash,
dbhip_sort_perm, a GroupBy with a String key (count), dbhip_window_bounds — each over a column of inline values (0 .. 12 bytes) and
over one of 24-byte values that each have their own bytes in the data buffer. Appends one JSON line: {label, library, name: [ms x 5]}.
profiles/strview_ab.json was taken with it."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402

N = 4 << 20


def timed(fn, reps=5, warm=2):
    L = T.lib()
    for _ in range(warm):
        fn()
    T.check(L.dbhip_stream_sync(None))
    e0, e1 = C.c_void_p(), C.c_void_p()
    T.check(L.dbhip_event_create(C.byref(e0)))
    T.check(L.dbhip_event_create(C.byref(e1)))
    out = []
    for _ in range(reps):
        T.check(L.dbhip_event_record(e0, None))
        fn()
        T.check(L.dbhip_event_record(e1, None))
        T.check(L.dbhip_stream_sync(None))
        ms = C.c_float()
        T.check(L.dbhip_event_elapsed_ms(e0, e1, C.byref(ms)))
        out.append(round(ms.value, 4))
    return out


def inline_col(rng, n, card=None, sort=False):
    """values of 0 .. 12 bytes over a small alphabet (card: that many distinct values)"""
    m = card or n
    lens = rng.integers(0, 13, m).astype(np.uint32)
    pay = rng.integers(97, 101, (m, 12)).astype(np.uint8)
    pay[np.arange(12)[None, :] >= lens[:, None]] = 0
    views = np.zeros((m, 4), np.uint32)
    views[:, 0] = lens
    views[:, 1:4] = pay.view(np.uint32).reshape(m, 3)
    if card:
        ids = rng.integers(0, card, n)
        if sort:
            ids = np.sort(ids)          # equal values adjacent
        views = views[ids]
    return D.Column(T.T_STRING, n, D.DeviceBuffer.from_numpy(np.ascontiguousarray(views)))


def long_col(rng, n, card, sort=False):
    """values of 24 bytes, `card` distinct ones; every row has its own bytes in the buffer"""
    pool = rng.integers(97, 101, (card, 24)).astype(np.uint8)
    ids = rng.integers(0, card, n)
    if sort:
        ids = np.sort(ids)
    data = pool[ids]
    views = np.zeros((n, 4), np.uint32)
    views[:, 0] = 24
    views[:, 1] = np.ascontiguousarray(data[:, :4]).view(np.uint32).reshape(n)
    views[:, 3] = np.arange(n, dtype=np.uint32) * 24
    dbuf = D.DeviceBuffer.from_numpy(data.reshape(-1))
    ptrs = D.DeviceBuffer.from_numpy(np.array([dbuf.ptr], dtype=np.uint64))
    return D.Column(T.T_STRING, n, D.DeviceBuffer.from_numpy(views), buffers=ptrs, keep=(dbuf,))


def main():
    label, out_path = sys.argv[1], sys.argv[2]
    D.init(0)
    L = T.lib()
    rng = np.random.default_rng(5)
    res = {"label": label, "library": T.library_path(), "rows": N}
    a, b = inline_col(rng, N), inline_col(rng, N)
    la, lb = long_col(rng, N, 1000), long_col(rng, N, 1000)
    bits = D.DeviceBuffer(((N + 63) // 64) * 8 + 8)
    for name, x, y in (("inline", a, b), ("long", la, lb)):
        cx, cy = x.c(), y.c()
        for op, opn in ((T.CMP_EQ, "eq"), (T.CMP_LT, "lt")):
            res[f"cmp_{opn}_{name}"] = timed(lambda: T.check(L.dbhip_cmp(op, C.byref(cx), C.byref(cy), C.c_int64(N), C.c_void_p(bits.ptr), None)))
    hashes = D.DeviceBuffer(N * 8)
    perm = D.DeviceBuffer(N * 4)
    zero = (C.c_uint8 * 1)(0)
    for name, x in (("inline", a), ("long", la)):
        arr = D._cols([x])
        res[f"group_hash_{name}"] = timed(lambda: T.check(L.dbhip_group_hash(arr, 1, C.c_int64(N), C.c_void_p(hashes.ptr), None)))
        res[f"sort_perm_{name}"] = timed(lambda: T.check(L.dbhip_sort_perm(arr, zero, zero, 1, C.c_int64(N), C.c_int64(0), C.c_void_p(perm.ptr), None)), reps=5, warm=1)
    for name, x in (("inline_1000", inline_col(rng, N, card=1000)), ("long_1000", long_col(rng, N, 1000))):
        g = D.GroupBy([T.T_STRING], [(T.AGG_COUNT, 0, 0, 0, 0)])

        def add():
            g.reset()
            g.add_block([x], [None], N)
        res[f"groupby_count_{name}"] = timed(add)
        res[f"groupby_groups_{name}"] = g.num_groups()
        g.destroy()
    for name, x in (("inline_1000", inline_col(rng, N, card=1000, sort=True)), ("long_1000", long_col(rng, N, 1000, sort=True))):
        arrays = [D.DeviceBuffer(N * 4) for _ in range(4)]
        rows = T.WindowRows()
        rows.n = N
        rows.part_start, rows.part_end, rows.peer_start, rows.peer_end = [q.ptr for q in arrays]
        arr = D._cols([x])
        res[f"window_bounds_{name}"] = timed(lambda: T.check(L.dbhip_window_bounds(arr, 1, None, 0, C.c_int64(N), C.byref(rows), None)))
        res[f"window_partitions_{name}"] = int(len(np.unique(arrays[0].to_numpy(np.uint32, N))))
    line = json.dumps(res)
    print(line)
    with open(out_path, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
