"""Times the window calls (include/dbhip.h a19) on one sorted input resident in HBM:
    python tools/window_probe.py [rows] [rows_per_partition]
defaults: 64 Mi rows, an i64 partition key with 1,000 rows per partition, an i64 order key with ties (three rows per value). The boundary
arrays and every output are allocated before the clock starts. Each shape runs once as a warm-up and then 5 times between two device
events on the synchronised stream. Prints one JSON line: per shape the 5 times, their median, the algorithmic bytes (what the call
must read and write given its shapes, not what the kernels move) and the share of the 8.0 TB/s HBM peak that median amounts to."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402

HBM_PEAK = 8.0e12


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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64 << 20
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    D.init(0)
    rng = np.random.default_rng(5)
    i = np.arange(n, dtype=np.int64)
    p = D.Column.from_numpy(i // per)
    o = D.Column.from_numpy((i % per) // 3)
    del i
    vi = D.Column.from_numpy(rng.integers(-10**12, 10**12, n))
    vf = D.Column.from_numpy(rng.standard_normal(n))
    w = D.Window([p], [o])
    out = D.DeviceBuffer(n * 8 + 64)
    val = D.DeviceBuffer(((n + 63) // 64) * 8 + 8)
    L = T.lib()
    pc, oc = D._cols([p]), D._cols([o])
    running = D.WindowFrame(T.WIN_ROWS, T.WIN_UNBOUNDED_PRECEDING, T.WIN_CURRENT_ROW)
    last10 = D.WindowFrame(T.WIN_ROWS, (T.WIN_PRECEDING, 10), T.WIN_CURRENT_ROW)
    around = D.WindowFrame(T.WIN_ROWS, (T.WIN_PRECEDING, 100), (T.WIN_FOLLOWING, 100))
    bit = 1 / 8
    shapes = [
        # name, call, algorithmic bytes per row
        ("bounds", lambda: T.check(L.dbhip_window_bounds(pc, 1, oc, 1, C.c_int64(n), C.byref(w.rows), None)), 8 + 8 + 4 * 4),
        ("rank", lambda: w.rank(T.WIN_RANK, out=out, device=True), 4 + 4 + 8),
        ("dense_rank", lambda: w.rank(T.WIN_DENSE_RANK, out=out, device=True), 4 + 4 + 8),
        ("running_sum_i64", lambda: w.aggregate(T.AGG_SUM, vi, running, out=out, out_validity=val, device=True), 8 + 4 + 8 + bit),
        ("running_sum_f64", lambda: w.aggregate(T.AGG_SUM, vf, running, out=out, out_validity=val, device=True), 8 + 4 + 8 + bit),
        ("min_f64_10_preceding", lambda: w.aggregate(T.AGG_MIN, vf, last10, out=out, out_validity=val, device=True), 8 + 4 + 8 + bit),
        ("sum_i64_100_around", lambda: w.aggregate(T.AGG_SUM, vi, around, out=out, out_validity=val, device=True), 8 + 4 + 4 + 8 + bit),
        ("lag_1_i64", lambda: w.shift(vi, -1, out=out, out_validity=val, device=True), 8 + 4 + 8 + bit),
    ]
    res = dict(rows=n, rows_per_partition=per, hbm_peak_bytes_per_s=HBM_PEAK, shapes={})
    for name, fn, per_row in shapes:
        ms = timed(fn)
        med = float(np.median(ms))
        nbytes = per_row * n
        res["shapes"][name] = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), algorithmic_bytes=int(nbytes),
                                   share_of_hbm_peak=round(nbytes / (med / 1e3) / HBM_PEAK, 4))
    # the results of the last runs against a plain prefix sum of the first partitions (a guard against timing a call that did nothing)
    k = 5 * per
    got = out.to_numpy(np.int64, k)
    src = vi.data.to_numpy(np.int64, k + 1)
    assert np.array_equal(got[1:per], src[:per - 1]) and got[per] == 0 and np.array_equal(got[per + 1:2 * per], src[per:2 * per - 1]), "lag(1)"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
