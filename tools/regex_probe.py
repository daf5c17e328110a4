"""Times dbhip_regex_eval (include/dbhip.h a25) on synthetic URL-like String columns resident in HBM:
    python tools/regex_probe.py [rows] [out.jsonl]
defaults: 4 Mi rows. Two columns, built with numpy from a pool of 4,000 distinct URLs (every row has its own bytes in the data
buffer, back to back without padding, as tools/like_probe.py builds them):
    urls           20 .. 90 bytes each
    urls_1pct_4k   the same pool with 1 % of the values replaced by URLs of 4 KB: the long-value cost the design accepts (a long value
                   is walked by its one lane and its wave waits)
Shapes, each once as a warm-up and then 5 times between two device events on the synchronised stream:
    literal   the pattern `google`, beside dbhip_str_match CONTAINS with the same literal (k_like.hip's word-wise search) on the same column
    url       ^https?://(?:www\\.)?([^/]+)/.*$, which has to walk every matching value to its end
Prints (and appends to out.jsonl) one JSON line per column: per shape the 5 times, their median, rows/s, value bytes per second (all
the value bytes of the column, an upper bound of what a walk that stops early reads), the spread (max - min) / median, the DFA's
figures and the number of matching rows (a guard against timing a call that did nothing). There is no target to meet."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from databend_amd import _lib as T          # noqa: E402
from databend_amd import device as D        # noqa: E402
from like_probe import TILE, build_column, timed   # noqa: E402

LITERAL = b"google"
URL = rb"^https?://(?:www\.)?([^/]+)/.*$"
HOSTS = [b"google", b"example", b"databend", b"wikipedia", b"github", b"kernel", b"python", b"rust-lang", b"archive", b"openstreetmap"]
TLDS = [b".com", b".org", b".net", b".io", b".dev"]
WORDS = [b"search", b"docs", b"index.html", b"q=regex", b"images", b"a", b"2026", b"10", b"api", b"v1", b"items", b"42", b"static", b"main.css"]


def url(rng, target=0):
    """one URL-like value; about one in five is no http(s) URL at all. target > 0: padded with path segments to that many bytes"""
    scheme = [b"http://", b"https://", b"https://", b"ftp://", b""][int(rng.integers(0, 5))]
    v = scheme + (b"www." if rng.random() < 0.5 else b"") + HOSTS[int(rng.integers(0, len(HOSTS)))] + TLDS[int(rng.integers(0, len(TLDS)))]
    for _ in range(int(rng.integers(0, 5))):
        v += b"/" + WORDS[int(rng.integers(0, len(WORDS)))]
    while len(v) < target:
        v += b"/" + WORDS[int(rng.integers(0, len(WORDS)))]
    return v[:target] if target else v


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4 << 20
    out_path = sys.argv[2] if len(sys.argv) > 2 else None
    D.init(0)
    rng = np.random.default_rng(25)
    L = T.lib()
    out = D.DeviceBuffer(((n + 63) // 64) * 8 + 8)
    pool = [url(rng) for _ in range(4000)]
    with_long = list(pool)
    for k in range(0, 4000, 100):
        with_long[k] = url(rng, 4096)
    pick = rng.integers(0, 4000, TILE)
    lines = []
    for name, values in (("urls", pool), ("urls_1pct_4k", with_long)):
        col, lens, _ = build_column(values, pick, n)
        cc = col.c()
        value_bytes = int(lens.astype(np.int64).sum())
        res = dict(column=name, rows=n, value_bytes=value_bytes, rows_over_1k=int((lens > 1024).sum()), shapes={})

        def record(label, fn, extra):
            ms = timed(fn)
            med = float(np.median(ms))
            hits = D.bitmap_count(D.Column(T.T_BOOL, n, out), n)
            res["shapes"][label] = dict(ms=[round(x, 3) for x in ms], median_ms=round(med, 3), spread=round((max(ms) - min(ms)) / med, 4),
                                        rows_per_s=round(n / (med / 1e3)), value_bytes_per_s=round(value_bytes / (med / 1e3)), matches=hits, **extra)

        for label, pattern in (("literal google", LITERAL), ("url", URL)):
            rx = D.Regex(pattern)
            record(f"regex {label}",
                   lambda: T.check(L.dbhip_regex_eval(C.c_void_p(rx.handle), C.byref(cc), C.c_int32(0), C.c_int64(n), C.c_void_p(out.ptr), None, None, None)),
                   dict(dfa_states=rx.info[0], byte_classes=rx.info[1], table_bytes=rx.info[2]))
            rx.destroy()
        buf = (C.c_uint8 * len(LITERAL)).from_buffer_copy(LITERAL)
        record("dbhip_str_match CONTAINS google",
               lambda: T.check(L.dbhip_str_match(T.LIKE_CONTAINS, C.byref(cc), buf, C.c_int32(len(LITERAL)), C.c_int32(0), C.c_int64(n), C.c_void_p(out.ptr), None)), {})
        line = json.dumps(res)
        print(line)
        lines.append(line)
        del col
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
