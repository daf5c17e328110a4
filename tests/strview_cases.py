"""The String column that the GPU tests of every family share to pin what the kernels' view helpers (databend_amd/csrc/dev_strview.h)
have in common. 257 rows — one more than a 256-thread workgroup, so the last row sits alone in a second block and wave — whose lengths
cycle through 0 .. 13, plus one value of 300 bytes; the long values are spread over two data buffers. build() makes the column twice
from the same strings: with clean padding, and with every inline view's bytes past its length set to 0xFF. A kernel that reads an
inline view without masking those bytes, or a long view through the wrong buffer, gives different results for the two."""
import numpy as np

from databend_amd import _lib as T
from tests import oracle_lib as O

N = 257
LONG_ROW = 100
STEMS = (b"ab", b"ba", b"aab", b"a\xff\x00")


def values(inline_only=False):
    """row i: the first i % 14 bytes (i % 13 with inline_only: no long value at all) of one of four repeating stems"""
    out = [(STEMS[(i // 14) % 4] * 7)[:i % (13 if inline_only else 14)] for i in range(N)]
    if not inline_only:
        out[LONG_ROW] = b"ab" * 150
    return out


def views_of(vals, dirty):
    """-> (views u32 [n, 4], [buffer 0, buffer 1] as numpy u8): long value k lies in buffer k % 2, behind three bytes of lead"""
    n = len(vals)
    views = np.zeros((n, 16), dtype=np.uint8)
    parts = [[b"xyz"], [b"xyz"]]
    sizes = [3, 3]
    k = 0
    for i, v in enumerate(vals):
        views[i, 0:4] = np.frombuffer(np.uint32(len(v)).tobytes(), np.uint8)
        if len(v) <= 12:
            views[i, 4:16] = 0xFF if dirty else 0
            views[i, 4:4 + len(v)] = np.frombuffer(v, np.uint8)
        else:
            b = k % 2
            k += 1
            views[i, 4:8] = np.frombuffer(v[:4], np.uint8)
            views[i, 8:16] = np.frombuffer(np.array([b, sizes[b]], dtype=np.uint32).tobytes(), np.uint8)
            parts[b].append(v)
            sizes[b] += len(v)
    return views.view(np.uint32).reshape(n, 4), [np.frombuffer(b"".join(p), dtype=np.uint8).copy() for p in parts]


class Pair:
    """clean / dirty: the two device Columns; host: the oracle's column over the clean views; vals: the strings"""

    def __init__(self, gpu, vals):
        self.vals = vals
        clean, bufs = views_of(vals, False)
        dirty, _ = views_of(vals, True)
        inline = np.array([len(v) <= 12 for v in vals])
        assert (clean[~inline] == dirty[~inline]).all() and (clean[:, 0] == dirty[:, 0]).all()
        assert any(len(v) < 12 for v in vals) and (clean != dirty).any()
        self.host = O.HostCol(T.T_STRING, clean, buffers=bufs)
        dbufs = [gpu.DeviceBuffer.from_numpy(b) for b in bufs]
        ptrs = gpu.DeviceBuffer.from_numpy(np.array([b.ptr for b in dbufs], dtype=np.uint64))
        self.clean, self.dirty = (self._column(gpu, v, ptrs, dbufs) for v in (clean, dirty))

    @staticmethod
    def _column(gpu, views, ptrs, dbufs):
        col = gpu.Column(T.T_STRING, len(views), gpu.DeviceBuffer.from_numpy(views), buffers=ptrs, keep=tuple(dbufs))
        col.n_buffers = 2
        return col

    def both(self):
        return (("clean", self.clean), ("dirty", self.dirty))


def build(gpu, vals=None):
    return Pair(gpu, values() if vals is None else vals)
