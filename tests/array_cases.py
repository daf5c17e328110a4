"""The one case list of the Array functions (include/dbhip.h a29): tests/test_array_host_cpu.py runs it through csrc/dev_array.h on the
host, tests/test_gpu_array.py through the kernels, both against tests/array_ref.py. A column is a list of rows, a row a list of
elements (None = a NULL element). The shapes are the smallest that reach every branch of k_array.hip: the row lengths around the wave
(63, 64, 65) and around the tier threshold T, one row that takes the wave pass several steps and a ragged tail, 64-row groups whose
element range is one below, at and one above the LDS stage, empty rows in front, behind and everywhere."""
import numpy as np

from tests import array_ref as R
from tests import float_ref as F

T = 32                  # DBHIP_ARRAY_LONG_LEN: a longer row goes to the wave-per-row pass
STEP = 64               # elements per step of that pass
STAGE_BYTES = 8192      # the LDS stage of a wave of the short-row pass
LONG_ROW = 5 * STEP + 3

# name -> (dbhip type code, numpy dtype of the stored value (None: 16-byte values), element bytes)
TYPES = {"i8": (2, np.int8, 1), "i16": (3, np.int16, 2), "i32": (4, np.int32, 4), "i64": (5, np.int64, 8), "u8": (6, np.uint8, 1), "u16": (7, np.uint16, 2),
         "u32": (8, np.uint32, 4), "u64": (9, np.uint64, 8), "f32": (10, np.float32, 4), "f64": (11, np.float64, 8), "date": (12, np.int32, 4),
         "timestamp": (13, np.int64, 8), "dec64": (14, np.int64, 8), "dec128": (15, None, 16), "string": (16, None, 16)}
NUMBERS = [t for t in TYPES if t != "string"]
EDGE_LENGTHS = [0, 0, 1, 63, 64, 65, T - 1, T, T + 1, LONG_ROW, 0, 5, 2, 0]     # leading and trailing empty rows
N_ROWS = [1, 63, 64, 65, 1027]

STRINGS = [b"", b"a", b"abc", b"abcd", b"abcde", b"abcdefghijkl", b"abcdefghijklm", b"abcdefghijklmn", b"abcdefghijklmno", b"abcdXfghijklm",
           b"abcdefghijklmnopqrstuvwxyz0123456789-+" * 2, bytes(range(1, 256)), bytes(range(1, 255)) + b"\x01", b"\xe2\x82\xac" * 5]
STR_NEEDLES = [b"", b"a", b"abcd", b"abcdefghijkl", b"abcdefghijklm", bytes(range(1, 256))]      # 0, 1, 4, 12, 13 and 255 bytes


def int_pool(tname):
    if tname == "dec64":
        lo, hi = -(10 ** 18 - 1), 10 ** 18 - 1
    elif tname == "dec128":
        lo, hi = -R.DEC128_MAX, R.DEC128_MAX
    else:
        info = np.iinfo(TYPES[tname][1])
        lo, hi = int(info.min), int(info.max)
    return [lo, hi, 0, 1, hi // 3, lo // 5 if lo else 7, hi - 1]


def values(tname, rng, count, for_sum=False):
    """count elements of the type: integers from a pool of seven (the type's ends among them, so sums wrap and needles repeat), floats
    from float_ref's pool (for_sum: its SUM pool and real-valued draws within MAX_SUM_ABS), Strings from STRINGS"""
    if tname == "string":
        return [STRINGS[k] for k in rng.integers(0, len(STRINGS), count)]
    if tname in ("f32", "f64"):
        dt = TYPES[tname][1]
        if for_sum:
            return list(F.mixed(rng, count, dt, for_sum=True, p_pool=0.05)) if count else []
        p = F.pool(dt)
        return [p[k] for k in rng.integers(0, len(p), count)]
    p = int_pool(tname)
    return [p[k] for k in rng.integers(0, len(p), count)]


def column(tname, lengths, seed, null_rate=0.2, for_sum=False):
    """rows of the given lengths; every seventh row with a value is a run of NULLs"""
    rng = np.random.default_rng(seed)
    rows = []
    for r, ln in enumerate(lengths):
        vals = values(tname, rng, ln, for_sum)
        nulls = rng.random(ln) < null_rate
        rows.append([None if (nulls[k] or r % 7 == 3) else vals[k] for k in range(ln)])
    return rows


def stage_lengths(es, delta):
    """64 rows (one wave of the short-row pass) whose elements are STAGE_BYTES / es + delta in all: 63 rows of at most T elements, and the
    33rd takes the rest (with small elements that is a row for the wave pass, which the short rows' range then spans)"""
    total = STAGE_BYTES // es + delta
    base = min(T, total // 64)
    out = [base] * 64
    out[32] = total - 63 * base
    assert sum(out) == total and max(out[:32] + out[33:]) <= T
    return out


def small_lengths(n, seed):
    """n rows of 0 .. 8 elements, every 97th one just past the tier threshold"""
    rng = np.random.default_rng(seed)
    out = [int(x) for x in rng.integers(0, 9, n)]
    for r in range(50, n, 97):
        out[r] = T + 1
    return out


def columns(tname, for_sum=False, full=True):
    """(name, rows) of every shape for the type; full = False: the edge lengths only (the types that share their kernels with another)"""
    es = TYPES[tname][2]
    out = [("edges", column(tname, EDGE_LENGTHS, 11, for_sum=for_sum))]
    if not full:
        return out
    out += [("n%d" % n, column(tname, small_lengths(n, n), 100 + n, for_sum=for_sum)) for n in N_ROWS]
    out += [("stage%+d" % d, column(tname, [0] * 64 + stage_lengths(es, d) + [3], 200 + d, for_sum=for_sum)) for d in (-1, 0, 1)]
    out.append(("all_empty", column(tname, [0] * 70, 1)))
    out.append(("no_nulls", column(tname, EDGE_LENGTHS, 12, null_rate=0.0, for_sum=for_sum)))
    return out


def offsets_of(rows, first=0):
    off = [first]
    for row in rows:
        off.append(off[-1] + len(row))
    return off


def flat(rows):
    return [e for row in rows for e in row]


def needles(tname, rows, seed):
    """one needle per row: an element of the row (every third row its LAST non-NULL one, so the first match is usually an earlier duplicate),
    a value of the pool that may be absent, or NULL (every fifth row)"""
    rng = np.random.default_rng(seed)
    out = []
    for r, row in enumerate(rows):
        have = [e for e in row if e is not None]
        if r % 5 == 4:
            out.append(None)
        elif have and r % 3 == 0:
            out.append(have[-1])
        elif have and r % 3 == 1:
            out.append(have[int(rng.integers(0, len(have)))])
        else:
            out.append(values(tname, rng, 1)[0])
    return out


GET_INDEXES = [0, 1, -1, 2, -2, R.INT64_MIN, R.INT64_MAX]


def get_indexes(rows):
    """per row: the indexes every row is asked for: 0, +-1, +-len, +-(len + 1), INT64_MIN, INT64_MAX"""
    return [sorted(set(GET_INDEXES + [len(row), -len(row), len(row) + 1, -len(row) - 1])) for row in rows]


def indexof_lane_rows():
    """INDEXOF in the wave pass: the first match in lane 63 of the first step, and in lane 0 of the second, each with a later duplicate"""
    a = list(range(1000, 1000 + LONG_ROW))
    b = list(a)
    a[63], a[200] = 7, 7
    b[64], b[300] = 7, 7
    c = list(range(1000, 1000 + LONG_ROW))
    c[LONG_ROW - 1] = 7                                       # in the ragged tail
    return [a, b, c, list(range(1000, 1000 + LONG_ROW))], 7, [64, 65, LONG_ROW, 0]


def dec128_overflow_rows():
    """the checked sum: rows whose exact sum leaves the decimal range (one of them far past 2^127) beside rows whose parts do and whose
    sum does not"""
    m = R.DEC128_MAX
    return [[m, 1], [m, -1, 1], [m] * 300, [m, m, -m, -m, 5], [-m, -1], [-m] * (T + 7), [m, None, -m], [3, 4]]


# ---- the stored bytes of an element (little endian), for the host checker and for raw device buffers ---------------------------------------
def is_float(tname):
    return tname in ("f32", "f64")


def is_signed(tname):
    return tname in ("i8", "i16", "i32", "i64", "date", "timestamp", "dec64", "dec128")


def encode(tname, v):
    """the es bytes of one element (None: the zero value)"""
    code, dt, es = TYPES[tname]
    if v is None:
        return bytes(es)
    if is_float(tname):
        return np.array([v], dtype=dt).tobytes()
    return int(v).to_bytes(es, "little", signed=is_signed(tname))


def decode(tname, b):
    code, dt, es = TYPES[tname]
    if is_float(tname):
        return np.frombuffer(bytes(b), dtype=dt)[0]
    return int.from_bytes(bytes(b), "little", signed=is_signed(tname))


def result_type(kind, tname):
    """the type name of a reduction's result (what dbhip_groupby_result_type gives): COUNT u64; SUM i64 / u64 / f64 / the decimal; MIN /
    MAX the elements' type. None: not offered."""
    if kind == R.COUNT:
        return "u64"
    if kind == R.SUM:
        cls = R.SUM_CLASS[tname]
        return {None: None, "i64": "dec64" if tname == "dec64" else "i64", "u64": "u64", "f": "f64", "dec128": "dec128"}[cls]
    return tname
