"""GPU: dbhip_like / dbhip_str_match (include/dbhip.h a20), every row asserted exactly against tests/like_ref.py (plain Python, held to
sqlite3 and to negative controls by tests/test_like_ref_cpu.py). Nothing is sampled. Columns are packed here, not by Column.strings: the
long values lie back to back in their data buffer without any padding, so a matcher that compares bytes outside a value reads its
neighbours' bytes — which the cases choose so that it then answers wrongly — and the output Bitmap is pre-filled with ones, so that
a word the call does not write, or a bit past n it leaves set, shows."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import like_ref as R

pytestmark = pytest.mark.gpu

LONG = T.LIKE_LONG_BYTES
BS = 0x5C
E2, E3, E4 = R.E2, R.E3, R.E4


# ---- helpers ----------------------------------------------------------------------------------------------------------------------
def pack(gpu, values, valid=None, lead=b"", n_buffers=1, buffer_of=None):
    """a String column whose long values (> 12 bytes) are packed back to back, behind `lead`, in n_buffers data buffers (long row k goes
    to buffer k % n_buffers unless buffer_of(row) says otherwise — it may name a buffer the column does not have); no byte follows the
    last value of a buffer"""
    n = len(values)
    lens = np.array([len(v) for v in values], dtype=np.uint32)
    views = np.zeros((n, 4), dtype=np.uint32)
    views[:, 0] = lens
    if n:
        inl = b"".join(v.ljust(12, b"\0") if len(v) <= 12 else v[:4].ljust(12, b"\0") for v in values)
        views[:, 1:4] = np.frombuffer(inl, dtype=np.uint32).reshape(n, 3)
    parts = [[lead] for _ in range(n_buffers)]
    sizes = [len(lead)] * n_buffers
    k = 0
    for i in np.nonzero(lens > 12)[0]:
        b = k % n_buffers if buffer_of is None else buffer_of(int(i))
        k += 1
        views[i, 2] = b
        if b < n_buffers:
            views[i, 3] = sizes[b]
            parts[b].append(values[i])
            sizes[b] += len(values[i])
        else:
            views[i, 3] = 0
    bufs = [gpu.DeviceBuffer.from_numpy(np.frombuffer(b"".join(p), dtype=np.uint8)) for p in parts]
    for b, size in zip(bufs, sizes):
        assert b.nbytes == size                      # the last value ends where the buffer ends
    ptrs = gpu.DeviceBuffer.from_numpy(np.array([b.ptr for b in bufs], dtype=np.uint64))
    vb = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(valid)) if valid is not None else None
    col = gpu.Column(T.T_STRING, n, gpu.DeviceBuffer.from_numpy(views), vb, buffers=ptrs, keep=tuple(bufs))
    col.n_buffers = n_buffers
    return col


def _bits(gpu, call, n):
    """runs call(out_ptr) on a Bitmap pre-filled with ones, checks that exactly ceil(n / 64) words were written and that the bits past n
    are zero, and returns the n bits"""
    words = (n + 63) // 64
    out = gpu.DeviceBuffer.from_numpy(np.full(words * 8 + 16, 0xFF, dtype=np.uint8))
    T.check(call(C.c_void_p(out.ptr)))
    raw = out.to_numpy(np.uint8)
    assert (raw[words * 8:] == 0xFF).all(), "wrote past ceil(n / 64) words"
    bits = np.unpackbits(raw[:words * 8], bitorder="little")
    assert not bits[n:].any(), "bits past n"
    return bits[:n].astype(bool).tolist()


def _host(b):
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0")


def run_like(gpu, col, pattern, escape=BS, negate=False, unit_byte=False, n=None):
    n = col.n if n is None else n
    cc = col.c()
    flags = (T.LIKE_NEGATE if negate else 0) | (T.LIKE_UNIT_BYTE if unit_byte else 0)
    return _bits(gpu, lambda out: T.lib().dbhip_like(C.byref(cc), _host(pattern), C.c_int32(len(pattern)), C.c_int32(escape), C.c_int32(flags),
                                                     C.c_int64(n), out, None), n)


def run_match(gpu, kind, col, needle, negate=False):
    cc = col.c()
    return _bits(gpu, lambda out: T.lib().dbhip_str_match(C.c_int32(kind), C.byref(cc), _host(needle), C.c_int32(len(needle)),
                                                          C.c_int32(T.LIKE_NEGATE if negate else 0), C.c_int64(col.n), out, None), col.n)


_expected = {}


def expect(values, valid, pattern, escape=BS, negate=False, unit_byte=False, cache=None):
    """the reference's bits; `cache` names a case shared between tests, whose reference is then computed once per (pattern, mode)"""
    if cache is None:
        return R.like_column(values, valid, pattern, escape, negate, unit_byte)
    key = (cache, pattern, escape, unit_byte)
    if key not in _expected:
        _expected[key] = R.like_column(values, valid, pattern, escape, False, unit_byte)
    ok = [True] * len(values) if valid is None else valid
    return [bool(k) and (e != negate) for e, k in zip(_expected[key], ok)]


def assert_rows(got, exp, values, what):
    if got != exp:
        bad = [i for i in range(len(exp)) if got[i] != exp[i]]
        raise AssertionError(f"{what}: {len(bad)} of {len(exp)} rows differ, first row {bad[0]} value {values[bad[0]][:80]!r} (len {len(values[bad[0]])}) "
                             f"got {got[bad[0]]} expected {exp[bad[0]]}")


def check_all(gpu, col, values, valid, patterns, modes=((False, False), (True, False), (False, True), (True, True)), what="", cache=None):
    """every pattern in every (negate, unit_byte) mode; the two answers must both occur somewhere (a test that only ever sees one proves little)"""
    seen = set()
    for pattern, escape in patterns:
        for negate, unit_byte in modes:
            exp = expect(values, valid, pattern, escape, negate, unit_byte, cache)
            got = run_like(gpu, col, pattern, escape, negate, unit_byte)
            assert_rows(got, exp, values, f"{what} pattern {pattern[:40]!r} escape {escape} negate {negate} unit_byte {unit_byte}")
            seen.update(exp)
    assert seen == {False, True}


KIND_PATTERNS = [(b"abab", BS), (b"ab", BS), (b"abab%", BS), (b"a%", BS), (b"%abab", BS), (b"%ababa", BS), (b"%aab%", BS), (b"%bababa%", BS), (b"%a%", BS),
                 (b"a%b", BS), (b"%ab%ba%", BS), (b"a_a%", BS), (b"%b_b", BS), (b"%a_b%", BS), (b"_%_", BS), (b"ab%%ab", BS), (b"%", BS), (b"", BS)]


def ab(rng, ln):
    return bytes(rng.choice(np.frombuffer(b"ab", np.uint8), ln).tolist())


# ---- row counts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099])
def test_row_counts(gpu, n):
    """the ballot words, the last partial word, bits past n zero; every kind"""
    rng = np.random.default_rng(n)
    pool = R.value_pool(7, n_random=60) + [ab(rng, int(k)) for k in rng.integers(13, 80, 40)] + [ab(rng, 300), b"ab" * 200]
    values = [pool[k] for k in rng.integers(0, len(pool), n)]
    col = pack(gpu, values)
    pats = [(b"ab", BS), (b"ab%", BS), (b"%ab", BS), (b"%aab%", BS), (b"%a%b_", BS), (b"%", BS)]
    if n == 0:
        for pattern, escape in pats:
            assert run_like(gpu, col, pattern, escape) == []
        return
    if n == 1:
        values = [b"xxabab"]
        col = pack(gpu, values)
    check_all(gpu, col, values, None, pats, modes=((False, False), (True, True)), what=f"n={n}")


# ---- kind x mode x value lengths ----------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 3, 4, 5, 11, 12, 13, 15, 16, 17, 31, 32, 33, 63, 64, 65, LONG - 1, LONG, LONG + 1]
_length_case = {}


def length_case():
    """per length: random {a, b} values, values with a needle at the start / in the middle / at the end, multi-byte ones; one 70,001-byte
    value among 12-byte ones at the end. The EQUALS patterns are the first value of every length up to 255."""
    if not _length_case:
        rng = np.random.default_rng(11)
        values, equals = [], []
        for ln in LENGTHS:
            first = ab(rng, ln)
            if ln <= 255:
                equals.append((first, BS))
            values += [first, ab(rng, ln), (b"abab" + ab(rng, ln))[:ln], (ab(rng, ln) + b"ababa")[-ln:] if ln else b"", (E2 * ln)[:ln], (b"a" + E3 * ln)[:ln],
                       (E4 * ln)[:max(ln - 1, 0)] + b"b"[:min(ln, 1)]]
            if ln >= 8:
                mid = ln // 2 - 3
                values.append(ab(rng, mid) + b"bababa" + ab(rng, ln - mid - 6))
        big = ab(rng, 70_001 - 6 - 60_000) + b"bababa" + b"a" * 60_000
        values += [b"abababababab", big, b"bababababa" + b"ab", big[:-1] + E2, b"a" * 12]
        _length_case.update(values=values, equals=equals)
    return _length_case["values"], _length_case["equals"]


@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("unit_byte", [False, True])
def test_kinds_modes_and_value_lengths(gpu, negate, unit_byte):
    """the inline / long switch (12 / 13), the prefix word, the word refills, the hand-over between the passes (LIKE_LONG_BYTES - 1, the
    threshold, + 1) and more than one stride of pass 2 (70,001 bytes)"""
    values, equals = length_case()
    assert len(values[-4]) == 70_001
    col = pack(gpu, values, lead=b"ab")
    check_all(gpu, col, values, None, KIND_PATTERNS + equals + [(b"%bababa" + b"a" * 200 + b"%", BS)], modes=((negate, unit_byte),), what="lengths", cache="lengths")


# ---- needle placements ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", range(17))
def test_needle_across_word_boundaries(gpu, offset):
    """the first long value starts `offset` bytes into its buffer, the next ones wherever the packing puts them: a 5-byte and a 9-byte
    needle at every position of values of 13 .. 40 bytes cross every 4- and 16-byte boundary of the buffer"""
    values = []
    for ln in (13, 14, 15, 16, 17, 21, 29, 40):
        for at in range(0, ln - 4):
            values.append(b"b" * at + b"abbba" + b"b" * (ln - at - 5))
        for at in range(0, ln - 8, 3):
            values.append(b"b" * at + b"abbbbabba" + b"b" * (ln - at - 9))
    col = pack(gpu, values, lead=b"abbbbabbabbbaabbbbabba"[:offset])
    pats = [(b"%abbba%", BS), (b"abbba%", BS), (b"%abbba", BS), (b"%abbbbabba%", BS), (b"abbbbabba%", BS), (b"%abbbbabba", BS), (b"%a_bba%", BS), (b"%a%a", BS),
            (b"b" * 8 + b"abbba", BS)]
    check_all(gpu, col, values, None, pats, modes=((False, False),), what=f"offset {offset}")


def test_needle_across_the_stride_of_pass_2(gpu):
    """values longer than LIKE_LONG_BYTES with the needle starting at positions 62, 63 and 64 — of the value, and of the search for a
    second segment that starts behind the first one's end"""
    values = []
    for ln in (LONG + 1, LONG + 44, 1000):
        for at in (0, 1, 61, 62, 63, 64, 65, 126, 127, 128, 129, ln - 6, ln - 5):
            values.append(b"b" * at + b"abbba" + b"b" * (ln - at - 5))
            values.append(b"abbba" + b"b" * at + b"abbba" + b"b" * (ln - at - 10))
            values.append(b"ca" + b"b" * at + E3 + b"ab" + b"b" * (ln - at - 7))
    values += [b"b" * 1000, b"abbb" * 100, b"b" * 300 + b"abbb"]
    col = pack(gpu, values, lead=b"abb")
    pats = [(b"%abbba%", BS), (b"%abbba%abbba%", BS), (b"abbba%abbba%", BS), (b"%abbba%abbba", BS), (b"ca%_ab%", BS), (b"%a_ab%", BS), (b"%abbba", BS), (b"abbba%", BS),
            (b"%abbba%b", BS), (b"c%abbba%", BS)]
    check_all(gpu, col, values, None, pats, what="stride")


def test_overlapping_occurrences(gpu):
    long_tail = b"x" * 300
    values = [b"aaab", b"aab", b"aaaab", b"abc", b"abbc", b"abcbc", b"ababc", b"aaab" * 4, b"a" * 15 + b"b", b"abc" + b"x" * 20, b"x" * 20 + b"abc",
              b"aaab" + long_tail, long_tail + b"aaab", b"abc" + long_tail, long_tail + b"abc" + long_tail, long_tail + b"abbc"]
    col = pack(gpu, values)
    got = run_like(gpu, col, b"%aab%")
    assert got[0] and got[1], "`aab` in `aaab` occurs only as an overlap of two partial occurrences"
    got = run_like(gpu, col, b"%ab%bc%")
    assert not got[3] and got[4], "%ab%bc% on abc must be false: the two segments' only matches overlap"
    check_all(gpu, col, values, None, [(b"%aab%", BS), (b"%ab%bc%", BS), (b"%aab", BS), (b"ab%bc", BS), (b"%ab%bc", BS), (b"ab%bc%", BS), (b"%abc%bc%", BS)],
              what="overlap")


# ---- neighbours in the buffer ---------------------------------------------------------------------------------------------------------
def test_neighbours_in_the_buffer(gpu):
    """values packed back to back: a value ends with the needle's first bytes and the NEXT one begins with the rest; the needle's tail
    lies just BEFORE a value's first byte (the lead); the last value lies flush against the end of its DeviceBuffer. None of these rows
    holds the needle."""
    needle = b"abbbabba"
    values = []
    for cut in range(1, len(needle)):
        for ln in (13, 16, 19, 33, LONG + 3):
            values.append(b"c" * (ln - cut) + needle[:cut])            # ends with the needle's head ...
            values.append(needle[cut:] + b"c" * (ln - len(needle) + cut))   # ... and the next one begins with the rest
    values.append(b"c" * 13 + needle[:5])                               # the last value: flush against the end of the buffer
    col = pack(gpu, values, lead=needle[:7])
    for pattern in (b"%" + needle + b"%", needle + b"%", b"%" + needle, b"%" + needle[:4] + b"%" + needle[4:] + b"%", b"%abbb_bba%"):
        for negate in (False, True):
            assert run_like(gpu, col, pattern, negate=negate) == [negate] * len(values), pattern
    # the same rows with rows that do hold it, so that both answers occur
    values2 = values + [b"c" * 9 + needle, needle + b"c" * 9, b"c" * 300 + needle, b"cc" + needle + b"c" * 300]
    col2 = pack(gpu, values2, lead=needle[1:])
    check_all(gpu, col2, values2, None, [(b"%" + needle + b"%", BS), (needle + b"%", BS), (b"%" + needle, BS), (b"%abbb_bba%", BS), (b"%" + needle[:3], BS)],
              what="neighbours")


# ---- nullable columns -----------------------------------------------------------------------------------------------------------------
def test_nullable_column_with_a_validity_offset(gpu):
    rng = np.random.default_rng(5)
    pool = R.value_pool(9, n_random=80) + [ab(rng, 20), ab(rng, 300), b"ab" * 150]
    n_all = 13 + 700 + 40
    values = [pool[k] for k in rng.integers(0, len(pool), n_all)]
    valid = rng.random(n_all) < 0.7
    whole = pack(gpu, values, valid=valid)
    col = whole.slice(13, 713)
    assert col.voff == 13
    v, ok = values[13:713], valid[13:713]
    check_all(gpu, col, v, ok, [(b"%ab%", BS), (b"ab%", BS), (b"%a", BS), (b"%a%b%", BS), (b"a_%", BS), (b"%", BS)], what="nullable")
    for negate in (False, True):
        got = run_like(gpu, col, b"%ab%", negate=negate)
        assert not any(g for g, k in zip(got, ok) if not k), "a NULL row's bit is 0, also under NEGATE"
        res = gpu.like(col, b"%ab%", negate=negate)
        assert res.dtype == T.T_BOOL and res.validity is col.validity and res.voff == 13 and res.n == 700
        assert res.to_numpy().tolist() == got and res.validity_numpy().tolist() == ok.tolist()
    # NULL rows are not dereferenced: their views may hold anything
    raw = whole.data.to_numpy(np.uint32).reshape(-1, 4).copy()
    raw[~valid] = [5000, 0x61616161, 77, 0xFFFFFF00]
    broken = gpu.Column(T.T_STRING, n_all, gpu.DeviceBuffer.from_numpy(raw), whole.validity, buffers=whole.buffers, keep=(whole,))
    assert run_like(gpu, broken, b"%ab%") == expect(values, valid, b"%ab%")


# ---- special columns ------------------------------------------------------------------------------------------------------------------
def test_scalar_column(gpu):
    for value in (b"", b"abab", b"xxababxx" * 3, b"x" * 300 + b"abab" + b"y" * 77):
        col = pack(gpu, [value])
        col.is_scalar = True
        for n in (1, 64, 130):
            for pattern, escape in [(b"%abab%", BS), (b"abab", BS), (b"%b", BS), (b"x%", BS), (b"%b_b%", BS), (b"", BS), (b"%", BS)]:
                for negate in (False, True):
                    exp = R.like(value, pattern, escape) != negate
                    assert run_like(gpu, col, pattern, escape, negate, n=n) == [exp] * n, (value[:20], pattern, n, negate)
    null = pack(gpu, [b"abab"], valid=np.array([False]))
    null.is_scalar = True
    assert run_like(gpu, null, b"abab", n=70) == [False] * 70 and run_like(gpu, null, b"abab", negate=True, n=70) == [False] * 70
    res = gpu.like(col, b"%abab%", n=130)
    assert res.n == 130 and all(res.to_numpy().tolist())


def test_view_with_a_buffer_index_out_of_range(gpu):
    rng = np.random.default_rng(6)
    values = [ab(rng, int(k)) for k in rng.integers(0, 60, 300)] + [ab(rng, 300) + b"abab", b"abab" * 100]
    bad = {i for i in range(len(values)) if len(values[i]) > 12 and i % 5 == 0}
    assert bad
    col = pack(gpu, values, buffer_of=lambda i: 7 if i in bad else 0)
    valid = np.array([i not in bad for i in range(len(values))])
    # its bit is 0 (also under NEGATE) and the other rows are unaffected: as if the row were NULL
    check_all(gpu, col, values, valid, [(b"%abab%", BS), (b"a%", BS), (b"%b", BS), (b"%a_a%", BS), (b"%", BS)], what="bad buffer index")
    nobuf = gpu.Column(T.T_STRING, col.n, col.data, keep=(col,))      # no buffer table at all: every long view is out of range
    valid = np.array([len(v) <= 12 for v in values])
    check_all(gpu, nobuf, values, valid, [(b"%ab%", BS), (b"a%", BS)], what="no buffers")


def test_column_with_two_buffers(gpu):
    rng = np.random.default_rng(8)
    values = [ab(rng, int(k)) for k in rng.integers(0, 90, 500)] + [ab(rng, 400), ab(rng, 257), b"ab" * 130]
    col = pack(gpu, values, n_buffers=2, lead=b"ba")
    check_all(gpu, col, values, None, [(b"%abab%", BS), (b"ab%", BS), (b"%ab", BS), (b"%ab%ba_", BS)], what="two buffers")


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def test_composition_with_filter_take_bitmap_and_groupby(gpu):
    rng = np.random.default_rng(9)
    words = [b"green", b"forest", b"special", b"requests", b"blue", b"packages", b"deposits", b"PROMO", b"BRASS", b"x"]
    n = 3000
    values = [b" ".join(words[k] for k in rng.integers(0, len(words), int(rng.integers(1, 7)))) for _ in range(n)]
    valid = rng.random(n) < 0.9
    col = pack(gpu, values, valid=valid)
    exp = expect(values, valid, b"%special%requests%")
    pred = gpu.like(col, b"%special%requests%")
    assert pred.to_numpy().tolist() == exp
    # like -> filter_select -> take
    sel, k = gpu.filter_select(pred)
    rows = [i for i in range(n) if exp[i]]
    assert k == len(rows) and 0 < k < n
    assert sel.to_numpy(np.uint32, k).tolist() == rows
    assert gpu.take(col, sel, k).string_values() == [values[i] for i in rows]
    # like AND a numeric cmp through bitmap_binary
    x = rng.integers(0, 100, n).astype(np.int64)
    cx = gpu.Column.from_numpy(x)
    lt = gpu.cmp(T.CMP_LT, cx, gpu.Column.scalar(50, T.T_I64))
    both = gpu.DeviceBuffer(((n + 63) // 64) * 8)
    T.check(T.lib().dbhip_bitmap_binary(0, C.c_void_p(pred.data.ptr), C.c_void_p(lt.data.ptr), C.c_int64(n), C.c_void_p(both.ptr), None))
    and_exp = [bool(e and xi < 50) for e, xi in zip(exp, x)]
    assert gpu.unpack_bits(both.to_numpy(np.uint8), n).tolist() == and_exp and any(and_exp)
    # the Bitmap as the pushed-down filter of an aggregation (NOT LIKE: the NULL rows' bits are 0 by themselves)
    nexp = np.array(expect(values, valid, b"%special%requests%", negate=True))
    npred = gpu.like(col, b"%special%requests%", negate=True)
    key = rng.integers(0, 7, n).astype(np.int64)
    g = gpu.GroupBy([T.T_I64], [(T.AGG_SUM, T.T_I64, 0, 0, 0), (T.AGG_COUNT, 0, 0, 0, 0)])
    g.add_block([gpu.Column.from_numpy(key)], [cx, None], n, filter=gpu.Column(T.T_BOOL, n, npred.data, keep=(npred,)))
    want = sorted((int(kk), int(x[nexp & (key == kk)].sum()), int((nexp & (key == kk)).sum())) for kk in np.unique(key[nexp]))
    assert sorted(g.result()) == want


# ---- literal needles --------------------------------------------------------------------------------------------------------------------
def test_literal_needles(gpu):
    """dbhip_str_match against Python's startswith / endswith / in / ==; `%`, `_` and `\\` inside the needle are taken literally"""
    rng = np.random.default_rng(10)
    values = R.value_pool(12, n_random=200) + R.long_values(13) + [ab(rng, int(k)) for k in rng.integers(13, 70, 60)]
    valid = rng.random(len(values)) < 0.9
    col = pack(gpu, values, valid=valid, lead=b"a")
    needles = [b"", b"a", b"ab", b"%", b"_", b"a%", b"a_b", b"\\", b"abab", b"ababa", b"a" * 12, b"a" * 13, E2, b"\xa9", b"\x00", R.P255_CONTAINS[1:-1], b"ab" * 100]
    seen = set()
    for needle in needles:
        for kind in (T.LIKE_EQUALS, T.LIKE_PREFIX, T.LIKE_SUFFIX, T.LIKE_CONTAINS):
            for negate in (False, True):
                exp = [bool(ok) and (R.str_match(kind, v, needle) != negate) for v, ok in zip(values, valid)]
                assert_rows(run_match(gpu, kind, col, needle, negate), exp, values, f"needle {needle[:20]!r} kind {kind} negate {negate}")
                seen.update(exp)
    assert seen == {False, True}
    res = gpu.str_match(T.LIKE_CONTAINS, col, b"a%")
    assert res.validity is col.validity and res.to_numpy().tolist() == [bool(ok) and b"a%" in v for v, ok in zip(values, valid)]
    assert gpu.like_kind(b"a\\%b") == T.LIKE_EQUALS and gpu.like_kind(b"%a%", escape=None) == T.LIKE_CONTAINS


def test_the_pattern_pool(gpu):
    """every pattern of like_ref.PATTERNS (escapes, a trailing lone escape, other escape bytes, the 255-byte and the 16-segment patterns)
    over the value pool, in the four modes"""
    values = R.value_pool(14, n_random=300) + R.long_values(15)
    col = pack(gpu, values, lead=b"ab")
    check_all(gpu, col, values, None, R.PATTERNS, what="pool")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_usable(gpu):
    values = [b"abab", b"x" * 20 + b"abab", b"", b"ab"]
    col = pack(gpu, values)
    cc = col.c()
    out = gpu.DeviceBuffer(64)
    L = T.lib()

    def like_rc(c, pattern, escape=BS, flags=0, n=4, length=None):
        return L.dbhip_like(C.byref(c), _host(pattern), C.c_int32(len(pattern) if length is None else length), C.c_int32(escape), C.c_int32(flags), C.c_int64(n),
                            C.c_void_p(out.ptr), None)

    def good():
        assert run_like(gpu, col, b"%abab") == [True, True, False, False]

    ints = gpu.Column.from_numpy(np.arange(4, dtype=np.int64)).c()
    cases = [
        (lambda: like_rc(cc, b"x" * 256), T.ERR_UNSUPPORTED), (lambda: like_rc(cc, b"%".join([b"a"] * 17)), T.ERR_UNSUPPORTED),
        (lambda: like_rc(cc, b"a", length=-1), T.ERR_INVALID), (lambda: like_rc(cc, b"a", escape=256), T.ERR_INVALID),
        (lambda: like_rc(cc, b"a", escape=-2), T.ERR_INVALID), (lambda: like_rc(ints, b"a"), T.ERR_INVALID), (lambda: like_rc(cc, b"a", flags=4), T.ERR_INVALID),
        (lambda: like_rc(cc, b"a", n=-1), T.ERR_INVALID),
        (lambda: L.dbhip_str_match(C.c_int32(T.LIKE_SEGMENTS), C.byref(cc), _host(b"a"), C.c_int32(1), C.c_int32(0), C.c_int64(4), C.c_void_p(out.ptr), None), T.ERR_INVALID),
        (lambda: L.dbhip_str_match(C.c_int32(T.LIKE_PREFIX), C.byref(cc), _host(b"a" * 256), C.c_int32(256), C.c_int32(0), C.c_int64(4), C.c_void_p(out.ptr), None),
         T.ERR_UNSUPPORTED),
        (lambda: L.dbhip_str_match(C.c_int32(T.LIKE_PREFIX), C.byref(ints), _host(b"a"), C.c_int32(1), C.c_int32(0), C.c_int64(4), C.c_void_p(out.ptr), None), T.ERR_INVALID),
    ]
    for call, code in cases:
        assert call() == code
        assert b"DBHIP_LIKE" not in L.dbhip_last_error()
        good()
    with pytest.raises(T.DbhipError) as e:
        gpu.like(col, b"x" * 256)
    assert e.value.code == T.ERR_UNSUPPORTED
    with pytest.raises(T.DbhipError):
        gpu.like_kind(b"x" * 256)
    assert like_rc(cc, b"a", n=0) == T.OK
    good()


# ---- 200,000 rows per kind ------------------------------------------------------------------------------------------------------------------
_big = {}


def big_case(gpu):
    """200,000 rows drawn from 4,000 distinct values of mixed lengths (the reference is evaluated once per distinct value); about one row
    in 2,000 is longer than LIKE_LONG_BYTES. Every row has its own bytes in the buffer, at whatever alignment the packing gives it."""
    if not _big:
        rng = np.random.default_rng(16)
        words = [b"green", b"forest", b"special", b"requests", b"PROMO", b"BRASS", b"MEDIUM POLISHED", b"Customer", b"Complaints", b"ab", b"a", E2, E3, b" "]
        short = [b"".join(words[k] for k in rng.integers(0, len(words), int(rng.integers(0, 9)))) for _ in range(3960)]
        longs = [b"".join(words[k] for k in rng.integers(0, len(words), int(rng.integers(60, 400)))) for _ in range(40)]
        assert all(len(v) > LONG for v in longs)
        n = 200_000
        pick = rng.integers(0, len(short), n)
        is_long = rng.random(n) < 1 / 2000
        values = [longs[int(k) % 40] if lg else short[int(k)] for k, lg in zip(pick, is_long)]
        valid = rng.random(n) < 0.95
        _big.update(values=values, valid=valid, col=pack(gpu, values, valid=valid), n_long=int(is_long.sum()))
    return _big


@pytest.mark.parametrize("pattern", [b"green", b"PROMO%", b"%BRASS", b"%green%", b"%special%requests%", b"%Customer%Complaints_"])
def test_200000_rows(gpu, pattern):
    case = big_case(gpu)
    assert 50 < case["n_long"] < 200
    exp = expect(case["values"], case["valid"], pattern, cache="big")
    assert 0 < sum(exp) < len(exp)
    assert_rows(run_like(gpu, case["col"], pattern), exp, case["values"], f"pattern {pattern!r}")
    nexp = expect(case["values"], case["valid"], pattern, negate=True, cache="big")
    assert_rows(run_like(gpu, case["col"], pattern, negate=True), nexp, case["values"], f"NOT pattern {pattern!r}")


# ---- the bytes past an inline value, and long values in a second buffer (tests/strview_cases.py) --------------------------------------
def test_like_ignores_the_bytes_past_an_inline_value(gpu):
    """the shared String column with clean and with 0xFF padding against a PREFIX and a SEGMENTS pattern (and one that asks for the
    padding byte itself): the reference's bits both times"""
    from tests import strview_cases as S
    p = S.build(gpu)
    for pattern in (b"ab%", b"%a%b%a", b"%\xff", b"a\xff%"):
        exp = expect(p.vals, None, pattern)
        assert True in exp and False in exp, pattern
        for name, col in p.both():
            assert_rows(run_like(gpu, col, pattern), exp, p.vals, f"{name} {pattern!r}")
    assert R.kind_of(b"ab%", BS) == R.PREFIX and R.kind_of(b"%a%b%a", BS) == R.SEGMENTS
