"""GPU: the hash join (k_join.hip) and the join on serialized keys (k_serialize.hip) at the edges of their kernels — probe blocks on both
sides of a tile, exact multiplicities around the saturated u8 count, keys one bit apart in every word, validity bytes read by nibbles,
build sides that grow from nothing, the occupancy filter for 16- and 32-byte keys, probe blocks long enough for the second step of
the pipelined count loop and for G = 2 / G = 4 in the emit pass of a selective join, serialized keys around the 8-byte step of their
hash — and the protocol of the C ABI around them (probe without count, capacity, the prepared state, sentinels past every output).
Every result is asserted exactly, whole arrays, against tests/join_ref.py (plain Python / numpy, never another device path) on the
case tables of tests/join_cases.py; tests/test_join_ref_cpu.py checks that reference and shows that the tables reject ten wrong joins."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import join_cases as J
from tests import join_ref as R

pytestmark = pytest.mark.gpu

SENT = 0xA5
SENT32 = 0xA5A5A5A5
ONES = 0xFFFFFFFFFFFFFFFF


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def packed(gpu, keys, valid, kb):
    """(n, KW) u64 keys + bool validity -> the key column HashJoin takes (PackedKeys: data, validity Bitmap at bit 0, n)"""
    data = gpu.DeviceBuffer.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64))
    vb = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(valid)) if valid is not None else None
    return gpu.PackedKeys(data, vb, len(keys), kb)


def build_table(gpu, d):
    j = gpu.HashJoin(d.expected_build_rows, key_bytes=d.key_bytes)
    for keys, valid in d.build_blocks:
        j.add_block(packed(gpu, keys, valid, d.key_bytes))
    j.final_build()
    return j


def filled(gpu, nbytes, byte=SENT):
    buf = gpu.DeviceBuffer(nbytes)
    T.check(T.lib().dbhip_memset(C.c_void_p(buf.ptr), byte, C.c_size_t(nbytes), None))
    return buf


def side(cols, rows):
    """the payload column of one side of an assembled join as i64 row numbers, -1 where it is NULL or the side is not returned"""
    if not cols:
        return np.full(rows, -1, dtype=np.int64)
    assert cols[0].n == rows
    out = cols[0].to_numpy().astype(np.int64)
    out[~cols[0].validity_numpy()] = -1
    return out


def assemble(gpu, j, d, kind, probe):
    pay_p, pay_b = gpu.Column.from_numpy(np.arange(d.n, dtype=np.uint32)), gpu.Column.from_numpy(np.arange(d.nb, dtype=np.uint32))
    pc, bc, rows = j.join(kind, probe, [pay_p], [pay_b])
    op, ob = [side(pc, rows)], [side(bc, rows)]
    if kind in ("right", "right_semi", "right_anti", "full"):
        pc, bc, rows = j.final_probe(kind, [pay_b], [pay_p])
        op.append(side(pc, rows))
        ob.append(side(bc, rows))
    return np.concatenate(op), np.concatenate(ob)


def check_case(gpu, case, assemblies=False):
    d = case.data()
    args = d.ref_args()
    exp_p, exp_b = R.inner_pairs(*args)
    j = build_table(gpu, d)
    probe = packed(gpu, d.probe_keys, d.probe_valid, d.key_bytes)
    got_p, got_b = j.probe_block(probe)
    assert len(got_p) == len(exp_p), (case, len(got_p), len(exp_p))
    assert np.array_equal(got_p, exp_p), (case, "probe_idx")
    assert np.array_equal(got_b, exp_b), (case, "build_row")
    exp_mark = np.zeros(d.n, dtype=bool)
    exp_mark[exp_p] = True
    assert np.array_equal(j.probe_mark(probe), exp_mark), (case, "probe_mark")
    if assemblies:
        for kind in ("left_anti", "full"):
            ep, eb = R.join_rows(kind, *args)
            gp, gb = assemble(gpu, j, d, kind, probe)
            assert np.array_equal(gp, ep) and np.array_equal(gb, eb), (case, kind)
    j.destroy()
    return len(exp_p)


# ---- the case tables through HashJoin ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", J.KEY_BYTES)
@pytest.mark.parametrize("n", J.SIZES)
def test_sizes(gpu, n, kb):
    """probe blocks of 1 .. 1 025 rows, with and without a validity: below a lane's four rows, one full tile with and without a tail,
    four tiles; a third of the probe keys differ from a build key in the last word only"""
    cases = [c for c in J.sizes_cases() if c.key_bytes == kb and c.data().n == n]
    assert len(cases) == 2
    for c in cases:
        assert check_case(gpu, c, assemblies=(n == 513)) > 0


@pytest.mark.parametrize("case", J.multiplicity_cases(), ids=repr)
def test_multiplicity(gpu, case):
    """1, 2, 3, 254, 255, 256, 257, 511 and 1 000 build rows per key, from three build blocks, probed in a full and in the ragged tile:
    the u8 count on both sides of its saturation, the recount, and a probe row's build rows ascending"""
    assert check_case(gpu, case, assemblies=(case.key_bytes == 16)) == 2 * sum(J.MULTIPLICITIES)


@pytest.mark.parametrize("case", J.single_bit_cases(), ids=repr)
def test_single_bit(gpu, case):
    """keys one bit (0, 31, 32, 63) apart in every word, each once in the build side and once not; word 0 at 0, 1, 63, 64, 65, 2^32, 2^63,
    2^64 - 1; runs k, k + 64, k + 128; a table of the minimum 1 024 buckets"""
    check_case(gpu, case, assemblies=(case.key_bytes == 32))


@pytest.mark.parametrize("kb", J.KEY_BYTES)
@pytest.mark.parametrize("pattern", J.PATTERNS)
def test_validity(gpu, pattern, kb):
    """validity Bitmaps of all ones, all zeros, 0x55, 0xAA, 0x0F, 0xF0, the first row only, the last row only — on the probe side
    (1 061 rows: a lane reads one nibble) and on the build side; NULL rows carry keys that match"""
    for s in ("probe", "build"):
        pairs = check_case(gpu, J.by_name(f"validity_{s}_{pattern}_kb{kb}"), assemblies=(pattern == "0x0F" and kb == 8))
        assert (pairs == 0) == (pattern == "zeros")


@pytest.mark.parametrize("case", J.growth_cases(), ids=repr)
def test_growth(gpu, case):
    """tables created for 0 or 1 rows that take blocks of 1, 1 023, 1, 1 024, 0, 3 000 and 70 000 rows; a table finalized without a row;
    a table whose every build row is NULL"""
    check_case(gpu, case, assemblies=(case.name in ("growth_kb16_expected1", "growth_all_null_kb8")))


@pytest.mark.parametrize("case", J.occupancy_cases(), ids=repr)
def test_occupancy(gpu, case):
    """270 000 build rows = 2^20 buckets: the occupancy filter in front of the bucket heads, for 16- and 32-byte keys (the <2, *, true> and
    <4, *, true> count kernels); half the probe keys differ from a build key in the last word only"""
    assert check_case(gpu, case, assemblies=(case.name == "occupancy_kb16_nullable")) > 50_000


@pytest.mark.parametrize("case", J.long_cases(), ids=repr)
def test_long_blocks(gpu, case):
    """4 195 333 probe rows (a wave of the count pass takes a second step: its prefetched keys and validity byte are used) for every key
    width, 8 388 869 and 16 777 477 rows (G = 2 and G = 4 in the emit pass) for 8-byte keys; the matches sit in 1 % of the tiles, with 2,
    3, 255 and 300 build rows among them. Thresholds: tests/join_cases.py count_steps / emit_group."""
    n = int(case.name.split("_")[1][1:])
    assert J.count_steps(n) >= 2 and J.emit_group(n) == {J.LONG_COUNT_N: 1, J.LONG_G2_N: 2, J.LONG_G4_N: 4}[n]
    assert check_case(gpu, case, assemblies=(case.key_bytes == 8 and n == J.LONG_COUNT_N)) > 10_000


# ---- the C ABI of the fixed-key join ----------------------------------------------------------------------------------------------------
class Block:
    """a probe block in HBM with its reference pairs against table data d"""

    def __init__(self, gpu, d, keys, valid):
        self.keys, self.valid, self.n = keys, valid, len(keys)
        self.col = packed(gpu, keys, valid, d.key_bytes)
        self.pairs = R.inner_pairs(d.build_keys(), d.build_valid(), keys, valid)
        self.total = len(self.pairs[0])

    @property
    def kptr(self):
        return C.c_void_p(self.col.data.ptr)

    @property
    def vptr(self):
        return C.c_void_p(self.col.validity.ptr) if self.col.validity is not None else None


def raw_count(j, blk):
    total = C.c_uint64(12345)
    T.check(T.lib().dbhip_join_probe_count(j.h, blk.kptr, blk.vptr, C.c_int64(blk.n), C.byref(total), None))
    return total.value


def raw_probe(gpu, j, blk, max_pairs, extra=8):
    """dbhip_join_probe into sentinel-filled buffers of max_pairs + extra words -> (rc, n_pairs, probe_idx words, build_row words)"""
    words = max(max_pairs, 0) + extra
    op, ob = filled(gpu, words * 4), filled(gpu, words * 4)
    got = C.c_uint64(12345)
    rc = T.lib().dbhip_join_probe(j.h, blk.kptr, blk.vptr, C.c_int64(blk.n), C.c_void_p(op.ptr), C.c_void_p(ob.ptr), C.c_int64(max_pairs),
                                  C.byref(got), None)
    return rc, got.value, op.to_numpy(np.uint32, words), ob.to_numpy(np.uint32, words)


def assert_pairs(res, blk, what):
    rc, got, op, ob = res
    assert rc == T.OK and got == blk.total, (what, rc, got, blk.total)
    assert np.array_equal(op[:got], blk.pairs[0]) and np.array_equal(ob[:got], blk.pairs[1]), what
    assert (op[got:] == SENT32).all() and (ob[got:] == SENT32).all(), (what, "words past n_pairs")


ABI_CASES = ("multiplicity_kb8", "sizes_n1025_kb16_nullable", "single_bit_kb32")


@pytest.mark.parametrize("name", ABI_CASES)
def test_probe_without_a_count_and_the_capacity_error(gpu, name):
    d = J.by_name(name).data()
    j = build_table(gpu, d)
    a = Block(gpu, d, d.probe_keys, d.probe_valid)
    assert a.total > 1
    assert_pairs(raw_probe(gpu, j, a, a.total), a, "no count before the probe, max_pairs == total")
    # one pair too many for the buffers: the error, the total, and nothing written
    for counted in (False, True):
        if counted:
            assert raw_count(j, a) == a.total
        rc, got, op, ob = raw_probe(gpu, j, a, a.total - 1)
        assert rc == T.ERR_CAPACITY and got == a.total, (counted, rc, got)
        assert (op == SENT32).all() and (ob == SENT32).all(), counted
        assert_pairs(raw_probe(gpu, j, a, a.total), a, "the probe after a capacity error")
    j.destroy()


@pytest.mark.parametrize("name", ABI_CASES)
def test_prepared_state_belongs_to_one_block_of_one_table(gpu, name):
    """the counts of dbhip_join_probe_count are reused by the probe of the SAME block only: blocks A and B have the same length and
    the same validity argument and differ in the key buffer alone (and, in a second round, in the validity buffer alone)"""
    d = J.by_name(name).data()
    j1, j2 = build_table(gpu, d), build_table(gpu, d)
    a = Block(gpu, d, d.probe_keys, d.probe_valid)
    b = Block(gpu, d, d.probe_keys[::-1].copy(), None if d.probe_valid is None else d.probe_valid[::-1].copy())
    assert a.total > 0 and not np.array_equal(a.pairs[0], b.pairs[0])
    blocks = [(a, b)]
    flipped = np.arange(a.n) % 3 != 0
    c1, c2 = Block(gpu, d, d.probe_keys, flipped), Block(gpu, d, d.probe_keys, ~flipped)
    c2.col.data = c1.col.data                                   # the same key buffer, two validity buffers
    blocks.append((c1, c2))
    for x, y in blocks:
        assert raw_count(j1, x) == x.total
        assert_pairs(raw_probe(gpu, j1, y, y.total), y, "count A, probe B")
        assert raw_count(j1, x) == x.total and raw_count(j1, y) == y.total
        assert_pairs(raw_probe(gpu, j1, x, x.total), x, "count A, count B, probe A")
        assert raw_count(j1, x) == x.total
        assert_pairs(raw_probe(gpu, j1, x, x.total), x, "count A, probe A")
        assert_pairs(raw_probe(gpu, j1, x, x.total), x, "... and A again without a count")
        # two tables interleaved
        assert raw_count(j1, x) == x.total and raw_count(j2, y) == y.total
        assert_pairs(raw_probe(gpu, j1, x, x.total), x, "t1 count A, t2 count B, t1 probe A")
        assert_pairs(raw_probe(gpu, j2, y, y.total), y, "t1 count A, t2 count B, t2 probe B")
        assert raw_count(j1, x) == x.total and raw_count(j2, x) == x.total
        assert_pairs(raw_probe(gpu, j2, y, y.total), y, "t1 count A, t2 count A, t2 probe B")
        assert_pairs(raw_probe(gpu, j1, x, x.total), x, "t1 count A, t2 count A, t1 probe A")
    j1.destroy()
    j2.destroy()


def test_keys_off_a_16_byte_boundary_take_the_general_count_kernel(gpu):
    """a key column of 8-byte keys that starts 8 bytes into an allocation (a sliced column): no tile goes through the 16-byte loads"""
    d = J.by_name("multiplicity_kb8").data()
    j = build_table(gpu, d)
    shifted = np.concatenate([np.zeros((1, 1), dtype=np.uint64), d.probe_keys])
    blk = Block(gpu, d, d.probe_keys, None)
    whole = gpu.DeviceBuffer.from_numpy(shifted)
    blk.col.data = gpu.BorrowedBuffer(whole.ptr + 8, d.n * 8, keep=whole)
    assert blk.col.data.ptr % 16 == 8
    assert raw_count(j, blk) == blk.total
    assert_pairs(raw_probe(gpu, j, blk, blk.total), blk, "keys at +8")
    j.destroy()


@pytest.mark.parametrize("kb", J.KEY_BYTES)
def test_probe_mark_writes_ceil_n_over_8_bytes(gpu, kb):
    d = J.by_name(f"sizes_n1025_kb{kb}_nullable").data()
    j = build_table(gpu, d)
    for n in (1, 7, 8, 9, 63, 64, 65, 257):
        for valid in (None, d.probe_valid[:n]):
            blk = Block(gpu, d, d.probe_keys[:n], valid)
            exp = np.zeros(n, dtype=bool)
            exp[blk.pairs[0]] = True
            nbytes = (n + 7) // 8
            bm = filled(gpu, nbytes + 24)
            matched = C.c_uint64(12345)
            T.check(T.lib().dbhip_join_probe_mark(j.h, blk.kptr, blk.vptr, C.c_int64(n), C.c_void_p(bm.ptr), C.byref(matched), None))
            raw = bm.to_numpy(np.uint8, nbytes + 24)
            assert (raw[nbytes:] == SENT).all(), (n, "bytes past ceil(n / 8)")
            bits = np.unpackbits(raw[:nbytes], bitorder="little")
            assert np.array_equal(bits[:n].astype(bool), exp) and not bits[n:].any(), n
            assert matched.value == int(exp.sum()) == int(bits.sum()), n
    j.destroy()


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 1000])
def test_mark_build_and_build_matched(gpu, nb):
    L = T.lib()
    j = gpu.HashJoin(nb, key_bytes=8)
    j.add_block(packed(gpu, np.arange(nb, dtype=np.uint64).reshape(-1, 1), None, 8))
    j.final_build()
    nbytes = (nb + 63) // 64 * 8

    def read():
        out = filled(gpu, nbytes + 32)
        rows = C.c_int64(-1)
        T.check(L.dbhip_join_build_matched(j.h, C.c_void_p(out.ptr), C.byref(rows), None))
        T.check(L.dbhip_stream_sync(None))
        raw = out.to_numpy(np.uint8, nbytes + 32)
        assert rows.value == nb
        assert (raw[nbytes:] == SENT).all(), "the copy is ceil(rows / 64) * 8 bytes"
        bits = np.unpackbits(raw[:nbytes], bitorder="little").astype(bool)
        assert not bits[nb:].any(), "bits at and past the row count"
        return bits[:nb]

    rows = C.c_int64(-1)
    T.check(L.dbhip_join_build_matched(j.h, None, C.byref(rows), None))
    assert rows.value == nb
    assert not read().any()                                                        # before any mark
    rng = np.random.default_rng(nb)
    first = np.concatenate([rng.integers(0, nb, 40), [0, 0, nb - 1, nb - 1, nb, nb + 1, nb + 63, 0xFFFFFFFF, 0x80000000]]).astype(np.uint32)
    second = np.concatenate([[nb, 0xFFFFFFFF], np.repeat(rng.integers(0, nb, 7), 300)]).astype(np.uint32)
    exp = np.zeros(nb, dtype=bool)
    for marks in (first, second, np.zeros(0, dtype=np.uint32)):
        buf = gpu.DeviceBuffer.from_numpy(marks)
        T.check(L.dbhip_join_mark_build(j.h, C.c_void_p(buf.ptr), C.c_int64(len(marks)), None))
        exp |= R.bits_set(marks, nb)
        assert np.array_equal(read(), exp), (nb, len(marks))                        # calls accumulate, ids >= rows are ignored
    assert exp.any() and (nb < 64 or not exp.all())
    j.destroy()


@pytest.mark.parametrize("nbits", [1, 31, 32, 33, 64, 1000])
def test_bitmap_set_indices(gpu, nbits):
    L = T.lib()
    words = (nbits + 31) // 32
    rng = np.random.default_rng(nbits)
    for n_idx in (0, 1, 63, 64, 65, 5000):
        runs = np.sort(rng.integers(0, max(nbits // 2, 1), n_idx)).astype(np.uint32)       # a pair list's probe rows: long runs of equal indices
        mixed = rng.integers(0, nbits + 40, n_idx).astype(np.uint32)                        # shuffled, some past the end
        if n_idx > 2:
            mixed[[0, n_idx // 2, n_idx - 1]] = [nbits, 0xFFFFFFFF, nbits - 1]
        for idx in (runs, mixed):
            bm = filled(gpu, words * 4 + 32)
            T.check(L.dbhip_memset(C.c_void_p(bm.ptr), 0, C.c_size_t(words * 4), None))
            ib = gpu.DeviceBuffer.from_numpy(idx)
            T.check(L.dbhip_bitmap_set_indices(C.c_void_p(ib.ptr), C.c_int64(n_idx), C.c_void_p(bm.ptr), C.c_int64(nbits), None))
            raw = bm.to_numpy(np.uint8, words * 4 + 32)
            assert (raw[words * 4:] == SENT).all(), (nbits, n_idx, "words past ceil(nbits / 32)")
            bits = np.unpackbits(raw[:words * 4], bitorder="little").astype(bool)
            assert np.array_equal(bits[:nbits], R.bits_set(idx, nbits)) and not bits[nbits:].any(), (nbits, n_idx)
    bm = filled(gpu, 64)
    ib = gpu.DeviceBuffer.from_numpy(np.zeros(4, dtype=np.uint32))
    for off in (1, 2, 3):
        assert L.dbhip_bitmap_set_indices(C.c_void_p(ib.ptr), C.c_int64(4), C.c_void_p(bm.ptr + off), C.c_int64(nbits), None) == T.ERR_INVALID
    assert (bm.to_numpy(np.uint8, 64) == SENT).all()


# ---- the join on serialized keys --------------------------------------------------------------------------------------------------------
def set_mask(mask):
    L = T.lib()
    L.dbhip_join_binary_debug_set_hash_mask.argtypes = [C.c_uint64]
    T.check(L.dbhip_join_binary_debug_set_hash_mask(C.c_uint64(mask)))


class RawRows:
    """a BinaryColumn in HBM: offsets[n + 1] that start at `base` (the bytes before it are not part of any row), data, validity"""

    def __init__(self, gpu, rows, valid, base=0):
        self.n = len(rows)
        lens = np.array([len(r) for r in rows], dtype=np.uint64)
        off = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(lens, dtype=np.uint64)]) + np.uint64(base)
        data = np.frombuffer(b"\xEE" * base + b"".join(rows) + b"\xEE" * 16, dtype=np.uint8)
        self.off, self.data = gpu.DeviceBuffer.from_numpy(off), gpu.DeviceBuffer.from_numpy(data)
        self.valid = gpu.DeviceBuffer.from_numpy(gpu.pack_bits(valid)) if valid is not None else None

    def args(self):
        return C.c_void_p(self.off.ptr), C.c_void_p(self.data.ptr), C.c_void_p(self.valid.ptr) if self.valid is not None else None, C.c_int64(self.n)


def raw_binary_table(gpu, d):
    L = T.lib()
    h = C.c_void_p()
    T.check(L.dbhip_join_create_binary(C.c_int64(d.expected_build_rows), C.byref(h)))
    for (rows, valid), base in zip(d.build_blocks, d.extra["offset_base"]):
        blk = RawRows(gpu, rows, valid, base)
        T.check(L.dbhip_join_add_build_binary(h, *blk.args(), None))
        T.check(L.dbhip_stream_sync(None))
    T.check(L.dbhip_join_finalize_binary(h, None))
    return h


def raw_binary_probe(gpu, h, blk, max_pairs=None):
    """-> (rc, candidates, n_pairs, probe_idx words, build_row words, matched bytes); buffers sentinel-filled past what may be written"""
    L = T.lib()
    cand = C.c_uint64(12345)
    T.check(L.dbhip_join_probe_count_binary(h, *blk.args(), C.byref(cand), None))
    m = cand.value if max_pairs is None else max_pairs
    words = max(m, 0) + 8
    op, ob = filled(gpu, words * 4), filled(gpu, words * 4)
    mbytes = (blk.n + 31) // 32 * 4
    mark = filled(gpu, mbytes + 32)
    got = C.c_uint64(12345)
    rc = L.dbhip_join_probe_binary(h, *blk.args(), C.c_void_p(op.ptr), C.c_void_p(ob.ptr), C.c_int64(m), C.byref(got), C.c_void_p(mark.ptr), None)
    T.check(L.dbhip_stream_sync(None))
    return rc, cand.value, got.value, op.to_numpy(np.uint32, words), ob.to_numpy(np.uint32, words), mark.to_numpy(np.uint8, mbytes + 32)


def check_binary(gpu, h, d, probe_rows, probe_valid, what):
    exp = R.inner_pairs_dict(d.build_keys(), d.build_valid(), probe_rows, probe_valid)
    n = len(probe_rows)
    blk = RawRows(gpu, probe_rows, probe_valid, base=3)
    rc, cand, got, op, ob, mark = raw_binary_probe(gpu, h, blk)
    assert rc == T.OK and got == len(exp[0]) and cand >= got, (what, rc, got, cand)
    assert np.array_equal(op[:got], exp[0]) and np.array_equal(ob[:got], exp[1]), what
    mbytes = (n + 31) // 32 * 4
    assert (mark[mbytes:] == SENT).all(), (what, "bytes past ceil(n / 32) * 4")
    bits = np.unpackbits(mark[:mbytes], bitorder="little").astype(bool)
    em = np.zeros(n, dtype=bool)
    em[exp[0]] = True
    assert np.array_equal(bits[:n], em) and not bits[n:].any(), (what, "matched")
    return blk, cand, got


@pytest.mark.parametrize("mask", [ONES, 0xFF, 0], ids=["full_hash", "8_bits", "no_hash"])
def test_binary_table(gpu, mask):
    """keys of 0, 1, 7, 8, 9, 15, 16, 17 and 4 096 bytes, b"a" / b"a\\0", every prefix of a 20-byte key, keys equal but for their last byte;
    NULL rows with matching bytes, duplicates on both sides, build blocks of 1, 2, 50 and 147 rows of which two have offsets that do not
    start at 0; with the hash masked to 8 and to 0 bits the byte compare decides every pair"""
    d = J.binary_cases()[0].data()
    set_mask(mask)
    try:
        h = raw_binary_table(gpu, d)
        blk, cand, got = check_binary(gpu, h, d, d.probe_keys, d.probe_valid, "whole table")
        assert got > 100
        if mask == 0:
            assert cand == int(d.probe_valid.sum()) * int(d.build_valid().sum())    # every pair of valid rows is a candidate
        for n in (1, 31, 32, 33):                                                    # the matched bitmap around one 32-bit word
            check_binary(gpu, h, d, d.probe_keys[4:4 + n], d.probe_valid[4:4 + n], n)
            check_binary(gpu, h, d, d.probe_keys[:n], None, n)
        # fewer pairs than candidates fit: refused, nothing written
        rc, cand2, _, op, ob, _ = raw_binary_probe(gpu, h, blk, max_pairs=cand - 1)
        assert rc == T.ERR_CAPACITY and cand2 == cand and (op == SENT32).all() and (ob == SENT32).all()
        check_binary(gpu, h, d, d.probe_keys, d.probe_valid, "after the capacity error")
        T.check(T.lib().dbhip_join_destroy_binary(h))
        # the same rows as a nullable String column through BinaryHashJoin (serialized: valid byte, u64 length, bytes)
        j = gpu.BinaryHashJoin(d.expected_build_rows)
        for rows, valid in d.build_blocks:
            j.add_block([gpu.Column.strings(rows, validity=valid)], len(rows))
        j.final_build()
        pi, bi, matched = j.probe_block([gpu.Column.strings(d.probe_keys, validity=d.probe_valid)], d.n)
        exp = R.inner_pairs_dict(*d.ref_args())
        assert np.array_equal(pi, exp[0]) and np.array_equal(bi, exp[1])
        assert np.array_equal(matched, np.isin(np.arange(d.n), exp[0]))
        j.destroy()
    finally:
        set_mask(ONES)


def test_binary_assemblies_from_the_matched_bitmap(gpu):
    """left_anti and full over the binary table, assembled the way a binding does: the pairs, the matched bitmap of the probe rows and
    dbhip_bitmap_set_indices over the pairs' build rows"""
    d = J.binary_cases()[0].data()
    args = d.ref_args()
    h = raw_binary_table(gpu, d)
    blk = RawRows(gpu, d.probe_keys, d.probe_valid)
    rc, _, got, op, ob, mark = raw_binary_probe(gpu, h, blk)
    assert rc == T.OK
    matched = np.unpackbits(mark[:(d.n + 31) // 32 * 4], bitorder="little")[:d.n].astype(bool)
    words = (d.nb + 31) // 32
    bm = gpu.DeviceBuffer(words * 4).zero()
    ib = gpu.DeviceBuffer.from_numpy(ob[:got])
    T.check(T.lib().dbhip_bitmap_set_indices(C.c_void_p(ib.ptr), C.c_int64(got), C.c_void_p(bm.ptr), C.c_int64(d.nb), None))
    built = np.unpackbits(bm.to_numpy(np.uint8, words * 4), bitorder="little")[:d.nb].astype(bool)
    none = lambda k: np.full(k, -1, dtype=np.int64)   # noqa: E731
    ep, eb = R.join_rows("left_anti", *args)
    assert np.array_equal(np.flatnonzero(~matched), ep) and (eb == -1).all()
    ep, eb = R.join_rows("full", *args)
    gp = np.concatenate([op[:got].astype(np.int64), np.flatnonzero(~matched), none(int((~built).sum()))])
    gb = np.concatenate([ob[:got].astype(np.int64), none(int((~matched).sum())), np.flatnonzero(~built)])
    assert np.array_equal(gp, ep) and np.array_equal(gb, eb)
    T.check(T.lib().dbhip_join_destroy_binary(h))
