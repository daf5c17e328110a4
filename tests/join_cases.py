"""The case tables of the hash-join edge suite: plain data, shared by tests/test_join_ref_cpu.py (which shows that the tables can see
wrong joins at all) and tests/test_gpu_join_edges.py (which runs them through HashJoin / BinaryHashJoin and the C ABI).

A Case is a name, a table, a key width and a recipe; Case.data() makes the rows: the build side as a LIST of blocks (growth across
add_block calls is part of the case), `expected_build_rows`, the probe keys and both validities. Keys are (n, KW) u64 arrays, or
lists of bytes in the `binary` table. The cases with hundreds of thousands of rows also carry one u64 id per row, equal ids <=> equal
keys (widen() is injective), so that the reference can join ids instead of 32-byte rows.

The two size thresholds of the long_blocks table restate the host code of k_join.hip; see count_steps() and emit_group()."""
import numpy as np

TILE = 256                      # JOIN_TILE: probe rows per wave and step
MAX_GRID = 4096                 # workgroups of four waves: the count and emit passes launch at most this many
U64 = np.uint64
_MUL = [U64(0x9E3779B97F4A7C15), U64(0xC2B2AE3D27D4EB4F), U64(0x165667B19E3779F9)]
_ODD = U64(0xD6E8FEB86659FD93)
KEY_BYTES = (8, 16, 32)


def count_steps(n):
    """Steps of the busiest wave in join_count_kernel. join_count_block: nfull = n / 256 full tiles, grid = ceil(nfull / 4) workgroups
    while nfull < 4 * 4096 and 4096 from there on; a wave walks tiles t, t + 4 * grid, ... So every wave takes ONE step up to
    nfull = 16 384, and wave w takes a second one iff w + 16 384 < nfull: the first probe block with a second step has
    nfull = 16 385 full tiles, n = 16 385 * 256 = 4 194 560 rows."""
    nfull = n // TILE
    if nfull == 0:
        return 0
    grid = -(-nfull // 4) if nfull < 4 * MAX_GRID else MAX_GRID
    return -(-nfull // (4 * grid))


def emit_group(n):
    """G of join_emit_kernel, the consecutive tiles a wave takes per step. dbhip_join_probe: ntiles = ceil(n / 256), grid as in the
    count pass, G doubles while grid * 4 * 2G <= ntiles (up to 64). Below 16 384 tiles grid * 4 >= ntiles, so G = 1; from there on
    grid * 4 = 16 384: G = 2 needs ntiles >= 32 768 (n >= 32 767 * 256 + 1 = 8 388 353), G = 4 needs ntiles >= 65 536
    (n >= 65 535 * 256 + 1 = 16 776 961)."""
    ntiles = -(-n // TILE)
    grid = -(-ntiles // 4) if ntiles < 4 * MAX_GRID else MAX_GRID
    g = 1
    while g < 64 and grid * 4 * (g * 2) <= ntiles:
        g *= 2
    return g


def widen(ids, kw):
    """An injective image of u64 ids in KW words: the last word is id * odd (a bijection of the u64s), the words before it depend on
    id >> 1 only — the keys of ids 2m and 2m + 1 differ in the LAST word alone."""
    ids = np.asarray(ids, dtype=U64)
    if kw == 1:
        return ids.reshape(-1, 1).copy()
    out = np.empty((len(ids), kw), dtype=U64)
    half = ids >> U64(1)
    for w in range(kw - 1):
        out[:, w] = half * _MUL[w] + U64(w)
    out[:, kw - 1] = ids * _ODD
    return out


class Data:
    def __init__(self, key_bytes, build_blocks, probe_keys, probe_valid=None, expected_build_rows=1024, build_ids=None, probe_ids=None, **extra):
        self.key_bytes, self.build_blocks, self.expected_build_rows = key_bytes, build_blocks, expected_build_rows
        self.probe_keys, self.probe_valid = probe_keys, probe_valid
        self.build_ids, self.probe_ids = build_ids, probe_ids
        self.extra = extra

    @property
    def kw(self):
        return self.key_bytes // 8

    @property
    def n(self):
        return len(self.probe_keys)

    @property
    def nb(self):
        return sum(len(k) for k, _ in self.build_blocks)

    def build_keys(self):
        ks = [k for k, _ in self.build_blocks]
        if self.key_bytes == 0:
            return [r for k in ks for r in k]
        return np.concatenate(ks) if ks else np.zeros((0, self.kw), dtype=U64)

    def build_valid(self):
        if all(v is None for _, v in self.build_blocks):
            return None
        return np.concatenate([np.ones(len(k), dtype=bool) if v is None else np.asarray(v, dtype=bool) for k, v in self.build_blocks])

    def ref_args(self):
        """(build keys, build validity, probe keys, probe validity) for tests/join_ref.py: the ids where the case has them"""
        if self.build_ids is not None:
            return self.build_ids.reshape(-1, 1), self.build_valid(), self.probe_ids.reshape(-1, 1), self.probe_valid
        return self.build_keys(), self.build_valid(), self.probe_keys, self.probe_valid


class Case:
    def __init__(self, table, name, key_bytes, make, big=False):
        self.table, self.name, self.key_bytes, self._make, self.big = table, name, key_bytes, make, big

    def data(self):
        return self._make()

    def __repr__(self):
        return self.name


def split(keys, valid, sizes):
    """(keys, valid) cut into consecutive blocks of the given sizes (the last one takes the rest when it is None)"""
    out, lo = [], 0
    for s in sizes:
        hi = len(keys) if s is None else lo + s
        out.append((keys[lo:hi], None if valid is None else valid[lo:hi]))
        lo = hi
    assert lo == len(keys)
    return out


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)


def _sizes(n, kb, with_valid):
    def make():
        bids = (np.arange(300, dtype=U64) % U64(220)) * U64(2)            # even ids, 80 of them twice
        i = np.arange(n, dtype=U64)
        hit = ((i * U64(7)) % U64(220)) * U64(2)
        near = ((i * U64(5)) % U64(220)) * U64(2) + U64(1)                   # the odd twin: equal up to the last key word
        pids = np.where(i % U64(3) == 1, near, hit)
        pids = np.where(i % U64(11) == 10, U64(10_000) + i, pids)
        pv = (i % U64(5) != 2) if with_valid else None                       # (the NULL rows 2, 12, 17, ... carry matching keys)
        return Data(kb, [(widen(bids, kb // 8), None)], widen(pids, kb // 8), pv, expected_build_rows=300)
    return Case("sizes", f"sizes_n{n}_kb{kb}_{'nullable' if with_valid else 'plain'}", kb, make)


# ---- multiplicity -----------------------------------------------------------------------------------------------------------------------
MULTIPLICITIES = (1, 2, 3, 254, 255, 256, 257, 511, 1000)


def _multiplicity(kb):
    def make():
        rng = np.random.default_rng(kb)
        blocks = []
        for j in range(3):                                                    # row r of a key goes to block r % 3: two rows, two blocks
            ids = np.concatenate([np.full((m - j + 2) // 3, 2 * (k + 1), dtype=U64) for k, m in enumerate(MULTIPLICITIES)])
            blocks.append(ids[rng.permutation(len(ids))])
        bids = np.concatenate(blocks)
        sizes = [len(b) for b in blocks]
        pids = U64(5_000) + np.arange(300, dtype=U64) * U64(2)                # absent
        for k in range(len(MULTIPLICITIES)):
            pids[7 * k + 3] = 2 * (k + 1)                                     # once in the full tile
            pids[256 + 2 * k + 1] = 2 * (k + 1)                               # once in the ragged tile
        pids[250] = 3                                                         # the odd twin of the key with one build row
        kw = kb // 8
        return Data(kb, split(widen(bids, kw), None, sizes), widen(pids, kw), None, expected_build_rows=1024,
                    block0_rows=sizes[0], block_rows=sizes)
    return Case("multiplicity", f"multiplicity_kb{kb}", kb, make)


# ---- single_bit -------------------------------------------------------------------------------------------------------------------------
BITS = (0, 31, 32, 63)
WORD0 = (0, 1, 63, 64, 65, 2**32, 2**63, 2**64 - 1)


def _single_bit(kb):
    def make():
        kw = kb // 8
        bases = [[0x5A5A5A5A3C3C3C3C + 0x0101010101010101 * w for w in range(kw)], [0xA5A5C3C3A5A5C3C3 - 0x1111 * w for w in range(kw)]]
        build, probe, flips = list(bases), list(bases), []
        for which, base in enumerate(bases):
            for w in range(kw):
                for bi, b in enumerate(BITS):
                    key = list(base)
                    key[w] ^= 1 << b
                    in_build = (bi + w + which) % 2 == 0               # every (word, bit) is in the build side for exactly one base
                    if in_build:
                        build.append(key)
                    flips.append((w, b, len(probe), in_build))
                    probe.append(key)
        for k, v in enumerate(WORD0):                                  # word 0 at the edges of the bucket arithmetic, the other words of base 0
            key = [v] + bases[0][1:]
            if k % 2 == 0:
                build.append(key)
            probe.append(key)
        for k, lead in enumerate((1 << 20, (1 << 40) + 17, 2**64 - 300)):   # runs k, k + 64, k + 128: consecutive buckets for one-word keys
            for step in range(3):
                key = [lead + 64 * step] + bases[0][1:]
                if (step == 1) == (k == 1):
                    build.append(key)
                probe.append(key)
        build = build + build[::3]                                     # some keys twice
        assert len(build) <= 512
        probe = (probe * (300 // len(probe) + 1))[:max(300, len(probe))]   # past one full tile: both count kernels see every key
        return Data(kb, [(np.array(build, dtype=U64).reshape(-1, kw), None)], np.array(probe, dtype=U64).reshape(-1, kw), None,
                    expected_build_rows=len(build), flips=flips)
    return Case("single_bit", f"single_bit_kb{kb}", kb, make)


# ---- validity ---------------------------------------------------------------------------------------------------------------------------
VALIDITY_N = 1024 + 37


def validity_pattern(name, n):
    i = np.arange(n)
    if name in ("0x55", "0xAA", "0x0F", "0xF0"):
        return ((int(name, 16) >> (i % 8)) & 1).astype(bool)
    return {"ones": np.ones(n, dtype=bool), "zeros": np.zeros(n, dtype=bool), "first": i == 0, "last": i == n - 1}[name]


PATTERNS = ("ones", "zeros", "0x55", "0xAA", "0x0F", "0xF0", "first", "last")


def _validity(side, pattern, kb):
    def make():
        kw, n = kb // 8, VALIDITY_N
        i = np.arange(n, dtype=U64)
        if side == "probe":
            bids = (np.arange(300, dtype=U64) % U64(211)) * U64(2)
            pids = ((i * U64(7)) % U64(300)) * U64(2)                        # ids below 422 match
            pids[0] = pids[n - 1] = 8
            return Data(kb, [(widen(bids, kw), None)], widen(pids, kw), validity_pattern(pattern, n), expected_build_rows=300)
        bids = (i % U64(211)) * U64(2)                                       # every key on five or six build rows, 211 apart
        pids = ((np.arange(600, dtype=U64) * U64(7)) % U64(300)) * U64(2)
        pids[5] = 0                                                          # build rows 0 and n - 1 have partners
        pids[6] = (n - 1) % 211 * 2
        return Data(kb, [(widen(bids, kw), validity_pattern(pattern, n))], widen(pids, kw), None, expected_build_rows=n)
    return Case("validity", f"validity_{side}_{pattern}_kb{kb}", kb, make)


# ---- growth -----------------------------------------------------------------------------------------------------------------------------
GROWTH_BLOCKS = (1, 1023, 1, 1024, 0, 3000, 70_000)


def _growth(kb, expected):
    def make():
        kw, nb = kb // 8, sum(GROWTH_BLOCKS)
        rng = np.random.default_rng(kb + expected)
        bids = rng.integers(0, 60_000, nb).astype(U64) * U64(2)
        bids[:2] = [0, 2]
        bv = rng.random(nb) < 0.9
        bv[:2] = True
        pids = rng.integers(0, 150_000, 5000).astype(U64)
        pids[:3] = [0, 2, 1]
        pv = rng.random(5000) < 0.9
        pv[:3] = True
        return Data(kb, split(widen(bids, kw), bv, list(GROWTH_BLOCKS)), widen(pids, kw), pv, expected_build_rows=expected,
                    block0_rows=GROWTH_BLOCKS[0])
    return Case("growth", f"growth_kb{kb}_expected{expected}", kb, make)


def _growth_empty(kb, blocks):
    def make():
        kw = kb // 8
        pids = np.arange(300, dtype=U64)
        return Data(kb, [(np.zeros((0, kw), dtype=U64), None)] * blocks, widen(pids, kw), None, expected_build_rows=0)
    return Case("growth", f"growth_empty_kb{kb}_{blocks}blocks", kb, make)


def _growth_all_null(kb):
    def make():
        kw = kb // 8
        ids = np.arange(300, dtype=U64)
        return Data(kb, [(widen(ids, kw), np.zeros(300, dtype=bool))], widen(ids, kw), None, expected_build_rows=1)
    return Case("growth", f"growth_all_null_kb{kb}", kb, make)


# ---- occupancy --------------------------------------------------------------------------------------------------------------------------
def _occupancy(kb, with_valid):
    def make():
        kw = kb // 8
        rng = np.random.default_rng(kb + with_valid)
        bids = rng.integers(0, 200_000, 270_000).astype(U64) * U64(2)        # even ids, duplicates; 540 000 < 2^20 buckets: OCC is built
        pids = rng.integers(0, 500_000, 300_077).astype(U64)                 # even: mostly hits; odd: the twin, equal up to the last word
        bv = (rng.random(270_000) < 0.95) if with_valid else None
        pv = (rng.random(300_077) < 0.9) if with_valid else None
        return Data(kb, split(widen(bids, kw), bv, [100_000, None]), widen(pids, kw), pv, expected_build_rows=270_000, build_ids=bids, probe_ids=pids,
                    block0_rows=100_000)
    return Case("occupancy", f"occupancy_kb{kb}_{'nullable' if with_valid else 'plain'}", kb, make, big=True)


# ---- long_blocks ------------------------------------------------------------------------------------------------------------------------
LONG_COUNT_N = 16_385 * 256 + 3 * 256 + 5        # count_steps() == 2: tiles 0..3 and 16 384..16 387 share a wave, five ragged rows
LONG_G2_N = 8_388_608 + 261                      # emit_group() == 2
LONG_G4_N = 16_777_216 + 261                     # emit_group() == 4
LONG_PARTNERS = (2, 3, 255, 300)


def hot_tiles(n):
    """the ~1 % of the tiles that hold every matching probe row of a long_blocks case: the tiles of the first wave's two steps, the
    last full and the ragged tile, and every 97th group of tiles in a pattern that leaves whole groups empty and others with gaps"""
    ntiles = -(-n // TILE)
    t = np.arange(ntiles)
    hot = (t % 97 == 5) | ((t % 1552 >= 776) & (t % 1552 < 780) & (t % 2 == 1)) | ((t % 3104 >= 2000) & (t % 3104 < 2004) & (t % 4 != 2))
    hot[:4] = True
    hot[16_384:16_388] = True
    hot[-2:] = True
    return hot


def _long(kb, n):
    def make():
        kw = kb // 8
        nkeys = 1000
        mult = np.ones(nkeys, dtype=np.int64)
        for k, m in enumerate(LONG_PARTNERS):
            mult[100 * k + 7::400] = m                                       # ids 7, 407, 807 have 2 partners, 107, 507, 907 have 3, ...
        bids = np.repeat(np.arange(nkeys, dtype=U64) * U64(2), mult)
        bids = bids[np.random.default_rng(3).permutation(len(bids))]
        i = np.arange(n, dtype=U64)
        h = (i * U64(0x9E3779B97F4A7C15)) >> U64(40)                         # 24 well-mixed bits per row
        pids = U64(1 << 32) + i                                              # absent, all different
        row_hot = np.repeat(hot_tiles(n), TILE)[:n]
        cand = row_hot & ((h & U64(1)) == 0)                                 # half the rows of a hot tile
        twin = (h >> U64(1)) & U64(7)                                        # one in eight of them probes the odd twin (a near miss)
        pids[cand] = ((h[cand] >> U64(4)) % U64(nkeys)) * U64(2) + (twin[cand] == 0).astype(U64)
        pv = ((h >> U64(14)) & U64(7)) != 0                                  # 1 / 8 NULL, NULL rows of hot tiles carry matching keys
        third = len(bids) // 3
        return Data(kb, split(widen(bids, kw), None, [third, third, None]), widen(pids, kw), pv, expected_build_rows=len(bids), build_ids=bids,
                    probe_ids=pids, block0_rows=third)
    return Case("long_blocks", f"long_n{n}_kb{kb}", kb, make, big=True)


# ---- binary -----------------------------------------------------------------------------------------------------------------------------
BINARY_BLOCKS = (1, 2, 50, None)
BINARY_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 4096)


def _binary():
    def make():
        long20 = b"0123456789abcdefghij"
        pool = [b""] + [bytes((37 * k + 11 * ln) % 251 for k in range(ln)) for ln in BINARY_LENGTHS] + [b"a", b"a\0"]
        pool += [long20[:k] for k in range(1, 20)] + [long20]
        pool += [b"equal but the last byte-1", b"equal but the last byte-2"]
        big = bytes((k * 7) % 256 for k in range(4096))
        pool += [big[:-1] + b"\x01"]                                         # 4 096 bytes, differs from nothing but in its last byte
        absent = [b"\0", b"a\0\0", long20 + b"k", big[:-1] + b"\x02", b"equal but the last byte-3", bytes(8), bytes(16)]
        in_build = [k for k in range(len(pool)) if k % 4 != 3 or k <= 10 or len(pool[k]) == 4096]   # some prefixes and a last-byte twin are probed only
        build = [pool[in_build[r % len(in_build)]] for r in range(200)]                        # every build key three to six times
        bv = np.array([r % 9 != 4 for r in range(200)])                                        # NULL rows carry keys that valid rows carry too
        both = pool + absent
        probe = [both[(5 * r) % len(both)] for r in range(300)]
        pv = np.array([r % 7 != 3 for r in range(300)])
        return Data(0, split(build, bv, list(BINARY_BLOCKS)), probe, pv, expected_build_rows=1, offset_base=(0, 0, 37, 5), block0_rows=1)
    return Case("binary", "binary", 0, make)


# ---- the tables -------------------------------------------------------------------------------------------------------------------------
def sizes_cases():
    return [_sizes(n, kb, v) for kb in KEY_BYTES for n in SIZES for v in (False, True)]


def multiplicity_cases():
    return [_multiplicity(kb) for kb in KEY_BYTES]


def single_bit_cases():
    return [_single_bit(kb) for kb in KEY_BYTES]


def validity_cases():
    return [_validity(side, p, kb) for kb in KEY_BYTES for side in ("probe", "build") for p in PATTERNS]


def growth_cases():
    out = [_growth(kb, e) for kb in KEY_BYTES for e in (0, 1)]
    out += [_growth_empty(8, 0), _growth_empty(16, 1), _growth_empty(32, 2)]
    return out + [_growth_all_null(kb) for kb in KEY_BYTES]


def occupancy_cases():
    return [_occupancy(kb, v) for kb in (16, 32) for v in (False, True)]


def long_cases():
    return [_long(kb, LONG_COUNT_N) for kb in KEY_BYTES] + [_long(8, LONG_G2_N), _long(8, LONG_G4_N)]


def binary_cases():
    return [_binary()]


def fixed_cases():
    return sizes_cases() + multiplicity_cases() + single_bit_cases() + validity_cases() + growth_cases() + occupancy_cases() + long_cases()


def by_name(name):
    for c in fixed_cases() + binary_cases():
        if c.name == name:
            return c
    raise KeyError(name)


# the cases whose expected result is empty by construction: a pair there would be the bug
NO_PAIRS = ("validity_probe_zeros", "validity_build_zeros", "growth_empty", "growth_all_null")
