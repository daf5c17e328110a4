"""CPU: tests/join_ref.py and tests/join_cases.py — the reference and the case tables that tests/test_gpu_join_edges.py holds the hash
join to — checked before anything runs on a device.

The reference: its dictionary form, its vectorised twin and (on one-word keys) the C oracle's orc_join_inner_u64 agree exactly.

The tables have teeth: every case has a pair and a probe row without a partner (the cases that are empty by construction have pairs
as soon as their validity is taken away), single_bit holds every (word, bit) once as a hit and once as a near miss, the long blocks
take the second count step and G = 2 / G = 4 with an empty group of tiles and a group with gaps.

The tables reject wrong joins. Each defect below is a join that is wrong in one way; the case named beside it tells it apart from the
right one:
  word0_only          compares word 0 only                                        single_bit_kb16
  low32_only          compares the low 32 bits of every word                      single_bit_kb8
  last_word_ignored   ignores the last key word                                   sizes_n257_kb32_plain
  nulls_match         validity is ignored on both sides                           validity_probe_0x55_kb8
  count_wraps_256     a probe row emits count mod 256 pairs                       multiplicity_kb8
  count_stuck_255     a count saturates at 255 and is not counted again           multiplicity_kb16
  ragged_tile_lost    the probe rows past the last full tile of 256 are dropped   sizes_n513_kb8_plain
  nibbles_swapped     the two nibbles of every probe validity byte are swapped    validity_probe_0x0F_kb8
  chain_order         a probe row's build rows come newest first, not ascending   multiplicity_kb32
  first_block_only    only the first build block is kept                          growth_kb8_expected0"""
import ctypes as C

import numpy as np
import pytest

from tests import join_cases as J
from tests import join_ref as R

SMALL = [c for c in J.fixed_cases() if not c.big]


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype == np.uint32


def oracle_pairs(oracle, bk, bv, pk, pv):
    bits = lambda v, n: np.concatenate([np.packbits(np.ones(n, bool) if v is None else v, bitorder="little"), np.zeros(8, np.uint8)])   # noqa: E731
    bk, pk = np.ascontiguousarray(bk.reshape(-1)), np.ascontiguousarray(pk.reshape(-1))
    bb, pb = bits(bv, len(bk)), bits(pv, len(pk))
    p = C.c_void_p
    count = oracle.orc_join_inner_u64(bk.ctypes.data_as(p), bb.ctypes.data_as(p), C.c_int64(len(bk)), pk.ctypes.data_as(p), pb.ctypes.data_as(p),
                                      C.c_int64(len(pk)), None, None, C.c_int64(0))
    op, ob = np.zeros(count + 1, np.uint32), np.zeros(count + 1, np.uint32)
    got = oracle.orc_join_inner_u64(bk.ctypes.data_as(p), bb.ctypes.data_as(p), C.c_int64(len(bk)), pk.ctypes.data_as(p), pb.ctypes.data_as(p),
                                    C.c_int64(len(pk)), op.ctypes.data_as(p), ob.ctypes.data_as(p), C.c_int64(count + 1))
    assert got == count
    return op[:count], ob[:count]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["sizes", "multiplicity", "single_bit", "validity", "growth"])
def test_dictionary_form_twin_and_oracle_agree(oracle, table):
    cases = [c for c in SMALL if c.table == table]
    assert cases
    for c in cases:
        d = c.data()
        args = (d.build_keys(), d.build_valid(), d.probe_keys, d.probe_valid)
        exp = R.inner_pairs_dict(*args)
        assert same(R.inner_pairs_fast(*args), exp), c
        assert same(R.inner_pairs(*args), exp), c
        if d.kw == 1:
            assert same(oracle_pairs(oracle, *args), exp), c
        order = np.lexsort((exp[1], exp[0]))
        assert np.array_equal(order, np.arange(len(order))), c            # sorted by (probe_idx, build_row)
        assert np.array_equal(R.matched_probe(*args), np.isin(np.arange(d.n), exp[0])), c


def test_binary_forms_agree_and_compare_bytes():
    d = J.binary_cases()[0].data()
    args = (d.build_keys(), d.build_valid(), d.probe_keys, d.probe_valid)
    exp = R.inner_pairs_dict(*args)
    assert same(R.inner_pairs_fast(*args), exp) and len(exp[0]) > 100
    bk, pk = args[0], args[2]
    assert all(bk[b] == pk[p] and args[1][b] and args[3][p] for p, b in zip(exp[0].tolist(), exp[1].tolist()))
    lengths = {len(pk[p]) for p in exp[0].tolist()}
    assert {0, 1, 7, 8, 9, 15, 16, 17, 4096} <= lengths                   # every length of the issue is joined at least once
    unmatched = {pk[p] for p in range(d.n) if d.probe_valid[p]} - {pk[p] for p in exp[0].tolist()}
    assert b"a\0\0" in unmatched and any(len(k) == 4096 for k in unmatched) and any(b"0123456789abcdefghij".startswith(k) for k in unmatched)
    assert [len(k) for k, _ in d.build_blocks] == [1, 2, 50, 147] and any(d.extra["offset_base"])


def test_ids_stand_for_wide_keys():
    """the big cases join ids: widen() keeps different ids apart and equal ids together, ids 2m and 2m + 1 differ in the last word only"""
    ids = np.concatenate([np.arange(5000, dtype=np.uint64), np.arange(2**40, 2**40 + 5000, dtype=np.uint64), np.arange(100, dtype=np.uint64)])
    for kw in (1, 2, 4):
        keys = J.widen(ids, kw)
        bid, _ = R.key_ids(keys, keys[:1])
        first = {}
        assert all(first.setdefault(int(k), int(i)) == int(i) for k, i in zip(bid, ids)) and len(first) == 10_000
        if kw > 1:
            assert np.array_equal(keys[0::2, :kw - 1][:2500], keys[1::2, :kw - 1][:2500]) and (keys[0:5000:2, kw - 1] != keys[1:5000:2, kw - 1]).all()
    d = J.by_name("occupancy_kb16_nullable").data()
    lo, hi = slice(0, 3000), slice(0, 20_000)
    wide = R.inner_pairs_dict(d.build_keys()[lo], d.build_valid()[lo], d.probe_keys[hi], d.probe_valid[hi])
    narrow = R.inner_pairs_dict(d.build_ids[lo].reshape(-1, 1), d.build_valid()[lo], d.probe_ids[hi].reshape(-1, 1), d.probe_valid[hi])
    assert same(wide, narrow) and len(wide[0]) > 50


def test_join_rows_and_bits_set_by_hand():
    bk = np.array([[5], [7], [5], [9], [7]], dtype=np.uint64)
    bv = np.array([1, 1, 1, 1, 0], dtype=bool)
    pk = np.array([[7], [5], [8], [5], [9]], dtype=np.uint64)
    pv = np.array([1, 1, 1, 0, 1], dtype=bool)
    rows = lambda kind: [tuple(int(x) for x in r) for r in zip(*R.join_rows(kind, bk, bv, pk, pv))]   # noqa: E731
    inner = [(0, 1), (1, 0), (1, 2), (4, 3)]
    assert rows("inner") == inner
    assert rows("left") == inner + [(2, -1), (3, -1)]
    assert rows("left_semi") == [(0, -1), (1, -1), (4, -1)]
    assert rows("left_anti") == [(2, -1), (3, -1)]
    assert rows("right") == inner + [(-1, 4)]
    assert rows("right_semi") == [(-1, 0), (-1, 1), (-1, 2), (-1, 3)]
    assert rows("right_anti") == [(-1, 4)]
    assert rows("full") == inner + [(2, -1), (3, -1), (-1, 4)]
    assert R.matched_build(R.inner_pairs(bk, bv, pk, pv), 5).tolist() == [True, True, True, True, False]
    assert R.bits_set([3, 3, 0, 9, 10, 0xFFFFFFFF], 10).tolist() == [True, False, False, True, False, False, False, False, False, True]
    assert R.bits_set([], 3).tolist() == [False] * 3


# ---- the tables have teeth --------------------------------------------------------------------------------------------------------------
def test_every_small_case_has_a_pair_and_a_row_without_a_partner():
    assert len(SMALL) == 78 + 3 + 3 + 48 + 12
    for c in SMALL + J.binary_cases():
        d = c.data()
        p, _ = R.inner_pairs(*d.ref_args())
        if c.name.startswith(J.NO_PAIRS):
            assert len(p) == 0, c                                              # empty by construction: all NULL, or no build row
            if "validity" in c.name or "all_null" in c.name:
                assert len(R.inner_pairs(d.build_keys(), None, d.probe_keys, None)[0]) > 0, c   # ... and only the validity makes it so
            continue
        assert len(p) > 0, c
        if d.n > 1:
            assert len(np.unique(p)) < d.n, c
        if d.probe_valid is not None and d.n > 2 and not d.probe_valid.all():   # a NULL probe row carries a key that would match
            assert R.matched_probe(d.build_keys(), d.build_valid(), d.probe_keys, None)[~d.probe_valid].any(), c


def test_sizes_and_multiplicities_are_the_ones_asked_for():
    assert sorted({c.data().n for c in J.sizes_cases()}) == [1, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
    for c in J.multiplicity_cases():
        d = c.data()
        p, b = R.inner_pairs(*d.ref_args())
        per_row = np.bincount(p, minlength=d.n)
        for tile in (per_row[:256], per_row[256:]):                            # each multiplicity in the full and in the ragged tile
            assert sorted(tile[tile > 0].tolist()) == [1, 2, 3, 254, 255, 256, 257, 511, 1000], c
        ends = np.cumsum(d.extra["block_rows"])
        for row in np.flatnonzero(per_row > 1):                                # one key's rows come from different blocks
            assert len(set(np.searchsorted(ends, b[p == row], side="right").tolist())) == min(int(per_row[row]), 3), c
    g = J.by_name("growth_kb8_expected0").data()
    assert [len(k) for k, _ in g.build_blocks] == [1, 1023, 1, 1024, 0, 3000, 70_000]


@pytest.mark.parametrize("case", J.single_bit_cases(), ids=repr)
def test_single_bit_holds_every_word_and_bit_as_a_hit_and_as_a_near_miss(case):
    d = case.data()
    hit = R.matched_probe(*d.ref_args())
    seen = {}
    for w, b, row, in_build in d.extra["flips"]:
        assert bool(hit[row]) == in_build
        seen.setdefault((w, b), set()).add(bool(hit[row]))
        near = d.probe_keys[row].copy()
        near[w] ^= np.uint64(1 << b)
        assert any((near == k).all() for k in d.build_keys())                  # one bit away from a key of the build side
    assert seen == {(w, b): {True, False} for w in range(d.kw) for b in J.BITS}
    assert d.nb <= 512 and d.n > 256
    word0 = set(d.probe_keys[:, 0].tolist())
    assert set(J.WORD0) <= word0 and {1 << 20, (1 << 20) + 64, (1 << 20) + 128} <= word0


def test_thresholds_of_the_long_blocks():
    """the sizes are the ones of the issue; the thresholds restate dbhip_join_probe and join_count_block (tests/join_cases.py)"""
    assert J.count_steps(16_384 * 256 + 255) == 1 and J.count_steps(16_385 * 256) == 2 and J.count_steps(J.LONG_COUNT_N) == 2
    assert J.emit_group(32_767 * 256) == 1 and J.emit_group(32_767 * 256 + 1) == 2 and J.emit_group(J.LONG_G2_N) == 2
    assert J.emit_group(65_535 * 256) == 2 and J.emit_group(65_535 * 256 + 1) == 4 and J.emit_group(J.LONG_G4_N) == 4
    assert J.emit_group(J.LONG_COUNT_N) == 1 and J.LONG_COUNT_N % 256 == 5
    assert (J.LONG_COUNT_N, J.LONG_G2_N, J.LONG_G4_N) == (4_195_333, 8_388_869, 16_777_477)


@pytest.mark.parametrize("n", [J.LONG_COUNT_N, J.LONG_G2_N, J.LONG_G4_N])
def test_long_blocks_are_selective_with_empty_groups_and_gaps(n):
    d = J.by_name(f"long_n{n}_kb8").data()
    p, b = R.inner_pairs_fast(*d.ref_args())
    ntiles = -(-n // J.TILE)
    per_tile = np.bincount(p // J.TILE, minlength=ntiles)
    assert 0.005 < (per_tile > 0).mean() < 0.02                               # the pairs sit in about 1 % of the tiles
    assert (per_tile[[0, 1, 2, 3, 16_384, 16_385, 16_386, 16_387, ntiles - 1]] > 0).all()   # both steps of the first waves, the ragged tile
    per_row = np.bincount(p, minlength=n)
    assert {2, 3, 255, 300} <= set(np.unique(per_row).tolist())
    assert {2, 3, 255, 300} <= set(np.unique(per_row[16_384 * 256:16_388 * 256]).tolist()) | set(np.unique(per_row[:1024]).tolist())
    assert (~d.probe_valid[:1024]).any() and (~d.probe_valid[16_384 * 256:16_388 * 256]).any() and len(np.unique(p)) < n
    g = J.emit_group(n)
    todo = np.zeros(-(-ntiles // g) * g, dtype=bool)
    todo[:ntiles] = per_tile > 0
    todo = todo.reshape(-1, g)
    assert (~todo.any(axis=1)).any()                                           # a group of tiles with nothing to emit
    if g > 1:
        some = todo.any(axis=1) & ~todo.all(axis=1)
        assert some.any()                                                      # a group with gaps
        assert (todo[:, -1] & ~todo[:, 0]).any() and (todo[:, 0] & ~todo[:, -1]).any()
    if g == 4:
        assert (todo[:, 0] & ~todo[:, 2] & todo[:, 3]).any()                   # a gap between two tiles that have pairs
    if n == J.LONG_COUNT_N:                                                    # the same ids for every key width
        for kb in (16, 32):
            w = J.by_name(f"long_n{n}_kb{kb}")
            assert w.key_bytes == kb
    # the dictionary form agrees on the rows that can match at all
    rows = np.flatnonzero(d.probe_ids < (1 << 32))
    sub = R.inner_pairs_dict(d.build_ids.reshape(-1, 1), d.build_valid(), d.probe_ids[rows].reshape(-1, 1), d.probe_valid[rows])
    assert np.array_equal(rows[sub[0]], p) and np.array_equal(sub[1], b)


def test_occupancy_cases_build_the_filter_and_join_ids():
    for c in J.occupancy_cases():
        d = c.data()
        assert d.nb == 270_000 and d.n == 300_077 and 2 * d.nb > (1 << 19) and c.key_bytes in (16, 32)
        p, _ = R.inner_pairs(*d.ref_args())
        assert len(p) > 50_000 and len(np.unique(p)) < d.n // 2
        odd = (d.probe_ids & np.uint64(1)) == 1
        assert odd.sum() > 100_000 and not np.isin(np.flatnonzero(odd), p).any()   # the odd twins are near misses
        assert np.array_equal(d.probe_keys[:50], J.widen(d.probe_ids[:50], d.kw))


# ---- the tables reject wrong joins ------------------------------------------------------------------------------------------------------
def _per_row(pairs, keep):
    """the pairs with each probe row's run cut or reordered by keep(run of build rows) -> build rows"""
    p, b = pairs
    op, ob = [], []
    for row in np.unique(p):
        run = keep(b[p == row])
        op += [row] * len(run)
        ob += list(run)
    return np.asarray(op, np.uint32), np.asarray(ob, np.uint32)


def defective(defect, d):
    bk, bv, pk, pv = d.build_keys(), d.build_valid(), d.probe_keys, d.probe_valid
    right = R.inner_pairs_dict(bk, bv, pk, pv)
    if defect == "word0_only":
        return R.inner_pairs_dict(bk, bv, pk, pv, key=lambda r: r[0])
    if defect == "low32_only":
        return R.inner_pairs_dict(bk, bv, pk, pv, key=lambda r: tuple(w & 0xFFFFFFFF for w in r))
    if defect == "last_word_ignored":
        return R.inner_pairs_dict(bk, bv, pk, pv, key=lambda r: r[:-1])
    if defect == "nulls_match":
        return R.inner_pairs_dict(bk, None, pk, None)
    if defect == "count_wraps_256":
        return _per_row(right, lambda run: run[:len(run) % 256])
    if defect == "count_stuck_255":
        return _per_row(right, lambda run: run[:255])
    if defect == "ragged_tile_lost":
        keep = right[0] < (d.n // 256) * 256
        return right[0][keep], right[1][keep]
    if defect == "nibbles_swapped":
        swapped = None if pv is None else np.concatenate([pv, np.zeros(-len(pv) % 8, bool)])[np.arange(len(pv)) ^ 4]
        return R.inner_pairs_dict(bk, bv, pk, swapped)
    if defect == "chain_order":
        return _per_row(right, lambda run: run[::-1])
    if defect == "first_block_only":
        keep = right[1] < d.extra.get("block0_rows", len(d.build_blocks[0][0]))
        return right[0][keep], right[1][keep]
    raise KeyError(defect)


DEFECTS = [("word0_only", "single_bit_kb16"), ("low32_only", "single_bit_kb8"), ("last_word_ignored", "sizes_n257_kb32_plain"),
           ("nulls_match", "validity_probe_0x55_kb8"), ("count_wraps_256", "multiplicity_kb8"), ("count_stuck_255", "multiplicity_kb16"),
           ("ragged_tile_lost", "sizes_n513_kb8_plain"), ("nibbles_swapped", "validity_probe_0x0F_kb8"), ("chain_order", "multiplicity_kb32"),
           ("first_block_only", "growth_kb8_expected0")]


def test_case_tables_reject_every_listed_defect():
    rejected = 0
    for defect, name in DEFECTS:
        d = J.by_name(name).data()
        right = R.inner_pairs_dict(d.build_keys(), d.build_valid(), d.probe_keys, d.probe_valid)
        wrong = defective(defect, d)
        assert not same(wrong, right), (defect, name)
        rejected += 1
    assert rejected == 10
    assert all(name in __doc__ and defect in __doc__ for defect, name in DEFECTS)


def test_defects_are_invisible_where_they_do_not_apply():
    """the defect models themselves: each leaves a case alone that has nothing for it to get wrong"""
    d = J.by_name("sizes_n256_kb8_plain").data()
    right = R.inner_pairs_dict(d.build_keys(), d.build_valid(), d.probe_keys, d.probe_valid)
    for defect in ("word0_only", "nulls_match", "count_wraps_256", "count_stuck_255", "ragged_tile_lost", "nibbles_swapped", "first_block_only"):
        assert same(defective(defect, d), right), defect
