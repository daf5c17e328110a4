"""CPU: tests/sort_ref.py — the plain statement of the sort order that tests/test_gpu_sort_edges.py holds the device to — checked three
ways. Its comparator, its vectorised twin and the C oracle (orc_sort_perm / orc_sort_bound_partition, written independently) agree
exactly on every small case of the shared case lists; permutations made by nine deliberately wrong orderings are told apart from the
right one on named cases of those lists, which shows that the cases can see such mistakes at all; and a few tiny cases with the
expected permutation written out by hand anchor the comparator to something no code shares."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from databend_amd.device import make_views_general, pack_bits
from tests import oracle_lib as O
from tests import sort_ref as R

TYPE_OF = {"bool": T.T_BOOL, "i8": T.T_I8, "i16": T.T_I16, "i32": T.T_I32, "i64": T.T_I64, "u8": T.T_U8, "u16": T.T_U16, "u32": T.T_U32,
           "u64": T.T_U64, "f32": T.T_F32, "f64": T.T_F64, "date": T.T_DATE, "ts": T.T_TIMESTAMP, "dec64": T.T_DEC64, "dec128": T.T_DEC128,
           "str": T.T_STRING, "lstr": T.T_STRING}

SORT_CASES = R.sort_cases()
PART_CASES = R.partition_cases()
BY_NAME = {c.name: c for c in SORT_CASES + PART_CASES}


def host_col(c):
    t = TYPE_OF[c.kind]
    if c.kind == "bool":
        return O.HostCol(t, pack_bits(c.values), c.valid)
    if c.kind == "dec128":
        return O.HostCol(t, O.i128_array(c.values), c.valid, 38, 0)
    if c.kind in R.STRING_KINDS:
        views, buf = make_views_general(c.values)
        return O.HostCol(t, views, c.valid, buffers=[buf])
    return O.HostCol(t, c.values, c.valid)


def u8s(xs):
    return (C.c_uint8 * len(xs))(*[int(x) for x in xs])


def oracle_sort(oracle, cols, desc, nf, limit=0):
    n = cols[0].n
    m = limit if 0 < limit < n else n
    out = np.zeros(max(m, 1), np.uint32)
    hcols = [host_col(c) for c in cols]           # (kept alive over the call: the OCol array holds bare pointers into them)
    assert oracle.orc_sort_perm(O.cols(hcols), u8s(desc), u8s(nf), len(cols), C.c_int64(n), C.c_int64(limit), out.ctypes.data_as(C.c_void_p)) == 0
    return out[:m]


def oracle_partition(oracle, rows, bounds, desc, nf):
    n, nb = rows[0].n, bounds[0].n if bounds else 0
    part, counts = np.zeros(max(n, 1), np.uint32), np.zeros(nb + 1, np.uint64)
    hrows, hbounds = [host_col(c) for c in rows], [host_col(c) for c in bounds]
    assert oracle.orc_sort_bound_partition(O.cols(hrows), O.cols(hbounds) if nb else None, u8s(desc), u8s(nf),
                                           len(rows), C.c_int64(n), C.c_int64(nb), part.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)) == 0
    return part[:n], counts


# ---- comparator == twin == oracle -------------------------------------------------------------------------------------------------------
def check_sort_case(oracle, case):
    cols = case.cols()
    for desc, nf, limit in case.orders:
        exp = R.sort_perm(cols, desc, nf, limit)
        assert R.explain(cols, desc, nf, R.sort_perm_fast(cols, desc, nf, limit), exp) == "", (case, desc, nf, limit, "twin")
        assert R.explain(cols, desc, nf, oracle_sort(oracle, cols, desc, nf, limit), exp) == "", (case, desc, nf, limit, "oracle")


@pytest.mark.parametrize("kind", R.ALL_KINDS)
def test_single_key_cases_comparator_twin_and_oracle_agree(oracle, kind):
    cases = [c for c in R.single_key_cases() if c.n <= R.SMALL and c.keys[0][0] == kind]
    assert len(cases) == 2 * (len(R.SIZES) - 1)
    for case in cases:
        check_sort_case(oracle, case)


@pytest.mark.parametrize("case", [c for c in R.multi_key_cases() if c.n <= R.SMALL], ids=repr)
def test_multi_key_cases_comparator_twin_and_oracle_agree(oracle, case):
    check_sort_case(oracle, case)


def test_the_multi_key_list_is_not_empty_and_the_builder_is_seeded():
    multi = [c for c in R.multi_key_cases() if c.n <= R.SMALL]
    assert len(multi) >= 30
    a, b = BY_NAME["eight-all-nullable-n65"].cols(), BY_NAME["eight-all-nullable-n65"].cols()
    for x, y in zip(a, b):
        assert x.py() == y.py() or x.kind in R.FLOAT_KINDS and np.array_equal(np.asarray(x.values).view(np.uint8), np.asarray(y.values).view(np.uint8))
        assert np.array_equal(x.valid, y.valid)
    assert len(a) == 8 and all(c.valid is not None and 0 < c.valid.sum() < c.n for c in a)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_float_pool_holds_what_it_promises(dtype):
    c = R.make_col(np.random.default_rng(5), 4097, "f32" if dtype == np.float32 else "f64")
    v = np.asarray(c.values)
    bits = v.view(np.uint32 if dtype == np.float32 else np.uint64)
    sign = bits >> (31 if dtype == np.float32 else 63)
    tiny = np.finfo(dtype).smallest_normal
    assert (np.isnan(v) & (sign == 1)).any() and (np.isnan(v) & (sign == 0)).any() and len(set(bits[np.isnan(v)].tolist())) >= 5
    assert ((v == 0) & (sign == 1)).any() and ((v == 0) & (sign == 0)).any()
    assert ((np.abs(v) < tiny) & (v != 0)).sum() > 100 and (v == tiny).any() and (v == -tiny).any()
    assert np.isposinf(v).any() and np.isneginf(v).any() and (v == np.finfo(dtype).max).any() and (v == np.finfo(dtype).min).any()


@pytest.mark.parametrize("case", PART_CASES, ids=repr)
def test_partition_cases_comparator_twin_and_oracle_agree(oracle, case):
    rows = case.rows()
    for desc, nf in case.orders:
        bounds = case.bounds(desc, nf)
        part, counts = R.bound_partition(rows, bounds, desc, nf)
        fpart, fcounts = R.bound_partition_fast(rows, bounds, desc, nf)
        assert np.array_equal(part, fpart) and np.array_equal(counts, fcounts), (case, desc, nf, "twin")
        opart, ocounts = oracle_partition(oracle, rows, bounds, desc, nf)
        assert np.array_equal(part, opart) and np.array_equal(counts, ocounts), (case, desc, nf, "oracle")
        assert int(counts.sum()) == case.n and len(counts) == case.nb + 1


@pytest.mark.parametrize("keyset", sorted(R.MERGE_KEYSETS))
@pytest.mark.parametrize("nruns", [0, 1, 2, 8, 33])
def test_merge_cases_are_sorted_runs_and_the_merge_is_the_sort(oracle, keyset, nruns):
    keys, desc, nf = R.MERGE_KEYSETS[keyset]
    cols, offs = R.merge_runs(70 + nruns, 3000, nruns, keys, desc, nf)
    assert len(offs) == nruns + 1 and offs[0] == 0 and all(a <= b for a, b in zip(offs[:-1], offs[1:]))
    if nruns >= 8:
        assert offs[0] == offs[1] and offs[-2] == offs[-1] and offs[nruns // 2] == offs[nruns // 2 + 1]
    for lo, hi in zip(offs[:-1], offs[1:]):       # every run is in order already
        assert np.array_equal(R.sort_perm([c.rows(lo, hi) for c in cols], desc, nf), np.arange(hi - lo))
    if nruns:
        for limit in (0, 25, 3000):
            exp = R.merge_perm(cols, offs, desc, nf, limit)
            assert np.array_equal(exp, R.sort_perm_fast(cols, desc, nf, limit)) and np.array_equal(exp, oracle_sort(oracle, cols, desc, nf, limit))


# ---- the cases reject wrong orderings ---------------------------------------------------------------------------------------------------
def wrong_perms(case_name, mutate):
    """for every order of the case: (the reference's permutation, the permutation of the mutated ordering)"""
    case = BY_NAME[case_name]
    cols = case.cols()
    return [(cols, desc, nf, R.sort_perm_fast(cols, desc, nf, limit), mutate(cols, desc, nf, limit)) for desc, nf, limit in case.orders]


def assert_rejected(case_name, mutate, what="key sequence differs"):
    found = [R.explain(cols, desc, nf, got, exp) for cols, desc, nf, exp, got in wrong_perms(case_name, mutate)]
    assert any(what in f for f in found), (case_name, found)


def with_col0(fn):
    """a mutant that sorts by the reference's rules after replacing key 0 by fn(key 0)"""
    return lambda cols, desc, nf, limit: R.sort_perm_fast([fn(cols[0])] + cols[1:], desc, nf, limit)


def ordered_bits(c):
    """floats -> the unsigned integer whose order is the order of the RAW bit patterns read as sign and magnitude"""
    v = np.asarray(c.values)
    wide = v.dtype == np.float64
    b = v.view(np.uint64 if wide else np.uint32).astype(np.uint64)
    top = np.uint64(1 << (63 if wide else 31))
    mask = np.uint64((1 << (64 if wide else 32)) - 1)
    return R.KeyCol("u64", np.where(b & top != 0, ~b & mask, b | top), c.valid)


@pytest.mark.parametrize("case", ["f32-n4097-plain", "f64-then-int-n4097", "f64-behind-low-key-n65"])
def test_rejects_the_ieee_less_than_on_floats(case):
    def mutate(cols, desc, nf, limit):
        import functools
        pys = [c.py() for c in cols]

        def cmp(i, j):
            for k, c in enumerate(cols):
                va, vb = c.valid is None or c.valid[i], c.valid is None or c.valid[j]
                if not va or not vb:
                    if va != vb:
                        return -1 if (nf[k] if not va else not nf[k]) else 1
                    continue
                r = (pys[k][i] > pys[k][j]) - (pys[k][i] < pys[k][j])      # NaN: unordered, reads as a tie with everything
                if r:
                    return -r if desc[k] else r
            return i - j
        return np.array(sorted(range(cols[0].n), key=functools.cmp_to_key(cmp)), dtype=np.uint32)
    assert_rejected(case, mutate)


@pytest.mark.parametrize("case", ["f32-n65-plain", "f64-n4097-nullable", "f32-zero-and-nan-ties-n65", "f64-zero-and-nan-ties-n4097"])
def test_rejects_floats_ordered_by_their_raw_bits(case):
    assert_rejected(case, with_col0(ordered_bits))


@pytest.mark.parametrize("case", ["f32-n4097-plain", "f64-n65-nullable", "f32-then-int-n4097"])
def test_rejects_subnormals_flushed_to_zero(case):
    def flush(c):
        v = np.asarray(c.values).copy()
        v[np.abs(v) < np.finfo(v.dtype).smallest_normal] = 0
        return R.KeyCol(c.kind, v, c.valid)
    assert_rejected(case, with_col0(flush))


@pytest.mark.parametrize("case", ["i16-n65-nullable", "lstr-n4097-nullable", "two-nullable-n65", "nulls-on-key3-only-n4097"])
def test_rejects_null_placement_that_flips_with_desc(case):
    assert_rejected(case, lambda cols, desc, nf, limit: R.sort_perm_fast(cols, desc, [f ^ d for f, d in zip(nf, desc)], limit))


@pytest.mark.parametrize("case", ["str-n65-plain", "lstr-n4097-nullable", "two-strings-n65"])
def test_rejects_strings_compared_by_length_then_bytes(case):
    assert_rejected(case, with_col0(lambda c: R.KeyCol(c.kind, [len(s).to_bytes(2, "big") + s for s in c.values], c.valid)))


@pytest.mark.parametrize("case", ["lstr-n65-plain", "lstr-n4097-nullable"])
def test_rejects_strings_compared_on_their_inline_bytes_only(case):
    assert_rejected(case, with_col0(lambda c: R.KeyCol(c.kind, [s[:12] for s in c.values], c.valid)))


@pytest.mark.parametrize("case", ["i16-n65-plain", "i16-n4097-nullable", "two-nullable-n65"])
def test_rejects_a_signed_16_bit_key_compared_unsigned(case):
    assert_rejected(case, with_col0(lambda c: R.KeyCol("u16", np.asarray(c.values).view(np.uint16), c.valid)))


@pytest.mark.parametrize("case", ["u8-n65-plain", "bool-n4097-nullable", "three-n4097", "later-key-all-null-n4097"])
def test_rejects_an_unstable_tie_order(case):
    def mutate(cols, desc, nf, limit):
        n = cols[0].n
        ranks = R.rank_keys(cols, desc, nf)
        order = np.lexsort([-np.arange(n)] + [ranks[k] for k in range(len(cols) - 1, -1, -1)]).astype(np.uint32)     # ties by DEscending row id
        return order[:limit] if 0 < limit < n else order
    assert_rejected(case, mutate, what="same key sequence, different tie order")


@pytest.mark.parametrize("case", ["duplicate-bounds", "negative-zero-bound", "nan-bound", "null-bound", "one-plain-key-nb63", "three-keys-nulls-on-2-and-3-nb64"])
def test_rejects_a_partition_that_counts_bounds_up_to_and_including_the_row(case):
    pc = BY_NAME[case]
    rows = pc.rows()
    differs = False
    for desc, nf in pc.orders:
        bounds = pc.bounds(desc, nf)
        nb = bounds[0].n
        wrong = np.array([sum(1 for p in range(nb) if R.compare_rows(bounds, p, rows, i, desc, nf) <= 0) for i in range(0, rows[0].n, 7)], np.uint32)
        differs |= not np.array_equal(wrong, R.bound_partition_fast(rows, bounds, desc, nf)[0][::7])
    assert differs


# ---- hand-checked anchors ---------------------------------------------------------------------------------------------------------------
NAN = float("nan")


def test_hand_checked_nan_and_zero_ties_with_a_second_key():
    #                 row:   0     1     2    3     4    5     6            7
    f = np.array([NAN, 0.0, -0.0, 1.0, -NAN, -1.0, 0.0, np.float32(1e-45)], dtype=np.float32)
    k = np.array([5, 3, 1, 0, 2, 0, 2, 9], dtype=np.int32)
    cols = [R.KeyCol("f32", f), R.KeyCol("i32", k)]
    # asc: -1 | the zeros by k: row 2 (k 1), row 6 (k 2), row 1 (k 3) | the subnormal | 1 | the NaNs by k: row 4 (k 2), row 0 (k 5)
    assert R.sort_perm(cols, [0, 0], [0, 0]).tolist() == [5, 2, 6, 1, 7, 3, 4, 0]
    # desc on the float, k still ascending inside the ties: NaNs first
    assert R.sort_perm(cols, [1, 0], [0, 0]).tolist() == [4, 0, 3, 7, 2, 6, 1, 5]
    # float asc, k desc
    assert R.sort_perm(cols, [0, 1], [0, 0]).tolist() == [5, 1, 6, 2, 7, 3, 0, 4]
    assert R.sort_perm(cols, [0, 0], [0, 0], limit=3).tolist() == [5, 2, 6]
    for d in ([0, 0], [1, 0], [0, 1]):
        assert np.array_equal(R.sort_perm_fast(cols, d, [0, 0]), R.sort_perm(cols, d, [0, 0]))


def test_hand_checked_nulls_first_and_last_under_both_directions():
    #                row:  0   1  2   3  4   5
    v = np.array([3, 1, 2, 1, 9, 2], dtype=np.int64)
    valid = np.array([1, 1, 0, 1, 0, 1], bool)        # rows 2 and 4 are NULL; what lies under them (2 and 9) never shows
    cols = [R.KeyCol("i64", v, valid)]
    assert R.sort_perm(cols, [0], [0]).tolist() == [1, 3, 5, 0, 2, 4]       # asc, NULLs last
    assert R.sort_perm(cols, [0], [1]).tolist() == [2, 4, 1, 3, 5, 0]       # asc, NULLs first
    assert R.sort_perm(cols, [1], [0]).tolist() == [0, 5, 1, 3, 2, 4]       # desc, NULLs STILL last
    assert R.sort_perm(cols, [1], [1]).tolist() == [2, 4, 0, 5, 1, 3]       # desc, NULLs STILL first
    for d in (0, 1):
        for f in (0, 1):
            assert np.array_equal(R.sort_perm_fast(cols, [d], [f]), R.sort_perm(cols, [d], [f]))
    # as bounds [1, 2, NULL] (asc, NULLs last): partition = bounds strictly before the row
    bounds = [R.KeyCol("i64", np.array([1, 2, 0], dtype=np.int64), np.array([1, 1, 0], bool))]
    part, counts = R.bound_partition(cols, bounds, [0], [0])
    assert part.tolist() == [2, 0, 2, 0, 2, 1] and counts.tolist() == [2, 1, 3, 0]
    assert R.bound_partition_fast(cols, bounds, [0], [0])[0].tolist() == part.tolist()


def test_hand_checked_prefix_strings():
    #       row: 0     1      2          3    4              5               6              7
    s = [b"ab", b"a", b"a\x00", b"", b"abcdefghijkl", b"abcdefghijklm", b"abcdefghijk", b"b"]
    cols = [R.KeyCol("lstr", s)]
    assert R.sort_perm(cols, [0], [0]).tolist() == [3, 1, 2, 0, 6, 4, 5, 7]
    assert R.sort_perm(cols, [1], [0]).tolist() == [7, 5, 4, 6, 0, 2, 1, 3]
    assert R.sort_perm_fast(cols, [0], [0]).tolist() == [3, 1, 2, 0, 6, 4, 5, 7]
