"""GPU: dbhip_sort_perm (with its LIMIT radix select and its onesweep passes), dbhip_merge_sorted_perm and dbhip_sort_bound_partition
at the edges of their contract — NULLs on every key position, up to eight keys, every key type, NaN payloads / signed zeros / subnormals
/ +-MAX / +-Inf, strings around the 12 inline bytes and at the 4096-byte maximum, sliced columns, both sides of every size switch in
k_sort.hip, and the shapes that must be refused. Every result is asserted exactly (the whole permutation, or the partition of every
row plus the counts) against tests/sort_ref.py — plain Python, never another device path; tests/test_sort_ref_cpu.py checks that
reference against the C oracle and shows that these cases reject nine wrong orderings. A failure says whether the key sequence differs
(the contract is broken) or only the order of ties (stability is broken)."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import _lib as T
from tests import sort_ref as R

pytestmark = pytest.mark.gpu

TYPE_OF = {"bool": T.T_BOOL, "i8": T.T_I8, "i16": T.T_I16, "i32": T.T_I32, "i64": T.T_I64, "u8": T.T_U8, "u16": T.T_U16, "u32": T.T_U32,
           "u64": T.T_U64, "f32": T.T_F32, "f64": T.T_F64, "date": T.T_DATE, "ts": T.T_TIMESTAMP, "dec64": T.T_DEC64, "dec128": T.T_DEC128,
           "str": T.T_STRING, "lstr": T.T_STRING}


def to_gpu(gpu, c):
    if c.kind == "bool":
        return gpu.Column.boolean(c.values, validity=c.valid)
    if c.kind == "dec128":
        return gpu.Column.decimal128(c.values, 38, 0, validity=c.valid)
    if c.kind in R.STRING_KINDS:
        return gpu.Column.strings(c.values, validity=c.valid)
    return gpu.Column.from_numpy(c.values, TYPE_OF[c.kind], validity=c.valid, precision=18 if c.kind == "dec64" else 0)


def to_gpu_sliced(gpu, c, seed):
    """the column as rows [13, 13 + n) of a column of n + 77 rows: value buffers by address, the validity Bitmap by bit offset"""
    rng = np.random.default_rng(seed)
    head, tail = R.make_col(rng, 13, c.kind, c.valid is not None), R.make_col(rng, 64, c.kind, c.valid is not None)
    whole = to_gpu(gpu, R.concat(R.concat(head, c), tail))
    assert whole.n == c.n + 77
    s = whole.slice(13, 13 + c.n)
    assert s.voff == 13
    return s


def reference(cols, desc, nf, limit=0):
    return (R.sort_perm if cols[0].n <= 65 else R.sort_perm_fast)(cols, desc, nf, limit)


def check_sort(gpu, cols, gcols, desc, nf, limit=0, what=""):
    exp = reference(cols, desc, nf, limit)
    got = gpu.sort_perm(gcols, desc, nf, limit)
    why = R.explain(cols, desc, nf, got, exp)
    assert why == "", (what, desc, nf, limit, why)


def check_case(gpu, case):
    cols = case.cols()
    gcols = [to_gpu(gpu, c) for c in cols]
    for desc, nf, limit in case.orders:
        check_sort(gpu, cols, gcols, desc, nf, limit, case.name)


# ---- dbhip_sort_perm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("kind", R.ALL_KINDS)
def test_single_key(gpu, kind, n):
    """one key of every type: plain asc / desc, nullable asc / desc x NULLs first / last; the sizes sit on both sides of the wave, the 4096-key
    scratch tile and the 8192-key pass tile"""
    cases = [c for c in R.single_key_cases() if c.n == n and c.keys[0][0] == kind]
    assert len(cases) == 2
    for case in cases:
        check_case(gpu, case)


@pytest.mark.parametrize("case", R.multi_key_cases(), ids=repr)
def test_multi_key(gpu, case):
    """2, 3, 5 and 8 keys of mixed types behind low-cardinality leading keys; NULLs on every key position, on one later key only, on all eight;
    a later key that is entirely NULL or constant; floats from the pool in front of and behind another key"""
    check_case(gpu, case)


@pytest.mark.parametrize("n", [1, 1000, 70_001])
@pytest.mark.parametrize("keys", [[("i32", True, "pool")], [("f64", True, "pool")], [("lstr", True, "pool")], [("str", True, "pool")],
                                  [("u8", True, "low"), ("f32", True, "pool"), ("lstr", True, "pool"), ("dec128", True, "pool")]], ids=lambda k: "+".join(x[0] for x in k))
def test_sliced_columns(gpu, keys, n):
    """Column.slice(13, 13 + n) of n + 77 rows: a validity bit offset that is no multiple of 8 or 64 on every key"""
    cols = R.make_cols(90, n, keys)
    gcols = [to_gpu_sliced(gpu, c, 91 + i) for i, c in enumerate(cols)]
    nk = len(keys)
    for desc, nf, limit in [([0] * nk, [0] * nk, 0), ([1] * nk, [1] * nk, 0), ([1] * nk, [0] * nk, 9)]:
        check_sort(gpu, cols, gcols, desc, nf, limit, "sliced")


@pytest.mark.parametrize("nullable", [False, True], ids=["plain", "nullable"])
def test_strings_of_4095_and_4096_bytes(gpu, nullable):
    """the longest value the sort takes (513 key images per value): values that share their first 4088 bytes and differ in the last ones or
    in the length only, mixed with short ones"""
    rng = np.random.default_rng(4096)
    base = bytes(rng.integers(0, 256, 4088, dtype=np.uint8))
    tails = [b"aaaaaaaa", b"aaaaaaab", b"aaaaaaa", b"baaaaaaa", b"\x00" * 8, b"\x00" * 7, b"\xff" * 8, b"\xff" * 7, b""]
    pool = [base + t for t in tails] + R.LONG_POOL
    vals = [pool[i] for i in rng.integers(0, len(pool), 300).tolist()]
    assert max(len(v) for v in vals) == 4096
    cols = [R.KeyCol("lstr", vals, rng.random(300) < 0.8 if nullable else None), R.KeyCol("i16", rng.integers(-2, 3, 300).astype(np.int16))]
    gcols = [to_gpu(gpu, c) for c in cols]
    for desc, nf in [([0, 0], [0, 0]), ([1, 0], [1, 0]), ([1, 1], [0, 0])]:
        check_sort(gpu, cols, gcols, desc, nf, 0, "4096-byte strings")
    check_sort(gpu, cols[:1], gcols[:1], [0], [1], 0, "4096-byte strings alone")


def raw_sort(gpu, gcols, nkeys, n):
    """dbhip_sort_perm called directly -> (status, the output buffer as it was left); the buffer is filled with 0xFF first"""
    from databend_amd.device import DeviceBuffer, _cols
    out = DeviceBuffer(max(n, 1) * 4)
    T.check(T.lib().dbhip_memset(C.c_void_p(out.ptr), 0xFF, C.c_size_t(max(n, 1) * 4), None))
    z = (C.c_uint8 * max(len(gcols), 1))()
    rc = T.lib().dbhip_sort_perm(_cols(gcols), z, z, nkeys, C.c_int64(n), C.c_int64(0), C.c_void_p(out.ptr), None)
    return rc, out.to_numpy(np.uint32, n)


def test_refusals_return_an_error_and_the_stream_sorts_on(gpu):
    """what the sort does not take is an error code with a message — never a crash, never a permutation of zeros — and the next valid
    call on the same stream is right"""
    n = 500
    ok = R.make_cols(7, n, [("i32", True, "pool"), ("lstr", True, "pool")])
    gok = [to_gpu(gpu, c) for c in ok]

    def still_sorts():
        check_sort(gpu, ok, gok, [1, 0], [0, 1], 0, "after a refusal")

    ints = [int(x) for x in np.random.default_rng(1).integers(-9, 9, n)]
    refused = {
        "a Decimal256 key": ([gok[0], gpu.Column.decimal256(ints, 76, 0)], T.ERR_UNSUPPORTED),
        "a Decimal256 key alone": ([gpu.Column.decimal256(ints, 76, 0)], T.ERR_UNSUPPORTED),
        "a scalar key": ([gok[0], gpu.Column.scalar(5, T.T_I64)], T.ERR_UNSUPPORTED),
        "a 4097-byte string": ([gpu.Column.strings([b"x" * 4097 if i == 250 else b"abc" for i in range(n)])], T.ERR_UNSUPPORTED),
    }
    nobuf = gpu.Column.strings([b"long enough to leave the view" if i % 3 == 0 else b"short" for i in range(n)])
    nobuf.buffers, nobuf.n_buffers = None, 0
    refused["long strings without data buffers"] = ([nobuf], T.ERR_INVALID)
    for what, (gcols, code) in refused.items():
        rc, out = raw_sort(gpu, gcols, len(gcols), n)
        assert rc == code, (what, rc)
        assert T.lib().dbhip_last_error().decode() != "", what
        assert (out == 0xFFFFFFFF).all(), (what, "the output was written")
        with pytest.raises(T.DbhipError):
            gpu.sort_perm(gcols)
        still_sorts()
    nine = [gok[0]] * 9
    for nkeys in (0, 9):
        rc, out = raw_sort(gpu, nine, nkeys, n)
        assert rc == T.ERR_INVALID and (out == 0xFFFFFFFF).all(), nkeys
        still_sorts()
    # the same shapes as rows or bounds of the range partition
    b = [gpu.Column.from_numpy(np.array([0, 5], np.int32), validity=np.array([True, True]))]
    for what, gcols, gb in [("Decimal256", [gpu.Column.decimal256(ints, 76, 0)], [gpu.Column.decimal256([0, 1], 76, 0)]),
                            ("a scalar bound", [gok[0]], [gpu.Column.scalar(5, T.T_I32)]),
                            ("a bound of another type", [gok[0]], [gpu.Column.from_numpy(np.array([0, 5], np.int64))]),
                            ("a 4097-byte bound", [gok[1]], [gpu.Column.strings([b"a", b"x" * 4097])]),
                            ("long rows, no buffers", [nobuf], [gpu.Column.strings([b"a", b"b"])])]:
        with pytest.raises(T.DbhipError) as e:
            gpu.sort_bound_partition(gcols, gb)
        assert e.value.code in (T.ERR_UNSUPPORTED, T.ERR_INVALID), what
        part, counts = gpu.sort_bound_partition([gok[0]], b)
        exp, ecounts = R.bound_partition_fast(ok[:1], [R.KeyCol("i32", np.array([0, 5], np.int32), np.array([True, True]))], [0], [0])
        assert np.array_equal(part.to_numpy(np.uint32, n), exp) and np.array_equal(counts, ecounts), what


# ---- LIMIT: the radix select on the first key --------------------------------------------------------------------------------------------
def limit_cols(seed, n, first, nullable_first=False):
    return R.make_cols(seed, n, [(first, nullable_first, "pool"), ("i16", True, "pool")])


@pytest.mark.parametrize("n,limit", [(65535, 10), (65536, 10), (65536, 16383), (65536, 16384), (65536, 1), (65536, 65535), (65536, 65536), (65536, 65537)])
def test_limit_on_both_sides_of_the_select(gpu, n, limit):
    """the select runs for n >= 65536 and limit * 4 < n; the answer is the first `limit` rows of the full stable sort either way"""
    for first in ("i64", "f32"):
        cols = limit_cols(n + limit, n, first)
        gcols = [to_gpu(gpu, c) for c in cols]
        for desc, nf in [([0, 0], [0, 0]), ([1, 1], [0, 1])]:
            check_sort(gpu, cols, gcols, desc, nf, limit, f"limit {first}")


@pytest.mark.parametrize("kind", R.ALL_KINDS)
def test_limit_with_every_type_as_the_first_key(gpu, kind):
    n = 70_001
    cols = limit_cols(100, n, kind)
    gcols = [to_gpu(gpu, c) for c in cols]
    for desc, nf, limit in [([0, 0], [0, 0], 100), ([1, 0], [0, 1], 100), ([1, 1], [0, 0], 9000), ([0, 1], [0, 0], 3)]:
        check_sort(gpu, cols, gcols, desc, nf, limit, f"limit {kind}")


@pytest.mark.parametrize("kind", ["i32", "f64", "lstr"])
def test_limit_with_a_nullable_first_key_takes_the_full_sort(gpu, kind):
    n = 65_600
    cols = limit_cols(101, n, kind, nullable_first=True)
    gcols = [to_gpu(gpu, c) for c in cols]
    for desc, nf in [([0, 0], [0, 0]), ([0, 0], [1, 1]), ([1, 0], [1, 0])]:
        check_sort(gpu, cols, gcols, desc, nf, 10, f"limit nullable {kind}")


def test_limit_with_a_constant_first_key(gpu):
    """no byte of the first key's image varies: nothing to select on, the later keys order everything"""
    n = 70_001
    for kind in ("i32", "f64", "str"):
        cols = R.make_cols(102, n, [(kind, False, "const"), ("f32", True, "pool"), ("u8", False, "pool")])
        gcols = [to_gpu(gpu, c) for c in cols]
        for desc in ([0, 0, 0], [1, 1, 0]):
            check_sort(gpu, cols, gcols, desc, [0, 0, 0], 100, f"limit constant {kind}")


@pytest.mark.parametrize("first", ["u8", "i64", "f64", "lstr"])
def test_limit_inside_the_run_of_one_of_five_values(gpu, first):
    """the candidates are every row up to and including the value's whole run — many times `limit` — and the second key picks among them"""
    n, rng = 100_000, np.random.default_rng(103)
    five = {"u8": np.array([0, 1, 7, 200, 255], np.uint8), "i64": np.array([-2**63, -1, 0, 1, 2**63 - 1], np.int64),
            "f64": np.array([-np.inf, -0.0, 5e-324, 1.0, np.nan]), "lstr": [b"", b"a", R.LONG40, R.LONG40 + b"x", R.LONG40 + b"y"]}[first]
    pick = rng.integers(0, 5, n)
    vals = five[pick] if isinstance(five, np.ndarray) else [five[i] for i in pick.tolist()]
    cols = [R.KeyCol(first, vals), R.make_col(rng, n, "f32", True), R.make_col(rng, n, "u16")]
    gcols = [to_gpu(gpu, c) for c in cols]
    for desc, limit in [([0, 0, 0], 20_500), ([1, 1, 0], 20_500), ([0, 1, 1], 100), ([1, 0, 0], 24_999)]:
        check_sort(gpu, cols, gcols, desc, [0, 1, 0], limit, f"five values {first}")


@pytest.mark.parametrize("per_bucket", [8192, 8193])
def test_limit_around_the_early_exit_of_the_select(gpu, per_bucket):
    """eight values of the first key's top byte with exactly 8192 or 8193 rows each: at 8192 the select stops after one byte and takes the
    bucket, at 8193 it goes on to the next byte"""
    n, rng = 8 * per_bucket, np.random.default_rng(per_bucket)
    top = rng.permutation(np.arange(n) % 8).astype(np.uint32)
    k0 = (top << 24) | rng.integers(0, 1 << 24, n).astype(np.uint32)
    cols = [R.KeyCol("u32", k0), R.make_col(rng, n, "i8", True)]
    assert n >= 65536 and np.bincount(k0 >> 24).tolist() == [per_bucket] * 8
    gcols = [to_gpu(gpu, c) for c in cols]
    for desc, limit in [([0, 0], 100), ([1, 0], 100), ([0, 1], 8192), ([0, 0], 8200), ([1, 1], 9000)]:
        check_sort(gpu, cols, gcols, desc, [0, 0], limit, f"early exit {per_bucket}")


def test_limit_whose_candidates_take_the_onesweep_passes(gpu):
    """4.3 M rows, LIMIT just over 2^20: the candidate set itself is past the onesweep switch"""
    n, limit, rng = 4_300_000, (1 << 20) + 24, np.random.default_rng(104)
    cols = [R.KeyCol("i64", rng.integers(-2**63, 2**63 - 1, n)), R.KeyCol("u8", rng.integers(0, 3, n).astype(np.uint8))]
    cols[0].values[rng.integers(0, n, n // 8)] = -2**62       # half a million ties on the first key, across row `limit` of the ascending order
    gcols = [to_gpu(gpu, c) for c in cols]
    for desc in ([0, 0], [1, 1]):
        check_sort(gpu, cols, gcols, desc, [0, 0], limit, "limit over 2^20")


# ---- onesweep ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [(1 << 20) - 1, 1 << 20, 2_500_001])
def test_onesweep_sizes(gpu, n):
    """64-bit images take the onesweep passes from 2^20 rows on, 32-bit images and null flags the histogram / scan / scatter passes"""
    combos = [([("i64", False, "pool")], [0], [0]), ([("u32", False, "pool")], [1], [0]), ([("u8", False, "low"), ("i64", True, "pool")], [0, 1], [0, 1]),
              ([("f64", True, "pool"), ("i32", False, "pool")], [1, 0], [0, 0]), ([("f64", False, "pool")], [0], [0]), ([("ts", True, "pool")], [0], [1])]
    for keys, desc, nf in combos:
        cols = R.make_cols(n % 1000, n, keys)
        check_sort(gpu, cols, [to_gpu(gpu, c) for c in cols], desc, nf, 0, f"onesweep {keys}")


# ---- dbhip_merge_sorted_perm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keyset", sorted(R.MERGE_KEYSETS))
@pytest.mark.parametrize("nruns", [0, 1, 2, 8, 33])
def test_merge_sorted_runs(gpu, keyset, nruns):
    """runs ordered by the reference, empty ones at the front, in the middle and at the end: merged order = the stable order of all rows"""
    keys, desc, nf = R.MERGE_KEYSETS[keyset]
    for n in (3000, 70_000):
        cols, offs = R.merge_runs(70 + nruns, n, nruns, keys, desc, nf)
        gcols = [to_gpu(gpu, c) for c in cols]
        if nruns == 0:
            assert len(gpu.merge_sorted_perm(gcols, [0], desc, nf)) == 0
            continue
        for limit in (0, 25, n):
            exp = R.sort_perm_fast(cols, desc, nf, limit)
            got = gpu.merge_sorted_perm(gcols, offs, desc, nf, limit)
            why = R.explain(cols, desc, nf, got, exp)
            assert why == "", (keyset, nruns, n, limit, why)


def test_merge_refuses_offsets_that_descend_or_do_not_start_at_zero(gpu):
    cols = R.make_cols(71, 100, [("i32", False, "pool")])
    order = R.sort_perm_fast(cols, [0], [0])
    cols = [c.take(order) for c in cols]
    gcols = [to_gpu(gpu, c) for c in cols]
    for offs in ([0, 60, 40, 100], [10, 100], [5, 5, 100], [0, 100, 99]):
        with pytest.raises(T.DbhipError) as e:
            gpu.merge_sorted_perm(gcols, offs)
        assert e.value.code == T.ERR_INVALID, offs
    assert np.array_equal(gpu.merge_sorted_perm(gcols, [0, 0, 100, 100]), np.arange(100))


# ---- dbhip_sort_bound_partition ----------------------------------------------------------------------------------------------------------
def check_partition(gpu, rows, grows, bounds, desc, nf, what):
    gb = [to_gpu(gpu, c) for c in bounds]
    part, counts = gpu.sort_bound_partition(grows, gb, desc, nf)
    got = part.to_numpy(np.uint32, rows[0].n)
    exp, ecounts = R.bound_partition_fast(rows, bounds, desc, nf)
    bad = np.nonzero(got != exp)[0]
    assert len(bad) == 0, (what, desc, nf, f"{len(bad)} rows in another range, first row {bad[0]}: {got[bad[0]]} for {exp[bad[0]]}")
    assert np.array_equal(counts, ecounts), (what, desc, nf, "counts")
    assert int(counts.sum()) == rows[0].n


@pytest.mark.parametrize("case", R.partition_cases(), ids=repr)
def test_bound_partition(gpu, case):
    """nullable rows against plain bounds and the converse, NULLs on keys 2 and 3, NULL / NaN / -0.0 bounds, duplicate bounds, every row
    on one side of the bounds, the bound counts at which the register, LDS-histogram and global paths change, bound images just under
    and over 32 KiB, inline rows against a long bound and the converse, eight keys"""
    rows = case.rows()
    grows = [to_gpu(gpu, c) for c in rows]
    for desc, nf in case.orders:
        check_partition(gpu, rows, grows, case.bounds(desc, nf), desc, nf, case.name)


@pytest.mark.parametrize("nb", [0, 7, 300])
def test_bound_partition_of_sliced_nullable_keys(gpu, nb):
    keys = [("i16", True, "low"), ("f64", True, "pool"), ("lstr", True, "pool")]
    rows = R.make_cols(80, 5003, keys)
    grows = [to_gpu_sliced(gpu, c, 81 + i) for i, c in enumerate(rows)]
    for desc, nf in [([0, 0, 0], [0, 0, 0]), ([1, 0, 1], [1, 1, 0])]:
        raw = R.make_cols(82, nb, keys) if nb else []
        bounds = [c.take(R.sort_perm_fast(raw, desc, nf)) for c in raw]
        check_partition(gpu, rows, grows, bounds, desc, nf, "sliced rows")
        check_partition(gpu, rows[:1], grows[:1], bounds[:1], desc[:1], nf[:1], "one sliced key")


# ---- the bytes past an inline value, and long values in a second buffer (tests/strview_cases.py) --------------------------------------
@pytest.mark.parametrize("inline_only", [False, True], ids=["with_long", "inline_only"])
def test_string_sort_ignores_the_bytes_past_an_inline_value(gpu, inline_only):
    """the shared String column with clean and with 0xFF padding: the reference's permutation both times. inline_only sorts by the two
    images of the inline view (no value longer than 12 bytes), the other column by the images of the bytes where they live."""
    from tests import strview_cases as S
    p = S.build(gpu, S.values(inline_only))
    for desc in (0, 1):
        exp = R.sort_perm([R.KeyCol("lstr", p.vals)], [desc], [0])
        for name, col in p.both():
            assert np.array_equal(gpu.sort_perm([col], desc=[desc]), exp), (name, desc)
