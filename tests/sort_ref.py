"""The order that dbhip_sort_perm, dbhip_merge_sorted_perm and dbhip_sort_bound_partition promise (include/dbhip.h, a16), stated
in plain Python over plain values, and nothing about how the device gets there.

Per key: NULL against a value is decided by nulls_first alone (never by desc), two NULLs tie, two values compare by type and the
result is negated for desc. Integers, dates, timestamps and decimals are Python ints, Boolean false < true, floats are
OrderedFloat (every NaN equals every NaN and is greater than everything else, -0.0 == +0.0, subnormals are ordinary distinct
values), strings are Python bytes (memcmp order, a proper prefix first). Rows that tie on every key come out by ascending row id.

Two statements of it: `compare_rows` / `sort_perm` / `bound_partition` (a three-way comparator under cmp_to_key, a linear count
of bounds) and the vectorised twins `sort_perm_fast` / `bound_partition_fast` (dense ranks per key + np.lexsort) for the sizes at
which the comparator is too slow. tests/test_sort_ref_cpu.py proves the twins equal to the comparator and to the C oracle on
every small case below, and shows that the cases reject nine wrong orderings.

The rest is the seeded case builder and the case lists that the CPU and the GPU module share."""
import functools
import itertools

import numpy as np

# ---- columns --------------------------------------------------------------------------------------------------------------------
INT_KINDS = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "u8": np.uint8, "u16": np.uint16, "u32": np.uint32,
             "u64": np.uint64, "date": np.int32, "ts": np.int64, "dec64": np.int64}
FLOAT_KINDS = {"f32": np.float32, "f64": np.float64}
STRING_KINDS = ("str", "lstr")          # values of at most 12 bytes (inline views) / of any length up to 4096
ALL_KINDS = ["bool", "i8", "i16", "i32", "i64", "u8", "u16", "u32", "u64", "f32", "f64", "date", "ts", "dec64", "dec128", "str", "lstr"]


class KeyCol:
    """one key column as plain data: `values` = a numpy array (integers, floats, Boolean) or a list (Decimal128 ints, bytes);
    `valid` = None or a bool array (False = NULL; the value under a NULL is arbitrary and must not matter)"""

    def __init__(self, kind, values, valid=None):
        self.kind, self.values = kind, values
        self.valid = None if valid is None else np.asarray(valid, dtype=bool)
        self.n = len(values)
        self._py = None

    def py(self):
        """the values as Python objects: int, bool, float, bytes"""
        if self._py is None:
            self._py = self.values.tolist() if isinstance(self.values, np.ndarray) else list(self.values)
        return self._py

    def take(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        vals = self.values[idx] if isinstance(self.values, np.ndarray) else [self.values[i] for i in idx.tolist()]
        return KeyCol(self.kind, vals, None if self.valid is None else self.valid[idx])

    def rows(self, lo, hi):
        return KeyCol(self.kind, self.values[lo:hi], None if self.valid is None else self.valid[lo:hi])


def concat(a, b):
    assert a.kind == b.kind or {a.kind, b.kind} == set(STRING_KINDS)
    vals = np.concatenate([a.values, b.values]) if isinstance(a.values, np.ndarray) else list(a.values) + list(b.values)
    valid = None
    if a.valid is not None or b.valid is not None:
        valid = np.concatenate([np.ones(a.n, bool) if a.valid is None else a.valid, np.ones(b.n, bool) if b.valid is None else b.valid])
    return KeyCol("lstr" if "lstr" in (a.kind, b.kind) else a.kind, vals, valid)


# ---- the comparator -------------------------------------------------------------------------------------------------------------
def cmp_float(a, b):
    """OrderedFloat: NaN == NaN, NaN greater than every number; -0.0 == 0.0 is what Python's == says already"""
    an, bn = a != a, b != b
    if an or bn:
        return int(an) - int(bn)
    return (a > b) - (a < b)


def cmp_plain(a, b):
    """ints, bools (False < True) and bytes (memcmp order, then the length) under Python's own order"""
    return (a > b) - (a < b)


def value_cmp(kind):
    return cmp_float if kind in FLOAT_KINDS else cmp_plain


def compare_rows(a_cols, i, b_cols, j, desc, nulls_first):
    """row i of a_cols against row j of b_cols (the same key kinds): -1 / 0 / 1"""
    for k, (a, b) in enumerate(zip(a_cols, b_cols)):
        va = a.valid is None or bool(a.valid[i])
        vb = b.valid is None or bool(b.valid[j])
        if not va or not vb:
            if va == vb:
                continue                                    # two NULLs tie
            a_first = bool(nulls_first[k]) if not va else not nulls_first[k]      # desc has no say here
            return -1 if a_first else 1
        r = value_cmp(a.kind)(a.py()[i], b.py()[j])
        if r:
            return -r if desc[k] else r
    return 0


def sort_perm(cols, desc, nulls_first, limit=0):
    n = cols[0].n
    for c in cols:
        c.py()

    def cmp(i, j):
        return compare_rows(cols, i, cols, j, desc, nulls_first) or (i > j) - (i < j)
    order = sorted(range(n), key=functools.cmp_to_key(cmp))
    return np.array(order[:limit] if 0 < limit < n else order, dtype=np.uint32)


def merge_perm(cols, run_offsets, desc, nulls_first, limit=0):
    """the runs lie back to back, so (run, position) is the row id: the merge is the stable sort of all rows"""
    assert len(run_offsets) == 0 or (run_offsets[0] == 0 and run_offsets[-1] == cols[0].n)
    return sort_perm(cols, desc, nulls_first, limit)


def bound_partition(rows, bounds, desc, nulls_first):
    """-> (for every row the number of bounds that compare strictly before it, the rows per range [nbounds + 1])"""
    n, nb = rows[0].n, bounds[0].n if bounds else 0
    part = np.zeros(n, np.uint32)
    for i in range(n):
        lo, hi = 0, nb                      # the bounds are ordered: the first one that is not before the row
        while lo < hi:
            mid = (lo + hi) // 2
            if compare_rows(bounds, mid, rows, i, desc, nulls_first) < 0:
                lo = mid + 1
            else:
                hi = mid
        part[i] = lo
    return part, np.bincount(part, minlength=nb + 1).astype(np.uint64)


# ---- the vectorised twin --------------------------------------------------------------------------------------------------------
def _dense_rank(col):
    """-> (rank of every row's VALUE among the column's distinct values under the value order, number of distinct values)"""
    v = col.values
    if col.kind in FLOAT_KINDS:
        with np.errstate(invalid="ignore"):         # (widening a signalling NaN raises the invalid flag)
            v = np.asarray(v).astype(np.float64)    # exact for float32, subnormals included
        nan = v != v
        v = np.where(v == 0, 0.0, v)                # -0.0 and +0.0 are one value
        u, inv = np.unique(v[~nan], return_inverse=True)
        rank = np.full(len(v), len(u), np.int64)    # all NaNs are one value above the rest
        rank[~nan] = inv
        return rank, len(u) + 1
    if isinstance(v, np.ndarray):
        u, inv = np.unique(v, return_inverse=True)
        return inv.astype(np.int64).reshape(-1), len(u)
    obj = np.empty(len(v), dtype=object)
    obj[:] = list(v)
    u, inv = np.unique(obj, return_inverse=True)    # Python's order of ints / bytes
    return inv.astype(np.int64).reshape(-1), len(u)


def rank_keys(cols, desc, nulls_first):
    """[nkeys][n] int64: rows compare like their columns of ranks, key 0 first"""
    out = []
    for k, c in enumerate(cols):
        rank, nd = _dense_rank(c)
        if desc[k]:
            rank = (nd - 1) - rank
        if c.valid is not None:
            rank = np.where(c.valid, rank, -1 if nulls_first[k] else nd)
        out.append(rank)
    return np.array(out, dtype=np.int64).reshape(len(cols), -1)


def sort_perm_fast(cols, desc, nulls_first, limit=0):
    n = cols[0].n
    ranks = rank_keys(cols, desc, nulls_first)
    order = np.lexsort([np.arange(n)] + [ranks[k] for k in range(len(cols) - 1, -1, -1)]).astype(np.uint32)
    return order[:limit] if 0 < limit < n else order


def bound_partition_fast(rows, bounds, desc, nulls_first):
    n, nb = rows[0].n, bounds[0].n if bounds else 0
    if nb == 0:
        return np.zeros(n, np.uint32), np.array([n], np.uint64)
    both = [concat(r, b) for r, b in zip(rows, bounds)]      # rows first: in the stable order a row precedes the bounds it ties with
    order = sort_perm_fast(both, desc, nulls_first).astype(np.int64)
    is_bound = order >= n
    before = np.cumsum(is_bound) - is_bound
    part = np.zeros(n + nb, np.int64)
    part[order] = before
    part = part[:n].astype(np.uint32)
    return part, np.bincount(part, minlength=nb + 1).astype(np.uint64)


def same_key_sequence(cols, desc, nulls_first, got, exp):
    """do two permutations list the same key values position by position? (then they differ in the order of ties at most)"""
    got, exp = np.asarray(got, dtype=np.int64), np.asarray(exp, dtype=np.int64)
    if got.shape != exp.shape or (len(got) and (got.max() >= cols[0].n)):
        return False
    ranks = rank_keys(cols, desc, nulls_first)
    return bool(np.array_equal(ranks[:, got], ranks[:, exp]))


def explain(cols, desc, nulls_first, got, exp):
    """'' when equal, else which of the two promises is broken"""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape == exp.shape and np.array_equal(got, exp):
        return ""
    if got.shape != exp.shape:
        return f"{len(got)} rows for {len(exp)}"
    at = int(np.nonzero(got != exp)[0][0])
    if same_key_sequence(cols, desc, nulls_first, got, exp):
        return f"same key sequence, different tie order (stability broken) from position {at}: row {got[at]} for row {exp[at]}"
    return f"key sequence differs (contract broken); first other row at position {at}: row {got[at]} for row {exp[at]}"


# ---- value pools ----------------------------------------------------------------------------------------------------------------
def float_specials(dtype):
    """+qNaN, -qNaN, an sNaN, NaNs with the full payload, +-0, +-smallest and largest subnormal, +-smallest normal, +-MAX, +-Inf"""
    if np.dtype(dtype) == np.float32:
        bits = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000]
        return np.array(bits, dtype=np.uint32).view(np.float32)
    bits = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x0000000000000000,
            0x8000000000000000, 0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF, 0x0010000000000000,
            0x8010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000]
    return np.array(bits, dtype=np.uint64).view(np.float64)


P10 = b"prefix_abc"                                      # the 11-, 12- and 13-byte family shares these 10 bytes
LONG40 = bytes(range(65, 105))                           # long values that differ in the last byte or in the length only
INLINE_POOL = [b"", b"a", b"a\x00", b"a\x00\x00", b"ab", b"b", P10, P10 + b"d", P10 + b"de", P10 + b"df", b"\xff" * 11, b"\xff" * 12,
               b"\x00", b"\x00" * 12, b"abcdefgh", b"abcdefgh\x00", b"abcdefgi"]
LONG_POOL = INLINE_POOL + [P10 + b"def", P10 + b"deg", P10 + b"de\x00", b"\xff" * 13, b"\xff" * 12 + b"\x00", LONG40, LONG40 + b"x", LONG40 + b"y",
                           LONG40 + b"\x00", LONG40[:39], LONG40[:16], LONG40[:17], b"a" * 24, b"a" * 25]


def _ints(rng, n, dtype, card):
    info = np.iinfo(dtype)
    lo, hi = int(info.min), int(info.max)
    dense = list(range(-3, 4)) if lo < 0 else list(range(0, 7))
    if card == "low":
        return np.array(dense[2:5], dtype=dtype)[rng.integers(0, 3, n)]
    edges = [lo, hi, lo + 1, hi - 1, 0, 1] + ([-1] if lo < 0 else [])
    pool = np.array(dense * 3 + edges * 2, dtype=dtype)
    out = pool[rng.integers(0, len(pool), n)]
    wide = rng.integers(lo, hi, n, dtype=dtype, endpoint=True)
    return np.where(rng.random(n) < 0.25, wide, out).astype(dtype)


def _floats(rng, n, dtype, card):
    reals = np.round(rng.standard_normal(n) * 3, 1).astype(dtype)
    if card == "low":
        return np.array([-0.0, 0.0, np.nan, 1.5], dtype=dtype)[rng.integers(0, 4, n)]
    sp = float_specials(dtype)
    tiny = (rng.integers(1, 50, n) * np.where(rng.random(n) < 0.5, -1, 1)).astype(np.int64)
    sub = (tiny.astype(np.float64) * float(np.finfo(dtype).smallest_subnormal)).astype(dtype)      # a run of small subnormals
    pick = rng.random(n)
    return np.where(pick < 0.4, sp[rng.integers(0, len(sp), n)], np.where(pick < 0.55, sub, reals)).astype(dtype)


def _strings(rng, n, long, card):
    if card == "low":
        pool = [b"a", b"a\x00", b"b"] if not long else [LONG40 + b"x", LONG40 + b"y", LONG40]
        return [pool[i] for i in rng.integers(0, 3, n).tolist()]
    pool = LONG_POOL if long else INLINE_POOL
    alpha = [b"a", b"b", b"\x00", b"\xff"]
    out = []
    picks, lens = rng.random(n).tolist(), rng.integers(0, 41 if long else 13, n).tolist()
    idx, letters = rng.integers(0, len(pool), n).tolist(), rng.integers(0, 4, (n, 4)).tolist()
    for i in range(n):
        if picks[i] < 0.6:
            out.append(pool[idx[i]])
        else:       # a low-entropy random value: a run of one letter with a three-letter tail, so that long common prefixes are the rule
            ln = lens[i]
            out.append((alpha[letters[i][0]] * ln + b"".join(alpha[x] for x in letters[i][1:]))[:ln])
    if long and n:
        out[0] = P10 + b"def"      # a long-string column always holds a value beyond the 12 inline bytes
    return out


def make_col(rng, n, kind, nullable=False, card="pool"):
    """one seeded column of `kind`; card = 'pool' (edges, a dense run of ties, the full range), 'low' (three or four values),
    'const' (one value) or 'null' (every row NULL)"""
    if kind == "bool":
        vals = rng.integers(0, 2, n).astype(bool)
    elif kind in INT_KINDS:
        vals = _ints(rng, n, INT_KINDS[kind], card)
    elif kind in FLOAT_KINDS:
        vals = _floats(rng, n, FLOAT_KINDS[kind], card)
    elif kind == "dec128":
        lo, hi = -(10**38 - 1), 10**38 - 1
        pool = [lo, hi, 0, 1, -1, 2**64, -2**64, 2**64 - 1, -2**64 - 1, 2**63, -2**63, 2**127 - 1, -2**127] + list(range(-3, 4)) * 3
        if card == "low":
            pool = [-2**64, 0, 2**64]
        r = rng.integers(-2**62, 2**62, n).tolist()
        pick, idx = rng.random(n).tolist(), rng.integers(0, len(pool), n).tolist()
        vals = [pool[idx[i]] if pick[i] < 0.7 or card == "low" else r[i] * (2**60 + 12345) for i in range(n)]
    else:
        vals = _strings(rng, n, kind == "lstr", card)
    if card == "const" and n:
        vals = vals[:1].repeat(n) if isinstance(vals, np.ndarray) else [vals[0]] * n
    valid = None
    if nullable or card == "null":
        valid = rng.random(n) < 0.75
        if n >= 2:
            valid[rng.integers(0, n)] = False
            valid[(int(np.nonzero(~valid)[0][0]) + 1) % n] = True
        if card == "null":
            valid[:] = False
    return KeyCol(kind, vals, valid)


def make_cols(seed, n, keys):
    """keys = [(kind, nullable, card)]; every column draws from its own stream, so a key is the same column whatever stands beside it"""
    return [make_col(np.random.default_rng([seed, pos, ALL_KINDS.index(kind)]), n, kind, nullable, card) for pos, (kind, nullable, card) in enumerate(keys)]


# ---- the shared case lists ------------------------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 100_003]      # the wave, the 4096-key scratch tile, the 8192-key pass tile
SMALL = 8193                                                                  # up to here the comparator runs in the CPU module


class SortCase:
    """columns (seed, n, keys) and the orders [(desc, nulls_first, limit)] to sort them by"""

    def __init__(self, name, seed, n, keys, orders):
        self.name, self.seed, self.n, self.keys, self.orders = name, seed, n, keys, orders

    def cols(self):
        return make_cols(self.seed, self.n, self.keys)

    def __repr__(self):
        return self.name


def single_key_cases():
    """every key type alone: plain asc / desc, nullable asc / desc x NULLs first / last, at every size"""
    out = []
    for kind in ALL_KINDS:
        for n in SIZES:
            out.append(SortCase(f"{kind}-n{n}-plain", n, n, [(kind, False, "pool")], [([0], [0], 0), ([1], [1], 0)]))
            out.append(SortCase(f"{kind}-n{n}-nullable", n + 1, n, [(kind, True, "pool")], [([d], [f], 0) for d in (0, 1) for f in (0, 1)]))
    return out


MIXED8 = ["u8", "f32", "str", "i64", "bool", "lstr", "dec128", "f64"]


def multi_key_cases():
    out = []
    two = [([d0, d1], [f0, f1], 0) for d0 in (0, 1) for d1 in (0, 1) for f0 in (0, 1) for f1 in (0, 1)]
    for n in (65, 4097, 20_011):
        out.append(SortCase(f"two-nullable-n{n}", 21, n, [("i16", True, "low"), ("f64", True, "pool")], two))
        out.append(SortCase(f"two-strings-n{n}", 22, n, [("str", True, "low"), ("lstr", True, "pool")], two[::3]))
        out.append(SortCase(f"three-n{n}", 23, n, [("bool", True, "pool"), ("date", True, "low"), ("dec64", True, "pool")],
                            [([0, 1, 0], [1, 0, 1], 0), ([1, 0, 1], [0, 1, 0], 0), ([1, 1, 1], [1, 1, 1], 7)]))
        out.append(SortCase(f"five-n{n}", 25, n, [("u8", True, "low"), ("bool", True, "pool"), ("f32", True, "low"), ("ts", True, "low"), ("str", True, "pool")],
                            [([0, 0, 0, 0, 0], [0, 0, 0, 0, 0], 0), ([1, 0, 1, 0, 1], [0, 1, 1, 0, 0], 0), ([1, 1, 1, 1, 1], [1, 1, 1, 1, 1], 50)]))
        rng = np.random.default_rng(8 + n)
        eight = [([0] * 8, [0] * 8, 0), ([1] * 8, [1] * 8, 0)] + [(rng.integers(0, 2, 8).tolist(), rng.integers(0, 2, 8).tolist(), 0) for _ in range(4)]
        out.append(SortCase(f"eight-all-nullable-n{n}", 28, n, [(k, True, "low" if i < 6 else "pool") for i, k in enumerate(MIXED8)], eight))
        out.append(SortCase(f"eight-nulls-on-odd-keys-n{n}", 29, n, [(k, i % 2 == 1, "low" if i < 5 else "pool") for i, k in enumerate(MIXED8[::-1])], eight[1:4]))
        for pos in range(1, 4):
            keys = [("i8", False, "low"), ("u16", False, "low"), ("i32", False, "low"), ("u32", False, "pool")]
            keys[pos] = (keys[pos][0], True, keys[pos][2])
            out.append(SortCase(f"nulls-on-key{pos + 1}-only-n{n}", 30 + pos, n, keys, [([0, 0, 0, 0], [0, 0, 0, 0], 0), ([0, 1, 1, 0], [1, 1, 1, 1], 0)]))
        out.append(SortCase(f"later-key-all-null-n{n}", 34, n, [("u8", False, "low"), ("i64", False, "null"), ("f32", True, "pool")], [([0, 0, 1], [0, 1, 0], 0), ([1, 1, 0], [1, 0, 1], 0)]))
        out.append(SortCase(f"later-key-constant-n{n}", 35, n, [("u8", True, "low"), ("f64", False, "const"), ("lstr", False, "const"), ("i16", True, "pool")],
                            [([0, 0, 0, 1], [0, 0, 0, 1], 0), ([1, 1, 1, 0], [1, 0, 0, 0], 0)]))
        for f in ("f32", "f64"):
            out.append(SortCase(f"{f}-then-int-n{n}", 36, n, [(f, True, "pool"), ("i32", False, "pool")], [([0, 0], [0, 0], 0), ([1, 1], [1, 0], 0), ([1, 0], [0, 0], 0)]))
            out.append(SortCase(f"{f}-behind-low-key-n{n}", 37, n, [("u8", False, "low"), (f, False, "pool")], [([0, 0], [0, 0], 0), ([0, 1], [0, 0], 0), ([1, 1], [0, 0], 0)]))
            out.append(SortCase(f"{f}-zero-and-nan-ties-n{n}", 38, n, [(f, False, "low"), ("i16", False, "pool")], [([0, 0], [0, 0], 0), ([1, 0], [0, 0], 0), ([0, 1], [0, 0], 0)]))
    return out


def sort_cases():
    return single_key_cases() + multi_key_cases()


class PartCase:
    """rows and bounds of the same keys: keys = [(kind, rows nullable, bounds nullable, rows card, bounds card)]"""

    def __init__(self, name, seed, n, nb, keys, orders, fixed_bounds=None):
        self.name, self.seed, self.n, self.nb, self.keys, self.orders, self.fixed_bounds = name, seed, n, nb, keys, orders, fixed_bounds

    def rows(self):
        return make_cols(self.seed, self.n, [(k, rn, rc) for k, rn, bn, rc, bc in self.keys])

    def bounds(self, desc, nulls_first):
        """the bounds in the order of (desc, nulls_first), by the reference's own sort"""
        if self.nb == 0:
            return []
        raw = self.fixed_bounds() if self.fixed_bounds else make_cols(self.seed + 1000, self.nb, [(k, bn, bc) for k, rn, bn, rc, bc in self.keys])
        order = sort_perm_fast(raw, desc, nulls_first)
        return [c.take(order) for c in raw]

    def __repr__(self):
        return self.name


def _asc_desc(nk, nf_patterns=((0,), (1,))):
    return [([d] * nk, [f[i % len(f)] for i in range(nk)]) for d in (0, 1) for f in nf_patterns]


def _fixed(kind, values, valid=None):
    dt = FLOAT_KINDS.get(kind) or INT_KINDS.get(kind)
    return lambda: [KeyCol(kind, np.array(values, dtype=dt) if dt else list(values), valid)]


NB_EDGES = [0, 1, 8, 9, 63, 64, 2047, 2048, 5000]       # register path <= 63, LDS histogram <= 2048 ranges, the global one


def partition_cases():
    out = []
    for nb in NB_EDGES:
        out.append(PartCase(f"one-plain-key-nb{nb}", 50, 6007, nb, [("i32", False, False, "pool", "pool")], _asc_desc(1)))
        out.append(PartCase(f"one-f64-key-nb{nb}", 51, 6007, nb, [("f64", False, False, "pool", "pool")], _asc_desc(1)))
        out.append(PartCase(f"nullable-rows-plain-bounds-nb{nb}", 52, 6007, nb, [("i16", True, False, "pool", "pool")], _asc_desc(1)))
        out.append(PartCase(f"plain-rows-nullable-bounds-nb{nb}", 53, 6007, nb, [("f32", False, True, "pool", "pool")], _asc_desc(1)))
        out.append(PartCase(f"three-keys-nulls-on-2-and-3-nb{nb}", 54, 6007, nb, [("u8", False, False, "low", "low"), ("date", True, False, "low", "low"), ("f64", False, True, "pool", "pool")],
                            _asc_desc(3, ((0, 0, 1), (1, 1, 0)))))
    for nb in (0, 9, 300):
        out.append(PartCase(f"three-keys-nullable-rows-plain-bounds-nb{nb}", 55, 6007, nb, [("i8", True, False, "low", "low"), ("str", True, False, "low", "low"), ("i64", True, False, "pool", "pool")],
                            _asc_desc(3, ((0, 1, 0), (1, 0, 1)))))
        out.append(PartCase(f"three-keys-plain-rows-nullable-bounds-nb{nb}", 56, 6007, nb, [("bool", False, True, "pool", "pool"), ("u16", False, True, "low", "low"), ("dec128", False, True, "pool", "pool")],
                            _asc_desc(3, ((0, 1, 0), (1, 0, 1)))))
        out.append(PartCase(f"eight-keys-nb{nb}", 57, 6007, nb, [(k, i % 2 == 0, i % 3 == 0, "low" if i < 6 else "pool", "low" if i < 6 else "pool") for i, k in enumerate(MIXED8)],
                            [([0] * 8, [0] * 8), ([1, 0, 1, 0, 1, 0, 1, 0], [1, 1, 0, 0, 1, 1, 0, 0])]))
    nan, inf = float("nan"), float("inf")
    out.append(PartCase("null-bound", 58, 3001, 5, [("i32", True, True, "pool", "pool")], _asc_desc(1), _fixed("i32", [-5, 0, 0, 7, 9], np.array([1, 0, 1, 1, 1], bool))))
    out.append(PartCase("nan-bound", 59, 3001, 4, [("f32", False, False, "pool", "pool")], _asc_desc(1), _fixed("f32", [-inf, 0.5, nan, inf])))
    out.append(PartCase("negative-zero-bound", 60, 3001, 1, [("f64", False, False, "low", "pool")], _asc_desc(1), _fixed("f64", [-0.0])))
    out.append(PartCase("positive-zero-bound-f32", 61, 3001, 2, [("f32", True, False, "low", "pool")], _asc_desc(1), _fixed("f32", [0.0, -0.0])))
    out.append(PartCase("duplicate-bounds", 62, 3001, 6, [("i64", False, False, "low", "pool")], _asc_desc(1), _fixed("i64", [-1, -1, 0, 0, 0, 1])))
    out.append(PartCase("all-rows-after-the-last-bound", 63, 3001, 3, [("u8", False, False, "pool", "pool")], [([0], [0])], _fixed("u8", [0, 0, 0])))
    out.append(PartCase("all-rows-before-the-first-bound", 64, 3001, 3, [("u8", False, False, "low", "pool")], [([0], [0])], _fixed("u8", [200, 201, 255])))
    # bounds of one inline-string key with a null flag = 3 images of 8 bytes: 1365 bounds are 32 760 bytes, 1366 are 32 784
    for nb in (1365, 1366):
        out.append(PartCase(f"string-bounds-around-32KiB-nb{nb}", 65, 4001, nb, [("str", True, True, "pool", "pool")], _asc_desc(1)))
    out.append(PartCase("inline-rows-long-bound", 66, 3001, 3, [("str", False, False, "pool", "pool")], _asc_desc(1), _fixed("lstr", [b"a\x00", P10 + b"def", b"\xff" * 13])))
    out.append(PartCase("long-rows-inline-bounds", 67, 3001, 40, [("lstr", True, False, "pool", "pool")], _asc_desc(1), lambda: make_cols(1067, 40, [("str", False, "pool")])))
    out.append(PartCase("long-rows-long-bounds-two-keys", 68, 3001, 40, [("u8", False, False, "low", "low"), ("lstr", True, True, "pool", "pool")], _asc_desc(2, ((0, 1), (1, 0)))))
    return out


MERGE_KEYSETS = {
    "f64-desc-nullable+long-string": ([("f64", True, "pool"), ("lstr", True, "pool")], [1, 0], [0, 1]),
    "dec128+bool+u16": ([("dec128", False, "low"), ("bool", False, "pool"), ("u16", False, "pool")], [0, 1, 0], [0, 0, 0]),
}


def merge_runs(seed, n, nruns, keys, desc, nulls_first):
    """`nruns` runs cut at seeded points — empty ones at the front, in the middle and at the end when there are eight or more — each
    ordered by the reference. -> (columns of the runs laid back to back, run offsets [nruns + 1])"""
    rng = np.random.default_rng(seed)
    raw = make_cols(seed, n, keys)
    if nruns == 0:
        return raw, [0]
    cuts = np.sort(rng.integers(0, n + 1, nruns - 1)).tolist()
    offs = [0] + cuts + [n]
    if nruns >= 8:
        offs[1] = 0                        # an empty run at the front,
        offs[nruns // 2] = offs[nruns // 2 + 1]      # one in the middle
        offs[nruns - 1] = n                # and one at the end
        offs = np.maximum.accumulate(offs).tolist()
    order = np.concatenate([lo + sort_perm_fast([c.rows(lo, hi) for c in raw], desc, nulls_first).astype(np.int64) for lo, hi in zip(offs[:-1], offs[1:])] + [np.zeros(0, np.int64)])
    return [c.take(order) for c in raw], offs


def product(*a):
    return list(itertools.product(*a))
