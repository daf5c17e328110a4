"""A plain-Python reference for the LIKE group (include/dbhip.h a20) that does not share the device's algorithm, and the seeded case
builder of tests/test_like_ref_cpu.py and tests/test_gpu_like.py.

The matcher is a set-of-positions DP over the parsed tokens (`%`, `_`, literal byte): S = the set of value positions the tokens read
so far can end at; the value matches when len(value) is in the final set. No segments, no leftmost search, no anchors. The set is
held as a Python integer with one BYTE per position (bit 8 p = "position p is in the set"), so that a literal token is one AND with a
per-byte-value mask made by bytes.translate and a shift by 8, and a `_` in unit mode is one numpy gather through the "next boundary"
array: a 70,001-byte value costs a few whole-value operations per token.

Units: with unit_byte a `_` reads one byte. Otherwise the unit boundaries of a value are position 0, position len and every position
whose byte is not 10xxxxxx, and a `_` reads from one boundary to the next one (so it cannot start inside a unit)."""
import numpy as np

PCT, UNDER = "%", "_"
EQUALS, PREFIX, SUFFIX, CONTAINS, SEGMENTS = range(5)
ERR_INVALID, ERR_UNSUPPORTED = 1, 7
MAX_PATTERN, MAX_SEGMENTS = 255, 16


def parse(pattern, escape=0x5C):
    """bytes -> tokens: PCT, UNDER or an int (a literal byte). escape: a byte value, or -1 / None for none."""
    esc = -1 if escape is None else int(escape)
    toks, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if esc >= 0 and c == esc:
            if i + 1 < len(pattern):
                toks.append(pattern[i + 1])
                i += 2
                continue
            toks.append(c)           # a trailing lone escape is itself a literal
        elif c == 0x25:
            toks.append(PCT)
        elif c == 0x5F:
            toks.append(UNDER)
        else:
            toks.append(c)
        i += 1
    return toks


def kind_of(pattern, escape=0x5C):
    """the classifier's answer: a kind, or -ERR_* for what the call refuses"""
    if escape is not None and not -1 <= escape <= 255:
        return -ERR_INVALID
    if len(pattern) > MAX_PATTERN:
        return -ERR_UNSUPPORTED
    toks = parse(pattern, escape)
    segs, cur = [], []
    for t in toks:
        if t == PCT:
            if cur:
                segs.append(cur)
            cur = []
        else:
            cur.append(t)
    if cur:
        segs.append(cur)
    if len(segs) > MAX_SEGMENTS:
        return -ERR_UNSUPPORTED
    if len(segs) != 1 or UNDER in segs[0]:
        return SEGMENTS
    front, back = toks[0] == PCT, toks[-1] == PCT
    return CONTAINS if front and back else (SUFFIX if front else (PREFIX if back else EQUALS))


_ONES = {}
_TABLES = {}
_PREPARED = {}


def _ones(n):
    """one byte 0x01 per position 0 .. n - 1"""
    m = _ONES.get(n)
    if m is None:
        m = _ONES[n] = int.from_bytes(b"\x01" * n, "little")
    return m


def _eq_mask(value, masks, b):
    m = masks.get(b)
    if m is None:
        t = _TABLES.get(b)
        if t is None:
            t = _TABLES[b] = bytes(1 if x == b else 0 for x in range(256))
        m = masks[b] = int.from_bytes(value.translate(t), "little")
    return m


def _prepared(value):
    p = _PREPARED.get(value)
    if p is None:
        if len(_PREPARED) > 4096:
            _PREPARED.clear()
        n = len(value)
        raw = np.frombuffer(value, dtype=np.uint8)
        isb = ((raw & 0xC0) != 0x80).astype(np.uint8)               # position p < len is a unit boundary
        if n:
            isb[0] = 1
        bnd = np.append(np.nonzero(isb)[0], n)
        nxt = np.zeros(n, dtype=np.int64)                            # boundary p < len -> the next boundary
        nxt[bnd[:-1]] = bnd[1:]
        p = _PREPARED[value] = (n, {}, (isb, nxt))
    return p


def like(value, pattern, escape=0x5C, unit_byte=False, tokens=None):
    toks = parse(pattern, escape) if tokens is None else tokens
    n, masks, nxt = _prepared(value)
    inside, upto = _ones(n), _ones(n + 1)
    S = 1                                                            # {0}
    for t in toks:
        if t == PCT:
            S = upto & ~((S & -S) - 1)                               # every position from the smallest one on
        elif t == UNDER:
            if unit_byte:
                S = (S & inside) << 8
            else:
                isb, nxt_of = nxt                                    # only a position that is a boundary can start a unit
                at = np.frombuffer((S & inside).to_bytes(n + 1, "little"), dtype=np.uint8)[:n]
                out = np.zeros(n + 1, dtype=np.uint8)
                out[nxt_of[np.nonzero(at & isb)[0]]] = 1
                S = int.from_bytes(out.tobytes(), "little")
        else:
            S = (S & _eq_mask(value, masks, t)) << 8
        if not S:
            return False
    return bool((S >> (8 * n)) & 1)


def like_column(values, valid, pattern, escape=0x5C, negate=False, unit_byte=False):
    """the filter bit of every row: a NULL row is False, also under negate"""
    toks = parse(pattern, escape)
    memo = {}
    out = []
    for i, v in enumerate(values):
        if valid is not None and not valid[i]:
            out.append(False)
            continue
        r = memo.get(v)
        if r is None:
            r = memo[v] = like(v, pattern, escape, unit_byte, toks)
        out.append(r != negate)
    return out


def str_match(kind, value, needle):
    return {EQUALS: value == needle, PREFIX: value.startswith(needle), SUFFIX: value.endswith(needle), CONTAINS: needle in value}[kind]


# ---- pools ------------------------------------------------------------------------------------------------------------------------
E2, E3, E4 = "é".encode(), "漢".encode(), "😀".encode()
PIECES = [b"a", b"b", b"ab", b"ba", b"A", E2, E3, E4, b"\x80", b"\xbf", b"\x00", b"\xff", b"%", b"_", b"\\", b"!"]

FIXED_VALUES = [
    b"", b"a", b"b", b"ab", b"abc", b"aaab", b"aab", b"AB", b"Ab", b"abab", b"ababa", b"bababa", b"abababab",
    b"a" * 12, b"ab" * 6, b"ab" * 6 + b"a", b"a" * 13, b"b" + b"a" * 12, b"a" * 12 + b"b",
    E2, E3, E4, b"a" + E2 + b"b", b"a" + E3 + b"b", b"a" + E4 + b"b", E2 + b"ab", b"ab" + E2, E2 + E3 + E4, E4 + E4 + E4 + b"a",
    b"\x80", b"a\x80b", b"\x80\x80", b"a\xbf", b"\xc3", b"a\xc3", b"\xc3\xa9\xa9", b"\x00", b"a\x00b", b"\xff", b"a\xffb", b"\x00\xff",
    b"%", b"_", b"\\", b"a%b", b"a_b", b"a\\b", b"100%", b"%ab", b"ab%", b"_ab", b"ab_", b"ab\\", b"\\%", b"a!b", b"a!%b",
    b"abbc", b"\xc3a", b"a\xc3b", b"a\xa9", b"ab\x80c",
]


def random_value(rng, max_pieces=9):
    return b"".join(PIECES[k] for k in rng.integers(0, len(PIECES), int(rng.integers(0, max_pieces + 1))))


def value_pool(seed, n_random=400):
    """the fixed values, every length 1 .. 13 over {a, b}, and seeded concatenations of PIECES"""
    rng = np.random.default_rng(seed)
    vals = list(FIXED_VALUES)
    for ln in range(1, 14):
        for _ in range(3):
            vals.append(bytes(rng.choice(np.frombuffer(b"ab", np.uint8), ln).tolist()))
    vals += [random_value(rng) for _ in range(n_random)]
    vals += [random_value(rng, 40) for _ in range(n_random // 8)]
    return vals


BS = 0x5C
P255_CONTAINS = b"%" + b"ab" * 126 + b"a%"                  # 255 bytes: a 253-byte needle
P255_SEGMENTS = b"ab" * 60 + b"%" + b"_" * 14 + b"ab" * 60  # 255 bytes, two segments, `_` in the second
P16 = b"%" + b"%".join([b"a", b"b"] * 8) + b"%"             # 16 segments
assert len(P255_CONTAINS) == 255 and len(P255_SEGMENTS) == 255

# (pattern, escape)
PATTERNS = [
    (b"ab", BS), (b"a", BS), (b"abab", BS), (b"ababa", BS), (b"abababab", BS), (b"ab" * 6, BS), (b"ab" * 6 + b"a", BS), (E3, BS),        # EQUALS
    (b"ab%", BS), (b"a%", BS), (b"abab%", BS), (b"ababa%", BS), (b"a" * 12 + b"%", BS), (b"a" * 13 + b"%", BS), (E2 + b"%", BS),             # PREFIX
    (b"%ab", BS), (b"%b", BS), (b"%abab", BS), (b"%babab", BS), (b"%" + b"a" * 12, BS), (b"%" + b"a" * 13, BS), (b"%" + E2, BS), (b"%\xa9", BS),  # SUFFIX
    (b"%ab%", BS), (b"%a%", BS), (b"%aab%", BS), (b"%abab%", BS), (b"%ababa%", BS), (b"%bababa%", BS), (b"%\x80%", BS), (b"%\x00%", BS),
    (b"%\xff%", BS), (b"%" + E4 + b"%", BS), (b"%A%", BS),                                                                                  # CONTAINS
    (b"%%ab%%", BS), (b"%%", BS), (b"%%%", BS), (b"a%%b", BS), (b"ab%%", BS), (b"%%ab", BS),                                               # doubled %
    (b"a%b", BS), (b"%a%b%", BS), (b"%ab%bc%", BS), (b"%ab%ba%", BS), (b"a%b%a", BS), (b"ab%ab", BS), (b"a%a", BS), (b"%a%a", BS), (b"a%a%", BS),
    (b"_", BS), (b"__", BS), (b"_ab", BS), (b"a_b", BS), (b"ab_", BS), (b"_%", BS), (b"%_", BS), (b"%_%", BS), (b"_%_", BS), (b"%_a", BS), (b"a_%", BS),
    (b"%a_b%", BS), (b"%_b", BS), (b"a__%", BS), (b"%__", BS), (b"_a%b_", BS), (b"%\xc3_", BS), (b"_\xa9", BS), (b"%_\x80%", BS), (b"a%_%b", BS),
    (b"_" * 12, BS), (b"_" * 13, BS), (b"%" + b"_" * 5 + b"%", BS),
    (b"\\%", BS), (b"\\_", BS), (b"\\\\", BS), (b"a\\%b", BS), (b"a\\_b", BS), (b"%\\%", BS), (b"\\%%", BS), (b"%\\_%", BS), (b"%\\\\%", BS),
    (b"100\\%", BS), (b"\\a\\b", BS),
    (b"ab\\", BS), (b"%\\", BS), (b"\\", BS), (b"a%\\", BS),                                                                                  # a trailing lone escape
    (b"a!%b", 0x21), (b"!_%", 0x21), (b"%!!%", 0x21), (b"a\\%", 0x21), (b"%!", 0x21), (b"a%%b", 0x25), (b"a\\%", -1), (b"\\%", -1), (b"%\\_", -1),
    (b"", BS), (b"%", BS),
    (P255_CONTAINS, BS), (P255_SEGMENTS, BS), (P16, BS),
]


def long_values(seed):
    """values that the 255-byte and the 16-segment patterns can match, and near misses"""
    rng = np.random.default_rng(seed)
    needle = P255_CONTAINS[1:-1]
    out = [needle, b"b" + needle + b"b", needle[:-1] + b"b", b"ab" * 200, b"ab" * 60 + E3 * 14 + b"ab" * 60, b"ab" * 60 + E3 * 13 + b"ab" * 60,
           b"ab" * 60 + b"x" * 14 + b"ab" * 60, b"ab" * 60 + b"ab" * 60, b"ab" * 8, b"ab" * 7 + b"a", b"ba" * 8, b"a" * 20 + b"b"]
    for _ in range(6):
        k = int(rng.integers(0, 40))
        out.append(random_value(rng, k) + needle + random_value(rng, k))
    return out
