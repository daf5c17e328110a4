"""CPU: tests/like_ref.py — the reference the GPU LIKE tests assert against — is held to sqlite3's LIKE on valid UTF-8, and named cases
reject five wrong matchers (negative controls, as in tests/test_window_ref_cpu.py). dbhip_like_kind, which needs no device, is checked
against a table of hand-written patterns, the limits and the error codes. The last tests compile the kernels' own matching steps
(databend_amd/csrc/like_match.h) for the host with checked loads and hold them to the reference at every buffer misalignment."""
import ctypes as C
import os
import re
import sqlite3
import subprocess

import numpy as np
import pytest

from tests import like_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIKE_SYMBOLS = ["dbhip_like_kind", "dbhip_like", "dbhip_str_match"]


def test_like_symbols_are_exported():
    from databend_amd import _lib
    header = open(os.path.join(ROOT, "include", "dbhip.h")).read()
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    for name in LIKE_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert re.search(r"\bT " + name + r"$", exported, flags=re.M), name
        assert name in _lib.SYMBOLS, name
    assert int(re.search(r"#define DBHIP_LIKE_LONG_BYTES (\d+)", header).group(1)) == _lib.LIKE_LONG_BYTES
    assert (_lib.LIKE_EQUALS, _lib.LIKE_PREFIX, _lib.LIKE_SUFFIX, _lib.LIKE_CONTAINS, _lib.LIKE_SEGMENTS) == (0, 1, 2, 3, 4)
    assert (R.EQUALS, R.PREFIX, R.SUFFIX, R.CONTAINS, R.SEGMENTS) == (0, 1, 2, 3, 4)
    from databend_amd import device
    assert device.like and device.str_match and device.like_kind


# ---- (a) the reference against sqlite3 ---------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "é", "漢", "_", "%", "\\", "ab"]


def test_reference_equals_sqlite_like():
    """40,000 seeded (value, pattern) draws over ALPHABET. sqlite differs by design only for a pattern that ends in a lone escape (it
    raises no error but never matches), so those are skipped; nothing else is. Values are drawn longer than patterns, and patterns are
    rich in `%`, so that both answers are well represented: each side must hold at least 5 % of the compared cases."""
    db = sqlite3.connect(":memory:")
    db.execute("PRAGMA case_sensitive_like=ON")
    rng = np.random.default_rng(20)
    weights = np.array([3, 3, 1, 1, 1.5, 3, 0.5, 1])
    weights = weights / weights.sum()
    compared = matches = skipped = 0
    for _ in range(40_000):
        value = "".join(ALPHABET[k] for k in rng.integers(0, 4, int(rng.integers(0, 7))))
        if rng.random() < 0.15:
            value += "".join(ALPHABET[k] for k in rng.integers(0, len(ALPHABET), 2))
        pattern = "".join(ALPHABET[k] for k in rng.choice(len(ALPHABET), int(rng.integers(0, 6)), p=weights))
        toks = R.parse(pattern.encode(), 0x5C)
        trailing = len(pattern) - len(pattern.rstrip("\\"))
        if trailing % 2 == 1:
            skipped += 1
            continue
        exp = db.execute("SELECT ? LIKE ? ESCAPE '\\'", (value, pattern)).fetchone()[0]
        got = R.like(value.encode(), pattern.encode(), 0x5C, unit_byte=False, tokens=toks)
        assert bool(exp) == got, (value, pattern)
        compared += 1
        matches += got
    assert skipped < 0.15 * 40_000, skipped
    assert matches >= 0.05 * compared and compared - matches >= 0.05 * compared, (compared, matches)


def test_byte_mode_equals_sqlite_on_ascii():
    """on ASCII a unit is a byte in both modes: the byte mode must agree with sqlite too"""
    db = sqlite3.connect(":memory:")
    db.execute("PRAGMA case_sensitive_like=ON")
    rng = np.random.default_rng(21)
    ab = ["a", "b", "_", "%", "ab"]
    for _ in range(5_000):
        value = "".join(ab[k] for k in rng.integers(0, 2, int(rng.integers(0, 8))))
        pattern = "".join(ab[k] for k in rng.integers(0, len(ab), int(rng.integers(0, 6))))
        exp = bool(db.execute("SELECT ? LIKE ? ESCAPE '\\'", (value, pattern)).fetchone()[0])
        assert R.like(value.encode(), pattern.encode(), 0x5C, unit_byte=True) == exp, (value, pattern)
        assert R.like(value.encode(), pattern.encode(), 0x5C, unit_byte=False) == exp, (value, pattern)


# ---- (b) negative controls ---------------------------------------------------------------------------------------------------------
# named cases: (value, pattern, escape, unit_byte, expected)
NAMED = {
    "underscore_is_a_unit": [(R.E2, b"_", 0x5C, False, True), (R.E2, b"__", 0x5C, False, False), (b"a" + R.E3 + b"b", b"a_b", 0x5C, False, True),
                             (R.E4, b"____", 0x5C, False, False), (R.E2, b"__", 0x5C, True, True), (b"\xc3", b"\xc3_", 0x5C, False, False)],
    "percent_may_be_empty": [(b"ab", b"a%b", 0x5C, False, True), (b"ab", b"%ab%", 0x5C, False, True), (b"", b"%", 0x5C, False, True),
                             (b"ab", b"ab%", 0x5C, False, True)],
    "anchors": [(b"xab", b"ab%", 0x5C, False, False), (b"abx", b"%ab", 0x5C, False, False), (b"xab", b"ab", 0x5C, False, False),
                (b"abx", b"a%b", 0x5C, False, False), (b"xab", b"a%b", 0x5C, False, False)],
    "case_sensitive": [(b"AB", b"ab", 0x5C, False, False), (b"Ab", b"%b", 0x5C, False, True), (b"aB", b"%b%", 0x5C, False, False)],
    "escape": [(b"a%b", b"a\\%b", 0x5C, False, True), (b"axb", b"a\\%b", 0x5C, False, False), (b"a_b", b"a\\_b", 0x5C, False, True),
               (b"axb", b"a\\_b", 0x5C, False, False), (b"a\\b", b"a\\\\b", 0x5C, False, True), (b"ab\\", b"ab\\", 0x5C, False, True),
               (b"a%b", b"a!%b", 0x21, False, True), (b"a!xb", b"a!%b", 0x21, False, False), (b"a\\x", b"a\\%", -1, False, True)],
}


def _wrong_matcher(flaw):
    """like_ref.like with one deliberate flaw"""
    def run(value, pattern, escape, unit_byte):
        if flaw == "underscore_is_a_unit":
            return R.like(value, pattern, escape, True)                       # `_` as one byte in unit mode
        if flaw == "case_sensitive":
            return R.like(value.lower(), pattern.lower(), escape, unit_byte)  # case folding
        if flaw == "escape":
            return R.like(value, pattern, -1, unit_byte)                      # escape ignored
        toks = R.parse(pattern, escape)
        if flaw == "percent_may_be_empty":                                    # `%` required to be non-empty
            toks = [x for t in toks for x in ((R.UNDER, R.PCT) if t == R.PCT else (t,))]
            return R.like(value, pattern, escape, True, toks)
        return R.like(value, pattern, escape, unit_byte, [R.PCT] + toks + [R.PCT])   # unanchored first and last segment
    return run


def test_named_cases_hold_for_the_reference():
    for name, cases in NAMED.items():
        for value, pattern, escape, unit_byte, exp in cases:
            assert R.like(value, pattern, escape, unit_byte) == exp, (name, value, pattern)


@pytest.mark.parametrize("flaw", sorted(NAMED))
def test_named_cases_reject_a_wrong_matcher(flaw):
    wrong = _wrong_matcher(flaw)
    assert any(wrong(v, p, e, u) != exp for v, p, e, u, exp in NAMED[flaw]), flaw


# ---- (c) the classifier --------------------------------------------------------------------------------------------------------------
def _kind(pattern, escape=0x5C):
    from databend_amd import _lib
    buf = (C.c_uint8 * max(len(pattern), 1)).from_buffer_copy(pattern or b"\0")
    return _lib.lib().dbhip_like_kind(buf, C.c_int32(len(pattern)), C.c_int32(escape))


KIND_TABLE = [
    (b"abc", 0x5C, R.EQUALS), (b"PROMO%", 0x5C, R.PREFIX), (b"%BRASS", 0x5C, R.SUFFIX), (b"%green%", 0x5C, R.CONTAINS),
    (b"%special%requests%", 0x5C, R.SEGMENTS), (b"MEDIUM POLISHED%", 0x5C, R.PREFIX), (b"%Customer%Complaints%", 0x5C, R.SEGMENTS),
    (b"forest%", 0x5C, R.PREFIX), (b"", 0x5C, R.SEGMENTS), (b"%", 0x5C, R.SEGMENTS), (b"%%", 0x5C, R.SEGMENTS), (b"%%a%%", 0x5C, R.CONTAINS),
    (b"a%%", 0x5C, R.PREFIX), (b"%%a", 0x5C, R.SUFFIX), (b"a_c", 0x5C, R.SEGMENTS), (b"_", 0x5C, R.SEGMENTS), (b"a_%", 0x5C, R.SEGMENTS),
    (b"%_a", 0x5C, R.SEGMENTS), (b"a%b", 0x5C, R.SEGMENTS), (b"a\\%", 0x5C, R.EQUALS), (b"a\\_b", 0x5C, R.EQUALS), (b"a\\_%", 0x5C, R.PREFIX),
    (b"\\%a", 0x5C, R.EQUALS), (b"%\\%", 0x5C, R.SUFFIX), (b"%\\", 0x5C, R.SUFFIX), (b"a\\", 0x5C, R.EQUALS), (b"\\", 0x5C, R.EQUALS),
    (b"\\\\%", 0x5C, R.PREFIX), (b"a\\%", -1, R.PREFIX), (b"a!%", 0x21, R.EQUALS), (b"a!_%", 0x21, R.PREFIX), (b"a%%b", 0x25, R.EQUALS),
    (b"a__b", 0x5F, R.EQUALS), (b"x" * 255, 0x5C, R.EQUALS), (b"%" + b"x" * 253 + b"%", 0x5C, R.CONTAINS), (R.P16, 0x5C, R.SEGMENTS),
    (b"%".join([b"a"] * 16), 0x5C, R.SEGMENTS), (b"\x00%", 0x5C, R.PREFIX), (b"%\xff", 0x5C, R.SUFFIX), (b"a%", 0, R.PREFIX), (b"\x00%", 0, R.EQUALS),
]


def test_classifier_table():
    for pattern, escape, exp in KIND_TABLE:
        assert R.kind_of(pattern, escape) == exp, (pattern, escape)
        assert _kind(pattern, escape) == exp, (pattern, escape)


def test_classifier_limits_and_errors():
    assert _kind(b"x" * 256) == -R.ERR_UNSUPPORTED
    assert _kind(b"%" * 256) == -R.ERR_UNSUPPORTED
    assert _kind(b"%".join([b"a"] * 17)) == -R.ERR_UNSUPPORTED
    assert _kind(b"%" + b"%".join([b"ab"] * 17) + b"%") == -R.ERR_UNSUPPORTED
    assert _kind(b"a", 256) == -R.ERR_INVALID and _kind(b"a", -2) == -R.ERR_INVALID
    from databend_amd import _lib
    buf = (C.c_uint8 * 1)()
    assert _lib.lib().dbhip_like_kind(buf, C.c_int32(-1), C.c_int32(0x5C)) == -R.ERR_INVALID
    assert _lib.lib().dbhip_like_kind(None, C.c_int32(0), C.c_int32(0x5C)) == R.SEGMENTS
    assert b"DBHIP_LIKE" not in _lib.lib().dbhip_last_error()


def test_classifier_agrees_with_the_reference_on_the_pool():
    rng = np.random.default_rng(22)
    pieces = [b"a", b"b", b"%", b"%", b"_", b"\\", b"!", R.E2]
    for pattern, escape in R.PATTERNS:
        assert _kind(pattern, escape) == R.kind_of(pattern, escape), (pattern, escape)
    for _ in range(3000):
        pattern = b"".join(pieces[k] for k in rng.integers(0, len(pieces), int(rng.integers(0, 40))))
        escape = [0x5C, 0x21, -1][int(rng.integers(0, 3))]
        assert _kind(pattern, escape) == R.kind_of(pattern, escape), (pattern, escape)


# ---- the kernels' matching steps on the host, with checked loads -------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("like") / "like_host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "like_host_check.cpp")])

    def run(cases):
        """cases: (pattern, escape, literal_kind, flags, value, before, behind, misalign) -> [(rc, kind, bit)]"""
        hx = lambda b: b.hex() if b else "-"   # noqa: E731
        text = "".join(f"{hx(p)} {e} {k} {f} {hx(v)} {hx(b0)} {hx(b1)} {m}\n" for p, e, k, f, v, b0, b1, m in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-400:]
        rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows
    return run


def _neighbours(pattern, escape):
    """bytes to put around a value so that a matcher that reads outside it answers wrongly: the pattern's own literal bytes"""
    lit = bytes(t for t in R.parse(pattern, escape) if isinstance(t, int)) or b"ab"
    return lit[-16:], lit[:16]


def test_matching_steps_equal_the_reference_on_the_pools(host_check):
    values = R.value_pool(1, n_random=250) + R.long_values(2)
    cases, exp = [], []
    for pi, (pattern, escape) in enumerate(R.PATTERNS):
        before, behind = _neighbours(pattern, escape)
        for flags in (0, 1, 2, 3):
            for vi, v in enumerate(values):
                if (vi + pi + flags) % 4 and len(v) < 200:      # a quarter of the short values per (pattern, flags); all long ones
                    continue
                cases.append((pattern, escape, -1, flags, v, before, behind, (vi * 7 + pi) % 16))
                exp.append(R.like(v, pattern, escape, bool(flags & 2)) != bool(flags & 1))
    got = host_check(cases)
    for c, g, e in zip(cases, got, exp):
        assert g[0] == 0 and g[1] == R.kind_of(c[0], c[1]) and bool(g[2]) == e, (c[:5], g, e)


def test_matching_steps_at_every_misalignment_and_length(host_check):
    """needles across every word boundary: values of 0 .. 70 and 250 .. 262 bytes with the needle at the start, in the middle and at the
    end, at each of the 16 misalignments, between neighbours that complete a partial needle"""
    rng = np.random.default_rng(3)
    patterns = [(b"abba", 0x5C), (b"abbab%", 0x5C), (b"%babba", 0x5C), (b"%abbab%", 0x5C), (b"%ab%_ba%", 0x5C), (b"ab%b_", 0x5C), (b"%a_b", 0x5C),
                (b"a%", 0x5C), (b"%b", 0x5C), (b"%bb%", 0x5C), (b"abbababbababba%", 0x5C), (b"%abbababbababba", 0x5C), (b"%abbababbababba%", 0x5C),
                (b"%abb%bab%", 0x5C), (b"ab%abba%b", 0x5C), (b"%abbab%abbababb%", 0x5C), (b"%a%b%a%b%", 0x5C)]
    cases, exp = [], []
    for ln in list(range(0, 71)) + list(range(250, 263)):
        base = bytes(rng.choice(np.frombuffer(b"ab", np.uint8), ln).tolist())
        for pattern, escape in patterns:
            lit = bytes(t for t in R.parse(pattern, escape) if isinstance(t, int))
            vals = {base}
            if ln >= len(lit):
                vals |= {lit + base[len(lit):], base[:ln - len(lit)] + lit, base[:(ln - len(lit)) // 2] + lit + base[(ln - len(lit)) // 2 + len(lit):]}
            for v in vals:
                for mis in range(16):
                    if (mis + ln) % 2 and ln > 40:
                        continue
                    cases.append((pattern, escape, -1, 0, v, lit[1:] or b"a", lit[:-1] or b"b", mis))
                    exp.append(R.like(v, pattern, escape))
    got = host_check(cases)
    assert sum(exp) > len(exp) // 10 and sum(exp) < len(exp) * 9 // 10
    for c, g, e in zip(cases, got, exp):
        assert g[0] == 0 and bool(g[2]) == e, (c, g, e)


def test_matching_steps_of_the_literal_needles(host_check):
    values = R.value_pool(4, n_random=150) + R.long_values(5)
    needles = [b"", b"a", b"ab", b"%", b"_", b"a%", b"a_b", b"\\", b"abab", b"ababa", b"a" * 12, b"a" * 13, R.E2, b"\xa9", R.P255_CONTAINS[1:-1], b"ab" * 100]
    cases, exp = [], []
    for needle in needles:
        for kind in (R.EQUALS, R.PREFIX, R.SUFFIX, R.CONTAINS):
            for vi, v in enumerate(values):
                cases.append((needle, -1, kind, vi & 1, v, needle[-8:] or b"a", needle[:8] or b"b", vi % 16))
                exp.append(R.str_match(kind, v, needle) != bool(vi & 1))
    got = host_check(cases)
    for c, g, e in zip(cases, got, exp):
        assert g[0] == 0 and bool(g[2]) == e, (c[:5], g, e)
    assert host_check([(b"a", -1, 4, 0, b"a", b"", b"", 0), (b"a" * 256, -1, 1, 0, b"a", b"", b"", 0)]) == [(1, -1, 0), (7, -1, 0)]
