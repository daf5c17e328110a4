"""CPU: databend_amd/csrc/dev_inlist.h — the row logic of the IN-list kernels (include/dbhip.h a23) — compiled for the host under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/inlist_host_check.cpp) and held to tests/inlist_ref.py: tables are built and
probed, String tails compared for values in exactly sized heap blocks at each of the four alignments, and the Python restatement of
the hash and the slot count (which the GPU tests use to build colliding lists) is compared with the header's."""
import os
import random
import struct
import subprocess

import pytest

from databend_amd import _lib as L
from tests import inlist_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "inlist_host_check.cpp")
TYPE = {"raw": L.T_I64, "f32": L.T_F32, "f64": L.T_F64, "d128": L.T_DEC128, "str": L.T_STRING}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inlist") / "inlist_host_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr[-2000:]    # only a missing runtime may fall back
        subprocess.check_call(base + ["-o", exe, SRC])

    def run(commands):
        text = "".join(" ".join(str(w) for w in c) + "\n" for c in commands)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        rows = [line.split() for line in out.stdout.splitlines()]
        assert len(rows) == len(commands)
        return rows
    return run


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def enc(kind, x):
    if kind == "str":
        return bytes(x).hex() if len(x) else "-"
    if kind == "f32":
        return struct.pack("<f", x).hex()
    if kind == "f64":
        return struct.pack("<d", x).hex()
    return (int(x) & ((1 << (128 if kind == "d128" else 64)) - 1)).to_bytes(16 if kind == "d128" else 8, "little").hex()


def run_set(host, kind, items, probes, force_table=False):
    """builds the set, probes every value (Strings at all four alignments) and compares with the reference; returns the build line"""
    leads = (0, 1, 2, 3) if kind == "str" else (0,)
    cmds = [("new", kind, int(force_table))] + [("add", enc(kind, e)) for e in items] + [("build",)]
    cmds += [("probe", enc(kind, p), lead) for p in probes for lead in leads]
    got = host(cmds)
    build = [int(x) for x in got[len(items) + 1]]
    answers = [bool(int(g[0])) for g in got[len(items) + 2:]]
    exp, _ = R.evaluate(TYPE[kind], probes, None, items)
    exp = [e for e in exp for _ in leads]
    bad = [(p, lead) for (p, lead), g, e in zip([(p, lead) for p in probes for lead in leads], answers, exp) if g != e]
    assert not bad, (len(bad), bad[:3])
    assert any(exp) and not all(exp), "a case sees both answers"
    return build


def int_neighbours(items):
    return sorted({x + d for x in items for d in (-1, 0, 1)})


def str_neighbours(items):
    out = set()
    for s in items:
        out.add(s)
        out.add(s + b"!")                                   # one byte longer
        if s:
            out.add(s[:-1])                                 # one byte shorter
            out.add(s[:-1] + bytes([s[-1] ^ 1]))            # the last byte changed
    return sorted(out)


def test_python_restatement_of_hash_and_slots(host):
    rng = random.Random(1)
    cases = [("raw", [0, 1, -1, 1 << 63, rng.getrandbits(64)]), ("f32", [0.0, -0.0, 1.5, float("nan"), float("inf")]),
             ("f64", [0.0, -0.0, 1e300, float("nan")]), ("d128", [0, -1, 1 << 64, -(1 << 100), rng.getrandbits(127)]),
             ("str", [b"", b"a", b"abcdefghijkl", b"abcdefghijklm", b"z" * 255])]
    for kind, values in cases:
        for n in (3, 17, 40):
            fill = [bytes([65 + k % 26]) * (1 + k % 30) + bytes([k]) for k in range(n)] if kind == "str" else ([float(k) for k in range(n)] if kind[0] == "f" else list(range(100, 100 + n)))
            got = host([("new", kind, 1)] + [("add", enc(kind, e)) for e in fill] + [("build",)] + [("hash", enc(kind, v)) for v in values])
            path, slots, distinct, _ = (int(x) for x in got[n + 1])
            assert (path, slots, distinct) == (2, R.inl_slots(n), n)
            for v, g in zip(values, got[n + 2:]):
                k0, k1, _ = R.key_image(TYPE[kind], v)
                assert (int(g[0], 16), int(g[1])) == (R.inl_hash(k0, k1), R.inl_hash(k0, k1) & (slots - 1)), (kind, v)


def test_path_threshold(host):
    assert run_set(host, "raw", list(range(R.COMPARE_MAX)), [0, R.COMPARE_MAX])[:3] == [1, 0, R.COMPARE_MAX]
    assert run_set(host, "raw", list(range(R.COMPARE_MAX + 1)), [0, R.COMPARE_MAX + 1])[:3] == [2, R.inl_slots(R.COMPARE_MAX + 1), R.COMPARE_MAX + 1]
    assert run_set(host, "raw", [5, 5, 5, 7], [5, 6, 7])[:3] == [1, 0, 2], "duplicates are stored once"
    got = host([("new", "raw", 0), ("build",), ("probe", enc("raw", 0), 0), ("new", "raw", 1), ("build",), ("probe", enc("raw", -1), 0)])
    assert [g[0] for g in (got[2], got[5])] == ["0", "0"], "IN () holds nothing, the empty slots' own key included"


@pytest.mark.parametrize("kind", ["raw", "d128"])
def test_eight_elements_with_one_home_slot(host, kind):
    slots = 64
    hit = R.colliding(TYPE[kind], 8, slots, 21, range(1000, 1 << 20))
    fill = [x for x in range(10, 40) if x not in hit][:12]
    items = hit + fill                                        # 20 elements: a table of 64 slots
    assert run_set(host, kind, items, int_neighbours(items))[:2] == [2, slots]
    got = host([("new", kind, 0)] + [("add", enc(kind, e)) for e in items] + [("build",)] + [("where", enc(kind, e)) for e in hit])
    at = sorted(int(g[0]) for g in got[len(items) + 2:])
    assert at[0] == 21 and at[-1] >= 28 and len(set(at)) == 8, at


def test_a_probe_run_that_wraps_past_the_tables_end(host):
    slots = 64
    hit = R.colliding(L.T_I64, 5, slots, slots - 1, range(1, 1 << 20))
    items = hit + list(range(2000, 2040))
    items = [x for x in items if x in hit or R.home(L.T_I64, x, slots) not in (0, 1, 2, 3, slots - 1)][:20]
    assert run_set(host, "raw", items, int_neighbours(items))[:2] == [2, slots]
    got = host([("new", "raw", 0)] + [("add", enc("raw", e)) for e in items] + [("build",)] + [("where", enc("raw", e)) for e in hit])
    assert sorted(int(g[0]) for g in got[len(items) + 2:]) == [0, 1, 2, 3, slots - 1]


def test_a_table_of_exactly_1024_elements(host):
    rng = random.Random(7)
    items = sorted({rng.getrandbits(64) - (1 << 63) for _ in range(1100)})[:1024]
    assert run_set(host, "raw", items, int_neighbours(items))[:3] == [2, 2048, 1024]
    strs = [b"%05d" % k + b"x" * (k % 23) for k in range(1024)]
    assert run_set(host, "str", strs, str_neighbours(strs[::37]) + [b"", b"0"])[:3] == [2, 2048, 1024]


@pytest.mark.parametrize("force_table", [False, True])
def test_strings_tails_prefixes_and_long_elements(host, force_table):
    a = b"same" + b"-" * 35 + b"A"
    b = b"same" + b"-" * 35 + b"B"                            # equal in length and first four bytes
    items = [b"", b"a", b"ab", b"abcdefghijkl", b"abcdefghijklm", b"abcdefghijklmnop", a, b, b"q" * 255, "naïve".encode(), a]
    probes = str_neighbours(items) + [b"same" + b"-" * 36, b"q" * 256, b"q" * 4000, b"abcd"]
    build = run_set(host, "str", items, probes, force_table)
    assert build[0] == (2 if force_table or len(items) - 1 > R.COMPARE_MAX else 1) and build[2] == len(items) - 1
    got = host([("new", "str", int(force_table))] + [("add", enc("str", e)) for e in items] + [("build",)] +
               [("bad", enc("str", e)) for e in items])
    assert [g[0] for g in got[len(items) + 2:]] == ["1" if len(e) <= 12 else "0" for e in items], "a long view that points nowhere is no member"


@pytest.mark.parametrize("force_table", [False, True])
def test_floats(host, force_table):
    nan2 = struct.unpack("<d", struct.pack("<Q", 0xFFF0000000000123))[0]
    items = [float("nan"), 0.0, float("inf"), 1.5]
    probes = [nan2, float("nan"), -0.0, 0.0, float("inf"), -float("inf"), 1.5, -1.5, 5e-324]
    run_set(host, "f64", items, probes, force_table)
    nan3 = struct.unpack("<f", struct.pack("<I", 0x7F800001))[0]
    run_set(host, "f32", [nan3, -0.0, -float("inf")], [float("nan"), 0.0, -0.0, float("inf"), -float("inf"), f32(1e-45)], force_table)


@pytest.mark.parametrize("kind", ["raw", "d128"])
@pytest.mark.parametrize("force_table", [False, True])
def test_a_value_equal_to_the_sentinel(host, kind, force_table):
    probes = [-1, 0, -2, 1] + ([(1 << 64) - 1, -(1 << 64) - 1] if kind == "d128" else [])    # (d128: all ones in one word only)
    assert run_set(host, kind, [-1, 3, 4], probes, force_table)[3] == 1, "the list holds the sentinel: kept as a flag, not stored"
    assert run_set(host, kind, [3, 4], probes + [3], force_table)[3] == 0, "and a row that equals it is no member of a list without it"
