"""CPU: databend_amd/csrc/dev_strsearch.h — the row logic of the String search and rewrite kernels (include/dbhip.h a28) — compiled for
the host under AddressSanitizer and UndefinedBehaviorSanitizer (tests/strsearch_host_check.cpp) and held to tests/strsearch_ref.py over
the case list of the GPU test (tests/strsearch_cases.py). Every value lies in an exactly sized heap block at each of the four
alignments, so a read outside the value is reported; every answer is compared: the position, the field's byte range and the full 16
bytes of its view, the rewrite's length and bytes."""
import os
import subprocess

import pytest

from tests import str_ref as S
from tests import strsearch_cases as K
from tests import strsearch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "strsearch_host_check.cpp")
INDEX, OFFSET = 7, 1000      # where the program says a long source value lies
SANITIZED = []               # whether the program runs under the sanitizers (test_the_sanitizers_are_on reports it)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("strsearch") / "strsearch_host_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    SANITIZED.append(san.returncode == 0)
    if san.returncode != 0:
        assert "sanitize" in san.stderr or "asan" in san.stderr or "ubsan" in san.stderr, san.stderr[-2000:]    # only a missing runtime may fall back
        subprocess.check_call(base + ["-o", exe, SRC])

    def run(commands):
        """commands: lists of words -> one output line (split) per command"""
        text = "".join(" ".join(str(w) for w in c) + "\n" for c in commands)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        rows = [line.split() for line in out.stdout.splitlines()]
        assert len(rows) == len(commands)
        return rows
    return run


def hx(b):
    return bytes(b).hex() if len(b) else "-"


def per_value(rows, command, expect):
    """rows (value first) -> every run of rows of one value at each of the four alignments: a `val` and then the run's commands"""
    runs = []
    for row in rows:
        if not runs or runs[-1][0] != row[0]:
            runs.append((row[0], [], [], []))
        runs[-1][1].append(command(row))
        runs[-1][2].append(expect(row))
        runs[-1][3].append(tuple(x[:40] if isinstance(x, bytes) else x for x in row))
    commands, exp, what = [], [], []
    for v, c, e, w in runs:
        for lead in range(4):
            commands += [("val", hx(v), lead)] + c
            exp += [["ok"]] + e
            what += [None] + w
    return commands, exp, what


def compare(host, commands, exp, what):
    got = host(commands)
    bad = [(w, g, e) for w, g, e in zip(what, got, exp) if g != e]
    assert not bad, (len(bad), bad[0])


@pytest.mark.parametrize("unit_byte", [0, 1])
def test_position(host, unit_byte):
    compare(host, *per_value(K.position_rows(bool(unit_byte)), lambda r: ("pos", hx(r[1]), r[2], unit_byte),
                             lambda r: [str(R.position(r[0], r[1], r[2], bool(unit_byte)))]))


def expect_split(v, delim, part):
    rng = R.split_range(v, delim, part)
    if rng is None:
        return ["0", "0", "0", S.ZERO_VIEW.hex()]
    return ["1", str(rng[0]), str(rng[1]), S.slice_view(v, rng, INDEX, OFFSET).hex()]


def test_split_part(host):
    def norm(rows):
        for r in rows:
            if len(r) == 4 and r[0] == "1" and r[1] == r[2]:      # an empty field, wherever it lies
                r[1:3] = ["0", "0"]
        return rows
    commands, exp, what = per_value(K.split_rows(), lambda r: ("split", hx(r[1]), r[2]), lambda r: expect_split(*r))
    got = norm(host(commands))
    bad = [(w, g, e) for w, g, e in zip(what, got, norm(exp)) if g != e]
    assert not bad, (len(bad), bad[0])


def expect_rewrite(op, v, k, x, y, unit_byte):
    out = R.rewrite(op, v, k, x, y, unit_byte)
    return ["toolong", "-"] if out == R.TOO_LONG else [str(len(out)), hx(out)]


def test_rewrites(host):
    compare(host, *per_value([(v, op, k, x, y, ub) for op, v, k, x, y, ub in K.rewrite_rows()], lambda r: ("rw", r[1], r[2], hx(r[3]), hx(r[4]), int(r[5])),
                             lambda r: expect_rewrite(r[1], r[0], r[2], r[3], r[4], r[5])))


def test_every_alignment(host):
    """one value that is searched, split and rewritten at each of the four leads"""
    v = b"xy" + S.E3 + b"-ab-" + S.E2 * 9 + b"-tail"
    commands, exp = [], []
    for lead in range(4):
        commands += [("val", hx(v), lead), ("pos", hx(b"-"), 7, 0), ("split", hx(b"-"), -2), ("rw", R.REVERSE, 0, "-", "-", 0), ("rw", R.LPAD, 40, hx(S.E3), "-", 0)]
        exp += [["ok"], [str(R.position(v, b"-", 7))], expect_split(v, b"-", -2), expect_rewrite(R.REVERSE, v, 0, b"", b"", False),
                expect_rewrite(R.LPAD, v, 40, S.E3, b"", False)]
    assert host(commands) == exp


def test_known_answers(host):
    got = host([("val", hx(b"aaaaa"), 1), ("rw", R.REPLACE, 0, hx(b"aa"), hx(b"b"), 0), ("val", hx(b"hi"), 2), ("rw", R.LPAD, 5, hx(b"xy"), "-", 0),
                ("rw", R.RPAD, 1, hx(b"x"), "-", 0), ("rw", R.LPAD, 5, "-", "-", 0), ("rw", R.REPEAT, R.INT64_MAX, "-", "-", 0), ("rw", R.LPAD, R.INT64_MAX, hx(b"ab"), "-", 0),
                ("val", hx(b"abc"), 3), ("pos", "-", 4, 0), ("pos", "-", 5, 0), ("val", hx(b"a,b,,c"), 0), ("split", hx(b","), 0), ("split", hx(b","), -5)])
    assert got == [["ok"], ["3", hx(b"bba")], ["ok"], ["5", hx(b"xyxhi")], ["1", hx(b"h")], ["0", "-"], ["toolong", "-"], ["toolong", "-"],
                   ["ok"], ["4"], ["0"], ["ok"], ["1", "0", "1", S.view(b"a").hex()], ["0", "0", "0", S.ZERO_VIEW.hex()]]


def test_the_sanitizers_are_on(host):
    """the fallback build without them is allowed only where their runtime is missing; say which build ran"""
    print("strsearch_host_check built with -fsanitize=address,undefined:", SANITIZED[0])
    assert SANITIZED and isinstance(SANITIZED[0], bool)
