"""CPU: databend_amd/csrc/dev_strfn.h — the row logic of the String function kernels (include/dbhip.h a22) — compiled for the host
under AddressSanitizer and UndefinedBehaviorSanitizer (tests/strfn_host_check.cpp) and held to tests/str_ref.py over the case list of
the GPU test (tests/strfn_cases.py). Every value lies in an exactly sized heap block at each of the four alignments, so a read outside
the value is reported; every answer is compared: the byte range and the full 16 bytes of the result view."""
import os
import subprocess

import pytest

from tests import str_ref as R
from tests import strfn_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "strfn_host_check.cpp")
INDEX, OFFSET = 7, 1000      # where the program says a long source value lies


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("strfn") / "strfn_host_check")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror"]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
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
        for r in rows:
            if len(r) == 3 and int(r[1]) <= int(r[0]):      # an empty range, wherever it lies
                r[:2] = ["0", "0"]
        return rows
    return run


def hx(b):
    return bytes(b).hex() if len(b) else "-"


def expect_slice(v, rng):
    s, e = rng
    if e <= s:
        s = e = 0
    return [str(s), str(e), R.slice_view(v, (s, e), INDEX, OFFSET).hex()]


def test_lengths(host):
    commands, exp = [], []
    for k, v in enumerate(K.values()):
        commands += [("val", hx(v), k % 4), ("len", 0), ("len", 1)]
        exp += [["ok"], [str(R.length(v))], [str(len(v))]]
    assert host(commands) == exp


@pytest.mark.parametrize("unit_byte", [0, 1])
def test_substr_left_right(host, unit_byte):
    commands, exp, what = [], [], []
    for k, v in enumerate(K.values()):
        commands.append(("val", hx(v), (k + unit_byte) % 4))
        exp.append(["ok"])
        what.append(None)
        for op, a, b in K.slice_args(v, bool(unit_byte)):
            commands.append(("sub", op, a, "-" if b is None else b, unit_byte))
            exp.append(expect_slice(v, R.slice_range(op, v, a, b, unit_byte=bool(unit_byte))))
            what.append((v[:40], len(v), op, a, b))
    got = host(commands)
    bad = [(w, g, e) for w, g, e in zip(what, got, exp) if g != e]
    assert not bad, (len(bad), bad[0])
    assert any(int(e[1]) - int(e[0]) == 12 for e in exp if len(e) == 3) and any(int(e[1]) - int(e[0]) == 13 for e in exp if len(e) == 3)


def test_trims(host):
    commands, exp, what = [], [], []
    for k, v in enumerate(K.values()):
        for lead in (k % 4, (k + 1) % 4):
            commands.append(("val", hx(v), lead))
            exp.append(["ok"])
            what.append(None)
            for pad in K.PADS:
                for op in (R.TRIM_LEADING, R.TRIM_TRAILING, R.TRIM_BOTH):
                    commands.append(("trim", op, hx(pad)))
                    exp.append(expect_slice(v, R.trim_range(v, pad, op)))
                    what.append((v[:40], len(v), op, pad[:20]))
    got = host(commands)
    bad = [(w, g, e) for w, g, e in zip(what, got, exp) if g != e]
    assert not bad, (len(bad), bad[0])
    assert any(e[:2] == ["0", "0"] for e in exp if len(e) == 3), "a value made only of pad"


def test_builds(host):
    rows = K.build_rows()
    got = host([("build", op, len(args)) + tuple(hx(a) for a in args) for op, args in rows])
    for (op, args), g in zip(rows, got):
        assert g == [str(int(R.non_ascii(args))), hx(R.build(op, args))], (op, [a[:20] for a in args], g)


def test_known_answers(host):
    got = host([("val", hx(b"hello"), 0), ("sub", 0, 2, 3, 0), ("sub", 0, -3, 2, 0), ("sub", 0, 0, 3, 0), ("sub", 0, 6, "-", 0), ("sub", 0, 5, "-", 0),
                ("sub", 0, -5, "-", 0), ("sub", 0, -6, "-", 0), ("val", hx(b"ababxab"), 0), ("trim", 5, hx(b"ab")), ("val", hx(b"aba"), 0), ("trim", 3, hx(b"ab")),
                ("val", hx(b"aaa"), 0), ("trim", 5, hx(b"aa"))])
    views = [bytes.fromhex(g[2]) for g in got if len(g) == 3]
    assert [v[4:4 + v[0]] for v in views] == [b"ell", b"ll", b"", b"", b"o", b"hello", b"", b"x", b"a", b"a"]
