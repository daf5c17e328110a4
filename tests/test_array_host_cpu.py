"""CPU: databend_amd/csrc/dev_array.h — the row logic of the Array kernels (include/dbhip.h a29) — compiled for the host under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/array_host_check.cpp) and held to tests/array_ref.py over the case list of the
GPU test (tests/array_cases.py). Every run lies in an exactly sized heap block, every long String value in its own at each of the four
alignments, so a read outside the run or the value is reported; every answer is compared: the run of a pair of offsets, get's element
and validity, the first match, every reduction's value, validity and error flag, the result types."""
import os
import subprocess

import numpy as np
import pytest

from tests import array_cases as K
from tests import array_ref as R
from tests import float_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "array_host_check.cpp")
SANITIZED = []               # whether the program runs under the sanitizers (test_the_sanitizers_are_on reports it)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("array") / "array_host_check")
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


def run_command(tname, row):
    es = K.TYPES[tname][2]
    bits = "".join("0" if e is None else "1" for e in row) or "-"
    return ("run", es, hx(b"".join(K.encode(tname, e) for e in row)), bits)


def rows_of(tname, for_sum=False):
    """the case list's rows of a type: every shape, but of the 1027-row column only the first 130 rows (the host has no waves or blocks)"""
    return [row for name, rows in K.columns(tname, for_sum) for row in (rows[:130] if name == "n1027" else rows)]


def test_runs_and_positions(host):
    pairs = [(0, 0, 0), (0, 5, 5), (3, 3, 9), (5, 3, 9), (2, 10, 9), (9, 9, 9), (10, 10, 9), (0, 2 ** 64 - 1, 2 ** 64 - 1), (2 ** 64 - 1, 0, 5)]
    got = host([("row",) + p for p in pairs])
    assert got == [[str(int(not bad)), str(s), str(ln)] for s, ln, bad in (R.row_runs([a, b], ne)[0] for a, b, ne in pairs)]
    lens = [0, 1, 2, 63, 64, K.T, 2 ** 32, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    asks = [(i, ln) for ln in lens for i in sorted({0, 1, -1, 2, -2, R.INT64_MIN, R.INT64_MAX, R.INT64_MIN + 1, min(ln, R.INT64_MAX), -min(ln, 2 ** 63),
                                                     min(ln + 1, R.INT64_MAX), -min(ln + 1, 2 ** 63)})]
    got = host([("pos", i, ln) for i, ln in asks])
    for (i, ln), g in zip(asks, got):
        exp = i - 1 if 1 <= i <= ln else (ln + i if -ln <= i <= -1 else None)
        assert g == (["0", "0"] if exp is None else ["1", str(exp)]), (i, ln, g)


@pytest.mark.parametrize("tname", list(K.NUMBERS))
def test_get(host, tname):
    es = K.TYPES[tname][2]
    commands, exp = [], []
    for row in rows_of(tname):
        commands.append(run_command(tname, row))
        exp.append(["ok"])
        for i in K.get_indexes([row])[0]:
            v = R.get(row, i)
            commands.append(("get", i))
            in_range = 1 <= i <= len(row) or -len(row) <= i <= -1
            # a NULL element inside the run: validity 0, and the value as stored (the zero value here)
            exp.append([str(int(v is not None)), hx(K.encode(tname, v) if in_range else bytes(es))])
    got = host(commands)
    bad = [(c, g, e) for c, g, e in zip(commands, got, exp) if g != e]
    assert not bad, (len(bad), bad[0][1:], bad[0][0][:2])


@pytest.mark.parametrize("tname", list(K.NUMBERS))
def test_find(host, tname):
    mode = {"f32": 1, "f64": 2}.get(tname, 0)
    commands, exp = [], []
    for name, rows in K.columns(tname):
        rows = rows[:130] if name == "n1027" else rows
        for row, x in zip(rows, K.needles(tname, rows, 5)):
            commands += [run_command(tname, row), ("find", mode, "null" if x is None else hx(K.encode(tname, x)))]
            exp += [["ok"], [str(R.indexof(row, x, K.is_float(tname)))]]
    if tname == "i64":
        rows, x, want = K.indexof_lane_rows()
        for row, w in zip(rows, want):
            commands += [run_command(tname, row), ("find", 0, hx(K.encode(tname, x)))]
            exp += [["ok"], [str(w)]]
    got = host(commands)
    bad = [(g, e) for g, e in zip(got, exp) if g != e]
    assert not bad, (len(bad), bad[0])
    assert sum(1 for e in exp if e != ["ok"] and int(e[0]) > 1) > 5


def check_reduce(tname, kind, row, g):
    """one answer of `red` against the reference"""
    exp = R.reduce(kind, row, tname)
    rt = K.result_type(kind, tname)
    valid, err, value = int(g[0]), int(g[1]), K.decode(rt, bytes.fromhex(g[2]))
    if exp is None or exp == R.OVERFLOW:
        return valid == 0 and err == int(exp == R.OVERFLOW) and value == 0
    if not valid or err:
        return False
    if K.is_float(tname) and kind == R.SUM:
        return F.sum_ok(value, exp)
    if K.is_float(tname) and kind in (R.MIN, R.MAX):
        vals = [float(e) for e in row if e is not None]
        return F.same_value(value, exp, K.TYPES[tname][1], F.one_signed_zero(vals))
    return value == exp


@pytest.mark.parametrize("tname", list(K.NUMBERS))
def test_reduce(host, tname):
    commands, checks = [], []
    rows = rows_of(tname, for_sum=True) + (rows_of(tname) if K.is_float(tname) else []) + (K.dec128_overflow_rows() if tname == "dec128" else [])
    for r, row in enumerate(rows):
        commands.append(run_command(tname, row))
        checks.append(None)
        for kind in (R.COUNT, R.SUM, R.MIN, R.MAX):
            if K.result_type(kind, tname) is None:
                continue
            if K.is_float(tname) and kind == R.SUM and R.reduce(kind, row, tname) is not None and R.reduce(kind, row, tname)[0] == "out of bounds":
                continue                                      # a MIN / MAX row (+-DBL_MAX): no SUM is judged over it
            for split in sorted({0, len(row) // 3, len(row)}):
                commands.append(("red", kind, K.TYPES[tname][0], split))
                checks.append((kind, row))
    got = host(commands)
    bad = [(c, g) for c, g, k in zip(commands, got, checks) if (g != ["ok"] if k is None else not check_reduce(tname, k[0], k[1], g))]
    assert not bad, (len(bad), bad[0])


def test_reduce_result_types(host):
    kinds = (R.COUNT, R.SUM, R.MIN, R.MAX)
    commands = [("rtype", k, K.TYPES[t][0], 20, 3) for t in K.TYPES for k in kinds] + [("rtype", k, c, 0, 0) for k in kinds for c in (1, 17, 0, 18)] + [("rtype", 4, 5, 0, 0)]
    got = host(commands)
    exp = []
    for t in K.TYPES:
        for k in kinds:
            rt = None if t == "string" else K.result_type(k, t)
            if rt is None:
                exp.append(["1", "0", "0", "0"])
            elif k == R.SUM and t in ("dec64", "dec128"):
                exp.append(["0", str(K.TYPES[rt][0]), "18" if t == "dec64" else "38", "3"])
            elif k == R.COUNT or k == R.SUM:
                exp.append(["0", str(K.TYPES[rt][0]), "0", "0"])
            else:
                exp.append(["0", str(K.TYPES[rt][0]), "20", "3"])
    exp += [[rc, "0", "0", "0"] for _ in kinds for rc in ("7", "7", "1", "1")] + [["1", "0", "0", "0"]]
    assert got == exp


def test_string_find(host):
    rng = np.random.default_rng(3)
    commands, exp = [], []
    for lead in range(4):
        for dirty in (0, 1):
            for row in K.column("string", [0, 1, 5, 30, 64, 65], 20 + lead):
                bits = "".join("0" if e is None else "1" for e in row) or "-"
                vals = [hx(e) if e is not None else hx(K.STRINGS[int(rng.integers(0, len(K.STRINGS)))]) for e in row]     # bytes under a NULL
                commands.append(("strs", lead, dirty, bits) + tuple(vals))
                exp.append(["ok"])
                for nd in K.STR_NEEDLES + [b"abcdXfghijklm", b"abcdefghijklmno", bytes(range(1, 255)) + b"\x01", b"zz"]:
                    commands.append(("finds", hx(nd)))
                    exp.append([str(R.indexof(row, nd))])
    # a view that names a buffer past the table matches nothing, whatever its length and prefix say
    commands += [("strs", 0, 0, "-", "!", hx(b"abcd" + b"x" * 16)), ("finds", hx(b"abcd" + b"x" * 16)), ("finds", hx(b"abcd" + b"\0" * 16))]
    exp += [["ok"], ["2"], ["0"]]
    got = host(commands)
    bad = [(c[:3], g, e) for c, g, e in zip(commands, got, exp) if g != e]
    assert not bad, (len(bad), bad[0])
    assert sum(1 for e in exp if e != ["ok"] and e != ["0"]) > 50


def test_the_sanitizers_are_on(host):
    """the fallback build without them is allowed only where their runtime is missing; say which build ran"""
    print("array_host_check built with -fsanitize=address,undefined:", SANITIZED[0])
    assert SANITIZED and isinstance(SANITIZED[0], bool)
