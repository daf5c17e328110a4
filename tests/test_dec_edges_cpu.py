"""CPU: the directed Decimal64 / Decimal128 cases of tests/dec_edge_cases.py. The census (every reachable branch of dec_row has a size
pair, every edge label enough rows), then two statements against the Python reference tests/dec256_ref.py on every row: the oracle
(orc_decimal_arith) and the host twin of the product's own dev_decimal.h / dev_common.h (tests/dec_host_check.cpp, g++), the latter a
second time built with -fsanitize=undefined,address."""
import os
import subprocess

import pytest

from tests import dec256_ref as R
from tests import dec_edge_cases as E
from tests.test_dec256_cpu import oracle_binary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "databend_amd", "csrc")


def describe(case, i=None):
    s = f"{E.OPNAME[case['op']]} {case['x'][0]}{case['x'][2]} {case['y'][0]}{case['y'][2]} -> {case['ret']}"
    if i is not None:
        s += f" row {i}: x = {case['x'][3][i]} y = {case['y'][3][i]} expected {case['expected'][i]} labels {sorted(case['labels'][i])}"
    return s


def test_census_every_branch_and_edge_is_carried():
    cases = E.cases()
    have = {c["label"] for c in cases}
    reach = E.reachable()
    assert not reach - have, f"reachable (op, T, precision, shift) labels without a size pair: {sorted(reach - have)}"
    assert not have - reach
    # plus / minus never shift: the eight labels the enumeration cannot reach
    assert E.all_case_labels() - reach == {(o, t, m, "shift+") for o in ("plus", "minus") for t in (64, 128) for m in ("maxp", "lowp")}
    cen = E.census(cases)
    thin = {k: cen.get(k, 0) for k in E.required_edge_labels() if cen.get(k, 0) < E.MIN_ROWS}
    assert not thin, f"edge labels on fewer than {E.MIN_ROWS} rows: {thin}\ncensus: {sorted(cen.items())}"
    assert len(cases) <= 48 and all(len(c["expected"]) <= 700 for c in cases)
    for c in cases:   # every case has rows that compute and, where its form can raise, rows that raise
        assert sum(e is not None for e in c["expected"]) >= 8, describe(c)


def test_the_labels_mean_what_they_say():
    """spot checks of the label arithmetic against the reference on rows built by hand"""
    dec = ("dec", (38, 12)), ("dec", (20, 0))
    lab = lambda x, y, op=R.OP_DIVIDE, s=dec: E.row_labels(op, s[0][0], s[0][1], s[1][0], s[1][1], x, y)   # noqa: E731
    assert {"tie:exact:++", "D:2^64", "D>=2^64", "path:native128", "N<2^128"} <= lab(2 ** 63, 2 ** 64)
    assert R.binary(R.OP_DIVIDE, 2 ** 63, "dec", (38, 12), 2 ** 64, "dec", (20, 0))[0] == 1          # half away from zero
    assert R.binary(R.OP_DIVIDE, -(2 ** 63), "dec", (38, 12), 2 ** 64, "dec", (20, 0))[0] == -1
    assert R.binary(R.OP_DIVIDE, 2 ** 63 - 1, "dec", (38, 12), 2 ** 64, "dec", (20, 0))[0] == 0
    assert "tie:below:+-" in lab(2 ** 63 - 1, -(2 ** 64)) and "tie:above:-+" in lab(-(2 ** 63) - 1, 2 ** 64)
    assert {"qlo:max", "qhi:nonzero", "rem:D-1", "path:2by1"} <= lab((2 * 2 ** 64 + 2 ** 64 - 1) * 3 + 2 - 1, 3)
    assert "raise:div0:-" in lab(-5, 0)
    m18 = ("dec", (12, 8)), ("dec", (10, 8))
    assert "range:mul18:+past" in lab(2 * 10 ** 18 - 1, 5000, R.OP_MULTIPLY, m18) and "range:mul18:-max" in lab(2 * 10 ** 18 - 2, -5000, R.OP_MULTIPLY, m18)
    with pytest.raises(R.RowError):
        R.binary(R.OP_MULTIPLY, 2 * 10 ** 18 - 1, "dec", (12, 8), 5000, "dec", (10, 8))
    assert R.binary(R.OP_MULTIPLY, 2 * 10 ** 18 - 2, "dec", (12, 8), -5000, "dec", (10, 8))[0] == -(10 ** 18 - 1)


@pytest.mark.parametrize("t", [64, 128])
def test_the_oracle_equals_the_python_statement(t):
    n = 0
    for case in E.cases():
        if case["label"][1] != t:
            continue
        got, cnt = oracle_binary(case)
        bad = [i for i, (g, e) in enumerate(zip(got, case["expected"])) if g != e]
        assert not bad, (describe(case, bad[0]), got[bad[0]], len(bad))
        assert cnt == sum(e is None for e in case["expected"])
        n += len(got)
    assert n > 1000


# ------------------------------------------------------------------------------------------------------------ host twin
def cut_headers(common=None, decimal=None):
    """the text under test: the u256 / division / pow10_i128 part of dev_common.h and the row functions of dev_decimal.h"""
    common = open(os.path.join(CSRC, "dev_common.h")).read() if common is None else common
    decimal = open(os.path.join(CSRC, "dev_decimal.h")).read() if decimal is None else decimal
    a = common.index("struct u256 {")
    b, c = decimal.index("struct DecOp {"), decimal.index("// host: decode one decimal call node")
    return common[a:] + "\n" + decimal[b:c]


def build_twin(tmp, text, sanitize=False):
    d = os.path.join(str(tmp), "san" if sanitize else "plain")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "dec_under_test.h"), "w") as f:
        f.write(text)
    exe = os.path.join(d, "dec_host_check")
    flags = ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", d, "-o", exe, os.path.join(ROOT, "tests", "dec_host_check.cpp")])
    return exe


def hex128(v):
    return "%032x" % (v & ((1 << 128) - 1))


def twin_stream(cases):
    lines = []
    for c in cases:
        (xk, _, xs, xv), (yk, _, ys, yv) = c["x"], c["y"]
        left, right, ret = R.result_size(c["op"], xs, ys)
        head = f"{c['op']} {int(xk == 'dec')} {xs[1]} {int(yk == 'dec')} {ys[1]} {left[0]} {left[1]} {right[0]} {right[1]} {ret[0]} {ret[1]}"
        lines += [f"{head} {hex128(x)} {hex128(y)}" for x, y in zip(xv, yv)]
    return "\n".join(lines) + "\n"


def run_twin(exe, cases):
    """-> per case the list of values (None = the row raised)"""
    # (the program allocates nothing; the leak check at exit needs ptrace rights a test runner may not have)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], input=twin_stream(cases), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    out, it = [], iter(r.stdout.split("\n"))
    for c in cases:
        vals = []
        for _ in c["expected"]:
            w = next(it).split()
            assert w[0] in ("ok", "err"), w
            if w[0] == "err":
                vals.append(None)
            else:
                v = int(w[1], 16)
                vals.append(v - (1 << 128) if v >> 127 else v)
        out.append(vals)
    return out


def twin_mismatches(exe, cases):
    return [(ci, i) for ci, (c, got) in enumerate(zip(cases, run_twin(exe, cases))) for i, (g, e) in enumerate(zip(got, c["expected"])) if g != e]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan_asan"])
def test_the_host_twin_of_dev_decimal_equals_the_python_statement(tmp_path, sanitize):
    """dec_row (and dec_row_nodiv where nothing divides) of the product's headers, compiled for the host: every row of every case.
    The sanitizer build is a stand-alone program run as a plain subprocess; any report ends it with a non-zero status."""
    cases = E.cases()
    exe = build_twin(tmp_path, cut_headers(), sanitize)
    bad = twin_mismatches(exe, cases)
    assert not bad, (len(bad), [describe(cases[ci], i) for ci, i in bad[:5]])
