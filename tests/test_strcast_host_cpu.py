"""CPU: databend_amd/csrc/dev_strcast.h — the row logic of the String cast kernels (include/dbhip.h a24) — compiled for the host under
AddressSanitizer and UndefinedBehaviorSanitizer (tests/strcast_host_check.cpp) and held to tests/strcast_ref.py over the case list of the
GPU test (tests/strcast_cases.py). Every value lies in an exactly sized heap block at each of the four alignments, so a read outside
the value is reported; every answer is compared: the status (ok / error / declined), the value, the text and the full 16 bytes of the
result view."""
import os
import random
import subprocess

import pytest

from databend_amd import _lib as T
from tests import strcast_cases as K
from tests import strcast_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "strcast_host_check.cpp")
MASK = (1 << 128) - 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("strcast") / "strcast_host_check")
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
        return rows
    return run


def hx(b):
    return bytes(b).hex() if len(b) else "-"


def image(v):
    """a number's two's complement image as the program prints it: the low and the high 64 bits"""
    v &= MASK
    return ["%016x" % (v & (2**64 - 1)), "%016x" % (v >> 64)]


def expect_parse(sp, value):
    st, v = R.parse(value, **sp)
    if sp["dtype"] != T.T_DEC128:
        v = v & (2**64 - 1) if sp["dtype"] != T.T_DEC64 else v     # a 64-bit target: the high word is the sign of a Decimal64 only
        if sp["dtype"] != T.T_DEC64:
            return [str(st), "%016x" % v, "%016x" % 0]
    return [str(st)] + image(v)


def test_case_list_holds_what_it_should():
    K.check_coverage()


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_parse(host, lead):
    commands, exp, what = [], [], []
    for name, sp, values in K.parse_groups():
        for k, v in enumerate(values):
            commands += [("val", hx(v), (k + lead) % 4), ("parse", sp["dtype"], sp["precision"], sp["scale"], int(sp["rounding"]), sp["offset_s"])]
            exp += [["ok"], expect_parse(sp, v)]
            what += [None, (name, v[:60], len(v))]
    got = host(commands)
    bad = [(w, g, e) for w, g, e in zip(what, got, exp) if g != e]
    assert not bad, (len(bad), bad[:3])


def test_format(host):
    commands, exp, what = [], [], []
    for name, sp, numbers in K.format_groups():
        for k, v in enumerate(numbers):
            t = R.text(v, sp["dtype"], sp["scale"], sp["offset_s"])
            lo, hi = image(v)
            commands.append(("fmt", sp["dtype"], sp["scale"], sp["offset_s"], lo, hi, 1000 + k))
            exp.append([str(R.ERROR if t is None else R.OK), hx(t or b""), R.view(t, 1000 + k).hex()])
            what.append((name, v))
    got = host(commands)
    bad = [(w, g, e) for w, g, e in zip(what, got, exp) if g != e]
    assert not bad, (len(bad), bad[:3])


def test_split_by_ten_to_the_nineteenth(host):
    """the 128-bit split the Decimal128 text rests on, against Python's divmod: edges and seeded random values up to 2^127"""
    rng = random.Random(24)
    vals = [0, 1, 10**19 - 1, 10**19, 10**19 + 1, 2**64 - 1, 2**64, 2**64 + 1, 10**38 - 1, 10**38, 2**127 - 1, 2**127, 5**19 * 2**19 - 1, 5**19, 2**19 - 1, 2**19]
    vals += [q * 10**19 + r for q in (1, 2**19 - 1, 2**19, 2**38, 2**57, 10**19 - 1) for r in (0, 10**19 - 1)]
    vals += [rng.getrandbits(rng.randint(1, 127)) for _ in range(4000)]
    got = host([("split", "%x" % (v >> 64), "%x" % (v & (2**64 - 1))) for v in vals])
    assert got == [[str(v // 10**19), str(v % 10**19)] for v in vals]


def test_round_trip(host):
    """parse(format(x)) == x through the host program, for every number of the format list that prints"""
    commands, exp = [], []
    for name, sp, numbers in K.format_groups():
        for v in numbers:
            t = R.text(v, sp["dtype"], sp["scale"], sp["offset_s"])
            if t is None or (sp["precision"] and abs(v) >= 10 ** sp["precision"]):
                continue
            commands += [("val", hx(t), len(t) % 4), ("parse", sp["dtype"], sp["precision"], sp["scale"], 0, sp["offset_s"])]
            low = image(v)
            if sp["dtype"] not in (T.T_DEC64, T.T_DEC128):
                low[1] = "%016x" % 0
            exp += [["ok"], ["0"] + low]
    assert len(commands) > 1000
    assert host(commands) == exp
