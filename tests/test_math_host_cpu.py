"""CPU: databend_amd/csrc/dev_math.h — the one implementation of the math functions (include/dbhip.h a26), which the kernels of
k_math.hip inline — compiled for the host in a stand-alone program (tests/math_host_check.cpp) and held to tests/math_ref.py bit for
bit on the whole shared case list (tests/math_cases.py): every (function, number type, digits) and every (function, DecimalSize,
digits). Where the compiler links it the program is built with -fsanitize=address,undefined -fno-sanitize-recover=all. Nothing is
loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import math_cases as K
from tests import math_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Host:
    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.files = exe, tmp, {}

    def put(self, key, raw):
        """file of raw bytes (cached by key)"""
        if key not in self.files:
            path = os.path.join(self.tmp, "in%d.bin" % len(self.files))
            with open(path, "wb") as f:
                f.write(raw)
            self.files[key] = path
        return self.files[key]

    def run(self, *words):
        out = os.path.join(self.tmp, "out.bin")
        p = subprocess.run([self.exe] + [str(w) for w in words] + [out], capture_output=True, text=True)
        assert p.returncode == 0, (words, p.returncode, p.stderr[-800:])
        with open(out, "rb") as f:
            return f.read()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("math"))
    exe = os.path.join(tmp, "math_host_check")
    src = os.path.join(ROOT, "tests", "math_host_check.cpp")
    base = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return Host(exe, tmp)


def ints_to_raw(values, bits):
    return b"".join((int(v) & ((1 << bits) - 1)).to_bytes(bits // 8, "little") for v in values)


def raw_to_ints(raw, bits):
    w = bits // 8
    return [int.from_bytes(raw[i:i + w], "little", signed=True) for i in range(0, len(raw), w)]


@pytest.mark.parametrize("typ", R.NUMBERS)
def test_numbers(host, typ):
    values = K.numbers(typ)
    f = host.put(("num", typ), values.tobytes())
    calls = K.number_calls(typ)
    assert len(calls) == (2 + 3 + 24 if typ not in R.UNSIGNED else 1 + 3 + 24)
    for fn, digits in calls:
        exp = R.number(fn, values, digits)
        got = np.frombuffer(host.run("num", fn, typ, digits, f), dtype=exp.dtype)
        bad = R.same_bits(got, exp, nan_any=fn != R.ABS)
        assert not len(bad), (R.NAMES[fn], typ, digits, len(bad), values[bad[0]], got[bad[0]], exp[bad[0]])


@pytest.mark.parametrize("p,s", K.DEC_SIZES)
def test_decimals(host, p, s):
    bits = 64 if p <= 18 else 128
    values = K.decimal_values(p)
    f = host.put(("dec", p), ints_to_raw(values, bits))
    for fn, digits in K.decimal_calls(p, s):
        exp = R.decimal(fn, values, p, s, digits)
        got = raw_to_ints(host.run("dec", fn, bits, p, s, digits, f), 8 if fn == R.SIGN else bits)
        bad = [i for i in range(len(values)) if got[i] != exp[i]]
        assert len(got) == len(exp) and not bad, (R.NAMES[fn], p, s, digits, len(bad), values[bad[0]], got[bad[0]], exp[bad[0]])


def test_decimals_at_the_ends_of_the_storage(host):
    """bit patterns beyond 10^p: nothing wraps before the division and nothing is undefined (the sanitizer is the judge)"""
    for bits, p, s in ((64, 18, 4), (64, 18, 18), (128, 38, 10), (128, 38, 38)):
        top = 1 << (bits - 1)
        values = [-top, -top + 1, top - 1, top - 2, -(top // 2), top // 2]
        f = host.put(("ends", bits), ints_to_raw(values, bits))
        for fn, digits in K.decimal_calls(p, s):
            exp = R.decimal(fn, values, p, s, digits, bits)
            got = raw_to_ints(host.run("dec", fn, bits, p, s, digits, f), 8 if fn == R.SIGN else bits)
            assert got == exp, (R.NAMES[fn], bits, p, s, digits, got, exp)


def test_the_128_by_64_division(host):
    rng = np.random.default_rng(2630)
    trip = []
    for k in range(1, 20):                                   # the divisors the kernels use, at the ends of the dividend
        for u in (0, 1, 10**k - 1, 10**k, 10**k + 1, 2**64 - 1, 2**64, 2**127, 2**128 - 1, 15 * 10**37):
            trip.append((u, 10**k))
    for _ in range(20000):                                   # and arbitrary ones: every normalisation shift, corrected digits
        v = int(rng.integers(1, 2**63)) >> int(rng.integers(0, 63)) or 1
        u = (int(rng.integers(0, 2**63)) << 65 | int(rng.integers(0, 2**63)) << 2 | int(rng.integers(0, 4))) >> int(rng.integers(0, 128))
        trip.append((u, v))
    trip += [(2**128 - 1, 2**64 - 1), (2**128 - 1, 1), (2**128 - 1, 2**63), (2**128 - 1, 2**32 + 1), ((2**64 - 1) << 64, 2**64 - 1)]
    raw = b"".join((u >> 64).to_bytes(8, "little") + (u & (2**64 - 1)).to_bytes(8, "little") + v.to_bytes(8, "little") for u, v in trip)
    out = host.run("div", host.put("div", raw))
    got = [int.from_bytes(out[i:i + 16], "little") for i in range(0, len(out), 16)]
    assert got == [u // v for u, v in trip]
