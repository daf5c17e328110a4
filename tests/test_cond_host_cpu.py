"""CPU: databend_amd/csrc/dev_cond.h — the one implementation of the conditionals (include/dbhip.h a27), which the kernels of
k_cond.hip inline — compiled for the host in a stand-alone program (tests/cond_host_check.cpp) and held to tests/cond_ref.py bit for bit
on the shared case list (tests/cond_cases.py): the chooser for 1, 2, 3 and 16 conditions, every element size, coalesce, the bit fetch at
offsets 0, 1, 63, 64 and 69, the rebased views, and all 9 x 9 Kleene operand pairs per operator. Where the compiler links it the
program is built with -fsanitize=address,undefined -fno-sanitize-recover=all. Nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import cond_cases as K
from tests import cond_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Host:
    def __init__(self, exe, tmp):
        self.exe, self.tmp, self.count = exe, tmp, 0

    def put(self, raw):
        """file of raw bytes"""
        self.count += 1
        path = os.path.join(self.tmp, "in%d.bin" % self.count)
        with open(path, "wb") as f:
            f.write(bytes(raw))
        return path

    def run(self, *words):
        out = os.path.join(self.tmp, "out.bin")
        words = [str(w) for w in words]
        words.insert(self.out_at(words[0]), out)
        p = subprocess.run([self.exe] + words, capture_output=True, text=True)
        assert p.returncode == 0, (words[:9], p.returncode, p.stderr[-800:])
        with open(out, "rb") as f:
            return f.read()

    @staticmethod
    def out_at(mode):
        return {"fetch": 5, "select": 7, "logic": 4, "check": 4}[mode]

    def bitmap(self, bits, off):
        """an unpacked column behind `off` junk bits, as a Bitmap file of exactly the bytes it needs"""
        rng = np.random.default_rng(off + len(bits))
        whole = np.concatenate([rng.integers(0, 2, off).astype(bool), np.asarray(bits, dtype=bool), rng.integers(0, 2, 7).astype(bool)])
        return self.put(np.packbits(whole[:off + len(bits)], bitorder="little"))

    def column(self, col, voff=0, data=None, n_buffers=0):
        """the five words of a column: a Boolean Col's bits (or `data`, raw element bytes) and its validity at bit offset voff"""
        if data is None:
            data = np.packbits(np.asarray(col.values, dtype=bool), bitorder="little")
        valid = "-" if col.valid is None else self.bitmap(col.valid, voff)
        return [self.put(data), valid, voff if col.valid is not None else 0, int(col.scalar), n_buffers]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("cond"))
    exe = os.path.join(tmp, "cond_host_check")
    src = os.path.join(ROOT, "tests", "cond_host_check.cpp")
    base = ["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, src]
    if subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True).returncode != 0:
        subprocess.check_call(base)
    return Host(exe, tmp)


def split(raw, n, size):
    words = (n + 63) // 64
    nd = n * size if size else words * 8
    assert len(raw) == nd + words * 8 + n
    valid = np.unpackbits(np.frombuffer(raw[nd:nd + words * 8], np.uint8), bitorder="little")
    assert not valid[n:].any(), "validity bits past n"
    return raw[:nd], valid[:n].astype(bool), np.frombuffer(raw[nd + words * 8:], np.uint8)


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("off", K.FETCH_OFFSETS)
def test_bit_fetch(host, off, misalign):
    for nbits in (off + 1, off + 63, off + 64, off + 65, off + 130, off + 1000):
        bits = np.random.default_rng(nbits).integers(0, 2, nbits).astype(bool)
        raw = np.packbits(bits, bitorder="little")
        got = np.frombuffer(host.run("fetch", host.put(raw), misalign, nbits, off), np.uint64)
        rows = bits[off:]
        exp = [sum(int(b) << i for i, b in enumerate(rows[r:r + 64])) for r in range(0, len(rows), 64)]
        assert [int(x) for x in got] == exp, (off, nbits, misalign)


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("size", (1, 2, 4, 8, 16, 32))
@pytest.mark.parametrize("k", K.COND_COUNTS)
def test_case(host, k, size, misalign):
    n = K.N if k < 16 else 6000
    conds, vals = K.conditions(n, k), K.values(size, n, k + 1, last_valid=k != 2)
    if k == 3:                                                    # CASE without ELSE: a NULL scalar, never dereferenced
        vals[-1] = R.Col(np.zeros((1, size), np.uint8), np.array([False]), True)
    args = []
    for j, c in enumerate(conds):
        args += host.column(c, K.FETCH_OFFSETS[j % 5])
    for j, v in enumerate(vals):
        args += host.column(v, K.FETCH_OFFSETS[(j + 2) % 5], data=b"" if v.scalar else v.values.tobytes())
    data, valid, branch = split(host.run("select", size, n, k, k + 1, 0, misalign, *args), n, size)
    exp, exp_valid, exp_branch = R.case_when(conds, vals, n, 0)
    assert (branch == exp_branch).all()
    assert set(exp_branch) == set(range(k + 1)), "the list must reach every branch"
    assert (valid == exp_valid).all()
    assert data == exp.tobytes()
    first_true = np.array(R.choose_case_rows(conds, n))
    assert (first_true == exp_branch).all()
    several = sum(1 for i in range(n) if sum(c.is_valid(i) and c.values[i] for c in conds) > 1)
    null_set = sum(1 for c in conds if c.valid is not None for i in range(n) if not c.valid[i] and c.values[i])
    assert (k == 1 or several > 0) and (k == 1 or null_set > 0) and (exp_branch == k).any()


@pytest.mark.parametrize("size", (1, 2, 4, 8, 16, 32))
@pytest.mark.parametrize("k", (1, 2, 3, 17))
def test_coalesce(host, k, size):
    n = K.N
    vals = K.arguments(size, n, k)
    args = []
    for j, v in enumerate(vals):
        args += host.column(v, K.FETCH_OFFSETS[j % 5], data=v.values.tobytes())
    data, valid, branch = split(host.run("select", size, n, 0, k, 0, 0, *args), n, size)
    exp, exp_valid, exp_branch = R.coalesce(vals, n, 0)
    assert (branch == exp_branch).all() and (valid == exp_valid).all() and data == exp.tobytes()
    assert (np.array(R.choose_coalesce_rows(vals, n)) == exp_branch).all()
    assert set(exp_branch) == set(range(k + 1)) or k == 17 and set(exp_branch) >= {0, 1, 2, 16, 17}, "every argument and the NULL branch"


def test_bool_values(host):
    n = K.N
    conds, vals = K.conditions(n, 2), K.bool_values(n, 3)
    args = []
    for j, c in enumerate(conds + vals):
        args += host.column(c, K.FETCH_OFFSETS[j % 5])
    data, valid, branch = split(host.run("select", 0, n, 2, 3, 0, 1, *args), n, 0)
    exp, exp_valid, exp_branch = R.case_when(conds, vals, n, False)
    got = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")
    assert not got[n:].any() and (got[:n].astype(bool) == exp).all() and (valid == exp_valid).all() and (branch == exp_branch).all()


def test_string_views_are_rebased(host):
    n = K.N
    rng = np.random.default_rng(27)
    n_buffers = [1, 2, 0]
    views = []
    for j, nb in enumerate(n_buffers):
        v = np.zeros((n, 4), np.uint32)
        lens = rng.choice([0, 3, 12, 13, 40], n) if nb else rng.choice([0, 3, 12], n)
        v[:, 0] = lens
        v[:, 1] = rng.integers(1, 2**32, n)
        v[:, 2] = np.where(lens > 12, rng.integers(0, max(nb, 1), n), rng.integers(1, 2**32, n))
        v[:, 3] = rng.integers(1, 2**32, n)
        views.append(v.view(np.uint8).reshape(n, 16))
    conds = K.conditions(n, 2)
    vals = [R.Col(views[j], K.validity(n, j)) for j in range(3)]
    args = []
    for c in conds:
        args += host.column(c, 5)
    for j, v in enumerate(vals):
        args += host.column(v, 69, data=v.values.tobytes(), n_buffers=n_buffers[j])
    data, valid, branch = split(host.run("select", 16, n, 2, 3, 1, 0, *args), n, 16)
    exp_branch = R.choose_case(conds, n)
    exp = R.select_views(views, [v.valid for v in vals], [False] * 3, n_buffers, exp_branch)
    assert data == exp and (branch == exp_branch).all()
    moved = sum(1 for i in range(n) if exp[16 * i:16 * i + 16] not in (bytes(16), views[exp_branch[i]][i].tobytes()))
    assert moved > 20, "long views of the second argument must have moved by one entry"


@pytest.mark.parametrize("op", (R.AND, R.OR, R.NOT, R.XOR))
def test_kleene(host, op):
    n = 333
    forms = K.kleene_operands(n)
    assert len(forms) == 9
    for i, (na, a) in enumerate(forms.items()):
        for j, (nb, b) in enumerate(forms.items()):
            if op == R.NOT and j:
                continue
            args = host.column(a, K.FETCH_OFFSETS[i % 5]) + (host.column(b, K.FETCH_OFFSETS[j % 5]) if op != R.NOT else [])
            raw = host.run("logic", op, n, (i + j) & 1, *args)
            bits = np.unpackbits(np.frombuffer(raw, np.uint8), bitorder="little").astype(bool)
            words = (n + 63) // 64
            t, v = R.bool_logic(op, a, b, n)
            assert (bits[:n] == t).all() and (bits[64 * words:64 * words + n] == v).all(), (R.NAMES[op], na, nb)
            assert not bits[n:64 * words].any() and not bits[64 * words + n:].any()


def test_check(host):
    def ask(coalesce, n_conds, n_vals, descs):
        words = [w for d in descs for w in d]
        return int(host.run("check", int(coalesce), n_conds, n_vals, *words).split()[0])

    b, i4 = (R.T_BOOL, 0, 0, 0, 0), (R.T_I32, 0, 0, 0, 0)
    assert ask(False, 1, 2, [b, i4, i4]) == R.OK
    assert ask(False, 16, 17, [b] * 16 + [i4] * 17) == R.OK
    assert ask(False, 17, 18, [b] * 17 + [i4] * 18) == R.UNSUPPORTED
    assert ask(False, 1, 3, [b, i4, i4, i4]) == R.INVALID
    assert ask(False, 1, 2, [i4, i4, i4]) == R.INVALID
    assert ask(False, 1, 2, [b, i4, (R.T_I64, 0, 0, 0, 0)]) == R.INVALID
    assert ask(True, 0, 17, [i4] * 17) == R.OK and ask(True, 0, 18, [i4] * 18) == R.UNSUPPORTED and ask(True, 0, 0, []) == R.INVALID
    d = (R.T_DEC128, 0, 0, 30, 4)
    assert ask(True, 0, 2, [d, d]) == R.OK and ask(True, 0, 2, [d, (R.T_DEC128, 0, 0, 30, 5)]) == R.INVALID
    assert ask(True, 0, 1, [(18, 0, 0, 0, 0)]) == R.INVALID and ask(True, 0, 1, [(0, 0, 0, 0, 0)]) == R.INVALID
