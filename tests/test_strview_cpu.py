"""CPU: databend_amd/csrc/dev_strview.h — the one definition of the 16-byte String view that every kernel includes — compiled for the
host (tests/strview_host_check.cpp) and held to plain Python bytes: the canonical words of an inline view whatever lies past its length,
where a value's bytes are, the checked form of that, building a view and reading it back, and rebasing."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INLINE_MAX = 12


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("strview") / "strview_host_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "strview_host_check.cpp")])

    def run(commands):
        """commands: lists of words -> one output line (split) per command"""
        text = "".join(" ".join(str(w) for w in c) + "\n" for c in commands)
        out = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr[-400:])
        rows = [line.split() for line in out.stdout.splitlines()]
        assert len(rows) == len(commands)
        return rows
    return run


def hx(b):
    return bytes(b).hex() if len(b) else "-"


def inline_view(value, pad):
    """{len, the value's bytes, `pad` in the payload bytes past them}"""
    assert len(value) <= INLINE_MAX and len(pad) == INLINE_MAX
    return struct.pack("<I", len(value)) + value + pad[len(value):]


def long_view(value, index, offset):
    assert len(value) > INLINE_MAX
    return struct.pack("<I", len(value)) + value[:4] + struct.pack("<II", index, offset)


def py_view(value, index, offset):
    return inline_view(value, bytes(12)) if len(value) <= INLINE_MAX else long_view(value, index, offset)


def test_canonical_words_ignore_what_lies_past_the_length(host):
    rng = np.random.default_rng(12)
    values, commands = [], []
    for ln in range(INLINE_MAX + 1):
        for v in (bytes(rng.integers(1, 256, ln, dtype=np.uint8)), b"\xff" * ln, b"\x00" * ln, b"abcdefghijkl"[:ln]):
            for pad in (bytes(12), b"\xff" * 12, bytes(rng.integers(0, 256, 12, dtype=np.uint8))):
                values.append(v)
                commands.append(("canon", hx(inline_view(v, pad))))
    got = host(commands)
    keys = host([("keys", c[1]) for c in commands])
    for v, g, k in zip(values, got, keys):
        exp = struct.unpack("<III", v + bytes(12 - len(v)))           # the zero-padded view's words
        assert g[0] == "1" and tuple(int(x) for x in g[1:]) == exp, (v, g)
        # the two key words: the zero-padded view's 16 bytes as two little-endian u64
        assert k[0] == "1" and tuple(int(x) for x in k[1:]) == struct.unpack("<QQ", inline_view(v, bytes(12))), (v, k)
    # equal words exactly when length and bytes are equal (a trailing NUL is a byte of the value, told apart by the length word)
    words = {}
    for v, g in zip(values, got):
        words.setdefault((len(v),) + tuple(g[1:]), set()).add(v)
    assert all(len(s) == 1 for s in words.values())
    assert len(words) == len(set(values))


def test_thirteen_bytes_are_not_inline(host):
    v = b"0123456789abc"
    got = host([("canon", hx(long_view(v, 1, 77))), ("canon", hx(inline_view(v[:12], b"\xff" * 12)))])
    assert got[0] == ["0", str(struct.unpack("<I", b"0123")[0]), "1", "77"]     # a long view's words are left alone
    assert got[1][0] == "1"
    assert host([("keys", hx(long_view(v, 1, 77)))])[0][0] == "0"


def test_byte_pointer(host):
    buf0, buf1 = bytes(range(40, 80)), bytes(range(100, 180))
    cases = [(inline_view(b"", b"\xff" * 12), -1, 4, b""), (inline_view(b"abc", b"\xff" * 12), -1, 4, b"abc"),
             (inline_view(b"abcdefghijkl", bytes(12)), -1, 4, b"abcdefghijkl"),
             (long_view(buf1[7:7 + 13], 1, 7), 1, 7, buf1[7:20]), (long_view(buf0[3:3 + 30], 0, 3), 0, 3, buf0[3:33]),
             (long_view(buf1[50:80], 1, 50), 1, 50, buf1[50:80])]
    for cmd in ("bytes", "bytesw"):                 # from the view's address, and from its words
        got = host([(cmd, hx(v), hx(buf0), hx(buf1)) for v, _, _, _ in cases])
        for (v, where, off, value), g in zip(cases, got):
            assert g == [str(where), str(off), hx(value)], (cmd, v, g)


def test_checked_byte_pointer(host):
    buf0, buf1 = bytes(range(40, 80)), bytes(range(100, 180))
    good = long_view(buf1[7:20], 1, 7)
    cases = [
        (good, buf0, buf1, 2, ["1", "7", hx(buf1[7:20])]),
        (long_view(buf0[3:33], 0, 3), buf0, buf1, 1, ["0", "3", hx(buf0[3:33])]),
        (inline_view(b"abc", b"\xff" * 12), b"", b"", 0, ["-1", "4", hx(b"abc")]),       # an inline view needs no table
        (good, buf0, buf1, 1, ["null"]),                                                   # index == n_buffers
        (long_view(buf0[3:33], 0, 3), buf0, buf1, 0, ["null"]),                            # no table at all
        (long_view(buf1[7:20], 0xFFFFFFFF, 7), buf0, buf1, 2, ["null"]),
        (long_view(buf1[7:20], 2, 7), buf0, buf1, 2, ["null"]),
        (good, buf0, b"", 2, ["null"]),                                                    # a null entry
        (long_view(buf0[3:33], 0, 3), b"", buf1, 2, ["null"]),
    ]
    got = host([("checked", hx(v), hx(b0), hx(b1), n) for v, b0, b1, n, _ in cases])
    for c, g in zip(cases, got):
        assert g == c[4], (c, g)


def test_build_then_read_and_rebase(host):
    rng = np.random.default_rng(13)
    values = [bytes(rng.integers(0, 256, ln, dtype=np.uint8)) for ln in list(range(14)) + [300]]
    buf0 = bytes(rng.integers(0, 256, 64, dtype=np.uint8))
    buf1 = bytes(rng.integers(0, 256, 17, dtype=np.uint8)) + values[-1] + values[13]
    place = {300: (1, 17), 13: (1, 317)}
    made = host([("make", hx(v)) + place.get(len(v), (1, 5)) for v in values])
    views = [bytes.fromhex(g[0]) for g in made]
    for v, view in zip(values, views):
        assert view == py_view(v, *place.get(len(v), (1, 5))), v
    back = host([("bytes", view.hex(), hx(buf0), hx(buf1)) for view in views])
    for v, g in zip(values, back):
        where, off = (-1, 4) if len(v) <= INLINE_MAX else place[len(v)]
        assert g == [str(where), str(off), hx(v)], (v, g)
    # rebase: long views move, inline views stay bit-identical whatever their padding holds
    dirty = [inline_view(v, b"\xff" * 12) for v in values if len(v) <= INLINE_MAX]
    moved = host([("rebase", view.hex(), 3, 0) for view in views + dirty] + [("rebase", view.hex(), 0, 1000) for view in views + dirty])
    n = len(views) + len(dirty)
    for k, view in enumerate(views + dirty):
        ln, w1, idx, off = struct.unpack("<IIII", view)
        by_index, by_offset = bytes.fromhex(moved[k][0]), bytes.fromhex(moved[n + k][0])
        if ln <= INLINE_MAX:
            assert by_index == view and by_offset == view
        else:
            assert by_index == struct.pack("<IIII", ln, w1, idx + 3, off) and by_offset == struct.pack("<IIII", ln, w1, idx, off + 1000)
