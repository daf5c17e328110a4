"""GPU: the long-row list (databend_amd/csrc/dev_longrows.h) past one wave's worth of the wave-per-row grid. Pass 2 of every two-tier
kernel runs on a fixed grid of 512 blocks x 4 waves = 2,048 waves that stride over the list; the other tests list a handful of rows per
call, so no wave of theirs takes a second row and no list index lies above 2,047. Here n = 4,225 rows (66 waves and one lane) and every
row at an even index is long: 2,113 rows are listed, 65 more than the grid has waves, and the last one sits alone in a ragged wave.

What "long" means is the kernels' own listing condition, read from their code:
  like          like_match.h like_lane_decide: len > DBHIP_LIKE_LONG_BYTES and the pattern's kind is CONTAINS (or SEGMENTS)
  str_length    k_strfn.hip strfn_rows_kernel: len > SF_LONG_BYTES in character mode (byte mode lists nothing)
  substr        the same kernel: len > SF_LONG_BYTES, character mode and sf_plan_walks (a start counted from the end, a start behind
                the first character, or a length)
  trim          the same kernel: len > SF_LONG_BYTES and a pad of at least one byte
  position      k_strsearch.hip ss_position_kernel: len > SF_LONG_BYTES and ss_position_walks (a needle no longer than the value)
  split_part    ss_split_kernel: len > SF_LONG_BYTES and ss_split_walks (a delimiter of 1 .. len bytes)
  replace       ss_count_kernel (the first list): len > SF_LONG_BYTES and ss_len_walks (a needle of 1 .. len bytes); ss_fill_kernel
                (the second list, in the same scratch block): the same rows, and every result of more than SF_LONG_BYTES
  lpad          ss_count_kernel: len > SF_LONG_BYTES, character mode and a length > 0; ss_fill_kernel: results > SF_LONG_BYTES
  concat, upper k_strfn.hip strfn_fill_kernel: a result of more than SF_LONG_BYTES (strfn_copy_kernel walks the list)
  array_*       k_array.hip lane_row: a row of more than DBHIP_ARRAY_LONG_LEN elements (for find, with a needle that is not NULL)
SF_LONG_BYTES is DBHIP_LIKE_LONG_BYTES (256), DBHIP_ARRAY_LONG_LEN is 32.

Every long value carries its own row index (a run of 1 + i mod 61 two-byte characters in front, the decimal index behind byte 256; an
array's elements are derived from the row index), so an answer taken from the wrong list slot, or a listed row that no wave takes, is a
wrong answer. Every row of every call is asserted against the project's references."""
import numpy as np
import pytest

from databend_amd import _lib as T
from tests import array_ref as AR
from tests import str_ref as S
from tests import strsearch_ref as R
from tests import test_gpu_array as GA
from tests import test_gpu_like as GL
from tests import test_gpu_strfn as GF
from tests import test_gpu_strsearch as GS

pytestmark = pytest.mark.gpu

N = 4225                                    # 66 waves and one lane
GRID_WAVES = 512 * 4                        # LONGROWS_PASS2_BLOCKS x the waves of a 256-thread block
LONG = T.LIKE_LONG_BYTES
N_LONG = (N + 1) // 2
assert N_LONG == 2113 == GRID_WAVES + 65 and (N - 1) % 64 == 0 and (N - 1) % 2 == 0 and (LONG, T.ARRAY_LONG_LEN) == (256, 32)


# ---- the String column ------------------------------------------------------------------------------------------------------------------
def long_value(i):
    """more than 256 bytes: 1 + i mod 61 two-byte characters, ASCII up to byte 260, then |<i>| and a part that two rows in three have"""
    head = S.E2 * (1 + i % 61)
    v = head + b"x" * (260 - len(head)) + b"|%d|" % i + (b"ab|" if i % 3 else b"cd|") + b"tail"
    assert len(v) > LONG
    return v


def short_value(i):
    """the odd rows: inline, NULL (None), empty, 13 .. 30 bytes"""
    return [b"s|%d" % i, None, b"", b"medium|%d|" % i + b"y" * (i % 13)][(i // 2) % 4]


_case = {}


def string_case():
    """(values with b"" under a NULL row, valid): computed once, never changed"""
    if not _case:
        raw = [long_value(i) if i % 2 == 0 else short_value(i) for i in range(N)]
        _case["values"] = [b"" if v is None else v for v in raw]
        _case["valid"] = np.array([v is not None for v in raw])
        assert sum(len(v) > LONG for v in _case["values"]) == N_LONG and len(_case["values"][N - 1]) > LONG
    return _case["values"], _case["valid"]


@pytest.fixture(scope="module")
def col(gpu):
    values, valid = string_case()
    return GF.pack(gpu, values, valid=valid, lead=b"\x80", n_buffers=2)


def test_like_contains(gpu, col):
    values, valid = string_case()
    exp = GL.expect(values, valid, b"%|ab|%")
    assert sum(exp) == sum(1 for i in range(0, N, 2) if i % 3) and not all(exp[::2])
    GL.assert_rows(GL.run_like(gpu, col, b"%|ab|%"), exp, values, "like CONTAINS")
    GL.assert_rows(GL.run_like(gpu, col, b"%|ab|%", negate=True), GL.expect(values, valid, b"%|ab|%", negate=True), values, "like CONTAINS negated")


def test_str_length_in_characters(gpu, col):
    values, valid = string_case()
    exp = [S.length(v) if ok else 0 for v, ok in zip(values, valid)]
    assert len(set(exp[::2])) > 61
    assert GF.run_length(gpu, col) == exp


def test_substr_in_characters(gpu, col):
    """a start counted from the end (the |<i>|..|tail behind byte 256) and a start behind the first character, in turn"""
    values, valid = string_case()
    a = [-(9 + len(b"%d" % i)) if i % 4 == 0 else 120 + i % 50 for i in range(N)]
    exp = GF.check_slice(gpu, col, values, valid, S.SUBSTR, a, 30, what="long rows")
    assert all(e[0] == 9 + len(b"%d" % (4 * q)) for q, e in enumerate(exp[::4])) and all(e[0] == 30 for e in exp[2::4])


def test_trim_with_a_pad(gpu, col):
    values, valid = string_case()
    exp = GF.check_slice(gpu, col, values, valid, S.TRIM_BOTH, pad=S.E2, what="long rows")
    assert {len(v) - int.from_bytes(e[:4], "little") for v, e in zip(values[::2], exp[::2])} == set(range(2, 124, 2))
    GF.check_slice(gpu, col, values, valid, S.TRIM_LEADING, pad=S.E2, what="long rows")


def test_position(gpu, col):
    values, valid = string_case()
    exp = GS.check_position(gpu, col, values, valid, b"|ab|", what="long rows")
    assert len(set(exp[::2])) > 50 and 0 in exp[::2]
    GS.check_position(gpu, col, values, valid, b"|", [1 + i % 5 for i in range(N)], what="long rows")


def test_split_part(gpu, col):
    values, valid = string_case()
    exp = GS.check_split(gpu, col, values, valid, b"|", [2 if i % 4 else -3 for i in range(N)], what="long rows")
    assert all(e[4:4 + e[0]] == b"%d" % i for i, e in list(enumerate(exp))[::2])


def test_replace(gpu, col):
    """the count's list and the fill's list in one scratch block"""
    values, valid = string_case()
    res = GS.check_rewrite(gpu, R.REPLACE, col, values, valid, None, b"|", b"<->", what="long rows")
    assert all(b"<->%d<->" % i in res[i] for i in range(0, N, 2))
    GS.check_rewrite(gpu, R.REPLACE, col, values, valid, None, b"|ab", b"", what="long rows")


def test_lpad_to_long_results(gpu, col):
    """long sources through the count's list (character mode), every result through the fill's"""
    values, valid = string_case()
    k = [270 + i % 50 for i in range(N)]
    res = GS.check_rewrite(gpu, R.LPAD, col, values, valid, k, S.E3 + b"p", what="long rows")
    assert all(len(r) > LONG for r, ok in zip(res, valid) if ok)


def build_rows(values, valid, shape):
    return [[(v if ok else None) if a is None else a for a in shape] for v, ok in zip(values, valid)]


def test_concat_and_upper_to_long_results(gpu, col):
    values, valid = string_case()
    dash = GF.pack(gpu, [b"-"])
    dash.is_scalar = True
    GF.check_build(gpu, S.CONCAT, [col, dash, col], build_rows(values, valid, [None, b"-", None]), "concat long rows")
    GF.check_build(gpu, S.UPPER, [col], build_rows(values, valid, [None]), "upper long rows")


# ---- the Array columns ------------------------------------------------------------------------------------------------------------------
def array_rows(elem, n_short):
    """even rows: 33 .. 35 elements derived from the row index; odd rows: empty, or up to n_short elements, a NULL among them"""
    rows = []
    for i in range(N):
        if i % 2 == 0:
            rows.append([elem(i, k) for k in range(33 + i % 3)])
        else:
            row = [elem(i, k) for k in range((i // 2) % (n_short + 1))]
            if len(row) > 1:
                row[1] = None
            rows.append(row)
    assert sum(len(r) > T.ARRAY_LONG_LEN for r in rows) == N_LONG and len(rows[-1]) > T.ARRAY_LONG_LEN
    return rows


@pytest.fixture(scope="module")
def numbers(gpu):
    rows = array_rows(lambda i, k: i * 64 + k, 4)
    return rows, GA.Arr(gpu, "i64", rows, first=3, voff=5, tail=2)


def test_array_sum(gpu, numbers):
    rows, a = numbers
    GA.check_reduce("i64", AR.SUM, rows, GA.run_reduce(gpu, AR.SUM, a))
    GA.check_reduce("i64", AR.MAX, rows, GA.run_reduce(gpu, AR.MAX, a))


def test_array_contains_numbers(gpu, numbers):
    """a needle column: row i's needle is its own element (i / 2) mod 40, which rows of fewer elements do not have"""
    rows, a = numbers
    needle = [i * 64 + (i // 2) % 40 for i in range(N)]
    exp = [AR.indexof(row, needle[r], False) for r, row in enumerate(rows)]
    assert len(set(exp[::2])) >= 34 and 0 in exp[::2]
    assert GA.run_find(gpu, AR.INDEXOF, a, needle) == exp
    assert GA.run_find(gpu, AR.CONTAINS, a, needle) == [e != 0 for e in exp]


def test_array_contains_strings(gpu):
    """the constant needle at element i mod 37 of row i, in the rows that have one"""
    nd = b"needle-of-13b"
    rows = array_rows(lambda i, k: nd if k == i % 37 else (b"row-%d-element-%d" % (i, k) if k % 5 == 4 else b"r%d.%d" % (i, k)), 3)
    a = GA.Arr(gpu, "string", rows, first=2, voff=3)
    exp = [AR.indexof(row, nd) for row in rows]
    assert len(set(exp[::2])) >= 34 and 0 in exp[::2]
    assert GA.run_find_str(gpu, AR.INDEXOF, a, nd) == exp
    assert GA.run_find_str(gpu, AR.CONTAINS, a, nd) == [e != 0 for e in exp]


def test_unnest(gpu, numbers):
    rows, a = numbers
    exp = [r for r, row in enumerate(rows) for _ in row]
    assert GA.run_unnest(gpu, a.offsets, a.n, a.n_elems, len(exp)) == exp
