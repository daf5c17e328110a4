"""CPU: tests/cond_ref.py, the plain restatement of the conditionals (include/dbhip.h a27), against hand-written truth tables and small
literal examples — so that the yardstick of the host checker's test and of the GPU test is itself pinned down."""
import numpy as np

from tests import cond_cases as K
from tests import cond_ref as R

T, F, N = True, False, None


def col(values, valid=None, scalar=False):
    return R.Col(np.array(values), None if valid is None else np.array(valid, dtype=bool), scalar)


def test_kleene_truth_tables():
    # the classical statements, each spelled out on its own
    for x in (T, F, N):
        assert R.kleene(R.AND, F, x) is F and R.kleene(R.AND, x, F) is F          # FALSE absorbs, NULL or not
        assert R.kleene(R.OR, T, x) is T and R.kleene(R.OR, x, T) is T            # TRUE absorbs
        assert R.kleene(R.XOR, N, x) is N and R.kleene(R.XOR, x, N) is N          # XOR knows nothing about a NULL
        assert R.kleene(R.AND, T, x) is x and R.kleene(R.OR, F, x) is x           # the neutral elements
    assert R.kleene(R.AND, N, N) is N and R.kleene(R.OR, N, N) is N
    assert R.kleene(R.AND, N, T) is N and R.kleene(R.OR, N, F) is N
    assert [R.kleene(R.NOT, x) for x in (T, F, N)] == [F, T, N]
    assert [R.kleene(R.XOR, a, b) for a in (T, F) for b in (T, F)] == [F, T, T, F]
    # De Morgan holds in Kleene logic: a check of the tables against each other
    for a in (T, F, N):
        for b in (T, F, N):
            assert R.kleene(R.NOT, R.kleene(R.AND, a, b)) is R.kleene(R.OR, R.kleene(R.NOT, a), R.kleene(R.NOT, b))


def test_bool_logic_columns():
    a = col([1, 1, 1, 0, 0, 0, 1, 0, 1], [1, 1, 1, 1, 1, 1, 0, 0, 0])            # T T T F F F N N N (NULL payloads 1, 0, 1)
    b = col([1, 0, 1, 1, 0, 0, 1, 0, 0], [1, 1, 0, 1, 1, 0, 1, 1, 0])            # T F N T F N T F N
    t, v = R.bool_logic(R.AND, a, b, 9)
    assert list(t) == [1, 0, 0, 0, 0, 0, 0, 0, 0] and list(v) == [1, 1, 0, 1, 1, 1, 0, 1, 0]
    t, v = R.bool_logic(R.OR, a, b, 9)
    assert list(t) == [1, 1, 1, 1, 0, 0, 1, 0, 0] and list(v) == [1, 1, 1, 1, 1, 0, 1, 0, 0]
    t, v = R.bool_logic(R.XOR, a, b, 9)
    assert list(t) == [0, 1, 0, 1, 0, 0, 0, 0, 0] and list(v) == [1, 1, 0, 1, 1, 0, 0, 0, 0]
    t, v = R.bool_logic(R.NOT, a, None, 9)
    assert list(t) == [0, 0, 0, 1, 1, 1, 0, 0, 0] and list(v) == [1, 1, 1, 1, 1, 1, 0, 0, 0]
    # a scalar operand is its one row, repeated
    t, v = R.bool_logic(R.OR, a, col([1], [0], True), 9)
    assert list(t) == [1, 1, 1, 0, 0, 0, 0, 0, 0] and list(v) == [1, 1, 1, 0, 0, 0, 0, 0, 0]


def test_case_when_literal():
    c0 = col([1, 0, 1, 0, 1, 0], [1, 1, 0, 1, 0, 1])                              # T F N(1) F N(1) F
    c1 = col([1, 1, 1, 0, 0, 0])                                                  # T T T F F F
    v0, v1 = col([10, 11, 12, 13, 14, 15]), col([20, 21, 22, 23, 24, 25], [1, 0, 1, 1, 1, 1])
    v2 = col([30, 31, 32, 33, 34, 35], [1, 1, 1, 0, 1, 1])
    out, valid, branch = R.case_when([c0, c1], [v0, v1, v2], 6, 0)
    assert list(branch) == [0, 1, 1, 2, 2, 2]                                     # first TRUE wins; a NULL condition is not TRUE
    assert list(valid) == [1, 0, 1, 0, 1, 1]
    assert list(out) == [10, 0, 22, 0, 34, 35]                                    # NULL rows hold zero, not the payload
    assert list(R.choose_case_rows([c0, c1], 6)) == [0, 1, 1, 2, 2, 2]
    # CASE without ELSE: the NULL scalar
    out, valid, branch = R.case_when([c1], [v0, col([99], [0], True)], 6, 0)
    assert list(branch) == [0, 0, 0, 1, 1, 1] and list(valid) == [1, 1, 1, 0, 0, 0] and list(out) == [10, 11, 12, 0, 0, 0]
    # constant conditions
    for bit, ok, want in ((1, 1, 0), (0, 1, 1), (1, 0, 1)):
        _, _, branch = R.case_when([col([bit], [ok], True)], [v0, v1], 6, 0)
        assert list(branch) == [want] * 6


def test_coalesce_literal():
    a, b = col([1, 2, 3, 4], [1, 0, 0, 1]), col([5, 6, 7, 8], [1, 1, 0, 0])
    out, valid, branch = R.coalesce([a, b], 4, 0)
    assert list(branch) == [0, 1, 2, 0] and list(valid) == [1, 1, 0, 1] and list(out) == [1, 6, 0, 4]
    out, valid, branch = R.coalesce([a, col([0], None, True)], 4, -1)             # coalesce(x, 0)
    assert list(branch) == [0, 1, 1, 0] and list(valid) == [1, 1, 1, 1] and list(out) == [1, 0, 0, 4]
    # lists of bytes go the row-by-row way and agree
    out, valid = R.select([R.Col([b"a", b"b"], [True, False]), R.Col([b"c", b"d"], None)], [0, 0], b"")
    assert out == [b"a", b""] and list(valid) == [True, False]
    assert R.nullif(col([1, 2, 3, 4], [1, 1, 0, 1]), col([1, 5, 3, 4], [1, 1, 1, 0]), 4) == [False, True, False, True]


def test_views_and_tables():
    assert R.table_bases([1, 2, 0, 3]) == ([0, 1, 3, 3], 6)
    inline = (5).to_bytes(4, "little") + b"hello" + bytes(7)
    long_ = (40).to_bytes(4, "little") + b"abcd" + (1).to_bytes(4, "little") + (100).to_bytes(4, "little")
    assert R.rebased_view(inline, 7) == inline
    assert R.rebased_view(long_, 3) == long_[:8] + (4).to_bytes(4, "little") + long_[12:]
    twelve = (12).to_bytes(4, "little") + b"abcdefghijkl"
    assert R.rebased_view(twelve, 9) == twelve                                    # 12 bytes are still inline
    views = [[inline, long_], [long_, long_]]
    got = R.select_views(views, [None, [True, False]], [False, False], [2, 2], [1, 1])
    assert got == R.rebased_view(long_, 2) + bytes(16)                            # a NULL row is the all-zero view
    # whole columns of views give what the rows give
    rng = np.random.default_rng(7)
    cols = []
    for k in range(3):
        v = rng.integers(0, 2**32, (200, 4), dtype=np.uint32)
        v[:, 0] %= 25
        cols.append(v.view(np.uint8).reshape(200, 16))
    valids = [rng.random(200) < 0.5, None, np.array([True])]
    branch = rng.integers(0, 4, 200)
    by_rows = R.select_views([[r for r in c] for c in cols], valids, [False, False, True], [2, 0, 5], list(branch))
    assert R.select_views(cols, valids, [False, False, True], [2, 0, 5], branch) == by_rows


def test_check_literal():
    b, i4 = R.T_BOOL, (R.T_I32, 0, 0)
    assert R.check([b], [i4, i4]) == R.OK and R.check(None, [i4]) == R.OK
    assert R.check([], [i4]) == R.INVALID and R.check([b], [i4]) == R.INVALID and R.check([R.T_I8], [i4, i4]) == R.INVALID
    assert R.check([b] * 17, [i4] * 18) == R.UNSUPPORTED and R.check(None, [i4] * 18) == R.UNSUPPORTED
    assert R.check(None, [(R.T_DEC64, 10, 2), (R.T_DEC64, 10, 3)]) == R.INVALID and R.check(None, [(0, 0, 0)]) == R.INVALID


def test_the_case_list_holds_what_it_promises():
    n = K.N
    conds = K.conditions(n, 3)
    assert any(c.valid is not None and (c.values & ~c.valid).any() for c in conds), "NULL conditions with the payload bit set"
    true = [R.valid_rows(c, n) & c.values for c in conds]
    assert (sum(t.astype(int) for t in true) > 1).any() and (sum(t.astype(int) for t in true) == 0).any()
    branch = R.choose_case(conds, n)
    words = branch[:960].reshape(15, 64)
    assert (words == words[:, :1]).all(axis=1).any() and (branch[1:] != branch[:-1]).sum() > n // 8
    for v in K.values(8, n, 3):
        assert (v.values != 0).all()
    assert any(len(s) > 12 for s in K.strings(n, 0)) and any(0 < len(s) <= 12 for s in K.strings(n, 0))
