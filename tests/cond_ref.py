"""A plain restatement of the conditionals (include/dbhip.h a27) for the tests: the chooser over unpacked bits, the result with zeros in
NULL rows, the rebased String views and tables, and Kleene logic from truth tables over {TRUE, FALSE, NULL}. Row by row in Python, and
(for the large cases) the same over whole numpy columns of unpacked bits; tests/test_cond_ref_cpu.py holds the two ways to each other.
No Bitmap word, no bit formula, nothing shared with csrc/dev_cond.h.

A column here is a Col: `values` (a list or array of anything that compares with ==; for a Boolean column Python bools), `valid` (a list
of bools, or None for a column that cannot be NULL) and `scalar` (one value, and one validity bit, for every row)."""
import numpy as np

OK, INVALID, UNSUPPORTED = 0, 1, 7
T_BOOL, T_I8, T_I16, T_I32, T_I64, T_U8, T_U16, T_U32, T_U64, T_F32, T_F64, T_DATE, T_TIMESTAMP, T_DEC64, T_DEC128, T_STRING, T_DEC256 = range(1, 18)
TYPES = tuple(range(1, 18))
SIZE = {T_BOOL: 0, T_I8: 1, T_U8: 1, T_I16: 2, T_U16: 2, T_I32: 4, T_U32: 4, T_F32: 4, T_DATE: 4, T_I64: 8, T_U64: 8, T_F64: 8, T_TIMESTAMP: 8,
        T_DEC64: 8, T_DEC128: 16, T_STRING: 16, T_DEC256: 32}
DECIMALS = (T_DEC64, T_DEC128, T_DEC256)
MAX_CONDS = 16
AND, OR, NOT, XOR = range(4)
NAMES = {AND: "and", OR: "or", NOT: "not", XOR: "xor"}


class Col:
    def __init__(self, values, valid=None, scalar=False):
        self.values, self.valid, self.scalar = values, valid, scalar

    def value(self, i):
        return self.values[0 if self.scalar else i]

    def is_valid(self, i):
        return True if self.valid is None else bool(self.valid[0 if self.scalar else i])


# ---- the chooser ----------------------------------------------------------------------------------------------------------------------
def choose_case_rows(conds, n):
    """branch of every row: the first condition that is TRUE (valid and set), len(conds) when none is. Row by row."""
    out = []
    for i in range(n):
        k = 0
        while k < len(conds) and not (conds[k].is_valid(i) and bool(conds[k].value(i))):
            k += 1
        out.append(k)
    return out


def choose_coalesce_rows(args, n):
    """branch of every row: the first argument that is valid, len(args) when none is. Row by row."""
    out = []
    for i in range(n):
        k = 0
        while k < len(args) and not args[k].is_valid(i):
            k += 1
        out.append(k)
    return out


def _rows(x, scalar, n):
    """one bool per row of unpacked bits (a scalar's one bit repeated)"""
    x = np.asarray(x, dtype=bool)
    return np.repeat(x[:1], n) if scalar else x[:n]


def valid_rows(col, n):
    return np.ones(n, dtype=bool) if col.valid is None else _rows(col.valid, col.scalar, n)


def choose_case(conds, n):
    """the same over whole columns of unpacked bits: later conditions are written first, so the first TRUE one stays"""
    branch = np.full(n, len(conds), dtype=np.int64)
    for k in reversed(range(len(conds))):
        branch[valid_rows(conds[k], n) & _rows(conds[k].values, conds[k].scalar, n)] = k
    return branch


def choose_coalesce(args, n):
    branch = np.full(n, len(args), dtype=np.int64)
    for k in reversed(range(len(args))):
        branch[valid_rows(args[k], n)] = k
    return branch


def select(values, branch, zero):
    """-> (result values, result validity): the chosen branch's value where it is valid, `zero` and NULL elsewhere (a branch index
    of len(values) is the NULL branch of a coalesce). Columns of numpy rows give a numpy result, lists a list."""
    n = len(branch)
    if isinstance(values[0].values, np.ndarray):
        first = values[0].values
        out = np.empty((n,) + first.shape[1:], dtype=first.dtype)
        out[...] = zero
        valid = np.zeros(n, dtype=bool)
        for k, col in enumerate(values):
            rows = (np.asarray(branch) == k) & valid_rows(col, n)
            valid |= rows
            if col.scalar:
                out[rows] = col.values[0]
            else:
                out[rows] = col.values[:n][rows]
        return out, valid
    out, valid = [], []
    for i, k in enumerate(branch):
        ok = k < len(values) and values[k].is_valid(i)
        valid.append(ok)
        out.append(values[k].value(i) if ok else zero)
    return out, np.asarray(valid, dtype=bool)


def case_when(conds, values, n, zero):
    assert len(values) == len(conds) + 1
    branch = choose_case(conds, n)
    out, valid = select(values, branch, zero)
    return out, valid, branch


def coalesce(args, n, zero):
    branch = choose_coalesce(args, n)
    out, valid = select(args, branch, zero)
    return out, valid, branch


# ---- Strings: views and tables --------------------------------------------------------------------------------------------------------
def table_bases(n_buffers):
    """where each argument's buffer table starts in the result's table"""
    bases, at = [], 0
    for k in n_buffers:
        bases.append(at)
        at += k
    return bases, at


def rebased_view(view, base):
    """a 16-byte view (sequence of 16 byte values) taken from an argument whose table starts at `base`: the buffer index of a long view
    (more than 12 bytes) moves by it, an inline view stays as it is"""
    raw = bytes(bytearray(int(x) for x in view))
    length = int.from_bytes(raw[0:4], "little")
    if length <= 12:
        return raw
    index = int.from_bytes(raw[8:12], "little")
    return raw[0:8] + ((index + base) % 2**32).to_bytes(4, "little") + raw[12:16]


def select_views(views, valids, scalars, n_buffers, branch):
    """views[k]: argument k's (rows, 16) view bytes -> the result's n views as one bytes object: the chosen view rebased, sixteen zero
    bytes for a NULL row"""
    bases, _ = table_bases(n_buffers)
    if isinstance(views[0], np.ndarray):                     # whole columns at once; the row-by-row way below says the same
        n = len(branch)
        out = np.zeros((n, 4), dtype=np.uint32)
        for k, v in enumerate(views):
            rows = np.asarray(branch) == k
            if valids[k] is not None:
                rows = rows & _rows(valids[k], scalars[k], n)
            words = np.ascontiguousarray(v).view(np.uint32).reshape(-1, 4)
            words = np.repeat(words[:1], n, axis=0) if scalars[k] else words[:n]
            words = words[rows].copy()
            words[:, 2] = np.where(words[:, 0] > 12, words[:, 2] + np.uint32(bases[k]), words[:, 2])
            out[rows] = words
        return out.tobytes()
    out = []
    for i, k in enumerate(branch):
        if k >= len(views):
            out.append(bytes(16))
            continue
        j = 0 if scalars[k] else i
        ok = valids[k] is None or bool(valids[k][j])
        out.append(rebased_view(views[k][j], bases[k]) if ok else bytes(16))
    return b"".join(out)


# ---- Kleene logic ---------------------------------------------------------------------------------------------------------------------
# None is NULL. Written out, not computed.
T, F, N = True, False, None
TABLE = {
    AND: {(T, T): T, (T, F): F, (T, N): N, (F, T): F, (F, F): F, (F, N): F, (N, T): N, (N, F): F, (N, N): N},
    OR:  {(T, T): T, (T, F): T, (T, N): T, (F, T): T, (F, F): F, (F, N): N, (N, T): T, (N, F): N, (N, N): N},
    XOR: {(T, T): F, (T, F): T, (T, N): N, (F, T): T, (F, F): F, (F, N): N, (N, T): N, (N, F): N, (N, N): N},
}
NOT_TABLE = {T: F, F: T, N: N}


def kleene(op, a, b=None):
    return NOT_TABLE[a] if op == NOT else TABLE[op][(a, b)]


def bool_logic(op, a, b, n):
    """-> (true rows, valid rows) as lists of bools: the two Bitmaps of dbhip_bool_logic"""
    three_values = (T, F, N)

    def codes(col):   # 0 TRUE, 1 FALSE, 2 NULL per row
        return np.where(valid_rows(col, n), np.where(_rows(col.values, col.scalar, n), 0, 1), 2)

    # the truth table looked up per row: result[code of a][code of b]
    table = [[kleene(op, x, y if op != NOT else None) for y in three_values] for x in three_values]
    ca = codes(a)
    cb = codes(b) if op != NOT else np.zeros(n, dtype=np.int64)
    t = np.array([[r is True for r in row] for row in table], dtype=bool)[ca, cb]
    v = np.array([[r is not None for r in row] for row in table], dtype=bool)[ca, cb]
    return t, v


def nullif(a, b, n):
    """-> validity of nullif(a, b): a's, cleared where both are valid and equal (the payload is a's, unchanged)"""
    return [a.is_valid(i) and not (b.is_valid(i) and a.value(i) == b.value(i)) for i in range(n)]


# ---- dbhip_case_check -----------------------------------------------------------------------------------------------------------------
def check(conds, values):
    """conds: list of type codes or None (a coalesce); values: list of (type, precision, scale) -> status"""
    if values is None:
        return INVALID
    if conds is None:
        if len(values) < 1:
            return INVALID
        if len(values) > MAX_CONDS + 1:
            return UNSUPPORTED
    else:
        if len(conds) < 1 or len(values) != len(conds) + 1:
            return INVALID
        if len(conds) > MAX_CONDS:
            return UNSUPPORTED
        if any(t != T_BOOL for t in conds):
            return INVALID
    t0 = values[0][0]
    if t0 not in SIZE:
        return INVALID
    for t, p, s in values:
        if t != t0 or (t0 in DECIMALS and (p, s) != tuple(values[0][1:])):
            return INVALID
    return OK


def pack(bools):
    """bools -> LSB-first Bitmap bytes in whole 64-bit words"""
    by = np.packbits(np.asarray(bools, dtype=bool), bitorder="little")
    return np.concatenate([by, np.zeros((-len(by)) % 8 if len(by) else 8, np.uint8)])
