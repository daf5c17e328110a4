"""The cases of the fused expression interpreter's tests (tests/test_expr_ref_cpu.py, tests/test_gpu_expr.py): sizes, value pools and a
seeded generator of well-typed register programs that stay inside every documented limit of dbhip_expr_eval — at most 24 instructions
after LOAD elimination (a decimal constant the host converts counts as one), 16 registers, 8 inputs, 2 Decimal128 inputs, 6 decimal
nodes, no OR / value-feeding AND over nullable operands unless wrapped in IS_TRUE, no raising IF branch, no nullable IF condition, and
at most 20 of the 24 LDS slots live (so that two-slot values that fragment the file still fit).

Every seed belongs to a steering class that names the kernel instantiation it is meant for: the input-count bound (2 / 4 / 8), whether
every input is a plain 8-byte non-scalar column, whether at most 8 slots are live (4 rows per lane) or at least 9 (2 rows per lane),
and the programs with a rounding decimal multiply / divide. census() counts what the committed seed list covers; the CPU test asserts
it, so the GPU test cannot quietly cover less than it says."""
import collections

import numpy as np

from databend_amd import _lib as T
from tests import datetime_ref as DR
from tests import expr_ref as R
from tests import float_ref as FR

SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1025, 4099)   # wave chunk: 128 / 256 rows, workgroup: 512 / 1024
MAX_INS, MAX_REGS, MAX_INPUTS, MAX_WIDE_INPUTS, MAX_DEC, MAX_LIVE = 24, 16, 8, 2, 6, 20
ALL_TYPES = R.NUMBERS + (T.T_BOOL, T.T_DATE, T.T_TIMESTAMP, T.T_DEC64, T.T_DEC128)
EIGHT = (T.T_I64, T.T_U64, T.T_F64, T.T_TIMESTAMP, T.T_DEC64)
DEC64_SIZES, DEC128_SIZES, DIV_SIZES = ((15, 2), (9, 0), (18, 4)), ((30, 4), (38, 6), (20, 0)), ((15, 8), (9, 4))
OP_NAMES = ["LOAD", "CONST", "PLUS", "MINUS", "MULTIPLY", "DIVIDE", "EQ", "NOTEQ", "LT", "LTE", "GT", "GTE", "AND", "OR", "NOT", "CAST", "IF",
            "IS_TRUE", "DT_PART", "DT_TRUNC"]


# ---- value pools -----------------------------------------------------------------------------------------------------------------
def int_pool(t):
    lo, hi = R.value_range(t)
    p = [lo, hi, 0, 1, hi - 1, lo + 1] + ([-1] if lo < 0 else [])
    if t == T.T_U64:
        p += [2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    return p


def pool(t, size=(0, 0)):
    """the edge values of a type (Decimal128: pairs that differ in the high word only)"""
    if t in (T.T_F32, T.T_F64):
        return FR.pool(R.NP[t])
    if t == T.T_BOOL:
        return np.array([False, True])
    if t == T.T_DATE:
        return np.array([DR.DATE_MIN, DR.DATE_MAX, 0, -1, 1, 10471, 19782], dtype=np.int32)
    if t == T.T_TIMESTAMP:
        return np.array([DR.TS_MIN, DR.TS_MAX, 0, -1, 1, 86399999999, -86400000001], dtype=np.int64)
    if t == T.T_DEC64:
        m = 10 ** size[0] - 1
        return np.array([0, 1, -1, m, -m, -2, m - 1], dtype=np.int64)
    if t == T.T_DEC128:
        m = 10 ** size[0] - 1
        hi = [k << 64 for k in (1, -1, 3) if abs(k << 64) + 7 <= m]
        return [0, 1, -1, m, -m, 7, -7] + [7 + h for h in hi] + [-7 + h for h in hi]
    return np.array(int_pool(t), dtype=R.NP[t])


def fill(rng, t, n, size=(0, 0), tame=False):
    """n values of type t: the pool first (as far as it fits), then draws over the whole range. tame: decimals stay small enough
    that a chain of nodes does not overflow on every row."""
    p = pool(t, size)
    if t == T.T_DEC128:
        m = 10 ** (min(size[0], 12) if tame else size[0]) - 1
        v = [int(rng.integers(-2 ** 62, 2 ** 62)) * int(rng.integers(1, 2 ** 62)) % (m + 1) * (1 if rng.integers(0, 2) else -1) for _ in range(n)]
        k = min(n, len(p))
        v[:k] = p[:k]
        return v
    if t in (T.T_F32, T.T_F64):
        v = FR.mixed(rng, n, R.NP[t], p_pool=0.15)
    elif t == T.T_BOOL:
        v = rng.integers(0, 2, n).astype(bool)
    elif t == T.T_DATE:
        v = rng.integers(DR.DATE_MIN, DR.DATE_MAX, n, endpoint=True).astype(np.int32)
    elif t == T.T_TIMESTAMP:
        v = rng.integers(DR.TS_MIN, DR.TS_MAX, n, endpoint=True).astype(np.int64)
    elif t == T.T_DEC64:
        m = 10 ** (min(size[0], 6) if tame else size[0]) - 1
        v = rng.integers(-m, m, n, endpoint=True).astype(np.int64)
        v[rng.random(n) < 0.1] = 0
    else:
        lo, hi = R.value_range(t)
        v = rng.integers(lo, hi, n, dtype=R.NP[t], endpoint=True)
        v[rng.random(n) < 0.1] = 0
    k = min(n, len(p))
    v[:k] = p[:k]
    return v


# ---- programs --------------------------------------------------------------------------------------------------------------------
Spec = collections.namedtuple("Spec", "dtype nullable scalar size")
Node = collections.namedtuple("Node", "reg dtype size dep raises")


def dt_part_type(part, src):
    """dbhip_dt_part_type restated: the narrowest unsigned type that holds the part; EPOCH_SECOND is Int64, DATE a Date"""
    if part == DR.EPOCH_SECOND:
        return T.T_I64
    if part == DR.DATE:
        return T.T_DATE
    if part in (DR.YEAR, DR.DAY_OF_YEAR, DR.ISO_YEAR):
        return T.T_U16
    if part in (DR.MICROSECOND, DR.YYYYMM, DR.YYYYMMDD):
        return T.T_U32
    return T.T_U64 if part in (DR.YYYYMMDDHH, DR.YYYYMMDDHHMMSS) else T.T_U8


def const_imm(t, value):
    if t in (T.T_F32, T.T_F64):
        return int(np.array([np.float32(value) if t == T.T_F32 else value], dtype=np.float64).view(np.uint64)[0])
    return int(value) & (2 ** 64 - 1)


class Builder:
    """device.ExprProgram's register discipline (lowest free register, operands released before the destination is chosen) without
    the library: result types come from expr_ref, decimal sizes from the oracle"""

    def __init__(self, specs, oracle):
        self.specs, self.oracle = list(specs), oracle
        self.ins, self.free, self.node = [], list(range(MAX_REGS)), {}
        self.n_dec = self.n_hidden = 0

    def emit(self, op, a, b, typ, imm=0, release=(), size=(0, 0), dep=False, raises=False):
        if op not in (T.EX_LOAD, T.EX_CONST):
            assert not set(reads((op, 0, a, b, typ, imm, size))) & set(self.free), "a node reads a released register"
        for r in set(release):
            if r not in self.free:
                self.free.append(r)
        self.free.sort()
        if not self.free:
            raise OutOfRoom
        dst = self.free.pop(0)
        self.ins.append((op, dst, a, b, typ, imm, tuple(size)))
        self.node[dst] = Node(dst, typ, tuple(size), dep, raises)
        return self.node[dst]

    def n_body(self):
        return sum(1 for i in self.ins if i[0] != T.EX_LOAD) + self.n_hidden

    def load(self, c):
        s = self.specs[c]
        return self.emit(T.EX_LOAD, c, 0, s.dtype, size=s.size, dep=s.nullable)

    def const(self, t, value, size=(0, 0)):
        return self.emit(T.EX_CONST, 0, 0, t, const_imm(t, value), size=size)._replace(raises=None)    # raises=None marks a constant

    def arith(self, op, x, y, release=()):
        dep, raises = x.dep or y.dep, bool(x.raises) or bool(y.raises)
        if x.dtype in R.DECIMALS or y.dtype in R.DECIMALS:
            ot, p, s = R.decimal_result(self.oracle, op, R.Val(x.dtype, None, size=x.size), R.Val(y.dtype, None, size=y.size))
            self.n_dec += 1
            self.n_hidden += (x.raises is None) + (y.raises is None)
            return self.emit(op, x.reg, y.reg, ot, release=release, size=(p, s), dep=dep, raises=True)
        return self.emit(op, x.reg, y.reg, R.arith_result_type(op, x.dtype, y.dtype), release=release, dep=dep, raises=raises or op == T.EX_DIVIDE)

    def cmp(self, op, x, y, release=()):
        return self.emit(op, x.reg, y.reg, T.T_BOOL, release=release, dep=x.dep or y.dep, raises=bool(x.raises) or bool(y.raises))

    def logic(self, op, x, y=None, release=()):
        if op == T.EX_NOT:
            return self.emit(op, x.reg, 0, T.T_BOOL, release=release, dep=x.dep, raises=bool(x.raises))
        assert not x.dep and not y.dep
        return self.emit(op, x.reg, y.reg, T.T_BOOL, release=release, raises=bool(x.raises) or bool(y.raises))

    def is_true(self, x, release=()):
        return self.emit(T.EX_IS_TRUE, x.reg, 0, T.T_BOOL, release=release, raises=bool(x.raises))

    def cast(self, x, t, release=(), size=(0, 0)):
        assert R.lossless_cast(x.dtype, t)
        size = (size[0] or 38, x.size[1]) if t == T.T_DEC128 else (0, 0)
        return self.emit(T.EX_CAST, x.reg, 0, t, release=release, size=size, dep=x.dep, raises=bool(x.raises))

    def if_(self, c, x, y, release=()):
        assert not c.dep and not x.raises and not y.raises and x.dtype == y.dtype
        return self.emit(T.EX_IF, c.reg, x.reg, x.dtype, imm=y.reg, release=release, size=(max(x.size[0], y.size[0]), x.size[1]), dep=x.dep or y.dep)

    def dt(self, op, x, code, typ, flags=0, offset_s=0, release=()):
        imm = (code & 0xFF) | ((flags & 0xFF) << 8) | ((int(offset_s) & 0xFFFFFFFF) << 32)
        return self.emit(op, x.reg, 0, typ, imm=imm, release=release, dep=x.dep, raises=bool(x.raises))


class OutOfRoom(Exception):
    pass


def reads(ins):
    op, _, a, b, _, imm, _ = ins
    if op in (T.EX_LOAD, T.EX_CONST):
        return ()
    if op in (T.EX_NOT, T.EX_CAST, T.EX_IS_TRUE, T.EX_DT_PART, T.EX_DT_TRUNC):
        return (a,)
    return (a, b, imm & 0xFF) if op == T.EX_IF else (a, b)


def live_width(ins, specs, root):
    """the peak total width (in LDS slots) of the live locations of a program: an input a LOADed register names lives from the start
    to its last read, a temporary from its definition to its last read (the root to the end); Decimal128 values are two slots wide;
    a decimal node with a constant operand holds a converted copy of it (up to two slots) beside it"""
    loc, width = {}, {}                      # register -> location id; location id -> width
    body = []                                # (reads [location], defined location, extra)
    for k, i in enumerate(ins):
        op, dst = i[0], i[1]
        if op == T.EX_LOAD:
            loc[dst] = ("in", i[2])
            width[loc[dst]] = 2 if specs[i[2]].dtype == T.T_DEC128 else 1
            continue
        rd = [loc[r] for r in reads(i)]
        loc[dst] = ("t", k)
        width[loc[dst]] = 2 if i[4] == T.T_DEC128 else 1
        extra = 0
        if op in R.ARITH and i[4] in R.DECIMALS:
            extra = 2 * sum(1 for l in rd if l[0] == "t" and ins[l[1]][0] == T.EX_CONST)
        body.append((rd, loc[dst], extra))
    last = {}
    for k, (rd, _, _) in enumerate(body):
        for l in rd:
            last[l] = k
    last[loc[root]] = len(body)
    live = {l for l in last if l[0] == "in"}
    peak = sum(width[l] for l in live)
    for k, (rd, d, extra) in enumerate(body):
        peak = max(peak, sum(width[l] for l in live) + extra)
        live = {l for l in live if last[l] > k}
        if last.get(d, -1) > k:
            live.add(d)
        peak = max(peak, sum(width[l] for l in live) + extra)
    return peak


Case = collections.namedtuple("Case", "seed klass specs ins root root_type root_size live")
Klass = collections.namedtuple("Klass", "nin all8 heavy div")


def _specs(rng, k):
    lo, hi = {2: (2 if k.div else 1, 2), 4: (3, 4), 8: (5, 8)}[k.nin]
    m = int(rng.integers(lo, hi + 1))
    out, wide = [], 0
    for c in range(m):
        if k.div and c < 2:
            t, size = T.T_DEC64, DIV_SIZES[int(rng.integers(0, 2))]
        else:
            t = (EIGHT if k.all8 else ALL_TYPES)[int(rng.integers(0, len(EIGHT if k.all8 else ALL_TYPES)))]
            if t == T.T_DEC128 and wide == MAX_WIDE_INPUTS:
                t = T.T_DEC64
            wide += t == T.T_DEC128
            size = (DEC64_SIZES if t == T.T_DEC64 else DEC128_SIZES)[int(rng.integers(0, 3))] if t in R.DECIMALS else (0, 0)
        scalar = (not k.all8) and c > 0 and rng.random() < 0.2
        out.append(Spec(t, bool(rng.random() < 0.35), bool(scalar), size))
    if not k.all8 and not k.div and all(s.dtype in EIGHT and not s.scalar for s in out):
        out[-1] = Spec(T.T_I16, out[-1].nullable, False, (0, 0))           # one input that is not a plain 8-byte column
    return out


def _pick(rng, xs):
    return xs[int(rng.integers(0, len(xs)))]


def _const_for(rng, b, x):
    """a constant of x's type (Decimal128: a Decimal64 one widened by CAST)"""
    t = x.dtype
    if t == T.T_DEC128:
        c = b.const(T.T_DEC64, int(rng.integers(-999, 1000)), (min(18, x.size[0]), x.size[1]))
        return b.cast(c, T.T_DEC128, release=(c.reg,), size=(x.size[0], 0))
    if t in (T.T_F32, T.T_F64):
        return b.const(t, _pick(rng, [0.0, -0.0, 1.5, -2.5, float("nan"), float("inf"), 1e10]))
    if t == T.T_BOOL:
        return b.const(t, int(rng.integers(0, 2)))
    if t == T.T_DEC64:
        return b.const(t, int(rng.integers(-999, 1000)), x.size)
    lo, hi = R.value_range(t)
    return b.const(t, _pick(rng, [lo, hi, 0, 1, int(rng.integers(max(lo, -1000), min(hi, 1000) + 1))]))


def _clean_cond(rng, b, c, release):
    """a Boolean an IF / AND / OR may read: IS_TRUE over a nullable one"""
    return b.is_true(c, release=release) if c.dep else c


def _generate(rng, k, want_root, feature, oracle):
    specs = _specs(rng, k)
    b = Builder(specs, oracle)
    skip = int(rng.integers(2, len(specs))) if len(specs) > 2 and rng.random() < 0.15 else -1      # an input the program never reads
    vals = [b.load(c) for c in range(len(specs)) if c != skip]
    keep_p = 0.85 if k.heavy else 0.3
    budget = int(rng.integers(10, 19)) if k.heavy else int(rng.integers(3, 15))

    def done(x, y=None):
        """which operands leave the pool after a node read them"""
        rel = []
        for o in {x.reg, y.reg if y is not None else x.reg}:
            if rng.random() > keep_p or len(b.free) < 4:
                rel.append(o)
        vals[:] = [v for v in vals if v.reg not in rel]
        return tuple(rel)

    def of(pred):
        return [v for v in vals if pred(v)]

    def dec_ok(op, x, y):
        if b.n_dec >= MAX_DEC:
            return False
        sa, sb = x.size[1] if x.dtype in R.DECIMALS else 0, y.size[1] if y.dtype in R.DECIMALS else 0
        divides = op == T.EX_DIVIDE or (op == T.EX_MULTIPLY and sa + sb > max(sa, sb, 12))
        if divides and not k.div:
            return False
        try:
            R.decimal_result(oracle, op, R.Val(x.dtype, None, size=x.size), R.Val(y.dtype, None, size=y.size))
        except R.Refused:
            return False
        return True

    if k.div:                                              # the node that needs the long division, first
        x, y = vals[0], vals[1]
        op = T.EX_DIVIDE if rng.random() < 0.5 or x.size[1] + y.size[1] <= 12 else T.EX_MULTIPLY
        vals.append(b.arith(op, x, y, release=done(x, y)))
    if feature == "wide_if":
        src = of(lambda v: v.dtype == T.T_DEC64 and not v.raises)
        x = b.cast(src[0], T.T_DEC128) if src else _const_for(rng, b, Node(0, T.T_DEC128, (30, 2), False, False))
        y = _const_for(rng, b, x)
        num = of(lambda v: v.dtype in R.NUMBERS + (T.T_DEC64, T.T_DATE, T.T_TIMESTAMP))
        c = b.cmp(_pick(rng, R.CMPS), num[0], _const_for(rng, b, num[0])) if num else b.const(T.T_BOOL, 1)
        c = _clean_cond(rng, b, c, (c.reg,))
        vals.append(b.if_(c, x, y, release=(c.reg, x.reg, y.reg)))
    if feature == "wide_cast":
        src = of(lambda v: v.dtype == T.T_DEC64)
        x = src[0] if src else b.const(T.T_DEC64, -12345, (15, 2))
        vals.append(b.cast(x, T.T_DEC128, release=done(x) if src else (x.reg,)))

    steps = 0
    while steps < budget and b.n_body() < MAX_INS - 8 and len(b.free) >= 3:
        steps += 1
        act = _pick(rng, ["arith", "arith", "arith", "carith", "cmp", "cmp", "logic", "not", "if", "cast", "dec", "dt", "dead", "self"])
        nums = of(lambda v: v.dtype in R.NUMBERS)
        bools = of(lambda v: v.dtype == T.T_BOOL)
        if act in ("arith", "self") and nums:
            x = _pick(rng, nums)
            y = x if act == "self" else _pick(rng, nums)
            vals.append(b.arith(_pick(rng, R.ARITH), x, y, release=done(x, y)))
        elif act == "carith" and nums:
            x = _pick(rng, nums)
            c = _const_for(rng, b, x)
            vals.append(b.arith(_pick(rng, R.ARITH), *((x, c) if rng.random() < 0.5 else (c, x)), release=done(x) + (c.reg,)))
        elif act == "cmp":
            x = _pick(rng, of(lambda v: True))
            same = of(lambda v: v.dtype == x.dtype and (x.dtype not in R.DECIMALS or v.size[1] == x.size[1]))
            if rng.random() < 0.5 and len(same) > 1:
                y = _pick(rng, same)
                vals.append(b.cmp(_pick(rng, R.CMPS), x, y, release=done(x, y)))
            else:
                c = _const_for(rng, b, x)
                vals.append(b.cmp(_pick(rng, R.CMPS), x, c, release=done(x) + (c.reg,)))
        elif act == "logic" and len(bools) >= 2:
            x, y = _pick(rng, bools), _pick(rng, bools)
            if x.reg == y.reg and x.dep:
                continue
            rel = done(x, y)
            cx = _clean_cond(rng, b, x, (x.reg,) if x.reg in rel else ())
            cy = cx if y.reg == x.reg else _clean_cond(rng, b, y, (y.reg,) if y.reg in rel else ())
            extra = tuple(c.reg for c, o in ((cx, x), (cy, y)) if c.reg != o.reg)
            vals.append(b.logic(_pick(rng, [T.EX_AND, T.EX_OR]), cx, cy, release=tuple(r for r in rel if r in (cx.reg, cy.reg)) + extra))
        elif act == "not" and bools:
            x = _pick(rng, bools)
            vals.append(b.logic(T.EX_NOT, x, release=done(x)))
        elif act == "if" and bools:
            c = _pick(rng, bools)
            cand = of(lambda v: not v.raises and v.reg != c.reg)
            if not cand:
                continue
            x = _pick(rng, cand)
            same = [v for v in cand if v.dtype == x.dtype and (x.dtype not in R.DECIMALS or v.size[1] == x.size[1])]
            rel = done(c)
            cc = _clean_cond(rng, b, c, rel)
            crel = (cc.reg,) if cc.reg != c.reg or c.reg in rel else ()
            if rng.random() < 0.5 and len(same) > 1:
                y = _pick(rng, same)
                vals.append(b.if_(cc, x, y, release=crel + done(x, y)))
            else:
                y = _const_for(rng, b, x)
                pair = (x, y) if rng.random() < 0.5 else (y, x)
                vals.append(b.if_(cc, pair[0], pair[1], release=crel + done(x) + (y.reg,)))
        elif act == "cast":
            src = of(lambda v: v.dtype in R.NUMBERS + (T.T_DEC64,))
            if not src:
                continue
            x = _pick(rng, src)
            to = [t for t in R.NUMBERS + (T.T_DEC128,) if t != x.dtype and R.lossless_cast(x.dtype, t)]
            if to:
                vals.append(b.cast(x, _pick(rng, to), release=done(x)))
        elif act == "dec":
            decs = of(lambda v: v.dtype in R.DECIMALS)
            if not decs:
                continue
            x = _pick(rng, decs)
            others = decs + of(lambda v: v.dtype in R.INT_PROPS)
            y = _pick(rng, others) if rng.random() < 0.7 else b.const(T.T_U8, int(rng.integers(1, 100)))
            op = _pick(rng, R.ARITH)
            pair = (x, y) if rng.random() < 0.6 else (y, x)
            if dec_ok(op, *pair):
                rel = done(x, y) if y.raises is not None else done(x) + (y.reg,)
                vals.append(b.arith(op, pair[0], pair[1], release=rel))
            elif y.raises is None:
                b.free.append(y.reg)                     # the constant was not used: a dead store
        elif act == "dt":
            ds = of(lambda v: v.dtype in (T.T_DATE, T.T_TIMESTAMP))
            if not ds:
                continue
            x = _pick(rng, ds)
            ts = x.dtype == T.T_TIMESTAMP
            off = _pick(rng, DR.OFFSETS) if ts else 0
            if rng.random() < 0.5:
                part = int(_pick(rng, list(range(19)) if ts else list(DR.DATE_PARTS)))
                vals.append(b.dt(T.EX_DT_PART, x, part, dt_part_type(part, x.dtype), offset_s=off, release=done(x)))
            else:
                unit = int(rng.integers(0, 8 if ts else 5))
                out = T.T_TIMESTAMP if ts and (unit > DR.U_DAY or rng.random() < 0.5) else T.T_DATE
                flags = DR.WEEK_SUNDAY if unit == DR.U_WEEK and rng.random() < 0.5 else 0
                vals.append(b.dt(T.EX_DT_TRUNC, x, unit, out, flags, off, release=done(x)))
        elif act == "dead" and nums:
            x = _pick(rng, nums)
            d = b.arith(T.EX_PLUS, x, x)                  # a value nobody reads; its register is overwritten by the next node
            b.free.append(d.reg)

    # fold the numbers that are still around into one value, so that what was kept alive is read again
    nums = of(lambda v: v.dtype in R.NUMBERS)
    while len(nums) > 1 and b.n_body() < MAX_INS - 6:
        x, y = nums[0], nums[1]
        r = b.arith(_pick(rng, R.ARITH[:3]), x, y, release=(x.reg, y.reg))
        vals[:] = [v for v in vals if v.reg not in (x.reg, y.reg)] + [r]
        nums = of(lambda v: v.dtype in R.NUMBERS)
    root = vals[-1]
    if want_root is not None and root.dtype != want_root:
        have = of(lambda v: v.dtype == want_root)
        if have and rng.random() < 0.5:
            root = have[-1]
        else:                                             # if(cond, x, y) of the wanted type; the condition reads what was computed
            src = nums[0] if nums else vals[-1]
            if src.dtype == T.T_BOOL:
                c = src
            else:
                k0 = _const_for(rng, b, src)
                c = b.cmp(_pick(rng, R.CMPS), src, k0, release=(k0.reg,))
            c = _clean_cond(rng, b, c, (c.reg,) if c.reg != src.reg else ())
            have = [v for v in have if not v.raises]
            ins_ = [i for i, s in enumerate(specs) if s.dtype == want_root]
            if have:
                x = have[-1]
            elif ins_ and rng.random() < 0.7:
                x = b.load(ins_[0])
            else:
                size = {T.T_DEC64: (15, 2), T.T_DEC128: (30, 2)}.get(want_root, (0, 0))
                x = _const_for(rng, b, Node(0, want_root, size, False, False))
            y = _const_for(rng, b, x)
            root = b.if_(c, x, y, release=(y.reg,))
    elif want_root is None and rng.random() < 0.1:
        root = vals[0]                                    # the result IS an input column
    return Case(None, k, specs, b.ins, root.reg, root.dtype, root.size, live_width(b.ins, specs, root.reg)), b


def within_limits(case):
    """every documented limit, checked on the instruction list itself"""
    body = [i for i in case.ins if i[0] != T.EX_LOAD]
    dec = [i for i in body if i[0] in R.ARITH and i[4] in R.DECIMALS]
    consts = {}
    hidden = 0
    for i in case.ins:
        if i in dec:
            hidden += sum(1 for r in (i[2], i[3]) if consts.get(r))
        consts[i[1]] = i[0] == T.EX_CONST
    return (len(body) + hidden <= MAX_INS and all(0 <= i[1] < MAX_REGS for i in case.ins) and len(case.specs) <= MAX_INPUTS
            and sum(s.dtype == T.T_DEC128 for s in case.specs) <= MAX_WIDE_INPUTS and len(dec) <= MAX_DEC and case.live <= MAX_LIVE)


def in_class(case):
    k, s = case.klass, case.specs
    nin_ok = {2: len(s) <= 2, 4: 2 < len(s) <= 4, 8: 4 < len(s) <= 8}[k.nin]
    all8 = all(x.dtype in EIGHT and not x.scalar for x in s)
    return nin_ok and (k.div or all8 == k.all8) and (k.div or (case.live >= 9) == k.heavy) and (not k.heavy or case.live >= 9) and has_division(case) == k.div


def has_division(case):
    types = {}
    for op, dst, a, b, typ, imm, size in case.ins:
        if op in R.ARITH and typ in R.DECIMALS:
            sa, sb = types[a][1][1] if types[a][0] in R.DECIMALS else 0, types[b][1][1] if types[b][0] in R.DECIMALS else 0
            if op == T.EX_DIVIDE or (op == T.EX_MULTIPLY and sa + sb > max(sa, sb, 12)):
                return True
        types[dst] = (typ, size)
    return False


def generate(seed, klass, want_root, feature, oracle):
    for attempt in range(400):
        rng = np.random.default_rng([seed, attempt])
        try:
            case, _ = _generate(rng, klass, want_root, feature, oracle)
        except OutOfRoom:
            continue
        if within_limits(case) and in_class(case) and (want_root is None or case.root_type == want_root):
            return case._replace(seed=seed)
    raise AssertionError(("no program for", seed, klass, want_root, feature))


KLASSES = [Klass(nin, all8, heavy, False) for nin in (2, 4, 8) for all8 in (True, False) for heavy in (False, True)] + \
          [Klass(nin, False, False, True) for nin in (2, 4, 8)]
SEEDS_PER_KLASS, SEEDS_PER_DIV = 8, 4


def seed_list():
    """(seed, class, wanted root type | None, feature | None): every second seed of a class asks for a root type, cycling through all
    fifteen; the first seeds of the classes with mixed inputs force a two-slot IF / CAST"""
    out, shaped = [], 0
    for ki, k in enumerate(KLASSES):
        for j in range(SEEDS_PER_DIV if k.div else SEEDS_PER_KLASS):
            want = None
            if j % 2 == 1 and not k.div:
                want = ALL_TYPES[shaped % len(ALL_TYPES)]
                shaped += 1
            feature = {0: "wide_if", 2: "wide_cast"}.get(j) if not k.all8 and not k.div else None
            out.append((1000 * ki + j, k, want, feature))
    return out


_CASES = None


def cases(oracle):
    global _CASES
    if _CASES is None:
        _CASES = [generate(s, k, w, f, oracle) for s, k, w, f in seed_list()]
    return _CASES


def make_inputs(case, n, seed=0):
    """[expr_ref.Input] of n rows for a case: pool values first, then draws; validity 3/4 valid; a scalar holds one value"""
    rng = np.random.default_rng([case.seed, n, seed])
    out = []
    for s in case.specs:
        m = 1 if s.scalar else n
        v = fill(rng, s.dtype, 8 if s.scalar else n, s.size, tame=True)
        if s.scalar:
            j = int(rng.integers(0, 8))
            v = v[j:j + 1]
        valid = (rng.random(m) < 0.75) if s.nullable else None
        out.append(R.Input(s.dtype, v, valid, s.scalar, *s.size))
    return out


def census(cs):
    """how often each op, node type, root type, steering class and the two-slot IF / CAST occur over a list of cases"""
    c = dict(op=collections.Counter(), node_type=collections.Counter(), root_type=collections.Counter(), klass=collections.Counter(),
             wide_if=0, wide_cast=0, live9=0, scalar_inputs=0, nullable_inputs=0, x_op_x=0, root_is_input=0)
    for case in cs:
        c["klass"][case.klass] += 1
        c["root_type"][case.root_type] += 1
        c["live9"] += case.live >= 9
        c["scalar_inputs"] += sum(s.scalar for s in case.specs)
        c["nullable_inputs"] += sum(s.nullable for s in case.specs)
        wide_if = wide_cast = False
        for i in case.ins:
            c["op"][OP_NAMES[i[0]]] += 1
            c["node_type"][i[4]] += 1
            wide_if |= i[0] == T.EX_IF and i[4] == T.T_DEC128
            wide_cast |= i[0] == T.EX_CAST and i[4] == T.T_DEC128
            c["x_op_x"] += i[0] in R.ARITH + R.CMPS and i[2] == i[3]
        c["root_is_input"] += [i for i in case.ins if i[1] == case.root][-1][0] == T.EX_LOAD
        c["wide_if"] += wide_if
        c["wide_cast"] += wide_cast
    return c
