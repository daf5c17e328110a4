"""Plain reference for the register programs of dbhip_expr_eval and the fused aggregation (csrc/dev_expr.h, k_expr.hip): one node at
a time over host arrays, a column per node, like the reference's Evaluator::run. It shares nothing with the device code and does not
ask the library for a result type.

* arith_result_type    ResultTypeOfBinary restated from arithmetics_type.rs: the widest operand doubled (up to 64 bits), signed if
                       either side is (always for minus), float if either side is, `/` always Float64
* lossless_cast        the CAST pairs a program may hold: every source value is a destination value (Decimal64 -> Decimal128 too)
* int_node_py / _np    an integer + - *: both operands cast `as` the result type, then the wrapping operation — once over Python
                       integers (mod 2^bits, reinterpreted), once in numpy uint64 arithmetic; tests/test_expr_ref_cpu.py holds them together
* run                  the evaluator: values, validity, raising rows and type of one register

Float nodes work in Float64, one rounding per node, never fused; a Float32 register is the Float64 value rounded to Float32 once.
DIVIDE is f64(a) / f64(b); a row raises where f64(b) == 0.0 (-0.0 too, a NaN does not) and holds 0. A value depends on the set of
nullable inputs below it: it is valid where all of them are, and a node raises only on such rows. IS_TRUE folds the operand's validity
into the value and depends on nothing; IF is a select whose set is then | else. Decimal nodes go through the oracle's binary_decimal
(pinned by tests/test_dec_edges_cpu.py), the calendar nodes through tests/datetime_ref.py."""
import ctypes as C

import numpy as np

from databend_amd import _lib as T
from tests import datetime_ref as DR
from tests import float_ref as FR
from tests import oracle_lib as O

# type -> (bits, class): 's' signed, 'u' unsigned, 'f' float, 'b' Boolean, 'w' 128-bit
INFO = {T.T_I8: (8, "s"), T.T_I16: (16, "s"), T.T_I32: (32, "s"), T.T_I64: (64, "s"), T.T_U8: (8, "u"), T.T_U16: (16, "u"), T.T_U32: (32, "u"),
        T.T_U64: (64, "u"), T.T_F32: (32, "f"), T.T_F64: (64, "f"), T.T_BOOL: (1, "b"), T.T_DATE: (32, "s"), T.T_TIMESTAMP: (64, "s"),
        T.T_DEC64: (64, "s"), T.T_DEC128: (128, "w")}
NUMBERS = (T.T_I8, T.T_I16, T.T_I32, T.T_I64, T.T_U8, T.T_U16, T.T_U32, T.T_U64, T.T_F32, T.T_F64)
NP = {T.T_I8: np.int8, T.T_I16: np.int16, T.T_I32: np.int32, T.T_I64: np.int64, T.T_U8: np.uint8, T.T_U16: np.uint16, T.T_U32: np.uint32,
      T.T_U64: np.uint64, T.T_F32: np.float32, T.T_F64: np.float64, T.T_DATE: np.int32, T.T_TIMESTAMP: np.int64, T.T_DEC64: np.int64}
DECIMALS = (T.T_DEC64, T.T_DEC128)
INT_PROPS = {T.T_I8: (3, 0), T.T_U8: (3, 0), T.T_I16: (5, 0), T.T_U16: (5, 0), T.T_I32: (10, 0), T.T_U32: (10, 0), T.T_I64: (19, 0), T.T_U64: (20, 0)}
ARITH = (T.EX_PLUS, T.EX_MINUS, T.EX_MULTIPLY, T.EX_DIVIDE)
CMPS = (T.EX_EQ, T.EX_NOTEQ, T.EX_LT, T.EX_LTE, T.EX_GT, T.EX_GTE)
OP_OF = {T.EX_PLUS: T.OP_PLUS, T.EX_MINUS: T.OP_MINUS, T.EX_MULTIPLY: T.OP_MULTIPLY, T.EX_DIVIDE: T.OP_DIVIDE}
_BY_SHAPE = {(b, c): t for t, (b, c) in INFO.items() if t in NUMBERS}


class Refused(Exception):
    """the program is outside what the library documents as fused (a cast that can overflow, a raising IF branch, ...)"""


def arith_result_type(op, ta, tb):
    """op: T.EX_PLUS .. T.EX_DIVIDE over two of the ten number types"""
    (ba, ca), (bb, cb) = INFO[ta], INFO[tb]
    if op == T.EX_DIVIDE:
        return T.T_F64
    bits = min(2 * max(ba, bb), 64)
    if "f" in (ca, cb):
        return _BY_SHAPE[(bits, "f")]
    signed = op == T.EX_MINUS or "s" in (ca, cb)
    return _BY_SHAPE[(bits, "s" if signed else "u")]


def value_range(t):
    bits, cls = INFO[t]
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if cls == "s" else (0, (1 << bits) - 1)


def lossless_cast(src, dst):
    """every value of src is a value of dst: integer ranges nest; an integer fits a float's significand (24 / 53 bits); a float widens"""
    if src == T.T_DEC64 and dst == T.T_DEC128:
        return True
    if src not in NUMBERS or dst not in NUMBERS:
        return False
    (bs, cs), (bd, cd) = INFO[src], INFO[dst]
    if cs == "f":
        return cd == "f" and bd >= bs
    lo, hi = value_range(src)
    if cd == "f":
        lim = 1 << (24 if bd == 32 else 53)
        return -lim <= lo and hi <= lim
    dlo, dhi = value_range(dst)
    return dlo <= lo and hi <= dhi


# ---- the integer node, twice -----------------------------------------------------------------------------------------------------
def wrap_py(v, bits, signed):
    v &= (1 << bits) - 1
    return v - (1 << bits) if signed and v >> (bits - 1) else v


def int_node_py(op, a, b, bits, signed):
    """a, b: lists of Python integers (the operands' values) -> list of Python integers of the result type"""
    f = {T.EX_PLUS: lambda x, y: x + y, T.EX_MINUS: lambda x, y: x - y, T.EX_MULTIPLY: lambda x, y: x * y}[op]
    return [wrap_py(f(wrap_py(x, bits, signed), wrap_py(y, bits, signed)), bits, signed) for x, y in zip(a, b)]


def _as_u64(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.int64 else x.astype(np.uint64)


def wrap_np(u, bits, signed):
    """u: uint64 images -> int64 (signed) or uint64 values of a `bits`-wide type"""
    sh = np.uint64(64 - bits)
    if signed:
        return np.right_shift(np.left_shift(u, sh).view(np.int64), np.int64(64 - bits))
    return np.right_shift(np.left_shift(u, sh), sh)


def int_node_np(op, a, b, bits, signed):
    """a, b: int64 / uint64 arrays -> int64 / uint64 array"""
    x, y = _as_u64(wrap_np(_as_u64(a), bits, signed)), _as_u64(wrap_np(_as_u64(b), bits, signed))
    with np.errstate(over="ignore"):
        z = x + y if op == T.EX_PLUS else (x - y if op == T.EX_MINUS else x * y)
    return wrap_np(z, bits, signed)


def of_cmp3_np(a, b):
    """OrderedFloat's three-way compare over float64 arrays: NaN == NaN, NaN above everything (float_ref.of_cmp, vectorised)"""
    an, bn = np.isnan(a), np.isnan(b)
    with np.errstate(invalid="ignore"):
        c = (a > b).astype(np.int8) - (a < b).astype(np.int8)
    return np.where(an | bn, an.astype(np.int8) - bn.astype(np.int8), c)


# ---- inputs and values -----------------------------------------------------------------------------------------------------------
class Input:
    """one input column: values (numpy array of the type's dtype; Boolean: bool array; Decimal128: list of Python integers),
    validity (bool array, one element for a scalar) or None, is_scalar"""

    def __init__(self, dtype, values, validity=None, is_scalar=False, precision=0, scale=0):
        self.dtype, self.is_scalar, self.precision, self.scale = dtype, bool(is_scalar), precision, scale
        self.values = list(values) if dtype == T.T_DEC128 else np.ascontiguousarray(values, dtype=bool if dtype == T.T_BOOL else NP[dtype])
        self.validity = None if validity is None else np.asarray(validity, dtype=bool)
        assert not is_scalar or len(self.values) == 1


class Val:
    def __init__(self, dtype, data, dep=frozenset(), size=(0, 0), may_raise=False):
        self.dtype, self.data, self.dep, self.size, self.may_raise = dtype, data, dep, size, may_raise


class Result:
    """raising: the rows on which some node raised; raise_events: how often a node raised (a row on which two nodes raise counts twice:
    every node reports its own rows, like the per-node functions; dbhip_expr_eval's err_count adds them up)"""

    def __init__(self, dtype, size, values, validity, raising, raise_events):
        self.type, self.size, self.values, self.validity, self.raising, self.raise_events = dtype, size, values, validity, raising, raise_events


def _store(cls, x):
    """the evaluator's image of a column: int64 / uint64 / float64 arrays, a list of Python integers for 128-bit values"""
    if cls == "w":
        return [int(v) for v in x]
    return np.asarray(x).astype({"s": np.int64, "u": np.uint64, "b": np.uint64, "f": np.float64}[cls])


def const_value(dtype, imm):
    bits, cls = INFO[dtype]
    if cls == "f":
        v = float(np.array([imm], np.uint64).view(np.float64)[0])
        return float(np.float32(v)) if dtype == T.T_F32 else v
    if cls == "b":
        return imm & 1
    return wrap_py(imm, bits, cls == "s")


def same(got, exp):
    """test_gpu_parity.same_bits: bit-equal, any NaN equals any NaN, signed zeros are told apart"""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    if got.dtype != exp.dtype or got.shape != exp.shape:
        return False
    if got.dtype.kind == "f":
        ng, ne = np.isnan(got), np.isnan(exp)
        if not np.array_equal(ng, ne):
            return False
        got, exp = np.where(ng, 0, got), np.where(ne, 0, exp)
    return np.array_equal(got.view(np.uint8), exp.view(np.uint8))


def _host_col(v, n):
    if v.dtype == T.T_DEC128:
        return O.HostCol(T.T_DEC128, O.i128_array(v.data), None, v.size[0], v.size[1])
    if v.dtype == T.T_DEC64:
        return O.HostCol(T.T_DEC64, v.data.astype(np.int64), None, v.size[0], v.size[1])
    return O.HostCol(v.dtype, v.data.astype(NP[v.dtype]))


def decimal_result(oracle, op, va, vb):
    """(type, precision, scale) of a decimal node, from the oracle's result_size"""
    ap = va.size if va.dtype in DECIMALS else INT_PROPS[va.dtype]
    bp = vb.size if vb.dtype in DECIMALS else INT_PROPS[vb.dtype]
    p, s = C.c_int(), C.c_int()
    if oracle.orc_decimal_result_size(OP_OF[op], ap[0], ap[1], bp[0], bp[1], C.byref(p), C.byref(s)) != 0:
        raise Refused("decimal result size")
    return (T.T_DEC64 if p.value <= 18 else T.T_DEC128), p.value, s.value


def _decimal_node(oracle, op, va, vb, n):
    from tests.test_gpu_fused import oracle_decimal
    for v in (va, vb):
        if v.dtype not in DECIMALS and v.dtype not in INT_PROPS:
            raise Refused("decimal arithmetic with a non-integer operand")
    vals, ok, ot, p, s = oracle_decimal(oracle, OP_OF[op], _host_col(va, n), _host_col(vb, n), n)
    bad = ~ok
    vals = [1 if b else v for v, b in zip(vals, bad.tolist())]          # error rows hold T::one(), like the reference builders
    return Val(ot, _store("w" if ot == T.T_DEC128 else "s", vals), va.dep | vb.dep, (p, s), True), bad


def run(ins, inputs, n, out, oracle=None, use_numpy=False):
    """ins: the instruction tuples of device.ExprProgram (op, dst, a, b, type, imm, (precision, scale)); inputs: [Input];
    out: the register to read, or ("input", c). -> Result. Raises Refused for what the library documents as not fused.
    use_numpy: integer nodes, comparisons and the float compare in numpy arithmetic instead of Python integers."""
    valid_of = []
    for c in inputs:
        if c.validity is None:
            valid_of.append(None)
        else:
            valid_of.append(np.full(n, bool(c.validity[0])) if c.is_scalar else c.validity[:n].copy())

    def dep_valid(dep):
        m = np.ones(n, bool)
        for c in dep:
            m &= valid_of[c]
        return m

    def load(i):
        c = inputs[i]
        cls = INFO[c.dtype][1]
        data = c.values
        if c.is_scalar:
            data = [data[0]] * n if cls == "w" else np.repeat(data[:1], n)
        else:
            data = data[:n]
        return Val(c.dtype, _store(cls, data), frozenset([i]) if c.validity is not None else frozenset(), (c.precision, c.scale))

    reg = {}
    raising = np.zeros(n, bool)
    events = 0
    for op, dst, a, b, typ, imm, size in ins:
        size = tuple(size)
        if op == T.EX_LOAD:
            assert inputs[a].dtype == typ
            reg[dst] = load(a)
            continue
        if op == T.EX_CONST:
            if typ == T.T_DEC128:
                raise Refused("CONST of Decimal128")
            cls = INFO[typ][1]
            reg[dst] = Val(typ, _store(cls, np.full(n, const_value(typ, imm), dtype=object)), frozenset(), size)
            continue
        va = reg[a]
        ca = INFO[va.dtype][1]
        if op in ARITH:
            vb = reg[b]
            if va.dtype in DECIMALS or vb.dtype in DECIMALS:
                r, bad = _decimal_node(oracle, op, va, vb, n)
                assert r.dtype == typ and (not size[0] or size == r.size), (typ, size, r.dtype, r.size)
                raising |= bad & dep_valid(r.dep)
                events += int((bad & dep_valid(r.dep)).sum())
                r.may_raise = True          # (the library knows some decimal nodes cannot raise; the reference does not need to)
                reg[dst] = r
                continue
            ot = arith_result_type(op, va.dtype, vb.dtype)
            assert ot == typ, ("the node's type is not ResultTypeOfBinary's", op, va.dtype, vb.dtype, typ, ot)
            bits, cls = INFO[ot]
            dep = va.dep | vb.dep
            may = va.may_raise or vb.may_raise
            if cls == "f":
                with np.errstate(all="ignore"):
                    x, y = va.data.astype(np.float64), vb.data.astype(np.float64)
                    if op == T.EX_DIVIDE:
                        zero = y == 0.0
                        r = np.where(zero, 0.0, x / np.where(zero, 1.0, y))
                        raising |= zero & dep_valid(dep)
                        events += int((zero & dep_valid(dep)).sum())
                        may = True
                    else:
                        r = x + y if op == T.EX_PLUS else (x - y if op == T.EX_MINUS else x * y)
                    if ot == T.T_F32:
                        r = r.astype(np.float32).astype(np.float64)
                reg[dst] = Val(ot, r, dep, may_raise=may)
            elif use_numpy:
                reg[dst] = Val(ot, int_node_np(op, va.data, vb.data, bits, cls == "s"), dep, may_raise=may)
            else:
                r = int_node_py(op, va.data.tolist(), vb.data.tolist(), bits, cls == "s")
                reg[dst] = Val(ot, np.array(r, dtype=np.int64 if cls == "s" else np.uint64), dep, may_raise=may)
        elif op in CMPS:
            vb = reg[b]
            assert va.dtype == vb.dtype and typ == T.T_BOOL and (va.dtype not in DECIMALS or va.size[1] == vb.size[1])
            name = FR.CMP_OPS[op - T.EX_EQ]
            if ca == "f":
                c3 = of_cmp3_np(va.data, vb.data) if use_numpy else FR.cmp3_array(va.data, vb.data)
            elif ca == "w" or not use_numpy:
                x, y = (va.data, vb.data) if ca == "w" else (va.data.tolist(), vb.data.tolist())
                c3 = np.array([(p > q) - (p < q) for p, q in zip(x, y)], dtype=np.int8).reshape(n)
            else:
                c3 = (va.data > vb.data).astype(np.int8) - (va.data < vb.data).astype(np.int8)
            reg[dst] = Val(T.T_BOOL, FR.holds_array(name, c3).astype(np.uint64), va.dep | vb.dep, may_raise=va.may_raise or vb.may_raise)
        elif op in (T.EX_AND, T.EX_OR):
            vb = reg[b]
            assert va.dtype == vb.dtype == typ == T.T_BOOL
            dep = va.dep | vb.dep
            r = (va.data & vb.data if op == T.EX_AND else va.data | vb.data) & np.uint64(1)
            reg[dst] = Val(T.T_BOOL, r, dep, may_raise=va.may_raise or vb.may_raise)
        elif op == T.EX_NOT:
            assert va.dtype == typ == T.T_BOOL
            reg[dst] = Val(T.T_BOOL, (va.data ^ np.uint64(1)) & np.uint64(1), va.dep, may_raise=va.may_raise)
        elif op == T.EX_IS_TRUE:
            assert va.dtype == typ == T.T_BOOL
            reg[dst] = Val(T.T_BOOL, (va.data & np.uint64(1)) * dep_valid(va.dep).astype(np.uint64), frozenset(), may_raise=va.may_raise)
        elif op == T.EX_IF:
            vt, ve = reg[b], reg[imm & 0xFF]
            assert va.dtype == T.T_BOOL and vt.dtype == ve.dtype == typ and (typ not in DECIMALS or vt.size[1] == ve.size[1])
            if vt.may_raise or ve.may_raise:
                raise Refused("a branch of if() can raise")
            if va.dep:
                raise Refused("if() on a nullable condition")
            t = (va.data & np.uint64(1)).astype(bool)
            if INFO[typ][1] == "w":
                r = [x if c else y for c, x, y in zip(t.tolist(), vt.data, ve.data)]
            else:
                r = np.where(t, vt.data, ve.data)
            reg[dst] = Val(typ, r, vt.dep | ve.dep, (max(vt.size[0], ve.size[0]), vt.size[1]))
        elif op == T.EX_CAST:
            if not lossless_cast(va.dtype, typ) or (typ == T.T_DEC128 and size[0] and (size[1] != va.size[1] or size[0] < va.size[0])):
                raise Refused("CAST %d -> %d" % (va.dtype, typ))
            if typ == T.T_DEC128:
                reg[dst] = Val(typ, _store("w", va.data.tolist()), va.dep, (size[0] or 38, va.size[1]), va.may_raise)
            else:
                cls = INFO[typ][1]
                with np.errstate(all="ignore"):
                    r = _store(cls, va.data)
                    if typ == T.T_F32:
                        r = r.astype(np.float32).astype(np.float64)
                reg[dst] = Val(typ, r, va.dep, va.size, va.may_raise)
        elif op in (T.EX_DT_PART, T.EX_DT_TRUNC):
            code, flags, off = imm & 0xFF, (imm >> 8) & 0xFF, wrap_py(imm >> 32, 32, True)
            src = DR.SRC_TS if va.dtype == T.T_TIMESTAMP else DR.SRC_DATE
            assert va.dtype in (T.T_DATE, T.T_TIMESTAMP)
            if op == T.EX_DT_PART:
                r = DR.part(code, va.data, src, tz=off)
            else:
                r = DR.trunc(code, flags, va.data, src, DR.SRC_TS if typ == T.T_TIMESTAMP else DR.SRC_DATE, off)
            reg[dst] = Val(typ, _store(INFO[typ][1], r), va.dep, may_raise=va.may_raise)
        else:
            raise AssertionError(("unknown op", op))
    v = load(out[1]) if isinstance(out, tuple) else reg[out]
    cls = INFO[v.dtype][1]
    if cls == "w":
        values = list(v.data)
    elif cls == "b":
        values = v.data.astype(bool)
    else:
        with np.errstate(all="ignore"):
            values = v.data.astype(NP[v.dtype])
    return Result(v.dtype, v.size, values, dep_valid(v.dep) if v.dep else None, np.flatnonzero(raising), events)


def wrapping_sum(values, valid, dtype):
    """the sum dbhip_expr_eval's want_sum reports for an integer result: the valid rows' values, wrapping at 64 bits"""
    m = np.ones(len(values), bool) if valid is None else valid
    s = sum(int(v) for v in np.asarray(values)[m].tolist())
    return wrap_py(s, 64, INFO[dtype][1] == "s")
