"""Directed cases for Decimal64 / Decimal128 arithmetic (results of at most 38 digits: T = i64 or i128), shared by the CPU test
(tests/test_dec_edges_cpu.py: oracle and host twin of dev_decimal.h against Python) and the GPU test (tests/test_gpu_decimal_edges.py).
Pure Python, deterministic, no GPU and no oracle.

cases() -> dicts op, x = (kind, type, (p, s), values), y likewise, ret, expected (tests/dec256_ref.binary; None = the row raises)
and labels: per row, the set of branch / edge labels the row carries. The labels are computed here from the sizes and from the
magnitudes the reference's formulas imply (numerator N, divisor D, quotient, remainder), never by running the code under test:

  case label   (op, T, "maxp" | "lowp", "shift0" | "shift+")                         every reachable one has a size pair (reachable())
  conv:T:...   operand conversion: dec_pass, dec_rescale, int_wrap, int_rescale       (rescales happen in plus / minus only)
  path:...     which division dev_decimal.h takes: 2by1 (udiv128_by_64: two double-precision estimates), native128 (the
               compiler's 128 / 128), loop256 (u256_div_128's bit loop), i64native (the unchecked i64 rounding multiply)
  D:<name>     |divisor| is one of DIVISORS;  D<2^64 / D>=2^64;  N<2^128 / N>=2^128 (T = i128 with a 256-bit numerator)
  qhi:zero / qhi:nonzero / qlo:max   quotient digits of the 2by1 path;  rem:0 / rem:D-1
  tie:<exact|below|above>:<signs>, tie:<kind>:<odd|even>D    2 r == D, the largest r below, the smallest r above (r = |a| 10^k mod D)
  range:...    a checked form exactly at its bound (":+max" / ":-max" pass) and one past it (":+past" / ":-past" raise)
  wrap:...     an unchecked form past its wrap point (the expected value is the wrapped one, as the reference computes it): the
               shift-0 multiply, the unchecked rounding multiply in i64 and in i128 (products on either side of 2^127 and 2^128),
               the quotient of a divide, an operand wider than T
  raise:div0:<sign of the numerator>

Values stay inside the operand's declared precision, with one exception. The checks at precision 18 (plus / minus / rounding multiply
in i64, checked_mul_T at 2^63, a rescale into i64) cannot fire for operands inside their precision: an unclamped result precision
always holds the result. Size pairs marked `beyond` therefore also take values up to the storage range (a Decimal64 column is an
i64 column; nothing in the reference or here validates it against its precision) — rows labelled "beyond".
"""
import math

import numpy as np

from tests import dec256_cases as K
from tests import dec256_ref as R

OPNAME = {R.OP_PLUS: "plus", R.OP_MINUS: "minus", R.OP_MULTIPLY: "mul", R.OP_DIVIDE: "div"}
DIVISORS = {"1": 1, "2": 2, "3": 3}
for _e in (32, 53, 63, 64):
    DIVISORS.update({f"2^{_e}-1": 2 ** _e - 1, f"2^{_e}": 2 ** _e, f"2^{_e}+1": 2 ** _e + 1})
for _j in (9, 18, 19, 20):
    DIVISORS.update({f"10^{_j}-1": 10 ** _j - 1, f"10^{_j}": 10 ** _j, f"10^{_j}+1": 10 ** _j + 1})
DIV_NAME = {v: k for k, v in DIVISORS.items()}
TIE_DIVISORS = [3, 4, 7, 10, 2 ** 32 - 1, 2 ** 32, 2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 1, 10 ** 18, 10 ** 19 + 1]
M64 = 2 ** 64 - 1
SIGNS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]


def D(p, s, bits=None, beyond=False):
    return ("dec", bits or R.storage_bits(p), (p, s), beyond)


def I(name):
    return (name, name, (R.INT_PROPS[name][0], 0), False)


# (op, x, y): at least one size pair per reachable (op, T, maxp, shift) label, and every operand conversion in each T
TABLE = [
    # ---- T = i64
    (R.OP_PLUS, D(10, 2), D(12, 2)),                       # lowp, both pass through
    (R.OP_PLUS, D(17, 2, beyond=True), D(17, 2, beyond=True)),   # precision 18: the checked form
    (R.OP_MINUS, D(17, 2, beyond=True), D(17, 2, beyond=True)),
    (R.OP_PLUS, D(10, 0, beyond=True), D(17, 6, beyond=True)),   # decimal rescale into i64, precision 18
    (R.OP_MINUS, D(9, 4), D(9, 1)),                        # lowp, decimal rescale
    (R.OP_PLUS, I("i32"), D(16, 6, beyond=True)),          # integer rescale, checked, i64
    (R.OP_MINUS, D(12, 0), I("u16")),                      # integer at scale 0
    (R.OP_MULTIPLY, D(9, 6), D(9, 6)),                     # shift 0, precision 18: nothing rounds, nothing is checked
    (R.OP_MULTIPLY, D(6, 2), D(6, 3)),                     # shift 0, lowp
    (R.OP_MULTIPLY, D(6, 2), I("i8")),
    (R.OP_MULTIPLY, D(12, 8, beyond=True), D(10, 8, beyond=True)),   # (18,12) shift 4: rounding multiply, range check
    (R.OP_MULTIPLY, D(9, 9), D(9, 9)),                     # (12,12) shift 6: rounding multiply in wrapping i64
    (R.OP_MULTIPLY, D(12, 12), D(12, 12)),                 # (12,12) shift 12: the i64 product wraps
    (R.OP_MULTIPLY, D(18, 18, beyond=True), D(18, 18, beyond=True)),   # (18,18) shift 18: checked, divisor 10^18
    (R.OP_DIVIDE, D(16, 12), D(3, 0)),                     # shift 0
    (R.OP_DIVIDE, D(18, 12), D(6, 0)),                     # (18,12) shift 0 at precision 18
    (R.OP_DIVIDE, D(12, 6), D(6, 0)),                      # (18,12) shift 6
    (R.OP_DIVIDE, D(8, 2), D(5, 4)),                       # (18,8) shift 10
    (R.OP_DIVIDE, D(10, 2), I("i64")),                     # (16,8) shift 6, divisors up to 2^63, INT64_MIN
    (R.OP_DIVIDE, D(10, 2), I("u64")),                     # (16,8): `as i64` turns 2^64 - 1 into -1
    (R.OP_DIVIDE, D(12, 12), I("u64")),                    # (12,12) shift 0
    (R.OP_DIVIDE, D(5, 2), D(38, 0)),                      # (11,8): a Decimal128 divisor under T = i64 keeps its low 64 bits
    (R.OP_DIVIDE, I("i32"), D(8, 2)),                      # integer numerator
    # ---- T = i128
    (R.OP_PLUS, D(20, 4), D(18, 4)),                       # lowp
    (R.OP_MINUS, D(19, 0), D(10, 3)),                      # lowp, decimal rescale
    (R.OP_PLUS, D(38, 0), D(38, 0)),                       # precision 38, checked
    (R.OP_MINUS, D(38, 5), D(38, 5)),
    (R.OP_PLUS, D(38, 0), D(38, 10)),                      # decimal rescale landing on / past precision 38
    (R.OP_MINUS, D(18, 0), D(38, 36)),                     # rescale by 10^36: 170 10^36 fits i128, 171 10^36 does not
    (R.OP_PLUS, I("i64"), D(38, 30)),                      # integer rescale, checked
    (R.OP_MINUS, D(38, 20), I("u64")),                     # u64 * 10^20 straddles 2^127
    (R.OP_PLUS, D(25, 0), I("u64")),                       # integer at scale 0
    (R.OP_MULTIPLY, D(15, 2), D(15, 2)),                   # shift 0, lowp
    (R.OP_MULTIPLY, D(38, 0), D(38, 0)),                   # shift 0 at precision 38: wraps at 2^127, unchecked
    (R.OP_MULTIPLY, D(20, 0), I("i64")),                   # (38,0) shift 0
    (R.OP_MULTIPLY, D(15, 8), D(15, 8)),                   # (26,12) shift 4, unchecked
    (R.OP_MULTIPLY, D(25, 12), D(24, 12)),                 # (37,12) shift 12, unchecked: the u128 product wraps past 2^127 and 2^128
    (R.OP_MULTIPLY, D(38, 10), D(18, 10)),                 # (38,12) shift 8: 256-bit product
    (R.OP_MULTIPLY, D(38, 20), D(38, 20)),                 # (38,20) shift 20: divisor 10^20 >= 2^64
    (R.OP_DIVIDE, D(38, 12), D(20, 0)),                    # (38,12) shift 0: free numerators, divisors past 2^64
    (R.OP_DIVIDE, D(30, 12), D(8, 0)),                     # (30,12) shift 0, lowp
    (R.OP_DIVIDE, D(15, 2), D(15, 2)),                     # (23,8) shift 8
    (R.OP_DIVIDE, D(38, 0), D(38, 10)),                    # (38,6) shift 16: quotients past 2^128 keep their low 128 bits
    (R.OP_DIVIDE, D(30, 4), D(15, 8)),                     # (38,10) shift 14
    (R.OP_DIVIDE, D(20, 2), I("u64")),                     # (26,8) shift 6
    (R.OP_DIVIDE, I("i64"), D(20, 10)),                    # (35,6) shift 16
]


def case_label(op, xs, ys):
    left, right, ret = R.result_size(op, xs, ys)
    bits = R.storage_bits(ret[0])
    shift = xs[1] + ys[1] - ret[1] if op == R.OP_MULTIPLY else (ys[1] + ret[1] - xs[1] if op == R.OP_DIVIDE else 0)
    return (OPNAME[op], bits, "maxp" if ret[0] == R.MAXP[bits] else "lowp", "shift+" if shift else "shift0")


_REACHABLE = None


def reachable():
    """every (op, T, maxp, shift) label some pair of operand sizes of at most 38 digits reaches (integer operands have the sizes
    (3|5|10|19|20, 0), which the enumeration contains); shifts beyond 38 are refused by the product and left out"""
    global _REACHABLE
    if _REACHABLE is None:
        sizes = [(p, s) for p in range(1, 39) for s in range(p + 1)]
        out = set()
        for op in (R.OP_PLUS, R.OP_MINUS, R.OP_MULTIPLY, R.OP_DIVIDE):
            for a in sizes:
                for b in sizes:
                    rs = R.result_size(op, a, b)
                    if rs is None or rs[2][0] > 38:
                        continue
                    lab = case_label(op, a, b)
                    out.add(lab)
        _REACHABLE = out
    return _REACHABLE


def all_case_labels():
    return {(o, t, m, s) for o in OPNAME.values() for t in (64, 128) for m in ("maxp", "lowp") for s in ("shift0", "shift+")}


# --------------------------------------------------------------------------------------------------------------- labels
def _div_labels(L, N, B, bits, wide):
    """the division N / B (magnitudes) as dev_decimal.h dispatches it"""
    if B in DIV_NAME:
        L.add("D:" + DIV_NAME[B])
    L.add("D<2^64" if B < 2 ** 64 else "D>=2^64")
    if wide:
        L.add("N<2^128" if N < 2 ** 128 else "N>=2^128")
    if wide and N >= 2 ** 128:
        path = "loop256"
    else:
        path = "2by1" if B < 2 ** 64 else "native128"
    L.add("path:" + path)
    Q, rem = divmod(N, B)
    if rem == 0:
        L.add("rem:0")
    if B >= 2 and rem == B - 1:
        L.add("rem:D-1")
    if path == "2by1":
        L.add("qhi:zero" if Q < 2 ** 64 else "qhi:nonzero")
        if Q & M64 == M64:
            L.add("qlo:max")
    return Q


def _tie_labels(L, mag, B, a, b):
    if B < 3:
        return
    r = mag % B
    kind = "exact" if 2 * r == B else ("below" if r == (B + 1) // 2 - 1 else ("above" if r == B // 2 + 1 else None))
    if kind:
        L.add(f"tie:{kind}:{'-' if a < 0 else '+'}{'-' if b < 0 else '+'}")
        L.add(f"tie:{kind}:{'odd' if B & 1 else 'even'}D")


def _edge(L, name, v, bound):
    if abs(v) == bound:
        L.add(f"range:{name}:{'-' if v < 0 else '+'}max")
    elif abs(v) == bound + 1:
        L.add(f"range:{name}:{'-' if v < 0 else '+'}past")


def row_labels(op, xk, xs, yk, ys, x, y):
    left, right, ret = R.result_size(op, xs, ys)
    bits = R.storage_bits(ret[0])
    overflow = ret[0] == R.MAXP[bits]
    L = set()
    conv = []
    for kind, size, to, v in ((xk, xs, left, x), (yk, ys, right, y)):
        d = to[1] - size[1]
        if kind == "dec":
            L.add(f"conv:{bits}:{'dec_rescale' if d else 'dec_pass'}")
            if abs(v) > 10 ** size[0] - 1:
                L.add("beyond")
            if not R.fits(v, bits):
                L.add(f"wrap:conv{bits}:dec")
        else:
            L.add(f"conv:{bits}:{'int_rescale' if to[1] else 'int_wrap'}")
            if to[1] == 0 and not R.fits(v, bits):
                L.add(f"wrap:conv{bits}:int")
            if v == -2 ** 63:
                L.add("int:INT64_MIN")
        if (d if kind == "dec" else to[1]):
            dd = d if kind == "dec" else to[1]
            k = "dec" if kind == "dec" else "int"
            _edge(L, f"rescale{bits}:{k}", v, 10 ** (to[0] - dd) - 1)       # |v| 10^dd lands on 10^tp - 10^dd (passes) / 10^tp (raises)
            _edge(L, f"cmul{bits}", v, (2 ** (bits - 1) - 1) // 10 ** dd)    # the largest |v| whose rescale fits T / the first that does not
        try:
            conv.append(R.convert_operand(v, kind, size[1], to, bits))
        except R.RowError:
            conv.append(None)
    a, b = conv
    if a is None or b is None:
        L.add("raise:conv")
        return L
    sg = (a < 0) == (b < 0)
    if op in (R.OP_PLUS, R.OP_MINUS):
        t = a + b if op == R.OP_PLUS else a - b
        if overflow:
            _edge(L, f"{OPNAME[op]}{ret[0]}", t, 10 ** ret[0] - 1)
        if not R.fits(t, bits):
            L.add(f"wrap:{OPNAME[op]}{bits}")
        return L
    if op == R.OP_MULTIPLY:
        k = xs[1] + ys[1] - ret[1]
        P = a * b
        if k == 0:
            if not R.fits(P, bits):
                L.add(f"wrap:mul{bits}:shift0")
            return L
        B = 10 ** k
        h = B // 2
        if not overflow:
            num = R.wrap(R.wrap(P, bits) + h if sg else R.wrap(P, bits) - h, bits)
            if num != (P + h if sg else P - h):
                L.add(f"wrap:mul{bits}:unchecked")
            else:
                _tie_labels(L, abs(P), B, a, b)
            if bits == 64:
                L.add("path:i64native")
                if B in DIV_NAME:
                    L.add("D:" + DIV_NAME[B])
            else:
                _div_labels(L, abs(num), B, bits, False)
            return L
        _tie_labels(L, abs(P), B, a, b)
        N = abs(P) + h
        Q = _div_labels(L, N, B, bits, bits == 128)
        q = Q if sg else -Q
        if bits == 64:
            _edge(L, "mul18", q, 10 ** 18 - 1)
        else:
            _edge(L, "mul38q", q, 2 ** 127 - 1)      # +max = 2^127 - 1, +past = 2^127 raises, -past = -2^127 is legal
            if abs(q) == 2 ** 127 + 1:
                L.add(f"range:mul38q:{'-' if q < 0 else '+'}past2")
        return L
    if b == 0:
        L.add(f"raise:div0:{'-' if a < 0 else '+'}")
        return L
    k = ys[1] + ret[1] - xs[1]
    B = abs(b)
    if bits == 64:
        am = R.wrap(a * 10 ** k, 128)
        if am != a * 10 ** k:
            L.add("wrap:div64:numerator")
            N = abs(R.wrap(am + R.tdiv(b, 2) if sg else am - R.tdiv(b, 2), 128))
        else:
            N = abs(a) * 10 ** k + B // 2
            _tie_labels(L, abs(a) * 10 ** k, B, a, b)
        Q = _div_labels(L, N, B, bits, False)
        if Q >= 2 ** 63:
            L.add("wrap:div64:as_i64")
    else:
        N = abs(a) * 10 ** k + B // 2
        _tie_labels(L, abs(a) * 10 ** k, B, a, b)
        Q = _div_labels(L, N, B, bits, True)
        if Q >= 2 ** 127:
            L.add("wrap:div128:low128")
    return L


# ------------------------------------------------------------------------------------------------------ directed values
def _range(side):
    kind, typ, size, beyond = side
    if kind == "dec":
        if beyond:
            return -(2 ** (typ - 1)), 2 ** (typ - 1) - 1
        return -(10 ** size[0] - 1), 10 ** size[0] - 1
    info = np.iinfo(K.INTS[kind][1])
    return int(info.min), int(info.max)


def _solve(c, r, m):
    """the smallest a >= 0 with c a == r (mod m), or None"""
    g = math.gcd(c, m)
    if r % g:
        return None
    mg = m // g
    if mg == 1:
        return 0
    return (r // g) * pow(c // g, -1, mg) % mg


def _steer(lo, hi, xmax, ymax, spread=1, tries=3000):
    """(x, y) with lo <= x y <= hi, 0 <= x <= xmax, 1 <= y <= ymax, or None; `spread` > 1 starts the search at a larger y"""
    if hi < 0 or xmax < 1:
        return None
    if lo <= 0:
        return 0, spread
    y0 = max(1, -(-lo // xmax)) * spread
    for y in range(y0, min(ymax, y0 + tries) + 1):
        x = hi // y
        if x <= xmax and x * y >= lo:
            return x, y
    return None


class _Rows:
    def __init__(self, xside, yside):
        (self.xlo, self.xhi), (self.ylo, self.yhi) = _range(xside), _range(yside)
        self.rows, self.seen, self.turn = [], set(), 0

    def add(self, x, y):
        if self.xlo <= x <= self.xhi and self.ylo <= y <= self.yhi and (x, y) not in self.seen:
            self.seen.add((x, y))
            self.rows.append((x, y))
            return True
        return False

    def add_signed(self, ax, ay):
        """magnitudes with the next sign combination that is legal (unsigned operands have one sign)"""
        for t in range(4):
            sx, sy = SIGNS[(self.turn + t) % 4]
            if self.add(sx * ax, sy * ay):
                self.turn += t + 1
                return


def _tie_targets(B):
    out = [("below", (B + 1) // 2 - 1), ("above", B // 2 + 1)]
    if B % 2 == 0:
        out.append(("exact", B // 2))
    return out


def _directed_divide(rows, k, bits):
    amax = max(abs(rows.xlo), abs(rows.xhi))
    for sx in (1, -1, rows.xhi, rows.xlo, 0, 2, -2, 3, -3):
        rows.add(sx, 0)                                   # zero divisors under numerators of both signs
    for j, Dv in enumerate(DIVISORS.values()):
        y = Dv if j % 2 == 0 else -Dv
        if not rows.ylo <= y <= rows.yhi:
            y = -y
        if not rows.ylo <= y <= rows.yhi:
            continue
        B = abs(R.wrap(y, bits))
        if B == 0:                                        # a divisor whose low bits are zero under a narrower T
            rows.add(1, y), rows.add(-1, y)
            continue
        h = B // 2
        qs = [0, 1, 2 ** 53 - 1, 2 ** 53 + 1, 2 ** 64, 2 ** 64 + 1, M64, ((B - 1) << 64) | M64]
        ns = []
        for Q in qs:
            ns += [Q * B + r for r in (0, 1, B - 1)]
        if bits == 128:
            qb = (2 ** 128 - 1) // B
            ns += [qb * B + B - 1, (qb + 1) * B, 2 ** 128 - 1, 2 ** 128]
        for N in ns:
            if N < h:
                continue
            A = N - h
            if k:   # numerators have the form A 10^k + D / 2: the A nearest the target whose remainder is exactly the target's,
                A //= 10 ** k                             # where D admits one (the quotient digits are then near, not at, Q)
                a0 = _solve(10 ** k, (N - h) % B, B)
                if a0 is not None:
                    step = B // math.gcd(10 ** k, B)
                    A = max(a0, a0 + (A - a0 + step // 2) // step * step)
                else:
                    A += rows.turn & 1
            if A <= amax:
                sa = SIGNS[rows.turn % 4][0]
                rows.turn += 1
                rows.add(sa * A, y) or rows.add(-sa * A, y)
    for Dv in TIE_DIVISORS:                               # ties: |a| 10^k == r (mod D) for r at, just below and just above D / 2
        B = abs(R.wrap(Dv, bits))
        if B < 3:
            continue
        for kind, r in _tie_targets(B):
            a0 = _solve(10 ** k, r, B)
            if a0 is None:
                continue
            step = B // math.gcd(10 ** k, B)
            for m in sorted({0, max(0, (amax - a0) // step)}):
                if a0 + m * step:
                    rows.add_signed(a0 + m * step, Dv)


EDGE_Q = (10 ** 18 - 1, 10 ** 18, 2 ** 127 - 1, 2 ** 127, 2 ** 127 + 1)


def _directed_multiply(rows, k, bits):
    xmax, ymax = max(abs(rows.xlo), abs(rows.xhi)), max(abs(rows.ylo), abs(rows.yhi))
    if k == 0:
        lim = 2 ** (bits - 1)
        for P in (lim - 1, lim, lim + 1, 2 * lim - 1, 2 * lim, 2 * lim + 1, 10 ** R.MAXP[bits] - 1, 10 ** R.MAXP[bits]):
            got = _steer(P, P, xmax, ymax) or _steer(P, P + (P >> 70), xmax, ymax)
            if got:
                for _ in range(2):
                    rows.add_signed(*got)
        return
    B = 10 ** k
    h = B // 2
    # ties, steered by a second operand of 1 or a small / large factor coprime to ten
    big = ymax - (ymax % 10) + 7 if ymax > 100 else 9
    while big > ymax or math.gcd(big, 10) != 1:
        big -= 2
    for f in (1, 3, 7, big):
        if f > ymax:
            continue
        for kind, r in _tie_targets(B):
            x0 = _solve(f, r, B)
            for m in sorted({0, 1, max(0, (xmax - x0) // B)}):
                rows.add_signed(x0 + m * B, f)
                if f <= xmax and x0 + m * B <= ymax:
                    rows.add_signed(f, x0 + m * B)
    # the product itself on either side of 2^(bits-1) and 2^bits, where the unchecked forms wrap (the +- D / 2 wraps with it)
    for Pt in (2 ** (bits - 1), 2 ** bits):
        for lo, hi in ((Pt - h - B, Pt - h - 1), (Pt - h, Pt - 1), (Pt, Pt + h - 1), (Pt + h, Pt + h + B)):
            for spread in (1, 3):
                got = _steer(lo, hi, xmax, ymax, spread)
                if got:
                    for sg in SIGNS:
                        rows.add(sg[0] * got[0], sg[1] * got[1])
    # quotient targets: the product lands in the window that rounds to Qt: its two ends, then anywhere inside
    qts = [0, 1, 2 ** 53 - 1, 2 ** 53 + 1, M64, 2 ** 64, 2 ** 64 + 1, ((B - 1) << 64) | M64, 10 ** 18 - 1, 10 ** 18,
           2 ** 127 - 1, 2 ** 127, 2 ** 127 + 1, (2 ** 128 - 1) // B, 2 ** 128 // B + 1, 10 ** 38 - 1, 10 ** 38]
    for Qt in qts:
        for lo, hi in ((Qt * B - h, Qt * B - h), (Qt * B + h - 1, Qt * B + h - 1), (Qt * B - h, Qt * B + h - 1)):
            got = _steer(lo, hi, xmax, ymax)
            if got:
                rows.add_signed(*got)
        if Qt in EDGE_Q:                                  # the checked bounds: three factorisations in every sign combination
            for spread in (1, 3, 11):
                got = _steer(Qt * B - h, Qt * B + h - 1, xmax, ymax, spread)
                if got:
                    for s in SIGNS:
                        rows.add(s[0] * got[0], s[1] * got[1])


def _directed_plus_minus(rows, op, xside, yside, left, bits):
    p, s = left
    dx, dy = s - xside[2][1], s - yside[2][1]
    if xside[0] != "dec":
        dx = s
    if yside[0] != "dec":
        dy = s
    sgn = 1 if op == R.OP_PLUS else -1
    bound = 10 ** p - 1
    smalls = (0, 1, -1, 7, -7, 10, -10, 123, -123)
    # results at +-(10^p - 1), +-10^p, +-(10^p + 1) and around the wrap point of T: t = x 10^dx + sgn y 10^dy
    targets = [s_ * (bound + e) for s_ in (1, -1) for e in (-1, 0, 1, 2)] + [s_ * (2 ** (bits - 1) + e) for s_ in (1, -1) for e in (-2, -1, 0, 1)]
    for t in targets:
        for u in smalls:
            # the rescaled side takes the small value, the other side the rest
            for small_is_x in (True, False):
                if small_is_x:
                    rest = t - u * 10 ** dx                 # = sgn y 10^dy
                    if rest % 10 ** dy == 0:
                        rows.add(u, sgn * rest // 10 ** dy)
                else:
                    rest = t - sgn * u * 10 ** dy           # = x 10^dx
                    if rest % 10 ** dx == 0:
                        rows.add(rest // 10 ** dx, u)
    # each rescale at the bound precision and at the range of T
    for d, is_x in ((dx, True), (dy, False)):
        if d == 0:
            continue
        for base in (10 ** (p - d) - 1, (2 ** (bits - 1) - 1) // 10 ** d):
            for v in (base - 1, base, base + 1, base + 2):
                for sv in (1, -1):
                    for u in (0, 1, -1, 3, -3, 5, -5, 9):
                        rows.add(sv * v, u) if is_x else rows.add(u, sv * v)


def _values(rng, side, n):
    kind, typ, size, _ = side
    if kind == "dec":
        vals = K.rand_values(rng, size[0], n)
        return vals[:n // 2] + [v % 10 ** min(size[0], 7) * (1 if v >= 0 else -1) for v in vals[n // 2:]]
    vals = K.rand_int_values(rng, kind, n)
    return vals[:n // 2] + [R.wrap(v, 8) if np.iinfo(K.INTS[kind][1]).min < 0 else v % 100 for v in vals[n // 2:]]


def build_case(index, op, xside, yside, filler=48):
    (xk, xt, xs, _), (yk, yt, ys, _) = xside, yside
    left, right, ret = R.result_size(op, xs, ys)
    bits = R.storage_bits(ret[0])
    rows = _Rows(xside, yside)
    for x in (rows.xlo, rows.xhi, 0, 1, -1):
        for y in (rows.ylo, rows.yhi, 1):
            rows.add(x, y)
    if op in (R.OP_PLUS, R.OP_MINUS):
        _directed_plus_minus(rows, op, xside, yside, left, bits)
    elif op == R.OP_MULTIPLY:
        _directed_multiply(rows, xs[1] + ys[1] - ret[1], bits)
    else:
        _directed_divide(rows, ys[1] + ret[1] - xs[1], bits)
    rng = np.random.default_rng(1000 + index)
    filler = max(filler, MIN_LEN - len(rows.rows))          # (every case is long enough for the 257-row prefix the GPU test takes)
    for x, y in zip(_values(rng, xside, filler), _values(rng, yside, filler)):
        rows.rows.append((x, y))
    xv, yv = [r[0] for r in rows.rows], [r[1] for r in rows.rows]
    exp, labels = [], []
    for x, y in rows.rows:
        try:
            exp.append(R.binary(op, x, xk, xs, y, yk, ys)[0])
        except R.RowError:
            exp.append(None)
        labels.append(row_labels(op, xk, xs, yk, ys, x, y))
    return dict(op=op, x=(xk, xt, xs, xv), y=(yk, yt, ys, yv), ret=ret, expected=exp, labels=labels, label=case_label(op, xs, ys), directed=len(rows.rows) - filler)


MIN_LEN = 260
_CASES = None


def cases():
    """the whole table, built once and shared (read-only) by the tests that need it"""
    global _CASES
    if _CASES is None:
        _CASES = [build_case(i, op, x, y) for i, (op, x, y) in enumerate(TABLE)]
    return _CASES


def census(cs=None):
    out = {}
    for c in cs or cases():
        for L in c["labels"]:
            for lab in L:
                out[lab] = out.get(lab, 0) + 1
    return out


def required_edge_labels():
    """the edge labels the census has to find on at least MIN_ROWS rows over the whole table. Left out because no operand inside
    its types can carry them: an integer rescale into i64 at its bounds (range:rescale64:int, cmul64 from an integer) — an
    integer type whose decimal precision leaves room for a scale under 18 digits is at most 32 bits wide, so value * 10^scale
    stays below both 10^precision and 2^63."""
    out = {f"tie:{k}:{s}" for k in ("exact", "below", "above") for s in ("++", "+-", "-+", "--")}
    out |= {"tie:exact:evenD", "tie:below:evenD", "tie:below:oddD", "tie:above:evenD", "tie:above:oddD"}
    out |= {"D:" + n for n in DIVISORS}
    out |= {"D<2^64", "D>=2^64", "N<2^128", "N>=2^128", "qhi:zero", "qhi:nonzero", "qlo:max", "rem:0", "rem:D-1"}
    out |= {"path:2by1", "path:native128", "path:loop256", "path:i64native"}
    for name in ("plus18", "minus18", "plus38", "minus38", "mul18", "mul38q", "rescale64:dec", "rescale128:dec", "rescale128:int", "cmul64", "cmul128"):
        out |= {f"range:{name}:{e}" for e in ("+max", "-max", "+past", "-past")}
    out |= {"range:mul38q:+past2", "range:mul38q:-past2"}
    out |= {f"conv:{t}:{c}" for t in (64, 128) for c in ("dec_pass", "dec_rescale", "int_wrap", "int_rescale")}
    out |= {"raise:div0:+", "raise:div0:-", "raise:conv", "wrap:conv64:int", "wrap:conv64:dec", "int:INT64_MIN", "wrap:mul64:unchecked", "wrap:mul128:unchecked",
            "wrap:mul128:shift0", "wrap:div128:low128"}
    return out


MIN_ROWS = 8


if __name__ == "__main__":   # python -m tests.dec_edge_cases: the size table and the census
    for c in cases():
        print(c["label"], c["x"][:3], c["y"][:3], "->", c["ret"], len(c["expected"]), "rows,", sum(e is None for e in c["expected"]), "raise")
    for lab, rows in sorted(census().items()):
        print(f"{rows:6d}  {lab}")
    print("unreachable:", sorted(all_case_labels() - reachable()))
