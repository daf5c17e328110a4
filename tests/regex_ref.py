"""A plain-Python restatement of the regular-expression predicates of include/dbhip.h a25: its own recursive-descent parser and a
set-of-threads simulation of the pattern's NFA (a Pike machine: no DFA, no byte classes, no `re`). tests/test_regex_ref_cpu.py holds it
to Python's `re` where the two are defined alike and shows where they differ on purpose; the host checker and the GPU tests are then
held to this file.

supported(pattern, flags) -> bool: the grammar, the pattern length and the cap on NFA positions (the DFA's own caps are the library's).
match(pattern, flags, value) -> True / False / DECLINED."""
import functools

CASE_INSENSITIVE, DOT_NL, UNIT_BYTE, FULL_MATCH = 1, 2, 4, 8
DECLINED = "declined"
MAX_PATTERN, MAX_POSITIONS, MAX_REPEAT, MAX_DEPTH = 1024, 4096, 1000, 64

PUNCT = frozenset(range(0x21, 0x30)) | frozenset(range(0x3A, 0x41)) | frozenset(range(0x5B, 0x61)) | frozenset(range(0x7B, 0x7F))
PERL = {"d": frozenset(range(0x30, 0x3A)),
        "w": frozenset(range(0x30, 0x3A)) | frozenset(range(0x41, 0x5B)) | frozenset(range(0x61, 0x7B)) | {0x5F},
        "s": frozenset({0x20, 9, 10, 11, 12, 13})}
SIMPLE = {ord("t"): 9, ord("n"): 10, ord("v"): 11, ord("f"): 12, ord("r"): 13}
LEAD, CONT = frozenset(range(0xC0, 0x100)), frozenset(range(0x80, 0xC0))


class Unsupported(Exception):
    pass


def _utf8_len(p, i):
    """the length of the well-formed UTF-8 sequence at p[i], or 0"""
    try:
        c = p[i]
        n = 2 if 0xC2 <= c <= 0xDF else 3 if 0xE0 <= c <= 0xEF else 4 if 0xF0 <= c <= 0xF4 else 0
        if n and len(p) >= i + n:
            p[i:i + n].decode("utf-8")
            return n
    except UnicodeDecodeError:
        pass
    return 0


class _Parser:
    def __init__(self, pattern, flags):
        self.p, self.i, self.flags, self.depth, self.needs_ascii = pattern, 0, flags, 0, bool(flags & CASE_INSENSITIVE)

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else -1

    def fold(self, s):
        if not self.flags & CASE_INSENSITIVE:
            return frozenset(s)
        out = set(s)
        for b in s:
            if 0x41 <= b <= 0x5A or 0x61 <= b <= 0x7A:
                out.add(b ^ 0x20)
        return frozenset(out)

    def unit_except(self, excluded):
        if self.flags & UNIT_BYTE:
            return ("set", frozenset(range(256)) - excluded)
        return ("alt", [("set", frozenset(range(128)) - excluded), ("cat", [("set", LEAD), ("rep", ("set", CONT), 0, None)])])

    def escape(self):
        """behind a backslash: ('byte', b) or ('perl', letter)"""
        c = self.peek()
        if c < 0:
            raise Unsupported("trailing backslash")
        self.i += 1
        if c in SIMPLE:
            return "byte", SIMPLE[c]
        if chr(c) in "dwsDWS":
            self.needs_ascii = True
            return "perl", chr(c)
        if c == ord("x"):
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(chr(x) not in "0123456789abcdefABCDEF" for x in h):
                raise Unsupported("\\x")
            self.i += 2
            v = int(h.decode(), 16)
            if v > 0x7F and not self.flags & UNIT_BYTE:
                raise Unsupported("\\x above 7F")
            return "byte", v
        if c in PUNCT:
            return "byte", c
        raise Unsupported("escape")

    def klass(self):
        negate = self.peek() == ord("^")
        if negate:
            self.i += 1
        items, first = set(), self.i
        pending = None                           # a single byte that may open a range
        while True:
            c = self.peek()
            if c < 0:
                raise Unsupported("unterminated class")
            if c == ord("]"):
                if self.i == first:
                    raise Unsupported("empty class")
                self.i += 1
                break
            if c >= 0x80 or c in (ord("["), ord("^")):
                raise Unsupported("class byte")
            if c in (ord("&"), ord("~"), ord("-")) and self.p[self.i + 1:self.i + 2] == bytes([c]):
                raise Unsupported("set operation")
            self.i += 1
            if c == ord("-"):
                if self.i - 1 == first or self.peek() == ord("]"):
                    items.add(c)
                    pending = None
                    continue
                if pending is None:
                    raise Unsupported("dash")
                h = self.peek()
                if h < 0:
                    raise Unsupported("unterminated class")
                self.i += 1
                if h == ord("\\"):
                    kind, h = self.escape()
                    if kind != "byte":
                        raise Unsupported("range end")
                elif h >= 0x80 or h in (ord("["), ord("]"), ord("^")):
                    raise Unsupported("range end")
                if h < pending:
                    raise Unsupported("descending range")
                items.update(range(pending, h + 1))
                pending = None
                continue
            if c == ord("\\"):
                kind, v = self.escape()
                if kind == "perl":
                    if v in "DWS":
                        raise Unsupported("negated perl class inside a class")
                    items |= PERL[v]
                    if self.peek() == ord("-") and self.p[self.i + 1:self.i + 2] != b"]":
                        raise Unsupported("range start")
                    pending = None
                    continue
                c = v
            items.add(c)
            pending = c
        items = self.fold(items)
        return self.unit_except(items) if negate else ("set", items)

    def literal(self, b):
        return ("set", self.fold({b}))

    def atom(self):
        c = self.peek()
        self.i += 1
        ch = chr(c)
        if ch in "*+?{":
            raise Unsupported("quantifier without an operand, or a stray {")
        if ch == "^":
            return ("bol",), False
        if ch == "$":
            return ("eol",), False
        if ch == ".":
            return self.unit_except(frozenset() if self.flags & DOT_NL else frozenset({10})), True
        if ch == "[":
            return self.klass(), True
        if ch == "(":
            if self.peek() == ord("?"):
                self.i += 1
                if self.peek() == ord(":"):
                    self.i += 1
                elif self.p[self.i:self.i + 2] == b"P<":
                    j = self.p.find(b">", self.i)
                    name = self.p[self.i + 2:j] if j >= 0 else b""
                    if not name or not all(chr(x).isascii() and (chr(x).isalnum() or x == 0x5F) for x in name) or chr(name[0]).isdigit():
                        raise Unsupported("group name")
                    self.i = j + 1
                else:
                    raise Unsupported("(? form")
            self.depth += 1
            if self.depth > MAX_DEPTH:
                raise Unsupported("nesting")
            node = self.alternation()
            self.depth -= 1
            if self.peek() != ord(")"):
                raise Unsupported("unterminated group")
            self.i += 1
            return node, True
        if ch == "\\":
            kind, v = self.escape()
            if kind == "byte":
                return self.literal(v), True
            return (("set", PERL[v]) if v.islower() else self.unit_except(PERL[v.lower()])), True
        if c < 0x80 or self.flags & UNIT_BYTE:
            return self.literal(c), True
        n = _utf8_len(self.p, self.i - 1)
        if not n:
            raise Unsupported("not UTF-8")
        seq = [self.literal(b) for b in self.p[self.i - 1:self.i - 1 + n]]
        self.i += n - 1
        return ("cat", seq), True

    def number(self):
        j = self.i
        while self.i < len(self.p) and 0x30 <= self.p[self.i] <= 0x39:
            self.i += 1
        if self.i == j:
            raise Unsupported("counted repetition")
        return int(self.p[j:self.i])

    def piece(self):
        node, quantifiable = self.atom()
        c = self.peek()
        if c < 0 or chr(c) not in "*+?{":
            return node
        if not quantifiable:
            raise Unsupported("quantifier on an anchor")
        self.i += 1
        if c == ord("*"):
            lo, hi = 0, None
        elif c == ord("+"):
            lo, hi = 1, None
        elif c == ord("?"):
            lo, hi = 0, 1
        else:
            lo = hi = self.number()
            if self.peek() == ord(","):
                self.i += 1
                hi = None if self.peek() == ord("}") else self.number()
            if self.peek() != ord("}"):
                raise Unsupported("counted repetition")
            self.i += 1
            if lo > MAX_REPEAT or (hi is not None and (hi > MAX_REPEAT or hi < lo)):
                raise Unsupported("repetition bounds")
        if self.peek() == ord("?"):
            self.i += 1
        c = self.peek()
        if c >= 0 and chr(c) in "*+?{":
            raise Unsupported("quantifier on a quantifier")
        return ("rep", node, lo, hi)

    def alternation(self):
        branches = []
        while True:
            seq = []
            while self.peek() >= 0 and self.peek() not in (ord("|"), ord(")")):
                seq.append(self.piece())
            branches.append(("cat", seq))
            if self.peek() == ord("|"):
                self.i += 1
                continue
            return ("alt", branches)


def positions(node):
    """the byte-consuming NFA states the node expands to: x{m,} counts max(m, 1) copies of x, x{m,n} counts n"""
    kind = node[0]
    if kind == "set":
        return 1
    if kind in ("cat", "alt"):
        return sum(positions(k) for k in node[1])
    if kind == "rep":
        return positions(node[1]) * (max(node[2], 1) if node[3] is None else node[3])
    return 0


def parse(pattern, flags):
    """-> (tree, needs ASCII rows); raises Unsupported"""
    pattern = bytes(pattern)
    if len(pattern) > MAX_PATTERN:
        raise Unsupported("pattern length")
    if flags & CASE_INSENSITIVE and any(b >= 0x80 for b in pattern):
        raise Unsupported("non-ASCII with CASE_INSENSITIVE")
    ps = _Parser(pattern, flags)
    tree = ps.alternation()
    if ps.i < len(pattern):
        raise Unsupported("unbalanced )")
    if flags & FULL_MATCH:
        tree = ("cat", [("bol",), tree, ("eol",)])
    if positions(tree) > MAX_POSITIONS:
        raise Unsupported("positions")
    return tree, ps.needs_ascii


# ---- the machine ----------------------------------------------------------------------------------------------------------------------
# instructions: ("char", set) | ("split", a, b) | ("jmp", a) | ("bol",) | ("eol",) | ("match",)
def _emit(node, prog):
    kind = node[0]
    if kind == "set":
        prog.append(("char", node[1]))
    elif kind == "cat":
        for k in node[1]:
            _emit(k, prog)
    elif kind == "alt":
        jumps = []
        for k in node[1][:-1]:
            split = len(prog)
            prog.append(None)
            _emit(k, prog)
            jumps.append(len(prog))
            prog.append(None)
            prog[split] = ("split", split + 1, len(prog))
        _emit(node[1][-1], prog)
        for j in jumps:
            prog[j] = ("jmp", len(prog))
    elif kind == "rep":
        _, kid, lo, hi = node
        for _ in range(lo):
            _emit(kid, prog)
        if hi is None:
            split = len(prog)
            prog.append(None)
            _emit(kid, prog)
            prog.append(("jmp", split))
            prog[split] = ("split", split + 1, len(prog))
        else:
            splits = []
            for _ in range(hi - lo):
                splits.append(len(prog))
                prog.append(None)
                _emit(kid, prog)
            for s in splits:
                prog[s] = ("split", s + 1, len(prog))
    elif kind in ("bol", "eol"):
        prog.append((kind,))


class Program:
    def __init__(self, pattern, flags):
        tree, self.needs_ascii = parse(pattern, flags)
        self.prog = []
        _emit(tree, self.prog)
        self.prog.append(("match",))
        self._closures = {}

    def closure(self, pc, at_start, at_end):
        """the char instructions reachable from pc without consuming, and whether the match is"""
        key = (pc, at_start, at_end)
        got = self._closures.get(key)
        if got is None:
            chars, matched, seen, stack = [], False, set(), [pc]
            while stack:
                q = stack.pop()
                if q in seen:
                    continue
                seen.add(q)
                ins = self.prog[q]
                if ins[0] == "char":
                    chars.append(q)
                elif ins[0] == "match":
                    matched = True
                elif ins[0] == "split":
                    stack += [ins[2], ins[1]]
                elif ins[0] == "jmp":
                    stack.append(ins[1])
                elif (ins[0] == "bol" and at_start) or (ins[0] == "eol" and at_end):
                    stack.append(q + 1)
            got = self._closures[key] = (tuple(chars), matched)
        return got

    def search(self, value):
        n = len(value)
        threads = set()
        for pos in range(n + 1):
            chars, matched = self.closure(0, pos == 0, pos == n)      # the search may begin at every position
            if matched:
                return True
            threads.update(chars)
            if pos == n:
                return False
            b = value[pos]
            nxt = set()
            for q in threads:
                if b in self.prog[q][1]:
                    chars, matched = self.closure(q + 1, False, pos + 1 == n)
                    if matched:
                        return True
                    nxt.update(chars)
            threads = nxt
        return False


@functools.lru_cache(maxsize=512)
def compiled(pattern, flags):
    return Program(pattern, flags)


def supported(pattern, flags=0):
    try:
        compiled(bytes(pattern), flags)
        return True
    except Unsupported:
        return False


def needs_ascii(pattern, flags=0):
    return compiled(bytes(pattern), flags).needs_ascii


def match(pattern, flags, value):
    prog = compiled(bytes(pattern), flags)
    value = bytes(value)
    if prog.needs_ascii and any(b >= 0x80 for b in value):
        return DECLINED
    return prog.search(value)


def column(pattern, flags, values, valid=None, negate=False):
    """-> (bits, declined bits) of dbhip_regex_eval over a column; identical values are decided once"""
    memo, bits, declined = {}, [], []
    for i, v in enumerate(values):
        if valid is not None and not valid[i]:
            bits.append(False)
            declined.append(False)
            continue
        v = bytes(v)
        if v not in memo:
            memo[v] = match(pattern, flags, v)
        r = memo[v]
        declined.append(r == DECLINED)
        bits.append(r != DECLINED and (bool(r) != negate))
    return bits, declined
