"""The patterns and the value generators shared by the tests of the regular-expression predicates (include/dbhip.h a25):
tests/test_regex_ref_cpu.py (the restatement against Python's `re`), tests/test_regex_host_cpu.py (the library's compiler and row walk
on the host against the restatement) and tests/test_gpu_regex.py (the kernels against the restatement). Plain Python, no device."""
import random

CI, NL, UB, FM = 1, 2, 4, 8            # CASE_INSENSITIVE, DOT_NL, UNIT_BYTE, FULL_MATCH

E2, E3, E4 = "é".encode(), "€".encode(), "😀".encode()
URL = rb"^https?://(?:www\.)?([^/]+)/.*$"
IPV4 = rb"[0-9]{1,3}(\.[0-9]{1,3}){3}"
WORDS = rb"(foo|bar|baz){2,5}qux"
DOT255 = rb".{255}"                                      # about 500 DFA states
BIG = rb"(a|b)*a(a|b){9}(x|y|z|0|1|2|3|4)$"             # more than 1,000 DFA states, 11 byte classes: a table of over 20 KB

# (pattern, create flags). Every one is inside the grammar and the limits.
PATTERNS = [
    (b"", 0), (b"", FM), (b"google", 0), (b"google", FM), (b"google", CI), (b"goo|gle", FM), (b"^(?:goo|gle)$", 0),
    (URL, 0), (URL, UB), (URL, NL),
    (rb"^.{3}$", 0), (rb"^.{3}$", UB), (b"a.c", 0), (b"a.c", UB), (b"a.c", NL), (E2 + b"+x", 0), (E2 + b"+x", UB), (b"a" + E3 + b"?" + E4, 0),
    (b"x[^y]z", 0), (b"x[^y]z", UB), (IPV4, 0), (IPV4, FM), (WORDS, 0), (WORDS, FM), (b"^(?:" + WORDS + b")$", 0), (DOT255, 0), (DOT255, UB), (BIG, 0),
    (rb"\d+\s\w+", 0), (rb"\d+\s\w+", UB), (rb"\D\W\S", 0), (rb"[\d_]+$", 0), (rb"^[\w.]+@[\w.]+$", 0), (b"k", CI), (b"[^k]x", CI), (b"[a-f]+[G-H]$", CI),
    (b"a$", 0), (b"^a", 0), (b"x$", 0), (b"^$", 0), (b"$", 0), (b"^", 0), (b"a|", 0), (b"(|a)b", 0), (b"(?P<n_1>ab)+c", 0), (b"ab*?c", 0), (b"ab+?c$", 0),
    (b"a{2}", 0), (b"a{2,}b", 0), (b"a{0}b", 0), (b"^a{0,2}b$", 0), (b"(ab){2,3}?x", 0), (b"()*a", 0), (b"(a*)*$", 0), (b"^(a|ab)(c|bcd)$", 0),
    (rb"[a-c-]+\.", 0), (rb"[-a]b", 0), (rb"[\]\[\\\^]", 0), (rb"\x41\x2e", 0), (rb"\t|\n", 0), (rb"[\t-\r]x", 0), (b"a}]", 0), (rb"\.\*\+", 0),
    (b".", 0), (b".", NL), (b".", UB), (b"^.*$", 0), (b"^.*$", NL), (b"^.*$", NL | UB), (b"[^a]$", 0), (b"^[^a]+$", 0), (b"^[^a]+$", UB), (rb"^\W$", 0),
    (rb"\xe9", UB), (E2, UB), (rb"[^\x00-\x7f]", UB), (rb"^[\x80-\xff]+$", UB), (b"(a|b)*abb", 0), (b"b$|^a", 0), (b"a$b|c", 0), (b"(^a|b)c", 0),
]

LENGTHS = (0, 1, 11, 12, 13, 15, 16, 17, 255, 256, 257)

FIXED = [
    b"", b"a", b"b", b"x", b"k", b"K", "\u212a".encode(), b"google", b"GooGle", b"goo", b"gle", b"xgooglex", b"goog\nle",
    b"http://www.google.com/", b"https://a.b/c", b"http://x", b"http:///", b"ftp://www.x/", b"https://www./", b"xhttp://a/", b"http://a/\n", b"http://a\n/b",
    b"http://" + E2 + b"/", b"https://www.example.org/a/b?c=d", b"https://www.example.org", b"http://www.a/",
    b"a\n", b"\n", b"\na", b"abc", b"a\nc", b"a" + E2 + b"c", b"a" + E3 + b"c", b"a" + E4 + b"c", b"ac", b"a" + E2 + E2 + b"c", b"abcd", b"ab",
    E2, E2 * 2, E2 * 3, E2 + b"x", E2 * 2 + b"x", b"\xc3x", b"\xa9", b"\xa9x", b"a\xa9c", b"\xc3\xa9\xa9", b"\xc3\xa9\xa9x", b"a\xc3", b"\xff\x80\x80\x80", b"\xe9", b"a\xe9c",
    E3 * 3, E4 * 3, E2 + E3 + E4, b"abc"[:3], b"ab" + E2, b"a" + E4, b"a" + E3 + E4, b"a" + E4 + b"x",
    b"xyz", b"xaz", b"xz", b"x" + E2 + b"z", b"x" + E3 + b"z", b"x\xa9z", b"x\nz", b"xyyz",
    b"1.2.3.4", b"999.999.999.9999", b"1.2.3", b"1..2.3.4", b"a1.2.3.4b", b"1234.1.1.1", b"1.2.3.",
    b"foobarqux", b"fooqux", b"foobarbazfoobarqux", b"foobarbazfoobarbazqux", b"foobazqu", b"xfoofooqux", b"foofooquxx", b"barbarqux",
    b"12 ab", "\u0661\u0662 ab".encode(), b"12\tab_9", b"12ab", b"1 " + E2, b"12 ab" + E2, E2 + b"12 ab", b"12\x1cab", b"7_", b"_", b"a@b", b"a.b@c.d", b"a@b@c", b"@", b"a b@c",
    b"aa", b"aaa", b"aab", b"b", b"ab", b"abab", b"ababx", b"ababab", b"ababababx", b"abc", b"abbc", b"ac", b"abcd", b"abbcd", b"abbb", b"aabb", b"c", b"ab\nc",
    b"a-c.", b"-.", b"-b", b"ab", b"]", b"[", b"\\", b"^", b"A.", b"A", b"\t", b"\rx", b"a}]", b".*+", b"abcdefG", b"ABCDEFh", b"abcdefg",
    b"aaaaaaaaaax", b"abababababa0", b"bbbbbbbbbbbx", b"a123456789x", b"aaaaaaaaaaaa", b"\x00", b"a\x00c", b"\x7f", b"x\x80", b"\x80x",
]


def ab(rng, n, alphabet=b"ab"):
    """n random bytes of the alphabet; rng: random.Random or a numpy Generator"""
    if hasattr(rng, "integers"):
        return bytes(alphabet[int(k)] for k in rng.integers(0, len(alphabet), n))
    return bytes(rng.choice(alphabet) for _ in range(n))


def length_values(seed=1):
    """for every length of LENGTHS: {a, b} values, some ending so that BIG matches, with a needle at the start / the end, multi-byte ones"""
    rng = random.Random(seed)
    out = []
    for ln in LENGTHS:
        out += [ab(rng, ln), (ab(rng, ln) + b"a" + ab(rng, 9) + b"3")[-ln:] if ln else b"", (b"google" + ab(rng, ln))[:ln], (ab(rng, ln) + b"google")[-ln:] if ln else b"",
                (E2 * ln)[:ln], (b"a" + E3 * ln)[:ln], (E4 * ln)[:max(ln - 1, 0)] + b"x"[:min(ln, 1)], (b"http://www.a/" + ab(rng, ln, b"ab/"))[:ln],
                (ab(rng, ln, b"0123456789.") + b" 1.22.333.4")[-ln:] if ln else b"", (b"foobarbaz" * 40)[:max(ln - 3, 0)] + b"qux"[:ln]]
    return out


def long_value(seed=2):
    """5,000 bytes: BIG, DOT255, `google` and `x$` all have to walk to its end"""
    rng = random.Random(seed)
    return ab(rng, 4983) + b"google" + b"a" + ab(rng, 9) + b"x"


def random_values(seed, n, max_len=40):
    rng = random.Random(seed)
    alphabets = [b"ab", b"abxyz01234", b"0123456789. ", b"gole", b"htps:/w.a", b"xyz\n", b"kK_ 9\t"]
    tokens = [b"foo", b"bar", b"baz", b"qux", E2, E3, E4, b"x", b"a", b"c", b"\n", b"1", b".", b" ", b"google", b"http://", b"www.", b"/"]
    out = []
    for _ in range(n):
        if rng.random() < 0.5:
            out.append(ab(rng, rng.randrange(max_len), rng.choice(alphabets)))
        else:
            out.append(b"".join(rng.choice(tokens) for _ in range(rng.randrange(8)))[:max_len])
    return out


def utf8_values(seed, n, max_len=12):
    """random VALID UTF-8 of code points of 1 to 4 bytes (and newlines)"""
    rng = random.Random(seed)
    pool = "abcxyz\n09 _/.kK" + "éüß" + "€あ\u212a" + "😀𝄞"
    return ["".join(rng.choice(pool) for _ in range(rng.randrange(max_len))).encode() for _ in range(n)]


def byte_values(seed, n, max_len=10):
    """random bytes, valid UTF-8 or not"""
    rng = random.Random(seed)
    pool = b"abxz\n0 ." + b"\xc3\xa9\x80\xbf\xe2\x82\xac\xf0\xff\xc0"
    return [bytes(rng.choice(pool) for _ in range(rng.randrange(max_len))) for _ in range(n)]


def all_values():
    """the pool of the host checker: every fixed value, every length, random ones and the long one"""
    return list(dict.fromkeys(FIXED + length_values() + random_values(3, 150) + byte_values(4, 80) + utf8_values(5, 80) + [long_value()]))
