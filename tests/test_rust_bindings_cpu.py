"""CPU: bindings/dbhip_sys.rs cannot be compiled where there is no Rust toolchain, and tests/test_abi.py compares it with what the
generator makes of the header — so a name that is no Rust identifier passes there. This file checks the identifiers themselves: no
struct field and no parameter of the generated FFI is a bare Rust keyword (a C parameter called `fn` or `type` is written `r#fn`,
`r#type`), and the generator's rule covers the whole keyword list."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_bindings as G  # noqa: E402

# The Rust Reference, "Keywords": strict, reserved, and the weak ones that are reserved in some edition
KEYWORDS = """as break const continue crate else enum extern false fn for if impl in let loop match mod move mut pub ref return self Self
static struct super trait true type unsafe use where while async await dyn abstract become box do final macro override priv typeof
unsized virtual yield try gen""".split()


def identifiers(text):
    """-> (struct field names, parameter names) as written, raw prefix included"""
    fields = []
    for body in re.findall(r"pub struct \w+ \{(.*?)\}", text, flags=re.S):
        fields += re.findall(r"pub ([^\s:]+):", body)
    params = []
    for args in re.findall(r"pub fn \w+\((.*?)\)", text, flags=re.S):
        params += [a.split(":")[0].strip() for a in args.split(",") if a.strip()]
    return fields, params


def test_no_identifier_of_the_committed_bindings_is_a_bare_keyword():
    text = open(os.path.join(ROOT, "bindings", "dbhip_sys.rs")).read()
    fields, params = identifiers(text)
    assert len(fields) > 40 and len(params) > 900
    bad = [n for n in fields + params if n in KEYWORDS]
    assert not bad, bad
    for n in fields + params:
        assert re.fullmatch(r"(r#)?[A-Za-z_][A-Za-z0-9_]*", n), n
    # the two parameters of the header that are keywords are there, raw
    assert "r#fn" in params and "r#type" in params and "r#type" in fields


def test_the_generator_escapes_every_keyword():
    for k in KEYWORDS:
        got = G.rust_ident(k)
        assert got != k and got not in KEYWORDS, k
        assert got == (k + "_" if k in ("self", "Self", "super", "crate") else "r#" + k), k      # (those four cannot be raw)
    for plain in ("src", "digits", "fn_", "types", "n", "out_type_host"):
        assert G.rust_ident(plain) == plain
    header = """typedef struct { int32_t type; int32_t match; const void* ref; } dbhip_probe;
int32_t dbhip_probe_call(int32_t fn, const dbhip_probe* in, int64_t loop, void* self);"""
    text, funcs = G.render(header)
    assert funcs == ["dbhip_probe_call"]
    assert "pub r#type: i32," in text and "pub r#match: i32," in text and "pub r#ref: *const c_void," in text
    assert "pub fn dbhip_probe_call(r#fn: i32, r#in: *const dbhip_probe, r#loop: i64, self_: *mut c_void) -> i32;" in text
