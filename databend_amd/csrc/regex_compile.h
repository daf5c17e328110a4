// regex_compile.h — a constant regular expression -> a byte-class DFA (include/dbhip.h a25). Host C++ only, no HIP and nothing of the
// library in it, so that a host program compiles the very same text under sanitizers (tests/regex_host_check.cpp).
//   parser     the grammar of the a25 comment, nothing more: whatever lies outside it is refused, never guessed at. The result is a
//              small syntax tree over BYTE SETS; a unit (`.`, a negated class, \D \W \S without UNIT_BYTE) is expanded right here into
//              ascii-set | [C0-FF][80-BF]*, a non-ASCII literal into the sequence of its bytes.
//   NFA        Thompson's construction, built back to front (every node is emitted with the state that follows it), counted
//              repetitions by emitting the operand again. A "position" is a state that consumes a byte.
//   DFA        subset construction over byte classes (the coarsest partition of 0..255 under which every position's set is a union
//              of classes). The search form re-adds the start state at every step; `^` is passable only in the initial closure, `$`
//              only when the input has ended, which a state remembers as its "accepts at end" flag. A state that has reached the
//              match without a `$` accepts whatever follows: all such sets are the one STICKY state. FULL_MATCH wraps the tree in
//              ^(?:..)$ and is otherwise no special case.
// No minimisation. Compilation stops at the first cap that is passed; no message names a constant of the group (tests/test_abi.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

constexpr int RX_MAX_PATTERN = 1024, RX_MAX_POSITIONS = 4096, RX_MAX_STATES = 4096, RX_MAX_TABLE_BYTES = 32768, RX_MAX_REPEAT = 1000,
              RX_MAX_DEPTH = 64;
constexpr int RX_F_CASE_INSENSITIVE = 1, RX_F_DOT_NL = 2, RX_F_UNIT_BYTE = 4, RX_F_FULL_MATCH = 8;
constexpr uint8_t RX_ACCEPT_END = 1, RX_STICKY = 2, RX_DEAD = 4;   // state flags
constexpr int RX_OK = 0, RX_INVALID = 1, RX_UNSUPPORTED = 2;        // rx_compile's result (the caller maps them to its status codes)

struct RxSet {
  uint64_t w[4];
  bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1u; }
  void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63); }
  void add_range(uint32_t lo, uint32_t hi) { for (uint32_t b = lo; b <= hi; ++b) add(b); }
  bool operator<(const RxSet& o) const { return memcmp(w, o.w, sizeof(w)) < 0; }
};

struct RxProgram {
  uint8_t cmap[256];             // byte -> class
  std::vector<uint16_t> table;   // [state][class] -> state; state 0 is the start
  std::vector<uint8_t> flags;    // per state: RX_ACCEPT_END | RX_STICKY | RX_DEAD
  uint32_t n_classes = 0;
  bool needs_ascii = false;      // CASE_INSENSITIVE, or one of \d \w \s \D \W \S in the pattern
  uint32_t n_positions = 0;
};

namespace rx_detail {

enum { N_EMPTY, N_SET, N_CAT, N_ALT, N_REP, N_BOL, N_EOL };
struct Node {
  int type, set, lo, hi;         // N_REP: lo .. hi repetitions, hi < 0: unbounded
  std::vector<int> kids;
  uint32_t positions, states;    // what the node emits, saturating
};

inline uint32_t sat_add(uint32_t a, uint32_t b) { return a + b > (1u << 20) ? (1u << 20) : a + b; }
inline uint32_t sat_mul(uint32_t a, uint32_t b) { const uint64_t p = (uint64_t)a * b; return p > (1u << 20) ? (1u << 20) : (uint32_t)p; }

struct Parser {
  const uint8_t* p;
  int len, at = 0, flags, depth = 0;
  const char* why = nullptr;
  bool needs_ascii = false;
  std::vector<Node> nodes;
  std::vector<RxSet> sets;
  std::map<RxSet, int> set_ids;

  bool fail(const char* w) { if (!why) why = w; return false; }
  bool unit_byte() const { return flags & RX_F_UNIT_BYTE; }
  int node(int type, int set = -1) {
    Node n{type, set, 0, 0, {}, type == N_SET ? 1u : 0u, (type == N_SET || type == N_BOL || type == N_EOL) ? 1u : 0u};
    nodes.push_back(n);
    return (int)nodes.size() - 1;
  }
  int set_node(const RxSet& s) {
    auto it = set_ids.find(s);
    if (it == set_ids.end()) { it = set_ids.emplace(s, (int)sets.size()).first; sets.push_back(s); }
    return node(N_SET, it->second);
  }
  int list(int type, const std::vector<int>& kids) {
    if (kids.size() == 1) return kids[0];
    if (kids.empty()) return node(N_EMPTY);
    const int n = node(type);
    nodes[n].kids = kids;
    uint32_t pos = 0, st = 0;
    for (int k : kids) { pos = sat_add(pos, nodes[k].positions); st = sat_add(st, nodes[k].states); }
    nodes[n].positions = pos;
    nodes[n].states = sat_add(st, type == N_ALT ? (uint32_t)kids.size() : 0u);
    return n;
  }
  // the copies Emit makes of a repetition's operand: x{m,} -> max(m, 1), x{m,n} -> n
  int repeat(int kid, int lo, int hi) {
    const int n = node(N_REP);
    const uint32_t copies = hi < 0 ? (uint32_t)(lo > 1 ? lo : 1) : (uint32_t)hi;
    nodes[n].kids = {kid};
    nodes[n].lo = lo;
    nodes[n].hi = hi;
    nodes[n].positions = sat_mul(nodes[kid].positions, copies);
    nodes[n].states = sat_mul(sat_add(nodes[kid].states, 1), copies ? copies : 1u);
    return n;
  }

  // ---- byte sets -------------------------------------------------------------------------------------------------------------------
  static RxSet none() { RxSet s; memset(&s, 0, sizeof(s)); return s; }
  void fold(RxSet& s) const {
    if (!(flags & RX_F_CASE_INSENSITIVE)) return;
    for (uint32_t c = 'a'; c <= 'z'; ++c) {
      if (s.has(c)) s.add(c - 32);
      if (s.has(c - 32)) s.add(c);
    }
  }
  static void add_perl(RxSet& s, uint8_t c) {     // d w s
    if (c == 'd' || c == 'w') s.add_range('0', '9');
    if (c == 'w') { s.add_range('A', 'Z'); s.add_range('a', 'z'); s.add('_'); }
    if (c == 's') { s.add(' '); s.add_range(9, 13); }
  }
  // one unit that is not in `excluded`: a byte (UNIT_BYTE), else an ASCII byte not excluded or a lead byte with its continuation bytes
  int unit_except(const RxSet& excluded) {
    RxSet s = none();
    const uint32_t top = unit_byte() ? 256 : 128;
    for (uint32_t b = 0; b < top; ++b) if (!excluded.has(b)) s.add(b);
    if (unit_byte()) return set_node(s);
    RxSet lead = none(), cont = none();
    lead.add_range(0xC0, 0xFF);
    cont.add_range(0x80, 0xBF);
    const int multi = list(N_CAT, {set_node(lead), repeat(set_node(cont), 0, -1)});
    return list(N_ALT, {set_node(s), multi});
  }
  static bool is_punct(uint8_t c) { return (c >= 0x21 && c <= 0x2F) || (c >= 0x3A && c <= 0x40) || (c >= 0x5B && c <= 0x60) || (c >= 0x7B && c <= 0x7E); }
  static int hex(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

  // an escape behind the backslash at p[at - 1]: a byte (>= 0), or -1 - c for the class escape c (d w s D W S), or -1000 (refused)
  int escape() {
    if (at >= len) { fail("a backslash at the end of the pattern"); return -1000; }
    const uint8_t c = p[at++];
    switch (c) {
      case 't': return 9; case 'n': return 10; case 'v': return 11; case 'f': return 12; case 'r': return 13;
      case 'd': case 'w': case 's': case 'D': case 'W': case 'S': needs_ascii = true; return -1 - (int)c;
      case 'x': {
        if (at + 2 > len || hex(p[at]) < 0 || hex(p[at + 1]) < 0) { fail("\\x needs two hexadecimal digits"); return -1000; }
        const int v = hex(p[at]) * 16 + hex(p[at + 1]);
        at += 2;
        if (v > 0x7F && !unit_byte()) { fail("\\x above 7F without the byte unit"); return -1000; }
        return v;
      }
      default: break;
    }
    if (is_punct(c)) return c;
    fail("an escape outside the grammar (word boundaries, \\A \\z, \\p{..}, backreferences ..)");
    return -1000;
  }

  bool klass(int* out) {       // behind '['
    bool negate = false;
    if (at < len && p[at] == '^') { negate = true; ++at; }
    RxSet s = none();
    const int first = at;
    int prev = -1;              // the last single byte, a candidate for the low end of a range; -1: none
    for (;;) {
      if (at >= len) return fail("a class without its closing bracket");
      uint8_t c = p[at];
      if (c == ']') {
        if (at == first) return fail("an empty class, or an unescaped ] at the start of a class");
        ++at;
        break;
      }
      if (c >= 0x80) return fail("a byte above 7F inside a class");
      if (c == '[') return fail("an unescaped [ inside a class (POSIX classes and nested classes are outside the grammar)");
      if (c == '^') return fail("an unescaped ^ inside a class");
      if ((c == '&' || c == '~' || c == '-') && at + 1 < len && p[at + 1] == c) return fail("a set operation inside a class");
      int lo;
      ++at;
      if (c == '-') {
        const bool last = at < len && p[at] == ']';
        if (at - 1 == first || last) { s.add('-'); prev = -1; continue; }
        if (prev < 0) return fail("a - inside a class that neither forms a range nor stands first or last");
        // the high end
        if (at >= len) return fail("a class without its closing bracket");
        uint8_t h = p[at++];
        int hi = h;
        if (h == '\\') { hi = escape(); if (hi == -1000) return false; if (hi < 0) return fail("a class escape as the end of a range"); }
        else if (h >= 0x80 || h == '[' || h == ']' || h == '^') return fail("a range end that must be escaped");
        if (hi < prev) return fail("a descending range inside a class");
        s.add_range((uint32_t)prev, (uint32_t)hi);
        prev = -1;
        continue;
      }
      if (c == '\\') {
        lo = escape();
        if (lo == -1000) return false;
        if (lo < 0) {
          const uint8_t k = (uint8_t)(-1 - lo);
          if (k == 'D' || k == 'W' || k == 'S') return fail("\\D \\W \\S inside a class");
          add_perl(s, k);
          if (at < len && p[at] == '-' && !(at + 1 < len && p[at + 1] == ']')) return fail("a class escape as the start of a range");
          prev = -1;
          continue;
        }
      } else lo = c;
      s.add((uint32_t)lo);
      prev = lo;
    }
    fold(s);
    if (!negate) { *out = set_node(s); return true; }
    *out = unit_except(s);
    return true;
  }

  static int utf8_len(const uint8_t* q, int left) {     // the length of the well-formed sequence at q, or 0
    const uint8_t c = q[0];
    int n;
    uint8_t lo = 0x80, hi = 0xBF;
    if (c >= 0xC2 && c <= 0xDF) n = 2;
    else if (c >= 0xE0 && c <= 0xEF) { n = 3; if (c == 0xE0) lo = 0xA0; if (c == 0xED) hi = 0x9F; }
    else if (c >= 0xF0 && c <= 0xF4) { n = 4; if (c == 0xF0) lo = 0x90; if (c == 0xF4) hi = 0x8F; }
    else return 0;
    if (left < n || q[1] < lo || q[1] > hi) return 0;
    for (int k = 2; k < n; ++k) if (q[k] < 0x80 || q[k] > 0xBF) return 0;
    return n;
  }
  int byte_node(uint32_t b) { RxSet s = none(); s.add(b); fold(s); return set_node(s); }

  // an atom with its quantifier; *out = -1 at the end of a branch
  bool piece(int* out) {
    *out = -1;
    if (at >= len) return true;
    const uint8_t c = p[at];
    if (c == '|' || c == ')') return true;
    int atom = -1;
    bool quantifiable = true;
    ++at;
    switch (c) {
      case '*': case '+': case '?': return fail("a quantifier with nothing to repeat");
      case '{': return fail("a { that does not form a counted repetition");
      case '^': atom = node(N_BOL); quantifiable = false; break;
      case '$': atom = node(N_EOL); quantifiable = false; break;
      case '.': { RxSet ex = none(); if (!(flags & RX_F_DOT_NL)) ex.add('\n'); atom = unit_except(ex); break; }
      case '[': if (!klass(&atom)) return false; break;
      case '(': {
        if (at < len && p[at] == '?') {
          ++at;
          if (at < len && p[at] == ':') ++at;
          else if (at + 1 < len && p[at] == 'P' && p[at + 1] == '<') {
            at += 2;
            const int name = at;
            while (at < len && (p[at] == '_' || (p[at] >= '0' && p[at] <= '9') || ((p[at] | 32) >= 'a' && (p[at] | 32) <= 'z'))) ++at;
            if (at == name || (p[name] >= '0' && p[name] <= '9') || at >= len || p[at] != '>') return fail("a group name that is no identifier");
            ++at;
          } else return fail("a (? group outside the grammar (inline flags, look-around ..)");
        }
        if (++depth > RX_MAX_DEPTH) return fail("groups nested more than 64 deep");
        if (!alternation(&atom)) return false;
        --depth;
        if (at >= len || p[at] != ')') return fail("a group without its closing parenthesis");
        ++at;
        break;
      }
      case '\\': {
        const int e = escape();
        if (e == -1000) return false;
        if (e >= 0) { atom = byte_node((uint32_t)e); break; }
        const uint8_t k = (uint8_t)(-1 - e);
        RxSet s = none();
        add_perl(s, (uint8_t)(k | 32));
        atom = (k & 32) ? set_node(s) : unit_except(s);
        break;
      }
      default:
        if (c < 0x80 || unit_byte()) { atom = byte_node(c); break; }
        {
          const int n = utf8_len(p + at - 1, len - at + 1);
          if (!n) return fail("a byte above 7F that is not part of a well-formed UTF-8 sequence");
          std::vector<int> seq;
          for (int k = 0; k < n; ++k) seq.push_back(byte_node(p[at - 1 + k]));
          at += n - 1;
          atom = list(N_CAT, seq);
        }
    }
    // the quantifier
    if (at < len && (p[at] == '*' || p[at] == '+' || p[at] == '?' || p[at] == '{')) {
      if (!quantifiable) return fail("a quantifier on ^ or $");
      int lo, hi;
      const uint8_t q = p[at++];
      if (q == '*') { lo = 0; hi = -1; }
      else if (q == '+') { lo = 1; hi = -1; }
      else if (q == '?') { lo = 0; hi = 1; }
      else {
        auto number = [&](int* v) {
          const int from = at;
          long x = 0;
          while (at < len && p[at] >= '0' && p[at] <= '9') { x = x * 10 + (p[at] - '0'); if (x > 100000) x = 100000; ++at; }
          *v = (int)x;
          return at > from;
        };
        if (!number(&lo)) return fail("a { that does not form a counted repetition");
        hi = lo;
        if (at < len && p[at] == ',') {
          ++at;
          if (at < len && p[at] == '}') hi = -1;
          else if (!number(&hi)) return fail("a { that does not form a counted repetition");
        }
        if (at >= len || p[at] != '}') return fail("a { that does not form a counted repetition");
        ++at;
        if (lo > RX_MAX_REPEAT || hi > RX_MAX_REPEAT) return fail("a repetition count above 1000");
        if (hi >= 0 && hi < lo) return fail("a counted repetition whose upper bound is below its lower bound");
      }
      if (at < len && p[at] == '?') ++at;      // lazy: the same set of values
      if (at < len && (p[at] == '*' || p[at] == '+' || p[at] == '?' || p[at] == '{')) return fail("a quantifier on a quantifier (possessive forms included)");
      atom = repeat(atom, lo, hi);
      if (nodes[atom].positions > (uint32_t)RX_MAX_POSITIONS || nodes[atom].states > 16u * RX_MAX_POSITIONS)
        return fail("more than 4096 NFA positions after expanding the counted repetitions");
    }
    *out = atom;
    return true;
  }

  bool alternation(int* out) {
    std::vector<int> branches;
    for (;;) {
      std::vector<int> seq;
      for (;;) {
        int a;
        if (!piece(&a)) return false;
        if (a < 0) break;
        seq.push_back(a);
      }
      branches.push_back(list(N_CAT, seq));
      if (at < len && p[at] == '|') { ++at; continue; }
      break;
    }
    *out = list(N_ALT, branches);
    if (nodes[*out].positions > (uint32_t)RX_MAX_POSITIONS || nodes[*out].states > 16u * RX_MAX_POSITIONS)
      return fail("more than 4096 NFA positions after expanding the counted repetitions");
    return true;
  }
};

enum { S_CHAR, S_SPLIT, S_BOL, S_EOL, S_MATCH };
struct State { int kind, set, out, out1; };

struct Emit {
  const std::vector<Node>& nodes;
  std::vector<State> st;
  int add(int kind, int set, int out, int out1 = -1) { st.push_back(State{kind, set, out, out1}); return (int)st.size() - 1; }
  int emit(int n, int next) {
    const Node& N = nodes[n];
    switch (N.type) {
      case N_EMPTY: return next;
      case N_SET: return add(S_CHAR, N.set, next);
      case N_BOL: return add(S_BOL, -1, next);
      case N_EOL: return add(S_EOL, -1, next);
      case N_CAT: { for (size_t k = N.kids.size(); k-- > 0;) next = emit(N.kids[k], next); return next; }
      case N_ALT: {
        int entry = emit(N.kids.back(), next);
        for (size_t k = N.kids.size() - 1; k-- > 0;) entry = add(S_SPLIT, -1, emit(N.kids[k], next), entry);
        return entry;
      }
      default: break;
    }
    const int kid = N.kids[0];
    if (nodes[kid].states == 0) return next;          // an operand that emits nothing matches the empty string only
    int entry, lo = N.lo;
    if (N.hi < 0) {
      const int loop = add(S_SPLIT, -1, -1, next);
      const int body = emit(kid, loop);
      st[loop].out = body;
      entry = lo == 0 ? loop : body;
      if (lo > 0) --lo;
    } else {
      entry = next;
      for (int k = N.lo; k < N.hi; ++k) entry = add(S_SPLIT, -1, emit(kid, entry), next);
    }
    for (int k = 0; k < lo; ++k) entry = emit(kid, entry);
    return entry;
  }
};

}  // namespace rx_detail

// Compiles pattern[0 .. len) under the create flags. RX_OK and *prog filled; else RX_INVALID / RX_UNSUPPORTED and *why set.
inline int rx_compile(const uint8_t* pattern, int32_t len, int32_t flags, RxProgram* prog, const char** why) {
  using namespace rx_detail;
  *why = "";
  if (len < 0 || (len > 0 && !pattern)) { *why = "NULL pattern or a negative length"; return RX_INVALID; }
  if (flags & ~(RX_F_CASE_INSENSITIVE | RX_F_DOT_NL | RX_F_UNIT_BYTE | RX_F_FULL_MATCH)) { *why = "unknown flag bits"; return RX_INVALID; }
  if (len > RX_MAX_PATTERN) { *why = "a pattern of more than 1024 bytes"; return RX_UNSUPPORTED; }
  if (flags & RX_F_CASE_INSENSITIVE)
    for (int32_t k = 0; k < len; ++k)
      if (pattern[k] >= 0x80) { *why = "a byte above 7F in a case-insensitive pattern"; return RX_UNSUPPORTED; }
  Parser P;
  P.p = pattern;
  P.len = len;
  P.flags = flags;
  P.needs_ascii = (flags & RX_F_CASE_INSENSITIVE) != 0;
  int root;
  if (!P.alternation(&root)) { *why = P.why; return RX_UNSUPPORTED; }
  if (P.at < len) { *why = "a closing parenthesis without its group"; return RX_UNSUPPORTED; }
  if (flags & RX_F_FULL_MATCH) root = P.list(N_CAT, {P.node(N_BOL), root, P.node(N_EOL)});

  Emit E{P.nodes, {}};
  E.st.reserve(P.nodes[root].states + 2);
  const int match = E.add(S_MATCH, -1, -1);
  const int start = E.emit(root, match);
  const std::vector<State>& st = E.st;
  const std::vector<RxSet>& sets = P.sets;

  // byte classes: bytes with the same membership in every set
  uint32_t ncls = 0;
  {
    std::map<std::string, uint32_t> sig_ids;
    std::string sig(sets.size(), '0');
    for (uint32_t b = 0; b < 256; ++b) {
      for (size_t k = 0; k < sets.size(); ++k) sig[k] = sets[k].has(b) ? '1' : '0';
      auto it = sig_ids.find(sig);
      if (it == sig_ids.end()) it = sig_ids.emplace(sig, ncls++).first;
      prog->cmap[b] = (uint8_t)it->second;
    }
  }
  std::vector<uint8_t> rep(ncls);                         // one byte of every class
  for (uint32_t b = 256; b-- > 0;) rep[prog->cmap[b]] = (uint8_t)b;
  if ((size_t)ncls * 2 > (size_t)RX_MAX_TABLE_BYTES) { *why = "a table beyond 32 KiB"; return RX_UNSUPPORTED; }

  // the closure of `seeds`: the positions in it (sorted), whether the match is reached as things stand (sticky) and whether it is
  // reached when the input ends here
  std::vector<uint32_t> stamp(st.size(), 0);
  uint32_t tick = 0;
  std::vector<int> stack, ends;
  auto closure = [&](const std::vector<int>& seeds, bool at_start, std::vector<int>* positions, bool* sticky, bool* accept_end) {
    ++tick;
    positions->clear();
    ends.clear();
    stack.assign(seeds.begin(), seeds.end());
    bool matched = false, at_end = false;
    for (int pass = 0; pass < 2; ++pass) {
      while (!stack.empty()) {
        const int s = stack.back();
        stack.pop_back();
        if (stamp[s] == tick) continue;
        stamp[s] = tick;
        const State& S = st[s];
        if (S.kind == S_CHAR) { if (!at_end) positions->push_back(s); }
        else if (S.kind == S_MATCH) matched = true;
        else if (S.kind == S_SPLIT) { stack.push_back(S.out1); stack.push_back(S.out); }
        else if (S.kind == S_BOL) { if (at_start) stack.push_back(S.out); }
        else if (at_end) stack.push_back(S.out);
        else ends.push_back(S.out);
      }
      if (pass == 0) {
        *sticky = matched;
        at_end = true;
        stack.assign(ends.begin(), ends.end());
      }
    }
    *accept_end = matched;
    std::sort(positions->begin(), positions->end());
  };

  std::map<std::vector<int>, uint32_t> ids;     // key: the positions, then -1 - flags
  std::vector<std::vector<int>> members;
  prog->flags.clear();
  prog->table.clear();
  auto intern = [&](std::vector<int>& positions, bool sticky, bool accept_end, uint32_t* id) {
    uint8_t f = 0;
    if (sticky) { positions.clear(); f = RX_STICKY | RX_ACCEPT_END; }
    else if (accept_end) f = RX_ACCEPT_END;
    else if (positions.empty()) f = RX_DEAD;
    positions.push_back(-1 - (int)f);
    auto it = ids.find(positions);
    if (it == ids.end()) {
      if (members.size() >= (size_t)RX_MAX_STATES) { *why = "more than 4096 DFA states"; return false; }
      if ((members.size() + 1) * ncls * 2 > (size_t)RX_MAX_TABLE_BYTES) { *why = "a table beyond 32 KiB"; return false; }
      it = ids.emplace(positions, (uint32_t)members.size()).first;
      positions.pop_back();
      members.push_back(positions);
      prog->flags.push_back(f);
    }
    *id = it->second;
    return true;
  };

  std::vector<int> seeds, positions;
  bool sticky, accept_end;
  uint32_t id;
  seeds.push_back(start);
  closure(seeds, true, &positions, &sticky, &accept_end);
  if (!intern(positions, sticky, accept_end, &id)) return RX_UNSUPPORTED;
  for (size_t s = 0; s < members.size(); ++s) {
    prog->table.resize((s + 1) * ncls);
    for (uint32_t c = 0; c < ncls; ++c) {
      if (prog->flags[s] & (RX_STICKY | RX_DEAD)) { prog->table[s * ncls + c] = (uint16_t)s; continue; }
      seeds.clear();
      for (int q : members[s]) if (sets[st[q].set].has(rep[c])) seeds.push_back(st[q].out);
      seeds.push_back(start);
      closure(seeds, false, &positions, &sticky, &accept_end);
      if (!intern(positions, sticky, accept_end, &id)) return RX_UNSUPPORTED;
      prog->table[s * ncls + c] = (uint16_t)id;
    }
  }
  prog->n_classes = ncls;
  prog->needs_ascii = P.needs_ascii;
  prog->n_positions = P.nodes[root].positions;
  return RX_OK;
}
