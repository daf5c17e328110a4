// dev_strfn.h — the row-level logic of the String functions (include/dbhip.h a22): units, slice ranges, trims, the result view, the
// bytes of a built value. Free of HIP, in the style of dev_strview.h, so that a host program compiles the very same text
// (tests/strfn_host_check.cpp). SF_FN is the functions' qualifier; SF_LOAD_U32(addr, value) is how an aligned word of a long value is
// read: the includer may define both.
// Everything here works on byte POSITIONS of one value and reads a byte only at a position below the value's length; the reader
// (SfValue::byte) turns that into naturally aligned 4-byte loads, each of which covers at least one byte of the value.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif
#include "dev_strview.h"

#if !defined(SF_FN) && (defined(__HIP__) || defined(__HIPCC_RTC__))
#define SF_FN __host__ __device__ __forceinline__
#elif !defined(SF_FN)
#define SF_FN inline
#endif
#ifndef SF_LOAD_U32
#define SF_LOAD_U32(addr, value) (*(const uint32_t*)(addr))
#endif

// the op codes are the public ones (k_strfn.hip asserts it)
enum { SF_SUBSTR = 0, SF_LEFT = 1, SF_RIGHT = 2, SF_TRIM_LEADING = 3, SF_TRIM_TRAILING = 4, SF_TRIM_BOTH = 5, SF_SLICE_COUNT = 6 };
enum { SF_CONCAT = 0, SF_UPPER = 1, SF_LOWER = 2, SF_BUILD_COUNT = 3 };
constexpr uint32_t SF_LONG_BYTES = 256;   // a lane walks no more than this many bytes of one value
constexpr int SF_MAX_PAD = 255, SF_MAX_ARGS = 8;

SF_FN bool sf_is_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }

// One value: its length, the (canonical) payload words of an inline value, the first byte's address of a long one.
struct SfValue {
  uint32_t len, w1, w2, w3;
  uintptr_t base;
  uintptr_t cached_at;   // 1: nothing cached (never a multiple of 4)
  uint32_t cached;
  SF_FN bool is_inline() const { return sv_is_inline(len); }
  SF_FN uint32_t load(uintptr_t a) const { return SF_LOAD_U32(a, *this); }
  SF_FN uint32_t inline_word(uint32_t pos) const {   // four bytes from `pos` of an inline value; past the view's 12: 0
    const uint32_t k = pos >> 2, sh = (pos & 3) * 8;
    const uint32_t lo = k == 0 ? w1 : (k == 1 ? w2 : (k == 2 ? w3 : 0u));
    const uint32_t hi = k == 0 ? w2 : (k == 1 ? w3 : 0u);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
  }
  SF_FN uint32_t byte(uint32_t pos) {   // pos < len
    if (is_inline()) return inline_word(pos) & 0xFFu;
    const uintptr_t a = base + pos, a0 = a & ~(uintptr_t)3;
    if (a0 != cached_at) { cached = load(a0); cached_at = a0; }
    return (cached >> (8 * (uint32_t)(a & 3))) & 0xFFu;
  }
};

// the value of a view that was loaded into registers (a long one: `bytes` is what sv_bytes_checked gave)
SF_FN SfValue sf_value(uint32_t len, uint32_t w1, uint32_t w2, uint32_t w3, const uint8_t* bytes) {
  SfValue v{len, w1, w2, w3, 0, 1, 0};
  if (sv_canon(len, v.w1, v.w2, v.w3)) v.base = 0;
  else v.base = (uintptr_t)bytes;
  return v;
}

// ---- units ---------------------------------------------------------------------------------------------------------------------------
// char_length: the number of units = the boundaries below len = len - (the 10xxxxxx bytes behind the first byte), whole words at a time
SF_FN uint32_t sf_cont4(uint32_t w) { return (w >> 7) & ~(w >> 6) & 0x01010101u; }   // 0x01 in every byte that is 10xxxxxx
SF_FN uint32_t sf_units(SfValue& v) {
  if (v.len == 0) return 0;
  uint32_t cont = 0;
  if (v.is_inline()) {      // canonical words: the zero bytes past len count nothing
    cont = (uint32_t)(__builtin_popcount(sf_cont4(v.w1)) + __builtin_popcount(sf_cont4(v.w2)) + __builtin_popcount(sf_cont4(v.w3)));
  } else {
    const uintptr_t end = v.base + v.len;
    for (uintptr_t p = v.base & ~(uintptr_t)3; p < end; p += 4) {
      uint32_t t = sf_cont4(v.load(p));
      if (p < v.base) t &= 0xFFFFFFFFu << (8 * (uint32_t)(v.base - p));
      if (end - p < 4) t &= 0xFFFFFFFFu >> (8 * (4 - (uint32_t)(end - p)));
      cont += (uint32_t)__builtin_popcount(t);
    }
  }
  return v.len - cont + (sf_is_cont(v.w1 & 0xFFu) ? 1u : 0u);     // w1 holds the first four bytes of any value, inline or not
}
// the position `k` units behind the boundary `from` (k >= 0), len when the value ends first
SF_FN uint32_t sf_forward(SfValue& v, uint32_t from, uint32_t k, bool unit_byte) {
  if (unit_byte) return k > v.len - from ? v.len : from + k;
  uint32_t p = from;
  while (k > 0 && p < v.len) {
    ++p;
    while (p < v.len && sf_is_cont(v.byte(p))) ++p;
    --k;
  }
  return p;
}
// the start of the m-th unit from the end (m >= 1); false when the value has fewer units
SF_FN bool sf_backward(SfValue& v, uint32_t m, bool unit_byte, uint32_t* at) {
  if (unit_byte) { if (m > v.len) return false; *at = v.len - m; return true; }
  uint32_t p = v.len;
  while (p > 0) {
    --p;
    if (p == 0 || !sf_is_cont(v.byte(p))) { if (--m == 0) { *at = p; return true; } }
  }
  return false;
}

// ---- SUBSTR / LEFT / RIGHT ---------------------------------------------------------------------------------------------------------------
// What the arguments ask for, decided by comparisons alone (every i64 is defined): nothing; or a start counted from the front
// (`front` units skipped) or from the end (the last `back` units), and then at most `take` units. All three are <= len.
struct SfPlan { bool empty, from_end, to_end; uint32_t front, back, take; };
SF_FN SfPlan sf_plan(int32_t op, uint32_t len, int64_t a, int64_t b, bool has_b) {
  SfPlan p{true, false, true, 0, 0, 0};
  if (len == 0) return p;
  const int64_t L = (int64_t)len;
  if (op == SF_LEFT || op == SF_RIGHT) {
    if (a <= 0) return p;
    p.empty = false;
    if (op == SF_LEFT) { p.to_end = a >= L; p.take = p.to_end ? len : (uint32_t)a; }
    else { p.from_end = true; p.back = a >= L ? len : (uint32_t)a; }
    return p;
  }
  if (a == 0 || (has_b && b <= 0)) return p;
  if (a > 0) {
    if (a - 1 >= L) return p;            // (a - 1: a > 0)
    p.front = (uint32_t)(a - 1);
  } else {
    if (a < -L) return p;
    p.from_end = true;
    p.back = (uint32_t)(-a);             // 1 .. len
  }
  p.empty = false;
  p.to_end = !has_b || b >= L;
  p.take = p.to_end ? len : (uint32_t)b;
  return p;
}
// does the plan read value bytes to find its range? (a lane may not when the value is longer than SF_LONG_BYTES)
SF_FN bool sf_plan_walks(const SfPlan& p, bool unit_byte) { return !p.empty && !unit_byte && (p.from_end || p.front || !p.to_end); }

// the byte range [*s, *e) of the plan; RIGHT with more units asked than the value has is the whole value, SUBSTR then empty
SF_FN void sf_plan_range(int32_t op, const SfPlan& p, SfValue& v, bool unit_byte, uint32_t* s, uint32_t* e) {
  *s = 0; *e = 0;
  if (p.empty) return;
  uint32_t st = 0;
  if (p.from_end) {
    if (!sf_backward(v, p.back, unit_byte, &st)) {
      if (op != SF_RIGHT) return;
      st = 0;
    }
  } else if (p.front) {
    st = sf_forward(v, 0, p.front, unit_byte);
    if (st >= v.len) return;
  }
  *s = st;
  *e = p.to_end ? v.len : sf_forward(v, st, p.take, unit_byte);
}

// ---- TRIM ----------------------------------------------------------------------------------------------------------------------------------
SF_FN bool sf_pad_at(SfValue& v, uint32_t pos, const uint8_t* pad, uint32_t p) {   // pos + p <= len
  for (uint32_t i = 0; i < p; ++i)
    if (v.byte(pos + i) != pad[i]) return false;
  return true;
}
SF_FN void sf_trim_range(int32_t op, SfValue& v, const uint8_t* pad, uint32_t p, uint32_t* s, uint32_t* e) {
  uint32_t lo = 0, hi = v.len;
  if (p > 0) {
    if (op == SF_TRIM_LEADING || op == SF_TRIM_BOTH)
      while (hi - lo >= p && sf_pad_at(v, lo, pad, p)) lo += p;
    if (op == SF_TRIM_TRAILING || op == SF_TRIM_BOTH)
      while (hi - lo >= p && sf_pad_at(v, hi - p, pad, p)) hi -= p;
  }
  *s = lo; *e = hi;
}

// Up to 12 bytes [s, s + n) of a long value (n >= 1) as three little-endian words, zero past n: at most four aligned loads, each of a
// word that holds one of those bytes.
SF_FN void sf_gather(const SfValue& v, uint32_t s, uint32_t n, uint32_t& w1, uint32_t& w2, uint32_t& w3) {
  const uintptr_t a = v.base + s, a0 = a & ~(uintptr_t)3, end = a + n;
  const uint32_t sh = (uint32_t)(a & 3) * 8;
  const uint32_t x0 = v.load(a0);
  const uint32_t x1 = a0 + 4 < end ? v.load(a0 + 4) : 0u;
  const uint32_t x2 = a0 + 8 < end ? v.load(a0 + 8) : 0u;
  const uint32_t x3 = a0 + 12 < end ? v.load(a0 + 12) : 0u;
  w1 = (uint32_t)((((uint64_t)x1 << 32) | x0) >> sh);
  w2 = (uint32_t)((((uint64_t)x2 << 32) | x1) >> sh);
  w3 = (uint32_t)((((uint64_t)x3 << 32) | x2) >> sh);
  sv_canon(n, w1, w2, w3);
}

// ---- the result view of a slice -------------------------------------------------------------------------------------------------------------
// bytes [s, e) of v as a view: inline and canonical up to 12 bytes, else {len', the slice's first four bytes, index, offset + s}
SF_FN void sf_slice_view(SfValue& v, uint32_t index, uint32_t offset, uint32_t s, uint32_t e, uint32_t (&w)[4]) {
  const uint32_t n = e - s;
  w[0] = n; w[1] = 0; w[2] = 0; w[3] = 0;
  if (n == 0) return;
  if (v.is_inline()) {
    w[1] = v.inline_word(s); w[2] = v.inline_word(s + 4); w[3] = v.inline_word(s + 8);
    sv_canon(n, w[1], w[2], w[3]);
    return;
  }
  if (sv_is_inline(n)) {
    if (s + n <= 4) {          // inside the view's own prefix word: no load
      w[1] = v.w1 >> (8 * s);
      sv_canon(n, w[1], w[2], w[3]);
      return;
    }
    sf_gather(v, s, n, w[1], w[2], w[3]);
    return;
  }
  if (s == 0) w[1] = v.w1;     // the view's own prefix word
  else { uint32_t x2, x3; sf_gather(v, s, 4, w[1], x2, x3); }
  w[2] = index;
  w[3] = offset + s;
}

// ---- built values: concat, upper, lower --------------------------------------------------------------------------------------------------
SF_FN uint32_t sf_map_byte(int32_t op, uint32_t c) {
  if (op == SF_UPPER) return (c - 0x61u) < 26u ? c - 0x20u : c;
  if (op == SF_LOWER) return (c - 0x41u) < 26u ? c + 0x20u : c;
  return c;
}
// Sends the result's bytes, in order, to sink.put(position, byte); args.get(k) is the k-th argument's value. Returns whether a byte
// >= 0x80 was among them.
template <class Args, class Sink>
SF_FN bool sf_emit(int32_t op, Args& args, int32_t nargs, Sink& sink) {
  uint32_t at = 0, high = 0;
  for (int32_t k = 0; k < nargs; ++k) {
    SfValue v = args.get(k);
    for (uint32_t i = 0; i < v.len; ++i) {
      const uint32_t c = v.byte(i);
      high |= c;
      sink.put(at++, sf_map_byte(op, c));
    }
  }
  return (high & 0x80u) != 0;
}
// a sink for results of up to 12 bytes: the view's three payload words
struct SfInlineSink {
  uint64_t lo;
  uint32_t hi;
  SF_FN void put(uint32_t at, uint32_t c) {
    if (at < 8) lo |= (uint64_t)c << (8 * at);
    else hi |= c << (8 * (at - 8));
  }
};
