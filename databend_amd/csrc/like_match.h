// like_match.h — the pattern table and the per-value matching steps of k_like.hip (include/dbhip.h a20), free of HIP so that a host
// program can run the very same steps with checked loads (tests/like_host_check.cpp). The includer defines LIKE_FN (the function
// qualifiers) and may define LIKE_LOAD_U32(addr, value) / LIKE_LOAD_U8(addr, value): how a value's bytes are read.
#pragma once
#include <stdint.h>
#include <string.h>
#include "dev_strview.h"

#ifndef LIKE_LOAD_U32
#define LIKE_LOAD_U32(addr, value) (*(const uint32_t*)(addr))
#define LIKE_LOAD_U8(addr, value) (*(const uint8_t*)(addr))
#endif

constexpr int LIKE_MAX_PATTERN = 255, LIKE_MAX_SEGMENTS = 16;

// The parsed pattern. `bytes` holds the segments' bytes back to back (a `_` holds 0), `under` one bit per byte ("is `_`").
struct LikeTable {
  uint32_t bytes[64];
  uint32_t under[8];
  uint8_t seg_off[LIKE_MAX_SEGMENTS + 1];   // segment s is bytes[seg_off[s] .. seg_off[s + 1])
  uint8_t nseg, anchor_start, anchor_end, kind;
  uint32_t min_len;                         // sum of the segments' lengths: every byte and every `_` needs at least one byte
};

// ---- host: pattern -> table ------------------------------------------------------------------------------------------------------
// `literal`: a needle, no wildcard and no escape. Returns DBHIP_OK, or the error code with *why set; no message names a constant
// of the group (tests/test_abi.py).
inline int32_t like_parse(const uint8_t* pat, int32_t len, int32_t escape, bool literal, LikeTable* t, const char** why) {
  memset(t, 0, sizeof(*t));
  if (len < 0 || (len > 0 && !pat)) { *why = "NULL pattern or a negative length"; return DBHIP_ERR_INVALID; }
  if (escape < -1 || escape > 255) { *why = "the escape must be a byte or -1"; return DBHIP_ERR_INVALID; }
  if (len > LIKE_MAX_PATTERN) { *why = "a pattern of more than 255 bytes: keep the CPU closure"; return DBHIP_ERR_UNSUPPORTED; }
  uint8_t* b = (uint8_t*)t->bytes;
  int nb = 0, nseg = 0;
  bool open = false, any_under = false, first_pct = false, last_pct = false;
  for (int i = 0; i < len; ++i) {
    uint8_t c = pat[i];
    bool lit = literal;
    if (!literal && escape >= 0 && c == (uint8_t)escape && i + 1 < len) { c = pat[++i]; lit = true; }
    else if (!literal && escape >= 0 && c == (uint8_t)escape) lit = true;     // a trailing lone escape is itself a literal
    if (!lit && c == '%') {
      if (open) { t->seg_off[++nseg] = (uint8_t)nb; open = false; }
      if (nb == 0 && nseg == 0) first_pct = true;
      last_pct = true;
      continue;
    }
    last_pct = false;
    if (!open) {
      if (nseg == LIKE_MAX_SEGMENTS) { *why = "more than 16 segments: keep the CPU closure"; return DBHIP_ERR_UNSUPPORTED; }
      open = true;
      t->seg_off[nseg] = (uint8_t)nb;
    }
    if (!lit && c == '_') { t->under[nb >> 5] |= 1u << (nb & 31); b[nb++] = 0; any_under = true; }
    else b[nb++] = c;
  }
  if (open) t->seg_off[++nseg] = (uint8_t)nb;
  t->nseg = (uint8_t)nseg;
  t->anchor_start = !first_pct;
  t->anchor_end = !last_pct;
  t->min_len = (uint32_t)nb;
  if (nseg == 1 && !any_under)
    t->kind = t->anchor_start ? (t->anchor_end ? DBHIP_LIKE_EQUALS : DBHIP_LIKE_PREFIX) : (t->anchor_end ? DBHIP_LIKE_SUFFIX : DBHIP_LIKE_CONTAINS);
  else
    t->kind = DBHIP_LIKE_SEGMENTS;
  return DBHIP_OK;
}

// dbhip_str_match's table: the needle as ONE literal segment of the given kind. An empty needle has no segment: equal to the empty value
// only, a prefix / suffix / part of every value.
inline int32_t like_parse_needle(int32_t kind, const uint8_t* needle, int32_t len, LikeTable* t, const char** why) {
  if (kind < DBHIP_LIKE_EQUALS || kind > DBHIP_LIKE_CONTAINS) { *why = "the kind must be one of the four literal kinds"; return DBHIP_ERR_INVALID; }
  const int32_t rc = like_parse(needle, len, -1, true, t, why);
  if (rc) return rc;
  t->anchor_start = kind == DBHIP_LIKE_EQUALS || (kind == DBHIP_LIKE_PREFIX && t->nseg);
  t->anchor_end = kind == DBHIP_LIKE_EQUALS || (kind == DBHIP_LIKE_SUFFIX && t->nseg);
  t->kind = t->nseg ? (uint8_t)kind : (uint8_t)DBHIP_LIKE_SEGMENTS;
  return DBHIP_OK;
}

// ---- the value -------------------------------------------------------------------------------------------------------------------
LIKE_FN bool is_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }
LIKE_FN uint32_t low_mask(uint32_t nbytes) { return nbytes >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nbytes)) - 1u); }

// One value of pass 1: its length, the view's three payload words, and for a value of more than 12 bytes its first byte's address.
// byte(): inline values from the registers (selected, not indexed); long ones through the last aligned word read.
struct LaneValue {
  uint32_t len, w1, w2, w3;
  uintptr_t base;
  uintptr_t cached_at;
  uint32_t cached;
  LIKE_FN bool is_inline() const { return sv_is_inline(len); }
  LIKE_FN uint32_t load(uintptr_t a) const { return LIKE_LOAD_U32(a, *this); }   // a is a multiple of 4 and the word holds a byte of the value
  // four value bytes from position `pos` of an inline value (bytes past the view's 12 read as 0)
  LIKE_FN uint32_t inline_word(uint32_t pos) const {
    const uint32_t k = pos >> 2, sh = (pos & 3) * 8;
    const uint32_t lo = k == 0 ? w1 : (k == 1 ? w2 : (k == 2 ? w3 : 0u));
    const uint32_t hi = k == 0 ? w2 : (k == 1 ? w3 : 0u);
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
  }
  LIKE_FN uint32_t byte(uint32_t pos) {   // pos < len
    if (is_inline()) return inline_word(pos) & 0xFFu;
    const uintptr_t a = base + pos, a0 = a & ~(uintptr_t)3;
    if (a0 != cached_at) { cached = load(a0); cached_at = a0; }
    return (cached >> (8 * (uint32_t)(a & 3))) & 0xFFu;
  }
};

// A listed row of pass 2: always longer than 12 bytes. Neighbouring lanes read neighbouring bytes.
struct WaveValue {
  uint32_t len;
  const uint8_t* base;
  LIKE_FN uint32_t byte(uint32_t pos) const { return LIKE_LOAD_U8(base + pos, *this); }
};

// value bytes [pos, pos + cnt) against the needle's bytes [noff, noff + cnt); noff is a multiple of 4, the range lies inside the value
LIKE_FN bool like_cmp_range(const LaneValue& v, const uint32_t* s_words, uint32_t pos, uint32_t noff, uint32_t cnt) {
  if (v.is_inline()) {
    for (uint32_t i = 0; i < cnt; i += 4) {
      const uint32_t m = low_mask(cnt - i);
      if ((v.inline_word(pos + i) ^ s_words[(noff + i) >> 2]) & m) return false;
    }
    return true;
  }
  const uintptr_t a = v.base + pos;
  uintptr_t p = a & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)(a & 3) * 8, have = 4 - (uint32_t)(a & 3);   // value bytes the word at p still holds
  uint32_t cur = v.load(p);
  for (uint32_t i = 0; i < cnt; i += 4) {
    const uint32_t rem = cnt - i;
    const uint32_t nxt = rem > have ? v.load(p + 4) : 0u;           // (read only when one of its bytes is compared)
    const uint32_t w = sh ? ((cur >> sh) | (nxt << (32 - sh))) : cur;
    if ((w ^ s_words[(noff + i) >> 2]) & low_mask(rem)) return false;
    cur = nxt;
    p += 4;
  }
  return true;
}

// leftmost occurrence test: does the needle (m bytes, m >= 1) occur in the value? (pass 1: len <= DBHIP_LIKE_LONG_BYTES)
LIKE_FN bool like_contains(const LaneValue& v, const uint32_t* s_words, uint32_t m) {
  const uint32_t nm = low_mask(m), n0 = s_words[0] & nm;
  if (v.is_inline()) {
    for (uint32_t pos = 0; pos + m <= v.len; ++pos)
      if ((v.inline_word(pos) & nm) == n0 && (m <= 4 || like_cmp_range(v, s_words, pos + 4, 4, m - 4))) return true;
    return false;
  }
  // sliding window over the aligned words of the value: `cur` is the word at p, `nxt` the one behind it (0 past the value's last word)
  const uintptr_t a = v.base, end = v.base + v.len;
  uintptr_t p = a & ~(uintptr_t)3;
  uint32_t cur = v.load(p);
  for (; p < end; p += 4) {
    const uint32_t nxt = p + 4 < end ? v.load(p + 4) : 0u;
    const uint64_t w = ((uint64_t)nxt << 32) | cur;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t pos = (int64_t)(p + j) - (int64_t)a;     // bytes in front of the value and candidates that would run past it are skipped
      if (pos >= 0 && (uint64_t)pos + m <= v.len && ((uint32_t)(w >> (8 * j)) & nm) == n0 &&
          (m <= 4 || like_cmp_range(v, s_words, (uint32_t)pos + 4, 4, m - 4)))
        return true;
    }
    cur = nxt;
  }
  return false;
}

// One segment (bytes sb[0 .. L), `_` flags su) from `start` forwards; *end = the position behind it.
template <class V>
LIKE_FN bool seg_forward(V& v, const uint8_t* sb, const uint8_t* su, uint32_t L, uint32_t start, bool unit_byte, uint32_t* end) {
  uint32_t p = start;
  for (uint32_t i = 0; i < L; ++i) {
    if (p >= v.len) return false;
    const uint32_t c = v.byte(p);
    if (su[i]) {
      if (!unit_byte) {
        if (p != 0 && is_cont(c)) return false;            // `_` covers one unit: it starts at a unit boundary
        while (p + 1 < v.len && is_cont(v.byte(p + 1))) ++p;
      }
    } else if (c != sb[i]) return false;
    ++p;
  }
  *end = p;
  return true;
}

// The same segment backwards from `stop` (the position behind its last byte); *start = its first position.
template <class V>
LIKE_FN bool seg_backward(V& v, const uint8_t* sb, const uint8_t* su, uint32_t L, uint32_t stop, bool unit_byte, uint32_t* start) {
  uint32_t p = stop;
  for (uint32_t i = L; i-- > 0;) {
    if (p == 0) return false;
    if (su[i]) {
      if (!unit_byte) {
        if (p < v.len && is_cont(v.byte(p))) return false;  // the unit ends at a boundary
        while (p - 1 > 0 && is_cont(v.byte(p - 1))) --p;    // and begins at the boundary before it
      }
    } else if (v.byte(p - 1) != sb[i]) return false;
    --p;
  }
  *start = p;
  return true;
}

struct LikeShared {
  uint32_t words[64];      // the segments' bytes (read as words by the literal kinds)
  uint8_t under[256];
  uint8_t seg_off[LIKE_MAX_SEGMENTS + 1];
};

// SEGMENTS for one lane's value (pass 1)
LIKE_FN bool like_segments_lane(LaneValue& v, const LikeShared& S, uint32_t nseg, bool a_start, bool a_end, bool unit_byte) {
  const uint8_t* sb = (const uint8_t*)S.words;
  uint32_t pos = 0, tail = v.len, first = 0, last = nseg;
  if (a_start) {
    if (!seg_forward(v, sb, S.under, S.seg_off[1], 0, unit_byte, &pos)) return false;
    if (nseg == 1 && a_end) return pos == v.len;
    first = 1;
  }
  if (a_end) {
    const uint32_t o = S.seg_off[nseg - 1];
    if (!seg_backward(v, sb + o, S.under + o, S.seg_off[nseg] - o, v.len, unit_byte, &tail)) return false;
    last = nseg - 1;
  }
  for (uint32_t s = first; s < last; ++s) {
    const uint32_t o = S.seg_off[s], L = S.seg_off[s + 1] - o;
    bool found = false;
    for (uint32_t st = pos; st + L <= tail; ++st) {
      uint32_t e;
      if (seg_forward(v, sb + o, S.under + o, L, st, unit_byte, &e)) { pos = e; found = true; break; }
    }
    if (!found) return false;
  }
  return pos <= tail;
}

// Pass 1's decision for one usable, non-NULL value; *listed = the value is left to pass 2 (the result is then meaningless).
LIKE_FN bool like_lane_decide(LaneValue& v, const LikeShared& S, uint32_t kind, uint32_t nseg, uint32_t m, bool a_start, bool a_end,
                              bool unit_byte, bool* listed) {
  if (v.len < m) return false;                  // a shorter value cannot match: every pattern byte needs one of its own
  if (nseg == 0) return !a_start || v.len == 0; // the empty pattern / all `%`
  if (kind == DBHIP_LIKE_EQUALS || kind == DBHIP_LIKE_PREFIX) {
    if (kind == DBHIP_LIKE_EQUALS && v.len != m) return false;
    if ((v.w1 ^ S.words[0]) & low_mask(m)) return false;      // the view's first word holds bytes 0..3 of any value, inline or not
    return m <= 4 || like_cmp_range(v, S.words, 4, 4, m - 4);
  }
  if (kind == DBHIP_LIKE_SUFFIX) return like_cmp_range(v, S.words, v.len - m, 0, m);
  if (v.len > DBHIP_LIKE_LONG_BYTES) { *listed = true; return false; }
  if (kind == DBHIP_LIKE_CONTAINS) return like_contains(v, S.words, m);
  return like_segments_lane(v, S, nseg, a_start, a_end, unit_byte);
}
