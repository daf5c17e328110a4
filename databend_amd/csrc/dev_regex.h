// dev_regex.h — the row walk of k_regex.hip (include/dbhip.h a25), free of HIP so that a host program runs the very same steps with
// checked loads (tests/regex_host_check.cpp). The includer defines REGEX_FN (the functions' qualifiers) and has included
// include/dbhip.h. The value is like_match.h's LaneValue: an inline value is walked from the view's registers, a longer one through
// LaneValue::load, the naturally aligned 4-byte read that covers at least one byte of the value (LIKE_LOAD_U32 for a checking host).
#pragma once
#include <stdint.h>
#ifndef LIKE_FN
#define LIKE_FN REGEX_FN
#endif
#include "like_match.h"

constexpr uint32_t REGEX_ACCEPT_END = 1, REGEX_STICKY = 2, REGEX_DEAD = 4;         // regex_compile.h's state flags
constexpr uint32_t REGEX_NO = 0, REGEX_YES = 1, REGEX_DECLINED = 2;                // regex_walk's answers

// The compiled pattern as the walk reads it (in LDS on the device): table[state * n_classes + cmap[byte]] is the next state.
struct RegexTables {
  const uint16_t* table;
  const uint8_t* flags;
  const uint8_t* cmap;
  uint32_t n_classes;
  uint32_t needs_ascii;
};

// bytes [first, first + cnt) of the word `w`, cnt >= 1 and first + cnt <= 4: the state after them, and their high bits into *high
REGEX_FN uint32_t regex_step_word(const RegexTables& R, uint32_t state, uint32_t w, uint32_t first, uint32_t cnt, uint32_t* high) {
  w >>= 8 * first;
  *high |= w & low_mask(cnt) & 0x80808080u;
  for (uint32_t j = 0; j < cnt; ++j) {
    state = R.table[state * R.n_classes + R.cmap[w & 0xFFu]];
    w >>= 8;
  }
  return state;
}

// One usable, non-NULL value. The walk goes word by word and stops at a sticky or a dead state (both are absorbing, so looking once a
// word is exact). A pattern that needs ASCII rows reads on — only the words' high bits by then — and declines the row at the first byte
// above 7F, wherever it lies.
REGEX_FN uint32_t regex_walk(const LaneValue& v, const RegexTables& R) {
  uint32_t state = 0, high = 0;
  bool settled = (R.flags[0] & (REGEX_STICKY | REGEX_DEAD)) != 0;
  if (!(settled && !R.needs_ascii)) {
    if (v.is_inline()) {
      for (uint32_t pos = 0; pos < v.len; pos += 4) {
        const uint32_t w = pos == 0 ? v.w1 : (pos == 4 ? v.w2 : v.w3);
        const uint32_t cnt = v.len - pos < 4 ? v.len - pos : 4;
        if (settled) high |= w & low_mask(cnt) & 0x80808080u;
        else state = regex_step_word(R, state, w, 0, cnt, &high);
        settled = (R.flags[state] & (REGEX_STICKY | REGEX_DEAD)) != 0;
        if (R.needs_ascii ? high != 0 : settled) break;
      }
    } else {
      uintptr_t p = v.base & ~(uintptr_t)3;
      uint32_t first = (uint32_t)(v.base & 3), left = v.len;
      while (left) {
        const uint32_t w = v.load(p);
        const uint32_t cnt = left < 4 - first ? left : 4 - first;
        if (settled) high |= (w >> (8 * first)) & low_mask(cnt) & 0x80808080u;
        else state = regex_step_word(R, state, w, first, cnt, &high);
        settled = (R.flags[state] & (REGEX_STICKY | REGEX_DEAD)) != 0;
        if (R.needs_ascii ? high != 0 : settled) break;
        left -= cnt;
        first = 0;
        p += 4;
      }
    }
  }
  if (R.needs_ascii && high) return REGEX_DECLINED;
  return (R.flags[state] & REGEX_ACCEPT_END) ? REGEX_YES : REGEX_NO;
}
