// dev_strsearch.h — the row-level logic of the String search and rewrite functions (include/dbhip.h a28): find-from, the greedy
// occurrence walk, the field range of split_part, the result length of every rewrite and the bytes of a rewritten value. Free of HIP
// and built on dev_strfn.h (SfValue, sf_forward, sf_units, sf_slice_view, SfInlineSink), so that a host program compiles the very same
// text (tests/strsearch_host_check.cpp). Everything works on byte POSITIONS of one value and reads a byte only below the value's
// length, through SfValue::byte.
// The constants of a call (needle / from / to / pad / delimiter) are SsConst: prepared once on the host, carried by value in the kernel
// arguments, staged in LDS.
#pragma once
#include "dev_strfn.h"

// the op codes are the public ones (k_strsearch.hip asserts it)
enum { SS_REPLACE = 0, SS_LPAD = 1, SS_RPAD = 2, SS_REPEAT = 3, SS_REVERSE = 4, SS_OP_COUNT = 5 };
constexpr int SS_MAX_CONST = 255;
constexpr uint32_t SS_NONE = 0xFFFFFFFFu;         // no occurrence (an occurrence starts below 2^32 - 1)
constexpr uint64_t SS_TOO_LONG = ~0ull;           // a result of more than 2^32 - 1 bytes

// x: needle / from / pad / delimiter, y: to. xu[u] is where unit u of x starts (xu[x_units] = x_len): the pad's own units.
struct SsConst {
  uint32_t x_len, y_len, x_units, _pad;
  uint8_t x[256], y[256], xu[256];
};
SF_FN void ss_prepare(SsConst& C, const uint8_t* x, uint32_t x_len, const uint8_t* y, uint32_t y_len, bool unit_byte) {   // lengths <= 255
  C.x_len = x_len; C.y_len = y_len; C.x_units = 0; C._pad = 0;
  for (uint32_t i = 0; i < 256; ++i) { C.x[i] = i < x_len ? x[i] : 0; C.y[i] = i < y_len ? y[i] : 0; C.xu[i] = 0; }
  for (uint32_t i = 0; i < x_len; ++i)
    if (i == 0 || unit_byte || !sf_is_cont(x[i])) C.xu[C.x_units++] = (uint8_t)i;
  C.xu[C.x_units] = (uint8_t)x_len;
}

// ---- find-from and the occurrence walk ---------------------------------------------------------------------------------------------------
// the smallest p >= from with value[p .. p + m) == nd (m >= 1), SS_NONE when there is none
SF_FN uint32_t ss_find_from(SfValue& v, uint32_t from, const uint8_t* nd, uint32_t m) {
  if (m > v.len) return SS_NONE;
  for (uint32_t p = from; p <= v.len - m; ++p) {
    uint32_t i = 0;
    while (i < m && v.byte(p + i) == nd[i]) ++i;
    if (i == m) return p;
  }
  return SS_NONE;
}
// the number of greedy left-to-right non-overlapping occurrences (m >= 1)
SF_FN uint32_t ss_count(SfValue& v, const uint8_t* nd, uint32_t m) {
  uint32_t c = 0, at = 0;
  for (;;) {
    const uint32_t p = ss_find_from(v, at, nd, m);
    if (p == SS_NONE) return c;
    ++c;
    at = p + m;
  }
}
// the boundaries q with 0 < q <= p (p < len): the unit index of position p
SF_FN uint32_t ss_bounds_upto(SfValue& v, uint32_t p) {
  uint32_t c = 0;
  for (uint32_t q = 1; q <= p; ++q) c += sf_is_cont(v.byte(q)) ? 0u : 1u;
  return c;
}

// ---- position ------------------------------------------------------------------------------------------------------------------------------
// may this start find anything at all? (decided before any arithmetic: every i64 is defined; U <= len)
SF_FN bool ss_start_possible(int64_t s, uint32_t len) { return s >= 1 && s - 1 <= (int64_t)len; }
// does the answer need the value's bytes? (a lane may not look when the value is longer than SF_LONG_BYTES)
SF_FN bool ss_position_walks(uint32_t len, uint32_t m, int64_t s, bool unit_byte) {
  return ss_start_possible(s, len) && (m > 0 ? m <= len : (!unit_byte && s > 1));
}
SF_FN bool ss_split_walks(uint32_t len, uint32_t m) { return m > 0 && m <= len; }
SF_FN uint64_t ss_position(SfValue& v, const uint8_t* nd, uint32_t m, int64_t s, bool unit_byte) {
  if (!ss_start_possible(s, v.len)) return 0;
  const uint32_t k = (uint32_t)(s - 1);                  // units to skip, <= len
  if (m == 0) return (k == 0 || k <= (unit_byte ? v.len : sf_units(v))) ? (uint64_t)s : 0;
  if (m > v.len) return 0;
  // (a start past the last unit lands on len, where a needle of one byte or more is not found: the same 0)
  const uint32_t b = k == 0 ? 0 : sf_forward(v, 0, k, unit_byte);
  const uint32_t p = ss_find_from(v, b, nd, m);
  if (p == SS_NONE) return 0;
  return 1 + (uint64_t)(unit_byte ? p : ss_bounds_upto(v, p));
}

// ---- split_part ------------------------------------------------------------------------------------------------------------------------------
// which field a part asks for, once the number of occurrences is known where it is needed: 0 = none, else the 1-based field index
SF_FN bool ss_part_from_end(int64_t part) { return part < 0; }
SF_FN uint64_t ss_field_index(int64_t part, uint32_t c) {      // part < 0: c occurrences, c + 1 fields
  if (part >= 0) return part == 0 ? 1 : (uint64_t)part;
  if (part < -(int64_t)((uint64_t)c + 1)) return 0;
  return (uint64_t)((int64_t)c + 2 + part);
}
// the byte range of field k (k >= 1) of the fields between the occurrences of nd (m >= 1); false when the list is shorter
SF_FN bool ss_field(SfValue& v, const uint8_t* nd, uint32_t m, uint64_t k, uint32_t* s, uint32_t* e) {
  uint32_t fs = 0;
  for (uint64_t idx = 1;; ++idx) {
    const uint32_t p = ss_find_from(v, fs, nd, m);
    if (idx == k) { *s = fs; *e = p == SS_NONE ? v.len : p; return true; }
    if (p == SS_NONE) return false;
    fs = p + m;
  }
}
SF_FN bool ss_field_range(SfValue& v, const uint8_t* nd, uint32_t m, int64_t part, uint32_t* s, uint32_t* e) {
  *s = 0; *e = 0;
  if (m == 0 || m > v.len) {                              // one field, the whole value
    if (part != 0 && part != 1 && part != -1) return false;
    *e = v.len;
    return true;
  }
  const uint64_t k = ss_field_index(part, ss_part_from_end(part) ? ss_count(v, nd, m) : 0);
  return k != 0 && ss_field(v, nd, m, k, s, e);
}

// ---- the result length of a rewrite ------------------------------------------------------------------------------------------------------
SF_FN uint64_t ss_checked(uint64_t total) { return total > 0xFFFFFFFFull ? SS_TOO_LONG : total; }
SF_FN bool ss_replace_walks(const SsConst& C, uint32_t len) { return C.x_len > 0 && C.x_len <= len; }     // else the value unchanged
SF_FN uint64_t ss_replace_len(const SsConst& C, uint32_t len, uint32_t c) {    // c <= len / x_len: no product leaves 2^40
  return ss_checked((uint64_t)len - (uint64_t)c * C.x_len + (uint64_t)c * C.y_len);
}
SF_FN uint64_t ss_repeat_len(uint32_t len, int64_t k) {
  if (k <= 0 || len == 0) return 0;
  if (k > (int64_t)(0xFFFFFFFFu / len)) return SS_TOO_LONG;
  return (uint64_t)len * (uint64_t)k;
}
// the bytes of F fill units taken cyclically from the pad's units (x_units >= 1, F < 2^32)
SF_FN uint64_t ss_fill_bytes(const SsConst& C, uint32_t F) { return (uint64_t)(F / C.x_units) * C.x_len + C.xu[F % C.x_units]; }
// LPAD / RPAD with the value's unit count U at hand: *cut is set when the result is the value's first L units (L <= U, the caller walks
// to them); otherwise the result's length
SF_FN uint64_t ss_pad_len(const SsConst& C, uint32_t len, uint32_t U, int64_t L, bool* cut) {
  *cut = false;
  if (L <= 0) return 0;
  if (L <= (int64_t)U) { *cut = true; return 0; }
  if (C.x_len == 0) return 0;
  if (L > 0xFFFFFFFFll) return SS_TOO_LONG;              // a unit is a byte or more
  return ss_checked((uint64_t)len + ss_fill_bytes(C, (uint32_t)(L - U)));
}
// does the length need the value's bytes? (a lane may not look when the value is longer than SF_LONG_BYTES)
SF_FN bool ss_len_walks(int32_t op, const SsConst& C, uint32_t len, int64_t k, bool unit_byte) {
  if (op == SS_REPLACE) return ss_replace_walks(C, len);
  if (op == SS_LPAD || op == SS_RPAD) return !unit_byte && k > 0;
  return false;
}
SF_FN uint64_t ss_rewrite_len(int32_t op, SfValue& v, int64_t k, const SsConst& C, bool unit_byte) {
  if (op == SS_REPLACE) return ss_replace_walks(C, v.len) ? ss_replace_len(C, v.len, ss_count(v, C.x, C.x_len)) : v.len;
  if (op == SS_LPAD || op == SS_RPAD) {
    if (k <= 0) return 0;
    bool cut;
    const uint64_t total = ss_pad_len(C, v.len, unit_byte ? v.len : sf_units(v), k, &cut);
    return cut ? sf_forward(v, 0, (uint32_t)k, unit_byte) : total;
  }
  if (op == SS_REPEAT) return ss_repeat_len(v.len, k);
  return v.len;                                            // REVERSE
}

// ---- the bytes of a rewrite -------------------------------------------------------------------------------------------------------------
// Sends the `total` bytes of the result (what ss_rewrite_len gave, not SS_TOO_LONG), in order, to sink.put(position, byte).
template <class Sink>
SF_FN void ss_emit(int32_t op, SfValue& v, const SsConst& C, uint32_t total, bool unit_byte, Sink& sink) {
  uint32_t at = 0;
  if (op == SS_REPLACE) {
    uint32_t pos = 0;
    if (ss_replace_walks(C, v.len)) {
      for (;;) {
        const uint32_t p = ss_find_from(v, pos, C.x, C.x_len);
        if (p == SS_NONE) break;
        while (pos < p) sink.put(at++, v.byte(pos++));
        for (uint32_t i = 0; i < C.y_len; ++i) sink.put(at++, C.y[i]);
        pos = p + C.x_len;
      }
    }
    while (pos < v.len) sink.put(at++, v.byte(pos++));
  } else if (op == SS_LPAD || op == SS_RPAD) {
    // longer than the value: the fill is total - len bytes, whole pads and then the pad's prefix; else the value's first `total` bytes
    const uint32_t fill = total > v.len ? total - v.len : 0, body = total - fill;
    if (op == SS_LPAD)
      for (uint32_t j = 0; j < fill; ++j) sink.put(at++, C.x[j % C.x_len]);
    for (uint32_t j = 0; j < body; ++j) sink.put(at++, v.byte(j));
    if (op == SS_RPAD)
      for (uint32_t j = 0; j < fill; ++j) sink.put(at++, C.x[j % C.x_len]);
  } else if (op == SS_REPEAT) {
    for (uint32_t j = 0, i = 0; j < total; ++j) {
      sink.put(at++, v.byte(i));
      if (++i == v.len) i = 0;
    }
  } else if (unit_byte) {
    for (uint32_t j = 0; j < total; ++j) sink.put(at++, v.byte(v.len - 1 - j));
  } else {
    for (uint32_t e = v.len; e > 0;) {                     // the units from the last to the first, each in its own order
      uint32_t a = e - 1;
      while (a > 0 && sf_is_cont(v.byte(a))) --a;
      for (uint32_t i = a; i < e; ++i) sink.put(at++, v.byte(i));
      e = a;
    }
  }
}
