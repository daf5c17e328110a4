// dev_strcast.h — the row-level logic of the String casts (include/dbhip.h a24): the whitespace trim, the four parsers (integers,
// decimals, dates, timestamps) and the digit generation of the format side. Free of HIP, in the style of dev_strfn.h, so that a host
// program compiles the very same text (tests/strcast_host_check.cpp). SC_FN is the functions' qualifier: an includer may define it.
// Value bytes are read through SfValue::byte (dev_strfn.h: naturally aligned 4-byte loads that each cover a byte of the value); the
// calendar is dev_datetime.h's. Every parser decides by comparisons BEFORE it does arithmetic: an accumulator takes another digit only
// when the comparison has shown that the result stays below the limit, so nothing wraps on any byte string. The format side builds
// the text in eleven 32-bit words that are indexed by constants only (they stay in registers): a zero-padded digit string of fixed
// width, then the point inserted by masks, then one barrel shift that drops the leading zeros.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif
#include "dev_datetime.h"
#include "dev_strfn.h"

#if !defined(SC_FN) && (defined(__HIP__) || defined(__HIPCC_RTC__))
#define SC_FN __host__ __device__ __forceinline__
#elif !defined(SC_FN)
#define SC_FN inline
#endif

// the type codes are the public ones (k_strcast.hip asserts it)
enum { SC_T_BOOL = 1, SC_T_I8 = 2, SC_T_I16 = 3, SC_T_I32 = 4, SC_T_I64 = 5, SC_T_U8 = 6, SC_T_U16 = 7, SC_T_U32 = 8, SC_T_U64 = 9,
       SC_T_F32 = 10, SC_T_F64 = 11, SC_T_DATE = 12, SC_T_TIMESTAMP = 13, SC_T_DEC64 = 14, SC_T_DEC128 = 15, SC_T_STRING = 16, SC_T_DEC256 = 17 };
enum { SC_OK = 0, SC_ERROR = 1, SC_DECLINED = 2 };
constexpr uint32_t SC_MAX_BYTES = 256;     // a longer value is declined unread
constexpr uint32_t SC_TEXT_WORDS = 11;     // 41 bytes: '-', 39 digits, '.'
constexpr uint32_t SC_TEXT_MAX = 41;
typedef unsigned __int128 sc_u128;

SC_FN bool sc_is_int(int t) { return t >= SC_T_I8 && t <= SC_T_U64; }
SC_FN bool sc_is_signed(int t) { return t >= SC_T_I8 && t <= SC_T_I64; }
SC_FN bool sc_supported(int t) { return sc_is_int(t) || (t >= SC_T_DATE && t <= SC_T_DEC128); }
SC_FN uint32_t sc_type_bytes(int t) {
  return (t == SC_T_I8 || t == SC_T_U8) ? 1u : (t == SC_T_I16 || t == SC_T_U16) ? 2u : (t == SC_T_I32 || t == SC_T_U32 || t == SC_T_DATE) ? 4u
       : t == SC_T_DEC128 ? 16u : 8u;
}
// the largest value of an integer type
SC_FN uint64_t sc_int_max(int t) {
  switch (t) {
    case SC_T_I8: return 0x7Fu;
    case SC_T_I16: return 0x7FFFu;
    case SC_T_I32: return 0x7FFFFFFFu;
    case SC_T_I64: return 0x7FFFFFFFFFFFFFFFull;
    case SC_T_U8: return 0xFFu;
    case SC_T_U16: return 0xFFFFu;
    case SC_T_U32: return 0xFFFFFFFFu;
    default: return 0xFFFFFFFFFFFFFFFFull;
  }
}

struct ScSpec {
  int32_t type;
  uint32_t precision, scale;   // decimals
  int32_t rounding;            // decimals: round half away from zero instead of truncating
  int32_t offset_s;            // timestamps
};

SC_FN bool sc_is_space(uint32_t c) { return c == 0x20u || (c - 0x09u) <= 4u; }
SC_FN bool sc_is_digit(uint32_t c) { return (c - 0x30u) <= 9u; }

// ---- trim ----------------------------------------------------------------------------------------------------------------------------
SC_FN void sc_trim(SfValue& v, uint32_t* s, uint32_t* e) {
  uint32_t lo = 0, hi = v.len;
  while (lo < hi && sc_is_space(v.byte(lo))) ++lo;
  while (hi > lo && sc_is_space(v.byte(hi - 1))) --hi;
  *s = lo; *e = hi;
}
SC_FN bool sc_all_digits(SfValue& v, uint32_t s, uint32_t e) {   // and at least one
  for (uint32_t p = s; p < e; ++p)
    if (!sc_is_digit(v.byte(p))) return false;
  return e > s;
}

// ---- integers: [+-]? [0-9]+ -----------------------------------------------------------------------------------------------------------
// what does not match: declined when it holds '.', 'e' or 'E' and otherwise only digits and signs, else the row error
SC_FN int sc_int_mismatch(SfValue& v, uint32_t s, uint32_t e) {
  bool mark = false;
  for (uint32_t p = s; p < e; ++p) {
    const uint32_t c = v.byte(p);
    if (c == '.' || c == 'e' || c == 'E') mark = true;
    else if (!sc_is_digit(c) && c != '+' && c != '-') return SC_ERROR;
  }
  return mark ? SC_DECLINED : SC_ERROR;
}
// *out: the value's two's complement image in 64 bits
SC_FN int sc_parse_int(SfValue& v, uint32_t s, uint32_t e, int type, uint64_t* out) {
  *out = 0;
  if (s == e) return SC_ERROR;
  uint32_t p = s;
  const uint32_t c0 = v.byte(p);
  const bool neg = c0 == '-';
  if (neg || c0 == '+') ++p;
  if (p == e) return sc_int_mismatch(v, s, e);
  const uint64_t lim = sc_int_max(type) + ((neg && sc_is_signed(type)) ? 1u : 0u);     // the largest magnitude (a signed max + 1 does not wrap)
  const uint64_t lim10 = lim / 10u, limd = lim - lim10 * 10u;
  uint64_t acc = 0;
  bool over = false;
  for (; p < e; ++p) {
    const uint32_t c = v.byte(p);
    if (!sc_is_digit(c)) return sc_int_mismatch(v, s, e);
    const uint32_t d = c - 0x30u;
    if (acc > lim10 || (acc == lim10 && d > limd)) over = true;     // decided before the multiply; once over, acc stays where it is
    else acc = acc * 10u + d;
  }
  if (neg && !sc_is_signed(type)) return SC_ERROR;                   // "-0" included
  if (over) return SC_ERROR;                                         // number overflowed
  *out = neg ? (uint64_t)0 - acc : acc;
  return SC_OK;
}

// ---- decimals: [+-]? [0-9]* ( . [0-9]* )?, at least one digit ---------------------------------------------------------------------------
// U: uint64_t for precision <= 18, sc_u128 for precision <= 38. *mag: |value| at the target scale, below 10^precision
template <class U>
SC_FN int sc_parse_decimal(SfValue& v, uint32_t s, uint32_t e, uint32_t precision, uint32_t scale, bool rounding, U* mag, bool* negative) {
  *mag = 0; *negative = false;
  if (s == e) return SC_ERROR;
  U lim1 = 1;                                     // 10^(precision - 1): an accumulator below it can take another digit
  for (uint32_t k = 1; k < precision; ++k) lim1 *= 10u;
  uint32_t p = s;
  const uint32_t c0 = v.byte(p);
  const bool neg = c0 == '-';
  if (neg || c0 == '+') ++p;
  U acc = 0;
  bool over = false, round_up = false;
  uint32_t digits = 0, frac = 0;
  for (; p < e; ++p) {
    const uint32_t c = v.byte(p);
    if (!sc_is_digit(c)) break;
    ++digits;
    if (acc >= lim1) over = true;                 // sticky; acc * 10 + d stays below 10^precision otherwise
    else acc = acc * 10u + (c - 0x30u);
  }
  if (p < e && v.byte(p) == '.') {
    for (++p; p < e; ++p) {
      const uint32_t c = v.byte(p);
      if (!sc_is_digit(c)) break;
      ++digits;
      if (frac < scale) {
        if (acc >= lim1) over = true;
        else acc = acc * 10u + (c - 0x30u);
      } else if (frac == scale) {
        round_up = c >= 0x35u;                    // the first digit that is cut decides; the ones behind it only have to be digits
      }
      if (frac <= scale) ++frac;
    }
  }
  if (digits == 0) return SC_ERROR;
  if (p < e) { const uint32_t c = v.byte(p); return (c == 'e' || c == 'E') ? SC_DECLINED : SC_ERROR; }
  for (uint32_t k = frac < scale ? frac : scale; k < scale; ++k) {      // the fraction digits that were not written
    if (acc >= lim1) over = true;
    else acc = acc * 10u;
  }
  if (rounding && round_up && !over) {
    acc += 1u;                                    // acc < 10^precision: no wrap
    if (acc >= lim1 * 10u) over = true;           // the carry left the precision
  }
  if (over) return SC_ERROR;                      // Decimal overflow
  *mag = acc;
  *negative = neg && acc != 0;
  return SC_OK;
}

// ---- dates and timestamps -------------------------------------------------------------------------------------------------------------
// Y{4}-M{1,2}-D{1,2} from *p on; false when the bytes are not of that form (*p is then wherever the match ended)
SC_FN bool sc_date_form(SfValue& v, uint32_t* pp, uint32_t e, uint32_t* y, uint32_t* m, uint32_t* d) {
  uint32_t p = *pp;
  if (e - p < 8) return false;
  uint32_t yy = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t c = v.byte(p + k);
    if (!sc_is_digit(c)) return false;
    yy = yy * 10u + (c - 0x30u);
  }
  p += 4;
  uint32_t part[2] = {0, 0};
  for (uint32_t k = 0; k < 2; ++k) {
    if (p >= e || v.byte(p) != '-') return false;
    ++p;
    if (p >= e || !sc_is_digit(v.byte(p))) return false;
    uint32_t x = v.byte(p++) - 0x30u;
    if (p < e && sc_is_digit(v.byte(p))) x = x * 10u + (v.byte(p++) - 0x30u);
    if (k == 0) part[0] = x; else part[1] = x;
  }
  *y = yy; *m = part[0]; *d = part[1]; *pp = p;
  return true;
}
SC_FN bool sc_date_valid(uint32_t y, uint32_t m, uint32_t d) { return y >= 1u && y <= 9999u && m >= 1u && m <= 12u && d >= 1u && d <= dt_month_days(y, m); }
// two digits at p (p + 2 <= e is checked here)
SC_FN bool sc_two_digits(SfValue& v, uint32_t p, uint32_t e, uint32_t* x) {
  if (e - p < 2 || p > e) return false;
  const uint32_t a = v.byte(p), b = v.byte(p + 1);
  if (!sc_is_digit(a) || !sc_is_digit(b)) return false;
  *x = (a - 0x30u) * 10u + (b - 0x30u);
  return true;
}

SC_FN int sc_parse_date(SfValue& v, uint32_t s, uint32_t e, int32_t* out) {
  *out = 0;
  if (s == e) return SC_ERROR;
  uint32_t p = s, y, m, d;
  if (!sc_date_form(v, &p, e, &y, &m, &d)) return sc_all_digits(v, s, e) ? SC_DECLINED : SC_ERROR;
  if (!sc_date_valid(y, m, d)) return SC_ERROR;
  if (p < e) { const uint32_t c = v.byte(p); return (c == ' ' || c == 'T') ? SC_DECLINED : SC_ERROR; }
  *out = (int32_t)(dt_n_from_civil(y, m, d) - DT_SHIFT);
  return SC_OK;
}

SC_FN int sc_parse_timestamp(SfValue& v, uint32_t s, uint32_t e, int32_t offset_s, int64_t* out) {
  *out = 0;
  if (s == e) return SC_ERROR;
  uint32_t p = s, y, m, d;
  if (!sc_date_form(v, &p, e, &y, &m, &d)) return sc_all_digits(v, s, e) ? SC_DECLINED : SC_ERROR;
  if (!sc_date_valid(y, m, d)) return SC_ERROR;
  uint32_t sod = 0, us = 0;
  int32_t off = offset_s;
  if (p < e && (v.byte(p) == ' ' || v.byte(p) == 'T')) {
    ++p;
    uint32_t hh, mi, ss = 0;
    if (!sc_two_digits(v, p, e, &hh) || e - p < 5 || v.byte(p + 2) != ':' || !sc_two_digits(v, p + 3, e, &mi)) return SC_ERROR;
    p += 5;
    if (p < e && v.byte(p) == ':') {
      if (!sc_two_digits(v, p + 1, e, &ss)) return SC_ERROR;
      p += 3;
      if (p < e && v.byte(p) == '.') {
        ++p;
        uint32_t k = 0;
        for (; p < e && sc_is_digit(v.byte(p)); ++p)
          if (k < 6) { us = us * 10u + (v.byte(p) - 0x30u); ++k; }       // the digits behind the sixth are dropped
        if (k == 0) return SC_ERROR;
        for (; k < 6; ++k) us *= 10u;
      }
    }
    if (hh > 23u || mi > 59u || ss > 59u) return SC_ERROR;
    sod = hh * 3600u + mi * 60u + ss;
  }
  if (p < e) {
    const uint32_t c = v.byte(p);
    if (c == 'Z') {
      off = 0;
      ++p;
    } else if (c == '+' || c == '-') {
      uint32_t zh, zm = 0;
      if (!sc_two_digits(v, p + 1, e, &zh)) return SC_ERROR;
      p += 3;
      if (p < e) {
        if (v.byte(p) == ':') ++p;
        if (!sc_two_digits(v, p, e, &zm)) return SC_ERROR;
        p += 2;
      }
      const uint32_t z = zh * 3600u + zm * 60u;
      if (zm > 59u || z > (uint32_t)DT_MAX_OFFSET_S) return SC_ERROR;
      off = c == '-' ? -(int32_t)z : (int32_t)z;
    }
    if (p != e) return SC_ERROR;
  }
  const int64_t utc = dt_join(dt_n_from_civil(y, m, d), sod, us, off);
  if (utc < DT_TS_MIN || utc > DT_TS_MAX) return SC_ERROR;
  *out = utc;
  return SC_OK;
}

// One value -> its two's complement image (lo, hi; narrower targets take the low bytes). A value longer than SC_MAX_BYTES is declined
// before any of its bytes is read.
SC_FN int sc_parse(SfValue& v, const ScSpec& S, uint64_t* lo, uint64_t* hi) {
  *lo = 0; *hi = 0;
  if (v.len > SC_MAX_BYTES) return SC_DECLINED;
  uint32_t s, e;
  sc_trim(v, &s, &e);
  if (sc_is_int(S.type)) return sc_parse_int(v, s, e, S.type, lo);
  if (S.type == SC_T_DATE) {
    int32_t d;
    const int st = sc_parse_date(v, s, e, &d);
    *lo = (uint64_t)(int64_t)d;
    return st;
  }
  if (S.type == SC_T_TIMESTAMP) {
    int64_t t;
    const int st = sc_parse_timestamp(v, s, e, S.offset_s, &t);
    *lo = (uint64_t)t;
    return st;
  }
  bool neg;
  if (S.type == SC_T_DEC64) {
    uint64_t mag;
    const int st = sc_parse_decimal<uint64_t>(v, s, e, S.precision, S.scale, S.rounding != 0, &mag, &neg);
    *lo = neg ? (uint64_t)0 - mag : mag;
    *hi = neg ? ~(uint64_t)0 : 0;
    return st;
  }
  sc_u128 mag;
  const int st = sc_parse_decimal<sc_u128>(v, s, e, S.precision, S.scale, S.rounding != 0, &mag, &neg);
  const sc_u128 r = neg ? (sc_u128)0 - mag : mag;
  *lo = (uint64_t)r;
  *hi = (uint64_t)(r >> 64);
  return st;
}

// ---- format: digit generation ----------------------------------------------------------------------------------------------------------
// The text of one value: bytes 0 .. len - 1 in w, little-endian, zero behind len.
struct ScText { uint32_t w[SC_TEXT_WORDS]; uint32_t len; };

SC_FN uint32_t sc_dig2(uint32_t x) { const uint32_t a = x / 10u; return a | ((x - a * 10u) << 8); }     // x < 100: two digit VALUES
SC_FN uint32_t sc_dig4(uint32_t x) {                                                                      // x < 10000: four characters
  const uint32_t a = x / 100u;
  return 0x30303030u + (sc_dig2(a) | (sc_dig2(x - a * 100u) << 16));
}
// twenty characters of v, zero padded, into w[0..4]
SC_FN void sc_dig20(uint64_t v, uint32_t* w) {
  const uint64_t top = v / 10000000000000000ull, rest = v - top * 10000000000000000ull;
  const uint32_t mid = (uint32_t)(rest / 100000000u), low = (uint32_t)(rest - (uint64_t)mid * 100000000u);
  const uint32_t m1 = mid / 10000u, l1 = low / 10000u;
  w[0] = sc_dig4((uint32_t)top);
  w[1] = sc_dig4(m1); w[2] = sc_dig4(mid - m1 * 10000u);
  w[3] = sc_dig4(l1); w[4] = sc_dig4(low - l1 * 10000u);
}
// (hi : lo) = q * 10^19 + r for a value of up to 2^127: the value >> 19 is divided by 5^19 (45 bits) in six steps of 19 bits, each a
// 64-bit division by a constant (remainder * 2^19 + 19 bits stays below 5^19 * 2^19 = 10^19 < 2^64). No 128-bit division.
SC_FN void sc_split19(uint64_t hi, uint64_t lo, uint64_t* q, uint64_t* r) {
  constexpr uint64_t D = 19073486328125ull, M = (1u << 19) - 1u;
  const uint64_t n_lo = (lo >> 19) | (hi << 45), n_hi = hi >> 19;
  const uint64_t limb[6] = {n_hi >> 31, (n_hi >> 12) & M, ((n_lo >> 57) | (n_hi << 7)) & M, (n_lo >> 38) & M, (n_lo >> 19) & M, n_lo & M};
  uint64_t rem = 0, quo = 0;
  for (int k = 0; k < 6; ++k) {
    const uint64_t cur = (rem << 19) | limb[k];
    const uint64_t qd = cur / D;
    rem = cur - qd * D;
    quo = (quo << 19) | qd;
  }
  *q = quo;
  *r = lo - quo * 10000000000000000000ull;      // below 10^19: the low 64 bits are the whole of it
}

SC_FN void sc_text_clear(ScText& T) {
  for (uint32_t j = 0; j < SC_TEXT_WORDS; ++j) T.w[j] = 0;
  T.len = 0;
}
// the text moves k bytes towards position 0 (k < 64): six conditional moves by constant distances
SC_FN void sc_text_drop(ScText& T, uint32_t k) {
  for (uint32_t step = 8; step >= 1; step >>= 1)              // whole words: 8, 4, 2, 1
    if (k & (step * 4u))
      for (uint32_t j = 0; j < SC_TEXT_WORDS; ++j) T.w[j] = j + step < SC_TEXT_WORDS ? T.w[j + step] : 0u;
  for (uint32_t b = 2; b >= 1; b >>= 1)                       // bytes: 2, 1
    if (k & b)
      for (uint32_t j = 0; j < SC_TEXT_WORDS; ++j)
        T.w[j] = (T.w[j] >> (8u * b)) | (j + 1 < SC_TEXT_WORDS ? T.w[j + 1] << (32u - 8u * b) : 0u);
}
// byte c is put in front of position `pos`: what lies at or behind it moves one byte up
SC_FN void sc_text_insert(ScText& T, uint32_t pos, uint32_t c) {
  for (uint32_t jj = SC_TEXT_WORDS; jj >= 1; --jj) {
    const uint32_t j = jj - 1;
    const uint32_t moved = (T.w[j] << 8) | (j ? T.w[j - 1] >> 24 : 0u);
    const uint32_t below = pos <= 4u * j ? 0u : (pos >= 4u * j + 4u ? 0xFFFFFFFFu : (1u << (8u * (pos - 4u * j))) - 1u);   // the bytes in front of pos
    uint32_t x = (T.w[j] & below) | (moved & ~below);
    if ((pos >> 2) == j) x = (x & ~(0xFFu << (8u * (pos & 3u)))) | (c << (8u * (pos & 3u)));
    T.w[j] = x;
  }
}
SC_FN void sc_text_cut(ScText& T) {           // zero behind len
  for (uint32_t j = 0; j < SC_TEXT_WORDS; ++j) {
    const uint32_t keep = T.len <= 4u * j ? 0u : (T.len >= 4u * j + 4u ? 0xFFFFFFFFu : (1u << (8u * (T.len - 4u * j))) - 1u);
    T.w[j] &= keep;
  }
}
// T.w holds `nd` zero-padded digits: the leading zeros go (one digit stays in front of the point), the point and the sign come in
SC_FN void sc_text_finish(ScText& T, uint32_t nd, uint32_t scale, bool neg) {
  uint32_t lz = 0;
  bool go = true;
  for (uint32_t j = 0; j < SC_TEXT_WORDS - 1; ++j) {
    const uint32_t x = T.w[j] ^ 0x30303030u;
    if (go) {
      if (x == 0) lz += 4;
      else { lz += (uint32_t)__builtin_ctz(x) >> 3; go = false; }
    }
  }
  const uint32_t intd = nd - scale;            // >= 1: scale < nd
  const uint32_t nz = lz < intd - 1 ? lz : intd - 1;
  if (scale) sc_text_insert(T, intd, '.');
  sc_text_drop(T, nz);
  T.len = nd - nz + (scale ? 1u : 0u);
  if (neg) { sc_text_insert(T, 0, '-'); ++T.len; }
  sc_text_cut(T);
}

// One value (its two's complement image, as sc_parse gives it) -> text. SC_ERROR: a Date / Timestamp outside the valid range, or whose
// local year is not 1 .. 9999; the text is then empty.
SC_FN int sc_format(int type, uint32_t scale, int32_t offset_s, uint64_t lo, uint64_t hi, ScText& T) {
  sc_text_clear(T);
  if (type == SC_T_DATE || type == SC_T_TIMESTAMP) {
    uint32_t n, sod = 0, us = 0;
    if (type == SC_T_DATE) {
      const int32_t days = (int32_t)(uint32_t)lo;
      if (days < DT_DATE_MIN || days > DT_DATE_MAX) return SC_ERROR;
      n = (uint32_t)days + DT_SHIFT;
    } else {
      const int64_t utc = (int64_t)lo;
      if (utc < DT_TS_MIN || utc > DT_TS_MAX) return SC_ERROR;
      n = dt_split(utc, offset_s, sod, us);
    }
    uint32_t y, m, d, doy;
    dt_civil_n(n, y, m, d, doy);
    if (y < 1u || y > 9999u) return SC_ERROR;
    const uint32_t mm = sc_dig2(m) + 0x3030u, dd = sc_dig2(d) + 0x3030u;
    T.w[0] = sc_dig4(y);
    T.w[1] = 0x2D00002Du | (mm << 8);                      // "-MM-"
    T.w[2] = dd;
    T.len = 10;
    if (type == SC_T_TIMESTAMP) {
      const uint32_t h = sod / 3600u, mi = sod / 60u - h * 60u, s = sod - (sod / 60u) * 60u;
      const uint32_t hh = sc_dig2(h) + 0x3030u, mn = sc_dig2(mi) + 0x3030u, ss = sc_dig2(s) + 0x3030u;
      const uint32_t u1 = us / 100u;
      T.w[2] = dd | (0x20u << 16) | ((hh & 0xFFu) << 24);  // "DD H"
      T.w[3] = (hh >> 8) | (0x3Au << 8) | (mn << 16);      // "H:MM"
      T.w[4] = 0x2E00003Au | (ss << 8);                    // ":SS."
      T.w[5] = sc_dig4(u1);
      T.w[6] = sc_dig2(us - u1 * 100u) + 0x3030u;
      T.len = 26;
    }
    return SC_OK;
  }
  if (type == SC_T_DEC128) {
    const bool neg = (hi >> 63) != 0;
    const sc_u128 val = ((sc_u128)hi << 64) | lo;
    const sc_u128 mag = neg ? (sc_u128)0 - val : val;        // up to 2^127
    uint64_t q, r;
    sc_split19((uint64_t)(mag >> 64), (uint64_t)mag, &q, &r);
    uint32_t low[5];
    sc_dig20(q, T.w);                                         // 20 digits of the quotient,
    sc_dig20(r, low);                                         // then the remainder's 19 (its first of 20 is always '0')
    for (uint32_t j = 0; j < 5; ++j) T.w[5 + j] = (low[j] >> 8) | (j + 1 < 5 ? low[j + 1] << 24 : 0u);
    sc_text_finish(T, 39, scale, neg);
    return SC_OK;
  }
  const bool neg = (sc_is_signed(type) || type == SC_T_DEC64) && (lo >> 63) != 0;
  sc_dig20(neg ? (uint64_t)0 - lo : lo, T.w);
  sc_text_finish(T, 20, type == SC_T_DEC64 ? scale : 0u, neg);
  return SC_OK;
}
// sign extension of a narrow integer loaded as its unsigned bytes
SC_FN uint64_t sc_widen(int type, uint64_t raw) {
  switch (type) {
    case SC_T_I8: return (uint64_t)(int64_t)(int8_t)raw;
    case SC_T_I16: return (uint64_t)(int64_t)(int16_t)raw;
    case SC_T_I32: case SC_T_DATE: return (uint64_t)(int64_t)(int32_t)raw;
    default: return raw;
  }
}
// the view of a text: inline and canonical up to 12 bytes, else {len, the first four bytes, buffer 0, offset}
SC_FN void sc_text_view(const ScText& T, uint32_t offset, uint32_t (&w)[4]) {
  w[0] = T.len; w[1] = T.w[0];
  if (sv_is_inline(T.len)) { w[2] = T.w[1]; w[3] = T.w[2]; }
  else { w[2] = 0; w[3] = offset; }
}
