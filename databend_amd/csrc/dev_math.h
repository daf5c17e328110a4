// dev_math.h — the row-level logic of the math functions (include/dbhip.h a26): abs, sign, ceil, floor, round, truncate, sqrt over
// numbers and over Decimal64 / Decimal128. Free of HIP, in the style of dev_strcast.h, so that a host program compiles the very same
// text (tests/math_host_check.cpp). MT_FN is the functions' qualifier: an includer may define it. Nothing but <stdint.h> is included:
// the floating-point primitives are the compiler's builtins (ceil, floor, trunc, round and sqrt of a double are correctly rounded IEEE
// operations on both sides). ABS of a float works on the bit pattern: the includer moves such a column as unsigned words.
//
// Numbers. Every function of a number is a function of x = (double)v except ABS and SIGN. ROUND / TRUNCATE at d digits multiply or
// divide by P[|d|], the f64 NEAREST to 10^|d|: a table of decimal literals, never pow or a running product (10.0^23 computed by
// multiplication already differs from 1e23 in the last bit). The expressions hold no a*b+c, so nothing can be contracted into a fused
// multiply-add; k_math.hip is nevertheless compiled with -ffp-contract=off, so that a later edit cannot change that silently.
//
// Decimals. A call is decoded ONCE, on the host, into an MtDec: what is added to the magnitude before the division (the half for
// ROUND, 10^s - 1 on one side for CEIL / FLOOR, nothing for TRUNCATE), the divisor 10^k as one or two 64-bit powers of ten, the
// multiplier 10^(-digits) of a negative digits, and the two degenerate forms (copy, all zero). The kernel reads the struct from its
// arguments, so every branch on it is wave-uniform. Rows work on the unsigned magnitude: |v| + addend stays below 2^64 / 2^128 for
// every stored bit pattern, so nothing wraps before the division and nothing is undefined. No 128-bit `/` or `%` appears (a compiler
// expands one into a 128-step loop on the device): 10^k, k <= 19, is one 128-by-64 division (mt_div128_64, schoolbook on 32-bit
// digits), and for k > 19 the quotient by 10^19 is divided again by 10^(k-19) — for unsigned operands floor(floor(u/a)/b) =
// floor(u/(ab)), and the addend went in first.
#pragma once
#include <stdint.h>

#if !defined(MT_FN) && (defined(__HIP__) || defined(__HIPCC_RTC__))
#define MT_FN __host__ __device__ inline __attribute__((always_inline))
#elif !defined(MT_FN)
#define MT_FN inline
#endif

// the function codes are the public ones (k_math.hip asserts it)
enum { MT_ABS = 0, MT_SIGN = 1, MT_CEIL = 2, MT_FLOOR = 3, MT_ROUND = 4, MT_TRUNCATE = 5, MT_SQRT = 6, MT_FN_COUNT = 7 };
constexpr int MT_MAX_DIGITS = 30;          // ROUND / TRUNCATE over a number: digits are clamped to +-30
typedef unsigned __int128 mt_u128;
typedef __int128 mt_i128;

// ---- numbers ------------------------------------------------------------------------------------------------------------------------
// the f64 nearest to 10^k, 0 <= k <= 30
MT_FN double mt_p10_f64(int k) {
  switch (k) {
    case 0: return 1e0;   case 1: return 1e1;   case 2: return 1e2;   case 3: return 1e3;   case 4: return 1e4;   case 5: return 1e5;
    case 6: return 1e6;   case 7: return 1e7;   case 8: return 1e8;   case 9: return 1e9;   case 10: return 1e10; case 11: return 1e11;
    case 12: return 1e12; case 13: return 1e13; case 14: return 1e14; case 15: return 1e15; case 16: return 1e16; case 17: return 1e17;
    case 18: return 1e18; case 19: return 1e19; case 20: return 1e20; case 21: return 1e21; case 22: return 1e22; case 23: return 1e23;
    case 24: return 1e24; case 25: return 1e25; case 26: return 1e26; case 27: return 1e27; case 28: return 1e28; case 29: return 1e29;
    default: return 1e30;
  }
}

// the decoded second argument of ROUND / TRUNCATE over a number: side 0 (d == 0), +1 (d > 0: multiply first) or -1 (divide first)
struct MtNum {
  int32_t fn;
  int32_t side;
  double p10;
};
MT_FN MtNum mt_num_decode(int fn, int32_t digits) {
  MtNum m;
  m.fn = fn; m.side = 0; m.p10 = 1e0;
  if (fn == MT_ROUND || fn == MT_TRUNCATE) {
    const int d = digits < -MT_MAX_DIGITS ? -MT_MAX_DIGITS : digits > MT_MAX_DIGITS ? MT_MAX_DIGITS : digits;
    m.side = d > 0 ? 1 : d < 0 ? -1 : 0;
    m.p10 = mt_p10_f64(d < 0 ? -d : d);
  }
  return m;
}

MT_FN uint32_t mt_abs_f32_bits(uint32_t b) { return b & 0x7FFFFFFFu; }
MT_FN uint64_t mt_abs_f64_bits(uint64_t b) { return b & 0x7FFFFFFFFFFFFFFFull; }
// abs of a signed integer into the unsigned type of its width: 0 - (uN)v, so the minimum is exact
template <typename S, typename U> MT_FN U mt_abs_int(S v) { return v < 0 ? (U)((U)0 - (U)v) : (U)v; }
// integers, floats (NaN and both zeros give 0) and decimals alike
template <typename T> MT_FN int8_t mt_sign(T v) { return v > (T)0 ? (int8_t)1 : v < (T)0 ? (int8_t)-1 : (int8_t)0; }

// half away from zero (C's round) or toward zero
MT_FN double mt_round_to(bool half_away, double x) { return half_away ? __builtin_round(x) : __builtin_trunc(x); }

// CEIL, FLOOR, ROUND, TRUNCATE, SQRT of x = (double)v; the three operations of a scaled rounding run in exactly this order
MT_FN double mt_num_f64(const MtNum& m, double x) {
  switch (m.fn) {
    case MT_CEIL: return __builtin_ceil(x);
    case MT_FLOOR: return __builtin_floor(x);
    case MT_SQRT: return __builtin_sqrt(x);
    default: {
      const bool half_away = m.fn == MT_ROUND;
      if (m.side == 0) return mt_round_to(half_away, x);
      if (m.side > 0) {
        const double scaled = x * m.p10;
        return mt_round_to(half_away, scaled) / m.p10;
      }
      const double scaled = x / m.p10;
      return mt_round_to(half_away, scaled) * m.p10;
    }
  }
}

// ---- decimals -----------------------------------------------------------------------------------------------------------------------
enum { MT_DEC_COPY = 0, MT_DEC_ZERO = 1, MT_DEC_ABS = 2, MT_DEC_DIV = 3 };
struct MtDec {
  int32_t mode;                    // MT_DEC_*
  int32_t k;                       // the divisor is 10^k (MT_DEC_DIV: 1 <= k <= 38)
  uint64_t div0, div1;             // 10^min(k, 19) and 10^(k - 19), or 1
  uint64_t add_pos_lo, add_pos_hi; // added to |v| when v > 0: the half (ROUND), 10^s - 1 (CEIL)
  uint64_t add_neg_lo, add_neg_hi; // added to |v| when v < 0: the half (ROUND), 10^s - 1 (FLOOR)
  uint64_t post_lo, post_hi;       // the quotient is multiplied by 10^(-digits) when digits < 0, else by 1
};

MT_FN mt_u128 mt_p10_u128(int k) {
  mt_u128 r = 1;
  for (int i = 0; i < k; ++i) r *= 10u;
  return r;
}

// the result's scale: CEIL / FLOOR 0, ROUND / TRUNCATE clamp(digits, 0, s), ABS s
MT_FN int mt_dec_result_scale(int fn, int s, int32_t digits) {
  if (fn == MT_CEIL || fn == MT_FLOOR) return 0;
  if (fn == MT_ROUND || fn == MT_TRUNCATE) return digits < 0 ? 0 : digits > s ? s : digits;
  return s;
}

// fn is ABS, CEIL, FLOOR, ROUND or TRUNCATE; 1 <= p <= 38, s <= p
MT_FN MtDec mt_dec_decode(int fn, int p, int s, int32_t digits) {
  MtDec d;
  d.mode = MT_DEC_COPY; d.k = 0; d.div0 = 1; d.div1 = 1;
  d.add_pos_lo = d.add_pos_hi = d.add_neg_lo = d.add_neg_hi = 0;
  d.post_lo = 1; d.post_hi = 0;
  if (fn == MT_ABS) { d.mode = MT_DEC_ABS; return d; }
  const bool to_digits = fn == MT_ROUND || fn == MT_TRUNCATE;
  const int64_t k = to_digits ? (int64_t)s - (int64_t)digits : (int64_t)s;
  if (k <= 0) return d;                           // nothing to cut: a copy
  if (k > p) { d.mode = MT_DEC_ZERO; return d; }  // every row is 0, written without forming 10^k
  d.mode = MT_DEC_DIV;
  d.k = (int32_t)k;
  d.div0 = (uint64_t)mt_p10_u128(k > 19 ? 19 : (int)k);
  d.div1 = k > 19 ? (uint64_t)mt_p10_u128((int)k - 19) : 1;
  const mt_u128 pk = mt_p10_u128((int)k);
  mt_u128 pos = 0, neg = 0;
  if (fn == MT_ROUND) pos = neg = pk / 2;
  else if (fn == MT_CEIL) pos = pk - 1;
  else if (fn == MT_FLOOR) neg = pk - 1;
  d.add_pos_lo = (uint64_t)pos; d.add_pos_hi = (uint64_t)(pos >> 64);
  d.add_neg_lo = (uint64_t)neg; d.add_neg_hi = (uint64_t)(neg >> 64);
  if (to_digits && digits < 0) {                  // k <= p, so -digits <= p - s <= 38
    const mt_u128 post = mt_p10_u128((int)(k - s));
    d.post_lo = (uint64_t)post; d.post_hi = (uint64_t)(post >> 64);
  }
  return d;
}

// (hi:lo) / v for hi < v, v != 0: the 64-bit quotient (Knuth's algorithm D on 32-bit digits, two quotient digits)
MT_FN uint64_t mt_div128_64_digit(uint64_t hi, uint64_t lo, uint64_t v) {
  const uint64_t b = 1ull << 32;
  const int sh = __builtin_clzll(v);
  v <<= sh;
  const uint64_t vn1 = v >> 32, vn0 = v & 0xFFFFFFFFull;
  const uint64_t un32 = sh ? ((hi << sh) | (lo >> (64 - sh))) : hi;
  const uint64_t un10 = lo << sh;
  const uint64_t un1 = un10 >> 32, un0 = un10 & 0xFFFFFFFFull;
  uint64_t q1 = un32 / vn1, rhat = un32 - q1 * vn1;
  while (q1 >= b || q1 * vn0 > ((rhat << 32) | un1)) {
    --q1; rhat += vn1;
    if (rhat >= b) break;
  }
  const uint64_t un21 = (un32 << 32) + un1 - q1 * v;   // wraps as intended: the true value is below v
  uint64_t q0 = un21 / vn1;
  rhat = un21 - q0 * vn1;
  while (q0 >= b || q0 * vn0 > ((rhat << 32) | un0)) {
    --q0; rhat += vn1;
    if (rhat >= b) break;
  }
  return (q1 << 32) + q0;
}
// u / v, v != 0, by two steps of the above; no 128-bit division
MT_FN mt_u128 mt_div128_64(mt_u128 u, uint64_t v) {
  const uint64_t hi = (uint64_t)(u >> 64), lo = (uint64_t)u;
  const uint64_t qh = hi / v;
  const uint64_t rh = hi - qh * v;
  const uint64_t ql = mt_div128_64_digit(rh, lo, v);
  return ((mt_u128)qh << 64) | ql;
}

MT_FN int64_t mt_dec64(const MtDec& d, int64_t v) {
  if (d.mode == MT_DEC_COPY) return v;
  if (d.mode == MT_DEC_ZERO) return 0;
  const bool neg = v < 0;
  uint64_t m = neg ? 0ull - (uint64_t)v : (uint64_t)v;
  if (d.mode == MT_DEC_DIV) {
    m += neg ? d.add_neg_lo : d.add_pos_lo;       // (an addend is below 10^k, so 0 stays 0)
    m = m / d.div0 * d.post_lo;                    // k <= 18: one divisor
    return (int64_t)(neg ? 0ull - m : m);
  }
  return (int64_t)m;                               // MT_DEC_ABS (wrapping at the minimum)
}

MT_FN mt_i128 mt_dec128(const MtDec& d, mt_i128 v) {
  if (d.mode == MT_DEC_COPY) return v;
  if (d.mode == MT_DEC_ZERO) return 0;
  const bool neg = v < 0;
  mt_u128 m = neg ? (mt_u128)0 - (mt_u128)v : (mt_u128)v;
  if (d.mode == MT_DEC_DIV) {
    m += neg ? (((mt_u128)d.add_neg_hi << 64) | d.add_neg_lo) : (((mt_u128)d.add_pos_hi << 64) | d.add_pos_lo);
    m = mt_div128_64(m, d.div0);
    if (d.div1 != 1) m = mt_div128_64(m, d.div1);
    m *= ((mt_u128)d.post_hi << 64) | d.post_lo;
    return (mt_i128)(neg ? (mt_u128)0 - m : m);
  }
  return (mt_i128)m;
}
