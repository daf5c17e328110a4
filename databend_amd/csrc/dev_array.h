// dev_array.h — the row-level logic of the Array functions (include/dbhip.h a29): a row's run in the offsets, get's index rule, find's
// equality per element type, the fold of count / sum / min / max with its Decimal128 range check, and the result type of a reduction.
// Free of HIP and built on dev_strfn.h (SfValue, for a String element), so that a host program compiles the very same text
// (tests/array_host_check.cpp). An element is read through ar_load only: one naturally aligned load of the element's own size.
#pragma once
#include "dev_strfn.h"

// the codes are the public ones (k_array.hip asserts it)
enum { AR_COUNT = 0, AR_SUM = 1, AR_MIN = 2, AR_MAX = 3, AR_KIND_COUNT = 4 };
enum { AR_CONTAINS = 0, AR_INDEXOF = 1, AR_FIND_COUNT = 2 };
enum { AR_T_BOOL = 1, AR_T_I8 = 2, AR_T_I16 = 3, AR_T_I32 = 4, AR_T_I64 = 5, AR_T_U8 = 6, AR_T_U16 = 7, AR_T_U32 = 8, AR_T_U64 = 9, AR_T_F32 = 10,
       AR_T_F64 = 11, AR_T_DATE = 12, AR_T_TIMESTAMP = 13, AR_T_DEC64 = 14, AR_T_DEC128 = 15, AR_T_STRING = 16, AR_T_DEC256 = 17 };

// The two tiers. A lane folds or searches no more than AR_LONG_LEN elements of one row; a longer row goes to the
// wave-per-row pass, AR_WAVE_STEP elements per step. A wave of the short-row pass stages AR_STAGE_BYTES of the child at a time in LDS.
constexpr uint32_t AR_LONG_LEN = 32;
constexpr uint32_t AR_WAVE_STEP = 64;
constexpr uint32_t AR_STAGE_BYTES = 8192;
constexpr int AR_MAX_NEEDLE = 255;

typedef __int128 ar_i128;
typedef unsigned __int128 ar_u128;

// how a type is folded: signed and unsigned 64-bit integers (narrower ones widened), the two floats, Decimal128
enum { AR_CLS_NONE = 0, AR_CLS_I = 1, AR_CLS_U = 2, AR_CLS_F32 = 3, AR_CLS_F64 = 4, AR_CLS_D128 = 5 };
// how two elements are compared for equality: by their bits (integers, dates, decimals) or as OrderedFloat
enum { AR_EQ_BITS = 0, AR_EQ_F32 = 1, AR_EQ_F64 = 2 };

SF_FN int ar_size(int32_t t) {
  switch (t) {
    case AR_T_I8: case AR_T_U8: return 1;
    case AR_T_I16: case AR_T_U16: return 2;
    case AR_T_I32: case AR_T_U32: case AR_T_F32: case AR_T_DATE: return 4;
    case AR_T_I64: case AR_T_U64: case AR_T_F64: case AR_T_TIMESTAMP: case AR_T_DEC64: return 8;
    case AR_T_DEC128: case AR_T_STRING: return 16;
    default: return 0;
  }
}
SF_FN int ar_class(int32_t t) {
  switch (t) {
    case AR_T_I8: case AR_T_I16: case AR_T_I32: case AR_T_I64: case AR_T_DATE: case AR_T_TIMESTAMP: case AR_T_DEC64: return AR_CLS_I;
    case AR_T_U8: case AR_T_U16: case AR_T_U32: case AR_T_U64: return AR_CLS_U;
    case AR_T_F32: return AR_CLS_F32;
    case AR_T_F64: return AR_CLS_F64;
    case AR_T_DEC128: return AR_CLS_D128;
    default: return AR_CLS_NONE;
  }
}
SF_FN int ar_eq_mode(int32_t t) { return t == AR_T_F32 ? AR_EQ_F32 : (t == AR_T_F64 ? AR_EQ_F64 : AR_EQ_BITS); }

// ---- a row's run --------------------------------------------------------------------------------------------------------------------------
// Row r owns the elements offsets[r] .. offsets[r + 1]. A pair that decreases or ends past n_elems is a BAD row: false, and an empty
// run that is never dereferenced.
SF_FN bool ar_row(const uint64_t* offsets, int64_t r, uint64_t n_elems, uint64_t* start, uint64_t* len) {
  const uint64_t a = offsets[r], b = offsets[r + 1];
  *start = 0; *len = 0;
  if (a > b || b > n_elems) return false;
  *start = a; *len = b - a;
  return true;
}

// ---- get --------------------------------------------------------------------------------------------------------------------------------------
// arr[i], 1-based, negative from the end: the position inside the run, decided by comparisons before any arithmetic (every i64 is
// defined). false: out of range (0, beyond the run either way, INT64_MIN, INT64_MAX on any real run).
SF_FN bool ar_get_pos(int64_t i, uint64_t len, uint64_t* pos) {
  *pos = 0;
  if (i >= 1) {
    if ((uint64_t)i > len) return false;
    *pos = (uint64_t)i - 1;
    return true;
  }
  if (i == 0) return false;
  const uint64_t back = (uint64_t)(-(i + 1)) + 1;            // |i| without negating INT64_MIN
  if (back > len) return false;
  *pos = len - back;
  return true;
}

// ---- an element ---------------------------------------------------------------------------------------------------------------------------
struct ArBits { uint64_t lo, hi; };
// element idx of the `es`-byte elements at base (es-aligned), zero-extended; sign-extended to 64 bits when `sign` is set (es <= 8)
SF_FN ArBits ar_load(const void* base, uint64_t idx, int es, bool sign) {
  ArBits v{0, 0};
  switch (es) {
    case 1: v.lo = sign ? (uint64_t)(int64_t)((const int8_t*)base)[idx] : (uint64_t)((const uint8_t*)base)[idx]; break;
    case 2: v.lo = sign ? (uint64_t)(int64_t)((const int16_t*)base)[idx] : (uint64_t)((const uint16_t*)base)[idx]; break;
    case 4: v.lo = sign ? (uint64_t)(int64_t)((const int32_t*)base)[idx] : (uint64_t)((const uint32_t*)base)[idx]; break;
    case 8: v.lo = ((const uint64_t*)base)[idx]; break;
    default: v.lo = ((const uint64_t*)base)[2 * idx]; v.hi = ((const uint64_t*)base)[2 * idx + 1]; break;
  }
  return v;
}
SF_FN void ar_store(void* base, uint64_t idx, int es, ArBits v) {
  switch (es) {
    case 1: ((uint8_t*)base)[idx] = (uint8_t)v.lo; break;
    case 2: ((uint16_t*)base)[idx] = (uint16_t)v.lo; break;
    case 4: ((uint32_t*)base)[idx] = (uint32_t)v.lo; break;
    case 8: ((uint64_t*)base)[idx] = v.lo; break;
    default: ((uint64_t*)base)[2 * idx] = v.lo; ((uint64_t*)base)[2 * idx + 1] = v.hi; break;
  }
}

// ---- find: equality -----------------------------------------------------------------------------------------------------------------------
// dbhip_cmp(EQ): integers, dates and decimals by their bits; floats as OrderedFloat, on the bits: NaN equals NaN whatever the sign or
// payload, -0.0 equals 0.0, everything else is equal exactly when its bits are.
SF_FN bool ar_eq(int mode, ArBits a, ArBits b) {
  if (mode == AR_EQ_F32) {
    const uint32_t x = (uint32_t)a.lo & 0x7FFFFFFFu, y = (uint32_t)b.lo & 0x7FFFFFFFu;
    if (x > 0x7F800000u || y > 0x7F800000u) return x > 0x7F800000u && y > 0x7F800000u;
    if ((x | y) == 0) return true;
    return (uint32_t)a.lo == (uint32_t)b.lo;
  }
  if (mode == AR_EQ_F64) {
    const uint64_t x = a.lo & 0x7FFFFFFFFFFFFFFFull, y = b.lo & 0x7FFFFFFFFFFFFFFFull;
    if (x > 0x7FF0000000000000ull || y > 0x7FF0000000000000ull) return x > 0x7FF0000000000000ull && y > 0x7FF0000000000000ull;
    if ((x | y) == 0) return true;
    return a.lo == b.lo;
  }
  return a.lo == b.lo && a.hi == b.hi;
}
// a String element against the constant needle: by length, then by the view's prefix, then by the bytes (aligned words of the value)
SF_FN bool ar_str_eq(SfValue& v, const uint8_t* nd, uint32_t m) {
  if (v.len != m) return false;
  uint32_t npre = 0;
  for (uint32_t i = 0; i < 4 && i < m; ++i) npre |= (uint32_t)nd[i] << (8 * i);
  const uint32_t pmask = m >= 4 ? 0xFFFFFFFFu : (m == 0 ? 0u : ((1u << (8 * m)) - 1u));
  if ((v.w1 ^ npre) & pmask) return false;
  for (uint32_t i = 4; i < m; ++i)
    if (v.byte(i) != nd[i]) return false;
  return true;
}

// ---- reduce: the fold -----------------------------------------------------------------------------------------------------------------------
// count: the non-NULL elements seen. v: the running integer sum (wrapping), the running min / max (a float's bits), the low 128 bits of
// a Decimal128 sum; ext: bits 128..191 of that sum (it is exact: 2^32 elements of 2^127 stay far inside 192 bits); f: the float sum.
struct ArAcc {
  uint64_t count;
  ar_u128 v;
  int64_t ext;
  double f;
};
SF_FN void ar_acc_init(ArAcc& a) { a.count = 0; a.v = 0; a.ext = 0; a.f = 0.0; }
SF_FN double ar_f32_of(uint64_t bits) { const uint32_t b = (uint32_t)bits; float x; __builtin_memcpy(&x, &b, 4); return (double)x; }
SF_FN double ar_f64_of(uint64_t bits) { double x; __builtin_memcpy(&x, &bits, 8); return x; }
// a < b in OrderedFloat's total order (NaN greatest and equal to itself; -0.0 equal to 0.0), both widened exactly to double
SF_FN bool ar_f_less(double a, double b) {
  if (a != a) return false;
  if (b != b) return true;
  return a < b;
}
template <int CLS>
SF_FN bool ar_less(ArBits a, ArBits b) {
  if (CLS == AR_CLS_I) return (int64_t)a.lo < (int64_t)b.lo;
  if (CLS == AR_CLS_U) return a.lo < b.lo;
  if (CLS == AR_CLS_F32) return ar_f_less(ar_f32_of(a.lo), ar_f32_of(b.lo));
  if (CLS == AR_CLS_F64) return ar_f_less(ar_f64_of(a.lo), ar_f64_of(b.lo));
  return (ar_i128)(((ar_u128)a.hi << 64) | a.lo) < (ar_i128)(((ar_u128)b.hi << 64) | b.lo);
}
SF_FN ArBits ar_bits_of(ar_u128 v) { return ArBits{(uint64_t)v, (uint64_t)(v >> 64)}; }
SF_FN ar_u128 ar_u128_of(ArBits x) { return ((ar_u128)x.hi << 64) | x.lo; }
// one non-NULL element (what ar_load gave: CLS_I sign-extended)
template <int CLS>
SF_FN void ar_fold(int kind, ArAcc& a, ArBits x) {
  const bool first = a.count == 0;
  ++a.count;
  if (kind == AR_SUM) {
    if (CLS == AR_CLS_F32) a.f += ar_f32_of(x.lo);
    else if (CLS == AR_CLS_F64) a.f += ar_f64_of(x.lo);
    else if (CLS == AR_CLS_D128) {
      const ar_u128 xv = ar_u128_of(x), s = a.v + xv;
      a.ext += ((int64_t)x.hi < 0 ? -1 : 0) + (s < xv ? 1 : 0);
      a.v = s;
    } else a.v = (uint64_t)((uint64_t)a.v + x.lo);
  } else if (kind == AR_MIN) {
    if (first || ar_less<CLS>(x, ar_bits_of(a.v))) a.v = ar_u128_of(x);
  } else if (kind == AR_MAX) {
    if (first || ar_less<CLS>(ar_bits_of(a.v), x)) a.v = ar_u128_of(x);
  }
}
// the fold of two parts of one row
template <int CLS>
SF_FN void ar_merge(int kind, ArAcc& a, const ArAcc& b) {
  if (kind == AR_SUM) {
    if (CLS == AR_CLS_F32 || CLS == AR_CLS_F64) a.f += b.f;
    else if (CLS == AR_CLS_D128) {
      const ar_u128 s = a.v + b.v;
      a.ext += b.ext + (s < b.v ? 1 : 0);
      a.v = s;
    } else a.v = (uint64_t)((uint64_t)a.v + (uint64_t)b.v);
  } else if (kind == AR_MIN) {
    if (b.count && (!a.count || ar_less<CLS>(ar_bits_of(b.v), ar_bits_of(a.v)))) a.v = b.v;
  } else if (kind == AR_MAX) {
    if (b.count && (!a.count || ar_less<CLS>(ar_bits_of(a.v), ar_bits_of(b.v)))) a.v = b.v;
  }
  a.count += b.count;
}
// 10^38 - 1, the largest Decimal128
SF_FN ar_u128 ar_dec128_max() { return (((ar_u128)0x4B3B4CA85A86C47Aull) << 64) | 0x098A223FFFFFFFFFull; }
// The row's result and its validity bit. *err: a Decimal128 sum outside +-(10^38 - 1): value 0, validity 0.
template <int CLS>
SF_FN bool ar_finish(int kind, const ArAcc& a, ArBits* out, bool* err) {
  *err = false;
  out->lo = 0; out->hi = 0;
  if (kind == AR_COUNT) { out->lo = a.count; return true; }
  if (a.count == 0) return false;
  if (kind == AR_SUM && (CLS == AR_CLS_F32 || CLS == AR_CLS_F64)) { __builtin_memcpy(&out->lo, &a.f, 8); return true; }
  if (kind == AR_SUM && CLS == AR_CLS_D128) {
    const ar_i128 s = (ar_i128)a.v;
    const bool fits = a.ext == (s < 0 ? -1 : 0);
    const ar_u128 mag = s < 0 ? (ar_u128)0 - (ar_u128)s : (ar_u128)s;
    if (!fits || mag > ar_dec128_max()) { *err = true; return false; }
  }
  *out = ar_bits_of(a.v);
  return true;
}

// ---- reduce: the result type (what dbhip_groupby_result_type gives for the same kind and argument) ---------------------------------------
// 0: accepted; 1: the pair is not offered (DBHIP_ERR_INVALID); 7: BOOL / Decimal256 elements (DBHIP_ERR_UNSUPPORTED)
SF_FN int ar_reduce_result(int32_t kind, int32_t t, uint8_t precision, uint8_t scale, int32_t* out_t, uint8_t* out_p, uint8_t* out_s) {
  if (t == AR_T_BOOL || t == AR_T_DEC256) return 7;
  if (kind < 0 || kind >= AR_KIND_COUNT || ar_class(t) == AR_CLS_NONE) return 1;
  *out_p = 0; *out_s = 0;
  if (kind == AR_COUNT) { *out_t = AR_T_U64; return 0; }
  if (kind == AR_SUM) {
    switch (t) {
      case AR_T_I8: case AR_T_I16: case AR_T_I32: case AR_T_I64: *out_t = AR_T_I64; return 0;
      case AR_T_U8: case AR_T_U16: case AR_T_U32: case AR_T_U64: *out_t = AR_T_U64; return 0;
      case AR_T_F32: case AR_T_F64: *out_t = AR_T_F64; return 0;
      case AR_T_DEC64: *out_t = AR_T_DEC64; *out_p = 18; *out_s = scale; return 0;
      case AR_T_DEC128: *out_t = AR_T_DEC128; *out_p = 38; *out_s = scale; return 0;
      default: return 1;                                     // the sum of dates or timestamps
    }
  }
  *out_t = t; *out_p = precision; *out_s = scale;
  return 0;
}
