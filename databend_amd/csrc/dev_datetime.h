// dev_datetime.h — civil-calendar arithmetic on Date (i32 days since 1970-01-01) and Timestamp (i64 microseconds since the epoch)
// values, once (include/dbhip.h a21 defines the semantics; DESIGN.md "Date and Timestamp functions"). k_datetime.hip's stand-alone
// kernels and the expression interpreter (dev_expr.h) call the same functions. Free of HIP so that a host program compiles the very
// same text (tests/datetime_host_check.cpp). DT_FN is the functions' qualifier: an includer may define it, otherwise it is host +
// device under a HIP compiler and plain `inline` elsewhere.
//
// How the row path is built:
//   - every value is moved once onto a non-negative axis: n = days + 865565 counts days from the 1st of March 400 years before year 0
//     (the year that starts in March puts the leap day last; one whole 400-year cycle = 146097 days = 20871 weeks of margin keeps
//     the local times of year 0, which a negative offset reaches, on the axis), a Timestamp becomes unsigned microseconds from the same day. From there all arithmetic is unsigned, so
//     every division is a floor division, and nothing can overflow or fault on a value outside the valid range (it wraps).
//   - days -> (year, month, day) and back are Euclidean affine functions (Neri & Schneider, "Euclidean affine functions and their
//     application to calendar algorithms", 2022): every divisor is a compile-time constant, which the compiler turns into a multiply-high
//     and a shift; the year-of-century quotient is written as the multiply-high it is. No division instruction sequence exists here.
//   - a Timestamp is split once: one 64-bit division by the constant 10^6 gives whole seconds and the microsecond; seconds >> 7 fits
//     32 bits, so days = (seconds >> 7) / 675 and everything after it is 32-bit until the final recombination.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#if !defined(DT_FN) && (defined(__HIP__) || defined(__HIPCC_RTC__))
#define DT_FN __host__ __device__ __forceinline__
#elif !defined(DT_FN)
#define DT_FN inline
#endif

// part and unit codes: the values of dbhip_dt_part_t / dbhip_dt_unit_t (k_datetime.hip pins them with static_asserts)
enum {
  DTP_YEAR = 0, DTP_QUARTER = 1, DTP_MONTH = 2, DTP_DAY = 3, DTP_DAY_OF_YEAR = 4, DTP_DOW_ISO = 5, DTP_DOW_SUNDAY0 = 6,
  DTP_ISO_YEAR = 7, DTP_ISO_WEEK = 8, DTP_HOUR = 9, DTP_MINUTE = 10, DTP_SECOND = 11, DTP_MICROSECOND = 12, DTP_EPOCH_SECOND = 13,
  DTP_YYYYMM = 14, DTP_YYYYMMDD = 15, DTP_YYYYMMDDHH = 16, DTP_YYYYMMDDHHMMSS = 17, DTP_DATE = 18, DTP_COUNT = 19
};
enum { DTU_YEAR = 0, DTU_QUARTER = 1, DTU_MONTH = 2, DTU_WEEK = 3, DTU_DAY = 4, DTU_HOUR = 5, DTU_MINUTE = 6, DTU_SECOND = 7, DTU_COUNT = 8 };
enum { DTF_WEEK_SUNDAY = 1 };

constexpr int32_t DT_DATE_MIN = -719162, DT_DATE_MAX = 2932896;                            // 0001-01-01 .. 9999-12-31
constexpr int64_t DT_TS_MIN = -62135596800000000LL, DT_TS_MAX = 253402300799999999LL;
constexpr int32_t DT_MAX_OFFSET_S = 64800, DT_MAX_TRANSITIONS = 512;
constexpr uint32_t DT_SHIFT = 719468 + 146097;                      // days from -0400-03-01 to 1970-01-01
constexpr uint32_t DT_YEAR_SHIFT = 400;
constexpr uint32_t DT_N_MIN = 306 + 146097;                         // n of 0001-01-01, a Monday: (n + 2) % 7 is 0 on Mondays (DT_N_MIN % 7 == 5)
static_assert((DT_N_MIN + 2) % 7 == 0, "weekday alignment of the day axis");
constexpr uint64_t DT_SHIFT_S = (uint64_t)DT_SHIFT * 86400u;
constexpr uint64_t DT_SHIFT_US = DT_SHIFT_S * 1000000u;

// bytes of a part's result: U8 / U16 / U32 / U64-or-I64 (DATE: the 4 bytes of a Date)
constexpr int dt_part_bytes(int part) {
  return (part == DTP_YEAR || part == DTP_DAY_OF_YEAR || part == DTP_ISO_YEAR) ? 2
       : (part == DTP_MICROSECOND || part == DTP_YYYYMM || part == DTP_YYYYMMDD || part == DTP_DATE) ? 4
       : (part == DTP_EPOCH_SECOND || part == DTP_YYYYMMDDHH || part == DTP_YYYYMMDDHHMMSS) ? 8 : 1;
}
// the part needs a time of day: Timestamp sources only
constexpr bool dt_part_needs_time(int part) {
  return part == DTP_HOUR || part == DTP_MINUTE || part == DTP_SECOND || part == DTP_MICROSECOND || part == DTP_EPOCH_SECOND ||
         part == DTP_YYYYMMDDHH || part == DTP_YYYYMMDDHHMMSS || part == DTP_DATE;
}

// ---- days <-> civil -----------------------------------------------------------------------------------------------------------------
// n -> year and day of year (1..366). `c`, `z`: century and year of century of the year that starts in March.
DT_FN void dt_year_doy_n(uint32_t n, uint32_t& year, uint32_t& doy, uint32_t& ny_out) {
  const uint32_t n1 = 4u * n + 3u;
  const uint32_t c = n1 / 146097u;
  const uint32_t nc = (n1 - c * 146097u) >> 2;                      // day of the century
  const uint32_t n2 = 4u * nc + 3u;
  const uint32_t z = (uint32_t)(((uint64_t)2939745u * n2) >> 32);   // n2 / 1461, exact below 28,825,529
  const uint32_t ny = nc - ((1461u * z) >> 2);                      // day of the March year, 0..365
  const uint32_t j = ny >= 306u;                                    // January or February: the civil year is the next one
  const uint32_t y = 100u * c + z;
  const uint32_t leap = ((z & 3u) == 0u) & ((z != 0u) | ((c & 3u) == 0u));   // of civil year y (the same 400 years later)
  year = y + j - DT_YEAR_SHIFT;
  doy = j ? ny - 305u : ny + 60u + leap;
  ny_out = ny;
}
DT_FN void dt_civil_n(uint32_t n, uint32_t& year, uint32_t& month, uint32_t& day, uint32_t& doy) {
  uint32_t ny;
  dt_year_doy_n(n, year, doy, ny);
  const uint32_t n3 = 2141u * ny + 197913u;
  const uint32_t m = n3 >> 16;                                      // 3..14
  day = (n3 & 0xffffu) / 2141u + 1u;
  month = ny >= 306u ? m - 12u : m;
}
// (year >= 0, month 1..12, day 1..31) -> n
DT_FN uint32_t dt_n_from_civil(uint32_t year, uint32_t month, uint32_t day) {
  const uint32_t j = month <= 2u;
  const uint32_t y0 = year + DT_YEAR_SHIFT - j, m0 = j ? month + 12u : month;
  const uint32_t c = y0 / 100u;
  return ((1461u * y0) >> 2) - c + (c >> 2) + ((979u * m0 - 2919u) >> 5) + (day - 1u);
}
DT_FN uint32_t dt_is_leap(uint32_t y) { return ((y & 3u) == 0u) & ((y % 25u != 0u) | ((y & 15u) == 0u)); }
DT_FN uint32_t dt_month_days(uint32_t y, uint32_t m) { return m == 2u ? 28u + dt_is_leap(y) : 30u + ((m + (m >> 3)) & 1u); }

// ---- Timestamp split ----------------------------------------------------------------------------------------------------------------
// utc micros -> whole seconds from day n = 0, 00:00 UTC (floor) and the microsecond of the second
DT_FN uint64_t dt_seconds(int64_t utc_us, uint32_t& us) {
  const uint64_t u = (uint64_t)utc_us + DT_SHIFT_US;
  const uint64_t s = u / 1000000u;
  us = (uint32_t)u - (uint32_t)s * 1000000u;                         // (the low words are enough: the result is below 2^20)
  return s;
}
// those seconds -> n and the second of the day
DT_FN uint32_t dt_days_of_seconds(uint64_t s, uint32_t& sod) {
  const uint32_t n = (uint32_t)(s >> 7) / 675u;                      // 86400 = 128 * 675; s >> 7 is below 2^32 for the whole range
  sod = (uint32_t)s - n * 86400u;
  return n;
}
// fixed-offset form of the two: local n, second of day, microsecond
DT_FN uint32_t dt_split(int64_t utc_us, int32_t offset_s, uint32_t& sod, uint32_t& us) {
  return dt_days_of_seconds(dt_seconds(utc_us, us) + (uint64_t)(int64_t)offset_s, sod);
}
// local (n, second of day, microsecond) -> utc micros
DT_FN int64_t dt_join(uint32_t n, uint32_t sod, uint32_t us, int32_t offset_s) {
  const uint64_t s = (uint64_t)n * 86400u + sod - (uint64_t)(int64_t)offset_s;
  return (int64_t)(s * 1000000u + us - DT_SHIFT_US);
}

// The offset in force at `utc_s` (seconds since the epoch, floor): offset_s before the first transition, offset_after_s[k] from
// at_utc_s[k] on — the number of transitions at or before utc_s, as np.searchsorted(at_utc_s, utc_s, 'right'). Nine halving steps
// cover 511 entries; a table of exactly 512 gets one more comparison at the end.
DT_FN int32_t dt_tz_offset(int64_t utc_s, int32_t offset_s, int32_t n_transitions, const int64_t* at_utc_s, const int32_t* offset_after_s) {
  int32_t pos = 0;
  for (int32_t step = 256; step; step >>= 1)
    if (pos + step <= n_transitions && at_utc_s[pos + step - 1] <= utc_s) pos += step;
  if (pos == 511 && n_transitions == 512 && at_utc_s[511] <= utc_s) pos = 512;
  return pos ? offset_after_s[pos - 1] : offset_s;
}

// ---- parts --------------------------------------------------------------------------------------------------------------------------
// `s_utc`: dt_seconds of the value (EPOCH_SECOND only). Results are the part's unsigned image (EPOCH_SECOND / DATE: two's complement).
DT_FN uint64_t dt_part_value(int part, uint32_t n, uint32_t sod, uint32_t us, uint64_t s_utc) {
  uint32_t y, m, d, doy, ny;
  switch (part) {
    case DTP_YEAR: dt_year_doy_n(n, y, doy, ny); return y;
    case DTP_DAY_OF_YEAR: dt_year_doy_n(n, y, doy, ny); return doy;
    case DTP_QUARTER: dt_civil_n(n, y, m, d, doy); return (m + 2u) / 3u;
    case DTP_MONTH: dt_civil_n(n, y, m, d, doy); return m;
    case DTP_DAY: dt_civil_n(n, y, m, d, doy); return d;
    case DTP_DOW_ISO: return (n + 2u) % 7u + 1u;
    case DTP_DOW_SUNDAY0: return (n + 3u) % 7u;
    case DTP_ISO_YEAR: case DTP_ISO_WEEK: {                          // the year and the week of the Thursday of the row's week
      const uint32_t th = n - (n + 2u) % 7u + 3u;
      dt_year_doy_n(th, y, doy, ny);
      return part == DTP_ISO_YEAR ? y : (doy - 1u) / 7u + 1u;
    }
    case DTP_HOUR: return sod / 3600u;
    case DTP_MINUTE: return sod / 60u - (sod / 3600u) * 60u;
    case DTP_SECOND: return sod % 60u;
    case DTP_MICROSECOND: return us;
    case DTP_EPOCH_SECOND: return s_utc - DT_SHIFT_S;
    case DTP_YYYYMM: dt_civil_n(n, y, m, d, doy); return y * 100u + m;
    case DTP_YYYYMMDD: dt_civil_n(n, y, m, d, doy); return y * 10000u + m * 100u + d;
    case DTP_YYYYMMDDHH: dt_civil_n(n, y, m, d, doy); return (uint64_t)(y * 10000u + m * 100u + d) * 100u + sod / 3600u;   // (9999123123 does not fit 32 bits)
    case DTP_YYYYMMDDHHMMSS: {
      dt_civil_n(n, y, m, d, doy);
      const uint32_t h = sod / 3600u, mi = sod / 60u - h * 60u, s = sod - (sod / 60u) * 60u;
      return (uint64_t)(y * 10000u + m * 100u + d) * 1000000u + (h * 10000u + mi * 100u + s);
    }
    default: return (uint64_t)(int64_t)(int32_t)(n - DT_SHIFT);      // DTP_DATE
  }
}
DT_FN uint64_t dt_part_date(int part, int32_t days) { return dt_part_value(part, (uint32_t)days + DT_SHIFT, 0, 0, 0); }
DT_FN uint64_t dt_part_ts(int part, int64_t utc_us, int32_t offset_s) {
  uint32_t us, sod;
  const uint64_t s = dt_seconds(utc_us, us);
  const uint32_t n = dt_days_of_seconds(s + (uint64_t)(int64_t)offset_s, sod);
  return dt_part_value(part, n, sod, us, s);
}

// ---- truncation ---------------------------------------------------------------------------------------------------------------------
// first day (as n) of the year / quarter / month / week of day n; DAY and the time units return n
DT_FN uint32_t dt_trunc_n(int unit, int flags, uint32_t n) {
  uint32_t y, m, d, doy, ny;
  switch (unit) {
    case DTU_YEAR: dt_year_doy_n(n, y, doy, ny); return n - (doy - 1u);
    case DTU_QUARTER: dt_civil_n(n, y, m, d, doy); return dt_n_from_civil(y, m - (m - 1u) % 3u, 1u);
    case DTU_MONTH: dt_civil_n(n, y, m, d, doy); return n - (d - 1u);
    case DTU_WEEK: return n - ((flags & DTF_WEEK_SUNDAY) ? (n + 3u) % 7u : (n + 2u) % 7u);
    default: return n;
  }
}
DT_FN uint32_t dt_trunc_sod(int unit, uint32_t sod) {
  switch (unit) {
    case DTU_HOUR: return sod - sod % 3600u;
    case DTU_MINUTE: return sod - sod % 60u;
    case DTU_SECOND: return sod;
    default: return 0;
  }
}
DT_FN int32_t dt_clamp_date(int32_t d) { return d < DT_DATE_MIN ? DT_DATE_MIN : (d > DT_DATE_MAX ? DT_DATE_MAX : d); }
DT_FN int64_t dt_clamp_ts(int64_t t) { return t < DT_TS_MIN ? DT_TS_MIN : (t > DT_TS_MAX ? DT_TS_MAX : t); }
// The four source / output pairs. The result is clamped into the output type's range: the floor of a valid value is valid except at the
// very start of year 1 (the Sunday start of the first week; local midnight of a zone east of UTC).
DT_FN int32_t dt_trunc_date_to_date(int unit, int flags, int32_t days) {
  return dt_clamp_date((int32_t)(dt_trunc_n(unit, flags, (uint32_t)days + DT_SHIFT) - DT_SHIFT));
}
DT_FN int64_t dt_trunc_date_to_ts(int unit, int flags, int32_t days, int32_t offset_s) {
  return dt_clamp_ts(dt_join(dt_trunc_n(unit, flags, (uint32_t)days + DT_SHIFT), 0, 0, offset_s));
}
DT_FN int64_t dt_trunc_ts_to_ts(int unit, int flags, int64_t utc_us, int32_t offset_s) {
  uint32_t sod, us;
  const uint32_t n = dt_split(utc_us, offset_s, sod, us);
  return dt_clamp_ts(dt_join(dt_trunc_n(unit, flags, n), dt_trunc_sod(unit, sod), 0, offset_s));
}
DT_FN int32_t dt_trunc_ts_to_date(int unit, int flags, int64_t utc_us, int32_t offset_s) {
  uint32_t sod, us;
  const uint32_t n = dt_split(utc_us, offset_s, sod, us);
  return dt_clamp_date((int32_t)(dt_trunc_n(unit, flags, n) - DT_SHIFT));
}

// ---- addition -----------------------------------------------------------------------------------------------------------------------
// false = the row error "date out of range". |delta| is bounded BEFORE any multiply, by a bound above the whole range's span in the
// unit (so a refused delta would have left the range anyway) and small enough that nothing below can wrap.
DT_FN bool dt_delta_ok(int64_t delta, int64_t bound) { return delta <= bound && delta >= -bound; }
// month arithmetic on day n: false when the target month lies outside 0000-01 .. 10000-12 (the caller's range check does the rest)
DT_FN bool dt_add_months_n(uint32_t n, int32_t months, uint32_t& out) {
  uint32_t y, m, d, doy;
  dt_civil_n(n, y, m, d, doy);
  const int32_t t = (int32_t)(y * 12u + (m - 1u)) + months;
  if (t < 0 || t > 10000 * 12 + 11) return false;
  const uint32_t y2 = (uint32_t)t / 12u, m2 = (uint32_t)t - y2 * 12u + 1u;
  const uint32_t last = dt_month_days(y2, m2);
  out = dt_n_from_civil(y2, m2, d < last ? d : last);
  return true;
}
DT_FN bool dt_add_date(int unit, int32_t days, int64_t delta, int32_t& out) {
  out = 0;
  if (days < DT_DATE_MIN || days > DT_DATE_MAX) return false;
  int32_t r;
  if (unit <= DTU_MONTH) {
    if (!dt_delta_ok(delta, 200000)) return false;
    uint32_t n2;
    if (!dt_add_months_n((uint32_t)days + DT_SHIFT, (int32_t)delta * (unit == DTU_YEAR ? 12 : (unit == DTU_QUARTER ? 3 : 1)), n2)) return false;
    r = (int32_t)(n2 - DT_SHIFT);
  } else {                                                            // WEEK, DAY (the host refuses the time units on a Date)
    if (!dt_delta_ok(delta, unit == DTU_WEEK ? 600000 : 4000000)) return false;   // the range spans 3,652,058 days
    r = days + (int32_t)delta * (unit == DTU_WEEK ? 7 : 1);
  }
  if (r < DT_DATE_MIN || r > DT_DATE_MAX) return false;
  out = r;
  return true;
}
DT_FN bool dt_add_ts(int unit, int64_t utc_us, int64_t delta, int32_t offset_s, int64_t& out) {
  out = 0;
  if (utc_us < DT_TS_MIN || utc_us > DT_TS_MAX) return false;
  int64_t r;
  if (unit <= DTU_MONTH) {
    if (!dt_delta_ok(delta, 200000)) return false;
    uint32_t sod, us, n2;
    const uint32_t n = dt_split(utc_us, offset_s, sod, us);
    if (!dt_add_months_n(n, (int32_t)delta * (unit == DTU_YEAR ? 12 : (unit == DTU_QUARTER ? 3 : 1)), n2)) return false;
    r = dt_join(n2, sod, us, offset_s);
  } else {
    // the range spans 3.156e17 microseconds: 3.2e17 / (the unit's microseconds) bounds every delta that could stay inside
    const int64_t unit_us = unit == DTU_WEEK ? 604800000000LL : unit == DTU_DAY ? 86400000000LL : unit == DTU_HOUR ? 3600000000LL
                          : unit == DTU_MINUTE ? 60000000LL : 1000000LL;
    const int64_t bound = unit == DTU_WEEK ? 529101LL : unit == DTU_DAY ? 3703704LL : unit == DTU_HOUR ? 88888889LL
                        : unit == DTU_MINUTE ? 5333333334LL : 320000000000LL;
    if (!dt_delta_ok(delta, bound)) return false;
    r = utc_us + delta * unit_us;
  }
  if (r < DT_TS_MIN || r > DT_TS_MAX) return false;
  out = r;
  return true;
}

// ---- difference ---------------------------------------------------------------------------------------------------------------------
// boundaries of `unit` crossed from a to b (days as n); YEAR / QUARTER / MONTH / WEEK / DAY
DT_FN int64_t dt_diff_n(int unit, uint32_t na, uint32_t nb) {
  if (unit == DTU_DAY) return (int64_t)(int32_t)(nb - na);
  if (unit == DTU_WEEK) return (int64_t)(int32_t)((nb + 2u) / 7u - (na + 2u) / 7u);   // (n + 2) / 7 = floor((days + 3) / 7) + a constant
  uint32_t ya, ma, yb, mb, d, doy;
  dt_civil_n(na, ya, ma, d, doy);
  dt_civil_n(nb, yb, mb, d, doy);
  if (unit == DTU_YEAR) return (int64_t)(int32_t)(yb - ya);
  if (unit == DTU_QUARTER) return (int64_t)(int32_t)((yb * 4u + (mb - 1u) / 3u) - (ya * 4u + (ma - 1u) / 3u));
  return (int64_t)(int32_t)((yb * 12u + mb) - (ya * 12u + ma));
}
DT_FN int64_t dt_diff_date(int unit, int32_t a, int32_t b) { return dt_diff_n(unit, (uint32_t)a + DT_SHIFT, (uint32_t)b + DT_SHIFT); }
DT_FN int64_t dt_diff_ts(int unit, int64_t a, int64_t b, int32_t offset_s) {
  if (unit >= DTU_HOUR) {                                             // floor quotients of local micros
    const uint64_t shift = DT_SHIFT_US + (uint64_t)((int64_t)offset_s * 1000000);
    const uint64_t la = (uint64_t)a + shift, lb = (uint64_t)b + shift;
    if (unit == DTU_HOUR) return (int64_t)(lb / 3600000000u - la / 3600000000u);   // (one constant per branch: no division by a variable)
    if (unit == DTU_MINUTE) return (int64_t)(lb / 60000000u - la / 60000000u);
    return (int64_t)(lb / 1000000u - la / 1000000u);
  }
  uint32_t sod, us;
  const uint32_t na = dt_split(a, offset_s, sod, us), nb = dt_split(b, offset_s, sod, us);
  return dt_diff_n(unit, na, nb);
}
