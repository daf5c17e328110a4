// k_datetime.hip — Date and Timestamp functions (include/dbhip.h a21): extract a part, truncate, add an interval, count boundaries.
//
// The arithmetic is dev_datetime.h's (one text for these kernels, the expression interpreter and the host checker); this file is the
// memory side. Every kernel is a map whose lanes each own a run of CONSECUTIVE rows sized so that the narrower of input and output
// moves as whole 16-byte vectors: a U8 part takes 16 rows per lane (4 or 8 dwordx4 loads, one dwordx4 store), U16 8, U32 / Date 4,
// 64-bit results 2. The last n mod rows-per-lane rows are done one per lane by the first workgroup. A scalar input is read once per lane.
// The loop of the one-input kernels and every memory access are dev_map.h's; the entry points insist on 16-byte bases, so the kernels
// pass std::true_type() and have its 16-byte form alone.
// Validity is not touched: it passes through (the binding reuses the source's bitmap); the add kernel reads a row's validity bits only
// when that row fails, to keep a NULL row from raising.
// Time zone: a fixed offset travels as a kernel argument and those instantiations use no LDS. A transition table (dbhip_dt_part only)
// is uploaded through the scratch, copied to LDS by every workgroup and searched there (dt_tz_offset: 9 halving steps).
#include <string.h>

#include <type_traits>

#include "dev_common.h"
#include "dev_datetime.h"
#include "dev_map.h"
#include "runtime.h"

using namespace dbhip;

// the codes dev_datetime.h and dev_expr.h use are the public ones
static_assert(DTP_YEAR == DBHIP_DT_PART_YEAR && DTP_QUARTER == DBHIP_DT_PART_QUARTER && DTP_MONTH == DBHIP_DT_PART_MONTH && DTP_DAY == DBHIP_DT_PART_DAY &&
              DTP_DAY_OF_YEAR == DBHIP_DT_PART_DAY_OF_YEAR && DTP_DOW_ISO == DBHIP_DT_PART_DOW_ISO && DTP_DOW_SUNDAY0 == DBHIP_DT_PART_DOW_SUNDAY0 &&
              DTP_ISO_YEAR == DBHIP_DT_PART_ISO_YEAR && DTP_ISO_WEEK == DBHIP_DT_PART_ISO_WEEK && DTP_HOUR == DBHIP_DT_PART_HOUR &&
              DTP_MINUTE == DBHIP_DT_PART_MINUTE && DTP_SECOND == DBHIP_DT_PART_SECOND && DTP_MICROSECOND == DBHIP_DT_PART_MICROSECOND &&
              DTP_EPOCH_SECOND == DBHIP_DT_PART_EPOCH_SECOND && DTP_YYYYMM == DBHIP_DT_PART_YYYYMM && DTP_YYYYMMDD == DBHIP_DT_PART_YYYYMMDD &&
              DTP_YYYYMMDDHH == DBHIP_DT_PART_YYYYMMDDHH && DTP_YYYYMMDDHHMMSS == DBHIP_DT_PART_YYYYMMDDHHMMSS && DTP_DATE == DBHIP_DT_PART_DATE,
              "dev_datetime.h part codes");
static_assert(DTU_YEAR == DBHIP_DT_UNIT_YEAR && DTU_QUARTER == DBHIP_DT_UNIT_QUARTER && DTU_MONTH == DBHIP_DT_UNIT_MONTH && DTU_WEEK == DBHIP_DT_UNIT_WEEK &&
              DTU_DAY == DBHIP_DT_UNIT_DAY && DTU_HOUR == DBHIP_DT_UNIT_HOUR && DTU_MINUTE == DBHIP_DT_UNIT_MINUTE && DTU_SECOND == DBHIP_DT_UNIT_SECOND &&
              DTF_WEEK_SUNDAY == DBHIP_DT_WEEK_SUNDAY, "dev_datetime.h unit codes");

namespace {

constexpr int DT_SCRATCH_SLOT = 23;

template <int BYTES> struct UIntOf;
template <> struct UIntOf<1> { typedef uint8_t type; };
template <> struct UIntOf<2> { typedef uint16_t type; };
template <> struct UIntOf<4> { typedef uint32_t type; };
template <> struct UIntOf<8> { typedef uint64_t type; };

struct MapArgs {
  const void* in;
  void* out;
  int64_t n;
  int32_t scalar, code, flags, offset;
  int32_t n_transitions, _pad;
  const int64_t* at_utc_s;       // device copies of the table (scratch)
  const int32_t* offset_after_s;
};

template <int PART, bool TS, bool TABLE>
struct PartOp {
  typedef typename std::conditional<TS, int64_t, int32_t>::type In;
  typedef typename UIntOf<dt_part_bytes(PART)>::type Out;
  static constexpr bool kTable = TABLE;
  static __device__ __forceinline__ Out apply(In v, const MapArgs& A, const int64_t* at, const int32_t* after) {
    if constexpr (!TS) {
      return (Out)dt_part_date(PART, v);
    } else if constexpr (!TABLE) {
      return (Out)dt_part_ts(PART, v, A.offset);
    } else {
      uint32_t us, sod;
      const uint64_t s = dt_seconds(v, us);
      const int32_t off = dt_tz_offset((int64_t)(s - DT_SHIFT_S), A.offset, A.n_transitions, at, after);
      const uint32_t n = dt_days_of_seconds(s + (uint64_t)(int64_t)off, sod);
      return (Out)dt_part_value(PART, n, sod, us, s);
    }
  }
};

template <bool TS_IN, bool TS_OUT>
struct TruncOp {
  typedef typename std::conditional<TS_IN, int64_t, int32_t>::type In;
  typedef typename std::conditional<TS_OUT, uint64_t, uint32_t>::type Out;
  static constexpr bool kTable = false;
  static __device__ __forceinline__ Out apply(In v, const MapArgs& A, const int64_t*, const int32_t*) {
    if constexpr (TS_IN && TS_OUT) return (Out)dt_trunc_ts_to_ts(A.code, A.flags, v, A.offset);
    else if constexpr (TS_IN) return (Out)dt_trunc_ts_to_date(A.code, A.flags, v, A.offset);
    else if constexpr (TS_OUT) return (Out)dt_trunc_date_to_ts(A.code, A.flags, v, A.offset);
    else return (Out)dt_trunc_date_to_date(A.code, A.flags, v);
  }
};

template <typename Op>
__global__ __launch_bounds__(256) void dt_map_kernel(const MapArgs A) {
  typedef typename Op::In In;
  typedef typename Op::Out Out;
  __shared__ int64_t s_at[Op::kTable ? DT_MAX_TRANSITIONS : 1];
  __shared__ int32_t s_after[Op::kTable ? DT_MAX_TRANSITIONS : 1];
  if constexpr (Op::kTable) {
    for (int i = threadIdx.x; i < A.n_transitions; i += 256) { s_at[i] = A.at_utc_s[i]; s_after[i] = A.offset_after_s[i]; }
    __syncthreads();
  }
  map_rows<In, Out>(A.in, std::true_type(), A.scalar != 0, A.out, std::true_type(), A.n, [&](In v) { return Op::apply(v, A, s_at, s_after); });
}

template <typename Op>
int32_t launch_map(const MapArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(dt_map_kernel<Op>, dim3(map_grid<typename Op::In, typename Op::Out>(A.n)), dim3(256), 0, s, A);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}
template <int PART>
int32_t launch_part(bool ts, bool table, const MapArgs& A, hipStream_t s) {
  if (!ts) {
    if constexpr (!dt_part_needs_time(PART)) return launch_map<PartOp<PART, false, false>>(A, s);
    else return DBHIP_ERR_INVALID;
  }
  return table ? launch_map<PartOp<PART, true, true>>(A, s) : launch_map<PartOp<PART, true, false>>(A, s);
}

// ---- add ------------------------------------------------------------------------------------------------------------------------------
struct AddArgs {
  const void* src;
  const int64_t* delta;
  void* out;
  const uint8_t *src_valid, *delta_valid;
  int64_t src_voff, delta_voff, n;
  int32_t src_scalar, delta_scalar, unit, offset;
  uint32_t* err_words;             // preset to all ones (may be NULL)
  unsigned long long* err_count;   // may be NULL
};

template <bool TS>
__device__ __forceinline__ typename std::conditional<TS, int64_t, int32_t>::type dt_add_row(const AddArgs& A, typename std::conditional<TS, int64_t, int32_t>::type v,
                                                                                             int64_t d, int64_t row, uint32_t& raised) {
  typename std::conditional<TS, int64_t, int32_t>::type r;
  bool ok;
  if constexpr (TS) ok = dt_add_ts(A.unit, v, d, A.offset, r);
  else ok = dt_add_date(A.unit, v, d, r);
  if (!ok) {   // "date out of range" — unless the row is NULL (either operand)
    const bool valid = (!A.src_valid || bit_get(A.src_valid, A.src_voff + (A.src_scalar ? 0 : row))) &&
                       (!A.delta_valid || bit_get(A.delta_valid, A.delta_voff + (A.delta_scalar ? 0 : row)));
    if (valid) {
      if (A.err_words) atomicAnd(&A.err_words[row >> 5], ~(1u << (row & 31)));
      ++raised;   // counted per lane, added once per wave at the end of the kernel: a delta that fails every row would otherwise
                  // serialise all n rows on the one counter word
    }
  }
  return r;
}

template <bool TS>
__global__ __launch_bounds__(256) void dt_add_kernel(const AddArgs A) {
  typedef typename std::conditional<TS, int64_t, int32_t>::type T;
  constexpr int ROWS = 16 / sizeof(T);
  const int64_t groups = A.n / ROWS;
  uint32_t raised = 0;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    T v[ROWS], r[ROWS];
    int64_t d[ROWS];
    map_fetch<T, ROWS>(A.src, std::true_type(), A.src_scalar != 0, g * ROWS, v);
    map_fetch<int64_t, ROWS>(A.delta, std::true_type(), A.delta_scalar != 0, g * ROWS, d);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) r[k] = dt_add_row<TS>(A, v[k], d[k], g * ROWS + k, raised);
    map_store<T, ROWS>(A.out, std::true_type(), g * ROWS, r);
  }
  const int64_t i = groups * ROWS + threadIdx.x;
  if (blockIdx.x == 0 && i < A.n)
    map_store_one<T>(A.out, i, dt_add_row<TS>(A, map_load_one<T>(A.src, A.src_scalar ? 0 : i), map_load_one<int64_t>(A.delta, A.delta_scalar ? 0 : i), i, raised));
  // every lane arrives here: one add per wave that raised at all
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) raised += __shfl_xor(raised, off, 64);
  if ((threadIdx.x & 63) == 0 && raised && A.err_count) atomicAdd(A.err_count, (unsigned long long)raised);
}

// ---- diff -----------------------------------------------------------------------------------------------------------------------------
struct DiffArgs {
  const void *a, *b;
  int64_t* out;
  int64_t n;
  int32_t a_scalar, b_scalar, unit, offset;
};

template <bool TS>
__global__ __launch_bounds__(256) void dt_diff_kernel(const DiffArgs A) {
  typedef typename std::conditional<TS, int64_t, int32_t>::type T;
  constexpr int ROWS = 16 / sizeof(T);   // Date: 4 rows, two 16-byte stores
  const int64_t groups = A.n / ROWS;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    T x[ROWS], y[ROWS];
    int64_t r[ROWS];
    map_fetch<T, ROWS>(A.a, std::true_type(), A.a_scalar != 0, g * ROWS, x);
    map_fetch<T, ROWS>(A.b, std::true_type(), A.b_scalar != 0, g * ROWS, y);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
      if constexpr (TS) r[k] = dt_diff_ts(A.unit, x[k], y[k], A.offset);
      else r[k] = dt_diff_date(A.unit, x[k], y[k]);
    }
    map_store<int64_t, ROWS>(A.out, std::true_type(), g * ROWS, r);
  }
  const int64_t i = groups * ROWS + threadIdx.x;
  if (blockIdx.x == 0 && i < A.n) {
    const T x = map_load_one<T>(A.a, A.a_scalar ? 0 : i), y = map_load_one<T>(A.b, A.b_scalar ? 0 : i);
    if constexpr (TS) map_store_one<int64_t>(A.out, i, dt_diff_ts(A.unit, x, y, A.offset));
    else map_store_one<int64_t>(A.out, i, dt_diff_date(A.unit, x, y));
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
bool dt_is_temporal(int32_t t) { return t == DBHIP_T_DATE || t == DBHIP_T_TIMESTAMP; }

// checks a dbhip_tz (NULL = UTC); *offset = the offset before the first transition
int32_t dt_check_tz(const dbhip_tz* tz, const char* who, int32_t* offset) {
  *offset = 0;
  if (!tz) return DBHIP_OK;
  if (tz->offset_s > DT_MAX_OFFSET_S || tz->offset_s < -DT_MAX_OFFSET_S) { set_error("%s: the offset %d s lies outside +-64800", who, tz->offset_s); return DBHIP_ERR_INVALID; }
  if (tz->n_transitions < 0 || tz->n_transitions > DT_MAX_TRANSITIONS) { set_error("%s: %d transitions (0..512)", who, tz->n_transitions); return DBHIP_ERR_INVALID; }
  if (tz->n_transitions > 0 && (!tz->at_utc_s || !tz->offset_after_s)) { set_error("%s: a transition table without its arrays", who); return DBHIP_ERR_INVALID; }
  for (int32_t i = 0; i < tz->n_transitions; ++i) {
    if (i > 0 && tz->at_utc_s[i] <= tz->at_utc_s[i - 1]) { set_error("%s: the transition times are not strictly ascending at entry %d", who, i); return DBHIP_ERR_INVALID; }
    if (tz->offset_after_s[i] > DT_MAX_OFFSET_S || tz->offset_after_s[i] < -DT_MAX_OFFSET_S) { set_error("%s: the offset of transition %d lies outside +-64800", who, i); return DBHIP_ERR_INVALID; }
  }
  *offset = tz->offset_s;
  return DBHIP_OK;
}
// trunc, add and diff go from local time back to UTC, which a transition table does not define everywhere
int32_t dt_fixed_offset_only(const dbhip_tz* tz, const char* who) {
  if (tz && tz->n_transitions > 0) { set_error("%s: a time zone with transitions is not supported here: keep the CPU closure", who); return DBHIP_ERR_UNSUPPORTED; }
  return DBHIP_OK;
}
bool dt_aligned(const dbhip_col* c) { return c->is_scalar || ((uintptr_t)c->data & 15) == 0; }

}  // namespace

extern "C" {

int32_t dbhip_dt_part_type(int32_t part, int32_t src_type) {
  if (part < 0 || part >= DTP_COUNT || !dt_is_temporal(src_type)) return -1;
  if (src_type == DBHIP_T_DATE && dt_part_needs_time(part)) return -1;
  if (part == DTP_EPOCH_SECOND) return DBHIP_T_I64;
  if (part == DTP_DATE) return DBHIP_T_DATE;
  switch (dt_part_bytes(part)) {
    case 1: return DBHIP_T_U8;
    case 2: return DBHIP_T_U16;
    case 4: return DBHIP_T_U32;
    default: return DBHIP_T_U64;
  }
}

int32_t dbhip_dt_part(int32_t part, const dbhip_col* src, const dbhip_tz* tz, int64_t n, void* out, void* stream) {
  DBHIP_REQUIRE(src && n >= 0, "dbhip_dt_part: NULL column or negative n");
  if (dbhip_dt_part_type(part, src->type) < 0) {
    set_error("dbhip_dt_part: part %d of a column of type %d (Date / Timestamp columns; the time parts need a Timestamp)", part, src->type);
    return DBHIP_ERR_INVALID;
  }
  int32_t offset;
  const int32_t rc = dt_check_tz(tz, "dbhip_dt_part", &offset);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(src->data && out, "dbhip_dt_part: NULL data or out");
  DBHIP_REQUIRE(((uintptr_t)out & 15) == 0 && dt_aligned(src), "dbhip_dt_part: data and out must be 16-byte aligned");
  hipStream_t s = resolve_stream(stream);
  const bool ts = src->type == DBHIP_T_TIMESTAMP;
  const bool table = ts && tz && tz->n_transitions > 0;
  MapArgs A;
  memset(&A, 0, sizeof(A));
  A.in = src->data; A.out = out; A.n = n; A.scalar = src->is_scalar; A.code = part; A.offset = ts ? offset : 0;
  if (table) {
    uint8_t* ws = (uint8_t*)scratch((size_t)DT_MAX_TRANSITIONS * 12, DT_SCRATCH_SLOT, s);
    if (!ws) return DBHIP_ERR_HIP;
    A.n_transitions = tz->n_transitions;
    A.at_utc_s = (const int64_t*)ws;
    A.offset_after_s = (const int32_t*)(ws + (size_t)DT_MAX_TRANSITIONS * 8);
    DBHIP_CHECK(hipMemcpyAsync(ws, tz->at_utc_s, (size_t)tz->n_transitions * 8, hipMemcpyHostToDevice, s));
    DBHIP_CHECK(hipMemcpyAsync(ws + (size_t)DT_MAX_TRANSITIONS * 8, tz->offset_after_s, (size_t)tz->n_transitions * 4, hipMemcpyHostToDevice, s));
    DBHIP_POLL_CANCEL(s, "dbhip_dt_part");
  }
  int32_t lrc = DBHIP_ERR_INVALID;
  switch (part) {
#define DT_PART_CASE(P) case P: lrc = launch_part<P>(ts, table, A, s); break;
    DT_PART_CASE(0) DT_PART_CASE(1) DT_PART_CASE(2) DT_PART_CASE(3) DT_PART_CASE(4) DT_PART_CASE(5) DT_PART_CASE(6) DT_PART_CASE(7)
    DT_PART_CASE(8) DT_PART_CASE(9) DT_PART_CASE(10) DT_PART_CASE(11) DT_PART_CASE(12) DT_PART_CASE(13) DT_PART_CASE(14)
    DT_PART_CASE(15) DT_PART_CASE(16) DT_PART_CASE(17) DT_PART_CASE(18)
#undef DT_PART_CASE
    default: break;
  }
  if (lrc) return lrc;
  if (table) DBHIP_CHECK(hipStreamSynchronize(s));   // the table came from caller-owned pageable memory
  return DBHIP_OK;
}

int32_t dbhip_dt_trunc(int32_t unit, int32_t flags, const dbhip_col* src, int32_t out_type, const dbhip_tz* tz, int64_t n, void* out, void* stream) {
  DBHIP_REQUIRE(src && n >= 0, "dbhip_dt_trunc: NULL column or negative n");
  DBHIP_REQUIRE(unit >= 0 && unit < DTU_COUNT && (flags & ~DTF_WEEK_SUNDAY) == 0, "dbhip_dt_trunc: unknown unit or flag bits");
  DBHIP_REQUIRE(dt_is_temporal(src->type) && dt_is_temporal(out_type), "dbhip_dt_trunc: the source and the output are Date or Timestamp");
  DBHIP_REQUIRE(unit <= DTU_DAY || (src->type == DBHIP_T_TIMESTAMP && out_type == DBHIP_T_TIMESTAMP),
                "dbhip_dt_trunc: HOUR, MINUTE and SECOND need a Timestamp source and a Timestamp output");
  int32_t offset;
  int32_t rc = dt_check_tz(tz, "dbhip_dt_trunc", &offset);
  if (rc) return rc;
  rc = dt_fixed_offset_only(tz, "dbhip_dt_trunc");
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(src->data && out, "dbhip_dt_trunc: NULL data or out");
  DBHIP_REQUIRE(((uintptr_t)out & 15) == 0 && dt_aligned(src), "dbhip_dt_trunc: data and out must be 16-byte aligned");
  hipStream_t s = resolve_stream(stream);
  MapArgs A;
  memset(&A, 0, sizeof(A));
  A.in = src->data; A.out = out; A.n = n; A.scalar = src->is_scalar; A.code = unit; A.flags = flags; A.offset = offset;
  const bool ts_in = src->type == DBHIP_T_TIMESTAMP, ts_out = out_type == DBHIP_T_TIMESTAMP;
  if (ts_in) return ts_out ? launch_map<TruncOp<true, true>>(A, s) : launch_map<TruncOp<true, false>>(A, s);
  return ts_out ? launch_map<TruncOp<false, true>>(A, s) : launch_map<TruncOp<false, false>>(A, s);
}

int32_t dbhip_dt_add(int32_t unit, const dbhip_col* src, const dbhip_col* delta, const dbhip_tz* tz, int64_t n, void* out, uint8_t* err_bitmap,
                     uint64_t* err_count_dev, void* stream) {
  DBHIP_REQUIRE(src && delta && n >= 0, "dbhip_dt_add: NULL column or negative n");
  DBHIP_REQUIRE(unit >= 0 && unit < DTU_COUNT, "dbhip_dt_add: unknown unit");
  DBHIP_REQUIRE(dt_is_temporal(src->type) && delta->type == DBHIP_T_I64, "dbhip_dt_add: a Date or Timestamp column and an Int64 delta");
  DBHIP_REQUIRE(unit <= DTU_DAY || src->type == DBHIP_T_TIMESTAMP, "dbhip_dt_add: HOUR, MINUTE and SECOND need a Timestamp (cast the Date first)");
  int32_t offset;
  int32_t rc = dt_check_tz(tz, "dbhip_dt_add", &offset);
  if (rc) return rc;
  rc = dt_fixed_offset_only(tz, "dbhip_dt_add");
  if (rc) return rc;
  if (n > 0) {   // every refusal comes before the first thing queued on the stream
    DBHIP_REQUIRE(src->data && delta->data && out, "dbhip_dt_add: NULL data or out");
    DBHIP_REQUIRE(((uintptr_t)out & 15) == 0 && dt_aligned(src) && dt_aligned(delta), "dbhip_dt_add: data and out must be 16-byte aligned");
  }
  hipStream_t s = resolve_stream(stream);
  if (err_bitmap) DBHIP_CHECK(hipMemsetAsync(err_bitmap, 0xFF, (size_t)ceil_div(n, 32) * 4, s));
  if (n == 0) return DBHIP_OK;
  AddArgs A;
  memset(&A, 0, sizeof(A));
  A.src = src->data; A.delta = (const int64_t*)delta->data; A.out = out; A.n = n;
  A.src_valid = src->validity; A.src_voff = src->validity_offset; A.delta_valid = delta->validity; A.delta_voff = delta->validity_offset;
  A.src_scalar = src->is_scalar; A.delta_scalar = delta->is_scalar; A.unit = unit; A.offset = offset;
  A.err_words = (uint32_t*)err_bitmap; A.err_count = (unsigned long long*)err_count_dev;
  const bool ts = src->type == DBHIP_T_TIMESTAMP;
  const int grid = grid_for(n / (ts ? 2 : 4), 256);
  if (ts) hipLaunchKernelGGL(dt_add_kernel<true>, dim3(grid), dim3(256), 0, s, A);
  else hipLaunchKernelGGL(dt_add_kernel<false>, dim3(grid), dim3(256), 0, s, A);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

int32_t dbhip_dt_diff(int32_t unit, const dbhip_col* a, const dbhip_col* b, const dbhip_tz* tz, int64_t n, int64_t* out, void* stream) {
  DBHIP_REQUIRE(a && b && n >= 0, "dbhip_dt_diff: NULL column or negative n");
  DBHIP_REQUIRE(unit >= 0 && unit < DTU_COUNT, "dbhip_dt_diff: unknown unit");
  DBHIP_REQUIRE(dt_is_temporal(a->type) && a->type == b->type, "dbhip_dt_diff: two Date or two Timestamp columns");
  DBHIP_REQUIRE(unit <= DTU_DAY || a->type == DBHIP_T_TIMESTAMP, "dbhip_dt_diff: HOUR, MINUTE and SECOND need Timestamps");
  int32_t offset;
  int32_t rc = dt_check_tz(tz, "dbhip_dt_diff", &offset);
  if (rc) return rc;
  rc = dt_fixed_offset_only(tz, "dbhip_dt_diff");
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(a->data && b->data && out, "dbhip_dt_diff: NULL data or out");
  DBHIP_REQUIRE(((uintptr_t)out & 15) == 0 && dt_aligned(a) && dt_aligned(b), "dbhip_dt_diff: data and out must be 16-byte aligned");
  hipStream_t s = resolve_stream(stream);
  DiffArgs A;
  memset(&A, 0, sizeof(A));
  A.a = a->data; A.b = b->data; A.out = out; A.n = n; A.a_scalar = a->is_scalar; A.b_scalar = b->is_scalar; A.unit = unit; A.offset = offset;
  const bool ts = a->type == DBHIP_T_TIMESTAMP;
  const int grid = grid_for(n / (ts ? 2 : 4), 256);
  if (ts) hipLaunchKernelGGL(dt_diff_kernel<true>, dim3(grid), dim3(256), 0, s, A);
  else hipLaunchKernelGGL(dt_diff_kernel<false>, dim3(grid), dim3(256), 0, s, A);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

}  // extern "C"
