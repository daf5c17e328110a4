// k_math.hip — math functions (include/dbhip.h a26): abs, sign, ceil, floor, round, truncate, sqrt over numbers and over
// Decimal64 / Decimal128.
//
// The arithmetic is dev_math.h's (one text for these kernels and the host checker); this file is the memory side. One kernel template,
// a grid-stride map with 256 lanes per workgroup, instantiated per (input type, output type, function class). Each lane owns a run of
// CONSECUTIVE rows sized so that the narrower of input and output moves as whole 16-byte vectors: 16 rows for I8 -> F64 (one dwordx4
// load, eight dwordx4 stores), 4 for I32 -> U32, 2 for F64 -> F64, 1 for Decimal128. The last n mod rows-per-lane rows are done one per
// lane by the first workgroup. A scalar source is read once per lane. The function code, the decoded digits (MtNum) and the decoded
// decimal call (MtDec) travel in the argument struct, so every branch on them is wave-uniform.
// Sliced columns: data and out need only be aligned to their element (a Decimal128 to 8 bytes). A wave-uniform test of each base picks
// the 16-byte form or a per-element form of the load and of the store, independently (as dev_load.h does for its quads). The loop, the
// tail rule and both forms of every access are dev_map.h's map_rows, which k_datetime.hip's kernels use as well.
// No LDS, no scratch memory, no atomics. Validity is not touched: it passes through (the binding reuses the source's Bitmap).
#include <string.h>

#include <type_traits>

#include "dev_map.h"
#include "dev_math.h"
#include "runtime.h"

using namespace dbhip;

static_assert(MT_ABS == DBHIP_MATH_ABS && MT_SIGN == DBHIP_MATH_SIGN && MT_CEIL == DBHIP_MATH_CEIL && MT_FLOOR == DBHIP_MATH_FLOOR &&
              MT_ROUND == DBHIP_MATH_ROUND && MT_TRUNCATE == DBHIP_MATH_TRUNCATE && MT_SQRT == DBHIP_MATH_SQRT, "dev_math.h function codes");

namespace {

struct MathArgs {
  const void* in;
  void* out;
  int64_t n;
  int32_t scalar, _pad;
  MtNum num;
  MtDec dec;
};

// ---- the function classes: In and Out are what moves through memory ------------------------------------------------------------------
template <typename S>
struct AbsIntOp {   // signed iN -> uN
  typedef S In;
  typedef typename std::make_unsigned<S>::type Out;
  static __device__ __forceinline__ Out apply(In v, const MathArgs&) { return mt_abs_int<In, Out>(v); }
};
template <typename U>
struct AbsFloatOp {   // a float column as its bit patterns: the sign bit cleared, a NaN keeps its payload
  typedef U In;
  typedef U Out;
  static __device__ __forceinline__ Out apply(In v, const MathArgs&) {
    if constexpr (sizeof(U) == 4) return mt_abs_f32_bits(v);
    else return mt_abs_f64_bits(v);
  }
};
template <typename T>
struct SignOp {   // any number, Decimal64 (int64_t), Decimal128 (__int128) -> I8
  typedef T In;
  typedef int8_t Out;
  static __device__ __forceinline__ Out apply(In v, const MathArgs&) { return mt_sign<In>(v); }
};
template <typename T>
struct F64Op {   // CEIL, FLOOR, ROUND, TRUNCATE, SQRT of any number -> F64
  typedef T In;
  typedef double Out;
  static __device__ __forceinline__ Out apply(In v, const MathArgs& A) { return mt_num_f64(A.num, (double)v); }
};
template <typename T>
struct DecOp {   // ABS, CEIL, FLOOR, ROUND, TRUNCATE of a decimal: the storage class stays
  typedef T In;
  typedef T Out;
  static __device__ __forceinline__ Out apply(In v, const MathArgs& A) {
    if constexpr (sizeof(T) == 8) return mt_dec64(A.dec, v);
    else return mt_dec128(A.dec, v);
  }
};

// at least 7 waves per SIMD: SignOp<__int128> holds 16 loaded quads and would otherwise take 73 VGPRs, one past the step from 7 to 6
template <typename Op>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7))) void math_map_kernel(const MathArgs A) {
  typedef typename Op::In In;
  typedef typename Op::Out Out;
  // read from the kernel arguments alone: wave-uniform
  const bool in_vec = ((unsigned long long)A.in & 15) == 0, out_vec = ((unsigned long long)A.out & 15) == 0;
  map_rows<In, Out>(A.in, in_vec, A.scalar != 0, A.out, out_vec, A.n, [&A](In v) { return Op::apply(v, A); });
}

template <typename Op>
int32_t launch_map(const MathArgs& A, hipStream_t s) {
  hipLaunchKernelGGL(math_map_kernel<Op>, dim3(map_grid<typename Op::In, typename Op::Out>(A.n)), dim3(256), 0, s, A);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

// Op<T> for the number type t
template <template <typename> class Op>
int32_t launch_number(int32_t t, const MathArgs& A, hipStream_t s) {
  switch (t) {
    case DBHIP_T_I8: return launch_map<Op<int8_t>>(A, s);
    case DBHIP_T_I16: return launch_map<Op<int16_t>>(A, s);
    case DBHIP_T_I32: return launch_map<Op<int32_t>>(A, s);
    case DBHIP_T_I64: return launch_map<Op<int64_t>>(A, s);
    case DBHIP_T_U8: return launch_map<Op<uint8_t>>(A, s);
    case DBHIP_T_U16: return launch_map<Op<uint16_t>>(A, s);
    case DBHIP_T_U32: return launch_map<Op<uint32_t>>(A, s);
    case DBHIP_T_U64: return launch_map<Op<uint64_t>>(A, s);
    case DBHIP_T_F32: return launch_map<Op<float>>(A, s);
    case DBHIP_T_F64: return launch_map<Op<double>>(A, s);
    default: return DBHIP_ERR_INVALID;
  }
}

bool is_signed_int(int32_t t) { return t >= DBHIP_T_I8 && t <= DBHIP_T_I64; }
bool is_unsigned_int(int32_t t) { return t >= DBHIP_T_U8 && t <= DBHIP_T_U64; }
bool is_number(int32_t t) { return t >= DBHIP_T_I8 && t <= DBHIP_T_F64; }

}  // namespace

extern "C" {

int32_t dbhip_math_result(int32_t fn, int32_t src_type, uint8_t src_precision, uint8_t src_scale, int32_t digits, int32_t* out_type_host,
                          uint8_t* out_precision_host, uint8_t* out_scale_host) {
  DBHIP_REQUIRE(out_type_host && out_precision_host && out_scale_host, "dbhip_math_result: NULL output pointer");
  DBHIP_REQUIRE(fn >= 0 && fn < MT_FN_COUNT, "dbhip_math_result: unknown function");
  *out_precision_host = 0;
  *out_scale_host = 0;
  if (is_number(src_type)) {
    if (fn == MT_ABS) {
      DBHIP_REQUIRE(!is_unsigned_int(src_type), "dbhip_math_result: abs of an unsigned column is the identity: pass the column through");
      *out_type_host = is_signed_int(src_type) ? src_type + (DBHIP_T_U8 - DBHIP_T_I8) : src_type;
    } else {
      *out_type_host = fn == MT_SIGN ? DBHIP_T_I8 : DBHIP_T_F64;
    }
    return DBHIP_OK;
  }
  if (src_type == DBHIP_T_DEC256) {   // for every function, SQRT included
    set_error("dbhip_math_result: Decimal256 sources are not supported: keep the CPU closure");
    return DBHIP_ERR_UNSUPPORTED;
  }
  if (src_type == DBHIP_T_DEC64 || src_type == DBHIP_T_DEC128) {
    DBHIP_REQUIRE(fn != MT_SQRT, "dbhip_math_result: sqrt of a decimal is not defined here: cast the column to Float64 first");
    const int max_p = src_type == DBHIP_T_DEC64 ? 18 : 38;
    DBHIP_REQUIRE(src_precision >= 1 && src_precision <= max_p && src_scale <= src_precision,
                  "dbhip_math_result: the precision must be 1..18 (Decimal64) / 1..38 (Decimal128) and the scale at most the precision");
    if (fn == MT_SIGN) {
      *out_type_host = DBHIP_T_I8;
      return DBHIP_OK;
    }
    *out_type_host = src_type;
    *out_precision_host = src_precision;
    *out_scale_host = (uint8_t)mt_dec_result_scale(fn, src_scale, digits);
    return DBHIP_OK;
  }
  set_error("dbhip_math_result: a source of type %d (numbers, Decimal64 and Decimal128 only)", src_type);
  return DBHIP_ERR_INVALID;
}

int32_t dbhip_math(int32_t fn, const dbhip_col* src, int32_t digits, int64_t n, void* out, void* stream) {
  DBHIP_REQUIRE(src && n >= 0, "dbhip_math: NULL column or negative n");
  int32_t out_type;
  uint8_t out_p, out_s;
  const int32_t rc = dbhip_math_result(fn, src->type, src->precision, src->scale, digits, &out_type, &out_p, &out_s);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(src->data && out, "dbhip_math: NULL data or out");
  const int32_t t = src->type;
  const bool dec = t == DBHIP_T_DEC64 || t == DBHIP_T_DEC128;
  // element alignment (a Decimal128 to 8 bytes); nothing more is asked, so a slice at any row is accepted
  const uintptr_t in_mask = (uintptr_t)(t == DBHIP_T_DEC128 ? 8 : type_size(t)) - 1;
  const uintptr_t out_mask = (uintptr_t)(out_type == DBHIP_T_DEC128 ? 8 : type_size(out_type)) - 1;
  DBHIP_REQUIRE(((uintptr_t)src->data & in_mask) == 0 && ((uintptr_t)out & out_mask) == 0, "dbhip_math: data and out must be aligned to their element");
  hipStream_t s = resolve_stream(stream);
  MathArgs A;
  memset(&A, 0, sizeof(A));
  A.in = src->data; A.out = out; A.n = n; A.scalar = src->is_scalar;
  A.num = mt_num_decode(fn, digits);
  if (fn == MT_SIGN) {
    if (t == DBHIP_T_DEC64) return launch_map<SignOp<int64_t>>(A, s);
    if (t == DBHIP_T_DEC128) return launch_map<SignOp<mt_i128>>(A, s);
    return launch_number<SignOp>(t, A, s);
  }
  if (dec) {
    A.dec = mt_dec_decode(fn, src->precision, src->scale, digits);
    return t == DBHIP_T_DEC64 ? launch_map<DecOp<int64_t>>(A, s) : launch_map<DecOp<mt_i128>>(A, s);
  }
  if (fn == MT_ABS) {
    switch (t) {
      case DBHIP_T_I8: return launch_map<AbsIntOp<int8_t>>(A, s);
      case DBHIP_T_I16: return launch_map<AbsIntOp<int16_t>>(A, s);
      case DBHIP_T_I32: return launch_map<AbsIntOp<int32_t>>(A, s);
      case DBHIP_T_I64: return launch_map<AbsIntOp<int64_t>>(A, s);
      case DBHIP_T_F32: return launch_map<AbsFloatOp<uint32_t>>(A, s);
      default: return launch_map<AbsFloatOp<uint64_t>>(A, s);
    }
  }
  return launch_number<F64Op>(t, A, s);
}

}  // extern "C"
