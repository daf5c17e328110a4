// k_strcast.hip — String casts (include/dbhip.h a24): String -> integers / decimals / Date / Timestamp, and those types -> String.
//
// The row logic is dev_strcast.h's (one text for these kernels and for the host checker); this file is the memory side.
//   parse    one launch, one lane per row. The view is loaded as one 16-byte vector; a value of more than DBHIP_STR_PARSE_MAX_BYTES bytes
//            is declined unread, so no lane walks more than 256 bytes: no second pass, no row list, no scratch. The bitmap is written as
//            whole 64-bit words from ballots; the two counters get one add per wave.
//   format   count (u32 bytes per row that go to out_data) -> dbscan::exclusive_scan_u32 -> fill, the protocol of dbhip_str_build. A
//            lane builds its row's text in registers (ScText: eleven words indexed by constants). A result of up to 12 bytes is the
//            view itself. The longer ones of a wave lie back to back in out_data, so the wave assembles them in LDS — each lane ORs its
//            words, shifted to the byte its text starts at, into a zeroed staging area — and then stores the area with whole, aligned
//            words, neighbouring lanes neighbouring words; only the first and the last word of the wave's range, which it shares with
//            the waves next to it, are stored byte by byte.
#include <string.h>
#include "dev_common.h"
#include "dev_scan.h"
#include "dev_strcast.h"
#include "runtime.h"

using namespace dbhip;

static_assert(SC_T_I8 == DBHIP_T_I8 && SC_T_I64 == DBHIP_T_I64 && SC_T_U8 == DBHIP_T_U8 && SC_T_U64 == DBHIP_T_U64 && SC_T_F32 == DBHIP_T_F32 &&
              SC_T_DATE == DBHIP_T_DATE && SC_T_TIMESTAMP == DBHIP_T_TIMESTAMP && SC_T_DEC64 == DBHIP_T_DEC64 && SC_T_DEC128 == DBHIP_T_DEC128 &&
              SC_T_STRING == DBHIP_T_STRING && SC_T_DEC256 == DBHIP_T_DEC256 && SC_T_BOOL == DBHIP_T_BOOL && SC_MAX_BYTES == DBHIP_STR_PARSE_MAX_BYTES &&
              SC_MAX_BYTES <= SF_LONG_BYTES, "dev_strcast.h codes");

namespace {

constexpr int STRCAST_SCRATCH_SLOT = 25;
constexpr int64_t STRCAST_MAX_ROWS = 0xFFFFFFFELL;
constexpr uint32_t STAGE_WORDS = 660;          // per wave: 64 rows of up to 41 bytes behind up to 3 bytes of lead = 2,627 bytes
static_assert(STAGE_WORDS * 4 >= 64 * SC_TEXT_MAX + 3 + 4, "staging area of a wave");

// ---- parse --------------------------------------------------------------------------------------------------------------------------------
struct ParseParams {
  const uint4* views;
  const uint8_t* validity;
  int64_t voff;
  const void* const* buffers;
  int32_t n_buffers, scalar;
  ScSpec spec;
  int32_t is_try;
  int64_t n;
  void* out;
  uint64_t* bitmap;
  unsigned long long *err_count, *declined_count;
};

__device__ __forceinline__ void parse_store(void* out, uint32_t bytes, int64_t i, uint64_t lo, uint64_t hi) {
  switch (bytes) {
    case 1: ((uint8_t*)out)[i] = (uint8_t)lo; break;
    case 2: ((uint16_t*)out)[i] = (uint16_t)lo; break;
    case 4: ((uint32_t*)out)[i] = (uint32_t)lo; break;
    case 8: ((uint64_t*)out)[i] = lo; break;
    default: ((uint64_t*)out)[2 * i] = lo; ((uint64_t*)out)[2 * i + 1] = hi; break;
  }
}

__global__ __launch_bounds__(256) void strcast_parse_kernel(const ParseParams P) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t bytes = sc_type_bytes(P.spec.type);
  uint32_t errs = 0, declined = 0;
  // every lane of a wave runs the same number of rounds (the wave's first row decides), so the ballots see whole waves
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool valid = false, bad = false;
    if (i < P.n) {
      const int64_t r = P.scalar ? 0 : i;
      valid = !P.validity || bit_get(P.validity, P.voff + r);
      uint64_t lo = 0, hi = 0;
      if (valid) {
        const uint4 vw = P.views[r];
        const uint8_t* at = nullptr;
        // a long view that points nowhere is the empty value
        const bool usable = sv_bytes_checked(P.views + r, vw.x, vw.z, vw.w, P.buffers, P.n_buffers, &at);
        SfValue v = usable ? sf_value(vw.x, vw.y, vw.z, vw.w, at) : sf_value(0, 0, 0, 0, nullptr);
        const int st = sc_parse(v, P.spec, &lo, &hi);
        if (st == SC_ERROR) { bad = true; errs += P.is_try ? 0u : 1u; }     // (a try_ cast turns the row NULL and raises nothing)
        else if (st == SC_DECLINED) ++declined;
        if (st != SC_OK) { lo = 0; hi = 0; }
      }
      parse_store(P.out, bytes, i, lo, hi);
    }
    if (P.bitmap) {
      // try: the result's validity (bits past n zero); otherwise ones except at the rows that raised
      const uint64_t word = P.is_try ? __ballot(valid && !bad) : ~__ballot(bad);
      if (lane == 0) P.bitmap[wave0 >> 6] = word;
    }
  }
  // every lane arrives here: one add per wave and counter
  errs = (uint32_t)wave_sum_u64(errs);
  declined = (uint32_t)wave_sum_u64(declined);
  if (lane == 0 && errs && P.err_count) atomicAdd(P.err_count, (unsigned long long)errs);
  if (lane == 0 && declined && P.declined_count) atomicAdd(P.declined_count, (unsigned long long)declined);
}

// ---- format -------------------------------------------------------------------------------------------------------------------------------
struct FormatParams {
  const void* data;
  const uint8_t* validity;
  int64_t voff;
  int32_t type, scalar, offset_s;
  uint32_t scale;
  int64_t n;
  uint32_t* counts;                  // count kernel: bytes of the row that go to out_data (may be NULL)
  unsigned long long* total;         // count kernel: their sum (may be NULL)
  const uint64_t* offsets;           // fill kernel: the scan of counts
  uint4* out_views;
  uint8_t* out_data;
  uint64_t out_data_bytes;
  unsigned long long* err_count;
};

// row i's text; false for a NULL row (the text is then empty). *st: SC_OK or SC_ERROR
__device__ __forceinline__ bool format_row(const FormatParams& P, int64_t i, ScText& T, int* st) {
  const int64_t r = P.scalar ? 0 : i;
  *st = SC_OK;
  if (P.validity && !bit_get(P.validity, P.voff + r)) { sc_text_clear(T); return false; }
  uint64_t lo = 0, hi = 0;
  switch (sc_type_bytes(P.type)) {
    case 1: lo = ((const uint8_t*)P.data)[r]; break;
    case 2: lo = ((const uint16_t*)P.data)[r]; break;
    case 4: lo = ((const uint32_t*)P.data)[r]; break;
    case 8: lo = ((const uint64_t*)P.data)[r]; break;
    default: lo = ((const uint64_t*)P.data)[2 * r]; hi = ((const uint64_t*)P.data)[2 * r + 1]; break;   // (8-byte loads: a sliced column's base)
  }
  *st = sc_format(P.type, P.scale, P.offset_s, sc_widen(P.type, lo), hi, T);
  return true;
}

__global__ __launch_bounds__(256) void strcast_count_kernel(const FormatParams P) {
  uint64_t sum = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * 256) {
    ScText T;
    int st;
    format_row(P, i, T, &st);
    const uint32_t c = T.len > SV_INLINE_MAX ? T.len : 0u;
    if (P.counts) P.counts[i] = c;
    sum += c;
  }
  if (P.total) {      // every lane arrives here: one add per wave
    sum = wave_sum_u64(sum);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(P.total, (unsigned long long)sum);
  }
}

__global__ __launch_bounds__(256) void strcast_fill_kernel(const FormatParams P) {
  __shared__ uint32_t s_stage[4][STAGE_WORDS];
  const uint32_t lane = threadIdx.x & 63;
  uint32_t* stage = s_stage[threadIdx.x >> 6];
  const uint64_t cap = P.out_data_bytes < 0x100000000ull ? P.out_data_bytes : 0x100000000ull;
  uint32_t errs = 0;
  // every wave of a block runs the same number of rounds (the block's first row decides): the barriers see whole blocks
  for (int64_t base = (int64_t)blockIdx.x * 256; base < P.n; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    ScText T;
    sc_text_clear(T);
    bool staged = false;
    uint64_t off = 0;
    if (i < P.n) {
      int st;
      const bool live = format_row(P, i, T, &st);
      if (live && st != SC_OK) ++errs;
      if (T.len > SV_INLINE_MAX) {
        off = P.offsets[i];
        if (off + T.len > cap) { ++errs; sc_text_clear(T); }       // it does not fit: the empty view, nothing written
        else staged = true;
      }
      uint32_t w[4];
      sc_text_view(T, (uint32_t)off, w);
      P.out_views[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // the long results of the wave lie back to back in out_data, in lane order: [a0, a1) from the first staged lane to the last
    const uint64_t sm = __ballot(staged);
    uintptr_t a0 = 0, a1 = 0;
    if (sm) {        // wave-uniform
      const uintptr_t mine = (uintptr_t)P.out_data + off;
      a0 = (uintptr_t)__shfl((unsigned long long)mine, __ffsll((unsigned long long)sm) - 1, 64);
      a1 = (uintptr_t)__shfl((unsigned long long)(mine + T.len), 63 - __clzll((long long)sm), 64);
    }
    const uintptr_t b0 = a0 & ~(uintptr_t)3;                        // the staging area's word 0
    uint32_t nwords = sm ? (uint32_t)((a1 - b0 + 3) >> 2) : 0u;
    if (nwords > STAGE_WORDS) nwords = 0;                           // (cannot happen: 64 texts of up to 41 bytes)
    for (uint32_t k = lane; k < nwords; k += 64) stage[k] = 0;
    __syncthreads();
    if (staged && nwords) {
      const uint32_t at = (uint32_t)((uintptr_t)P.out_data + off - b0), k0 = at >> 2, sh = (at & 3u) * 8u;
      if (k0 + SC_TEXT_WORDS + 1 <= STAGE_WORDS) {
        uint32_t prev = 0;
#pragma unroll
        for (uint32_t j = 0; j <= SC_TEXT_WORDS; ++j) {             // the text moved up by `at & 3` bytes: one word more
          const uint32_t cur = j < SC_TEXT_WORDS ? T.w[j] : 0u;
          const uint32_t x = sh ? (cur << sh) | (prev >> (32u - sh)) : cur;
          prev = cur;
          if (x) atomicOr(&stage[k0 + j], x);                      // the bytes behind the text are zero: neighbours are left alone
        }
      }
    }
    __syncthreads();
    for (uint32_t k = lane; k < nwords; k += 64) {
      const uintptr_t a = b0 + 4u * (uintptr_t)k;
      const uint32_t x = stage[k];
      if (a >= a0 && a + 4 <= a1) {
        *(uint32_t*)a = x;
      } else {
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b)
          if (a + b >= a0 && a + b < a1) *(uint8_t*)(a + b) = (uint8_t)(x >> (8u * b));
      }
    }
    __syncthreads();                                                // the next round zeroes the area again
  }
  errs = (uint32_t)wave_sum_u64(errs);
  if (lane == 0 && errs && P.err_count) atomicAdd(P.err_count, (unsigned long long)errs);
}

int32_t check_rows(int64_t n, const char* who) {
  if (n < 0 || n > STRCAST_MAX_ROWS) { set_error("%s: row count outside 0 .. 2^32 - 2", who); return DBHIP_ERR_INVALID; }
  return DBHIP_OK;
}

int32_t format_params(const dbhip_col* src, int32_t offset_s, int64_t n, FormatParams& P, const char* who) {
  if (!src) { set_error("%s: NULL column", who); return DBHIP_ERR_INVALID; }
  if (!sc_supported(src->type)) {
    set_error("%s: a source of type %d (integers, Decimal64 / Decimal128, Date and Timestamp only): keep the CPU closure", who, src->type);
    return DBHIP_ERR_UNSUPPORTED;
  }
  const int32_t rc = check_rows(n, who);
  if (rc) return rc;
  if (offset_s > DT_MAX_OFFSET_S || offset_s < -DT_MAX_OFFSET_S) { set_error("%s: an offset beyond 18 hours", who); return DBHIP_ERR_INVALID; }
  const bool dec = src->type == DBHIP_T_DEC64 || src->type == DBHIP_T_DEC128;
  if (dec && (src->scale > src->precision || src->precision < 1 || src->precision > (src->type == DBHIP_T_DEC64 ? 18 : 38))) {
    set_error("%s: precision %d / scale %d outside the column's decimal class", who, (int)src->precision, (int)src->scale);
    return DBHIP_ERR_INVALID;
  }
  const uint32_t es = sc_type_bytes(src->type);
  if (n > 0 && (!src->data || ((uintptr_t)src->data & ((es > 8 ? 8 : es) - 1)))) { set_error("%s: NULL or misaligned column data", who); return DBHIP_ERR_INVALID; }
  memset(&P, 0, sizeof(P));
  P.data = src->data;
  P.validity = src->validity;
  P.voff = src->validity_offset;
  P.type = src->type;
  P.scalar = src->is_scalar ? 1 : 0;
  P.offset_s = offset_s;
  P.scale = dec ? src->scale : 0;
  P.n = n;
  return DBHIP_OK;
}

}  // namespace

extern "C" {

int32_t dbhip_str_parse(const dbhip_col* src, int32_t dst_type, uint8_t dst_precision, uint8_t dst_scale, int32_t is_try, int32_t rounding_mode,
                        int32_t offset_s, int64_t n, void* out, uint8_t* bitmap, uint64_t* err_count_dev, uint64_t* declined_count_dev, void* stream) {
  const char* who = "dbhip_str_parse";
  if (!src || src->type != DBHIP_T_STRING) { set_error("%s: the column must be a String column", who); return DBHIP_ERR_INVALID; }
  if (!sc_supported(dst_type)) {
    set_error("%s: a target of type %d (integers, Decimal64 / Decimal128, Date and Timestamp only): keep the CPU closure", who, dst_type);
    return DBHIP_ERR_UNSUPPORTED;
  }
  if (dst_type == DBHIP_T_DEC64 || dst_type == DBHIP_T_DEC128) {
    const int32_t want = dst_precision <= 18 ? DBHIP_T_DEC64 : DBHIP_T_DEC128;
    if (dst_precision < 1 || dst_precision > 38 || dst_scale > dst_precision || dst_type != want) {
      set_error("%s: precision %d / scale %d do not belong to the target's decimal class", who, (int)dst_precision, (int)dst_scale);
      return DBHIP_ERR_INVALID;
    }
  }
  int32_t rc = check_rows(n, who);
  if (rc) return rc;
  if (offset_s > DT_MAX_OFFSET_S || offset_s < -DT_MAX_OFFSET_S) { set_error("%s: an offset beyond 18 hours", who); return DBHIP_ERR_INVALID; }
  if (is_try && !bitmap) { set_error("%s: try_ casts need the validity output", who); return DBHIP_ERR_INVALID; }
  if (n == 0) return DBHIP_OK;
  const uint32_t es = sc_type_bytes(dst_type);
  if (!src->data || ((uintptr_t)src->data & 15) || !out || ((uintptr_t)out & (es - 1)) || ((uintptr_t)bitmap & 7)) {
    set_error("%s: NULL views or out, views not 16-byte aligned, out not element-aligned or the bitmap not 8-byte aligned", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  ParseParams P;
  memset(&P, 0, sizeof(P));
  P.views = (const uint4*)src->data;
  P.validity = src->validity;
  P.voff = src->validity_offset;
  P.buffers = src->buffers;
  P.n_buffers = src->buffers && src->n_buffers > 0 ? src->n_buffers : 0;
  P.scalar = src->is_scalar ? 1 : 0;
  P.spec.type = dst_type;
  P.spec.precision = dst_precision;
  P.spec.scale = dst_scale;
  P.spec.rounding = rounding_mode ? 1 : 0;
  P.spec.offset_s = offset_s;
  P.is_try = is_try ? 1 : 0;
  P.n = n;
  P.out = out;
  P.bitmap = (uint64_t*)bitmap;
  P.err_count = (unsigned long long*)err_count_dev;
  P.declined_count = (unsigned long long*)declined_count_dev;
  hipLaunchKernelGGL(strcast_parse_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

int32_t dbhip_str_format_bytes(const dbhip_col* src, int32_t offset_s, int64_t n, uint64_t* out_bytes_host, void* stream) {
  const char* who = "dbhip_str_format_bytes";
  FormatParams P;
  const int32_t rc = format_params(src, offset_s, n, P, who);
  if (rc) return rc;
  if (!out_bytes_host) { set_error("%s: NULL out_bytes_host", who); return DBHIP_ERR_INVALID; }
  *out_bytes_host = 0;
  if (n == 0) return DBHIP_OK;
  hipStream_t s = resolve_stream(stream);
  uint8_t* ws = (uint8_t*)scratch(64, STRCAST_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  P.total = (unsigned long long*)ws;
  DBHIP_CHECK(hipMemsetAsync(ws, 0, 16, s));
  hipLaunchKernelGGL(strcast_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  uint64_t* host = pinned_words(0);
  DBHIP_CHECK(hipMemcpyAsync(host, ws, 8, hipMemcpyDeviceToHost, s));
  DBHIP_CHECK(hipStreamSynchronize(s));
  *out_bytes_host = host[0];
  return DBHIP_OK;
}

int32_t dbhip_str_format(const dbhip_col* src, int32_t offset_s, int64_t n, void* out_views, uint8_t* out_data, uint64_t out_data_bytes,
                         uint64_t* err_count_dev, void* stream) {
  const char* who = "dbhip_str_format";
  FormatParams P;
  const int32_t rc = format_params(src, offset_s, n, P, who);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  if (!out_views || ((uintptr_t)out_views & 15) || (out_data_bytes > 0 && !out_data)) {
    set_error("%s: NULL or misaligned out_views, or out_data_bytes without out_data", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  // scratch: counts | offsets | block sums
  const size_t nn = (size_t)n, nblk = (size_t)ceil_div(n, SCAN_TILE) + 2;
  const size_t off_counts = 64, off_offsets = off_counts + ((nn * 4 + 63) & ~(size_t)63), off_blk = off_offsets + nn * 8;
  uint8_t* ws = (uint8_t*)scratch(off_blk + nblk * 8 + 64, STRCAST_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  P.counts = (uint32_t*)(ws + off_counts);
  P.offsets = (const uint64_t*)(ws + off_offsets);
  P.out_views = (uint4*)out_views;
  P.out_data = out_data;
  P.out_data_bytes = out_data_bytes;
  P.err_count = (unsigned long long*)err_count_dev;
  hipLaunchKernelGGL(strcast_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  const int32_t src_rc = dbscan::exclusive_scan_u32(P.counts, n, (uint64_t*)(ws + off_blk), (uint64_t*)(ws + off_offsets), s);
  if (src_rc) return src_rc;
  DBHIP_POLL_CANCEL(s, who);
  hipLaunchKernelGGL(strcast_fill_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

}  // extern "C"
