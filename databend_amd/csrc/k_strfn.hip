// k_strfn.hip — String functions (include/dbhip.h a22): length, substr / left / right, trim, concat, upper / lower.
//
// The row logic is dev_strfn.h's (one text for these kernels and for the host checker); this file is the memory side and the
// wave-per-row forms of the same steps.
//   length / slice   pass 1: one lane per row. The view is loaded as one 16-byte vector; an inline value is worked on in registers, a
//            long one through naturally aligned 4-byte loads that each cover a byte of the value (SfValue::byte). A slice result is
//            a view again: 16 B in, 16 B out, and value bytes only where units or pads have to be looked at (byte mode: none, except
//            the first four bytes of a long result that does not start at the value's start, and the bytes of a result that turns
//            inline). A value longer than DBHIP_LIKE_LONG_BYTES that needs a walk is not walked here: its row id goes into the
//            long-row list (dev_longrows.h) and its output is written as zero.
//            pass 2: one wave per listed row (dev_longrows.h). A step is 64 aligned words (256 bytes, dev_strwave.h): every
//            lane marks the unit boundaries (or the pad mismatches) of its four bytes, ballots and popcounts find the k-th one.
//   build    count (u32 bytes per row that go to out_data) -> dbscan::exclusive_scan_u32 -> fill: one lane per row writes the view (a
//            result of up to 12 bytes from registers). The bytes of results of 13 .. DBHIP_LIKE_LONG_BYTES are copied by the row's own
//            wave, one row after the other, 64 neighbouring bytes per step: the rows of a wave lie back to back in out_data, so loads
//            and stores coalesce (a lane that copied its own row byte by byte wrote 64 different cache lines per store). Longer
//            results go through the row list to a wave-per-row copy.
#include <string.h>
#include "dev_common.h"
#include "dev_scan.h"
#include "dev_strfn.h"
#include "dev_strwave.h"
#include "runtime.h"

using namespace dbhip;

static_assert(SF_SUBSTR == DBHIP_STR_SUBSTR && SF_LEFT == DBHIP_STR_LEFT && SF_RIGHT == DBHIP_STR_RIGHT && SF_TRIM_LEADING == DBHIP_STR_TRIM_LEADING &&
              SF_TRIM_TRAILING == DBHIP_STR_TRIM_TRAILING && SF_TRIM_BOTH == DBHIP_STR_TRIM_BOTH && SF_CONCAT == DBHIP_STR_CONCAT &&
              SF_UPPER == DBHIP_STR_UPPER && SF_LOWER == DBHIP_STR_LOWER && SF_LONG_BYTES == DBHIP_LIKE_LONG_BYTES, "dev_strfn.h codes");

namespace {

constexpr int STRFN_SCRATCH_SLOT = 24;

// ---- the wave-per-row forms of dev_strfn.h's steps (the column frame and the word walk they use: dev_strwave.h) -------------------------------
// sf_units for the wave
__device__ __forceinline__ uint32_t wave_units(const WaveWords& W, uint32_t lane) {
  uint32_t acc = 0;
  for (int64_t wb = 0; wb < (int64_t)W.nwords; wb += 64) {
    uint32_t in;
    const uint32_t w = ww_load(W, wb + lane, 0, W.len, in);
    uint32_t bits = noncont4(w) & in;
    if (wb + lane == 0) bits |= 1u << W.lead;            // position 0 is a boundary whatever its byte
    acc += (uint32_t)__popc(bits);
  }
  return (uint32_t)wave_sum_u64(acc);
}
// sf_backward for the wave (m >= 1): the start of the m-th unit from the end
__device__ __forceinline__ bool wave_backward(const WaveWords& W, uint32_t m, uint32_t lane, uint32_t* at) {
  uint32_t rem = m;
  for (int64_t top = W.nwords; top > 0; top -= 64) {     // the words [top - 64, top)
    const int64_t widx = top - 64 + lane;
    uint32_t in;
    const uint32_t w = ww_load(W, widx, 0, W.len, in);
    uint32_t bits = noncont4(w) & in;
    if (widx == 0) bits |= 1u << W.lead;
    Ballots B;
    const uint32_t total = ballots_of(bits, B);
    if (rem <= total) {
      const uint32_t after = ballots_masked(B, lanes_above(lane));
      const bool hit = after < rem && rem <= after + (uint32_t)__popc(bits);
      uint32_t pos = 0, r = rem - after;
      if (hit) {
#pragma unroll
        for (int j = 3; j >= 0; --j)
          if ((bits >> j) & 1u) { if (--r == 0) pos = (uint32_t)(widx * 4 + j - W.lead); }
      }
      const uint64_t hm = __ballot(hit);
      *at = (uint32_t)__shfl((int)pos, __ffsll((unsigned long long)hm) - 1, 64);
      return true;
    }
    rem -= total;
  }
  return false;
}
// sf_plan_range for the wave
__device__ __forceinline__ void wave_plan_range(int32_t op, const SfPlan& p, const WaveWords& W, uint32_t lane, uint32_t* s, uint32_t* e) {
  *s = 0; *e = 0;
  if (p.empty) return;
  uint32_t st = 0;
  if (p.from_end) {
    if (!wave_backward(W, p.back, lane, &st)) {
      if (op != SF_RIGHT) return;
      st = 0;
    }
  } else if (p.front) {
    st = wave_forward(W, 0, p.front, lane);
    if (st >= W.len) return;
  }
  *s = st;
  *e = p.to_end ? W.len : wave_forward(W, st, p.take, lane);
}
// sf_trim_range for the wave (p >= 1, pad in LDS): the first byte that differs from the pad repeated from the start, the last one
// that differs from the pad repeated towards the end; whole pads in front of / behind them go
__device__ __forceinline__ void wave_trim_range(int32_t op, const WaveWords& W, const uint8_t* pad, uint32_t p, uint32_t lane, uint32_t* s, uint32_t* e) {
  uint32_t lo = 0, hi = W.len;
  if (op == SF_TRIM_LEADING || op == SF_TRIM_BOTH) {
    uint32_t q = W.len;
    for (int64_t wb = 0; wb < (int64_t)W.nwords; wb += 64) {
      const int64_t widx = wb + lane;
      uint32_t in, mm = 0;
      const uint32_t w = ww_load(W, widx, 0, W.len, in);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((in >> j) & 1u) {
          const uint32_t pos = (uint32_t)(widx * 4 + j - W.lead);
          if (((w >> (8 * j)) & 0xFFu) != pad[pos % p]) mm |= 1u << j;
        }
      const uint64_t any = __ballot(mm != 0);
      if (any) {
        const uint32_t pos = (uint32_t)(widx * 4 + (__ffs((int)mm) - 1) - W.lead);
        q = (uint32_t)__shfl((int)pos, __ffsll((unsigned long long)any) - 1, 64);
        break;
      }
    }
    lo = (q / p) * p;
  }
  if (op == SF_TRIM_TRAILING || op == SF_TRIM_BOTH) {
    uint32_t q = W.len - lo;
    for (int64_t top = W.nwords; top > 0; top -= 64) {
      const int64_t widx = top - 64 + lane;
      uint32_t in, mm = 0;
      const uint32_t w = ww_load(W, widx, lo, W.len, in);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((in >> j) & 1u) {
          const uint32_t pos = (uint32_t)(widx * 4 + j - W.lead);
          if (((w >> (8 * j)) & 0xFFu) != pad[p - 1 - ((W.len - 1 - pos) % p)]) mm |= 1u << j;
        }
      const uint64_t any = __ballot(mm != 0);
      if (any) {
        const uint32_t pos = (uint32_t)(widx * 4 + (31 - __clz((int)mm)) - W.lead);
        q = W.len - 1 - (uint32_t)__shfl((int)pos, 63 - __clzll((long long)any), 64);
        break;
      }
      if ((top - 64) * 4 - (int64_t)W.lead <= (int64_t)lo) break;     // the step reached the leading cut
    }
    hi = W.len - (q / p) * p;
  }
  *s = lo; *e = hi;
}

// ---- length and slices -------------------------------------------------------------------------------------------------------------------
struct SliceParams {
  StrCol col;
  const int64_t *a, *b;
  uint4* out_views;       // slices
  uint64_t* out_len;      // length
  LongList list;
  int64_t n;
  int32_t op, unit_byte, a_scalar, b_scalar;
  uint32_t pad_len, _pad;
  uint32_t pad[64];
};

__device__ __forceinline__ void pad_stage(const SliceParams& P, uint32_t* s_pad) {   // 256 threads
  if (threadIdx.x < 64) s_pad[threadIdx.x] = P.pad[threadIdx.x];
  __syncthreads();
}

// what a launch does: the instantiations keep the byte-mode slices (no value bytes to look at, nothing to list, no pad) and the byte
// length free of the walks' code
enum { M_LENGTH_BYTE = 0, M_LENGTH_UNIT = 1, M_PLAN_BYTE = 2, M_PLAN_UNIT = 3, M_TRIM = 4 };

template <int MODE>
__global__ __launch_bounds__(256) void strfn_rows_kernel(const SliceParams P) {
  __shared__ uint32_t s_pad[MODE == M_TRIM ? 64 : 1];
  if constexpr (MODE == M_TRIM) pad_stage(P, s_pad);
  constexpr bool unit_byte = MODE == M_LENGTH_BYTE || MODE == M_PLAN_BYTE;
  constexpr bool lists = MODE == M_LENGTH_UNIT || MODE == M_PLAN_UNIT || MODE == M_TRIM;
  const uint32_t lane = threadIdx.x & 63;
  // every lane of a wave runs the same number of rounds (the wave's first row decides), so the ballots see whole waves
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool listed = false;
    if (i < P.n) {
      SfValue v;
      uint32_t index = 0, offset = 0;
      bool null_row;
      const bool usable = str_value(P.col, i, v, index, offset, null_row);
      if constexpr (MODE == M_LENGTH_BYTE || MODE == M_LENGTH_UNIT) {
        uint64_t u = 0;
        if (usable) {
          if (unit_byte) u = v.len;
          else if (v.len > SF_LONG_BYTES) listed = true;
          else u = sf_units(v);
        }
        P.out_len[i] = u;
      } else {
        uint32_t w[4] = {0, 0, 0, 0};
        if (usable) {
          uint32_t s = 0, e = 0;
          if constexpr (MODE != M_TRIM) {
            const SfPlan plan = sf_plan(P.op, v.len, P.a[P.a_scalar ? 0 : i], P.b ? P.b[P.b_scalar ? 0 : i] : 0, P.b != nullptr);
            if (!unit_byte && v.len > SF_LONG_BYTES && sf_plan_walks(plan, unit_byte)) listed = true;
            else sf_plan_range(P.op, plan, v, unit_byte, &s, &e);
          } else if (v.len > SF_LONG_BYTES && P.pad_len > 0) {
            listed = true;
          } else {
            sf_trim_range(P.op, v, (const uint8_t*)s_pad, P.pad_len, &s, &e);
          }
          if (!listed) sf_slice_view(v, index, offset, s, e, w);
        }
        P.out_views[i] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    if constexpr (lists) list_rows(listed, lane, i, P.list);
  }
}

// pass 2: one wave per listed row (a long view that pass 1 has checked, longer than DBHIP_LIKE_LONG_BYTES)
template <bool LENGTH>
__global__ __launch_bounds__(256) void strfn_long_kernel(const SliceParams P) {
  __shared__ uint32_t s_pad[64];
  pad_stage(P, s_pad);
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    const int64_t r = P.col.scalar ? 0 : i;
    const uint4 vw = P.col.views[r];
    const uintptr_t base = (uintptr_t)P.col.buffers[vw.z] + vw.w;
    const WaveWords W = ww_of(base, vw.x);
    if constexpr (LENGTH) {
      const uint32_t u = wave_units(W, lane);
      if (lane == 0) P.out_len[i] = u;
    } else {
      uint32_t s = 0, e = 0;
      if (P.op <= SF_RIGHT) {
        const SfPlan plan = sf_plan(P.op, vw.x, P.a[P.a_scalar ? 0 : i], P.b ? P.b[P.b_scalar ? 0 : i] : 0, P.b != nullptr);
        wave_plan_range(P.op, plan, W, lane, &s, &e);
      } else {
        wave_trim_range(P.op, W, (const uint8_t*)s_pad, P.pad_len, lane, &s, &e);
      }
      if (lane == 0) {
        SfValue v = sf_value(vw.x, vw.y, vw.z, vw.w, (const uint8_t*)base);
        uint32_t w[4];
        sf_slice_view(v, vw.z, vw.w, s, e, w);
        P.out_views[i] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
}

int32_t check_string_col(const dbhip_col* c, const char* who) {
  if (!c || c->type != DBHIP_T_STRING) { set_error("%s: the column must be a String column", who); return DBHIP_ERR_INVALID; }
  return DBHIP_OK;
}
int32_t check_rows(int64_t n, const char* who) {
  if (n < 0 || n > LONGROWS_MAX_ROWS) { set_error("%s: row count outside 0 .. 2^32 - 2", who); return DBHIP_ERR_INVALID; }
  return DBHIP_OK;
}

template <int MODE>
int32_t slice_run(SliceParams& P, hipStream_t s, const char* who) {
  constexpr bool may_list = MODE == M_LENGTH_UNIT || MODE == M_PLAN_UNIT || MODE == M_TRIM;
  constexpr bool LENGTH = MODE == M_LENGTH_BYTE || MODE == M_LENGTH_UNIT;
  if (may_list) {
    uint8_t* ws = (uint8_t*)scratch(long_list_bytes(P.n), STRFN_SCRATCH_SLOT, s);
    if (!ws) return DBHIP_ERR_HIP;
    P.list = long_list_at(ws);
    DBHIP_CHECK(long_list_clear(ws, s));
  }
  hipLaunchKernelGGL(strfn_rows_kernel<MODE>, dim3(grid_for(P.n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  if (may_list) {
    DBHIP_POLL_CANCEL(s, who);
    long_launch(strfn_long_kernel<LENGTH>, P, s);
    DBHIP_LAUNCH_CHECK();
  }
  return DBHIP_OK;
}

// ---- build: concat, upper, lower ---------------------------------------------------------------------------------------------------------
struct BuildParams {
  StrCol arg[SF_MAX_ARGS];
  int32_t nargs, op;
  int64_t n;
  uint32_t* counts;                  // count kernel: bytes of the row that go to out_data (may be NULL)
  unsigned long long* total;         // count kernel: their sum (may be NULL)
  const uint64_t* offsets;           // fill kernel: the scan of counts
  uint4* out_views;
  uint8_t* out_data;
  uint64_t out_data_bytes;
  uint64_t* out_validity;
  unsigned long long *err_count, *non_ascii;
  LongList list;
};

enum { ROW_DEAD = 0, ROW_EMPTY = 1, ROW_TOO_LONG = 2, ROW_OK = 3 };
// what row i is: a NULL argument -> DEAD; an argument that points nowhere -> EMPTY; else its total length
__device__ __forceinline__ int build_row_kind(const BuildParams& P, int64_t i, uint64_t& total) {
  total = 0;
  bool broken = false;
  for (int32_t k = 0; k < P.nargs; ++k) {
    const StrCol& c = P.arg[k];
    const int64_t r = c.scalar ? 0 : i;
    if (c.validity && !bit_get(c.validity, c.voff + r)) return ROW_DEAD;
  }
  for (int32_t k = 0; k < P.nargs; ++k) {
    const StrCol& c = P.arg[k];
    const int64_t r = c.scalar ? 0 : i;
    const uint32_t* vw = (const uint32_t*)(c.views + r);
    const uint32_t len = vw[0];
    if (!sv_is_inline(len) && (vw[2] >= (uint32_t)c.n_buffers || c.buffers[vw[2]] == nullptr)) broken = true;
    total += len;
  }
  if (broken) return ROW_EMPTY;
  return total > 0xFFFFFFFFull ? ROW_TOO_LONG : ROW_OK;
}
// the arguments of a row that build_row_kind has found usable
struct DevArgs {
  const BuildParams& P;
  int64_t i;
  __device__ __forceinline__ SfValue get(int32_t k) const {
    const StrCol& c = P.arg[k];
    const int64_t r = c.scalar ? 0 : i;
    const uint4 vw = c.views[r];
    return sf_value(vw.x, vw.y, vw.z, vw.w, sv_is_inline(vw.x) ? nullptr : (const uint8_t*)c.buffers[vw.z] + vw.w);
  }
};
// The wave copies one row's bytes to dst (they fit: the fill kernel has checked), 64 neighbouring bytes per step; returns whether a
// byte >= 0x80 was among them (wave-uniform).
__device__ __forceinline__ bool wave_copy_row(const BuildParams& P, int64_t row, uint8_t* dst, uint32_t lane) {
  DevArgs args{P, row};
  uint32_t high = 0;
  for (int32_t a = 0; a < P.nargs; ++a) {
    const SfValue v = args.get(a);
    const uint8_t* src = (const uint8_t*)v.base;
    for (uint32_t b = lane; b < v.len; b += 64) {
      const uint32_t c = v.is_inline() ? (v.inline_word(b) & 0xFFu) : (uint32_t)src[b];
      high |= c;
      dst[b] = (uint8_t)sf_map_byte(P.op, c);
    }
    dst += v.len;
  }
  return __ballot((high & 0x80u) != 0) != 0;
}

__global__ __launch_bounds__(256) void strfn_count_kernel(const BuildParams P) {
  uint64_t sum = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * 256) {
    uint64_t total;
    const int kind = build_row_kind(P, i, total);
    const uint32_t c = kind == ROW_OK && total > SV_INLINE_MAX ? (uint32_t)total : 0u;
    if (P.counts) P.counts[i] = c;
    sum += c;
  }
  if (P.total) {      // every lane arrives here: one add per wave
    sum = wave_sum_u64(sum);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(P.total, (unsigned long long)sum);
  }
}

__global__ __launch_bounds__(256) void strfn_fill_kernel(const BuildParams P) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t cap = P.out_data_bytes < 0x100000000ull ? P.out_data_bytes : 0x100000000ull;
  uint32_t errs = 0, highs = 0;
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool listed = false, live = false, coop = false;
    uint64_t dst_off = 0;
    if (i < P.n) {
      uint64_t total;
      const int kind = build_row_kind(P, i, total);
      live = kind != ROW_DEAD;
      uint32_t w[4] = {0, 0, 0, 0};
      if (kind == ROW_TOO_LONG) {
        ++errs;
      } else if (kind == ROW_OK && total > 0) {
        DevArgs args{P, i};
        if (total <= SV_INLINE_MAX) {
          SfInlineSink sink{0, 0};
          highs += sf_emit(P.op, args, P.nargs, sink) ? 1u : 0u;
          w[0] = (uint32_t)total; w[1] = (uint32_t)sink.lo; w[2] = (uint32_t)(sink.lo >> 32); w[3] = sink.hi;
        } else {
          const uint64_t off = P.offsets[i];
          if (off + total > cap) {
            ++errs;
          } else {
            w[0] = (uint32_t)total; w[2] = 0; w[3] = (uint32_t)off;
            uint32_t got = 0;      // the first four bytes; the bytes themselves are copied by the wave, below or in the next pass
            for (int32_t k = 0; k < P.nargs && got < 4; ++k) {
              SfValue v = args.get(k);
              for (uint32_t b = 0; b < v.len && got < 4; ++b) w[1] |= sf_map_byte(P.op, v.byte(b)) << (8 * got++);
            }
            if (total <= SF_LONG_BYTES) { coop = true; dst_off = off; }
            else listed = true;
          }
        }
      }
      P.out_views[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // results of 13 .. DBHIP_LIKE_LONG_BYTES bytes: the wave copies its rows one after the other, so that neighbouring lanes read and
    // write neighbouring bytes (the rows of a wave lie back to back in out_data)
    for (uint64_t cm = __ballot(coop); cm; cm &= cm - 1) {
      const int l = __ffsll((unsigned long long)cm) - 1;
      const uint64_t at = __shfl(dst_off, l, 64);
      if (wave_copy_row(P, wave0 + l, P.out_data + at, lane) && lane == 0) ++highs;
    }
    const uint64_t lives = __ballot(live);
    if (P.out_validity && lane == 0) P.out_validity[wave0 >> 6] = lives;    // bits past n are 0: those lanes are not live
    list_rows(listed, lane, i, P.list);
  }
  // every lane arrives here: one add per wave and counter
  errs = (uint32_t)wave_sum_u64(errs);
  highs = (uint32_t)wave_sum_u64(highs);
  if (lane == 0 && errs && P.err_count) atomicAdd(P.err_count, (unsigned long long)errs);
  if (lane == 0 && highs && P.non_ascii) atomicAdd(P.non_ascii, (unsigned long long)highs);
}

// one wave per listed row: its bytes fit (the fill kernel has checked), the result is longer than DBHIP_LIKE_LONG_BYTES
__global__ __launch_bounds__(256) void strfn_copy_kernel(const BuildParams P) {
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  uint32_t highs = 0;
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    if (wave_copy_row(P, i, P.out_data + P.offsets[i], lane) && lane == 0) ++highs;
  }
  if (lane == 0 && highs && P.non_ascii) atomicAdd(P.non_ascii, (unsigned long long)highs);
}

int32_t build_params(int32_t op, const dbhip_col* args, int32_t nargs, int64_t n, BuildParams& P, const char* who) {
  if (op < 0 || op >= SF_BUILD_COUNT) { set_error("%s: unknown op %d", who, op); return DBHIP_ERR_INVALID; }
  if (!args || nargs < 1 || nargs > (op == SF_CONCAT ? SF_MAX_ARGS : 1)) {
    set_error("%s: %d arguments (concat takes 1 to 8, upper and lower exactly 1)", who, nargs);
    return DBHIP_ERR_INVALID;
  }
  int32_t rc = check_rows(n, who);
  if (rc) return rc;
  memset(&P, 0, sizeof(P));
  for (int32_t k = 0; k < nargs; ++k) {
    rc = check_string_col(&args[k], who);
    if (rc) return rc;
    if (n > 0 && (!args[k].data || ((uintptr_t)args[k].data & 15))) { set_error("%s: NULL views or views not 16-byte aligned", who); return DBHIP_ERR_INVALID; }
    P.arg[k] = str_col(&args[k]);
  }
  P.nargs = nargs;
  P.op = op;
  P.n = n;
  return DBHIP_OK;
}

}  // namespace

extern "C" {

int32_t dbhip_str_length(const dbhip_col* col, int32_t flags, int64_t n, uint64_t* out, void* stream) {
  const char* who = "dbhip_str_length";
  int32_t rc = check_string_col(col, who);
  if (rc) return rc;
  if (flags & ~DBHIP_STR_UNIT_BYTE) { set_error("%s: unknown flag bits", who); return DBHIP_ERR_INVALID; }
  rc = check_rows(n, who);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  if (!col->data || !out || ((uintptr_t)out & 7) || ((uintptr_t)col->data & 15)) {
    set_error("%s: NULL views or out, views not 16-byte aligned or out not 8-byte aligned", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  SliceParams P;
  memset(&P, 0, sizeof(P));
  P.col = str_col(col);
  P.out_len = out;
  P.n = n;
  P.unit_byte = (flags & DBHIP_STR_UNIT_BYTE) ? 1 : 0;
  return P.unit_byte ? slice_run<M_LENGTH_BYTE>(P, s, who) : slice_run<M_LENGTH_UNIT>(P, s, who);
}

int32_t dbhip_str_slice(int32_t op, const dbhip_col* col, const dbhip_col* a, const dbhip_col* b, const uint8_t* pad_host, int32_t pad_len,
                        int32_t flags, int64_t n, void* out_views, void* stream) {
  const char* who = "dbhip_str_slice";
  int32_t rc = check_string_col(col, who);
  if (rc) return rc;
  if (op < 0 || op >= SF_SLICE_COUNT) { set_error("%s: unknown op %d", who, op); return DBHIP_ERR_INVALID; }
  if (flags & ~DBHIP_STR_UNIT_BYTE) { set_error("%s: unknown flag bits", who); return DBHIP_ERR_INVALID; }
  const bool trim = op >= SF_TRIM_LEADING;
  if (trim) {
    if (pad_len < 0 || (pad_len > 0 && !pad_host)) { set_error("%s: NULL pad or a negative length", who); return DBHIP_ERR_INVALID; }
    if (pad_len > SF_MAX_PAD) { set_error("%s: a pad of more than 255 bytes: keep the CPU closure", who); return DBHIP_ERR_UNSUPPORTED; }
  } else {
    if (!a || a->type != DBHIP_T_I64 || (b && b->type != DBHIP_T_I64)) { set_error("%s: the position and the length are Int64 columns or scalars", who); return DBHIP_ERR_INVALID; }
    if (n > 0 && (!a->data || (b && !b->data))) { set_error("%s: NULL position or length data", who); return DBHIP_ERR_INVALID; }
  }
  rc = check_rows(n, who);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  if (!col->data || !out_views || ((uintptr_t)out_views & 15) || ((uintptr_t)col->data & 15)) {
    set_error("%s: NULL views or out_views, or views not 16-byte aligned", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  SliceParams P;
  memset(&P, 0, sizeof(P));
  P.col = str_col(col);
  P.out_views = (uint4*)out_views;
  P.n = n;
  P.op = op;
  P.unit_byte = (flags & DBHIP_STR_UNIT_BYTE) ? 1 : 0;
  if (trim) {
    P.pad_len = (uint32_t)pad_len;
    if (pad_len) memcpy(P.pad, pad_host, (size_t)pad_len);
    return slice_run<M_TRIM>(P, s, who);
  }
  P.a = (const int64_t*)a->data;
  P.a_scalar = a->is_scalar ? 1 : 0;
  if (op == SF_SUBSTR && b) { P.b = (const int64_t*)b->data; P.b_scalar = b->is_scalar ? 1 : 0; }
  return P.unit_byte ? slice_run<M_PLAN_BYTE>(P, s, who) : slice_run<M_PLAN_UNIT>(P, s, who);
}

int32_t dbhip_str_build_bytes(int32_t op, const dbhip_col* args_host, int32_t nargs, int64_t n, uint64_t* out_bytes_host, void* stream) {
  const char* who = "dbhip_str_build_bytes";
  BuildParams P;
  const int32_t rc = build_params(op, args_host, nargs, n, P, who);
  if (rc) return rc;
  if (!out_bytes_host) { set_error("%s: NULL out_bytes_host", who); return DBHIP_ERR_INVALID; }
  *out_bytes_host = 0;
  if (n == 0) return DBHIP_OK;
  hipStream_t s = resolve_stream(stream);
  uint8_t* ws = (uint8_t*)scratch(64, STRFN_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  P.total = (unsigned long long*)ws;
  DBHIP_CHECK(hipMemsetAsync(ws, 0, 16, s));
  hipLaunchKernelGGL(strfn_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  uint64_t* host = pinned_words(0);
  DBHIP_CHECK(hipMemcpyAsync(host, ws, 8, hipMemcpyDeviceToHost, s));
  DBHIP_CHECK(hipStreamSynchronize(s));
  *out_bytes_host = host[0];
  return DBHIP_OK;
}

int32_t dbhip_str_build(int32_t op, const dbhip_col* args_host, int32_t nargs, int64_t n, void* out_views, uint8_t* out_data, uint64_t out_data_bytes,
                        uint8_t* out_validity, uint64_t* err_count_dev, uint64_t* non_ascii_count_dev, void* stream) {
  const char* who = "dbhip_str_build";
  BuildParams P;
  const int32_t rc = build_params(op, args_host, nargs, n, P, who);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  if (!out_views || ((uintptr_t)out_views & 15) || ((uintptr_t)out_validity & 7) || (out_data_bytes > 0 && !out_data)) {
    set_error("%s: NULL or misaligned out_views, out_validity not 8-byte aligned, or out_data_bytes without out_data", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  // scratch: list count | counts | offsets | block sums | row ids
  const size_t nn = (size_t)n, nblk = (size_t)ceil_div(n, SCAN_TILE) + 2;
  const size_t off_counts = 64, off_offsets = off_counts + ((nn * 4 + 63) & ~(size_t)63), off_blk = off_offsets + nn * 8, off_rows = off_blk + nblk * 8;
  uint8_t* ws = (uint8_t*)scratch(off_rows + nn * 4 + 64, STRFN_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  P.counts = (uint32_t*)(ws + off_counts);
  P.offsets = (const uint64_t*)(ws + off_offsets);
  P.list = long_list_at(ws, 0, off_rows);
  P.out_views = (uint4*)out_views;
  P.out_data = out_data;
  P.out_data_bytes = out_data_bytes;
  P.out_validity = (uint64_t*)out_validity;
  P.err_count = (unsigned long long*)err_count_dev;
  P.non_ascii = (unsigned long long*)non_ascii_count_dev;
  DBHIP_CHECK(long_list_clear(ws, s));
  hipLaunchKernelGGL(strfn_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  const int32_t src = dbscan::exclusive_scan_u32(P.counts, n, (uint64_t*)(ws + off_blk), (uint64_t*)(ws + off_offsets), s);
  if (src) return src;
  DBHIP_POLL_CANCEL(s, who);
  hipLaunchKernelGGL(strfn_fill_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  long_launch(strfn_copy_kernel, P, s);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

}  // extern "C"
