// k_array.hip — Array functions (include/dbhip.h a29): length, get, contains / indexof, count / sum / min / max, the unnest selection.
//
// The row logic is dev_array.h's (one text for these kernels and for the host checker); this file is the memory side. Two tiers, as in
// k_strfn.hip and k_strsearch.hip:
//   short rows  one wave takes 64 consecutive rows. Their runs are one contiguous range of the child (gaps only where a long or a bad
//            row lies), so the wave loads that range itself: every lane holds a cursor into its own run, the wave takes the smallest
//            cursor c0, stages the child's bytes from c0 on (AR_STAGE_BYTES, from the 16-byte boundary at or below c0, 16-byte loads
//            wherever the 16 bytes lie inside the child) and the validity bits that go with them in LDS, and every lane folds or
//            searches the part of its run that lies in the stage, out of LDS. The lane with the smallest cursor advances, so the
//            loop ends. A row of more than AR_LONG_LEN elements is not touched: its id goes into the long-row list (dev_longrows.h)
//            and its output is written as zero.
//   long rows   one wave per listed row (dev_longrows.h), AR_WAVE_STEP elements per step loaded
//            straight from the child (neighbouring lanes, neighbouring elements); the parts are folded with shuffles, the first match is
//            the lowest bit of a ballot.
//   get and length are maps with one lane per row; unnest_sel stages ROW IDS in LDS the same way (a lane writes its run's slots, the
//            wave copies the stage out in order) and writes a long row's run with the whole wave.
// A bad row (offsets that decrease or end past n_elems) is an empty run in every kernel; nothing is read through it. No loop waits for
// another wave.
#include <string.h>
#include "dev_common.h"
#include "dev_array.h"
#include "dev_longrows.h"
#include "runtime.h"

using namespace dbhip;

static_assert(AR_COUNT == DBHIP_ARR_COUNT && AR_SUM == DBHIP_ARR_SUM && AR_MIN == DBHIP_ARR_MIN && AR_MAX == DBHIP_ARR_MAX &&
              AR_CONTAINS == DBHIP_ARR_CONTAINS && AR_INDEXOF == DBHIP_ARR_INDEXOF, "dev_array.h codes");
static_assert(AR_COUNT == DBHIP_AGG_COUNT && AR_SUM == DBHIP_AGG_SUM && AR_MIN == DBHIP_AGG_MIN && AR_MAX == DBHIP_AGG_MAX, "the kinds are dbhip_agg_kind's");
static_assert(AR_T_BOOL == DBHIP_T_BOOL && AR_T_I8 == DBHIP_T_I8 && AR_T_I64 == DBHIP_T_I64 && AR_T_U8 == DBHIP_T_U8 && AR_T_U64 == DBHIP_T_U64 &&
              AR_T_F32 == DBHIP_T_F32 && AR_T_F64 == DBHIP_T_F64 && AR_T_DATE == DBHIP_T_DATE && AR_T_TIMESTAMP == DBHIP_T_TIMESTAMP &&
              AR_T_DEC64 == DBHIP_T_DEC64 && AR_T_DEC128 == DBHIP_T_DEC128 && AR_T_STRING == DBHIP_T_STRING && AR_T_DEC256 == DBHIP_T_DEC256,
              "dev_array.h types");
static_assert(AR_LONG_LEN == DBHIP_ARRAY_LONG_LEN && AR_WAVE_STEP == DBHIP_WAVE && AR_STAGE_BYTES % 16 == 0, "a step is one element per lane");

namespace {

constexpr int AR_SCRATCH_SLOT = 28;
constexpr uint32_t AR_NO_ROW = 0xFFFFFFFFu;    // an empty slot of unnest's stage (a row id is at most 2^32 - 3)
constexpr uint32_t AR_STAGE_SLOTS = AR_STAGE_BYTES / 4;
constexpr int AR_LONG_UNROLL = 4;              // steps of the wave-per-row pass whose loads are issued together

struct ArParams {
  const uint64_t* offsets;
  int64_t n;
  uint64_t n_elems;
  const uint8_t* data;               // the child's values
  const uint8_t* validity;           // its validity, read from bit voff
  int64_t voff;
  const void* const* buffers;        // a String child's buffer table
  int32_t n_buffers, es, op, mode;   // es: bytes per element; op: the kind / find op; mode: AR_EQ_*
  const uint8_t* nd_data;            // find: the needle (one value when nd_scalar)
  const uint8_t* nd_validity;
  int64_t nd_voff;
  int32_t nd_scalar, out_es;
  void* out;
  unsigned long long* out_words;     // the validity / CONTAINS Bitmap, as words
  unsigned long long* err_count;
  LongList list;
  uint32_t* out_sel;
  uint64_t num_out;
  uint32_t nd_len, _pad;
  uint8_t nd[256];                   // find_str: the needle's bytes
};

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint64_t o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
// what one wave wrote to its LDS stage is visible to its own lanes behind this
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ bool elem_valid(const ArParams& P, uint64_t e) { return !P.validity || bit_get(P.validity, P.voff + (int64_t)e); }

// ---- the short-row pass: the wave's stage -------------------------------------------------------------------------------------------------
struct Stage {
  uint4 data[AR_STAGE_BYTES / 16];
  uint8_t bits[AR_STAGE_BYTES / 8 + 8];        // one bit per element of the smallest size, and the bits in front of the first
};
// The rows' elements from the smallest cursor on. Op: elem(the stage's first element, the element's index in the stage, its position in
// the run, valid) -> whether the lane goes on. Every lane of the wave calls this, with len = 0 when it has no run.
template <class Op>
__device__ __forceinline__ void wave_runs(const ArParams& P, Stage& S, uint32_t lane, uint64_t start, uint64_t len, Op& op) {
  const uint32_t es = (uint32_t)P.es;
  const uintptr_t lo = (uintptr_t)P.data, hi = lo + P.n_elems * es;
  uint64_t cur = start;
  const uint64_t end = start + len;
  for (;;) {
    const uint64_t c0 = wave_min_u64(cur < end ? cur : ~0ull);
    if (c0 == ~0ull) break;                                  // wave-uniform
    const uintptr_t a0 = lo + c0 * es, a0a = a0 & ~(uintptr_t)15;
    const uint32_t lead = (uint32_t)(a0 - a0a);              // a multiple of es: the child is es-aligned and es divides 16
    uint64_t c1 = c0 + (AR_STAGE_BYTES - lead) / es;
    const uint64_t last = wave_max_u64(cur < end ? end : 0);  // where the last unfinished run of the wave ends (<= n_elems: the runs are good)
    c1 = c1 < last ? c1 : last;
    const uint32_t groups = (uint32_t)((lead + (c1 - c0) * es + 15) >> 4);
    for (uint32_t g = lane; g < groups; g += 64) {
      const uintptr_t a = a0a + 16u * g;
      if (a >= lo && a + 16 <= hi) {
        S.data[g] = *(const uint4*)a;
      } else {                                               // the child's first or last 16 bytes: only what lies inside it
        uint8_t* d = (uint8_t*)&S.data[g];
        for (uint32_t b = 0; b < 16; ++b) d[b] = (a + b >= lo && a + b < hi) ? *(const uint8_t*)(a + b) : (uint8_t)0;
      }
    }
    const uint64_t bit0 = (uint64_t)P.voff + c0;
    const uint32_t blead = (uint32_t)(bit0 & 7);
    if (P.validity) {
      const uint32_t nbytes = (uint32_t)((blead + (c1 - c0) + 7) >> 3);
      for (uint32_t j = lane; j < nbytes; j += 64) S.bits[j] = P.validity[(bit0 >> 3) + j];
    }
    wave_lds_sync();
    if (cur < end && cur < c1) {                             // cur >= c0
      const uint64_t stop = end < c1 ? end : c1;
      const uint8_t* base = (const uint8_t*)S.data + lead;
      for (uint64_t e = cur; e < stop; ++e) {
        const uint32_t at = (uint32_t)(e - c0);
        const bool valid = !P.validity || ((S.bits[(blead + at) >> 3] >> ((blead + at) & 7)) & 1);
        if (!op.elem(base, at, e - start, valid)) { cur = end; break; }
      }
      if (cur < end) cur = stop;
    }
    wave_lds_sync();                                         // the stage is rewritten by the next round
  }
}

// the 64 rows of a wave: the lane's run (empty for a row past n, a bad row and a row left to the wave pass) and whether it is listed
__device__ __forceinline__ void lane_row(const ArParams& P, int64_t i, uint64_t& start, uint64_t& len, bool& listed) {
  start = 0; len = 0; listed = false;
  if (i < P.n && ar_row(P.offsets, i, P.n_elems, &start, &len) && len > AR_LONG_LEN) { listed = true; len = 0; }
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
template <int CLS>
struct ReduceOp {
  int kind, es;
  ArAcc acc;
  __device__ __forceinline__ bool elem(const uint8_t* base, uint32_t at, uint64_t, bool valid) {
    if (valid) ar_fold<CLS>(kind, acc, ar_load(base, at, es, CLS == AR_CLS_I));
    return true;
  }
};
template <int CLS>
__global__ __launch_bounds__(256) void ar_reduce_kernel(const ArParams P) {
  __shared__ Stage stages[4];
  Stage& S = stages[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63;
  uint32_t errs = 0;
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    uint64_t start, len;
    bool listed;
    lane_row(P, i, start, len, listed);
    ReduceOp<CLS> op{P.op, P.es};
    ar_acc_init(op.acc);
    wave_runs(P, S, lane, start, len, op);
    ArBits r;
    bool err;
    bool ok = ar_finish<CLS>(P.op, op.acc, &r, &err);
    if (err) ++errs;
    ok = i < P.n && (P.op == AR_COUNT || (ok && !listed));
    if (i < P.n) ar_store(P.out, (uint64_t)i, P.out_es, r);
    const uint64_t word = __ballot(ok);
    if (lane == 0 && P.out_words) P.out_words[wave0 >> 6] = word;
    list_rows(listed, lane, i, P.list);
  }
  errs = (uint32_t)wave_sum_u64(errs);                       // every lane arrives here: one add per wave
  if (lane == 0 && errs && P.err_count) atomicAdd(P.err_count, (unsigned long long)errs);
}
template <int CLS>
__global__ __launch_bounds__(256) void ar_reduce_long_kernel(const ArParams P) {
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    uint64_t start, len;
    ar_row(P.offsets, i, P.n_elems, &start, &len);           // pass 1 found it good and long
    ArAcc acc;
    ar_acc_init(acc);
    for (uint64_t e0 = 0; e0 < len; e0 += AR_LONG_UNROLL * AR_WAVE_STEP) {    // wave-uniform bounds; the steps' loads are in flight together
      ArBits x[AR_LONG_UNROLL];
      bool ok[AR_LONG_UNROLL];
#pragma unroll
      for (int u = 0; u < AR_LONG_UNROLL; ++u) {
        const uint64_t k = e0 + (uint64_t)u * AR_WAVE_STEP + lane;
        ok[u] = k < len && elem_valid(P, start + k);
        x[u] = ok[u] ? ar_load(P.data, start + k, P.es, CLS == AR_CLS_I) : ArBits{0, 0};
      }
#pragma unroll
      for (int u = 0; u < AR_LONG_UNROLL; ++u)
        if (ok[u]) ar_fold<CLS>(P.op, acc, x[u]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      ArAcc o;
      o.count = __shfl_xor(acc.count, off, 64);
      o.v = ((ar_u128)__shfl_xor((uint64_t)(acc.v >> 64), off, 64) << 64) | __shfl_xor((uint64_t)acc.v, off, 64);
      o.ext = (int64_t)__shfl_xor((uint64_t)acc.ext, off, 64);
      o.f = __shfl_xor(acc.f, off, 64);
      ar_merge<CLS>(P.op, acc, o);
    }
    if (lane == 0) {
      ArBits r;
      bool err;
      const bool ok = ar_finish<CLS>(P.op, acc, &r, &err);
      ar_store(P.out, (uint64_t)i, P.out_es, r);
      if (ok && P.op != AR_COUNT && P.out_words) atomicOr(P.out_words + (i >> 6), 1ull << (i & 63));
      if (err && P.err_count) atomicAdd(P.err_count, 1ull);
    }
  }
}

// ---- find ---------------------------------------------------------------------------------------------------------------------------------
// the needle of row i; false when it is NULL
__device__ __forceinline__ bool needle_of(const ArParams& P, int64_t i, ArBits& nd) {
  const int64_t r = P.nd_scalar ? 0 : i;
  if (P.nd_validity && !bit_get(P.nd_validity, P.nd_voff + r)) return false;
  nd = ar_load(P.nd_data, (uint64_t)r, P.es, false);
  return true;
}
struct FindOp {
  int mode, es;
  ArBits nd;
  uint64_t pos;                      // 1-based, 0: not found
  __device__ __forceinline__ bool elem(const uint8_t* base, uint32_t at, uint64_t k, bool valid) {
    if (valid && ar_eq(mode, ar_load(base, at, es, false), nd)) { pos = k + 1; return false; }
    return true;
  }
};
// a String element against the needle: a view that points nowhere does not match and is not dereferenced
__device__ __forceinline__ bool view_eq(const ArParams& P, const uint4* view, const uint8_t* nd) {
  const uint4 vw = *view;
  const uint8_t* bytes = nullptr;
  if (!sv_bytes_checked(view, vw.x, vw.z, vw.w, P.buffers, P.n_buffers, &bytes)) return false;
  SfValue v = sf_value(vw.x, vw.y, vw.z, vw.w, bytes);
  return ar_str_eq(v, nd, P.nd_len);
}
struct FindStrOp {
  const ArParams& P;
  const uint8_t* nd;
  uint64_t pos;
  __device__ __forceinline__ bool elem(const uint8_t* base, uint32_t at, uint64_t k, bool valid) {
    if (valid && view_eq(P, (const uint4*)base + at, nd)) { pos = k + 1; return false; }
    return true;
  }
};
__device__ __forceinline__ void needle_stage(const ArParams& P, uint8_t* nd) {     // 256 threads
  nd[threadIdx.x] = P.nd[threadIdx.x];
  __syncthreads();
}
// STR: a String child and the constant needle; otherwise a needle column or scalar of the elements' type
template <bool STR>
__global__ __launch_bounds__(256) void ar_find_kernel(const ArParams P) {
  __shared__ Stage stages[4];
  __shared__ uint8_t nd_bytes[256];
  if (STR) needle_stage(P, nd_bytes);
  Stage& S = stages[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63;
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    uint64_t start, len, pos = 0;
    bool listed;
    lane_row(P, i, start, len, listed);
    if (STR) {
      FindStrOp op{P, nd_bytes, 0};
      wave_runs(P, S, lane, start, len, op);
      pos = op.pos;
    } else {
      FindOp op{P.mode, P.es, ArBits{0, 0}, 0};
      if (i < P.n && !needle_of(P, i, op.nd)) { len = 0; listed = false; }       // a NULL needle: 0 / false, and the row is not walked
      wave_runs(P, S, lane, start, len, op);
      pos = op.pos;
    }
    if (P.op == AR_CONTAINS) {
      const uint64_t word = __ballot(pos != 0);
      if (lane == 0) P.out_words[wave0 >> 6] = word;
    } else if (i < P.n) {
      ((uint64_t*)P.out)[i] = pos;
    }
    list_rows(listed, lane, i, P.list);
  }
}
template <bool STR>
__global__ __launch_bounds__(256) void ar_find_long_kernel(const ArParams P) {
  __shared__ uint8_t nd_bytes[256];
  if (STR) needle_stage(P, nd_bytes);
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    uint64_t start, len, pos = 0;
    ar_row(P.offsets, i, P.n_elems, &start, &len);           // pass 1 found it good and long, and its needle not NULL
    ArBits nd{0, 0};
    if (!STR) needle_of(P, i, nd);
    for (uint64_t e0 = 0; e0 < len && !pos; e0 += AR_LONG_UNROLL * AR_WAVE_STEP) {    // wave-uniform bounds; the steps' loads are in flight together
      bool hit[AR_LONG_UNROLL];
#pragma unroll
      for (int u = 0; u < AR_LONG_UNROLL; ++u) {
        const uint64_t k = e0 + (uint64_t)u * AR_WAVE_STEP + lane;
        hit[u] = false;
        if (k < len && elem_valid(P, start + k))
          hit[u] = STR ? view_eq(P, (const uint4*)P.data + start + k, nd_bytes) : ar_eq(P.mode, ar_load(P.data, start + k, P.es, false), nd);
      }
#pragma unroll
      for (int u = 0; u < AR_LONG_UNROLL; ++u) {             // in order: the FIRST match
        const uint64_t hm = __ballot(hit[u]);
        if (hm && !pos) pos = e0 + (uint64_t)u * AR_WAVE_STEP + (uint64_t)(__ffsll((unsigned long long)hm) - 1) + 1;
      }
    }
    if (lane == 0 && pos) {
      if (P.op == AR_CONTAINS) atomicOr(P.out_words + (i >> 6), 1ull << (i & 63));
      else ((uint64_t*)P.out)[i] = pos;
    }
  }
}

// ---- unnest_sel ---------------------------------------------------------------------------------------------------------------------------
// out_sel[k - offsets[0]] = r for the elements k of row r; only slots below num_out are written
__global__ __launch_bounds__(256) void ar_unnest_kernel(const ArParams P) {
  __shared__ uint32_t stages[4][AR_STAGE_SLOTS];
  uint32_t* S = stages[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t o0 = P.offsets[0];
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    uint64_t start, len;
    bool listed;
    lane_row(P, i, start, len, listed);
    if (start < o0) len = 0;                                 // (malformed: a run in front of the first)
    uint64_t cur = start;
    const uint64_t end = start + len;
    for (;;) {
      const uint64_t c0 = wave_min_u64(cur < end ? cur : ~0ull);
      if (c0 == ~0ull) break;                                // wave-uniform
      const uint64_t last = wave_max_u64(cur < end ? end : 0);                   // where the last unfinished run of the wave ends
      const uint32_t span = last - c0 < AR_STAGE_SLOTS ? (uint32_t)(last - c0) : AR_STAGE_SLOTS;
      for (uint32_t j = lane; j < span; j += 64) S[j] = AR_NO_ROW;
      wave_lds_sync();
      if (cur < end && cur - c0 < span) {
        const uint64_t stop = end - c0 < span ? end : c0 + span;
        for (uint64_t e = cur; e < stop; ++e) S[e - c0] = (uint32_t)i;
        cur = stop;
      }
      wave_lds_sync();
      for (uint32_t j = lane; j < span; j += 64) {
        const uint32_t r = S[j];
        const uint64_t k = c0 - o0 + j;
        if (r != AR_NO_ROW && k < P.num_out) P.out_sel[k] = r;
      }
      wave_lds_sync();                                       // the stage is rewritten by the next round
    }
    list_rows(listed, lane, i, P.list);
  }
}
__global__ __launch_bounds__(256) void ar_unnest_long_kernel(const ArParams P) {
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  const uint64_t o0 = P.offsets[0];
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    uint64_t start, len;
    ar_row(P.offsets, i, P.n_elems, &start, &len);
    if (start < o0) continue;
    for (uint64_t e0 = lane; e0 < len; e0 += AR_WAVE_STEP) {
      const uint64_t k = start - o0 + e0;
      if (k < P.num_out) P.out_sel[k] = (uint32_t)i;
    }
  }
}

// ---- length and get: one lane per row -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ar_length_kernel(const uint64_t* offsets, int64_t n, uint64_t n_elems, uint64_t* out, unsigned long long* bad_rows) {
  uint32_t bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    uint64_t start, len;
    if (!ar_row(offsets, i, n_elems, &start, &len)) ++bad;
    out[i] = len;
  }
  if (bad_rows) {                    // wave-uniform: one add per wave
    bad = (uint32_t)wave_sum_u64(bad);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(bad_rows, (unsigned long long)bad);
  }
}
__global__ __launch_bounds__(256) void ar_get_kernel(const ArParams P, const int64_t* index, int32_t index_scalar) {
  const uint32_t lane = threadIdx.x & 63;
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool ok = false;
    if (i < P.n) {
      uint64_t start, len, pos;
      ArBits v{0, 0};
      if (ar_row(P.offsets, i, P.n_elems, &start, &len) && ar_get_pos(index[index_scalar ? 0 : i], len, &pos)) {
        v = ar_load(P.data, start + pos, P.es, false);
        ok = elem_valid(P, start + pos);
      }
      ar_store(P.out, (uint64_t)i, P.es, v);
    }
    const uint64_t word = __ballot(ok);
    if (lane == 0) P.out_words[wave0 >> 6] = word;
  }
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------
// what every call checks. *done: the call is over (n = 0) with the returned status.
int32_t check_array(const uint64_t* offsets, int64_t n, const dbhip_col* elems, uint64_t n_elems, bool need_elems, const char* who) {
  if (n < 0 || n > LONGROWS_MAX_ROWS) { set_error("%s: row count outside 0 .. 2^32 - 2", who); return DBHIP_ERR_INVALID; }
  if (n > 0 && (!offsets || ((uintptr_t)offsets & 7))) { set_error("%s: NULL offsets or offsets not 8-byte aligned", who); return DBHIP_ERR_INVALID; }
  if (!need_elems) return DBHIP_OK;
  if (!elems) { set_error("%s: NULL elems", who); return DBHIP_ERR_INVALID; }
  if (elems->is_scalar) { set_error("%s: the child column cannot be a scalar", who); return DBHIP_ERR_INVALID; }
  if (elems->type == DBHIP_T_BOOL || elems->type == DBHIP_T_DEC256) {
    set_error("%s: Boolean and Decimal256 elements are not offered: keep the CPU closure", who);
    return DBHIP_ERR_UNSUPPORTED;
  }
  const int es = ar_size(elems->type);
  if (es == 0) { set_error("%s: unknown element type %d", who, elems->type); return DBHIP_ERR_INVALID; }
  if (n > 0 && n_elems > 0 && (!elems->data || ((uintptr_t)elems->data & (uintptr_t)(es - 1)))) {
    set_error("%s: NULL element data or data not aligned to the element size", who);
    return DBHIP_ERR_INVALID;
  }
  if (elems->validity_offset < 0) { set_error("%s: negative validity_offset", who); return DBHIP_ERR_INVALID; }
  return DBHIP_OK;
}
void base_params(ArParams& P, const dbhip_col* elems, const uint64_t* offsets, int64_t n, uint64_t n_elems) {
  memset(&P, 0, sizeof(P));
  P.offsets = offsets;
  P.n = n;
  P.n_elems = n_elems;
  if (elems) {
    P.data = (const uint8_t*)elems->data;
    P.validity = elems->validity;
    P.voff = elems->validity_offset;
    P.buffers = elems->buffers;
    P.n_buffers = elems->buffers && elems->n_buffers > 0 ? elems->n_buffers : 0;
    P.es = ar_size(elems->type);
    P.mode = ar_eq_mode(elems->type);
  }
}
int32_t check_find(int32_t op, void* out, const char* who) {
  if (!out || ((uintptr_t)out & 7)) { set_error("%s: NULL out or out not 8-byte aligned", who); return DBHIP_ERR_INVALID; }
  (void)op;
  return DBHIP_OK;
}

}  // namespace

extern "C" {

int32_t dbhip_array_length(const uint64_t* offsets, int64_t n, uint64_t n_elems, uint64_t* out, uint64_t* bad_rows_dev, void* stream) {
  const char* who = "dbhip_array_length";
  const int32_t rc = check_array(offsets, n, nullptr, n_elems, false, who);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  if (!out || ((uintptr_t)out & 7) || ((uintptr_t)bad_rows_dev & 7)) { set_error("%s: NULL or misaligned out, or bad_rows_dev not 8-byte aligned", who); return DBHIP_ERR_INVALID; }
  hipStream_t s = resolve_stream(stream);
  hipLaunchKernelGGL(ar_length_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, offsets, n, n_elems, out, (unsigned long long*)bad_rows_dev);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

int32_t dbhip_array_get(const dbhip_col* elems, const uint64_t* offsets, int64_t n, uint64_t n_elems, const dbhip_col* index, void* out_values,
                        uint8_t* out_validity, void* stream) {
  const char* who = "dbhip_array_get";
  const int32_t rc = check_array(offsets, n, elems, n_elems, true, who);
  if (rc) return rc;
  if (!index || index->type != DBHIP_T_I64) { set_error("%s: the index is an Int64 column or scalar", who); return DBHIP_ERR_INVALID; }
  if (n == 0) return DBHIP_OK;
  const int es = ar_size(elems->type);
  if (!index->data || ((uintptr_t)index->data & 7) || !out_values || ((uintptr_t)out_values & (uintptr_t)(es - 1)) || !out_validity || ((uintptr_t)out_validity & 7)) {
    set_error("%s: NULL or misaligned index data, out_values or out_validity", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  ArParams P;
  base_params(P, elems, offsets, n, n_elems);
  P.out = out_values;
  P.out_words = (unsigned long long*)out_validity;
  hipLaunchKernelGGL(ar_get_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P, (const int64_t*)index->data, index->is_scalar ? 1 : 0);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

int32_t dbhip_array_find(int32_t op, const dbhip_col* elems, const uint64_t* offsets, int64_t n, uint64_t n_elems, const dbhip_col* needle, void* out,
                         void* stream) {
  const char* who = "dbhip_array_find";
  if (op < 0 || op >= AR_FIND_COUNT) { set_error("%s: unknown op %d", who, op); return DBHIP_ERR_INVALID; }
  int32_t rc = check_array(offsets, n, elems, n_elems, true, who);
  if (rc) return rc;
  if (elems->type == DBHIP_T_STRING) { set_error("%s: String elements go through dbhip_array_find_str", who); return DBHIP_ERR_INVALID; }
  if (!needle || needle->type != elems->type) { set_error("%s: the needle must have the elements' type", who); return DBHIP_ERR_INVALID; }
  if ((elems->type == DBHIP_T_DEC64 || elems->type == DBHIP_T_DEC128) && (needle->precision != elems->precision || needle->scale != elems->scale)) {
    set_error("%s: the needle's precision and scale must equal the elements'", who);
    return DBHIP_ERR_INVALID;
  }
  if (n == 0) return DBHIP_OK;
  const int es = ar_size(elems->type);
  if (!needle->data || ((uintptr_t)needle->data & (uintptr_t)(es - 1)) || needle->validity_offset < 0) { set_error("%s: NULL or misaligned needle data", who); return DBHIP_ERR_INVALID; }
  if ((rc = check_find(op, out, who))) return rc;
  hipStream_t s = resolve_stream(stream);
  ArParams P;
  base_params(P, elems, offsets, n, n_elems);
  P.op = op;
  P.nd_data = (const uint8_t*)needle->data;
  P.nd_validity = needle->validity;
  P.nd_voff = needle->validity_offset;
  P.nd_scalar = needle->is_scalar ? 1 : 0;
  P.out = out;
  P.out_words = (unsigned long long*)out;
  return long_two_passes(P, ar_find_kernel<false>, ar_find_long_kernel<false>, AR_SCRATCH_SLOT, s, who);
}

int32_t dbhip_array_find_str(int32_t op, const dbhip_col* elems, const uint64_t* offsets, int64_t n, uint64_t n_elems, const uint8_t* needle_host,
                             int32_t needle_len, void* out, void* stream) {
  const char* who = "dbhip_array_find_str";
  if (op < 0 || op >= AR_FIND_COUNT) { set_error("%s: unknown op %d", who, op); return DBHIP_ERR_INVALID; }
  int32_t rc = check_array(offsets, n, elems, n_elems, true, who);
  if (rc) return rc;
  if (elems->type != DBHIP_T_STRING) { set_error("%s: the elements must be Strings", who); return DBHIP_ERR_INVALID; }
  if (needle_len < 0 || (needle_len > 0 && !needle_host)) { set_error("%s: NULL needle or a negative length", who); return DBHIP_ERR_INVALID; }
  if (needle_len > AR_MAX_NEEDLE) { set_error("%s: a needle of more than 255 bytes: keep the CPU closure", who); return DBHIP_ERR_UNSUPPORTED; }
  if (n == 0) return DBHIP_OK;
  if ((rc = check_find(op, out, who))) return rc;
  hipStream_t s = resolve_stream(stream);
  ArParams P;
  base_params(P, elems, offsets, n, n_elems);
  P.op = op;
  P.nd_len = (uint32_t)needle_len;
  if (needle_len) memcpy(P.nd, needle_host, (size_t)needle_len);
  P.out = out;
  P.out_words = (unsigned long long*)out;
  return long_two_passes(P, ar_find_kernel<true>, ar_find_long_kernel<true>, AR_SCRATCH_SLOT, s, who);
}

int32_t dbhip_array_reduce_result(int32_t kind, int32_t elem_type, uint8_t precision, uint8_t scale, int32_t* out_type_host, uint8_t* out_precision_host,
                                  uint8_t* out_scale_host) {
  const char* who = "dbhip_array_reduce_result";
  if (!out_type_host) { set_error("%s: NULL out_type_host", who); return DBHIP_ERR_INVALID; }
  uint8_t p = 0, sc = 0;
  int32_t t = 0;
  const int rc = ar_reduce_result(kind, elem_type, precision, scale, &t, &p, &sc);
  if (rc == 7) { set_error("%s: Boolean and Decimal256 elements are not offered: keep the CPU closure", who); return DBHIP_ERR_UNSUPPORTED; }
  if (rc) { set_error("%s: no reduction %d over element type %d", who, kind, elem_type); return DBHIP_ERR_INVALID; }
  *out_type_host = t;
  if (out_precision_host) *out_precision_host = p;
  if (out_scale_host) *out_scale_host = sc;
  return DBHIP_OK;
}

int32_t dbhip_array_reduce(int32_t kind, const dbhip_col* elems, const uint64_t* offsets, int64_t n, uint64_t n_elems, void* out, uint8_t* out_validity,
                           uint64_t* err_count_dev, void* stream) {
  const char* who = "dbhip_array_reduce";
  int32_t rc = check_array(offsets, n, elems, n_elems, true, who);
  if (rc) return rc;
  int32_t out_t = 0;
  uint8_t p, sc;
  if ((rc = dbhip_array_reduce_result(kind, elems->type, elems->precision, elems->scale, &out_t, &p, &sc))) return rc;
  if (n == 0) return DBHIP_OK;
  const int out_es = ar_size(out_t);
  if (!out || ((uintptr_t)out & (uintptr_t)(out_es - 1)) || ((uintptr_t)out_validity & 7) || ((uintptr_t)err_count_dev & 7) || (!out_validity && kind != AR_COUNT)) {
    set_error("%s: NULL or misaligned out, out_validity (required but for COUNT) or err_count_dev", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  ArParams P;
  base_params(P, elems, offsets, n, n_elems);
  P.op = kind;
  P.out = out;
  P.out_es = out_es;
  P.out_words = (unsigned long long*)out_validity;
  P.err_count = (unsigned long long*)err_count_dev;
  switch (ar_class(elems->type)) {
    case AR_CLS_I: return long_two_passes(P, ar_reduce_kernel<AR_CLS_I>, ar_reduce_long_kernel<AR_CLS_I>, AR_SCRATCH_SLOT, s, who);
    case AR_CLS_U: return long_two_passes(P, ar_reduce_kernel<AR_CLS_U>, ar_reduce_long_kernel<AR_CLS_U>, AR_SCRATCH_SLOT, s, who);
    case AR_CLS_F32: return long_two_passes(P, ar_reduce_kernel<AR_CLS_F32>, ar_reduce_long_kernel<AR_CLS_F32>, AR_SCRATCH_SLOT, s, who);
    case AR_CLS_F64: return long_two_passes(P, ar_reduce_kernel<AR_CLS_F64>, ar_reduce_long_kernel<AR_CLS_F64>, AR_SCRATCH_SLOT, s, who);
    default: return long_two_passes(P, ar_reduce_kernel<AR_CLS_D128>, ar_reduce_long_kernel<AR_CLS_D128>, AR_SCRATCH_SLOT, s, who);
  }
}

int32_t dbhip_array_unnest_sel(const uint64_t* offsets, int64_t n, uint64_t n_elems, uint32_t* out_sel, int64_t num_out, void* stream) {
  const char* who = "dbhip_array_unnest_sel";
  const int32_t rc = check_array(offsets, n, nullptr, n_elems, false, who);
  if (rc) return rc;
  if (num_out < 0) { set_error("%s: negative num_out", who); return DBHIP_ERR_INVALID; }
  if (n == 0 || num_out == 0) return DBHIP_OK;
  if (!out_sel || ((uintptr_t)out_sel & 3)) { set_error("%s: NULL or misaligned out_sel", who); return DBHIP_ERR_INVALID; }
  hipStream_t s = resolve_stream(stream);
  ArParams P;
  base_params(P, nullptr, offsets, n, n_elems);
  P.out_sel = out_sel;
  P.num_out = (uint64_t)num_out;
  return long_two_passes(P, ar_unnest_kernel, ar_unnest_long_kernel, AR_SCRATCH_SLOT, s, who);
}

}  // extern "C"
