// k_like.hip — LIKE and literal-needle predicates over String columns (include/dbhip.h a20).
//
// Reference: register_like / generate_like_pattern (src/query/functions/src/scalars/comparison.rs), LikePattern::{OrdinalStr,
// StartOfPercent, EndOfPercent, SurroundByPercent, SimplePattern, ComplexPattern}, and the scalar functions starts_with, ends_with and
// position(..) > 0. The host parses the constant pattern once into a table of segments (maximal runs of literal bytes and `_`,
// separated by `%`); the table travels in the kernels' parameter struct and every workgroup stages it in LDS.
//   pass 1   one lane per row. Values of <= 12 bytes are matched from the view's own registers. Longer ones are read with naturally
//            aligned 4-byte loads that each cover at least one byte of the value (head and tail by shifting and masking), so nothing
//            outside the value's own words is touched. The 64 result bits of a wave come from one __ballot and one lane stores them.
//            A row longer than DBHIP_LIKE_LONG_BYTES that needs a search (CONTAINS, SEGMENTS) is not walked here: its row id goes
//            into the long-row list (dev_longrows.h) and its bit is written as 0.
//   pass 2   one wave per listed row (dev_longrows.h). The lanes try 64 consecutive start positions of a
//            segment at a time; the leftmost hit is picked from a __ballot and its end carried, wave-uniformly, to the next segment.
//            A row that matches (after NEGATE) gets its bit with a 32-bit atomic OR; pass 1 has finished by then (same stream).
// SEGMENTS runs the segments left to right, each at its leftmost match at or after the previous one's end: exact, because under
// either unit definition a segment's end is monotone in its start. An end-anchored last segment is matched backwards from the end.
#include <string.h>
#include "dev_common.h"
#include "dev_longrows.h"
#include "dev_strview.h"
#include "runtime.h"
#define LIKE_FN __device__ __forceinline__
#include "like_match.h"

using namespace dbhip;

namespace {

constexpr int LIKE_SCRATCH_SLOT = 22;

struct LikeParams {
  LikeTable t;
  const uint4* views;
  const uint8_t* validity;
  int64_t voff;
  const void* const* buffers;
  uint64_t* out;
  LongList list;
  int64_t n;
  int32_t n_buffers, negate, unit_byte, _pad;
};

__device__ __forceinline__ void like_stage(const LikeParams& P, LikeShared& S) {   // 256 threads
  const uint32_t t = threadIdx.x;
  if (t < 64) S.words[t] = P.t.bytes[t];
  S.under[t] = (uint8_t)((P.t.under[t >> 5] >> (t & 31)) & 1u);
  if (t <= LIKE_MAX_SEGMENTS) S.seg_off[t] = P.t.seg_off[t];
  __syncthreads();
}

__global__ __launch_bounds__(256) void like_rows_kernel(const LikeParams P) {
  __shared__ LikeShared S;
  like_stage(P, S);
  const uint32_t kind = P.t.kind, nseg = P.t.nseg, m = P.t.min_len;
  const bool a_start = P.t.anchor_start, a_end = P.t.anchor_end, unit_byte = P.unit_byte != 0;
  const uint32_t lane = threadIdx.x & 63;
  // every lane of a wave runs the same number of rounds (the wave's first row decides), so the ballots see whole waves
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool bit = false, listed = false;
    if (i < P.n && (!P.validity || bit_get(P.validity, P.voff + i))) {
      const uint4 vw = P.views[i];
      LaneValue v{vw.x, vw.y, vw.z, vw.w, 0, 1, 0};
      bool usable = true;
      if (!v.is_inline()) {
        const uint8_t* bytes = nullptr;
        usable = sv_bytes_checked(P.views + i, vw.x, vw.z, vw.w, P.buffers, P.n_buffers, &bytes);   // (false: a long view that points nowhere)
        if (usable) v.base = (uintptr_t)bytes;
      }
      if (usable) {
        const bool hit = like_lane_decide(v, S, kind, nseg, m, a_start, a_end, unit_byte, &listed);
        bit = !listed && (hit != (P.negate != 0));
      }
    }
    const uint64_t word = __ballot(bit);
    list_rows(listed, lane, i, P.list);
    if (lane == 0) P.out[wave0 >> 6] = word;   // bits past n are 0: those lanes never set `bit`
  }
}

// pass 2: one wave per listed row (CONTAINS and SEGMENTS only; the value is longer than DBHIP_LIKE_LONG_BYTES and its buffer was checked)
__global__ __launch_bounds__(256) void like_long_kernel(const LikeParams P) {
  __shared__ LikeShared S;
  like_stage(P, S);
  const uint32_t nseg = P.t.nseg;
  const bool a_start = P.t.anchor_start, a_end = P.t.anchor_end, unit_byte = P.unit_byte != 0;
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  const uint8_t* sb = (const uint8_t*)S.words;
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const uint32_t row = P.list.rows[q];
    const uint4 vw = P.views[row];
    WaveValue v{vw.x, (const uint8_t*)P.buffers[vw.z] + vw.w};   // (a long view that pass 1 has checked: dev_strview.h sv_bytes_checked)
    // the anchored segments: every lane does the same work on the same bytes
    uint32_t pos = 0, tail = v.len, first = 0, last = nseg;
    bool ok = true, done = false;
    if (a_start) {
      ok = seg_forward(v, sb, S.under, S.seg_off[1], 0, unit_byte, &pos);
      first = 1;
      if (nseg == 1 && a_end) { ok = ok && pos == v.len; done = true; }
    }
    if (ok && !done && a_end) {
      const uint32_t o = S.seg_off[nseg - 1];
      ok = seg_backward(v, sb + o, S.under + o, S.seg_off[nseg] - o, v.len, unit_byte, &tail);
      last = nseg - 1;
    }
    ok = __builtin_amdgcn_readfirstlane(ok);
    done = __builtin_amdgcn_readfirstlane(done);
    pos = __builtin_amdgcn_readfirstlane(pos);
    tail = __builtin_amdgcn_readfirstlane(tail);
    if (ok && !done) {
      for (uint32_t s = first; s < last; ++s) {
        const uint32_t o = S.seg_off[s], L = S.seg_off[s + 1] - o;
        bool found = false;
        for (uint32_t b0 = pos; b0 + L <= tail; b0 += 64) {     // wave-uniform bounds: the ballot sees all 64 lanes
          const uint32_t st = b0 + lane;
          uint32_t e = 0;
          const bool hit = st + L <= tail && seg_forward(v, sb + o, S.under + o, L, st, unit_byte, &e);
          const uint64_t hits = __ballot(hit);
          if (hits) {
            pos = __builtin_amdgcn_readfirstlane(__shfl(e, __ffsll((unsigned long long)hits) - 1, 64));
            found = true;
            break;
          }
        }
        if (!found) { ok = false; break; }
      }
      ok = ok && pos <= tail;
    }
    if (lane == 0 && (ok != (P.negate != 0))) atomicOr((uint32_t*)P.out + (row >> 5), 1u << (row & 31));
  }
}

// a scalar column: the one decided bit to all n rows
__global__ __launch_bounds__(256) void like_fill_kernel(const uint64_t* one, uint64_t* out, int64_t n) {
  const uint64_t all = (*one & 1ull) ? ~0ull : 0ull;
  const int64_t words = (n + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256) {
    const int64_t left = n - w * 64;
    out[w] = left >= 64 ? all : (all & ((1ull << left) - 1ull));
  }
}

int32_t like_run(const LikeTable& t, const dbhip_col* col, int32_t flags, int64_t n, uint8_t* out_bitmap, void* stream, const char* who) {
  if (!col || col->type != DBHIP_T_STRING) { set_error("%s: the column must be a String column", who); return DBHIP_ERR_INVALID; }
  if (flags & ~(DBHIP_LIKE_NEGATE | DBHIP_LIKE_UNIT_BYTE)) { set_error("%s: unknown flag bits", who); return DBHIP_ERR_INVALID; }
  if (n < 0 || n > LONGROWS_MAX_ROWS) { set_error("%s: row count outside 0 .. 2^32 - 2", who); return DBHIP_ERR_INVALID; }
  if (n == 0) return DBHIP_OK;
  if (!col->data || !out_bitmap || ((uintptr_t)out_bitmap & 7) || ((uintptr_t)col->data & 15)) {
    set_error("%s: NULL views or bitmap, views not 16-byte aligned or bitmap not 8-byte aligned", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  const bool searches = t.nseg > 0 && (t.kind == DBHIP_LIKE_CONTAINS || t.kind == DBHIP_LIKE_SEGMENTS);   // only these list long rows
  const int64_t rows = col->is_scalar ? 1 : n;
  // scratch: count | (scalar: the one result word) | row ids
  uint8_t* ws = (uint8_t*)scratch(long_list_bytes(searches ? rows : 0), LIKE_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  LikeParams P;
  memset(&P, 0, sizeof(P));
  P.t = t;
  P.views = (const uint4*)col->data;
  P.validity = col->validity;
  P.voff = col->validity_offset;
  P.buffers = col->buffers;
  P.n_buffers = col->buffers && col->n_buffers > 0 ? col->n_buffers : 0;
  P.out = col->is_scalar ? (uint64_t*)(ws + 8) : (uint64_t*)out_bitmap;
  P.list = long_list_at(ws);
  P.n = rows;
  P.negate = (flags & DBHIP_LIKE_NEGATE) ? 1 : 0;
  P.unit_byte = (flags & DBHIP_LIKE_UNIT_BYTE) ? 1 : 0;
  DBHIP_CHECK(long_list_clear(ws, s));
  hipLaunchKernelGGL(like_rows_kernel, dim3(grid_for(rows, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  if (searches) {
    DBHIP_POLL_CANCEL(s, who);
    long_launch(like_long_kernel, P, s);
    DBHIP_LAUNCH_CHECK();
  }
  if (col->is_scalar) {
    DBHIP_POLL_CANCEL(s, who);
    hipLaunchKernelGGL(like_fill_kernel, dim3(grid_for((n + 63) >> 6, 256)), dim3(256), 0, s, (const uint64_t*)(ws + 8), (uint64_t*)out_bitmap, n);
    DBHIP_LAUNCH_CHECK();
  }
  return DBHIP_OK;
}

}  // namespace

extern "C" {

int32_t dbhip_like_kind(const uint8_t* pattern_host, int32_t pattern_len, int32_t escape) {
  LikeTable t;
  const char* why = "";
  const int32_t rc = like_parse(pattern_host, pattern_len, escape, false, &t, &why);
  if (rc) set_error("dbhip_like_kind: %s", why);
  return rc ? -rc : (int32_t)t.kind;
}

int32_t dbhip_like(const dbhip_col* col, const uint8_t* pattern_host, int32_t pattern_len, int32_t escape, int32_t flags, int64_t n,
                   uint8_t* out_bitmap, void* stream) {
  LikeTable t;
  const char* why = "";
  const int32_t rc = like_parse(pattern_host, pattern_len, escape, false, &t, &why);
  if (rc) { set_error("dbhip_like: %s", why); return rc; }
  return like_run(t, col, flags, n, out_bitmap, stream, "dbhip_like");
}

int32_t dbhip_str_match(int32_t kind, const dbhip_col* col, const uint8_t* needle_host, int32_t needle_len, int32_t flags, int64_t n,
                        uint8_t* out_bitmap, void* stream) {
  LikeTable t;
  const char* why = "";
  const int32_t rc = like_parse_needle(kind, needle_host, needle_len, &t, &why);
  if (rc) { set_error("dbhip_str_match: %s", why); return rc; }
  return like_run(t, col, flags, n, out_bitmap, stream, "dbhip_str_match");
}

}  // extern "C"
