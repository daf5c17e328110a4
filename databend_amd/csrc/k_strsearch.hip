// k_strsearch.hip — String search and rewrite (include/dbhip.h a28): position / locate, split_part, replace, lpad / rpad, repeat, reverse.
//
// The row logic is dev_strsearch.h's (one text for these kernels and for the host checker); this file is the memory side and the
// wave-per-row forms of the same steps. The structure is k_strfn.hip's:
//   position / split_part   pass 1: one lane per row. The view is loaded as one 16-byte vector; a value of up to DBHIP_LIKE_LONG_BYTES is
//            searched by its lane through naturally aligned 4-byte loads (SfValue::byte). A longer value that has to be searched is
//            not: its row id goes into the long-row list (dev_longrows.h) and its output is written as zero.
//            pass 2: one wave per listed row (dev_longrows.h), the value as aligned words (dev_strwave.h).
//   rewrite  count (u32 bytes per row that go to out_data; long values that need a walk through the list and a wave-per-row count) ->
//            dbscan::exclusive_scan_u32 -> fill: one lane per row writes the view of a result of up to 12 bytes from registers; results
//            of 13 .. DBHIP_LIKE_LONG_BYTES are written by the row's own wave, one row after the other, so that neighbouring lanes
//            write neighbouring bytes; longer results, and long values that need a walk, go through a second list to a wave-per-row
//            fill.
//   the wave's search (wave_walk): a step is 64 aligned words, 256 start positions. Every lane tests the four positions of its word
//            against the needle's first four bytes (its own word and its neighbour's, the neighbour of lane 63 being the next step's
//            first word, so a match that straddles two steps is found), verifies the rest of a longer needle, and four ballots hold
//            the step's candidates. The greedy non-overlapping selection is a wave-uniform loop over their set bits.
// The constants (needle / from / to / pad / delimiter, up to 255 bytes each) travel by value in the kernel arguments and are staged in
// LDS. No loop waits for another wave; every loop advances by construction.
#include <string.h>
#include "dev_common.h"
#include "dev_scan.h"
#include "dev_strsearch.h"
#include "dev_strwave.h"
#include "runtime.h"

using namespace dbhip;

static_assert(SS_REPLACE == DBHIP_STRW_REPLACE && SS_LPAD == DBHIP_STRW_LPAD && SS_RPAD == DBHIP_STRW_RPAD && SS_REPEAT == DBHIP_STRW_REPEAT &&
              SS_REVERSE == DBHIP_STRW_REVERSE && SF_LONG_BYTES == DBHIP_LIKE_LONG_BYTES, "dev_strsearch.h codes");

namespace {

constexpr int SS_SCRATCH_SLOT = 27;

// ---- the column frame, a long value as aligned words and the long-row list: dev_strwave.h and dev_longrows.h -------------------------------
// the unit boundaries at the positions [lo, hi) of the value, position 0 counted as one whatever its byte
__device__ __forceinline__ uint32_t wave_bounds(const WaveWords& W, uint32_t lo, uint32_t hi, uint32_t lane) {
  uint32_t acc = 0;
  if (hi > W.len) hi = W.len;
  if (lo >= hi) return 0;
  const int64_t wend = (((int64_t)W.lead + hi - 1) >> 2) + 1;
  for (int64_t wb = ((int64_t)W.lead + lo) >> 2; wb < wend; wb += 64) {          // wave-uniform bounds
    uint32_t in;
    const uint32_t w = ww_load(W, wb + lane, lo, hi, in);
    uint32_t bits = noncont4(w) & in;
    if (wb + lane == 0 && lo == 0) bits |= 1u << W.lead;
    acc += (uint32_t)__popc(bits);
  }
  return (uint32_t)wave_sum_u64(acc);
}

// ---- the wave's occurrence walk -------------------------------------------------------------------------------------------------------------
// Visits the greedy left-to-right non-overlapping occurrences of nd (m >= 1 bytes, in LDS) at positions >= from, in order:
// vis.begin_step(word index, word, mask of its bytes inside the value) per step and lane, vis.occ(p) per occurrence (wave-uniform; false
// ends the walk), vis.end_step() per step.
template <class V>
__device__ __forceinline__ void wave_walk(const WaveWords& W, uint32_t from, const uint8_t* nd, uint32_t m, uint32_t lane, V& vis) {
  uint32_t npre = 0;
  for (uint32_t i = 0; i < 4 && i < m; ++i) npre |= (uint32_t)nd[i] << (8 * i);
  const uint32_t pmask = m >= 4 ? 0xFFFFFFFFu : ((1u << (8 * m)) - 1u);
  uint32_t next_ok = from;                               // the smallest position the next occurrence may have
  for (int64_t wb = ((int64_t)W.lead + from) >> 2; wb < (int64_t)W.nwords; wb += 64) {      // wave-uniform bounds
    const int64_t widx = wb + lane;
    uint32_t in, in_next;
    const uint32_t w0 = ww_load(W, widx, 0, W.len, in);
    const uint32_t wn = ww_load(W, wb + 64, 0, W.len, in_next);     // the next step's first word, for lane 63
    uint32_t w1 = (uint32_t)__shfl((int)w0, (int)((lane + 1) & 63), 64);
    if (lane == 63) w1 = wn;
    const uint64_t both = ((uint64_t)w1 << 32) | w0;
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t p = widx * 4 + j - W.lead;
      if (p >= (int64_t)from && p + m <= (int64_t)W.len && ((((uint32_t)(both >> (8 * j))) ^ npre) & pmask) == 0) {
        bool same = true;
        for (uint32_t i = 4; i < m && same; ++i) same = ww_byte(W, (uint32_t)p + i) == nd[i];
        if (same) bits |= 1u << j;
      }
    }
    Ballots B;
    ballots_of(bits, B);
    vis.begin_step(W, widx, w0, in);
    const int64_t s0 = wb * 4 - W.lead;                  // the position of lane 0's first byte
    bool go_on = true;
    for (;;) {                                           // every round selects a position >= next_ok and moves next_ok past it
      uint32_t best = SS_NONE;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t t = (int64_t)next_ok - s0 - j;     // lanes l with s0 + 4 l + j >= next_ok
        const uint64_t b = B.b[j] & lanes_from(t <= 0 ? 0u : (uint32_t)((t + 3) >> 2));
        if (b) {
          const uint32_t p = (uint32_t)(s0 + 4 * (int64_t)(__ffsll((unsigned long long)b) - 1) + j);
          best = p < best ? p : best;
        }
      }
      if (best == SS_NONE) break;
      next_ok = best + m;
      if (!vis.occ(best)) { go_on = false; break; }
    }
    vis.end_step();
    if (!go_on) return;
  }
}
struct FirstV {            // ss_find_from
  uint32_t p = SS_NONE;
  __device__ __forceinline__ void begin_step(const WaveWords&, int64_t, uint32_t, uint32_t) {}
  __device__ __forceinline__ void end_step() {}
  __device__ __forceinline__ bool occ(uint32_t at) { p = at; return false; }
};
struct CountV {            // ss_count
  uint32_t c = 0;
  __device__ __forceinline__ void begin_step(const WaveWords&, int64_t, uint32_t, uint32_t) {}
  __device__ __forceinline__ void end_step() {}
  __device__ __forceinline__ bool occ(uint32_t) { ++c; return true; }
};
struct FieldV {            // ss_field: field k lies behind occurrence k - 1 and in front of occurrence k
  uint64_t k;
  uint32_t m;
  uint64_t c = 0;
  uint32_t fs = 0, fe = 0;
  bool done = false;
  __device__ __forceinline__ void begin_step(const WaveWords&, int64_t, uint32_t, uint32_t) {}
  __device__ __forceinline__ void end_step() {}
  __device__ __forceinline__ bool occ(uint32_t p) {
    ++c;
    if (c == k) { fe = p; done = true; return false; }
    if (c + 1 == k) fs = p + m;
    return true;
  }
};

// ---- the parameters of every kernel here ---------------------------------------------------------------------------------------------------
struct SearchParams {
  StrCol col;
  const int64_t* k;                  // start / part / length / count (may be NULL where the function allows)
  int64_t n;
  uint64_t* out_pos;                 // position
  uint4* out_views;                  // split_part, rewrite
  uint32_t* counts;                  // rewrite: bytes of the row that go to out_data (NULL in the _bytes call)
  uint64_t* lens;                    // rewrite: the result length of a row that the wave counted (SS_TOO_LONG: too long)
  unsigned long long* total;         // _bytes: the sum of counts
  const uint64_t* offsets;           // the scan of counts
  uint8_t* out_data;
  uint64_t out_data_bytes;
  unsigned long long* err_count;
  LongList list;
  int32_t op, unit_byte, k_scalar, _pad;
  SsConst C;
};
__device__ __forceinline__ void const_stage(const SearchParams& P, SsConst& S) {   // 256 threads
  static_assert(sizeof(SsConst) % 4 == 0 && sizeof(SsConst) / 4 <= 256, "SsConst");
  if (threadIdx.x < sizeof(SsConst) / 4) ((uint32_t*)&S)[threadIdx.x] = ((const uint32_t*)&P.C)[threadIdx.x];
  __syncthreads();
}
__device__ __forceinline__ int64_t k_of(const SearchParams& P, int64_t i, int64_t otherwise) {
  return P.k ? P.k[P.k_scalar ? 0 : i] : otherwise;
}

// ---- position -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ss_position_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  const bool unit_byte = P.unit_byte != 0;
  // every lane of a wave runs the same number of rounds (the wave's first row decides), so the ballots see whole waves
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool listed = false;
    if (i < P.n) {
      SfValue v;
      uint32_t index, offset;
      uint64_t r = 0;
      if (str_value(P.col, i, v, index, offset)) {
        const int64_t s = k_of(P, i, 1);
        if (v.len > SF_LONG_BYTES && ss_position_walks(v.len, S.x_len, s, unit_byte)) listed = true;
        else r = ss_position(v, S.x, S.x_len, s, unit_byte);
      }
      P.out_pos[i] = r;
    }
    list_rows(listed, lane, i, P.list);
  }
}
__global__ __launch_bounds__(256) void ss_position_long_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  const bool unit_byte = P.unit_byte != 0;
  const LongWalk lw = long_walk(P.list);
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    uint4 vw;
    const WaveWords W = ww_of((uintptr_t)str_bytes(P.col, i, vw), vw.x);
    const int64_t s = k_of(P, i, 1);                     // pass 1: 1 <= s <= len + 1
    const uint32_t skip = (uint32_t)(s - 1);
    uint64_t r = 0;
    if (S.x_len == 0) {
      r = skip <= wave_bounds(W, 0, W.len, lane) ? (uint64_t)s : 0;
    } else {
      const uint32_t b = skip == 0 ? 0 : (unit_byte ? skip : wave_forward(W, 0, skip, lane));
      FirstV first;
      wave_walk(W, b, S.x, S.x_len, lane, first);
      if (first.p != SS_NONE) r = 1 + (uint64_t)(unit_byte ? first.p : wave_bounds(W, 1, first.p + 1, lane));
    }
    if (lane == 0) P.out_pos[i] = r;
  }
}

// ---- split_part ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ss_split_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool listed = false;
    if (i < P.n) {
      SfValue v;
      uint32_t index = 0, offset = 0;
      uint32_t w[4] = {0, 0, 0, 0};
      if (str_value(P.col, i, v, index, offset)) {
        if (v.len > SF_LONG_BYTES && ss_split_walks(v.len, S.x_len)) {
          listed = true;
        } else {
          uint32_t s, e;
          if (ss_field_range(v, S.x, S.x_len, k_of(P, i, 1), &s, &e)) sf_slice_view(v, index, offset, s, e, w);
        }
      }
      P.out_views[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    list_rows(listed, lane, i, P.list);
  }
}
__global__ __launch_bounds__(256) void ss_split_long_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    uint4 vw;
    const uint8_t* bytes = str_bytes(P.col, i, vw);
    const WaveWords W = ww_of((uintptr_t)bytes, vw.x);
    const int64_t part = k_of(P, i, 1);
    uint32_t c = 0;
    if (ss_part_from_end(part)) {
      CountV cv;
      wave_walk(W, 0, S.x, S.x_len, lane, cv);
      c = cv.c;
    }
    FieldV f{ss_field_index(part, c), S.x_len};
    bool found = false;
    if (f.k != 0) {
      wave_walk(W, 0, S.x, S.x_len, lane, f);
      found = f.done || f.c + 1 == f.k;                  // the last field ends with the value
      if (!f.done) f.fe = W.len;
    }
    if (lane == 0 && found) {
      SfValue v = sf_value(vw.x, vw.y, vw.z, vw.w, bytes);
      uint32_t w[4];
      sf_slice_view(v, vw.z, vw.w, f.fs, f.fe, w);
      P.out_views[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

// ---- rewrite: the length of a row -------------------------------------------------------------------------------------------------------------
// what a lane may decide: false when a value longer than DBHIP_LIKE_LONG_BYTES has to be walked for its result's length
__device__ __forceinline__ bool lane_len(const SearchParams& P, const SsConst& S, SfValue& v, int64_t k, uint64_t& total) {
  if (v.len > SF_LONG_BYTES && ss_len_walks(P.op, S, v.len, k, P.unit_byte != 0)) return false;
  total = ss_rewrite_len(P.op, v, k, S, P.unit_byte != 0);
  return true;
}
// ss_rewrite_len for the wave, of a row that lane_len has left
__device__ __forceinline__ uint64_t wave_len(const SearchParams& P, const SsConst& S, const WaveWords& W, int64_t k, uint32_t lane) {
  if (P.op == SS_REPLACE) {
    CountV cv;
    wave_walk(W, 0, S.x, S.x_len, lane, cv);
    return ss_replace_len(S, W.len, cv.c);
  }
  bool cut;                                              // LPAD / RPAD in units, k > 0
  const uint64_t total = ss_pad_len(S, W.len, wave_bounds(W, 0, W.len, lane), k, &cut);
  return cut ? wave_forward(W, 0, (uint32_t)k, lane) : total;
}

__global__ __launch_bounds__(256) void ss_count_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  uint64_t sum = 0;
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool listed = false;
    if (i < P.n) {
      SfValue v;
      uint32_t index, offset, c = 0;
      if (str_value(P.col, i, v, index, offset)) {
        uint64_t total;
        if (!lane_len(P, S, v, k_of(P, i, 0), total)) listed = true;
        else if (total != SS_TOO_LONG && total > SV_INLINE_MAX) c = (uint32_t)total;
      }
      if (P.counts) P.counts[i] = c;
      sum += c;
    }
    list_rows(listed, lane, i, P.list);
  }
  if (P.total) {      // every lane arrives here: one add per wave
    sum = wave_sum_u64(sum);
    if (lane == 0 && sum) atomicAdd(P.total, (unsigned long long)sum);
  }
}
__global__ __launch_bounds__(256) void ss_count_long_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  const LongWalk lw = long_walk(P.list);
  uint64_t sum = 0;
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    uint4 vw;
    const WaveWords W = ww_of((uintptr_t)str_bytes(P.col, i, vw), vw.x);
    const uint64_t total = wave_len(P, S, W, k_of(P, i, 0), lane);
    const uint32_t c = total != SS_TOO_LONG && total > SV_INLINE_MAX ? (uint32_t)total : 0u;
    if (lane == 0) {
      if (P.counts) P.counts[i] = c;
      if (P.lens) P.lens[i] = total;
      sum += c;
    }
  }
  if (P.total && lane == 0 && sum) atomicAdd(P.total, (unsigned long long)sum);
}

// ---- rewrite: the bytes of a row, written by its wave -------------------------------------------------------------------------------------
// where the bytes go: out_data for a result of more than 12 bytes, and the first 12 into three words for the view
struct RowSink {
  uint8_t* dst;
  uint64_t total;
  uint32_t h0 = 0, h1 = 0, h2 = 0;
  __device__ __forceinline__ void put(uint64_t at, uint32_t c) {
    if (at >= total) return;                             // (never, by the count: a store outside the row is not made)
    if (total > SV_INLINE_MAX) dst[at] = (uint8_t)c;
    if (at < 4) h0 |= c << (8 * at);
    else if (at < 8) h1 |= c << (8 * (at - 4));
    else if (at < 12) h2 |= c << (8 * (at - 8));
  }
};
struct ReplaceV {          // ss_emit's REPLACE: a step's bytes move by (occurrences in front of them) * (y_len - x_len)
  RowSink& sink;
  const uint8_t* y;
  uint32_t xl, yl, lane;
  uint64_t c = 0;
  uint32_t drop_until = 0;                               // the end of the last occurrence: its bytes are not copied
  int64_t q0 = 0;
  uint32_t w = 0, in = 0, dropped = 0, cnt[4] = {0, 0, 0, 0};
  uint64_t base_c = 0;
  __device__ __forceinline__ int64_t delta() const { return (int64_t)yl - (int64_t)xl; }
  __device__ __forceinline__ void begin_step(const WaveWords& W, int64_t widx, uint32_t w0, uint32_t in0) {
    q0 = widx * 4 - W.lead;
    w = w0; in = in0; dropped = 0; base_c = c;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      cnt[j] = 0;
      if (q0 + j < (int64_t)drop_until) dropped |= 1u << j;
    }
  }
  __device__ __forceinline__ bool occ(uint32_t p) {
    const int64_t d = (int64_t)p + (int64_t)c * delta();
    for (uint32_t b = lane; b < yl; b += 64) sink.put((uint64_t)(d + b), y[b]);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (q0 + j >= (int64_t)p) {
        ++cnt[j];
        if (q0 + j < (int64_t)p + xl) dropped |= 1u << j;
      }
    ++c;
    drop_until = p + xl;
    return true;
  }
  __device__ __forceinline__ void end_step() {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (((in >> j) & 1u) && !((dropped >> j) & 1u))
        sink.put((uint64_t)(q0 + j + (int64_t)(base_c + cnt[j]) * delta()), (w >> (8 * j)) & 0xFFu);
  }
};
// ss_emit's REVERSE in units: a step is 64 bytes, one per lane. A byte of the unit [a, b) at position i goes to len - b + (i - a): a is
// the last boundary at or below i (carried from the steps before when the step holds none), b the first one above (looked for in the
// steps behind when the step holds none; what that search finds serves every step up to it).
__device__ __forceinline__ void wave_reverse_units(const uint8_t* src, uint32_t len, uint32_t lane, RowSink& sink) {
  uint32_t carry_a = 0;
  uint64_t nb = 0;                                       // the first boundary at or behind the end of some earlier step, or len
  bool nb_known = false;
  for (uint64_t c0 = 0; c0 < len; c0 += 64) {
    const uint64_t i = c0 + lane;
    const uint32_t c = i < len ? src[i] : 0u;
    const uint64_t B = __ballot(i < len && (i == 0 || !sf_is_cont(c)));
    if (c0 + 64 >= len) {
      nb = len;
    } else if (!nb_known || nb < c0 + 64) {
      nb = len;
      for (uint64_t d0 = c0 + 64; d0 < len; d0 += 64) {
        const uint64_t i2 = d0 + lane;
        const uint64_t B2 = __ballot(i2 < len && !sf_is_cont(src[i2 < len ? i2 : 0]));
        if (B2) { nb = d0 + (uint64_t)(__ffsll((unsigned long long)B2) - 1); break; }
      }
      nb_known = true;
    }
    const uint64_t below = B & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    const uint64_t above = B & lanes_from(lane + 1);
    const uint64_t a = below ? c0 + (uint64_t)(63 - __clzll((long long)below)) : carry_a;
    const uint64_t b = above ? c0 + (uint64_t)(__ffsll((unsigned long long)above) - 1) : nb;
    if (i < len) sink.put((uint64_t)len - b + (i - a), c);
    if (B) carry_a = (uint32_t)(c0 + (uint64_t)(63 - __clzll((long long)B)));
  }
}
// The wave writes row i's result of `total` bytes (1 .. 2^32 - 1, what the count gave) at out_data + off (it fits: the caller has
// checked) and the row's view.
__device__ __forceinline__ void wave_fill_row(const SearchParams& P, const SsConst& S, int64_t i, uint64_t total, uint64_t off, uint32_t lane) {
  uint4 vw;
  const uint8_t* src = str_bytes(P.col, i, vw);
  const uint32_t len = vw.x;
  RowSink sink{total > SV_INLINE_MAX ? P.out_data + off : nullptr, total};
  if (P.op == SS_REPLACE) {
    if (ss_replace_walks(S, len)) {
      ReplaceV rv{sink, S.y, S.x_len, S.y_len, lane};
      wave_walk(ww_of((uintptr_t)src, len), 0, S.x, S.x_len, lane, rv);
    } else {
      for (uint64_t j = lane; j < total; j += 64) sink.put(j, src[j]);
    }
  } else if (P.op == SS_LPAD || P.op == SS_RPAD) {
    const uint64_t fill = total > len ? total - len : 0, body = total - fill;
    const uint64_t lead = P.op == SS_LPAD ? fill : 0, pad_at = P.op == SS_LPAD ? 0 : body;
    for (uint64_t j = lane; j < total; j += 64) {
      const bool in_body = j >= lead && j - lead < body;
      sink.put(j, in_body ? (uint32_t)src[j - lead] : (uint32_t)S.x[(j - pad_at) % (S.x_len ? S.x_len : 1u)]);
    }
  } else if (P.op == SS_REPEAT) {
    for (uint64_t j = lane; j < total; j += 64) sink.put(j, src[j % len]);
  } else if (P.unit_byte) {
    for (uint64_t j = lane; j < total; j += 64) sink.put(j, src[len - 1 - j]);
  } else {
    wave_reverse_units(src, len, lane, sink);
  }
  const uint32_t h0 = (uint32_t)wave_sum_u64(sink.h0), h1 = (uint32_t)wave_sum_u64(sink.h1), h2 = (uint32_t)wave_sum_u64(sink.h2);   // disjoint bytes
  if (lane == 0) P.out_views[i] = total > SV_INLINE_MAX ? make_uint4((uint32_t)total, h0, 0u, (uint32_t)off) : make_uint4((uint32_t)total, h0, h1, h2);
}

__global__ __launch_bounds__(256) void ss_fill_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t cap = P.out_data_bytes < 0x100000000ull ? P.out_data_bytes : 0x100000000ull;
  uint32_t errs = 0;
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool listed = false, coop = false;
    uint64_t total = 0, off = 0;
    if (i < P.n) {
      SfValue v;
      uint32_t index, offset;
      uint32_t w[4] = {0, 0, 0, 0};
      if (str_value(P.col, i, v, index, offset)) {
        if (!lane_len(P, S, v, k_of(P, i, 0), total)) {
          listed = true;                                 // the wave count has left its length in P.lens
        } else if (total == SS_TOO_LONG) {
          ++errs;
        } else if (total > SV_INLINE_MAX) {
          off = P.offsets[i];
          if (off + total > cap) ++errs;
          else if (total <= SF_LONG_BYTES) coop = true;
          else { listed = true; P.lens[i] = total; }
        } else if (total > 0) {
          SfInlineSink sink{0, 0};
          ss_emit(P.op, v, S, (uint32_t)total, P.unit_byte != 0, sink);
          w[0] = (uint32_t)total; w[1] = (uint32_t)sink.lo; w[2] = (uint32_t)(sink.lo >> 32); w[3] = sink.hi;
        }
      }
      if (!coop) P.out_views[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    // results of 13 .. DBHIP_LIKE_LONG_BYTES bytes: the wave writes its rows one after the other, so that neighbouring lanes write
    // neighbouring bytes (the rows of a wave lie back to back in out_data)
    for (uint64_t cm = __ballot(coop); cm; cm &= cm - 1) {
      const int l = __ffsll((unsigned long long)cm) - 1;
      wave_fill_row(P, S, wave0 + l, __shfl(total, l, 64), __shfl(off, l, 64), lane);
    }
    list_rows(listed, lane, i, P.list);
  }
  errs = (uint32_t)wave_sum_u64(errs);                   // every lane arrives here: one add per wave
  if (lane == 0 && errs && P.err_count) atomicAdd(P.err_count, (unsigned long long)errs);
}
// one wave per listed row: a result longer than DBHIP_LIKE_LONG_BYTES, or a value that long which the lane could not walk
__global__ __launch_bounds__(256) void ss_fill_long_kernel(const SearchParams P) {
  __shared__ SsConst S;
  const_stage(P, S);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t cap = P.out_data_bytes < 0x100000000ull ? P.out_data_bytes : 0x100000000ull;
  const LongWalk lw = long_walk(P.list);
  uint32_t errs = 0;
  for (uint32_t q = lw.first; q < lw.count; q += lw.stride) {
    const int64_t i = P.list.rows[q];
    const uint64_t total = P.lens[i];
    if (total == 0) continue;                            // (the view is zero already)
    const uint64_t off = total != SS_TOO_LONG && total > SV_INLINE_MAX ? P.offsets[i] : 0;
    if (total == SS_TOO_LONG || (total > SV_INLINE_MAX && off + total > cap)) { ++errs; continue; }
    wave_fill_row(P, S, i, total, off, lane);
  }
  if (lane == 0 && errs && P.err_count) atomicAdd(P.err_count, (unsigned long long)errs);
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------
int32_t check_common(const dbhip_col* c, int32_t flags, int64_t n, const char* who) {
  if (!c || c->type != DBHIP_T_STRING) { set_error("%s: the column must be a String column", who); return DBHIP_ERR_INVALID; }
  if (flags & ~DBHIP_STR_UNIT_BYTE) { set_error("%s: unknown flag bits", who); return DBHIP_ERR_INVALID; }
  if (n < 0 || n > LONGROWS_MAX_ROWS) { set_error("%s: row count outside 0 .. 2^32 - 2", who); return DBHIP_ERR_INVALID; }
  return DBHIP_OK;
}
int32_t check_const(const uint8_t* p, int32_t len, const char* what, const char* who) {
  if (len < 0 || (len > 0 && !p)) { set_error("%s: NULL %s or a negative length", who, what); return DBHIP_ERR_INVALID; }
  if (len > SS_MAX_CONST) { set_error("%s: a %s of more than 255 bytes: keep the CPU closure", who, what); return DBHIP_ERR_UNSUPPORTED; }
  return DBHIP_OK;
}
int32_t check_i64(const dbhip_col* k, bool required, int64_t n, const char* what, const char* who) {
  if (!k) {
    if (required) { set_error("%s: the %s is an Int64 column or scalar", who, what); return DBHIP_ERR_INVALID; }
    return DBHIP_OK;
  }
  if (k->type != DBHIP_T_I64) { set_error("%s: the %s is an Int64 column or scalar", who, what); return DBHIP_ERR_INVALID; }
  if (n > 0 && (!k->data || ((uintptr_t)k->data & 7))) { set_error("%s: NULL or misaligned %s data", who, what); return DBHIP_ERR_INVALID; }
  return DBHIP_OK;
}
void base_params(SearchParams& P, const dbhip_col* col, const dbhip_col* k, int64_t n, int32_t flags) {
  memset(&P, 0, sizeof(P));
  P.col = str_col(col);
  if (k) { P.k = (const int64_t*)k->data; P.k_scalar = k->is_scalar ? 1 : 0; }
  P.n = n;
  P.unit_byte = (flags & DBHIP_STR_UNIT_BYTE) ? 1 : 0;
}
// the arguments of dbhip_str_rewrite_bytes / dbhip_str_rewrite that the two share
int32_t rewrite_params(int32_t op, const dbhip_col* col, const dbhip_col* k, const uint8_t* x, int32_t x_len, const uint8_t* y, int32_t y_len,
                       int32_t flags, int64_t n, SearchParams& P, const char* who) {
  if (op < 0 || op >= SS_OP_COUNT) { set_error("%s: unknown op %d", who, op); return DBHIP_ERR_INVALID; }
  int32_t rc = check_common(col, flags, n, who);
  if (rc) return rc;
  const bool uses_k = op == SS_LPAD || op == SS_RPAD || op == SS_REPEAT;
  const bool uses_x = op == SS_REPLACE || op == SS_LPAD || op == SS_RPAD, uses_y = op == SS_REPLACE;
  if (uses_x && (rc = check_const(x, x_len, op == SS_REPLACE ? "needle" : "pad", who))) return rc;
  if (uses_y && (rc = check_const(y, y_len, "replacement", who))) return rc;
  if (uses_k && (rc = check_i64(k, true, n, op == SS_REPEAT ? "count" : "length", who))) return rc;
  if (n > 0 && (!col->data || ((uintptr_t)col->data & 15))) { set_error("%s: NULL views or views not 16-byte aligned", who); return DBHIP_ERR_INVALID; }
  base_params(P, col, uses_k ? k : nullptr, n, flags);
  P.op = op;
  ss_prepare(P.C, x, uses_x ? (uint32_t)x_len : 0u, y, uses_y ? (uint32_t)y_len : 0u, P.unit_byte != 0);
  return DBHIP_OK;
}

}  // namespace

extern "C" {

int32_t dbhip_str_position(const dbhip_col* col, const uint8_t* needle_host, int32_t needle_len, const dbhip_col* start, int32_t flags,
                           int64_t n, uint64_t* out, void* stream) {
  const char* who = "dbhip_str_position";
  int32_t rc = check_common(col, flags, n, who);
  if (rc) return rc;
  if ((rc = check_const(needle_host, needle_len, "needle", who))) return rc;
  if ((rc = check_i64(start, false, n, "start", who))) return rc;
  if (n == 0) return DBHIP_OK;
  if (!col->data || !out || ((uintptr_t)out & 7) || ((uintptr_t)col->data & 15)) {
    set_error("%s: NULL views or out, views not 16-byte aligned or out not 8-byte aligned", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  SearchParams P;
  base_params(P, col, start, n, flags);
  P.out_pos = out;
  ss_prepare(P.C, needle_host, (uint32_t)needle_len, nullptr, 0, P.unit_byte != 0);
  return long_two_passes(P, ss_position_kernel, ss_position_long_kernel, SS_SCRATCH_SLOT, s, who);
}

int32_t dbhip_str_split_part(const dbhip_col* col, const uint8_t* delim_host, int32_t delim_len, const dbhip_col* part, int64_t n,
                             void* out_views, void* stream) {
  const char* who = "dbhip_str_split_part";
  int32_t rc = check_common(col, 0, n, who);
  if (rc) return rc;
  if ((rc = check_const(delim_host, delim_len, "delimiter", who))) return rc;
  if ((rc = check_i64(part, true, n, "part", who))) return rc;
  if (n == 0) return DBHIP_OK;
  if (!col->data || !out_views || ((uintptr_t)out_views & 15) || ((uintptr_t)col->data & 15)) {
    set_error("%s: NULL views or out_views, or views not 16-byte aligned", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  SearchParams P;
  base_params(P, col, part, n, 0);
  P.out_views = (uint4*)out_views;
  ss_prepare(P.C, delim_host, (uint32_t)delim_len, nullptr, 0, true);
  return long_two_passes(P, ss_split_kernel, ss_split_long_kernel, SS_SCRATCH_SLOT, s, who);
}

int32_t dbhip_str_rewrite_bytes(int32_t op, const dbhip_col* col, const dbhip_col* k, const uint8_t* x_host, int32_t x_len, const uint8_t* y_host,
                                int32_t y_len, int32_t flags, int64_t n, uint64_t* out_bytes_host, void* stream) {
  const char* who = "dbhip_str_rewrite_bytes";
  SearchParams P;
  const int32_t rc = rewrite_params(op, col, k, x_host, x_len, y_host, y_len, flags, n, P, who);
  if (rc) return rc;
  if (!out_bytes_host) { set_error("%s: NULL out_bytes_host", who); return DBHIP_ERR_INVALID; }
  *out_bytes_host = 0;
  if (n == 0) return DBHIP_OK;
  hipStream_t s = resolve_stream(stream);
  uint8_t* ws = (uint8_t*)scratch(long_list_bytes(n), SS_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  P.list = long_list_at(ws);
  P.total = (unsigned long long*)(ws + 8);
  DBHIP_CHECK(long_list_clear(ws, s));
  hipLaunchKernelGGL(ss_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  long_launch(ss_count_long_kernel, P, s);
  DBHIP_LAUNCH_CHECK();
  uint64_t* host = pinned_words(0);
  DBHIP_CHECK(hipMemcpyAsync(host, ws + 8, 8, hipMemcpyDeviceToHost, s));
  DBHIP_CHECK(hipStreamSynchronize(s));
  *out_bytes_host = host[0];
  return DBHIP_OK;
}

int32_t dbhip_str_rewrite(int32_t op, const dbhip_col* col, const dbhip_col* k, const uint8_t* x_host, int32_t x_len, const uint8_t* y_host,
                          int32_t y_len, int32_t flags, int64_t n, void* out_views, uint8_t* out_data, uint64_t out_data_bytes,
                          uint64_t* err_count_dev, void* stream) {
  const char* who = "dbhip_str_rewrite";
  SearchParams P;
  const int32_t rc = rewrite_params(op, col, k, x_host, x_len, y_host, y_len, flags, n, P, who);
  if (rc) return rc;
  if (n == 0) return DBHIP_OK;
  if (!out_views || ((uintptr_t)out_views & 15) || ((uintptr_t)err_count_dev & 7) || (out_data_bytes > 0 && !out_data)) {
    set_error("%s: NULL or misaligned out_views, err_count_dev not 8-byte aligned, or out_data_bytes without out_data", who);
    return DBHIP_ERR_INVALID;
  }
  hipStream_t s = resolve_stream(stream);
  // scratch: the two lists' counts | counts | offsets | block sums | wave-counted lengths | row ids of the count's list | of the fill's
  const size_t nn = (size_t)n, nblk = (size_t)ceil_div(n, SCAN_TILE) + 2;
  const size_t off_counts = 64, off_offsets = off_counts + ((nn * 4 + 63) & ~(size_t)63), off_blk = off_offsets + nn * 8, off_lens = off_blk + nblk * 8,
               off_rows_a = off_lens + nn * 8, off_rows_b = off_rows_a + nn * 4;
  uint8_t* ws = (uint8_t*)scratch(off_rows_b + nn * 4 + 64, SS_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  P.counts = (uint32_t*)(ws + off_counts);
  P.offsets = (const uint64_t*)(ws + off_offsets);
  P.lens = (uint64_t*)(ws + off_lens);
  P.out_views = (uint4*)out_views;
  P.out_data = out_data;
  P.out_data_bytes = out_data_bytes;
  P.err_count = (unsigned long long*)err_count_dev;
  P.list = long_list_at(ws, 0, off_rows_a);
  DBHIP_CHECK(long_list_clear(ws, s));
  hipLaunchKernelGGL(ss_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  long_launch(ss_count_long_kernel, P, s);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  const int32_t src = dbscan::exclusive_scan_u32(P.counts, n, (uint64_t*)(ws + off_blk), (uint64_t*)(ws + off_offsets), s);
  if (src) return src;
  DBHIP_POLL_CANCEL(s, who);
  P.list = long_list_at(ws, 1, off_rows_b);
  hipLaunchKernelGGL(ss_fill_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  long_launch(ss_fill_long_kernel, P, s);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

}  // extern "C"
