// dev_strwave.h — the String column frame of k_strfn.hip and k_strsearch.hip, and a long value as aligned words for one wave.
//
// StrCol is a String column in a kernel's parameter struct; str_value is what a lane of pass 1 reads of a row, str_bytes what a wave of
// pass 2 does. WaveWords walks a value by naturally aligned 4-byte words that each hold a byte of it, 64 words per step; the unit
// boundaries of a step are four ballots (Ballots), and wave_forward finds the k-th of them.
// The types here have external linkage (their copies sat in anonymous namespaces): a kernel file that wants a StrCol, WaveWords or
// Ballots of its own shape must keep it in its anonymous namespace, or two definitions under one name meet in the library unnoticed.
// HIP only: not for the headers the host checkers compile, and not embedded for the run-time specialised kernels (the Makefile's JIT_HDRS).
#pragma once
#include "dev_common.h"
#include "dev_strfn.h"
#include "dev_longrows.h"

struct StrCol {
  const uint4* views;
  const uint8_t* validity;
  int64_t voff;
  const void* const* buffers;
  int32_t n_buffers, scalar;
};
inline StrCol str_col(const dbhip_col* c) {
  StrCol s;
  s.views = (const uint4*)c->data;
  s.validity = c->validity;
  s.voff = c->validity_offset;
  s.buffers = c->buffers;
  s.n_buffers = c->buffers && c->n_buffers > 0 ? c->n_buffers : 0;
  s.scalar = c->is_scalar ? 1 : 0;
  return s;
}

// row i of a column: false for a NULL row (*null_row) and for a long view that points nowhere; neither is dereferenced
__device__ __forceinline__ bool str_value(const StrCol& c, int64_t i, SfValue& v, uint32_t& index, uint32_t& offset, bool& null_row) {
  const int64_t r = c.scalar ? 0 : i;
  null_row = c.validity && !bit_get(c.validity, c.voff + r);
  if (null_row) return false;
  const uint4 vw = c.views[r];
  const uint8_t* bytes = nullptr;
  if (!sv_bytes_checked(c.views + r, vw.x, vw.z, vw.w, c.buffers, c.n_buffers, &bytes)) return false;
  v = sf_value(vw.x, vw.y, vw.z, vw.w, bytes);
  index = vw.z;
  offset = vw.w;
  return true;
}
__device__ __forceinline__ bool str_value(const StrCol& c, int64_t i, SfValue& v, uint32_t& index, uint32_t& offset) {
  bool null_row;
  return str_value(c, i, v, index, offset, null_row);
}
// the bytes of row i for a wave: pass 1 has found the row usable. An inline value is read in place, in the view.
__device__ __forceinline__ const uint8_t* str_bytes(const StrCol& c, int64_t i, uint4& vw) {
  const int64_t r = c.scalar ? 0 : i;
  vw = c.views[r];
  return sv_is_inline(vw.x) ? (const uint8_t*)(c.views + r) + 4 : (const uint8_t*)c.buffers[vw.z] + vw.w;
}

// ---- a long value as aligned words, for one wave -------------------------------------------------------------------------------------------
struct WaveWords {
  const uint32_t* words;   // the aligned word that holds the value's first byte
  uint32_t lead, len, nwords;
};
__device__ __forceinline__ WaveWords ww_of(uintptr_t base, uint32_t len) {
  WaveWords W;
  W.lead = (uint32_t)(base & 3);
  W.words = (const uint32_t*)(base - W.lead);
  W.len = len;
  W.nwords = (uint32_t)(((uint64_t)W.lead + len + 3) >> 2);
  return W;
}
// word `widx` (only when it holds a byte of the value) and the 4-bit mask of its bytes whose positions lie in [lo, hi)
__device__ __forceinline__ uint32_t ww_load(const WaveWords& W, int64_t widx, uint32_t lo, uint32_t hi, uint32_t& in) {
  in = 0;
  if (widx < 0 || widx >= (int64_t)W.nwords) return 0;
  const int64_t p0 = widx * 4 - W.lead;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (p0 + j >= (int64_t)lo && p0 + j < (int64_t)hi) in |= 1u << j;
  return in ? W.words[widx] : 0u;
}
__device__ __forceinline__ uint32_t ww_byte(const WaveWords& W, uint32_t pos) {   // pos < len
  const uint64_t a = (uint64_t)W.lead + pos;
  return (W.words[a >> 2] >> (8 * (uint32_t)(a & 3))) & 0xFFu;
}
__device__ __forceinline__ uint32_t noncont4(uint32_t w) {   // bit j: byte j is not 10xxxxxx
  const uint32_t nc = ~((w >> 7) & ~(w >> 6)) & 0x01010101u;
  return (nc | (nc >> 7) | (nc >> 14) | (nc >> 21)) & 0xFu;
}
__device__ __forceinline__ uint64_t lanes_above(uint32_t lane) { return lane == 63 ? 0ull : (~0ull << (lane + 1)); }
__device__ __forceinline__ uint64_t lanes_from(uint32_t lane) { return lane >= 64 ? 0ull : (~0ull << lane); }

// the boundaries of a step as four ballots; returns their number
struct Ballots { uint64_t b[4]; };
__device__ __forceinline__ uint32_t ballots_of(uint32_t bits, Ballots& B) {
  uint32_t total = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { B.b[j] = __ballot((bits >> j) & 1u); total += (uint32_t)__popcll(B.b[j]); }
  return total;
}
__device__ __forceinline__ uint32_t ballots_masked(const Ballots& B, uint64_t m) {
  return (uint32_t)(__popcll(B.b[0] & m) + __popcll(B.b[1] & m) + __popcll(B.b[2] & m) + __popcll(B.b[3] & m));
}

// sf_forward for the wave (k >= 1): the k-th boundary behind `from`, len when the value ends first
__device__ __forceinline__ uint32_t wave_forward(const WaveWords& W, uint32_t from, uint32_t k, uint32_t lane) {
  if (from + 1 >= W.len) return W.len;
  uint32_t rem = k;
  for (int64_t wb = ((int64_t)W.lead + from + 1) >> 2; wb < (int64_t)W.nwords; wb += 64) {      // wave-uniform bounds
    const int64_t widx = wb + lane;
    uint32_t in;
    const uint32_t w = ww_load(W, widx, from + 1, W.len, in);
    const uint32_t bits = noncont4(w) & in;
    Ballots B;
    const uint32_t total = ballots_of(bits, B);
    if (rem <= total) {
      const uint32_t before = ballots_masked(B, lanes_below(lane));
      const bool hit = before < rem && rem <= before + (uint32_t)__popc(bits);
      uint32_t pos = 0, r = rem - before;
      if (hit) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((bits >> j) & 1u) { if (--r == 0) pos = (uint32_t)(widx * 4 + j - W.lead); }
      }
      const uint64_t hm = __ballot(hit);
      return (uint32_t)__shfl((int)pos, __ffsll((unsigned long long)hm) - 1, 64);
    }
    rem -= total;
  }
  return W.len;
}
