// dev_strview.h — the 16-byte String view, once (DESIGN.md "The String view"). A String column is an array of views
//   {len, w1, w2, w3}   four little-endian 32-bit words (binview/view.rs:30-42)
//   len <= 12 : the value's bytes sit in w1..w3 (the view's bytes 4..15); what lies past `len` there is NOT defined
//   len  > 12 : w1 = the first four bytes, w2 = index into the column's buffer table, w3 = byte offset inside that buffer
// Free of HIP so that a host program compiles the very same text (tests/strview_host_check.cpp). SV_FN is the functions' qualifier:
// an includer may define it, otherwise it is host + device under a HIP compiler and plain `inline` elsewhere.
#pragma once
#ifndef __HIPCC_RTC__
#include <stdint.h>
#endif

#if !defined(SV_FN) && (defined(__HIP__) || defined(__HIPCC_RTC__))
#define SV_FN __host__ __device__ __forceinline__
#elif !defined(SV_FN)
#define SV_FN inline
#endif

constexpr uint32_t SV_INLINE_MAX = 12;   // the longest value that lives in the view itself

SV_FN bool sv_is_inline(uint32_t len) { return len <= SV_INLINE_MAX; }

// The canonical words of an inline view: the bytes past `len` zeroed (branch-free), so that equal strings are equal words.
// Returns whether the view is inline; the words of a long view are left as they are.
SV_FN bool sv_canon(uint32_t len, uint32_t& w1, uint32_t& w2, uint32_t& w3) {
  const uint32_t m1 = len >= 4 ? 0xffffffffu : (len == 0 ? 0u : (0xffffffffu >> (8 * (4 - len))));
  const uint32_t m2 = len >= 8 ? 0xffffffffu : (len <= 4 ? 0u : (0xffffffffu >> (8 * (8 - len))));
  const uint32_t m3 = len >= 12 ? 0xffffffffu : (len <= 8 ? 0u : (0xffffffffu >> (8 * (12 - len))));
  w1 &= m1; w3 &= m3; w2 &= m2;   // in the order the fused kernels' key words use them: their instruction schedule follows it
  return sv_is_inline(len);
}
// The same as the two key words of gb_layout.h: k0 = len | w1 << 32, k1 = w2 | w3 << 32.
SV_FN bool sv_key_words(uint32_t len, uint32_t w1, uint32_t w2, uint32_t w3, uint64_t& k0, uint64_t& k1) {
  const bool in = sv_canon(len, w1, w2, w3);
  k0 = ((uint64_t)w1 << 32) | len;
  k1 = ((uint64_t)w3 << 32) | w2;
  return in;
}

// Where the value's bytes are. `view` is the address of the view itself: an inline value is read in place.
// UNCHECKED: a long view's index is trusted (DESIGN.md lists the callers).
SV_FN const uint8_t* sv_bytes(const void* view, const void* const* buffers) {
  const uint32_t* v = (const uint32_t*)view;
  return sv_is_inline(v[0]) ? (const uint8_t*)(v + 1) : (const uint8_t*)buffers[v[2]] + v[3];
}
// The same for a caller that holds the view's words in registers already.
SV_FN const uint8_t* sv_bytes(const void* view, uint32_t len, uint32_t index, uint32_t offset, const void* const* buffers) {
  if (sv_is_inline(len)) return (const uint8_t*)view + 4;
  return (const uint8_t*)buffers[index] + offset;
}

// The same, checked: false, and *bytes untouched, for a long view whose index lies past the table's n_buffers entries (0 when there
// is no table, never negative) or whose entry is null. Nothing is read through the table or the entry in those cases.
SV_FN bool sv_bytes_checked(const void* view, uint32_t len, uint32_t index, uint32_t offset, const void* const* buffers, int32_t n_buffers,
                            const uint8_t** bytes) {
  if (sv_is_inline(len)) { *bytes = (const uint8_t*)view + 4; return true; }
  if (index >= (uint32_t)n_buffers || buffers[index] == nullptr) return false;
  *bytes = (const uint8_t*)buffers[index] + offset;
  return true;
}

// The view of the `len` bytes at `bytes`, which (when longer than 12) lie at `offset` of buffer `index` of the column.
SV_FN void sv_make(const uint8_t* bytes, uint32_t len, uint32_t index, uint32_t offset, uint32_t (&w)[4]) {
  w[0] = len; w[1] = 0; w[2] = 0; w[3] = 0;
  if (sv_is_inline(len)) {
    for (uint32_t b = 0; b < len; ++b) w[1 + (b >> 2)] |= (uint32_t)bytes[b] << (8 * (b & 3));
  } else {
    w[1] = (uint32_t)bytes[0] | ((uint32_t)bytes[1] << 8) | ((uint32_t)bytes[2] << 16) | ((uint32_t)bytes[3] << 24);
    w[2] = index;
    w[3] = offset;
  }
}

// A long view moves to another buffer table (index) or to another place in its buffer (offset); an inline view stays as it is.
SV_FN void sv_rebase(uint32_t len, uint32_t& index, uint32_t& offset, uint32_t index_add, uint32_t offset_add) {
  if (!sv_is_inline(len)) { index += index_add; offset += offset_add; }
}
