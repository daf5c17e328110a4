// dev_inlist.h — the row logic of constant IN-list membership (include/dbhip.h a23): the canonical key image of a value, the hash, the
// table build, the probe, the linear comparison and the String tail comparison. Free of HIP, in the style of dev_strfn.h and
// like_match.h, so that a host program compiles the very same text (tests/inlist_host_check.cpp). IN_FN is the functions' qualifier;
// IN_LOAD_U32(addr, base, len) is how an aligned word of a long String value (its first byte at `base`, `len` bytes) is read: the
// includer may define both.
//
// Key image. Every value becomes two 64-bit words (k0, k1); equal values — in the sense of dbhip_cmp(DBHIP_CMP_EQ) — have equal images.
//   integers, Date, Timestamp, DEC64   k0 = the value's bits zero-extended from its width, k1 = 0
//   F32 / F64                          the same after inl_canon_f32 / _f64: every NaN is one NaN, -0.0 is +0.0 (OrderedFloat)
//   DEC128                             k0 = low word, k1 = high word
//   String of <= 12 bytes              sv_key_words: k0 = len | w1 << 32, k1 = w2 | w3 << 32, the bytes past len zeroed
//   String of more bytes               k0 = len | first four bytes << 32; an ELEMENT's k1 is the byte offset of its bytes in the set's
//                                      long-byte block (a multiple of 4, the element zero-padded to whole words); a column VALUE has
//                                      no k1: it hashes with k1 = 0 and a slot that matches k0 is verified by inl_tail_equal
// Table. Open addressing, linear probing, inl_slots(n) = the power of two >= 2 n (at least 4) slots of 8 bytes (k0; types of <= 8
// bytes) or 16 bytes (k0, k1; DEC128 and Strings). The load is at most one half, so every probe run ends at an empty slot. An empty
// slot holds the all-ones key INL_EMPTY (in both words of a wide slot). That key is legal column data (U64 2^64 - 1, I64 -1, DEC128 -1),
// so it is never stored: a list that holds it says so in the set's `has_sentinel`, and a row that equals it is answered from that flag
// alone, before any probe. No String has that image (a length of 2^32 - 1 is never inline, and a long value is told apart by is_long).
// Equality needs equal length, so a lane compares at most 255 bytes (the longest element) however long the column's value is.
#pragma once
#include <stdint.h>
#include "dev_strview.h"

#if !defined(IN_FN) && defined(__HIP__)
#define IN_FN __host__ __device__ __forceinline__
#elif !defined(IN_FN)
#define IN_FN inline
#endif
#ifndef IN_LOAD_U32
#define IN_LOAD_U32(addr, base, len) (*(const uint32_t*)(addr))
#endif

// Lists of at most this many distinct elements are compared one by one (COMPARE); longer ones go through the table (TABLE).
// DESIGN.md §2.15 has the measurements behind the value.
constexpr int INL_COMPARE_MAX = 7;
constexpr int INL_MAX_ITEMS = 1024, INL_MAX_ITEM_BYTES = 255, INL_MAX_LONG_BYTES = 16384;
constexpr uint64_t INL_EMPTY = ~0ull;

IN_FN uint32_t inl_canon_f32(uint32_t b) {
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC00000u;   // every NaN
  return b == 0x80000000u ? 0u : b;                          // -0.0
}
IN_FN uint64_t inl_canon_f64(uint64_t b) {
  if ((b & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0x7FF8000000000000ull;
  return b == 0x8000000000000000ull ? 0ull : b;
}

IN_FN uint64_t inl_hash(uint64_t k0, uint64_t k1) {
  uint64_t x = k0 ^ (k1 * 0x9E3779B97F4A7C15ull);
  x ^= x >> 32;
  x *= 0xd6e8feb86659fd93ull;
  x ^= x >> 32;
  x *= 0xd6e8feb86659fd93ull;
  x ^= x >> 32;
  return x;
}
IN_FN uint32_t inl_slots(uint32_t n_items) {
  uint32_t s = 4;
  while (s < 2 * n_items) s <<= 1;
  return s;
}

// One column value, ready to be looked up. A long String carries where its bytes are instead of k1; nothing is read through
// `buffers` before a slot (or an element) has matched k0, that is: length and first four bytes.
struct InlValue {
  uint64_t k0, k1;
  bool is_long;
  uint32_t index, offset;
  const void* const* buffers;
  int32_t n_buffers;
};
IN_FN InlValue inl_value(uint64_t k0, uint64_t k1) { return InlValue{k0, k1, false, 0, 0, nullptr, 0}; }
// the value of a view held in registers
IN_FN InlValue inl_string_value(uint32_t len, uint32_t w1, uint32_t w2, uint32_t w3, const void* const* buffers, int32_t n_buffers) {
  InlValue v{0, 0, false, w2, w3, buffers, n_buffers};
  if (!sv_key_words(len, w1, w2, w3, v.k0, v.k1)) { v.is_long = true; v.k1 = 0; }
  return v;
}

IN_FN uint32_t inl_low_mask(uint32_t nbytes) { return nbytes >= 4 ? 0xFFFFFFFFu : ((1u << (8 * nbytes)) - 1u); }

// Bytes [4, len) of the long value `v` (len = the low half of k0, 13 .. 255 here) against the element whose words begin at ew (its
// first word holds bytes 0..3, which k0 has compared already). Naturally aligned 4-byte loads, each covering at least one byte of the
// value, as like_match.h's like_cmp_range. A view whose buffer index is >= n_buffers or whose table entry is NULL matches nothing.
IN_FN bool inl_tail_equal(const InlValue& v, const uint32_t* ew) {
  if (v.index >= (uint32_t)v.n_buffers || v.buffers[v.index] == nullptr) return false;
  const uintptr_t base = (uintptr_t)v.buffers[v.index] + v.offset;
  const uint32_t len = (uint32_t)v.k0, cnt = len - 4;
  const uintptr_t a = base + 4;
  uintptr_t p = a & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)(a & 3) * 8, have = 4 - (uint32_t)(a & 3);   // value bytes the word at p still holds
  uint32_t cur = IN_LOAD_U32(p, base, len);
  for (uint32_t i = 0; i < cnt; i += 4) {
    const uint32_t rem = cnt - i;
    const uint32_t nxt = rem > have ? IN_LOAD_U32(p + 4, base, len) : 0u;   // (read only when one of its bytes is compared)
    const uint32_t w = sh ? ((cur >> sh) | (nxt << (32 - sh))) : cur;
    if ((w ^ ew[1 + (i >> 2)]) & inl_low_mask(rem)) return false;
    cur = nxt;
    p += 4;
  }
  return true;
}

// does the stored key (s0, s1) equal the value? `wide`: 16-byte keys. long_words: the set's long-byte block.
IN_FN bool inl_key_equal(uint64_t s0, uint64_t s1, const InlValue& v, bool wide, const uint32_t* long_words) {
  if (s0 != v.k0) return false;
  if (!wide) return true;
  if (!v.is_long) return s1 == v.k1;
  return inl_tail_equal(v, long_words + ((uint32_t)s1 >> 2));
}

IN_FN bool inl_is_sentinel(const InlValue& v, bool wide) { return !v.is_long && v.k0 == INL_EMPTY && (!wide || v.k1 == INL_EMPTY); }

// TABLE: `table` = slots keys of one or two words. The caller has answered the sentinel already.
IN_FN bool inl_table_probe(const uint64_t* table, uint32_t slots, bool wide, const InlValue& v, const uint32_t* long_words) {
  const uint32_t mask = slots - 1;
  uint32_t at = (uint32_t)inl_hash(v.k0, v.k1) & mask;
  for (uint32_t step = 0; step < slots; ++step) {   // (the bound never ends the loop: half the slots are empty)
    const uint64_t s0 = wide ? table[2 * at] : table[at], s1 = wide ? table[2 * at + 1] : 0;
    if (s0 == INL_EMPTY && (!wide || s1 == INL_EMPTY)) return false;
    if (inl_key_equal(s0, s1, v, wide, long_words)) return true;   // on a tail mismatch the run goes on: two elements may share k0
    at = (at + 1) & mask;
  }
  return false;
}

// COMPARE: `items` = n keys of two words each, whatever the type's width.
IN_FN bool inl_compare_probe(const uint64_t (*items)[2], uint32_t n, bool wide, const InlValue& v, const uint32_t* long_words) {
  bool hit = false;
  for (uint32_t k = 0; k < n; ++k) hit = hit || inl_key_equal(items[k][0], items[k][1], v, wide, long_words);
  return hit;
}

IN_FN bool inl_member(const InlValue& v, bool wide, bool has_sentinel, const uint64_t* table, uint32_t slots,
                      const uint64_t (*items)[2], uint32_t n_items, const uint32_t* long_words) {
  if (inl_is_sentinel(v, wide)) return has_sentinel;
  return slots ? inl_table_probe(table, slots, wide, v, long_words) : inl_compare_probe(items, n_items, wide, v, long_words);
}

// ---- host: the table build -----------------------------------------------------------------------------------------------------------
// Puts the key into a table that inl_table_probe reads; `long_element`: hash k0 alone (k1 is the offset of the bytes). Returns false
// when an equal key is there already. The caller gives equal long elements one offset, so they are equal keys too, and never passes
// the sentinel.
inline bool inl_table_insert(uint64_t* table, uint32_t slots, bool wide, uint64_t k0, uint64_t k1, bool long_element) {
  const uint32_t mask = slots - 1;
  uint32_t at = (uint32_t)inl_hash(k0, long_element ? 0 : k1) & mask;
  for (;;) {
    uint64_t& s0 = wide ? table[2 * at] : table[at];
    if (s0 == INL_EMPTY && (!wide || table[2 * at + 1] == INL_EMPTY)) {
      s0 = k0;
      if (wide) table[2 * at + 1] = k1;
      return true;
    }
    if (s0 == k0 && (!wide || table[2 * at + 1] == k1)) return false;
    at = (at + 1) & mask;
  }
}

// ---- host: a list of constants -> what the kernels read ---------------------------------------------------------------------------------
// dbhip_inlist_create and the host checker prepare a set with this same text: the key image of every element, duplicates removed, the
// sentinel kept as a flag, long String elements packed into the long-byte block (equal ones share one offset), then the path and the
// image: the bitmap (BITS), nothing but the long-byte block (COMPARE: the keys go into `items`), or the table followed by that block.
#include <string.h>
#include <vector>

enum { INL_PATH_BITS = 0, INL_PATH_COMPARE = 1, INL_PATH_TABLE = 2 };        // the public dbhip_inlist_path_t (k_inlist.hip asserts it)
enum { INL_ADD_OK = 0, INL_ADD_ITEM_TOO_LONG = 1, INL_ADD_TOO_MANY_LONG_BYTES = 2 };

struct InlSet {
  int elem_size = 8;            // 1, 2, 4, 8 or 16 bytes; Strings: 16
  bool is_float = false, is_string = false, has_sentinel = false;
  std::vector<uint64_t> k0s, k1s;   // distinct keys, the sentinel not among them
  std::vector<uint8_t> is_long;
  std::vector<uint32_t> long_words, bitmap;
  size_t long_bytes = 0;        // of all long elements given, duplicates included
  // what inl_set_finish decides
  int path = INL_PATH_COMPARE;
  uint32_t slots = 0, long_at = 0;
  std::vector<uint32_t> image;
  uint64_t items[INL_COMPARE_MAX][2] = {};
  bool bits() const { return elem_size <= 2; }
  bool wide() const { return elem_size == 16; }
};

inline void inl_set_init(InlSet& s, int elem_size, bool is_float, bool is_string) {
  s = InlSet();
  s.elem_size = elem_size; s.is_float = is_float; s.is_string = is_string;
  if (s.bits()) s.bitmap.assign(elem_size == 1 ? 8 : 2048, 0u);
}
inline void inl_set_add_key(InlSet& s, uint64_t k0, uint64_t k1, bool lng) {
  if (s.bits()) { s.bitmap[k0 >> 5] |= 1u << (k0 & 31); return; }
  if (!lng && k0 == INL_EMPTY && (!s.wide() || k1 == INL_EMPTY)) { s.has_sentinel = true; return; }
  for (size_t e = 0; e < s.k0s.size(); ++e)
    if (s.k0s[e] == k0 && s.k1s[e] == k1 && (s.is_long[e] != 0) == lng) return;
  s.k0s.push_back(k0); s.k1s.push_back(k1); s.is_long.push_back(lng);
}
// one element of a fixed-width type: its elem_size little-endian bytes
inline void inl_set_add_fixed(InlSet& s, const uint8_t* p) {
  uint64_t k0 = 0, k1 = 0;
  memcpy(&k0, p, s.elem_size < 8 ? s.elem_size : 8);
  if (s.elem_size == 16) memcpy(&k1, p + 8, 8);
  if (s.is_float) k0 = s.elem_size == 4 ? inl_canon_f32((uint32_t)k0) : inl_canon_f64(k0);
  inl_set_add_key(s, k0, k1, false);
}
// one String element; INL_ADD_* says why a list is refused
inline int inl_set_add_string(InlSet& s, const uint8_t* p, uint32_t len) {
  if (len > (uint32_t)INL_MAX_ITEM_BYTES) return INL_ADD_ITEM_TOO_LONG;
  uint64_t k0 = 0, k1 = 0;
  if (sv_is_inline(len)) {
    uint32_t w[4];
    sv_make(p, len, 0, 0, w);
    sv_key_words(w[0], w[1], w[2], w[3], k0, k1);
    inl_set_add_key(s, k0, k1, false);
    return INL_ADD_OK;
  }
  s.long_bytes += len;
  if (s.long_bytes > (size_t)INL_MAX_LONG_BYTES) return INL_ADD_TOO_MANY_LONG_BYTES;
  uint32_t pre;
  memcpy(&pre, p, 4);
  k0 = ((uint64_t)pre << 32) | len;
  const uint32_t nw = (len + 3) / 4;
  std::vector<uint32_t> ew(nw, 0u);
  memcpy(ew.data(), p, len);
  uint32_t at = (uint32_t)s.long_words.size();
  for (size_t e = 0; e < s.k0s.size(); ++e)   // an equal element seen before: its offset
    if (s.is_long[e] && s.k0s[e] == k0 && !memcmp(&s.long_words[s.k1s[e] / 4], ew.data(), (size_t)nw * 4)) { at = (uint32_t)(s.k1s[e] / 4); break; }
  if (at == s.long_words.size()) s.long_words.insert(s.long_words.end(), ew.begin(), ew.end());
  inl_set_add_key(s, k0, (uint64_t)at * 4, true);
  return INL_ADD_OK;
}
// `force_table`: the host checker's way to probe a table of few elements; the library passes false
inline void inl_set_finish(InlSet& s, bool force_table) {
  const uint32_t n = (uint32_t)s.k0s.size();
  s.image.clear();
  s.slots = 0;
  if (s.bits()) {
    s.path = INL_PATH_BITS;
    s.image = s.bitmap;
  } else if (!force_table && n + (s.has_sentinel ? 1u : 0u) <= (uint32_t)INL_COMPARE_MAX) {
    s.path = INL_PATH_COMPARE;
    for (uint32_t e = 0; e < n; ++e) { s.items[e][0] = s.k0s[e]; s.items[e][1] = s.k1s[e]; }
  } else {
    s.path = INL_PATH_TABLE;
    s.slots = inl_slots(n);
    std::vector<uint64_t> table((size_t)s.slots * (s.wide() ? 2 : 1), INL_EMPTY);
    for (uint32_t e = 0; e < n; ++e) inl_table_insert(table.data(), s.slots, s.wide(), s.k0s[e], s.k1s[e], s.is_long[e] != 0);
    s.image.resize(table.size() * 2);
    memcpy(s.image.data(), table.data(), table.size() * 8);
  }
  s.long_at = (uint32_t)s.image.size();
  if (!s.bits()) s.image.insert(s.image.end(), s.long_words.begin(), s.long_words.end());
  while (s.image.size() % 4) s.image.push_back(0u);   // whole 16-byte units: the kernels stage the image with 16-byte loads
}
