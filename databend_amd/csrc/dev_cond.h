// dev_cond.h — the row-level logic of the conditionals (include/dbhip.h a27): CASE / if, coalesce and Kleene AND / OR / NOT / XOR.
// Free of HIP, in the style of dev_strview.h and dev_math.h, so that a host program compiles the very same text
// (tests/cond_host_check.cpp). CD_FN is the functions' qualifier: an includer may define it. Nothing but <stdint.h> is included.
//
// Everything here works on 64-ROW WORDS of LSB-first Bitmaps. A conditional is a select, and which branch a row takes is a function of
// Bitmaps alone — the conditions' values and validities for a CASE, the arguments' validities for a coalesce — so 64 rows are decided
// by a handful of word operations and no row is looked at on its own:
//   cd_fetch64      64 bits of a Bitmap from an arbitrary bit position (validity_offset + row), never a byte that holds none of them
//   CdChooser       the chooser: fed the branches in order, it hands back for each the rows that take it (the first TRUE condition,
//                   the first valid argument), and at the end the rows nothing took
//   cd_kleene       the four three-valued operators of dbhip_bool_logic
//   cd_expand_*     a few row bits widened to the bytes those rows occupy, for the masked merge of a chosen branch's elements
//   cd_check        what dbhip_case_check decides, over the descriptors' plain fields
//   cd_table_bases  where each argument's buffer table starts in the result's table (Strings)
#pragma once
#include <stdint.h>

#if !defined(CD_FN) && (defined(__HIP__) || defined(__HIPCC_RTC__))
#define CD_FN __host__ __device__ inline __attribute__((always_inline))
#elif !defined(CD_FN)
#define CD_FN inline
#endif

// the operator codes, the limit and the type codes are the public ones (k_cond.hip asserts it)
enum { CD_AND = 0, CD_OR = 1, CD_NOT = 2, CD_XOR = 3, CD_OP_COUNT = 4 };
constexpr int CD_MAX_CONDS = 16;                 // conditions of one CASE; a coalesce takes CD_MAX_CONDS + 1 arguments
constexpr int CD_MAX_VALUES = CD_MAX_CONDS + 1;
enum { CD_T_BOOL = 1, CD_T_DEC64 = 14, CD_T_DEC128 = 15, CD_T_STRING = 16, CD_T_DEC256 = 17 };
enum { CD_OK = 0, CD_INVALID = 1, CD_UNSUPPORTED = 7 };

// ---- Bitmaps ------------------------------------------------------------------------------------------------------------------------
// Bits [bit, bit + count) of the LSB-first Bitmap `bm`, 1 <= count <= 64, as the low bits of a word; the bits above them are zero.
// An 8-byte aligned Bitmap is read as one or two aligned 64-bit words, each of which holds at least one of the bits asked for (on the
// device such a word lies in the page of that bit; a host caller sizes an aligned Bitmap in whole words). Any other Bitmap is read byte
// by byte, and only the bytes that hold an asked bit.
CD_FN uint64_t cd_fetch64(const uint8_t* bm, int64_t bit, int count) {
  const uint64_t keep = count >= 64 ? ~0ull : ((1ull << count) - 1);
  if ((((uintptr_t)bm) & 7) == 0) {
    const uint64_t* w = (const uint64_t*)bm + (bit >> 6);
    const int sh = (int)(bit & 63);
    uint64_t r = w[0] >> sh;
    if (sh + count > 64) r |= w[1] << (64 - sh);
    return r & keep;
  }
  const uint8_t* p = bm + (bit >> 3);
  const int sh = (int)(bit & 7);
  const int nbytes = (sh + count + 7) >> 3;      // 1 .. 9
  uint64_t r = 0;
  for (int b = 0; b < 8 && b < nbytes; ++b) r |= (uint64_t)p[b] << (8 * b);
  r >>= sh;
  if (nbytes == 9) r |= (uint64_t)p[8] << (64 - sh);   // sh > 0 here
  return r & keep;
}

// the word of a constant: all rows alike
CD_FN uint64_t cd_splat(bool bit) { return bit ? ~0ull : 0ull; }

// the rows of the word that starts at row `row0` which exist in a column of n rows
CD_FN uint64_t cd_live(int64_t row0, int64_t n) {
  const int64_t left = n - row0;
  return left >= 64 ? ~0ull : (left <= 0 ? 0ull : ((1ull << left) - 1));
}

// ---- the chooser --------------------------------------------------------------------------------------------------------------------
// Branches are offered in order. A CASE offers condition k as (value word, validity word): the rows where it is TRUE are value AND
// validity — a NULL condition is not TRUE whatever its payload bit says — and ELSE as all ones. A coalesce offers argument k's
// validity word. take() returns the rows that take the branch offered: those where it is TRUE and no earlier branch was.
struct CdChooser {
  uint64_t open;                                 // rows no branch has taken yet
};
CD_FN CdChooser cd_chooser(uint64_t live) { CdChooser c; c.open = live; return c; }
CD_FN uint64_t cd_true_rows(uint64_t value, uint64_t validity) { return value & validity; }
CD_FN uint64_t cd_take(CdChooser& c, uint64_t true_rows) {
  const uint64_t m = c.open & true_rows;
  c.open &= ~true_rows;
  return m;
}
// what is left when every branch has been offered: the NULL rows of a coalesce; none after a CASE, whose ELSE takes every row
CD_FN uint64_t cd_rest(const CdChooser& c) { return c.open; }

// ---- Kleene logic -------------------------------------------------------------------------------------------------------------------
// a, b: value words; va, vb: validity words (all ones for an operand that has none). t: the rows that are TRUE; v: the rows that are
// not NULL. FALSE and NULL rows both have t = 0. NOT ignores b and vb.
CD_FN void cd_kleene(int op, uint64_t a, uint64_t va, uint64_t b, uint64_t vb, uint64_t& t, uint64_t& v) {
  switch (op) {
    case CD_AND: v = (va & vb) | (va & ~a) | (vb & ~b); t = va & a & vb & b; break;
    case CD_OR:  v = (va & vb) | (va & a) | (vb & b);   t = (va & a) | (vb & b); break;
    case CD_NOT: v = va;                                t = va & ~a; break;
    default:     v = va & vb;                           t = v & (a ^ b); break;
  }
}

// ---- row bits to element bytes ------------------------------------------------------------------------------------------------------
// four row bits -> the four bytes of a 32-bit word, 0xFF where the bit is set (rows of one byte); two row bits -> its two halves
CD_FN uint32_t cd_expand_bytes(uint32_t bits4) {
  const uint32_t x = (bits4 & 1u) | ((bits4 & 2u) << 7) | ((bits4 & 4u) << 14) | ((bits4 & 8u) << 21);   // bits 0, 8, 16, 24
  return x * 0xFFu;
}
CD_FN uint32_t cd_expand_halves(uint32_t bits2) {
  return ((bits2 & 1u) ? 0x0000FFFFu : 0u) | ((bits2 & 2u) ? 0xFFFF0000u : 0u);
}
// The mask of 32-bit word d of a lane's run of rows: `bits` holds one bit per row of the run, a row is SIZE bytes, the run is
// consecutive rows from its first byte on. SIZE 1, 2: several rows per word; 4: one; 8, 16, 32: a row is 2, 4, 8 words.
template <int SIZE>
CD_FN uint32_t cd_word_mask(uint32_t bits, int d) {
  if (SIZE == 1) return cd_expand_bytes((bits >> (4 * d)) & 15u);
  if (SIZE == 2) return cd_expand_halves((bits >> (2 * d)) & 3u);
  return ((bits >> (d / (SIZE / 4 > 0 ? SIZE / 4 : 1))) & 1u) ? 0xFFFFFFFFu : 0u;
}

// ---- dbhip_case_check ---------------------------------------------------------------------------------------------------------------
// the plain fields of a dbhip_col that the check reads; no pointer
struct CdDesc {
  int32_t type, is_scalar, n_buffers;
  uint8_t precision, scale;
};
// bytes of one element; 0 for BOOL (a Bitmap), -1 for a type that does not exist
CD_FN int cd_elem_size(int32_t t) {
  switch (t) {
    case 1: return 0;
    case 2: case 6: return 1;
    case 3: case 7: return 2;
    case 4: case 8: case 10: case 12: return 4;
    case 5: case 9: case 11: case 13: case 14: return 8;
    case 15: case 16: return 16;
    case 17: return 32;
    default: return -1;
  }
}
enum {   // why a check failed: the caller turns it into a message
  CD_WHY_NONE = 0, CD_WHY_NULL_ARRAY, CD_WHY_NO_COND, CD_WHY_COUNT, CD_WHY_NO_ARG, CD_WHY_TOO_MANY, CD_WHY_COND_TYPE, CD_WHY_TYPE,
  CD_WHY_MIXED, CD_WHY_DEC_SIZE, CD_WHY_DESC
};
// conds == nullptr and n_conds == 0: a coalesce of n_values arguments; otherwise a CASE of n_conds conditions and n_conds + 1 values
CD_FN int cd_check(const CdDesc* conds, int32_t n_conds, const CdDesc* values, int32_t n_values, int* why) {
  const bool coalesce = conds == nullptr && n_conds == 0;
  *why = CD_WHY_NULL_ARRAY;
  if (!values) return CD_INVALID;
  if (!coalesce && !conds) return CD_INVALID;
  if (coalesce) {
    *why = CD_WHY_NO_ARG;
    if (n_values < 1) return CD_INVALID;
  } else {
    *why = CD_WHY_NO_COND;
    if (n_conds < 1) return CD_INVALID;
    *why = CD_WHY_COUNT;
    if (n_values != n_conds + 1) return CD_INVALID;
  }
  *why = CD_WHY_TOO_MANY;
  if (n_conds > CD_MAX_CONDS || n_values > CD_MAX_VALUES) return CD_UNSUPPORTED;
  for (int k = 0; k < n_conds; ++k) {
    *why = CD_WHY_COND_TYPE;
    if (conds[k].type != CD_T_BOOL) return CD_INVALID;
    *why = CD_WHY_DESC;
    if (conds[k].is_scalar != 0 && conds[k].is_scalar != 1) return CD_INVALID;
  }
  const int32_t t = values[0].type;
  *why = CD_WHY_TYPE;
  if (cd_elem_size(t) < 0) return CD_INVALID;
  const bool dec = t == CD_T_DEC64 || t == CD_T_DEC128 || t == CD_T_DEC256;
  int64_t tables = 0;
  for (int k = 0; k < n_values; ++k) {
    *why = CD_WHY_MIXED;
    if (values[k].type != t) return CD_INVALID;
    *why = CD_WHY_DEC_SIZE;
    if (dec && (values[k].precision != values[0].precision || values[k].scale != values[0].scale)) return CD_INVALID;
    *why = CD_WHY_DESC;
    if ((values[k].is_scalar != 0 && values[k].is_scalar != 1) || values[k].n_buffers < 0) return CD_INVALID;
    tables += t == CD_T_STRING ? values[k].n_buffers : 0;
  }
  *why = CD_WHY_DESC;
  if (tables > 0x7fffffff) return CD_INVALID;
  *why = CD_WHY_NONE;
  return CD_OK;
}

// ---- Strings ------------------------------------------------------------------------------------------------------------------------
// The result's buffer table is the arguments' tables back to back in argument order: base[k] is where argument k's starts, which is
// what sv_rebase (dev_strview.h) adds to the buffer index of a long view taken from argument k. Returns the length of the result's table.
CD_FN int32_t cd_table_bases(const int32_t* n_buffers, int n_values, uint32_t* base) {
  int32_t at = 0;
  for (int k = 0; k < n_values; ++k) { base[k] = (uint32_t)at; at += n_buffers[k]; }
  return at;
}
