// k_cond.hip — conditionals (include/dbhip.h a27): dbhip_case / dbhip_coalesce, a type-agnostic select over up to 17 branch columns,
// and dbhip_bool_logic, Kleene AND / OR / NOT / XOR over nullable Booleans.
//
// The logic is dev_cond.h's (one text for these kernels and the host checker); this file is the memory side. Which branch a row takes is
// decided on 64-row Bitmap words (dev_cond.h), never row by row, and the elements are moved as raw 32-bit words: nothing here knows
// what a type means, only that an element is 1, 2, 4, 8, 16 or 32 bytes.
//
// cond_select_kernel<SIZE> (every type but BOOL): a wave owns 64 * R consecutive rows per step, R = 16 / SIZE rows per lane (1 for 16-
// and 32-byte elements), so every lane moves 16 bytes per branch column (32 for a Decimal256) and a wave's step covers R WHOLE words of
// each output Bitmap. For each branch in order a lane fetches the Bitmap word of its rows (the 64 / R lanes that share a word ask for
// the same address: one load instruction per Bitmap per step, no lane fetches a bit of its own), the chooser gives the rows of the
// word that take the branch, and the lane shifts its R bits out of it. Only if some lane of the wave took a non-NULL value of the
// branch (a ballot) is the branch column read at all, and then only by the lanes that took one: a branch nobody chose costs its
// Bitmap words and nothing else. The chosen elements are merged by mask into the lane's output words, which start as zero, so a NULL
// row holds zero without a second pass. The validity word of 64 rows is computed whole, from words, by every lane that owns rows of it;
// the lane that owns its first row stores it. No word is written by two lanes, nothing is atomic, and nothing needs a ballot to be
// assembled. out_branch is merged the same way, one byte per row.
// Sliced columns: a wave-uniform test of each base picks 16-byte or per-element accesses (as dev_map.h); the rows of the last, partial
// run go per element. A scalar is read where a lane took it, one address for the wave.
// cond_bits_kernel (BOOL values) and bool_logic_kernel are word-wise: a lane owns one 64-row word of the outputs and builds it from
// input words fetched at their bit offsets. No LDS, no scratch memory, no atomics anywhere.
#include <string.h>

#include "runtime.h"

#include "dev_cond.h"
#include "dev_strview.h"

using namespace dbhip;

static_assert(CD_AND == DBHIP_BOOL_AND && CD_OR == DBHIP_BOOL_OR && CD_NOT == DBHIP_BOOL_NOT && CD_XOR == DBHIP_BOOL_XOR, "dev_cond.h operator codes");
static_assert(CD_MAX_CONDS == DBHIP_CASE_MAX_CONDS, "dev_cond.h limit");
static_assert(CD_T_BOOL == DBHIP_T_BOOL && CD_T_DEC64 == DBHIP_T_DEC64 && CD_T_DEC128 == DBHIP_T_DEC128 && CD_T_STRING == DBHIP_T_STRING &&
              CD_T_DEC256 == DBHIP_T_DEC256, "dev_cond.h type codes");
static_assert(CD_OK == DBHIP_OK && CD_INVALID == DBHIP_ERR_INVALID && CD_UNSUPPORTED == DBHIP_ERR_UNSUPPORTED, "dev_cond.h status codes");

namespace {

struct CondCol {
  const void* data;
  const uint8_t* validity;
  int64_t voff;
  uint32_t is_scalar, table_base;   // table_base: where this argument's buffer table starts in the result's (Strings)
};
struct CondArgs {   // travels by value in the kernel arguments: 33 * 32 + 48 bytes
  CondCol conds[CD_MAX_CONDS];
  CondCol vals[CD_MAX_VALUES];
  void* out;
  uint64_t* out_validity;
  uint8_t* out_branch;
  int64_t n;
  int32_t n_conds, n_vals, is_string, _pad;
};
static_assert(sizeof(CondArgs) <= 2048, "the argument struct stays far below the 4 KiB limit");

struct alignas(16) Quad { uint32_t w[4]; };

// the validity word of the rows from row0 on; a scalar's one bit for every row
__device__ __forceinline__ uint64_t validity_word(const CondCol& c, int64_t row0, int count) {
  if (!c.validity) return ~0ull;
  if (c.is_scalar) return cd_splat(cd_fetch64(c.validity, c.voff, 1) != 0);
  return cd_fetch64(c.validity, c.voff + row0, count);
}
// the value word of a Boolean column (a Bitmap at bit 0). `vv` is its validity word: a scalar that is NULL is not dereferenced
__device__ __forceinline__ uint64_t bool_word(const CondCol& c, uint64_t vv, int64_t row0, int count) {
  if (c.is_scalar) return vv ? cd_splat(cd_fetch64((const uint8_t*)c.data, 0, 1) != 0) : 0ull;
  return cd_fetch64((const uint8_t*)c.data, row0, count);
}
// the rows of the word where branch k is TRUE, and the rows where its value is valid
__device__ __forceinline__ void branch_words(const CondArgs& A, int k, int64_t row0, int count, uint64_t& t, uint64_t& vv) {
  vv = validity_word(A.vals[k], row0, count);
  if (A.n_conds == 0) { t = vv; return; }                      // coalesce: the first valid argument
  if (k == A.n_conds) { t = ~0ull; return; }                   // ELSE
  const uint64_t cv = validity_word(A.conds[k], row0, count);
  t = cd_true_rows(bool_word(A.conds[k], cv, row0, count), cv);
}

// R consecutive elements of SIZE bytes as raw words. `lr` of them exist. 16-byte accesses when the base is 16-byte aligned and the run
// is whole (first * SIZE is a multiple of 16 by the choice of R), else one access per element (a 16- or 32-byte one in 8-byte pieces)
template <int SIZE, int R, int W>
__device__ __forceinline__ void load_run(const CondCol& c, int64_t first, int lr, uint32_t (&v)[W]) {
#pragma unroll
  for (int d = 0; d < W; ++d) v[d] = 0;
  const bool vec = (((uintptr_t)c.data) & 15) == 0;             // from the kernel arguments: wave-uniform
  if (!c.is_scalar && vec && lr == R) {
    const Quad* p = (const Quad*)((const char*)c.data + first * SIZE);
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      const Quad t = p[q];
#pragma unroll
      for (int d = 0; d < 4; ++d) v[4 * q + d] = t.w[d];
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r >= lr) continue;
    const int64_t i = c.is_scalar ? 0 : first + r;
    if constexpr (SIZE == 1) v[r >> 2] |= (uint32_t)((const uint8_t*)c.data)[i] << (8 * (r & 3));
    else if constexpr (SIZE == 2) v[r >> 1] |= (uint32_t)((const uint16_t*)c.data)[i] << (16 * (r & 1));
    else if constexpr (SIZE == 4) v[r] = ((const uint32_t*)c.data)[i];
    else {
      const uint64_t* p = (const uint64_t*)c.data + i * (SIZE / 8);
#pragma unroll
      for (int h = 0; h < SIZE / 8; ++h) {
        const uint64_t x = p[h];
        v[r * (SIZE / 4) + 2 * h] = (uint32_t)x;
        v[r * (SIZE / 4) + 2 * h + 1] = (uint32_t)(x >> 32);
      }
    }
  }
}
template <int SIZE, int R, int W>
__device__ __forceinline__ void store_run(void* out, bool vec, int64_t first, int lr, const uint32_t (&v)[W]) {
  if (vec && lr == R) {
    Quad* p = (Quad*)((char*)out + first * SIZE);
#pragma unroll
    for (int q = 0; q < W / 4; ++q) {
      Quad t;
#pragma unroll
      for (int d = 0; d < 4; ++d) t.w[d] = v[4 * q + d];
      p[q] = t;
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r >= lr) continue;
    const int64_t i = first + r;
    if constexpr (SIZE == 1) ((uint8_t*)out)[i] = (uint8_t)(v[r >> 2] >> (8 * (r & 3)));
    else if constexpr (SIZE == 2) ((uint16_t*)out)[i] = (uint16_t)(v[r >> 1] >> (16 * (r & 1)));
    else if constexpr (SIZE == 4) ((uint32_t*)out)[i] = v[r];
    else {
      uint64_t* p = (uint64_t*)out + i * (SIZE / 8);
#pragma unroll
      for (int h = 0; h < SIZE / 8; ++h) p[h] = ((uint64_t)v[r * (SIZE / 4) + 2 * h + 1] << 32) | v[r * (SIZE / 4) + 2 * h];
    }
  }
}

template <int SIZE>
__global__ __launch_bounds__(256) void cond_select_kernel(const CondArgs A) {
  constexpr int R = SIZE >= 16 ? 1 : 16 / SIZE;        // rows per lane
  constexpr int W = R * SIZE / 4;                      // 32-bit words per lane: 4, or 8 for a Decimal256
  constexpr uint32_t RMASK = (1u << R) - 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256 + threadIdx.x) >> 6));
  const int64_t waves = (int64_t)gridDim.x * 4;
  const int64_t steps = (A.n + 64 * R - 1) / (64 * R);
  const bool out_vec = (((uintptr_t)A.out) & 15) == 0;
  const bool br_vec = (((uintptr_t)A.out_branch) & (R - 1)) == 0;
  const int nb = A.n_vals;
  for (int64_t c = wave; c < steps; c += waves) {
    const int64_t first = (c * 64 + lane) * R;         // this lane's first row
    const int64_t row0 = first & ~63ll;                // the first row of the Bitmap word its rows lie in
    const int sh = (int)(first & 63);
    const int64_t left = A.n - first;
    const int lr = left >= R ? R : (left > 0 ? (int)left : 0);
    const int64_t wleft = A.n - row0;
    const int count = wleft >= 64 ? 64 : (int)wleft;   // <= 0: the whole word lies past n, and so do this lane's rows
    CdChooser ch = cd_chooser(cd_live(row0, A.n));
    uint32_t o[W], br[4] = {0, 0, 0, 0};
#pragma unroll
    for (int d = 0; d < W; ++d) o[d] = 0;
    uint64_t validw = 0;
    for (int k = 0; k < nb; ++k) {
      uint64_t t = 0, vv = 0;
      if (count > 0) branch_words(A, k, row0, count, t, vv);
      const uint64_t m = cd_take(ch, t);
      const uint64_t mv = m & vv;
      validw |= mv;
      const uint32_t mine = (uint32_t)(m >> sh) & RMASK;        // my rows that take branch k
      const uint32_t minev = (uint32_t)(mv >> sh) & RMASK;      // ... and get a value from it
      if (A.out_branch) {
#pragma unroll
        for (int d = 0; d < (R + 3) / 4; ++d) br[d] |= cd_expand_bytes((mine >> (4 * d)) & 15u) & ((uint32_t)k * 0x01010101u);
      }
      if (__ballot(minev != 0) != 0) {                          // a column no lane of the wave chose is not read
        if (minev != 0) {
          uint32_t v[W];
          load_run<SIZE, R, W>(A.vals[k], first, lr, v);
          if (SIZE == 16 && A.is_string) sv_rebase(v[0], v[2], v[3], A.vals[k].table_base, 0);
#pragma unroll
          for (int d = 0; d < W; ++d) o[d] |= v[d] & cd_word_mask<SIZE>(minev, d);
        }
      }
    }
    if (lr > 0) store_run<SIZE, R, W>(A.out, out_vec, first, lr, o);
    if (A.out_validity && sh == 0 && count > 0) A.out_validity[row0 >> 6] = validw;
    if (A.out_branch && lr > 0) {
      const uint32_t rest = (uint32_t)(cd_rest(ch) >> sh) & RMASK;   // the NULL rows of a coalesce
#pragma unroll
      for (int d = 0; d < (R + 3) / 4; ++d) br[d] |= cd_expand_bytes((rest >> (4 * d)) & 15u) & ((uint32_t)nb * 0x01010101u);
      uint8_t* p = A.out_branch + first;
      if (br_vec && lr == R) {
        if constexpr (R == 16) { Quad q; q.w[0] = br[0]; q.w[1] = br[1]; q.w[2] = br[2]; q.w[3] = br[3]; *(Quad*)p = q; }
        else if constexpr (R == 8) *(uint64_t*)p = ((uint64_t)br[1] << 32) | br[0];
        else if constexpr (R == 4) *(uint32_t*)p = br[0];
        else if constexpr (R == 2) *(uint16_t*)p = (uint16_t)br[0];
        else *p = (uint8_t)br[0];
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r < lr) p[r] = (uint8_t)(br[r >> 2] >> (8 * (r & 3)));
        }
      }
    }
  }
}

// BOOL values: the result is a Bitmap, so a lane builds one whole 64-row word of it from the branches' words
__global__ __launch_bounds__(256) void cond_bits_kernel(const CondArgs A) {
  const int64_t words = (A.n + 63) >> 6;
  const int nb = A.n_vals;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256) {
    const int64_t row0 = w << 6;
    const int64_t wleft = A.n - row0;
    const int count = wleft >= 64 ? 64 : (int)wleft;
    CdChooser ch = cd_chooser(cd_live(row0, A.n));
    uint64_t validw = 0, bits = 0;
    for (int k = 0; k < nb; ++k) {
      uint64_t t, vv;
      branch_words(A, k, row0, count, t, vv);
      const uint64_t m = cd_take(ch, t);
      const uint64_t mv = m & vv;
      validw |= mv;
      if (mv) bits |= mv & bool_word(A.vals[k], mv, row0, count);
      if (A.out_branch) {
        for (uint64_t x = m; x; x &= x - 1) A.out_branch[row0 + __builtin_ctzll(x)] = (uint8_t)k;
      }
    }
    if (A.out_branch) {
      for (uint64_t x = cd_rest(ch); x; x &= x - 1) A.out_branch[row0 + __builtin_ctzll(x)] = (uint8_t)nb;
    }
    ((uint64_t*)A.out)[w] = bits;
    if (A.out_validity) A.out_validity[w] = validw;
  }
}

struct LogicArgs {
  CondCol a, b;
  uint64_t* out_values;
  uint64_t* out_validity;
  int64_t n;
  int32_t op, _pad;
};
__global__ __launch_bounds__(256) void bool_logic_kernel(const LogicArgs A) {
  const int64_t words = (A.n + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256) {
    const int64_t row0 = w << 6;
    const int64_t wleft = A.n - row0;
    const int count = wleft >= 64 ? 64 : (int)wleft;
    const uint64_t live = cd_live(row0, A.n);
    const uint64_t va = validity_word(A.a, row0, count);
    const uint64_t a = bool_word(A.a, va, row0, count);
    uint64_t vb = ~0ull, b = 0;
    if (A.op != CD_NOT) {
      vb = validity_word(A.b, row0, count);
      b = bool_word(A.b, vb, row0, count);
    }
    uint64_t t, v;
    cd_kleene(A.op, a, va, b, vb, t, v);
    A.out_values[w] = t & live;
    if (A.out_validity) A.out_validity[w] = v & live;
  }
}

CdDesc desc_of(const dbhip_col& c) {
  CdDesc d;
  d.type = c.type; d.is_scalar = c.is_scalar; d.n_buffers = c.n_buffers; d.precision = c.precision; d.scale = c.scale;
  return d;
}

// dbhip_case_check for the call `who`
int32_t check_call(const char* who, const dbhip_col* conds, int32_t n_conds, const dbhip_col* values, int32_t n_values) {
  CdDesc dc[CD_MAX_CONDS], dv[CD_MAX_VALUES];
  // the counts are judged before anything is copied: the descriptors of a call beyond the limits are never read
  const bool fits = n_conds >= 0 && n_conds <= CD_MAX_CONDS && n_values >= 0 && n_values <= CD_MAX_VALUES;
  if (fits) {
    for (int k = 0; conds && k < n_conds; ++k) dc[k] = desc_of(conds[k]);
    for (int k = 0; values && k < n_values; ++k) dv[k] = desc_of(values[k]);
  }
  int why = CD_WHY_NONE;
  const int rc = cd_check(conds ? dc : nullptr, n_conds, values ? dv : nullptr, n_values, &why);
  switch (why) {
    case CD_WHY_NONE: break;
    case CD_WHY_NULL_ARRAY: set_error("%s: NULL array of conditions or values", who); break;
    case CD_WHY_NO_COND: set_error("%s: a CASE needs at least one condition", who); break;
    case CD_WHY_COUNT: set_error("%s: %d conditions need %d values (the last is ELSE), not %d", who, n_conds, n_conds + 1, n_values); break;
    case CD_WHY_NO_ARG: set_error("%s: a coalesce needs at least one argument", who); break;
    case CD_WHY_TOO_MANY: set_error("%s: more than %d conditions or %d arguments: nest the call or keep the CPU closure", who, CD_MAX_CONDS, CD_MAX_VALUES); break;
    case CD_WHY_COND_TYPE: set_error("%s: a condition must be a Boolean column or scalar", who); break;
    case CD_WHY_TYPE: set_error("%s: values of unknown type %d", who, values[0].type); break;
    case CD_WHY_MIXED: set_error("%s: the values must all have one type (the planner casts)", who); break;
    case CD_WHY_DEC_SIZE: set_error("%s: decimal values must share one precision and one scale (the planner casts)", who); break;
    default: set_error("%s: is_scalar must be 0 or 1 and n_buffers must not be negative", who); break;
  }
  return rc;
}

bool fill_col(CondCol& d, const dbhip_col& c, uintptr_t align_mask) {
  d.data = c.data; d.validity = c.validity; d.voff = c.validity_offset; d.is_scalar = c.is_scalar ? 1u : 0u; d.table_base = 0;
  if (c.validity_offset < 0) return false;
  if (!c.data && !(c.is_scalar && c.validity)) return false;     // only a scalar that can be NULL may come without data
  return (((uintptr_t)c.data) & align_mask) == 0;
}

int32_t run_select(const char* who, const dbhip_col* conds, int32_t n_conds, const dbhip_col* values, int32_t n_values, int64_t n, void* out,
                   uint8_t* out_validity, uint8_t* out_branch, const void** out_buffers_dev, int32_t* out_n_buffers_host, void* stream) {
  const int32_t rc = check_call(who, conds, n_conds, values, n_values);
  if (rc) return rc;
  if (n < 0) { set_error("%s: negative n", who); return DBHIP_ERR_INVALID; }
  const int32_t t = values[0].type;
  const int size = cd_elem_size(t);
  int32_t nb[CD_MAX_VALUES];
  uint32_t base[CD_MAX_VALUES];
  for (int k = 0; k < n_values; ++k) nb[k] = t == DBHIP_T_STRING ? values[k].n_buffers : 0;
  const int32_t tables = cd_table_bases(nb, n_values, base);
  if (out_n_buffers_host) *out_n_buffers_host = tables;
  if (n == 0) return DBHIP_OK;
  // element alignment (a Decimal128 / 256 to 8 bytes, a view to 16, a Bitmap to 8 as an output and to nothing as an input)
  const uintptr_t in_mask = t == DBHIP_T_STRING ? 15 : (size >= 16 ? 7 : (size ? size - 1 : 0));
  const uintptr_t out_mask = size == 0 ? 7 : in_mask;
  bool ok = out && (((uintptr_t)out) & out_mask) == 0 && (((uintptr_t)out_validity) & 7) == 0;
  CondArgs A;
  memset(&A, 0, sizeof(A));
  for (int k = 0; k < n_conds; ++k) ok = fill_col(A.conds[k], conds[k], 0) && ok;
  for (int k = 0; k < n_values; ++k) {
    ok = fill_col(A.vals[k], values[k], in_mask) && ok;
    A.vals[k].table_base = base[k];
    if (nb[k] > 0 && !values[k].buffers) ok = false;
  }
  if (tables > 0 && !out_buffers_dev) ok = false;
  if (!ok) {
    set_error("%s: NULL or misaligned data / out (elements to their size, Decimal128 / 256 to 8 bytes, views to 16, output Bitmaps to 8), "
              "a negative validity_offset, or String arguments with buffers and no out_buffers_dev", who);
    return DBHIP_ERR_INVALID;
  }
  A.out = out; A.out_validity = (uint64_t*)out_validity; A.out_branch = out_branch; A.n = n;
  A.n_conds = n_conds; A.n_vals = n_values; A.is_string = t == DBHIP_T_STRING;
  hipStream_t s = resolve_stream(stream);
  for (int k = 0; k < n_values; ++k) {   // the result's buffer table: the arguments' tables back to back
    if (nb[k] > 0) DBHIP_CHECK(hipMemcpyAsync((void*)(out_buffers_dev + base[k]), values[k].buffers, (size_t)nb[k] * sizeof(void*), hipMemcpyDeviceToDevice, s));
  }
  const int64_t rows_per_lane = size == 0 ? 64 : (size >= 16 ? 1 : 16 / size);
  const int64_t lanes = size == 0 ? ceil_div(n, 64) : ceil_div(n, 64 * rows_per_lane) * 64;
  const dim3 grid(grid_for(lanes, 256)), block(256);
  switch (size) {
    case 0: hipLaunchKernelGGL(cond_bits_kernel, grid, block, 0, s, A); break;
    case 1: hipLaunchKernelGGL(cond_select_kernel<1>, grid, block, 0, s, A); break;
    case 2: hipLaunchKernelGGL(cond_select_kernel<2>, grid, block, 0, s, A); break;
    case 4: hipLaunchKernelGGL(cond_select_kernel<4>, grid, block, 0, s, A); break;
    case 8: hipLaunchKernelGGL(cond_select_kernel<8>, grid, block, 0, s, A); break;
    case 16: hipLaunchKernelGGL(cond_select_kernel<16>, grid, block, 0, s, A); break;
    default: hipLaunchKernelGGL(cond_select_kernel<32>, grid, block, 0, s, A); break;
  }
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

}  // namespace

extern "C" {

int32_t dbhip_case_check(const dbhip_col* conds_host, int32_t n_conds, const dbhip_col* values_host, int32_t n_values) {
  return check_call("dbhip_case_check", conds_host, n_conds, values_host, n_values);
}

int32_t dbhip_case(const dbhip_col* conds_host, int32_t n_conds, const dbhip_col* values_host, int64_t n, void* out, uint8_t* out_validity,
                   uint8_t* out_branch, const void** out_buffers_dev, int32_t* out_n_buffers_host, void* stream) {
  DBHIP_REQUIRE(conds_host && n_conds >= 1, "dbhip_case: NULL conditions or no condition (a coalesce is dbhip_coalesce)");
  return run_select("dbhip_case", conds_host, n_conds, values_host, n_conds < INT32_MAX ? n_conds + 1 : n_conds, n, out, out_validity, out_branch, out_buffers_dev, out_n_buffers_host, stream);
}

int32_t dbhip_coalesce(const dbhip_col* args_host, int32_t n_args, int64_t n, void* out, uint8_t* out_validity, uint8_t* out_branch,
                       const void** out_buffers_dev, int32_t* out_n_buffers_host, void* stream) {
  return run_select("dbhip_coalesce", nullptr, 0, args_host, n_args, n, out, out_validity, out_branch, out_buffers_dev, out_n_buffers_host, stream);
}

int32_t dbhip_bool_logic(int32_t op, const dbhip_col* a, const dbhip_col* b, int64_t n, uint8_t* out_values, uint8_t* out_validity, void* stream) {
  DBHIP_REQUIRE(op >= 0 && op < CD_OP_COUNT, "dbhip_bool_logic: unknown operator");
  DBHIP_REQUIRE(a && (b || op == CD_NOT) && n >= 0, "dbhip_bool_logic: NULL operand or negative n");
  DBHIP_REQUIRE(a->type == DBHIP_T_BOOL && (op == CD_NOT || b->type == DBHIP_T_BOOL), "dbhip_bool_logic: the operands must be Boolean columns or scalars");
  if (n == 0) return DBHIP_OK;
  LogicArgs A;
  memset(&A, 0, sizeof(A));
  bool ok = out_values && (((uintptr_t)out_values) & 7) == 0 && (((uintptr_t)out_validity) & 7) == 0;
  ok = fill_col(A.a, *a, 0) && ok;
  if (op != CD_NOT) ok = fill_col(A.b, *b, 0) && ok;
  DBHIP_REQUIRE(ok, "dbhip_bool_logic: NULL data or out_values, a negative validity_offset, or an output Bitmap that is not 8-byte aligned");
  A.out_values = (uint64_t*)out_values; A.out_validity = (uint64_t*)out_validity; A.n = n; A.op = op;
  hipStream_t s = resolve_stream(stream);
  hipLaunchKernelGGL(bool_logic_kernel, dim3(grid_for(ceil_div(n, 64), 256)), dim3(256), 0, s, A);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

}  // extern "C"
