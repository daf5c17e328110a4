// k_inlist.hip — constant IN-list membership -> filter Bitmap (include/dbhip.h a23). The row logic is dev_inlist.h.
//
// dbhip_inlist_create canonicalises the elements once on the host, removes duplicates and uploads ONE image the kernels stage in LDS:
//   BITS     I8 / U8 / I16 / U16: a direct bitmap of 256 or 65,536 bits. No comparison, no hash.
//   COMPARE  at most INL_COMPARE_MAX distinct elements: their keys travel in the parameter struct; the image is the long-byte block of a
//            String set (empty otherwise).
//   TABLE    up to 1024 elements: the open-addressing table, then the long-byte block. The dynamic LDS size is the image's own.
// One kernel shape for all three. A lane owns R consecutive rows (16 for the one- and two-byte types, otherwise 32 bytes' worth) and
// reads them with 16-byte loads; a column whose base is not 16-byte aligned (a slice), a scalar column and the last rows of a call are
// read element by element instead. Each lane packs its R member bits and R valid bits; for every 64 rows of the wave one __shfl brings
// each lane the bits of the lane that owns "its" row, one __ballot makes the word and one lane stores it. Equality needs equal length,
// so no lane compares more than 255 bytes of a String: there is no wave-per-row pass and no row list.
#include <string.h>

#include <new>
#include <vector>

#include "dev_common.h"
#include "dev_map.h"
#include "dev_strview.h"
#include "runtime.h"
#include "dev_inlist.h"

using namespace dbhip;

static_assert(INL_MAX_ITEMS == DBHIP_IN_MAX_ITEMS && INL_MAX_ITEM_BYTES == DBHIP_IN_MAX_ITEM_BYTES && INL_MAX_LONG_BYTES == DBHIP_IN_MAX_LONG_BYTES,
              "dev_inlist.h restates the public limits");
static_assert(INL_PATH_BITS == DBHIP_IN_PATH_BITS && INL_PATH_COMPARE == DBHIP_IN_PATH_COMPARE && INL_PATH_TABLE == DBHIP_IN_PATH_TABLE,
              "dev_inlist.h restates the public path codes");

struct dbhip_inlist {
  int32_t type, path, has_null, has_sentinel, wide;
  uint8_t precision, scale;
  uint32_t n_items;        // distinct, the sentinel not counted
  uint32_t slots;          // TABLE: the table's slot count, else 0
  uint32_t long_at;        // word offset of the long-byte block in the image
  uint32_t image_words;
  uint32_t* image_dev;     // owned (NULL when image_words == 0)
  uint64_t items[INL_COMPARE_MAX][2];
};

namespace {

constexpr int64_t IN_MAX_ROWS = 0xFFFFFFFELL;
enum { K_RAW = 0, K_F32 = 1, K_F64 = 2, K_D128 = 3, K_STR = 4 };

struct InParams {
  const void* data;
  const uint8_t* validity;
  int64_t voff;
  const void* const* buffers;
  uint64_t* out;
  uint64_t* out_valid;
  const uint32_t* image;
  int64_t n;
  uint32_t image_words, slots, long_at, n_items;
  int32_t n_buffers, negate, has_null, has_sentinel, is_scalar, vector_loads;
  uint64_t items[INL_COMPARE_MAX][2];
};

struct alignas(16) Wide16 { uint32_t x, y, z, w; };

template <typename T_, int R_, int KIND_, bool BITS_>
struct Shape {
  using T = T_;
  static constexpr int R = R_, KIND = KIND_;
  static constexpr bool BITS = BITS_;
};

template <class S>
__device__ __forceinline__ bool in_row_member(const typename S::T& x, const InParams& P, const uint32_t* lds) {
  if constexpr (S::BITS) {
    const uint32_t key = (uint32_t)x;
    return (lds[key >> 5] >> (key & 31)) & 1u;
  } else {
    constexpr bool wide = S::KIND == K_D128 || S::KIND == K_STR;
    InlValue v;
    if constexpr (S::KIND == K_RAW) v = inl_value((uint64_t)x, 0);
    else if constexpr (S::KIND == K_F32) v = inl_value(inl_canon_f32((uint32_t)x), 0);
    else if constexpr (S::KIND == K_F64) v = inl_value(inl_canon_f64((uint64_t)x), 0);
    else if constexpr (S::KIND == K_D128) v = inl_value(((uint64_t)x.y << 32) | x.x, ((uint64_t)x.w << 32) | x.z);
    else v = inl_string_value(x.x, x.y, x.z, x.w, P.buffers, P.n_buffers);
    return inl_member(v, wide, P.has_sentinel != 0, (const uint64_t*)lds, P.slots, P.items, P.n_items, lds + P.long_at);
  }
}

template <class S>
__global__ __launch_bounds__(256) void inlist_kernel(const InParams P) {
  extern __shared__ __attribute__((aligned(16))) uint32_t in_lds[];
  for (uint32_t t = threadIdx.x; t < P.image_words / 4; t += 256) ((uint4*)in_lds)[t] = ((const uint4*)P.image)[t];   // (whole 16-byte units: inl_set_finish)
  __syncthreads();
  using T = typename S::T;
  constexpr int R = S::R;
  const T* data = (const T*)P.data;
  const uint32_t lane = threadIdx.x & 63;
  constexpr int64_t WAVE_ROWS = 64 * R;
  // the loop's bounds are the same for all lanes of a wave: the shuffles and ballots below see whole waves
  for (int64_t w0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * WAVE_ROWS; w0 < P.n; w0 += (int64_t)gridDim.x * 4 * WAVE_ROWS) {
    const int64_t i0 = w0 + (int64_t)lane * R;
    T x[R];
    if (P.vector_loads && i0 + R <= P.n) {
      map_load<T, R>(data, std::true_type(), i0, x);
    } else {
#pragma unroll
      for (int k = 0; k < R; ++k) x[k] = i0 + k < P.n ? data[P.is_scalar ? 0 : i0 + k] : T{};
    }
    uint32_t member = 0, valid = 0;
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (i0 + k < P.n && (!P.validity || bit_get(P.validity, P.voff + (P.is_scalar ? 0 : i0 + k)))) {   // a NULL row is not looked at
        valid |= 1u << k;
        member |= (uint32_t)in_row_member<S>(x[k], P, in_lds) << k;
      }
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      if (w0 + 64 * j >= P.n) break;                       // wave-uniform
      const uint32_t row = 64u * j + lane, src = row / R, sh = row % R;
      const bool m = (__shfl(member, src, 64) >> sh) & 1u, v = (__shfl(valid, src, 64) >> sh) & 1u;
      const uint64_t word = __ballot(v && (P.negate ? (!m && !P.has_null) : m));
      if (lane == 0) P.out[(w0 >> 6) + j] = word;          // bits past n are 0: those rows are never valid
      if (P.out_valid) {
        const uint64_t vword = __ballot(v && (m || !P.has_null));
        if (lane == 0) P.out_valid[(w0 >> 6) + j] = vword;
      }
    }
  }
}

template <class S>
int32_t in_launch(const InParams& P, hipStream_t s) {
  const int grid = grid_for(ceil_div(P.n, S::R), 256, 1024);
  hipLaunchKernelGGL(inlist_kernel<S>, dim3(grid), dim3(256), (size_t)P.image_words * 4, s, P);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

bool in_type_ok(int32_t t) {
  switch (t) {
    case DBHIP_T_I8: case DBHIP_T_I16: case DBHIP_T_I32: case DBHIP_T_I64: case DBHIP_T_U8: case DBHIP_T_U16: case DBHIP_T_U32:
    case DBHIP_T_U64: case DBHIP_T_F32: case DBHIP_T_F64: case DBHIP_T_DATE: case DBHIP_T_TIMESTAMP: case DBHIP_T_DEC64:
    case DBHIP_T_DEC128: case DBHIP_T_STRING: return true;
    default: return false;
  }
}

}  // namespace

extern "C" {

int32_t dbhip_inlist_create(int32_t type, uint8_t precision, uint8_t scale, const void* values_host, const uint32_t* offsets_host,
                            int32_t n_items, int32_t has_null, dbhip_inlist** out_host) {
  DBHIP_REQUIRE(out_host, "dbhip_inlist_create: NULL out");
  *out_host = nullptr;
  DBHIP_REQUIRE(type >= DBHIP_T_BOOL && type <= DBHIP_T_DEC256, "dbhip_inlist_create: unknown type");
  DBHIP_REQUIRE(n_items >= 0, "dbhip_inlist_create: a negative element count");
  if (!in_type_ok(type)) { set_error("dbhip_inlist_create: Boolean and Decimal256 lists stay on the CPU"); return DBHIP_ERR_UNSUPPORTED; }
  const bool str = type == DBHIP_T_STRING;
  DBHIP_REQUIRE(n_items == 0 || (values_host && (!str || offsets_host)), "dbhip_inlist_create: NULL values or offsets");
  if (str)
    for (int32_t k = 0; k < n_items; ++k)
      DBHIP_REQUIRE(offsets_host[k] <= offsets_host[k + 1], "dbhip_inlist_create: descending offsets");
  if (n_items > INL_MAX_ITEMS) { set_error("dbhip_inlist_create: more than 1024 elements: plan the semi-join"); return DBHIP_ERR_UNSUPPORTED; }

  const int es = type_size(type);
  InlSet set;
  inl_set_init(set, es, type == DBHIP_T_F32 || type == DBHIP_T_F64, str);
  const uint8_t* vb = (const uint8_t*)values_host;
  for (int32_t k = 0; k < n_items; ++k) {
    if (!str) { inl_set_add_fixed(set, vb + (size_t)es * k); continue; }
    const int why = inl_set_add_string(set, vb + offsets_host[k], offsets_host[k + 1] - offsets_host[k]);
    if (why == INL_ADD_ITEM_TOO_LONG) { set_error("dbhip_inlist_create: an element of more than 255 bytes: plan the semi-join"); return DBHIP_ERR_UNSUPPORTED; }
    if (why) { set_error("dbhip_inlist_create: more than 16 KiB of long elements: plan the semi-join"); return DBHIP_ERR_UNSUPPORTED; }
  }
  inl_set_finish(set, false);

  dbhip_inlist* s = new (std::nothrow) dbhip_inlist();
  DBHIP_REQUIRE(s, "dbhip_inlist_create: out of host memory");
  memset(s, 0, sizeof(*s));
  s->type = type; s->precision = precision; s->scale = scale; s->has_null = has_null ? 1 : 0; s->has_sentinel = set.has_sentinel; s->wide = set.wide();
  s->n_items = (uint32_t)set.k0s.size();
  s->path = set.path;
  s->slots = set.slots;
  s->long_at = set.long_at;
  memcpy(s->items, set.items, sizeof(s->items));
  const std::vector<uint32_t>& image = set.image;
  s->image_words = (uint32_t)image.size();
  if (s->image_words) {
    int32_t rc = dbhip_alloc((size_t)s->image_words * 4, (void**)&s->image_dev);
    if (!rc && hipMemcpy(s->image_dev, image.data(), (size_t)s->image_words * 4, hipMemcpyHostToDevice) != hipSuccess) {
      set_error("dbhip_inlist_create: the copy of the set to the device failed");
      rc = DBHIP_ERR_HIP;
    }
    if (rc) {
      if (s->image_dev) (void)dbhip_free(s->image_dev);
      delete s;
      return rc;
    }
  }
  *out_host = s;
  return DBHIP_OK;
}

int32_t dbhip_inlist_path(const dbhip_inlist* s) { return s ? s->path : -DBHIP_ERR_INVALID; }

int32_t dbhip_inlist_eval(const dbhip_inlist* s, const dbhip_col* col, int32_t flags, int64_t n, uint8_t* out_bitmap, uint8_t* out_validity,
                          void* stream) {
  DBHIP_REQUIRE(s && col, "dbhip_inlist_eval: NULL set or column");
  DBHIP_REQUIRE(!(flags & ~DBHIP_IN_NEGATE), "dbhip_inlist_eval: unknown flag bits");
  DBHIP_REQUIRE(n >= 0 && n <= IN_MAX_ROWS, "dbhip_inlist_eval: row count outside 0 .. 2^32 - 2");
  DBHIP_REQUIRE(col->type == s->type, "dbhip_inlist_eval: the column's type is not the set's");
  if (s->type == DBHIP_T_DEC64 || s->type == DBHIP_T_DEC128)
    DBHIP_REQUIRE(col->precision == s->precision && col->scale == s->scale, "dbhip_inlist_eval: the column's precision and scale are not the set's");
  if (n == 0) return DBHIP_OK;
  const int es = type_size(s->type);
  DBHIP_REQUIRE(col->data && out_bitmap && !((uintptr_t)out_bitmap & 7) && !((uintptr_t)out_validity & 7),
                "dbhip_inlist_eval: NULL data or bitmap, or a bitmap that is not 8-byte aligned");
  DBHIP_REQUIRE(!((uintptr_t)col->data & (uintptr_t)(es - 1)), "dbhip_inlist_eval: column data not element-aligned (String views: 16 bytes)");
  InParams P;
  memset(&P, 0, sizeof(P));
  P.data = col->data;
  P.validity = col->validity;
  P.voff = col->validity_offset;
  P.buffers = col->buffers;
  P.n_buffers = col->buffers && col->n_buffers > 0 ? col->n_buffers : 0;
  P.out = (uint64_t*)out_bitmap;
  P.out_valid = (uint64_t*)out_validity;
  P.image = s->image_dev;
  P.n = n;
  P.image_words = s->image_words;
  P.slots = s->slots;
  P.long_at = s->long_at;
  P.n_items = s->path == DBHIP_IN_PATH_COMPARE ? s->n_items : 0;
  P.negate = (flags & DBHIP_IN_NEGATE) ? 1 : 0;
  P.has_null = s->has_null;
  P.has_sentinel = s->has_sentinel;
  P.is_scalar = col->is_scalar ? 1 : 0;
  P.vector_loads = !col->is_scalar && !((uintptr_t)col->data & 15);
  memcpy(P.items, s->items, sizeof(P.items));
  hipStream_t st = resolve_stream(stream);
  switch (s->type) {
    case DBHIP_T_I8: case DBHIP_T_U8: return in_launch<Shape<uint8_t, 16, K_RAW, true>>(P, st);
    case DBHIP_T_I16: case DBHIP_T_U16: return in_launch<Shape<uint16_t, 16, K_RAW, true>>(P, st);
    case DBHIP_T_I32: case DBHIP_T_U32: case DBHIP_T_DATE: return in_launch<Shape<uint32_t, 8, K_RAW, false>>(P, st);
    case DBHIP_T_F32: return in_launch<Shape<uint32_t, 8, K_F32, false>>(P, st);
    case DBHIP_T_I64: case DBHIP_T_U64: case DBHIP_T_TIMESTAMP: case DBHIP_T_DEC64: return in_launch<Shape<uint64_t, 4, K_RAW, false>>(P, st);
    case DBHIP_T_F64: return in_launch<Shape<uint64_t, 4, K_F64, false>>(P, st);
    case DBHIP_T_DEC128: return in_launch<Shape<Wide16, 2, K_D128, false>>(P, st);
    default: return in_launch<Shape<Wide16, 2, K_STR, false>>(P, st);
  }
}

int32_t dbhip_inlist_destroy(dbhip_inlist* s) {
  if (!s) return DBHIP_OK;
  if (s->image_dev) {   // (a set without an image never reached the device)
    (void)hipDeviceSynchronize();
    (void)dbhip_free(s->image_dev);
  }
  delete s;
  return DBHIP_OK;
}

}  // extern "C"
