// k_regex.hip — constant regular-expression predicates over String columns -> filter Bitmap (include/dbhip.h a25).
//
// dbhip_regex_create compiles the pattern once on the host (regex_compile.h: parser -> Thompson NFA -> subset construction over byte
// classes) and uploads ONE image: the uint16 transition table [state][class], the state flags, the 256-byte class map. Every workgroup
// stages the image in dynamic LDS sized to the handle (at most 32 KiB + 4 KiB + 256 B); the row walk is dev_regex.h.
//   one launch   256-thread workgroups, one lane per row, grid-stride. Values of <= 12 bytes are walked from the view's registers,
//                longer ones with naturally aligned 4-byte loads that each cover at least one byte of the value. The 64 result bits of a
//                wave come from one __ballot and one lane's store; a second ballot gives the declined word, and a wave whose declined
//                word is not zero adds its population count to the caller's counter with one atomic.
//   long values  are walked by their lane; the wave waits. There is no wave-per-row pass and no row list.
//   scalar       one lane decides the one value into 16 bytes of scratch and a fill kernel expands it to n rows.
#include <string.h>

#include <new>

#include "dev_common.h"
#include "dev_strview.h"
#include "runtime.h"
#define REGEX_FN __device__ __forceinline__
#include "dev_regex.h"
#include "regex_compile.h"

using namespace dbhip;

static_assert(RX_MAX_PATTERN == DBHIP_REGEX_MAX_PATTERN && RX_MAX_STATES == DBHIP_REGEX_MAX_STATES && RX_MAX_TABLE_BYTES == DBHIP_REGEX_MAX_TABLE_BYTES,
              "regex_compile.h restates the public limits");
static_assert(RX_F_CASE_INSENSITIVE == DBHIP_REGEX_CASE_INSENSITIVE && RX_F_DOT_NL == DBHIP_REGEX_DOT_NL && RX_F_UNIT_BYTE == DBHIP_REGEX_UNIT_BYTE &&
                  RX_F_FULL_MATCH == DBHIP_REGEX_FULL_MATCH,
              "regex_compile.h restates the create flags");
static_assert(RX_ACCEPT_END == REGEX_ACCEPT_END && RX_STICKY == REGEX_STICKY && RX_DEAD == REGEX_DEAD, "dev_regex.h restates the state flags");

struct dbhip_regex {
  uint32_t n_states, n_classes, table_bytes, needs_ascii;
  uint32_t flags_at, cmap_at, image_bytes;   // byte offsets inside the image; all three are multiples of 16
  uint8_t* image_dev;                        // owned
};

namespace {

constexpr int REGEX_SCRATCH_SLOT = 26;
constexpr int64_t REGEX_MAX_ROWS = 0xFFFFFFFELL;

struct RegexParams {
  const uint4* views;
  const uint8_t* validity;
  int64_t voff;
  const void* const* buffers;
  uint64_t* out;
  uint64_t* out_declined;
  unsigned long long* declined_count;
  const uint8_t* image;
  int64_t n;
  uint32_t image_bytes, flags_at, cmap_at, n_classes;
  int32_t n_buffers, negate, needs_ascii, _pad;
};

__global__ __launch_bounds__(256) void regex_rows_kernel(const RegexParams P) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rx_lds[];
  for (uint32_t t = threadIdx.x; t < P.image_bytes / 16; t += 256) ((uint4*)rx_lds)[t] = ((const uint4*)P.image)[t];
  __syncthreads();
  const RegexTables R{(const uint16_t*)rx_lds, rx_lds + P.flags_at, rx_lds + P.cmap_at, P.n_classes, (uint32_t)P.needs_ascii};
  const uint32_t lane = threadIdx.x & 63;
  // every lane of a wave runs the same number of rounds (the wave's first row decides), so the ballots see whole waves
  for (int64_t wave0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); wave0 < P.n; wave0 += (int64_t)gridDim.x * 256) {
    const int64_t i = wave0 + lane;
    bool bit = false, declined = false;
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
        const uint32_t r = regex_walk(v, R);
        declined = r == REGEX_DECLINED;
        bit = !declined && ((r == REGEX_YES) != (P.negate != 0));
      }
    }
    const uint64_t word = __ballot(bit);
    const uint64_t dword = __ballot(declined);
    if (lane == 0) {
      P.out[wave0 >> 6] = word;                   // bits past n are 0: those lanes never set `bit`
      if (P.out_declined) P.out_declined[wave0 >> 6] = dword;
      if (dword && P.declined_count) atomicAdd(P.declined_count, (unsigned long long)__popcll(dword));
    }
  }
}

// a scalar column: the one decided bit, and the one declined bit, to all n rows
__global__ __launch_bounds__(256) void regex_fill_kernel(const uint64_t* one, uint64_t* out, uint64_t* out_declined, unsigned long long* declined_count, int64_t n) {
  const uint64_t all = (one[0] & 1ull) ? ~0ull : 0ull, dall = (one[1] & 1ull) ? ~0ull : 0ull;
  const int64_t words = (n + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (int64_t)gridDim.x * 256) {
    const int64_t left = n - w * 64;
    const uint64_t m = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    out[w] = all & m;
    if (out_declined) out_declined[w] = dall & m;
  }
  if (dall && declined_count && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(declined_count, (unsigned long long)n);
}

int32_t regex_status(int rc) { return rc == RX_OK ? DBHIP_OK : (rc == RX_INVALID ? DBHIP_ERR_INVALID : DBHIP_ERR_UNSUPPORTED); }

}  // namespace

extern "C" {

int32_t dbhip_regex_check(const uint8_t* pattern_host, int32_t pattern_len, int32_t flags, int32_t* out_info_host) {
  RxProgram prog;
  const char* why = "";
  const int rc = rx_compile(pattern_host, pattern_len, flags, &prog, &why);
  if (rc) { set_error("dbhip_regex_check: %s%s", why, rc == RX_UNSUPPORTED ? ": keep the CPU closure" : ""); return regex_status(rc); }
  if (out_info_host) {
    out_info_host[0] = (int32_t)prog.flags.size();
    out_info_host[1] = (int32_t)prog.n_classes;
    out_info_host[2] = (int32_t)(prog.table.size() * 2);
    out_info_host[3] = prog.needs_ascii ? 1 : 0;
  }
  return DBHIP_OK;
}

int32_t dbhip_regex_create(const uint8_t* pattern_host, int32_t pattern_len, int32_t flags, dbhip_regex** out_host) {
  DBHIP_REQUIRE(out_host, "dbhip_regex_create: NULL out");
  *out_host = nullptr;
  RxProgram prog;
  const char* why = "";
  const int rc = rx_compile(pattern_host, pattern_len, flags, &prog, &why);
  if (rc) { set_error("dbhip_regex_create: %s%s", why, rc == RX_UNSUPPORTED ? ": keep the CPU closure" : ""); return regex_status(rc); }

  dbhip_regex* r = new (std::nothrow) dbhip_regex();
  DBHIP_REQUIRE(r, "dbhip_regex_create: out of host memory");
  memset(r, 0, sizeof(*r));
  r->n_states = (uint32_t)prog.flags.size();
  r->n_classes = prog.n_classes;
  r->table_bytes = (uint32_t)prog.table.size() * 2;
  r->needs_ascii = prog.needs_ascii ? 1 : 0;
  r->flags_at = (r->table_bytes + 15u) & ~15u;
  r->cmap_at = r->flags_at + ((r->n_states + 15u) & ~15u);
  r->image_bytes = r->cmap_at + 256;
  std::vector<uint8_t> image(r->image_bytes, 0);
  memcpy(image.data(), prog.table.data(), r->table_bytes);
  memcpy(image.data() + r->flags_at, prog.flags.data(), r->n_states);
  memcpy(image.data() + r->cmap_at, prog.cmap, 256);
  int32_t st = dbhip_alloc(r->image_bytes, (void**)&r->image_dev);
  if (!st && hipMemcpy(r->image_dev, image.data(), r->image_bytes, hipMemcpyHostToDevice) != hipSuccess) {
    set_error("dbhip_regex_create: the copy of the tables to the device failed");
    st = DBHIP_ERR_HIP;
  }
  if (st) {
    if (r->image_dev) (void)dbhip_free(r->image_dev);
    delete r;
    return st;
  }
  *out_host = r;
  return DBHIP_OK;
}

int32_t dbhip_regex_eval(const dbhip_regex* r, const dbhip_col* col, int32_t flags, int64_t n, uint8_t* out_bitmap, uint8_t* out_declined,
                         uint64_t* declined_count_dev, void* stream) {
  DBHIP_REQUIRE(r && col, "dbhip_regex_eval: NULL handle or column");
  DBHIP_REQUIRE(!(flags & ~DBHIP_REGEX_NEGATE), "dbhip_regex_eval: unknown flag bits");
  DBHIP_REQUIRE(col->type == DBHIP_T_STRING, "dbhip_regex_eval: the column must be a String column");
  DBHIP_REQUIRE(n >= 0 && n <= REGEX_MAX_ROWS, "dbhip_regex_eval: row count outside 0 .. 2^32 - 2");
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(col->data && out_bitmap && !((uintptr_t)out_bitmap & 7) && !((uintptr_t)out_declined & 7) && !((uintptr_t)col->data & 15) &&
                    !((uintptr_t)declined_count_dev & 7),
                "dbhip_regex_eval: NULL views or bitmap, views not 16-byte aligned, or a bitmap or counter not 8-byte aligned");
  hipStream_t s = resolve_stream(stream);
  RegexParams P;
  memset(&P, 0, sizeof(P));
  P.views = (const uint4*)col->data;
  P.validity = col->validity;
  P.voff = col->validity_offset;
  P.buffers = col->buffers;
  P.n_buffers = col->buffers && col->n_buffers > 0 ? col->n_buffers : 0;
  P.out = (uint64_t*)out_bitmap;
  P.out_declined = (uint64_t*)out_declined;
  P.declined_count = (unsigned long long*)declined_count_dev;
  P.image = r->image_dev;
  P.n = n;
  P.image_bytes = r->image_bytes;
  P.flags_at = r->flags_at;
  P.cmap_at = r->cmap_at;
  P.n_classes = r->n_classes;
  P.negate = (flags & DBHIP_REGEX_NEGATE) ? 1 : 0;
  P.needs_ascii = (int32_t)r->needs_ascii;
  if (!col->is_scalar) {
    // the grid: at most four workgroups per CU fit beside each other with the largest image in LDS
    hipLaunchKernelGGL(regex_rows_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), r->image_bytes, s, P);
    DBHIP_LAUNCH_CHECK();
    return DBHIP_OK;
  }
  uint64_t* ws = (uint64_t*)scratch(16, REGEX_SCRATCH_SLOT, s);   // the one result word | the one declined word: both written by the rows kernel
  if (!ws) return DBHIP_ERR_HIP;
  P.out = ws;
  P.out_declined = ws + 1;
  P.declined_count = nullptr;
  P.n = 1;
  hipLaunchKernelGGL(regex_rows_kernel, dim3(1), dim3(256), r->image_bytes, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, "dbhip_regex_eval");
  hipLaunchKernelGGL(regex_fill_kernel, dim3(grid_for((n + 63) >> 6, 256)), dim3(256), 0, s, (const uint64_t*)ws, (uint64_t*)out_bitmap, (uint64_t*)out_declined,
                     (unsigned long long*)declined_count_dev, n);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

int32_t dbhip_regex_destroy(dbhip_regex* r) {
  if (!r) return DBHIP_OK;
  (void)hipDeviceSynchronize();
  (void)dbhip_free(r->image_dev);
  delete r;
  return DBHIP_OK;
}

}  // extern "C"
