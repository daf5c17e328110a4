// k_window.hip — window functions over a sorted block (include/dbhip.h a19).
//
// Reference: TransformWindow (pipelines/processors/transforms/window/transform_window.rs, window_function.rs, frame_bound.rs)
// walks a block that is already ordered by (partition keys, order keys), keeps the partition and peer-group boundaries of the
// current row and evaluates one function per row over its frame. Device form, one call over the whole sorted input:
//   bounds     head flags from neighbour compares on the key columns (per-type equality with the sort's ties: NULL = NULL, every
//              NaN one value, -0.0 = +0.0, strings by length and bytes), then a forward max-scan of the head positions (starts)
//              and a reverse min-scan of the next head (ends): tile summaries -> one block over the summaries -> apply
//   rank       one pass over the four boundary arrays; dense_rank = a segmented count of peer heads (the scan below)
//   aggregate  a segmented inclusive scan over the partitions with a typed operator (tile summaries -> one block over the
//              summaries -> apply; no workgroup ever waits for another one), then one pass that resolves every row's frame:
//              scan[hi - 1] for frames that start at the partition, the difference of two scan entries for wrapping sums and
//              counts; float SUM and MIN / MAX over a moving start combine the frame's own terms only (a walk, over per-256 and
//              per-65536-row partials when the frame can be long)
//   shift / value   a gather through the row's source position with the validity word of 64 rows built from one ballot
#include <string.h>
#include <type_traits>
#include "dev_common.h"
#include "dev_strview.h"
#include "runtime.h"

using namespace dbhip;

namespace {

constexpr int WIN_ITEMS = 4;                 // consecutive rows per thread: 16-byte loads and stores of the u32 boundary arrays
constexpr int WIN_TILE = 256 * WIN_ITEMS;    // rows per workgroup
constexpr int WIN_SCRATCH_SLOT = 7;          // the sort's slot: a window follows a sort and neither holds scratch across calls
constexpr uint32_t WIN_P1 = 256, WIN_P2 = 65536;   // rows per first- and second-level partial of the walk

struct WinKey {
  const void* data;
  const uint8_t* validity;
  int64_t voff;
  const void* const* buffers;
  int32_t type;
  int32_t n_buffers;
};
struct WinKeys {
  WinKey k[16];      // partition keys, then order keys
  int32_t n_part, n_all;
};

struct WinRows { const uint32_t* part_start; const uint32_t* part_end; const uint32_t* peer_start; const uint32_t* peer_end; };
struct WinFrame { int32_t units, sk, ek, _pad; uint64_t so, eo; };
struct WinArg { const void* data; const uint8_t* validity; int64_t voff; int32_t type; int32_t is_scalar; };

// ---- key equality (the ties of dbhip_sort_perm) --------------------------------------------------------------------------------
__device__ __forceinline__ bool win_key_equal(const WinKey& c, uint32_t a, uint32_t b, uint32_t* bad) {
  if (c.validity) {
    const bool va = bit_get(c.validity, c.voff + a), vb = bit_get(c.validity, c.voff + b);
    if (!va || !vb) return va == vb;       // NULL ties with NULL; the values under NULLs are not read
  }
  switch (c.type) {
    case DBHIP_T_BOOL: return bit_get((const uint8_t*)c.data, a) == bit_get((const uint8_t*)c.data, b);
    case DBHIP_T_I8: case DBHIP_T_U8: return ((const uint8_t*)c.data)[a] == ((const uint8_t*)c.data)[b];
    case DBHIP_T_I16: case DBHIP_T_U16: return ((const uint16_t*)c.data)[a] == ((const uint16_t*)c.data)[b];
    case DBHIP_T_I32: case DBHIP_T_U32: case DBHIP_T_DATE: return ((const uint32_t*)c.data)[a] == ((const uint32_t*)c.data)[b];
    case DBHIP_T_I64: case DBHIP_T_U64: case DBHIP_T_TIMESTAMP: case DBHIP_T_DEC64:
      return ((const uint64_t*)c.data)[a] == ((const uint64_t*)c.data)[b];
    case DBHIP_T_F32: {   // OrderedFloat: every NaN is one value; == already ties the two zeros
      const float x = ((const float*)c.data)[a], y = ((const float*)c.data)[b];
      return x == y || (x != x && y != y);
    }
    case DBHIP_T_F64: {
      const double x = ((const double*)c.data)[a], y = ((const double*)c.data)[b];
      return x == y || (x != x && y != y);
    }
    case DBHIP_T_DEC128: {
      const uint64_t* p = (const uint64_t*)c.data + 2 * (uint64_t)a;
      const uint64_t* q = (const uint64_t*)c.data + 2 * (uint64_t)b;
      return p[0] == q[0] && p[1] == q[1];
    }
    case DBHIP_T_STRING: {
      const uint32_t* va = (const uint32_t*)c.data + 4 * (uint64_t)a;
      const uint32_t* vb = (const uint32_t*)c.data + 4 * (uint64_t)b;
      const uint32_t len = va[0];
      if (len != vb[0]) return false;
      if (sv_is_inline(len)) {
        const uint8_t* pa = (const uint8_t*)(va + 1);
        const uint8_t* pb = (const uint8_t*)(vb + 1);
        for (uint32_t k = 0; k < len; ++k)
          if (pa[k] != pb[k]) return false;
        return true;
      }
      if (va[1] != vb[1]) return false;      // the 4-byte prefix
      if (!c.buffers || va[2] >= (uint32_t)c.n_buffers || vb[2] >= (uint32_t)c.n_buffers) { *bad = 1; return false; }   // no table, or a view that points past it
      const uint8_t* pa = sv_bytes(va, c.buffers);
      const uint8_t* pb = sv_bytes(vb, c.buffers);
      if (pa == pb) return true;
      uint32_t k = 4;
      if ((((uintptr_t)pa | (uintptr_t)pb) & 7) == 0) {   // both values begin on an 8-byte boundary: whole words, then the tail
        for (k = 0; k + 8 <= len; k += 8)
          if (*(const uint64_t*)(pa + k) != *(const uint64_t*)(pb + k)) return false;
      }
      for (; k < len; ++k)
        if (pa[k] != pb[k]) return false;
      return true;
    }
  }
  return true;
}

__device__ __forceinline__ void win_load4(const uint32_t* p, int64_t i0, int64_t n, bool al16, uint32_t fill, uint32_t (&v)[WIN_ITEMS]) {
  if (al16 && i0 + WIN_ITEMS <= n) {
    const uint4 q = *(const uint4*)(p + i0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j) v[j] = i0 + j < n ? p[i0 + j] : fill;
  }
}

__device__ __forceinline__ void win_store4(uint32_t* p, int64_t i0, int64_t n, bool al16, const uint32_t (&v)[WIN_ITEMS]) {
  if (al16 && i0 + WIN_ITEMS <= n) {
    *(uint4*)(p + i0) = make_uint4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j)
      if (i0 + j < n) p[i0 + j] = v[j];
  }
}

// the validity (or Boolean value) bits of the 64 rows of a wave, rows [row0, row0 + 64), row0 a multiple of 64: one ballot, eight byte stores
__device__ __forceinline__ void win_put_bits(uint8_t* out, int64_t row0, int64_t n, bool bit) {
  const uint64_t m = __ballot(bit);
  const int lane = lane_id();
  if (lane < 8 && row0 < n) out[(row0 >> 3) + lane] = (uint8_t)(m >> (8 * lane));   // (the bitmap holds ceil(n / 64) words)
}

// ---- boundaries ----------------------------------------------------------------------------------------------------------------
// flags[i]: bit 0 = row i begins a partition, bit 1 = row i begins a peer group. tsum[tile] = {last partition head, last peer head
// (0 when the tile has none: row 0 is a head of both), first partition head, first peer head (n when none)}
__global__ __launch_bounds__(256) void win_heads_kernel(WinKeys keys, int64_t n, uint8_t* flags, uint4* tsum, uint32_t* bad) {
  __shared__ uint4 wsum[4];
  const int64_t i0 = (int64_t)blockIdx.x * WIN_TILE + threadIdx.x * WIN_ITEMS;
  uint32_t f[WIN_ITEMS];
  uint4 s = make_uint4(0u, 0u, (uint32_t)n, (uint32_t)n);
  uint32_t lbad = 0;
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; ++j) {
    const int64_t i = i0 + j;
    f[j] = 0;
    if (i >= n) continue;
    bool part_head = i == 0, peer_head = i == 0;
    if (i > 0) {
      for (int k = 0; k < keys.n_all && !peer_head; ++k) {
        if (!win_key_equal(keys.k[k], (uint32_t)(i - 1), (uint32_t)i, &lbad)) {
          peer_head = true;
          part_head = k < keys.n_part;
        }
      }
    }
    f[j] = (part_head ? 1u : 0u) | (peer_head ? 2u : 0u);
    if (part_head) { s.x = (uint32_t)i; if (s.z == (uint32_t)n) s.z = (uint32_t)i; }
    if (peer_head) { s.y = (uint32_t)i; if (s.w == (uint32_t)n) s.w = (uint32_t)i; }
  }
  if (i0 < n) {   // four flag bytes as one word (i0 is a multiple of 4; the scratch array is padded to a multiple of 4)
    *(uint32_t*)(flags + i0) = f[0] | (f[1] << 8) | (f[2] << 16) | (f[3] << 24);
  }
  if (lbad) atomicOr(bad, 1u);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t x = __shfl_xor(s.x, off, 64), y = __shfl_xor(s.y, off, 64), z = __shfl_xor(s.z, off, 64), w = __shfl_xor(s.w, off, 64);
    s.x = x > s.x ? x : s.x; s.y = y > s.y ? y : s.y; s.z = z < s.z ? z : s.z; s.w = w < s.w ? w : s.w;
  }
  if (lane_id() == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      const uint4 o = wsum[w];
      s.x = o.x > s.x ? o.x : s.x; s.y = o.y > s.y ? o.y : s.y; s.z = o.z < s.z ? o.z : s.z; s.w = o.w < s.w ? o.w : s.w;
    }
    tsum[blockIdx.x] = s;
  }
}

// one workgroup over the tile summaries: tsum[t] becomes {last heads in the tiles before t, first heads in the tiles after t}.
// Thread k owns a contiguous run of tiles: fold the run, scan the 1024 folds, walk the run again.
__global__ __launch_bounds__(1024) void win_heads_carry_kernel(uint4* tsum, int64_t nt, uint32_t n) {
  __shared__ uint4 wave_tot[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t chunk = (nt + 1023) / 1024;
  const int64_t lo = tid * chunk < nt ? tid * chunk : nt, hi = lo + chunk < nt ? lo + chunk : nt;
  uint4 a = make_uint4(0u, 0u, n, n);
  for (int64_t t = lo; t < hi; ++t) {
    const uint4 o = tsum[t];
    a.x = o.x > a.x ? o.x : a.x; a.y = o.y > a.y ? o.y : a.y; a.z = o.z < a.z ? o.z : a.z; a.w = o.w < a.w ? o.w : a.w;
  }
  // forward inclusive max of (x, y), reverse inclusive min of (z, w) over the threads
  uint4 inc = a;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t x = __shfl_up(inc.x, d, 64), y = __shfl_up(inc.y, d, 64), z = __shfl_down(inc.z, d, 64), w = __shfl_down(inc.w, d, 64);
    if (lane >= d) { inc.x = x > inc.x ? x : inc.x; inc.y = y > inc.y ? y : inc.y; }
    if (lane + d < 64) { inc.z = z < inc.z ? z : inc.z; inc.w = w < inc.w ? w : inc.w; }
  }
  if (lane == 63) { wave_tot[wave].x = inc.x; wave_tot[wave].y = inc.y; }
  if (lane == 0) { wave_tot[wave].z = inc.z; wave_tot[wave].w = inc.w; }
  __syncthreads();
  uint4 pre = make_uint4(0u, 0u, n, n);
  for (int w = 0; w < wave; ++w) { pre.x = wave_tot[w].x > pre.x ? wave_tot[w].x : pre.x; pre.y = wave_tot[w].y > pre.y ? wave_tot[w].y : pre.y; }
  for (int w = 15; w > wave; --w) { pre.z = wave_tot[w].z < pre.z ? wave_tot[w].z : pre.z; pre.w = wave_tot[w].w < pre.w ? wave_tot[w].w : pre.w; }
  {
    const uint32_t x = __shfl_up(inc.x, 1, 64), y = __shfl_up(inc.y, 1, 64), z = __shfl_down(inc.z, 1, 64), w = __shfl_down(inc.w, 1, 64);
    if (lane > 0) { pre.x = x > pre.x ? x : pre.x; pre.y = y > pre.y ? y : pre.y; }
    if (lane < 63) { pre.z = z < pre.z ? z : pre.z; pre.w = w < pre.w ? w : pre.w; }
  }
  // the run again: forward for the starts, backward for the ends (two sweeps, the second one over what the first left in x, y)
  uint32_t rx = pre.x, ry = pre.y;
  for (int64_t t = lo; t < hi; ++t) {
    uint4 o = tsum[t];
    const uint32_t ox = o.x, oy = o.y;
    o.x = rx; o.y = ry;
    tsum[t] = o;
    rx = ox > rx ? ox : rx; ry = oy > ry ? oy : ry;
  }
  uint32_t rz = pre.z, rw = pre.w;
  for (int64_t t = hi - 1; t >= lo; --t) {
    uint4 o = tsum[t];
    const uint32_t oz = o.z, ow = o.w;
    o.z = rz; o.w = rw;
    tsum[t] = o;
    rz = oz < rz ? oz : rz; rw = ow < rw ? ow : rw;
  }
}

__global__ __launch_bounds__(256) void win_bounds_apply_kernel(const uint8_t* flags, const uint4* tsum, int64_t n, uint32_t* part_start,
                                                               uint32_t* part_end, uint32_t* peer_start, uint32_t* peer_end, int al16) {
  __shared__ uint4 wave_tot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * WIN_TILE + tid * WIN_ITEMS;
  const uint32_t N = (uint32_t)n;
  uint32_t f[WIN_ITEMS] = {0, 0, 0, 0};
  if (i0 < n) {
    const uint32_t w = *(const uint32_t*)(flags + i0);
#pragma unroll
    for (int j = 0; j < WIN_ITEMS; ++j) f[j] = i0 + j < n ? (w >> (8 * j)) & 0xFF : 0u;
  }
  // the thread's own last / first heads
  uint4 a = make_uint4(0u, 0u, N, N);
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; ++j) {
    if (f[j] & 1) { a.x = (uint32_t)(i0 + j); if (a.z == N) a.z = (uint32_t)(i0 + j); }
    if (f[j] & 2) { a.y = (uint32_t)(i0 + j); if (a.w == N) a.w = (uint32_t)(i0 + j); }
  }
  uint4 inc = a;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t x = __shfl_up(inc.x, d, 64), y = __shfl_up(inc.y, d, 64), z = __shfl_down(inc.z, d, 64), w = __shfl_down(inc.w, d, 64);
    if (lane >= d) { inc.x = x > inc.x ? x : inc.x; inc.y = y > inc.y ? y : inc.y; }
    if (lane + d < 64) { inc.z = z < inc.z ? z : inc.z; inc.w = w < inc.w ? w : inc.w; }
  }
  if (lane == 63) { wave_tot[wave].x = inc.x; wave_tot[wave].y = inc.y; }
  if (lane == 0) { wave_tot[wave].z = inc.z; wave_tot[wave].w = inc.w; }
  __syncthreads();
  uint4 pre = tsum[blockIdx.x];      // heads before / after this tile
  for (int w = 0; w < wave; ++w) { pre.x = wave_tot[w].x > pre.x ? wave_tot[w].x : pre.x; pre.y = wave_tot[w].y > pre.y ? wave_tot[w].y : pre.y; }
  for (int w = 3; w > wave; --w) { pre.z = wave_tot[w].z < pre.z ? wave_tot[w].z : pre.z; pre.w = wave_tot[w].w < pre.w ? wave_tot[w].w : pre.w; }
  {
    const uint32_t x = __shfl_up(inc.x, 1, 64), y = __shfl_up(inc.y, 1, 64), z = __shfl_down(inc.z, 1, 64), w = __shfl_down(inc.w, 1, 64);
    if (lane > 0) { pre.x = x > pre.x ? x : pre.x; pre.y = y > pre.y ? y : pre.y; }
    if (lane < 63) { pre.z = z < pre.z ? z : pre.z; pre.w = w < pre.w ? w : pre.w; }
  }
  if (i0 >= n) return;
  uint32_t ps[WIN_ITEMS], qs[WIN_ITEMS], pe[WIN_ITEMS], qe[WIN_ITEMS];
  uint32_t rx = pre.x, ry = pre.y;
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; ++j) {      // start of row i = the last head at or before i
    if (f[j] & 1) rx = (uint32_t)(i0 + j);
    if (f[j] & 2) ry = (uint32_t)(i0 + j);
    ps[j] = rx; qs[j] = ry;
  }
  uint32_t rz = pre.z, rw = pre.w;
#pragma unroll
  for (int j = WIN_ITEMS - 1; j >= 0; --j) {  // end of row i = the first head after i
    pe[j] = rz; qe[j] = rw;
    if (f[j] & 1) rz = (uint32_t)(i0 + j);
    if (f[j] & 2) rw = (uint32_t)(i0 + j);
  }
  win_store4(part_start, i0, n, al16 & 1, ps);
  win_store4(part_end, i0, n, al16 & 1, pe);
  win_store4(peer_start, i0, n, al16 & 1, qs);
  win_store4(peer_end, i0, n, al16 & 1, qe);
}

// ---- the frame of a row --------------------------------------------------------------------------------------------------------
// [lo, hi) clamped into [ps, pe]; every compare is made before the arithmetic it guards, so offsets up to 2^63 - 1 cannot wrap
__device__ __forceinline__ void win_frame(const WinFrame& f, uint32_t i, uint32_t ps, uint32_t pe, uint32_t qs, uint32_t qe, uint32_t* lo,
                                          uint32_t* hi) {
  uint32_t l, h;
  switch (f.sk) {
    case DBHIP_WIN_UNBOUNDED_PRECEDING: l = ps; break;
    case DBHIP_WIN_PRECEDING: l = f.so > (uint64_t)(i - ps) ? ps : i - (uint32_t)f.so; break;
    case DBHIP_WIN_CURRENT_ROW: l = f.units == DBHIP_WIN_RANGE ? qs : i; break;
    default: l = f.so > (uint64_t)(pe - i) ? pe : i + (uint32_t)f.so; break;    // FOLLOWING
  }
  switch (f.ek) {
    case DBHIP_WIN_UNBOUNDED_FOLLOWING: h = pe; break;
    case DBHIP_WIN_PRECEDING: h = f.eo > (uint64_t)(i - ps) ? ps : i - (uint32_t)f.eo + 1; break;
    case DBHIP_WIN_CURRENT_ROW: h = f.units == DBHIP_WIN_RANGE ? qe : i + 1; break;
    default: h = f.eo >= (uint64_t)(pe - i) ? pe : i + (uint32_t)f.eo + 1; break;   // FOLLOWING
  }
  *lo = l;
  *hi = h;
}

// ---- rank family ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void win_rank_kernel(WinRows r, int64_t n, int kind, uint64_t buckets, void* out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t ps = r.part_start[i];
    switch (kind) {
      case DBHIP_WIN_ROW_NUMBER: ((uint64_t*)out)[i] = (uint64_t)((uint32_t)i - ps) + 1; break;
      case DBHIP_WIN_RANK: ((uint64_t*)out)[i] = (uint64_t)(r.peer_start[i] - ps) + 1; break;
      case DBHIP_WIN_PERCENT_RANK: {
        const uint32_t rows = r.part_end[i] - ps;
        ((double*)out)[i] = rows <= 1 ? 0.0 : (double)(r.peer_start[i] - ps) / (double)(rows - 1);
        break;
      }
      case DBHIP_WIN_CUME_DIST: ((double*)out)[i] = (double)(r.peer_end[i] - ps) / (double)(r.part_end[i] - ps); break;
      default: {   // ntile
        const uint64_t rows = r.part_end[i] - ps, k = (uint32_t)i - ps;
        const uint64_t q = rows / buckets, rem = rows % buckets;
        ((uint64_t*)out)[i] = k < rem * (q + 1) ? k / (q + 1) + 1 : (k - rem * (q + 1)) / q + rem + 1;   // (q = 0 leaves rem = rows > k)
        break;
      }
    }
  }
}

// ---- typed operators of the segmented scan ---------------------------------------------------------------------------------------
__device__ __forceinline__ bool of_less(double a, double b) {   // OrderedFloat: NaN is the largest value
  const bool an = a != a, bn = b != b;
  if (an || bn) return !an && bn;
  return a < b;
}

__device__ __forceinline__ int64_t win_load_int(const WinArg& a, uint32_t i) {
  switch (a.type) {
    case DBHIP_T_I8: return ((const int8_t*)a.data)[i];
    case DBHIP_T_I16: return ((const int16_t*)a.data)[i];
    case DBHIP_T_I32: case DBHIP_T_DATE: return ((const int32_t*)a.data)[i];
    case DBHIP_T_U8: return ((const uint8_t*)a.data)[i];
    case DBHIP_T_U16: return ((const uint16_t*)a.data)[i];
    case DBHIP_T_U32: return ((const uint32_t*)a.data)[i];
    default: return ((const int64_t*)a.data)[i];     // I64, U64 (its bits), TIMESTAMP, DEC64
  }
}
__device__ __forceinline__ double win_load_f64(const WinArg& a, uint32_t i) {
  return a.type == DBHIP_T_F32 ? (double)((const float*)a.data)[i] : ((const double*)a.data)[i];
}
__device__ __forceinline__ i128 win_load_i128(const WinArg& a, uint32_t i) {
  const uint64_t* p = (const uint64_t*)a.data + 2 * (uint64_t)i;
  return (i128)(((u128)p[1] << 64) | p[0]);
}

enum { WOP_ADD_U64, WOP_ADD_F64, WOP_ADD_U128, WOP_SAT_U128, WOP_MIN_I64, WOP_MAX_I64, WOP_MIN_U64, WOP_MAX_U64, WOP_MIN_F64, WOP_MAX_F64,
       WOP_MIN_I128, WOP_MAX_I128 };

template <int OP> struct WinOp;
template <> struct WinOp<WOP_ADD_U64> {   // wrapping i64 / u64 sums: the same bits
  typedef uint64_t T;
  static __device__ __forceinline__ T load(const WinArg& a, uint32_t i) { return (uint64_t)win_load_int(a, i); }
  static __device__ __forceinline__ T comb(T a, T b) { return a + b; }
  static __device__ __forceinline__ T sub(T a, T b) { return a - b; }
};
template <> struct WinOp<WOP_ADD_F64> {
  typedef double T;
  static __device__ __forceinline__ T load(const WinArg& a, uint32_t i) { return win_load_f64(a, i); }
  static __device__ __forceinline__ T comb(T a, T b) { return a + b; }
  static __device__ __forceinline__ T sub(T a, T) { return a; }     // (never a difference of float prefixes: such frames walk)
};
template <> struct WinOp<WOP_ADD_U128> {
  typedef u128 T;
  static __device__ __forceinline__ T load(const WinArg& a, uint32_t i) { return (u128)win_load_i128(a, i); }
  static __device__ __forceinline__ T comb(T a, T b) { return a + b; }
  static __device__ __forceinline__ T sub(T a, T b) { return a - b; }
};
template <> struct WinOp<WOP_SAT_U128> {  // sum of |x|, saturating: the gate of the Decimal128 sum
  typedef u128 T;
  static __device__ __forceinline__ T load(const WinArg& a, uint32_t i) { const i128 v = win_load_i128(a, i); return v < 0 ? (u128)0 - (u128)v : (u128)v; }
  static __device__ __forceinline__ T comb(T a, T b) { const T s = a + b; return s < a ? ~(u128)0 : s; }
  static __device__ __forceinline__ T sub(T a, T) { return a; }
};
#define WIN_MINMAX_OP(NAME, TYPE, LOAD, TAKE_B)                                                              \
  template <> struct WinOp<NAME> {                                                                           \
    typedef TYPE T;                                                                                          \
    static __device__ __forceinline__ T load(const WinArg& a, uint32_t i) { return (TYPE)LOAD(a, i); }       \
    static __device__ __forceinline__ T comb(T a, T b) { return (TAKE_B) ? b : a; }                          \
    static __device__ __forceinline__ T sub(T a, T) { return a; }                                            \
  };
WIN_MINMAX_OP(WOP_MIN_I64, int64_t, win_load_int, b < a)
WIN_MINMAX_OP(WOP_MAX_I64, int64_t, win_load_int, a < b)
WIN_MINMAX_OP(WOP_MIN_U64, uint64_t, win_load_int, b < a)
WIN_MINMAX_OP(WOP_MAX_U64, uint64_t, win_load_int, a < b)
WIN_MINMAX_OP(WOP_MIN_F64, double, win_load_f64, of_less(b, a))
WIN_MINMAX_OP(WOP_MAX_F64, double, win_load_f64, of_less(a, b))
WIN_MINMAX_OP(WOP_MIN_I128, i128, win_load_i128, b < a)
WIN_MINMAX_OP(WOP_MAX_I128, i128, win_load_i128, a < b)
#undef WIN_MINMAX_OP

__device__ __forceinline__ bool win_valid(const WinArg& a, uint32_t i) { return !a.validity || bit_get(a.validity, a.voff + i); }

// what a row contributes: its value when it is valid
template <int OP> struct ArgLoader {
  WinArg a;
  __device__ __forceinline__ bool get(uint32_t i, typename WinOp<OP>::T* v) const {
    if (!win_valid(a, i)) return false;     // the value under a NULL is not read
    *v = WinOp<OP>::load(a, i);
    return true;
  }
};
struct ValidLoader {      // count(col): only the number of valid rows is wanted
  WinArg a;
  __device__ __forceinline__ bool get(uint32_t i, uint64_t* v) const { *v = 0; return win_valid(a, i); }
};
struct PeerHeadLoader {   // dense_rank: 1 for the first row of a peer group
  const uint32_t* peer_start;
  __device__ __forceinline__ bool get(uint32_t i, uint64_t* v) const { *v = peer_start[i] == i ? 1 : 0; return true; }
};

// an element of the segmented scan: the fold of the valid rows of a span, their number, and whether a partition begins inside the span
template <int OP> struct Seg {
  typename WinOp<OP>::T v;
  uint32_t cnt, head;
};

template <int OP> __device__ __forceinline__ Seg<OP> seg_identity() {
  Seg<OP> r;
  r.v = typename WinOp<OP>::T();
  r.cnt = 0;
  r.head = 0;
  return r;
}

template <int OP> __device__ __forceinline__ Seg<OP> seg_comb(const Seg<OP>& a, const Seg<OP>& b) {
  if (b.head) return b;          // a partition begins inside b: nothing of a reaches past it
  Seg<OP> r;
  r.head = a.head;
  if (a.cnt == 0) { r.v = b.v; r.cnt = b.cnt; }
  else if (b.cnt == 0) { r.v = a.v; r.cnt = a.cnt; }
  else { r.v = WinOp<OP>::comb(a.v, b.v); r.cnt = a.cnt + b.cnt; }
  return r;
}

template <class T> __device__ __forceinline__ T win_shfl_up(T v, int d) {
  static_assert(sizeof(T) % 4 == 0, "whole dwords");
  uint32_t w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (unsigned k = 0; k < sizeof(T) / 4; ++k) w[k] = __shfl_up(w[k], d, 64);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}

// exclusive segmented scan of one element per thread over the workgroup; *total (thread 0 only, may be NULL) = the fold of all
template <int OP, int NT> __device__ __forceinline__ Seg<OP> block_excl_scan(const Seg<OP>& x, Seg<OP>* wave_tot, Seg<OP>* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Seg<OP> inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Seg<OP> o = win_shfl_up(inc, d);
    if (lane >= d) inc = seg_comb<OP>(o, inc);
  }
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  Seg<OP> pre = seg_identity<OP>();
  for (int w = 0; w < wave; ++w) pre = seg_comb<OP>(pre, wave_tot[w]);
  const Seg<OP> prev = win_shfl_up(inc, 1);
  if (lane > 0) pre = seg_comb<OP>(pre, prev);
  if (total && threadIdx.x == 0) {
    Seg<OP> t = wave_tot[0];
    for (int w = 1; w < NT / 64; ++w) t = seg_comb<OP>(t, wave_tot[w]);
    *total = t;
  }
  return pre;
}

template <int OP, class LD> __device__ __forceinline__ void win_tile_elems(const LD& ld, const uint32_t* part_start, int64_t n, int al16, int64_t i0,
                                                                           Seg<OP> (&e)[WIN_ITEMS]) {
  uint32_t ps[WIN_ITEMS];
  win_load4(part_start, i0, n, al16 & 1, 0xFFFFFFFFu, ps);
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; ++j) {
    e[j] = seg_identity<OP>();
    const int64_t i = i0 + j;
    if (i < n) {
      typename WinOp<OP>::T v;
      if (ld.get((uint32_t)i, &v)) { e[j].v = v; e[j].cnt = 1; }
      e[j].head = ps[j] == (uint32_t)i ? 1u : 0u;
    }
  }
}

// pass 1: the fold of every tile
template <int OP, class LD>
__global__ __launch_bounds__(256) void win_scan_tiles_kernel(LD ld, const uint32_t* part_start, int64_t n, int al16, Seg<OP>* tsum) {
  __shared__ Seg<OP> wave_tot[4];
  const int64_t i0 = (int64_t)blockIdx.x * WIN_TILE + threadIdx.x * WIN_ITEMS;
  Seg<OP> e[WIN_ITEMS];
  win_tile_elems<OP, LD>(ld, part_start, n, al16, i0, e);
  Seg<OP> a = e[0];
#pragma unroll
  for (int j = 1; j < WIN_ITEMS; ++j) a = seg_comb<OP>(a, e[j]);
  Seg<OP> total;
  block_excl_scan<OP, 256>(a, wave_tot, &total);
  if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// pass 2: one workgroup turns the tile folds into what every tile inherits from the tiles before it
template <int OP> __global__ __launch_bounds__(1024) void win_scan_carry_kernel(Seg<OP>* tsum, int64_t nt) {
  __shared__ Seg<OP> wave_tot[16];
  const int tid = threadIdx.x;
  const int64_t chunk = (nt + 1023) / 1024;
  const int64_t lo = tid * chunk < nt ? tid * chunk : nt, hi = lo + chunk < nt ? lo + chunk : nt;
  Seg<OP> a = seg_identity<OP>();
  for (int64_t t = lo; t < hi; ++t) a = seg_comb<OP>(a, tsum[t]);
  Seg<OP> run = block_excl_scan<OP, 1024>(a, wave_tot, nullptr);
  for (int64_t t = lo; t < hi; ++t) {
    const Seg<OP> o = tsum[t];
    tsum[t] = run;
    run = seg_comb<OP>(run, o);
  }
}

// pass 3: the inclusive scan of every row. S[i] = fold of the valid rows of [part_start, i] (zero when there is none), C[i] = their number;
// `over` (the Decimal128 gate): nothing is stored, a fold above `limit` raises the word
template <int OP, class LD>
__global__ __launch_bounds__(256) void win_scan_apply_kernel(LD ld, const uint32_t* part_start, int64_t n, int al16, const Seg<OP>* tsum,
                                                             typename WinOp<OP>::T* S, uint32_t* C, uint32_t* over, typename WinOp<OP>::T limit) {
  __shared__ Seg<OP> wave_tot[4];
  const int64_t i0 = (int64_t)blockIdx.x * WIN_TILE + threadIdx.x * WIN_ITEMS;
  Seg<OP> e[WIN_ITEMS];
  win_tile_elems<OP, LD>(ld, part_start, n, al16, i0, e);
#pragma unroll
  for (int j = 1; j < WIN_ITEMS; ++j) e[j] = seg_comb<OP>(e[j - 1], e[j]);
  Seg<OP> pre = block_excl_scan<OP, 256>(e[WIN_ITEMS - 1], wave_tot, nullptr);
  pre = seg_comb<OP>(tsum[blockIdx.x], pre);
  uint32_t c[WIN_ITEMS];
  bool raise = false;
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; ++j) {
    const Seg<OP> r = seg_comb<OP>(pre, e[j]);
    c[j] = r.cnt;
    if (i0 + j < n) {
      if (over) raise |= r.v > limit;
      else if (S) S[i0 + j] = r.v;
    }
  }
  if (C && i0 < n) win_store4(C, i0, n, 1, c);
  if (raise) atomicOr(over, 1u);
}

// ---- results -------------------------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ void win_store_val(void* out, int out_type, uint32_t i, T v) {
  if constexpr (std::is_same<T, double>::value) {
    if (out_type == DBHIP_T_F32) ((float*)out)[i] = (float)v;     // (MIN / MAX of an f32: the widened value narrows back exactly)
    else ((double*)out)[i] = v;
  } else if constexpr (sizeof(T) == 16) {
    uint64_t* p = (uint64_t*)out + 2 * (uint64_t)i;
    p[0] = (uint64_t)(u128)v;
    p[1] = (uint64_t)((u128)v >> 64);
  } else {
    switch (out_type) {
      case DBHIP_T_I8: case DBHIP_T_U8: ((uint8_t*)out)[i] = (uint8_t)v; break;
      case DBHIP_T_I16: case DBHIP_T_U16: ((uint16_t*)out)[i] = (uint16_t)v; break;
      case DBHIP_T_I32: case DBHIP_T_U32: case DBHIP_T_DATE: ((uint32_t*)out)[i] = (uint32_t)v; break;
      default: ((uint64_t*)out)[i] = (uint64_t)v; break;
    }
  }
}

// frames answered from the scan: scan[hi - 1], less scan[lo - 1] when the frame starts after the partition does (wrapping sums, counts)
template <int OP>
__global__ __launch_bounds__(256) void win_resolve_kernel(WinRows r, WinFrame f, int64_t n, const typename WinOp<OP>::T* S, const uint32_t* C,
                                                          int count_only, void* out, int out_type, uint8_t* out_validity) {
  typedef typename WinOp<OP>::T T;
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < n; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + threadIdx.x;
    bool valid = false;
    if (i < n) {
      const uint32_t ps = r.part_start[i];
      uint32_t lo, hi;
      win_frame(f, (uint32_t)i, ps, r.part_end[i], r.peer_start[i], r.peer_end[i], &lo, &hi);
      T v = T();
      uint32_t c = 0;
      if (hi > lo) {
        c = C[hi - 1];
        if (!count_only) v = S[hi - 1];
        if (lo > ps) {
          c -= C[lo - 1];
          if (!count_only) v = WinOp<OP>::sub(v, S[lo - 1]);
        }
      }
      if (count_only) { ((uint64_t*)out)[i] = c; valid = true; }
      else { valid = c != 0; win_store_val<T>(out, out_type, (uint32_t)i, valid ? v : T()); }
    }
    win_put_bits(out_validity, i - lane_id(), n, valid);
  }
}

__global__ __launch_bounds__(256) void win_count_star_kernel(WinRows r, WinFrame f, int64_t n, uint64_t* out, uint8_t* out_validity) {
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < n; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + threadIdx.x;
    if (i < n) {
      uint32_t lo, hi;
      win_frame(f, (uint32_t)i, r.part_start[i], r.part_end[i], r.peer_start[i], r.peer_end[i], &lo, &hi);
      out[i] = hi > lo ? hi - lo : 0;
    }
    win_put_bits(out_validity, i - lane_id(), n, i < n);
  }
}

// partials of the walk: the fold of the valid rows of every aligned run of 256 rows (partitions do not matter: a partial is only
// used when its whole run lies inside a frame), then of 256 such partials
template <int OP> __device__ __forceinline__ void win_fold(typename WinOp<OP>::T* acc, uint32_t* cnt, typename WinOp<OP>::T v, uint32_t c) {
  if (c == 0) return;
  *acc = *cnt ? WinOp<OP>::comb(*acc, v) : v;
  *cnt += c;
}

template <int OP>
__global__ __launch_bounds__(256) void win_partial_kernel(ArgLoader<OP> ld, const typename WinOp<OP>::T* in_v, const uint32_t* in_c, int64_t n_in,
                                                          typename WinOp<OP>::T* out_v, uint32_t* out_c) {
  typedef typename WinOp<OP>::T T;
  __shared__ T wv[4];
  __shared__ uint32_t wc[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  T v = T();
  uint32_t c = 0;
  if (i < n_in) {
    if (in_v) { v = in_v[i]; c = in_c[i]; }
    else if (ld.get((uint32_t)i, &v)) c = 1;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {      // in row order, like everything else here
    const T ov = win_shfl_up(v, d);
    const uint32_t oc = __shfl_up(c, d, 64);
    if (lane_id() >= d) {
      T a = ov;
      uint32_t ac = oc;
      win_fold<OP>(&a, &ac, v, c);
      v = a; c = ac;
    }
  }
  if (lane_id() == 63) { wv[threadIdx.x >> 6] = v; wc[threadIdx.x >> 6] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    T a = wv[0];
    uint32_t ac = wc[0];
    for (int w = 1; w < 4; ++w) win_fold<OP>(&a, &ac, wv[w], wc[w]);
    out_v[blockIdx.x] = ac ? a : T();
    out_c[blockIdx.x] = ac;
  }
}

// frames with a moving start under float SUM and MIN / MAX: the frame's own terms and nothing else
template <int OP>
__global__ __launch_bounds__(256) void win_walk_kernel(ArgLoader<OP> ld, WinRows r, WinFrame f, int64_t n, const typename WinOp<OP>::T* p1v,
                                                       const uint32_t* p1c, const typename WinOp<OP>::T* p2v, const uint32_t* p2c, void* out,
                                                       int out_type, uint8_t* out_validity) {
  typedef typename WinOp<OP>::T T;
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < n; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + threadIdx.x;
    bool valid = false;
    if (i < n) {
      uint32_t lo, hi;
      win_frame(f, (uint32_t)i, r.part_start[i], r.part_end[i], r.peer_start[i], r.peer_end[i], &lo, &hi);
      T acc = T();
      uint32_t cnt = 0;
      uint64_t p = lo;
      const uint64_t e = hi;
      T v;
      if (p1v) {
        for (; p < e && (p & (WIN_P1 - 1)); ++p)
          if (ld.get((uint32_t)p, &v)) win_fold<OP>(&acc, &cnt, v, 1);
        for (; p + WIN_P1 <= e && (p & (WIN_P2 - 1)); p += WIN_P1) win_fold<OP>(&acc, &cnt, p1v[p >> 8], p1c[p >> 8]);
        for (; p + WIN_P2 <= e; p += WIN_P2) win_fold<OP>(&acc, &cnt, p2v[p >> 16], p2c[p >> 16]);
        for (; p + WIN_P1 <= e; p += WIN_P1) win_fold<OP>(&acc, &cnt, p1v[p >> 8], p1c[p >> 8]);
      }
      for (; p < e; ++p)
        if (ld.get((uint32_t)p, &v)) win_fold<OP>(&acc, &cnt, v, 1);
      valid = cnt != 0;
      win_store_val<T>(out, out_type, (uint32_t)i, valid ? acc : T());
    }
    win_put_bits(out_validity, i - lane_id(), n, valid);
  }
}

// ---- shift (lag / lead) and first / last / nth value: a gather ---------------------------------------------------------------------
struct WinBit {};                               // Boolean values: one bit per row
struct WinV32 { uint4 a, b; };                  // Decimal256

enum { WIN_GATHER_SHIFT = 0, WIN_GATHER_VALUE = 1 };

template <class V>
__global__ __launch_bounds__(256) void win_gather_kernel(WinRows r, int64_t n, int mode, int64_t offset, int vkind, uint64_t nth, WinFrame f,
                                                         WinArg arg, WinArg dflt, int has_dflt, void* out, uint8_t* out_validity) {
  constexpr bool BIT = std::is_same<V, WinBit>::value;
  typedef typename std::conditional<BIT, uint8_t, V>::type E;
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < n; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + threadIdx.x;
    bool valid = false, bit = false;
    if (i < n) {
      const uint32_t ps = r.part_start[i], pe = r.part_end[i], row = (uint32_t)i;
      bool has = false;
      uint32_t src = row;
      if (mode == WIN_GATHER_SHIFT) {
        if (offset < 0) {
          const uint64_t k = (uint64_t)0 - (uint64_t)offset;
          has = k <= (uint64_t)(row - ps);
          if (has) src = row - (uint32_t)k;
        } else {
          const uint64_t k = (uint64_t)offset;
          has = k <= (uint64_t)(pe - 1 - row);
          if (has) src = row + (uint32_t)k;
        }
      } else {
        uint32_t lo, hi;
        win_frame(f, row, ps, pe, r.peer_start[i], r.peer_end[i], &lo, &hi);
        if (hi > lo) {
          if (vkind == DBHIP_WIN_FIRST_VALUE) { has = true; src = lo; }
          else if (vkind == DBHIP_WIN_LAST_VALUE) { has = true; src = hi - 1; }
          else if (nth - 1 < (uint64_t)(hi - lo)) { has = true; src = lo + (uint32_t)(nth - 1); }
        }
      }
      const bool use_dflt = !has && has_dflt;      // (selected field by field: a pointer to a kernel argument would live in scratch memory)
      if (use_dflt) { src = dflt.is_scalar ? 0u : row; has = true; }
      const void* data = use_dflt ? dflt.data : arg.data;
      const uint8_t* validity = use_dflt ? dflt.validity : arg.validity;
      const int64_t voff = use_dflt ? dflt.voff : arg.voff;
      if (has) valid = !validity || bit_get(validity, voff + src);
      if constexpr (BIT) {
        bit = valid && bit_get((const uint8_t*)data, src);
      } else {
        E v = E();
        if (valid) v = ((const E*)data)[src];
        ((E*)out)[i] = v;
      }
    }
    if constexpr (BIT) win_put_bits((uint8_t*)out, i - lane_id(), n, bit);
    win_put_bits(out_validity, i - lane_id(), n, valid);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
constexpr int64_t WIN_MAX_ROWS = 0xFFFFFFFELL;     // 2^32 - 2: row positions and one-past-the-end are u32

inline int win_grid(int64_t n) { return grid_for(n, 256, 1 << 20); }
inline int al16_of(const void* p) { return ((uintptr_t)p & 15) == 0 ? 1 : 0; }

int32_t win_check_rows(const dbhip_window_rows* rows, const char* who) {
  if (!rows || rows->n < 0 || rows->n > WIN_MAX_ROWS) { set_error("%s: NULL rows or a row count outside 0 .. 2^32 - 2", who); return DBHIP_ERR_INVALID; }
  if (rows->n > 0 && (!rows->part_start || !rows->part_end || !rows->peer_start || !rows->peer_end)) {
    set_error("%s: a boundary array is NULL", who);
    return DBHIP_ERR_INVALID;
  }
  return DBHIP_OK;
}

WinRows win_rows(const dbhip_window_rows* rows) { return WinRows{rows->part_start, rows->part_end, rows->peer_start, rows->peer_end}; }

int32_t win_check_frame(const dbhip_window_frame* fr, const char* who, WinFrame* f) {
  if (!fr) { set_error("%s: NULL frame", who); return DBHIP_ERR_INVALID; }
  const int sk = fr->start_kind, ek = fr->end_kind;
  const bool s_off = sk == DBHIP_WIN_PRECEDING || sk == DBHIP_WIN_FOLLOWING, e_off = ek == DBHIP_WIN_PRECEDING || ek == DBHIP_WIN_FOLLOWING;
  bool bad = (fr->units != DBHIP_WIN_ROWS && fr->units != DBHIP_WIN_RANGE) || sk < DBHIP_WIN_UNBOUNDED_PRECEDING || sk > DBHIP_WIN_UNBOUNDED_FOLLOWING ||
             ek < DBHIP_WIN_UNBOUNDED_PRECEDING || ek > DBHIP_WIN_UNBOUNDED_FOLLOWING;
  bad = bad || (s_off && fr->start_offset < 0) || (e_off && fr->end_offset < 0);
  bad = bad || sk == DBHIP_WIN_UNBOUNDED_FOLLOWING || ek == DBHIP_WIN_UNBOUNDED_PRECEDING || sk > ek;
  bad = bad || (sk == DBHIP_WIN_PRECEDING && ek == DBHIP_WIN_PRECEDING && fr->start_offset < fr->end_offset);
  bad = bad || (sk == DBHIP_WIN_FOLLOWING && ek == DBHIP_WIN_FOLLOWING && fr->start_offset > fr->end_offset);
  if (bad) {
    set_error("%s: not a frame (units %d, start %d offset %lld, end %d offset %lld)", who, fr->units, sk, (long long)fr->start_offset, ek, (long long)fr->end_offset);
    return DBHIP_ERR_INVALID;
  }
  if (fr->units == DBHIP_WIN_RANGE && (s_off || e_off)) {
    set_error("%s: RANGE with an offset needs arithmetic on the order key: keep the CPU operator", who);
    return DBHIP_ERR_UNSUPPORTED;
  }
  *f = WinFrame{fr->units, sk, ek, 0, s_off ? (uint64_t)fr->start_offset : 0, e_off ? (uint64_t)fr->end_offset : 0};
  return DBHIP_OK;
}

WinArg win_arg(const dbhip_col* c) { return WinArg{c->data, c->validity, c->validity_offset, c->type, c->is_scalar}; }

// scratch of the scan: S [n] (when wanted) | C [n] (when wanted) | tile folds [nt]
template <int OP> struct ScanWs {
  typename WinOp<OP>::T* S;
  uint32_t* C;
  Seg<OP>* tsum;
  uint8_t* rest;     // `extra` more bytes
};
template <int OP> int32_t scan_ws(int64_t n, bool want_s, bool want_c, size_t extra, hipStream_t s, ScanWs<OP>* ws) {
  typedef typename WinOp<OP>::T T;
  const int64_t nt = ceil_div(n, WIN_TILE);
  const size_t s_bytes = want_s ? ((size_t)n * sizeof(T) + 31) & ~(size_t)31 : 0, c_bytes = want_c ? ((size_t)n * 4 + 31) & ~(size_t)31 : 0, t_bytes = (size_t)nt * sizeof(Seg<OP>);
  uint8_t* p = (uint8_t*)scratch(s_bytes + c_bytes + t_bytes + extra + 256, WIN_SCRATCH_SLOT, s);
  if (!p) return DBHIP_ERR_HIP;
  ws->S = want_s ? (T*)p : nullptr;
  ws->C = want_c ? (uint32_t*)(p + s_bytes) : nullptr;
  ws->tsum = (Seg<OP>*)(p + s_bytes + c_bytes);
  ws->rest = p + s_bytes + c_bytes + t_bytes;
  return DBHIP_OK;
}

// the three passes of the segmented scan
template <int OP, class LD>
int32_t run_scan(const LD& ld, const uint32_t* part_start, int64_t n, Seg<OP>* tsum, typename WinOp<OP>::T* S, uint32_t* C, uint32_t* over,
                 typename WinOp<OP>::T limit, hipStream_t s, const char* who) {
  const int64_t nt = ceil_div(n, WIN_TILE);
  const int al = al16_of(part_start);
  hipLaunchKernelGGL((win_scan_tiles_kernel<OP, LD>), dim3((unsigned)nt), dim3(256), 0, s, ld, part_start, n, al, tsum);
  DBHIP_POLL_CANCEL(s, who);
  hipLaunchKernelGGL((win_scan_carry_kernel<OP>), dim3(1), dim3(1024), 0, s, tsum, nt);
  DBHIP_POLL_CANCEL(s, who);
  hipLaunchKernelGGL((win_scan_apply_kernel<OP, LD>), dim3((unsigned)nt), dim3(256), 0, s, ld, part_start, n, al, (const Seg<OP>*)tsum, S, C, over, limit);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

template <int OP>
int32_t agg_by_scan(const dbhip_window_rows* rows, const WinFrame& f, const dbhip_col* arg, int out_type, void* out, uint8_t* out_validity, hipStream_t s) {
  const int64_t n = rows->n;
  ScanWs<OP> ws;
  int32_t rc = scan_ws<OP>(n, true, true, 0, s, &ws);
  if (rc) return rc;
  ArgLoader<OP> ld{win_arg(arg)};
  if ((rc = run_scan<OP, ArgLoader<OP>>(ld, rows->part_start, n, ws.tsum, ws.S, ws.C, nullptr, typename WinOp<OP>::T(), s, "dbhip_window_aggregate"))) return rc;
  DBHIP_POLL_CANCEL(s, "dbhip_window_aggregate");
  hipLaunchKernelGGL((win_resolve_kernel<OP>), dim3(win_grid(n)), dim3(256), 0, s, win_rows(rows), f, n, (const typename WinOp<OP>::T*)ws.S, (const uint32_t*)ws.C, 0, out,
                     out_type, out_validity);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

// the widest frame the bounds allow, in rows (saturating)
uint64_t frame_max_width(const WinFrame& f) {
  if (f.units == DBHIP_WIN_RANGE || f.sk == DBHIP_WIN_UNBOUNDED_PRECEDING || f.ek == DBHIP_WIN_UNBOUNDED_FOLLOWING) return ~0ULL;
  const uint64_t cap = 1ULL << 40;
  const uint64_t before = f.sk == DBHIP_WIN_PRECEDING ? (f.so < cap ? f.so : cap) : 0;
  const uint64_t after = f.ek == DBHIP_WIN_FOLLOWING ? (f.eo < cap ? f.eo : cap) : 0;
  return before + after + 1;
}

template <int OP>
int32_t agg_by_walk(const dbhip_window_rows* rows, const WinFrame& f, const dbhip_col* arg, int out_type, void* out, uint8_t* out_validity, hipStream_t s) {
  typedef typename WinOp<OP>::T T;
  const int64_t n = rows->n;
  ArgLoader<OP> ld{win_arg(arg)};
  T *p1v = nullptr, *p2v = nullptr;
  uint32_t *p1c = nullptr, *p2c = nullptr;
  if (frame_max_width(f) > 2 * WIN_P1) {     // frames that can be long: partials, so that a row costs at most ~1000 steps + n / 65536
    const int64_t n1 = ceil_div(n, WIN_P1), n2 = ceil_div(n1, 256);
    uint8_t* p = (uint8_t*)scratch((size_t)(n1 + n2) * (sizeof(T) + 4) + 256, WIN_SCRATCH_SLOT, s);
    if (!p) return DBHIP_ERR_HIP;
    p1v = (T*)p;
    p2v = p1v + n1;
    p1c = (uint32_t*)(p2v + n2);
    p2c = p1c + n1;
    hipLaunchKernelGGL((win_partial_kernel<OP>), dim3((unsigned)n1), dim3(256), 0, s, ld, (const T*)nullptr, (const uint32_t*)nullptr, n, p1v, p1c);
    DBHIP_POLL_CANCEL(s, "dbhip_window_aggregate");
    hipLaunchKernelGGL((win_partial_kernel<OP>), dim3((unsigned)n2), dim3(256), 0, s, ld, (const T*)p1v, (const uint32_t*)p1c, n1, p2v, p2c);
    DBHIP_POLL_CANCEL(s, "dbhip_window_aggregate");
  }
  hipLaunchKernelGGL((win_walk_kernel<OP>), dim3(win_grid(n)), dim3(256), 0, s, ld, win_rows(rows), f, n, (const T*)p1v, (const uint32_t*)p1c, (const T*)p2v,
                     (const uint32_t*)p2c, out, out_type, out_validity);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

template <int OP>
int32_t agg_dispatch(bool by_scan, const dbhip_window_rows* rows, const WinFrame& f, const dbhip_col* arg, int out_type, void* out, uint8_t* out_validity,
                     hipStream_t s) {
  return by_scan ? agg_by_scan<OP>(rows, f, arg, out_type, out, out_validity, s) : agg_by_walk<OP>(rows, f, arg, out_type, out, out_validity, s);
}

template <class V>
void launch_gather(hipStream_t s, const dbhip_window_rows* rows, int mode, int64_t offset, int vkind, uint64_t nth, const WinFrame& f, const dbhip_col* arg,
                   const dbhip_col* dflt, void* out, uint8_t* out_validity) {
  WinArg d{nullptr, nullptr, 0, 0, 0};
  if (dflt) d = win_arg(dflt);
  hipLaunchKernelGGL((win_gather_kernel<V>), dim3(win_grid(rows->n)), dim3(256), 0, s, win_rows(rows), rows->n, mode, offset, vkind, nth, f, win_arg(arg), d,
                     dflt ? 1 : 0, out, out_validity);
}

int32_t run_gather(hipStream_t s, const dbhip_window_rows* rows, int mode, int64_t offset, int vkind, uint64_t nth, const WinFrame& f, const dbhip_col* arg,
                   const dbhip_col* dflt, void* out, uint8_t* out_validity) {
  if (arg->type == DBHIP_T_BOOL) launch_gather<WinBit>(s, rows, mode, offset, vkind, nth, f, arg, dflt, out, out_validity);
  else switch (type_size(arg->type)) {
    case 1: launch_gather<uint8_t>(s, rows, mode, offset, vkind, nth, f, arg, dflt, out, out_validity); break;
    case 2: launch_gather<uint16_t>(s, rows, mode, offset, vkind, nth, f, arg, dflt, out, out_validity); break;
    case 4: launch_gather<uint32_t>(s, rows, mode, offset, vkind, nth, f, arg, dflt, out, out_validity); break;
    case 8: launch_gather<uint64_t>(s, rows, mode, offset, vkind, nth, f, arg, dflt, out, out_validity); break;
    case 16: launch_gather<uint4>(s, rows, mode, offset, vkind, nth, f, arg, dflt, out, out_validity); break;
    default: launch_gather<WinV32>(s, rows, mode, offset, vkind, nth, f, arg, dflt, out, out_validity); break;
  }
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

// the gather loads whole elements (16-byte halves of a Decimal256): the values must be aligned to that
bool win_values_aligned(const dbhip_col* c) {
  return c->type == DBHIP_T_BOOL || ((uintptr_t)c->data % (type_size(c->type) > 16 ? 16 : type_size(c->type))) == 0;
}

int32_t win_check_value_col(const dbhip_col* arg, const char* who) {
  if (!arg || !arg->data || arg->is_scalar || !((arg->type >= DBHIP_T_BOOL && arg->type <= DBHIP_T_DEC256))) {
    set_error("%s: the argument must be a column of a known type", who);
    return DBHIP_ERR_INVALID;
  }
  if (!win_values_aligned(arg)) {
    set_error("%s: the argument's values are not aligned to their width", who);
    return DBHIP_ERR_INVALID;
  }
  return DBHIP_OK;
}

}  // namespace

extern "C" {

int32_t dbhip_window_bounds(const dbhip_col* partition_keys, int32_t n_partition, const dbhip_col* order_keys, int32_t n_order, int64_t n,
                            dbhip_window_rows* rows, void* stream) {
  DBHIP_REQUIRE(n_partition >= 0 && n_partition <= 8 && n_order >= 0 && n_order <= 8, "dbhip_window_bounds: 0..8 partition keys and 0..8 order keys");
  DBHIP_REQUIRE((n_partition == 0 || partition_keys) && (n_order == 0 || order_keys) && rows, "dbhip_window_bounds: NULL argument");
  DBHIP_REQUIRE(n >= 0 && n <= WIN_MAX_ROWS, "dbhip_window_bounds: row count outside 0 .. 2^32 - 2");
  WinKeys keys;
  memset(&keys, 0, sizeof(keys));
  keys.n_part = n_partition;
  keys.n_all = n_partition + n_order;
  bool strings = false;
  for (int k = 0; k < keys.n_all; ++k) {
    const dbhip_col& c = k < n_partition ? partition_keys[k] : order_keys[k - n_partition];
    if (!(c.type >= DBHIP_T_BOOL && c.type <= DBHIP_T_STRING) || c.is_scalar) {
      set_error("dbhip_window_bounds: key %d has unsupported type %d or is a scalar (the key types of dbhip_sort_perm)", k, c.type);
      return DBHIP_ERR_UNSUPPORTED;
    }
    DBHIP_REQUIRE(c.data || n == 0, "dbhip_window_bounds: NULL key column");
    strings |= c.type == DBHIP_T_STRING;
    keys.k[k] = WinKey{c.data, c.validity, c.validity_offset, c.buffers, c.type, c.buffers && c.n_buffers > 0 ? c.n_buffers : 0};
  }
  rows->n = n;
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(rows->part_start && rows->part_end && rows->peer_start && rows->peer_end, "dbhip_window_bounds: a boundary array is NULL");
  hipStream_t s = resolve_stream(stream);
  const int64_t nt = ceil_div(n, WIN_TILE);
  const size_t flag_bytes = ((size_t)n + 31) & ~(size_t)31;
  uint8_t* ws = (uint8_t*)scratch(flag_bytes + (size_t)nt * sizeof(uint4) + 256, WIN_SCRATCH_SLOT, s);
  if (!ws) return DBHIP_ERR_HIP;
  uint8_t* flags = ws;
  uint4* tsum = (uint4*)(ws + flag_bytes);
  uint32_t* bad = (uint32_t*)(ws + flag_bytes + (size_t)nt * sizeof(uint4));
  DBHIP_CHECK(hipMemsetAsync(bad, 0, 4, s));
  hipLaunchKernelGGL(win_heads_kernel, dim3((unsigned)nt), dim3(256), 0, s, keys, n, flags, tsum, bad);
  DBHIP_POLL_CANCEL(s, "dbhip_window_bounds");
  hipLaunchKernelGGL(win_heads_carry_kernel, dim3(1), dim3(1024), 0, s, tsum, nt, (uint32_t)n);
  DBHIP_POLL_CANCEL(s, "dbhip_window_bounds");
  const int al = al16_of(rows->part_start) & al16_of(rows->part_end) & al16_of(rows->peer_start) & al16_of(rows->peer_end);
  hipLaunchKernelGGL(win_bounds_apply_kernel, dim3((unsigned)nt), dim3(256), 0, s, (const uint8_t*)flags, (const uint4*)tsum, n, rows->part_start, rows->part_end,
                     rows->peer_start, rows->peer_end, al);
  DBHIP_LAUNCH_CHECK();
  if (strings) {   // a value of more than 12 bytes in a column without data buffers cannot be compared: the kernel says so
    uint32_t h = 0;
    DBHIP_CHECK(hipMemcpyAsync(&h, bad, 4, hipMemcpyDeviceToHost, s));
    DBHIP_CHECK(hipStreamSynchronize(s));
    DBHIP_REQUIRE(!h, "dbhip_window_bounds: a string key holds a value longer than 12 bytes whose view names no data buffer of the column");
  }
  return DBHIP_OK;
}

int32_t dbhip_window_rank(const dbhip_window_rows* rows, int32_t kind, uint64_t buckets, void* out, void* stream) {
  int32_t rc = win_check_rows(rows, "dbhip_window_rank");
  if (rc) return rc;
  DBHIP_REQUIRE(kind >= DBHIP_WIN_ROW_NUMBER && kind <= DBHIP_WIN_NTILE, "dbhip_window_rank: unknown kind");
  DBHIP_REQUIRE(kind != DBHIP_WIN_NTILE || buckets >= 1, "dbhip_window_rank: ntile needs at least one bucket");
  const int64_t n = rows->n;
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(out, "dbhip_window_rank: NULL out");
  hipStream_t s = resolve_stream(stream);
  if (kind == DBHIP_WIN_DENSE_RANK) {     // peer groups begun in [part_start, i]: the segmented scan, written straight into `out`
    ScanWs<WOP_ADD_U64> ws;
    if ((rc = scan_ws<WOP_ADD_U64>(n, false, false, 0, s, &ws))) return rc;
    PeerHeadLoader ld{rows->peer_start};
    return run_scan<WOP_ADD_U64, PeerHeadLoader>(ld, rows->part_start, n, ws.tsum, (uint64_t*)out, nullptr, nullptr, 0, s, "dbhip_window_rank");
  }
  hipLaunchKernelGGL(win_rank_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, win_rows(rows), n, kind, buckets, out);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}

int32_t dbhip_window_shift(const dbhip_window_rows* rows, const dbhip_col* arg, int64_t offset, const dbhip_col* dflt, void* out,
                           uint8_t* out_validity, void* stream) {
  int32_t rc = win_check_rows(rows, "dbhip_window_shift");
  if (rc) return rc;
  if ((rc = win_check_value_col(arg, "dbhip_window_shift"))) return rc;
  if (dflt) {
    DBHIP_REQUIRE(dflt->data && dflt->type == arg->type, "dbhip_window_shift: the default must have the argument's type");
    if (arg->type == DBHIP_T_STRING) {
      set_error("dbhip_window_shift: a String default has its own data buffers: keep the CPU operator");
      return DBHIP_ERR_UNSUPPORTED;
    }
    DBHIP_REQUIRE(win_values_aligned(dflt), "dbhip_window_shift: the default's values are not aligned to their width");
  }
  if (rows->n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(out && out_validity, "dbhip_window_shift: out and out_validity are required");
  return run_gather(resolve_stream(stream), rows, WIN_GATHER_SHIFT, offset, 0, 0, WinFrame{0, 0, 0, 0, 0, 0}, arg, dflt, out, out_validity);
}

int32_t dbhip_window_value(const dbhip_window_rows* rows, int32_t kind, int64_t nth, const dbhip_col* arg, const dbhip_window_frame* frame, void* out,
                           uint8_t* out_validity, void* stream) {
  int32_t rc = win_check_rows(rows, "dbhip_window_value");
  if (rc) return rc;
  DBHIP_REQUIRE(kind >= DBHIP_WIN_FIRST_VALUE && kind <= DBHIP_WIN_NTH_VALUE, "dbhip_window_value: unknown kind");
  DBHIP_REQUIRE(kind != DBHIP_WIN_NTH_VALUE || nth >= 1, "dbhip_window_value: nth_value counts from 1");
  if ((rc = win_check_value_col(arg, "dbhip_window_value"))) return rc;
  WinFrame f;
  if ((rc = win_check_frame(frame, "dbhip_window_value", &f))) return rc;
  if (rows->n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(out && out_validity, "dbhip_window_value: out and out_validity are required");
  return run_gather(resolve_stream(stream), rows, WIN_GATHER_VALUE, 0, kind, kind == DBHIP_WIN_NTH_VALUE ? (uint64_t)nth : 1, f, arg, nullptr, out, out_validity);
}

int32_t dbhip_window_aggregate(const dbhip_window_rows* rows, const dbhip_agg_desc* agg, const dbhip_col* arg, const dbhip_window_frame* frame, void* out,
                               uint8_t* out_validity, void* stream) {
  const char* who = "dbhip_window_aggregate";
  int32_t rc = win_check_rows(rows, who);
  if (rc) return rc;
  DBHIP_REQUIRE(agg && agg->kind >= DBHIP_AGG_COUNT && agg->kind <= DBHIP_AGG_MAX, "dbhip_window_aggregate: NULL or unknown aggregate");
  WinFrame f;
  if ((rc = win_check_frame(frame, who, &f))) return rc;
  DBHIP_REQUIRE(agg->kind == DBHIP_AGG_COUNT || arg, "dbhip_window_aggregate: sum / min / max need an argument");
  DBHIP_REQUIRE(!arg || (arg->data && !arg->is_scalar && arg->type >= DBHIP_T_BOOL && arg->type <= DBHIP_T_DEC256), "dbhip_window_aggregate: the argument must be a column of a known type");
  DBHIP_REQUIRE(!arg || agg->kind == DBHIP_AGG_COUNT || arg->type == agg->arg_type, "dbhip_window_aggregate: agg->arg_type is not the argument's type");
  const int t = arg ? arg->type : 0;
  const int64_t n = rows->n;
  // what runs, decided before anything is launched: a refused shape leaves the stream as it was
  int op = -1, out_type = DBHIP_T_U64;
  if (agg->kind == DBHIP_AGG_SUM) {
    switch (t) {
      case DBHIP_T_I8: case DBHIP_T_I16: case DBHIP_T_I32: case DBHIP_T_I64: op = WOP_ADD_U64; out_type = DBHIP_T_I64; break;
      case DBHIP_T_U8: case DBHIP_T_U16: case DBHIP_T_U32: case DBHIP_T_U64: op = WOP_ADD_U64; out_type = DBHIP_T_U64; break;
      case DBHIP_T_DEC64: op = WOP_ADD_U64; out_type = DBHIP_T_DEC64; break;
      case DBHIP_T_F32: case DBHIP_T_F64: op = WOP_ADD_F64; out_type = DBHIP_T_F64; break;
      case DBHIP_T_DEC128: op = WOP_ADD_U128; out_type = DBHIP_T_DEC128; break;
    }
    if (op < 0) { set_error("dbhip_window_aggregate: sum over type %d: keep the CPU operator", t); return DBHIP_ERR_UNSUPPORTED; }
  } else if (agg->kind != DBHIP_AGG_COUNT) {
    const bool mx = agg->kind == DBHIP_AGG_MAX;
    out_type = t;
    switch (t) {
      case DBHIP_T_I8: case DBHIP_T_I16: case DBHIP_T_I32: case DBHIP_T_I64: case DBHIP_T_DATE: case DBHIP_T_TIMESTAMP: case DBHIP_T_DEC64:
        op = mx ? WOP_MAX_I64 : WOP_MIN_I64; break;
      case DBHIP_T_U8: case DBHIP_T_U16: case DBHIP_T_U32: case DBHIP_T_U64: op = mx ? WOP_MAX_U64 : WOP_MIN_U64; break;
      case DBHIP_T_F32: case DBHIP_T_F64: op = mx ? WOP_MAX_F64 : WOP_MIN_F64; break;
      case DBHIP_T_DEC128: op = mx ? WOP_MAX_I128 : WOP_MIN_I128; break;
    }
    if (op < 0) { set_error("dbhip_window_aggregate: min / max over type %d: keep the CPU operator", t); return DBHIP_ERR_UNSUPPORTED; }
  }
  if (op >= 0 && type_size(t) > 1 && ((uintptr_t)arg->data % (type_size(t) > 8 ? 8 : type_size(t))) != 0) {
    set_error("dbhip_window_aggregate: the argument's values are not aligned to their width");
    return DBHIP_ERR_INVALID;
  }
  if (n == 0) return DBHIP_OK;
  DBHIP_REQUIRE(out && out_validity, "dbhip_window_aggregate: out and out_validity are required");
  hipStream_t s = resolve_stream(stream);
  if (agg->kind == DBHIP_AGG_COUNT) {
    if (!arg) {
      hipLaunchKernelGGL(win_count_star_kernel, dim3(win_grid(n)), dim3(256), 0, s, win_rows(rows), f, n, (uint64_t*)out, out_validity);
      DBHIP_LAUNCH_CHECK();
      return DBHIP_OK;
    }
    ScanWs<WOP_ADD_U64> ws;
    if ((rc = scan_ws<WOP_ADD_U64>(n, false, true, 0, s, &ws))) return rc;
    ValidLoader ld{win_arg(arg)};
    if ((rc = run_scan<WOP_ADD_U64, ValidLoader>(ld, rows->part_start, n, ws.tsum, nullptr, ws.C, nullptr, 0, s, who))) return rc;
    DBHIP_POLL_CANCEL(s, who);
    hipLaunchKernelGGL((win_resolve_kernel<WOP_ADD_U64>), dim3(win_grid(n)), dim3(256), 0, s, win_rows(rows), f, n, (const uint64_t*)nullptr, (const uint32_t*)ws.C, 1, out,
                       DBHIP_T_U64, out_validity);
    DBHIP_LAUNCH_CHECK();
    return DBHIP_OK;
  }
  if (op == WOP_ADD_U128 && agg->arg_precision > 18) {
    // no prefix and no frame can leave +-(10^38 - 1) when the sum of |x| of every partition stays inside it
    ScanWs<WOP_SAT_U128> ws;
    if ((rc = scan_ws<WOP_SAT_U128>(n, false, false, 64, s, &ws))) return rc;
    uint32_t* over = (uint32_t*)ws.rest;
    DBHIP_CHECK(hipMemsetAsync(over, 0, 4, s));
    ArgLoader<WOP_SAT_U128> ld{win_arg(arg)};
    u128 limit = 1;
    for (int k = 0; k < 38; ++k) limit *= 10;
    limit -= 1;
    if ((rc = run_scan<WOP_SAT_U128, ArgLoader<WOP_SAT_U128>>(ld, rows->part_start, n, ws.tsum, nullptr, nullptr, over, limit, s, who))) return rc;
    uint32_t h = 0;
    DBHIP_CHECK(hipMemcpyAsync(&h, over, 4, hipMemcpyDeviceToHost, s));
    DBHIP_CHECK(hipStreamSynchronize(s));
    if (h) {
      set_error("dbhip_window_aggregate: the sum of |x| of a partition exceeds 10^38 - 1: the CPU operator raises the overflow itself");
      return DBHIP_ERR_UNSUPPORTED;
    }
  }
  // wrapping sums are differences of two scan entries; everything else is read from the scan only when the frame starts with its partition
  const bool by_scan = f.sk == DBHIP_WIN_UNBOUNDED_PRECEDING || op == WOP_ADD_U64 || op == WOP_ADD_U128;
  switch (op) {
    case WOP_ADD_U64: return agg_by_scan<WOP_ADD_U64>(rows, f, arg, out_type, out, out_validity, s);
    case WOP_ADD_F64: return agg_dispatch<WOP_ADD_F64>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    case WOP_ADD_U128: return agg_by_scan<WOP_ADD_U128>(rows, f, arg, out_type, out, out_validity, s);
    case WOP_MIN_I64: return agg_dispatch<WOP_MIN_I64>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    case WOP_MAX_I64: return agg_dispatch<WOP_MAX_I64>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    case WOP_MIN_U64: return agg_dispatch<WOP_MIN_U64>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    case WOP_MAX_U64: return agg_dispatch<WOP_MAX_U64>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    case WOP_MIN_F64: return agg_dispatch<WOP_MIN_F64>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    case WOP_MAX_F64: return agg_dispatch<WOP_MAX_F64>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    case WOP_MIN_I128: return agg_dispatch<WOP_MIN_I128>(by_scan, rows, f, arg, out_type, out, out_validity, s);
    default: return agg_dispatch<WOP_MAX_I128>(by_scan, rows, f, arg, out_type, out, out_validity, s);
  }
}

}  // extern "C"
