// dev_longrows.h — the long-row list of the two-tier kernels (k_like.hip, k_strfn.hip, k_strsearch.hip, k_array.hip).
//
// Pass 1 has one lane per row and does not walk a long row: the row's id goes into a list in scratch (one ballot and one atomic add per
// wave, list_rows) and its output is written as zero. Pass 2 runs one wave per listed row on a fixed grid and reads the list's length on
// the device (long_walk), so the host never waits for the count. Scratch: a head of LONGROWS_HEAD_BYTES that is cleared before pass 1
// (the counts of up to two lists, and 8 bytes a caller may use for a sum of its own) | up to byte 64 | row ids (long_list_bytes); a call
// with two lists gives each its own row ids (long_list_at).
// HIP only: not for the headers the host checkers compile, and not embedded for the run-time specialised kernels (the Makefile's JIT_HDRS).
#pragma once
#include "runtime.h"

constexpr int LONGROWS_PASS2_BLOCKS = 512;        // fixed grid of the wave-per-row passes: 2,048 waves that stride over the list
constexpr int64_t LONGROWS_MAX_ROWS = 0xFFFFFFFELL;   // a row id in the list is 32 bits wide
constexpr size_t LONGROWS_HEAD_BYTES = 16;        // what long_list_clear zeroes: two counts and a caller's 8 bytes
constexpr size_t LONGROWS_IDS_OFF = 64;           // where the row ids start when the scratch block holds the list alone

struct LongList {
  uint32_t* count;
  uint32_t* rows;
};

__device__ __forceinline__ uint64_t lanes_below(uint32_t lane) { return (1ull << lane) - 1ull; }

// one ballot and one atomic add per wave: the listed lanes' rows go into the list
__device__ __forceinline__ void list_rows(bool listed, uint32_t lane, int64_t i, const LongList& L) {
  const uint64_t lmask = __ballot(listed);
  if (lmask) {                                // wave-uniform
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(L.count, (uint32_t)__popcll(lmask));
    at = __shfl(at, 0, 64);
    if (listed) L.rows[at + (uint32_t)__popcll(lmask & lanes_below(lane))] = (uint32_t)i;
  }
}

// pass 2, 256 threads: for (uint32_t q = w.first; q < w.count; q += w.stride) row = L.rows[q];
struct LongWalk { uint32_t count, stride, first; };
__device__ __forceinline__ LongWalk long_walk(const LongList& L) {
  LongWalk w;
  w.count = *L.count;
  w.stride = gridDim.x * 4;
  w.first = blockIdx.x * 4 + (threadIdx.x >> 6);
  return w;
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------
inline size_t long_list_bytes(int64_t n) { return LONGROWS_IDS_OFF + (size_t)n * 4 + 64; }
// list `which` (0, 1) of the scratch block ws, its row ids at ids_off
inline LongList long_list_at(uint8_t* ws, int which = 0, size_t ids_off = LONGROWS_IDS_OFF) {
  return LongList{(uint32_t*)ws + which, (uint32_t*)(ws + ids_off)};
}
inline hipError_t long_list_clear(uint8_t* ws, hipStream_t s) { return hipMemsetAsync(ws, 0, LONGROWS_HEAD_BYTES, s); }
template <class K, class Params>
inline void long_launch(K long_kernel, const Params& P, hipStream_t s) {
  hipLaunchKernelGGL(long_kernel, dim3(LONGROWS_PASS2_BLOCKS), dim3(256), 0, s, P);
}
// pass 1 and the wave-per-row pass over its list; Params has n and the LongList `list`
template <class Params, class K1, class K2>
inline int32_t long_two_passes(Params& P, K1 rows_kernel, K2 long_kernel, int slot, hipStream_t s, const char* who) {
  uint8_t* ws = (uint8_t*)dbhip::scratch(long_list_bytes(P.n), slot, s);
  if (!ws) return DBHIP_ERR_HIP;
  P.list = long_list_at(ws);
  DBHIP_CHECK(long_list_clear(ws, s));
  hipLaunchKernelGGL(rows_kernel, dim3(dbhip::grid_for(P.n, 256)), dim3(256), 0, s, P);
  DBHIP_LAUNCH_CHECK();
  DBHIP_POLL_CANCEL(s, who);
  long_launch(long_kernel, P, s);
  DBHIP_LAUNCH_CHECK();
  return DBHIP_OK;
}
