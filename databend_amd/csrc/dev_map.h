// dev_map.h — the row-run map shared by the element-wise kernels (k_math.hip, k_datetime.hip; k_inlist.hip uses the loader).
//
// Each lane owns a run of CONSECUTIVE rows sized so that the narrower of input and output moves as whole 16-byte vectors (MapRun).
// The last n mod rows-per-lane rows are done one per lane by the first workgroup. A scalar source is splatted. Every access has a
// 16-byte form and a per-element form. `vec` says which: a bool the caller computes from the kernel arguments alone (so the choice
// is wave-uniform), or std::true_type() from a kernel whose entry point insists on 16-byte bases, which has no other form compiled.
// Not embedded for the run-time specialised kernels (the Makefile's JIT_HDRS): nothing here is part of their text or their cache key.
#pragma once
#include <type_traits>

#include "dev_load.h"
#include "runtime.h"

template <typename T> using Vec16 = VecT<T, 16 / sizeof(T)>;
// Beside a per-element branch the 16-byte access is ONE load or store of a vector type. A copy of a Vec16 is split into element
// accesses, which the compiler finds again in the per-element branch: it merges the two branches, keeps the weaker alignment and
// emits dwordx3 + dword pairs or element stores where dwordx4 was meant (abs(Int32) then takes 1.4 times as long).
typedef uint32_t MapQuad __attribute__((ext_vector_type(4)));
template <typename Vec> constexpr bool kMapAlways16 = std::is_same<Vec, std::true_type>::value;

// one value from an address aligned to the element; a 16-byte value as two 8-byte words (a Decimal128 column need only be 8-byte
// aligned)
template <typename T>
__device__ __forceinline__ T map_load_one(const void* base, int64_t i) {
  if constexpr (sizeof(T) == 16) {
    const uint64_t* p = (const uint64_t*)base + 2 * i;
    const uint64_t w[2] = {p[0], p[1]};
    T v;
    __builtin_memcpy(&v, w, 16);
    return v;
  } else {
    return ((const T*)base)[i];
  }
}
template <typename T>
__device__ __forceinline__ void map_store_one(void* base, int64_t i, T v) {
  if constexpr (sizeof(T) == 16) {
    uint64_t* p = (uint64_t*)base + 2 * i;
    uint64_t w[2];
    __builtin_memcpy(w, &v, 16);
    p[0] = w[0];
    p[1] = w[1];
  } else {
    ((T*)base)[i] = v;
  }
}

// ROWS consecutive values from row `first`: 16-byte accesses when `vec` (the base is 16-byte aligned; first * sizeof(T) is a multiple
// of 16 by the choice of ROWS), element accesses otherwise
template <typename T, int ROWS, typename Vec>
__device__ __forceinline__ void map_load(const void* base, Vec vec, int64_t first, T (&v)[ROWS]) {
  constexpr int PER = 16 / sizeof(T);
  static_assert(ROWS % PER == 0, "whole 16-byte vectors");
  if constexpr (kMapAlways16<Vec>) {
    const Vec16<T>* p = (const Vec16<T>*)((const T*)base + first);
#pragma unroll
    for (int q = 0; q < ROWS / PER; ++q) {
      const Vec16<T> t = p[q];
#pragma unroll
      for (int k = 0; k < PER; ++k) v[q * PER + k] = t.v[k];
    }
  } else if (vec) {
    const MapQuad* p = (const MapQuad*)((const T*)base + first);
#pragma unroll
    for (int q = 0; q < ROWS / PER; ++q) {
      const MapQuad t = p[q];
      __builtin_memcpy(&v[q * PER], &t, 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < ROWS; ++k) v[k] = map_load_one<T>(base, first + k);
  }
}
template <typename T, int ROWS, typename Vec>
__device__ __forceinline__ void map_store(void* base, Vec vec, int64_t first, const T (&v)[ROWS]) {
  constexpr int PER = 16 / sizeof(T);
  static_assert(ROWS % PER == 0, "whole 16-byte vectors");
  if constexpr (kMapAlways16<Vec>) {
    Vec16<T>* p = (Vec16<T>*)((T*)base + first);
#pragma unroll
    for (int q = 0; q < ROWS / PER; ++q) {
      Vec16<T> t;
#pragma unroll
      for (int k = 0; k < PER; ++k) t.v[k] = v[q * PER + k];
      p[q] = t;
    }
  } else if (vec) {
    MapQuad* p = (MapQuad*)((T*)base + first);
#pragma unroll
    for (int q = 0; q < ROWS / PER; ++q) {
      MapQuad t;
      __builtin_memcpy(&t, &v[q * PER], 16);
      p[q] = t;
    }
  } else {
#pragma unroll
    for (int k = 0; k < ROWS; ++k) map_store_one<T>(base, first + k, v[k]);
  }
}

// an operand's ROWS values: a scalar column's one value ROWS times, a full column's run
template <typename T, int ROWS, typename Vec>
__device__ __forceinline__ void map_fetch(const void* base, Vec vec, bool scalar, int64_t first, T (&v)[ROWS]) {
  if (scalar) {
    const T s = map_load_one<T>(base, 0);
#pragma unroll
    for (int k = 0; k < ROWS; ++k) v[k] = s;
  } else {
    map_load<T, ROWS>(base, vec, first, v);
  }
}

template <typename In, typename Out>
struct MapRun {
  static constexpr int kRows = 16 / (int)(sizeof(In) < sizeof(Out) ? sizeof(In) : sizeof(Out));
};

// out[i] = f(in[i]) for i < n: a grid-stride loop over the runs, 256 lanes per workgroup (launch with map_grid)
template <typename In, typename Out, typename VecIn, typename VecOut, typename F>
__device__ __forceinline__ void map_rows(const void* in, VecIn in_vec, bool scalar, void* out, VecOut out_vec, int64_t n, F f) {
  constexpr int ROWS = MapRun<In, Out>::kRows;
  const int64_t groups = n / ROWS;
  // a scalar source is read once, before the loop: with map_fetch inside the loop the 16-row kernels of an 8-byte source and a 1-byte
  // result (k_math.hip's SignOp) compiled to 70 VGPRs instead of 42 - 44 and lost a wave of occupancy
  In s = In();
  if (scalar) s = map_load_one<In>(in, 0);
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
    In v[ROWS];
    Out r[ROWS];
    if (scalar) {
#pragma unroll
      for (int k = 0; k < ROWS; ++k) v[k] = s;
    } else {
      map_load<In, ROWS>(in, in_vec, g * ROWS, v);
    }
#pragma unroll
    for (int k = 0; k < ROWS; ++k) r[k] = f(v[k]);
    map_store<Out, ROWS>(out, out_vec, g * ROWS, r);
  }
  // the last n mod ROWS rows, one per lane
  const int64_t i = groups * ROWS + threadIdx.x;
  if (blockIdx.x == 0 && i < n) map_store_one<Out>(out, i, f(scalar ? s : map_load_one<In>(in, i)));
}

template <typename In, typename Out>
inline int map_grid(int64_t n) {
  return dbhip::grid_for(n / MapRun<In, Out>::kRows, 256);
}
