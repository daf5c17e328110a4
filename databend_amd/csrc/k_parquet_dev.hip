// k_parquet_dev.hip — scan side, DEVICE mode: the page payload of a Parquet column chunk never passes through
// the host.
//
// Stands where the reference hands a block's raw column chunks to arrow-rs (column_chunks_to_record_batch,
// src/query/storages/fuse/src/io/read/block/parquet/deserialize.rs:33-81, then block_reader_parquet_deserialize.rs) — the same
// boundary as k_parquet.hip, whose open() walks run headers, length prefixes and (for compressed chunks) decompresses every page
// on the CPU. Here the host reads the thrift PAGE HEADERS only (a few dozen bytes per page: sizes, value counts, encodings) and
// uploads that page table; everything that touches payload bytes runs on the GPU from the HBM copy of the chunk as stored:
//   dv_inflate_lz_kernel   one wave per page: Snappy raw format (google/snappy format_description.txt) or LZ4 block format
//                       (lz4_Block_format.md) -> the decompressed IMAGE in HBM. The sequence stream is inherently serial: the wave
//                       parses it on the scalar unit from register-held chunks of the payload (dv_wave.h), the 64 lanes move literal
//                       and match bytes through a 16 KiB LDS ring (a short literal and the match behind it in ONE LDS round trip),
//                       references that reach further back read the image; the ring is written to HBM with 16-byte stores.
//   dv_levels_kernel    one workgroup per data page of a nullable column: the RLE / bit-packed hybrid walk of the definition
//                       levels (Encodings.md "RLE/bit-packing hybrid") -> validity bits at the page's rows + the page's count
//                       of non-null values.
//   dv_scan_kernel      exclusive scan of those counts: where each page's values start among the non-null values.
//   dv_dict_kernel      the dictionary page -> dictionary in the output type (PLAIN; BYTE_ARRAY: the length-prefix chain).
//   dv_values_kernel    one workgroup per data page: PLAIN (fixed width, BOOLEAN bits, BYTE_ARRAY length chain -> 16-byte views
//                       that point into the image), PLAIN_DICTIONARY / RLE_DICTIONARY (hybrid walk of the indices + gather), RLE
//                       booleans, DELTA_BINARY_PACKED (INT32 / INT64: block / miniblock walk, workgroup prefix sum of the deltas).
//   dv_values_ext_kernel BYTE_STREAM_SPLIT, DELTA_LENGTH_BYTE_ARRAY (views into the image), DELTA_BYTE_ARRAY (views into the chunk's
//                       arena, which dv_dba_size_kernel sizes and dv_dba_replay_kernel fills) — launched only for batches with such pages.
//   pq_popc / scan / pq_spread (pq_common.h)   nullable columns: dense values -> rows.
// Nothing is validated on the host beyond the page table, so every device access is checked against the page payload, the
// dictionary and the output size; the first violation is recorded in a device word and decode returns DBHIP_ERR_INVALID.
//   dv_inflate_zstd2_kernel  ZSTD (the reference's DEFAULT codec, table_compression.rs:27-28): two waves per page — one walks the frame
//                       with zstd_core.h (Huffman literals by up to four lanes, FSE sequences from a look-ahead window in registers) and
//                       queues commands, the other replays them through a 4 KiB LDS ring + far references from the image: dv_wave.h.
// Nested leaves (dbhip_pq_chunk_open_device_nested): dv_levels_kernel<true> leaves every level entry's (r, d) as bytes, pq_nest_count_kernel
// counts the slots each 32-entry word opens in every index space, one scan per space, and pq_nest_finish_kernel writes every node's offsets and
// validity and moves the leaf values to their slots.
// dbhip_pq_chunks_decode_device decodes MANY chunks with one launch set (one inflate launch per codec family over all their pages, one
// levels / scan / dictionary / values launch over all their data pages, one read-back): a scan keeps dozens of column chunks in flight.
#include "pq_common.h"

#include <stdlib.h>
#include "dv_wave.h"

namespace {

enum { DV_OK = 0, DV_CORRUPT = 1, DV_UNSUPPORTED = 2 };
enum { ENC_DELTA_BINARY_PACKED = 5, ENC_DELTA_LENGTH_BYTE_ARRAY = 6, ENC_DELTA_BYTE_ARRAY = 7, ENC_BYTE_STREAM_SPLIT = 9 };
// the encodings dv_values_ext_kernel decodes (dv_values_kernel never sees their pages)
__host__ __device__ __forceinline__ bool dv_ext_enc(uint32_t e) {
  return e == ENC_DELTA_LENGTH_BYTE_ARRAY || e == ENC_DELTA_BYTE_ARRAY || e == ENC_BYTE_STREAM_SPLIT;
}
enum { CODEC_NONE = 0, CODEC_SNAPPY = 1, CODEC_ZSTD = 6, CODEC_LZ4_RAW = 7 };
enum { PQ_NODE_LIST = 1, PQ_NODE_STRUCT = 2 };   // dbhip_pq_node.kind
// bits of a level whose largest value is v (parquet's bit width of the level streams)
inline uint32_t bit_width_u32(uint32_t v) { uint32_t b = 0; for (; v; v >>= 1) ++b; return b; }

__device__ __forceinline__ void dv_fail(uint32_t* ctl, uint32_t code) { atomicCAS(&ctl[0], 0u, code); }

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// ---------------------------------------------------------------------------------------------
// page decompression (dv_wave.h)
// ---------------------------------------------------------------------------------------------
// ZSTD, two waves per page: wave 0 parses (ZProd), wave 1 copies (dv_wave.h)
__global__ __launch_bounds__(128) void dv_inflate_zstd2_kernel(const DvJob* __restrict__ jobs, uint32_t ring) {
  extern __shared__ __align__(16) uint8_t dv_lds[];
  const DvJob P = jobs[blockIdx.x];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t lev = P.lev_len;
  const uint32_t raw = P.compressed ? lev : P.uncomp_len;
  for (uint32_t i = threadIdx.x; i < raw; i += 128) P.dst[i] = P.src[i];
  if (!P.compressed || P.uncomp_len == lev) return;
  ZQueue Q;
  Q.slots = (u32x4q*)(dv_lds + ring + ZW_TABLES);
  Q.ctl = (uint32_t*)(dv_lds + ring + ZW_TABLES + ZQ_CAP * 16);
  if (threadIdx.x < 4) Q.ctl[threadIdx.x] = 0;
  __syncthreads();
  if (wave == 0) {
    ZProd a;
    a.begin(P, dv_lds, ring, lane);
    a.qbegin(Q);
    int rc = zc::decode_frames(a, a.in_len);
    if (rc == zc::OK && a.op_ != a.cap_) rc = zc::CORRUPT_;
    a.end((uint32_t)rc);
  } else {
    ZWave b;
    b.begin(P, dv_lds, ring, lane);
    const int rc = (int)zq_consume(b, Q);
    b.flush(true);
    if (rc) dv_fail(P.ctl, rc == zc::UNSUPPORTED ? DV_UNSUPPORTED : DV_CORRUPT);
  }
}

// LZ4 / Snappy on the same wave (16 KiB ring, the payload as one forward stream in registers)
__global__ __launch_bounds__(64) void dv_inflate_lz_kernel(const DvJob* __restrict__ jobs, uint32_t ring) {
  extern __shared__ __align__(16) uint8_t dv_lds[];
  const DvJob P = jobs[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  const uint32_t lev = P.lev_len;
  const uint32_t raw = P.compressed ? lev : P.uncomp_len;
  for (uint32_t i = lane; i < raw; i += 64) P.dst[i] = P.src[i];
  if (!P.compressed || P.uncomp_len == lev) return;
  ZWave w;
  w.begin(P, dv_lds, ring, lane);
  FwdStream in;
  in.open(w.srcA, w.safeA, w.a0, lane);
  bool ok = P.codec == CODEC_SNAPPY ? snappy_raw(w, in) : lz4_block(w, in);
  if (ok && w.op_ != w.cap_) ok = false;
  w.flush(true);
  if (!ok) dv_fail(P.ctl, DV_CORRUPT);
}

// ---------------------------------------------------------------------------------------------
// RLE / bit-packed hybrid streams, walked by a whole workgroup (every thread follows the same headers)
// ---------------------------------------------------------------------------------------------
// up to 8 bytes at s[pos ..) as a little-endian word; bytes at or past `len` read as 0
__device__ __forceinline__ uint64_t dv_peek8(const uint8_t* __restrict__ s, uint32_t pos, uint32_t len) {
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (pos + (uint32_t)k < len) v |= (uint64_t)s[pos + k] << (8 * k);
  return v;
}

// varint at s[*pos ..): false when it runs past `len` or does not end within 10 bytes
__device__ __forceinline__ bool dv_varint(const uint8_t* __restrict__ s, uint32_t* pos, uint32_t len, uint64_t* out) {
  const uint64_t w = dv_peek8(s, *pos, len);
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) {
    if (*pos + (uint32_t)k >= len) return false;
    const uint32_t b = (uint32_t)(w >> (8 * k)) & 0xFFu;
    v |= (uint64_t)(b & 0x7F) << (7 * k);
    if (!(b & 0x80)) { *pos += (uint32_t)k + 1; *out = v; return true; }
  }
  // bytes 9 and 10 (a zigzag 64-bit first value / min delta)
  for (int k = 8; k < 10; ++k) {
    if (*pos + (uint32_t)k >= len) return false;
    const uint32_t b = s[*pos + k];
    v |= (uint64_t)(b & 0x7F) << (7 * k);
    if (!(b & 0x80)) { *pos += (uint32_t)k + 1; *out = v; return true; }
  }
  return false;
}

// rle(first, n, value) / bp(first, n, packed bytes): called by every thread of the workgroup with the same arguments
template <class Rle, class Bp>
__device__ __forceinline__ bool dv_walk_hybrid(const uint8_t* __restrict__ s, uint32_t len, int bitw, uint32_t nvals, Rle&& rle, Bp&& bp) {
  uint32_t pos = 0, done = 0;
  const uint32_t vbytes = (uint32_t)(bitw + 7) >> 3;
  while (done < nvals) {
    uint64_t h;
    if (!dv_varint(s, &pos, len, &h)) return false;
    const uint32_t avail = len - pos;
    if (h & 1) {
      const uint64_t groups = h >> 1;
      if (groups == 0 || groups > 0x1FFFFFFFull) return false;
      uint64_t n64 = groups * 8;
      const uint32_t n = n64 > (uint64_t)(nvals - done) ? nvals - done : (uint32_t)n64;
      if ((uint64_t)n * (uint64_t)bitw > (uint64_t)avail * 8) return false;  // the bytes present cover the n values that are expanded
      bp(done, n, s + pos);
      const uint64_t bytes = groups * (uint64_t)bitw;
      pos += bytes < (uint64_t)avail ? (uint32_t)bytes : avail;
      done += n;
    } else {
      const uint64_t n64 = h >> 1;
      if (n64 == 0 || avail < vbytes) return false;
      const uint64_t w = dv_peek8(s, pos, len);
      const uint64_t v = vbytes >= 8 ? w : (w & ((1ull << (8 * vbytes)) - 1));
      pos += vbytes;
      if (bitw < 64 && (v >> bitw) != 0) return false;
      const uint32_t n = n64 > (uint64_t)(nvals - done) ? nvals - done : (uint32_t)n64;
      rle(done, n, (uint32_t)v);
      done += n;
    }
  }
  return true;
}

// The same walk by ONE WAVE over streams staged in LDS, with the run headers read out of a 256-byte register window (lane l = dword l,
// v_readlane: scalar results, no memory round trip per header — the chain header -> next header is what a List page's thousands of
// short runs wait for). Positions are byte offsets from the start of the staged region.
struct LvWin {
  const uint8_t* sA;     // 4-byte aligned LDS address at or below the staged bytes
  uint32_t a0, lim;      // first staged byte - sA; bytes readable from sA (a multiple of 4)
  uint32_t wlo, w, lane;
  __device__ __forceinline__ void slide(uint32_t wl) {
    wlo = rfl(wl);
    const uint32_t o = wlo + 4 * lane;
    w = *(const __attribute__((address_space(3))) uint32_t*)(uintptr_t)(sA + (o + 4 <= lim ? o : lim - 4));
  }
  __device__ __forceinline__ void open(const uint8_t* s, const uint8_t* end, uint32_t ln) {
    a0 = (uint32_t)((uintptr_t)s & 3u); sA = s - a0; lim = (uint32_t)(end - sA) & ~3u; lane = ln;
    slide(0);
  }
  __device__ __forceinline__ uint64_t u64(uint32_t pos) {
    const uint32_t a = rfl(pos + a0);
    if (a < wlo || a + 8 > wlo + 256) slide(a & ~3u);
    const uint32_t i = (a - wlo) >> 2;
    const uint32_t d0 = rdl(w, i), d1 = rdl(w, i + 1), d2 = rdl(w, i + 2 < 64 ? i + 2 : 63);
    const uint64_t lo = (uint64_t)d0 | ((uint64_t)d1 << 32);
    const uint32_t sft = 8 * (a & 3);
    return sft ? (lo >> sft) | ((uint64_t)d2 << (64 - sft)) : lo;
  }
};

// the stream is the `len` bytes at offset `at` of the staged region (whose bytes are at `base`); bit width <= 8
template <class Rle, class Bp>
__device__ __forceinline__ bool dv_walk_hybrid_wave(LvWin& W, const uint8_t* base, uint32_t at, uint32_t len, int bitw, uint32_t nvals, Rle&& rle, Bp&& bp) {
  uint32_t pos = 0, done = 0;
  while (done < nvals) {
    if (pos >= len) return false;
    const uint64_t h8 = W.u64(at + pos);
    uint64_t h;
    uint32_t used;
    if (!(h8 & 0x80u)) { h = h8 & 0x7F; used = 1; }
    else if (!(h8 & 0x8000u)) { h = (h8 & 0x7F) | ((h8 >> 1) & 0x3F80); used = 2; }
    else if (!(h8 & 0x800000u)) { h = (h8 & 0x7F) | ((h8 >> 1) & 0x3F80) | ((h8 >> 2) & 0x1FC000); used = 3; }
    else {
      h = 0; used = 0;
      for (uint32_t k = 0; k < 10; ++k) {
        if (pos + k >= len) return false;
        const uint32_t b = (uint32_t)W.u64(at + pos + k) & 0xFFu;
        h |= (uint64_t)(b & 0x7F) << (7 * k);
        if (!(b & 0x80)) { used = k + 1; break; }
      }
      if (used == 0) return false;
    }
    if (used > len - pos) return false;
    pos = rfl(pos + used);
    const uint32_t avail = len - pos;
    if (h & 1) {
      const uint64_t groups = h >> 1;
      if (groups == 0 || groups > 0x1FFFFFFFull) return false;
      const uint64_t n64 = groups * 8;
      const uint32_t n = n64 > (uint64_t)(nvals - done) ? nvals - done : (uint32_t)n64;
      if ((uint64_t)n * (uint64_t)bitw > (uint64_t)avail * 8) return false;
      bp(done, n, base + at + pos);
      const uint64_t bytes = groups * (uint64_t)bitw;
      pos = rfl(pos + (bytes < (uint64_t)avail ? (uint32_t)bytes : avail));
      done = rfl(done + n);
    } else {
      const uint64_t n64 = h >> 1;
      if (n64 == 0 || avail < 1) return false;
      const uint32_t v = (uint32_t)W.u64(at + pos) & 0xFFu;
      pos += 1;
      if ((v >> bitw) != 0) return false;
      const uint32_t n = n64 > (uint64_t)(nvals - done) ? nvals - done : (uint32_t)n64;
      rle(done, n, v);
      done = rfl(done + n);
    }
  }
  return true;
}

// n <= 8 bytes at p, little-endian. LDS = true: p points into the workgroup's LDS (a staged level stream) and the bytes are read with
// ds_read — a flat load would do, but it counts on vmcnt as well, and the wave would wait for the atomics of the run before at every run.
template <bool LDS>
__device__ __forceinline__ uint64_t lv_load_le(const uint8_t* p, int n) {
  if (!LDS) return load_le(p, n);
  const __attribute__((address_space(3))) uint8_t* q = (const __attribute__((address_space(3))) uint8_t*)(uintptr_t)p;
  uint64_t v = 0;
  for (int b = 0; b < n; ++b) v |= (uint64_t)q[b] << (8 * b);
  return v;
}
template <bool LDS>
__device__ __forceinline__ uint32_t lv_extract_bits(const uint8_t* src, uint64_t i, int bitw) {
  const uint64_t bit = i * (uint64_t)bitw;
  const int sh = (int)(bit & 7);
  const uint64_t v = lv_load_le<LDS>(src + (bit >> 3), (sh + bitw + 7) >> 3);
  return (uint32_t)((v >> sh) & ((bitw >= 32) ? 0xFFFFFFFFu : ((1u << bitw) - 1)));
}

// bits [dst0, dst0 + n) of the zeroed LSB-first bitmap := the first n bits of `src` (packed, bit width 1; src == nullptr: ones).
// Returns this thread's share of the number of ones. Called by all `nthr` threads.
template <bool LDS = false>
__device__ __forceinline__ uint32_t dv_put_bits(uint32_t* __restrict__ bitmap, uint64_t dst0, uint32_t n, const uint8_t* __restrict__ src,
                                                uint32_t tid, uint32_t nthr) {
  if (n == 0) return 0;
  uint32_t ones = 0;
  const uint64_t first_word = dst0 >> 5, last_word = (dst0 + n - 1) >> 5;
  for (uint64_t w = first_word + tid; w <= last_word; w += nthr) {
    const uint64_t lo = w << 5;
    const uint64_t a = lo > dst0 ? lo : dst0;
    const uint64_t e = (lo + 32 < dst0 + n) ? lo + 32 : dst0 + n;
    const int nb = (int)(e - a);
    uint32_t bits;
    if (!src) {
      bits = (nb == 32 ? 0xFFFFFFFFu : ((1u << nb) - 1)) << (a - lo);
    } else {
      const uint64_t s0 = a - dst0;
      const uint8_t* p = src + (s0 >> 3);
      const int sh = (int)(s0 & 7);
      const uint64_t v = lv_load_le<LDS>(p, (sh + nb + 7) >> 3);
      bits = (uint32_t)((v >> sh) & (nb == 32 ? 0xFFFFFFFFull : ((1ull << nb) - 1))) << (a - lo);
    }
    if (bits) {
      if (nb == 32) bitmap[w] = bits; else atomicOr(&bitmap[w], bits);
      ones += (uint32_t)__popc(bits);
    }
  }
  return ones;
}

__device__ __forceinline__ uint32_t dv_block_sum(uint32_t v, uint32_t* sh4) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}

// one chunk of a batch as the decode kernels see it (device copy; the arrays sit in the batch's blob)
struct DvChunkD {
  const DvPage* pages;
  const uint32_t* dp;      // index into `pages` of every data page
  uint32_t* nn;            // per data page: non-null values
  uint32_t* voff;          // per data page: where the values start in the page
  uint64_t* vbase;         // per data page: values before it (+ the total)
  const uint8_t* img;      // what is decoded: the decompressed image, or the chunk itself (UNCOMPRESSED)
  const void* dict;
  void* dict_out;
  void* target;            // values: the output, or the dense buffer of a column with NULLs
  uint32_t* bitmap;        // validity (nullable columns)
  uint32_t* hdr;           // [0] first failure (DV_*), [2..3] non-null values of the chunk (u64)
  PqConv cv;
  uint32_t dict_n, dict_page, nd, slices;
  uint64_t rows;
  // List columns: bit width of the definition levels (0 = a flat column), the largest level, the list's own nullability, and the
  // entry bitmaps next to `bitmap` (= the entry carries a value): continues a row / is an element (NULL or not) / the list is not NULL
  uint32_t ldw, lmax, lnull, lpad;
  uint32_t* isrep;
  uint32_t* iselem;
  uint32_t* lvalid;
  // nested leaves: bit width of the repetition levels (List columns: 1; 0 = the leaf has no LIST above it, v1 pages carry no repetition
  // stream), the largest repetition level, and the per-entry level bytes dv_levels_kernel<true> writes (List columns: the bitmaps above)
  uint32_t rw, rmax;
  uint8_t* lrep;
  uint8_t* ldef;
};

// the n bytes at p := v, by all `nthr` threads (the aligned middle as words)
__device__ __forceinline__ void dv_fill_bytes(uint8_t* __restrict__ p, uint32_t n, uint8_t v, uint32_t tid, uint32_t nthr) {
  const uint32_t a = (4u - (uint32_t)((uintptr_t)p & 3u)) & 3u, head = a < n ? a : n;
  if (tid < head) p[tid] = v;
  const uint32_t nw = (n - head) >> 2;
  uint32_t* __restrict__ pw = (uint32_t*)(p + head);
  const uint32_t v4 = (uint32_t)v * 0x01010101u;
  for (uint32_t i = tid; i < nw; i += nthr) pw[i] = v4;
  const uint32_t done = head + 4 * nw;
  if (tid < n - done) p[done + tid] = v;
}

// nested leaves: `n` levels from entry dst0 on — packed at width bw (src) or a run of `run` — as one byte per entry into lev; with a
// bitmap (the definition levels), also the entries whose level is vmax (= carry a value), of which this thread's share is returned.
// *bad: a level above vmax. Called by all `nthr` threads (whole waves); packed levels one entry per lane, as dv_put_def.
template <bool LDS = false>
__device__ __forceinline__ uint32_t dv_put_lev(uint8_t* __restrict__ lev, uint32_t* __restrict__ bitmap, uint32_t vmax, uint32_t bw, uint64_t dst0, uint32_t n,
                                               const uint8_t* __restrict__ src, uint32_t run, uint32_t tid, uint32_t nthr, bool* bad) {
  if (n == 0) return 0;
  if (!src) {
    if (run > vmax) *bad = true;
    dv_fill_bytes(lev + dst0, n, (uint8_t)run, tid, nthr);
    return bitmap && run == vmax ? dv_put_bits(bitmap, dst0, n, nullptr, tid, nthr) : 0u;
  }
  uint32_t ones = 0;
  const uint32_t lane = tid & 63u;
  for (uint32_t base = tid & ~63u; base < n; base += nthr) {
    const uint32_t x = base + lane;
    const bool in = x < n;
    const uint32_t v = in ? lv_extract_bits<LDS>(src, x, (int)bw) : 0u;
    if (in && v > vmax) *bad = true;
    if (in) lev[dst0 + x] = (uint8_t)v;
    if (!bitmap) continue;
    const uint64_t mv = __ballot(in && v == vmax);
    if (lane < 3) {
      const uint64_t p0 = dst0 + base;
      const uint32_t sh = (uint32_t)(p0 & 31);
      const uint32_t bv = lane == 0 ? (uint32_t)(mv << sh) : lane == 1 ? (uint32_t)(mv >> (32 - sh)) : (sh ? (uint32_t)(mv >> (64 - sh)) : 0u);
      if (bv) atomicOr(&bitmap[(p0 >> 5) + lane], bv);
      if (lane == 0) ones += (uint32_t)__popcll(mv);
    }
  }
  return ones;
}

// definition levels of `n` entries from dst0 on — packed at width dw (src) or a run of `run` — into the three entry bitmaps; returns this
// thread's share of the entries that carry a value. *bad: a level above the column's maximum. Called by all `nthr` threads (whole waves).
// A run of one level fills whole words, one per thread. Packed levels take ONE ENTRY PER LANE: a wave extracts 64 levels at once, three
// ballots are the 64 bits of the three bitmaps, and lanes 0..2 put the (at most three) 32-bit words they touch — a page's levels are
// mostly short packed runs between RLE runs, where one thread extracting a word's 32 levels one after the other was the whole cost
// (12.8 of the 16.1 ms of a 6 M-row List<Int64> chunk, profiles/r05_pq_list_kernel_stats.csv).
template <bool LDS = false>
__device__ __forceinline__ uint32_t dv_put_def(const DvChunkD& C, uint64_t dst0, uint32_t n, const uint8_t* __restrict__ src, uint32_t run, uint32_t tid,
                                               uint32_t nthr, bool* bad) {
  if (n == 0) return 0;
  uint32_t ones = 0;
  const uint32_t D = C.lmax, L = C.lnull;
  if (!src) {
    if (run > D) *bad = true;
    const bool isv = run == D, ise = run >= L + 1, isl = run >= L && L;
    const uint64_t first_word = dst0 >> 5, last_word = (dst0 + n - 1) >> 5;
    for (uint64_t w = first_word + tid; w <= last_word; w += nthr) {
      const uint64_t lo = w << 5;
      const uint64_t a = lo > dst0 ? lo : dst0;
      const uint64_t e = (lo + 32 < dst0 + n) ? lo + 32 : dst0 + n;
      const int nb = (int)(e - a);
      const uint32_t bits = (nb == 32 ? 0xFFFFFFFFu : ((1u << nb) - 1)) << (a - lo);
      if (isv) { atomicOr(&C.bitmap[w], bits); ones += (uint32_t)__popc(bits); }
      if (ise) atomicOr(&C.iselem[w], bits);
      if (isl) atomicOr(&C.lvalid[w], bits);
    }
    return ones;
  }
  const uint32_t lane = tid & 63u;
  for (uint32_t base = tid & ~63u; base < n; base += nthr) {          // (wave-uniform: this wave's entries base .. base + 63 of the run)
    const uint32_t x = base + lane;
    const bool in = x < n;
    const uint32_t v = in ? lv_extract_bits<LDS>(src, x, (int)C.ldw) : 0u;
    if (in && v > D) *bad = true;
    const uint64_t mv = __ballot(in && v == D), me = __ballot(in && v >= L + 1), ml = L ? __ballot(in && v >= L) : 0ull;
    if (lane < 3) {
      const uint64_t p0 = dst0 + base;                                 // entry of mask bit 0
      const uint32_t sh = (uint32_t)(p0 & 31);
      const uint64_t w = (p0 >> 5) + lane;
      // word `lane` of the 96-bit value (mask << sh)
      const uint32_t bv = lane == 0 ? (uint32_t)(mv << sh) : lane == 1 ? (uint32_t)(mv >> (32 - sh)) : (sh ? (uint32_t)(mv >> (64 - sh)) : 0u);
      const uint32_t be = lane == 0 ? (uint32_t)(me << sh) : lane == 1 ? (uint32_t)(me >> (32 - sh)) : (sh ? (uint32_t)(me >> (64 - sh)) : 0u);
      const uint32_t bl = lane == 0 ? (uint32_t)(ml << sh) : lane == 1 ? (uint32_t)(ml >> (32 - sh)) : (sh ? (uint32_t)(ml >> (64 - sh)) : 0u);
      if (bv) atomicOr(&C.bitmap[w], bv);
      if (be) atomicOr(&C.iselem[w], be);
      if (bl) atomicOr(&C.lvalid[w], bl);
      if (lane == 0) ones += (uint32_t)__popcll(mv);
    }
  }
  return ones;
}

// definition levels of one data page -> validity bits + the page's non-null count and the offset of its values
// A List page's level streams are thousands of short runs, and the walk is a chain: header -> position of the next header. Read from the
// image every hop is an HBM / L2 round trip (plus one for the run's payload): 9.7 ms for the 300 pages of a 6 M-row List<Int64> chunk,
// ~1 us per run. With `lds_bytes` of dynamic LDS (batches that hold a List chunk) the workgroup first copies both streams into LDS — they
// are contiguous in the page, 25-35 KB for a 1 MiB page — and walks them there; streams that do not fit are walked in place as before.
// NEST: the instantiation for a nested leaf (dv_put_lev; a batch that holds one is that chunk alone); flat and List chunks keep the other.
constexpr uint32_t LV_LDS = 40960;
template <bool NEST>
__global__ __launch_bounds__(256) void dv_levels_kernel(const DvChunkD* __restrict__ cds, const uint2* __restrict__ map, uint32_t lds_bytes) {
  extern __shared__ __align__(16) uint8_t lv_lds[];
  __shared__ uint32_t sh4[4];
  const uint2 m = map[blockIdx.x];
  const DvChunkD& C = cds[m.x];
  const uint32_t d = m.y;
  const DvPage* __restrict__ pages = C.pages;
  const uint8_t* __restrict__ img = C.img;
  uint32_t* __restrict__ nn = C.nn;
  uint32_t* __restrict__ voff = C.voff;
  uint32_t* __restrict__ bitmap = C.bitmap;
  uint32_t* __restrict__ ctl = C.hdr;
  const DvPage P = pages[C.dp[d]];
  const uint8_t* s = img + P.img_off;
  uint32_t len, vo;
  const uint8_t* stream;
  if (C.ldw) {
    // a List column's / nested leaf's page: repetition levels (width rw), then definition levels (width ldw), then the values
    const uint8_t* rep;
    uint32_t rlen;
    bool ok = true;
    if (P.type == PG_DATA) {
      const uint32_t rh = !NEST || C.rw ? 4u : 0u;     // (a nested leaf without a LIST above it: no repetition stream)
      ok = P.uncomp_len >= rh + 4;
      rlen = ok && rh ? (uint32_t)load_le(s, 4) : 0;
      ok = ok && rlen <= P.uncomp_len - rh - 4;
      rep = s + rh;
      len = ok ? (uint32_t)load_le(s + rh + rlen, 4) : 0;
      ok = ok && len <= P.uncomp_len - rh - 4 - rlen;
      stream = s + rh + 4 + rlen;
      vo = rh + 4 + rlen + len;
    } else {
      rlen = P.rep_len; rep = s;              // (the host checked rep_len <= lev_len <= uncomp_len)
      len = P.lev_len - P.rep_len; stream = s + rlen;
      vo = P.lev_len;
    }
    if (!ok) { dv_fail(ctl, DV_CORRUPT); if (threadIdx.x == 0) { nn[d] = 0; voff[d] = P.uncomp_len; } return; }
    const uint32_t tid = threadIdx.x;
    const uint64_t r0 = P.row_start;
    bool bad = false;
    {
      const uint32_t span = (uint32_t)((stream + len) - rep);       // repetition levels, (v1: the 4-byte length,) definition levels
      const uint32_t k = (uint32_t)((uintptr_t)rep & 3u);           // the copy keeps the address modulo 4: whole dwords in the middle
      if (span + k + 4 <= lds_bytes) {
        const uint32_t head = ((4u - k) & 3u) < span ? ((4u - k) & 3u) : span;
        if (tid < head) lv_lds[k + tid] = rep[tid];
        const uint32_t nw = (span - head) >> 2;
        const uint32_t* __restrict__ gw = (const uint32_t*)(rep + head);
        uint32_t* lw = (uint32_t*)(lv_lds + k + head);
        for (uint32_t w = tid; w < nw; w += 256) lw[w] = gw[w];
        const uint32_t done = head + 4 * nw;
        if (tid < span - done) lv_lds[k + done + tid] = rep[done + tid];
        __syncthreads();
        if (tid >= 64) return;             // one wave walks the page: its runs are a chain (no barrier follows on this path)
        LvWin W;
        W.open(lv_lds + k, lv_lds + lds_bytes, tid);
        const uint8_t* base = lv_lds + k;
        const uint32_t dat = (uint32_t)(stream - rep);
        ok = (NEST && C.rw == 0) || dv_walk_hybrid_wave(
            W, base, 0, rlen, NEST ? (int)C.rw : 1, P.num_values,
            [&](uint32_t first, uint32_t n, uint32_t v) {
              if constexpr (NEST) (void)dv_put_lev(C.lrep, nullptr, C.rmax, C.rw, r0 + first, n, nullptr, v, tid, 64, &bad);
              else if (v == 1) (void)dv_put_bits(C.isrep, r0 + first, n, nullptr, tid, 64);
            },
            [&](uint32_t first, uint32_t n, const uint8_t* src) {
              if constexpr (NEST) (void)dv_put_lev<true>(C.lrep, nullptr, C.rmax, C.rw, r0 + first, n, src, 0, tid, 64, &bad);
              else (void)dv_put_bits<true>(C.isrep, r0 + first, n, src, tid, 64);
            });
        uint32_t mine = 0;
        ok = ok && dv_walk_hybrid_wave(
            W, base, dat, len, (int)C.ldw, P.num_values,
            [&](uint32_t first, uint32_t n, uint32_t v) {
              if constexpr (NEST) mine += dv_put_lev(C.ldef, C.bitmap, C.lmax, C.ldw, r0 + first, n, nullptr, v, tid, 64, &bad);
              else mine += dv_put_def(C, r0 + first, n, nullptr, v, tid, 64, &bad);
            },
            [&](uint32_t first, uint32_t n, const uint8_t* src) {
              if constexpr (NEST) mine += dv_put_lev<true>(C.ldef, C.bitmap, C.lmax, C.ldw, r0 + first, n, src, 0, tid, 64, &bad);
              else mine += dv_put_def<true>(C, r0 + first, n, src, 0, tid, 64, &bad);
            });
        for (int dd = 32; dd >= 1; dd >>= 1) mine += __shfl_xor(mine, dd, 64);
        if (!ok || __ballot(bad) != 0) { dv_fail(ctl, DV_CORRUPT); ok = false; }
        if (tid == 0) { nn[d] = ok ? mine : 0; voff[d] = ok ? vo : P.uncomp_len; }
        return;
      }
    }
    ok = (NEST && C.rw == 0) || dv_walk_hybrid(
        rep, rlen, NEST ? (int)C.rw : 1, P.num_values,
        [&](uint32_t first, uint32_t n, uint32_t v) {
          if constexpr (NEST) (void)dv_put_lev(C.lrep, nullptr, C.rmax, C.rw, r0 + first, n, nullptr, v, tid, 256, &bad);
          else if (v == 1) (void)dv_put_bits(C.isrep, r0 + first, n, nullptr, tid, 256);
        },
        [&](uint32_t first, uint32_t n, const uint8_t* src) {
          if constexpr (NEST) (void)dv_put_lev(C.lrep, nullptr, C.rmax, C.rw, r0 + first, n, src, 0, tid, 256, &bad);
          else (void)dv_put_bits(C.isrep, r0 + first, n, src, tid, 256);
        });
    uint32_t mine = 0;
    ok = ok && dv_walk_hybrid(
        stream, len, (int)C.ldw, P.num_values,
        [&](uint32_t first, uint32_t n, uint32_t v) {
          if constexpr (NEST) mine += dv_put_lev(C.ldef, C.bitmap, C.lmax, C.ldw, r0 + first, n, nullptr, v, tid, 256, &bad);
          else mine += dv_put_def(C, r0 + first, n, nullptr, v, tid, 256, &bad);
        },
        [&](uint32_t first, uint32_t n, const uint8_t* src) {
          if constexpr (NEST) mine += dv_put_lev(C.ldef, C.bitmap, C.lmax, C.ldw, r0 + first, n, src, 0, tid, 256, &bad);
          else mine += dv_put_def(C, r0 + first, n, src, 0, tid, 256, &bad);
        });
    const uint32_t total = dv_block_sum(mine, sh4);
    if (!ok || __syncthreads_or(bad ? 1 : 0)) { dv_fail(ctl, DV_CORRUPT); ok = false; }
    if (tid == 0) { nn[d] = ok ? total : 0; voff[d] = ok ? vo : P.uncomp_len; }
    return;
  }
  if (P.type == PG_DATA) {
    if (P.uncomp_len < 4) { dv_fail(ctl, DV_CORRUPT); if (threadIdx.x == 0) { nn[d] = 0; voff[d] = P.uncomp_len; } return; }
    len = (uint32_t)load_le(s, 4);
    if (len > P.uncomp_len - 4) { dv_fail(ctl, DV_CORRUPT); if (threadIdx.x == 0) { nn[d] = 0; voff[d] = P.uncomp_len; } return; }
    stream = s + 4;
    vo = 4 + len;
  } else {
    len = P.lev_len;  // (the host checked lev_len <= uncomp_len)
    stream = s;
    vo = len;
  }
  uint32_t mine = 0, runs = 0;
  const uint32_t tid = threadIdx.x;
  const uint64_t r0 = P.row_start;
  const bool ok = dv_walk_hybrid(
      stream, len, 1, P.num_values,
      [&](uint32_t first, uint32_t n, uint32_t v) {
        if (v == 1) { (void)dv_put_bits(bitmap, r0 + first, n, nullptr, tid, 256); runs += n; }
      },
      [&](uint32_t first, uint32_t n, const uint8_t* src) { mine += dv_put_bits(bitmap, r0 + first, n, src, tid, 256); });
  const uint32_t total = dv_block_sum(mine, sh4) + runs;
  if (!ok) dv_fail(ctl, DV_CORRUPT);
  if (tid == 0) { nn[d] = ok ? total : 0; voff[d] = ok ? vo : P.uncomp_len; }
}

// vbase[d] = number of non-null values in the data pages before d; vbase[n] = all of them (also into the chunk's header). One workgroup per chunk.
__global__ __launch_bounds__(256) void dv_scan_kernel(const DvChunkD* __restrict__ cds) {
  const DvChunkD& C = cds[blockIdx.x];
  const uint32_t* __restrict__ nn = C.nn;
  const uint32_t n = C.nd;
  uint64_t* __restrict__ vbase = C.vbase;
  __shared__ uint64_t wt[4];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (uint32_t c = 0; c < n; c += 256) {
    const uint32_t i = c + threadIdx.x;
    uint64_t v = i < n ? nn[i] : 0, incl = v;
    for (int dd = 1; dd < 64; dd <<= 1) {
      const uint64_t t = __shfl_up(incl, dd, 64);
      if ((int)(threadIdx.x & 63) >= dd) incl += t;
    }
    if ((threadIdx.x & 63) == 63) wt[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint64_t wb = carry;
    for (uint32_t k = 0; k < (threadIdx.x >> 6); ++k) wb += wt[k];
    if (i < n) vbase[i] = wb + incl - v;
    __syncthreads();
    if (threadIdx.x == 255) carry = wb + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) { vbase[n] = carry; *(uint64_t*)(C.hdr + 2) = carry; }
}

// ---------------------------------------------------------------------------------------------
// values
// ---------------------------------------------------------------------------------------------
constexpr uint32_t SW_TILE = 16384;  // bytes of a BYTE_ARRAY page staged in LDS at a time

struct DvStrShared {
  uint32_t queue[256];
  uint32_t cur, cnt, err;
  __align__(16) uint8_t tile[SW_TILE];
};

// PLAIN BYTE_ARRAY: `count` values at img[base ..) (region of `rlen` bytes) -> views out[o0 ..). The chain of 4-byte length
// prefixes is serial: the region is staged in LDS 16 KiB at a time, thread 0 follows the lengths inside the staged tile (an LDS
// round trip per value instead of an L2 one) and queues up to 256 value offsets, then every thread turns one offset into a view.
__device__ bool dv_walk_strings(const uint8_t* __restrict__ img, uint64_t base, uint32_t rlen, uint32_t count, void* __restrict__ out,
                                uint64_t o0, DvStrShared* S) {
  const uint32_t tid = threadIdx.x;
  if (tid == 0) { S->cur = 0; S->err = 0; }
  __syncthreads();
  uint32_t k = 0;
  while (k < count) {
    const uint32_t cur0 = S->cur;
    // stage [cur0, cur0 + SW_TILE) of the region, from the 16-byte aligned address at or before it
    const uint8_t* p0 = img + base + cur0;
    const uint32_t x0 = (uint32_t)((uintptr_t)p0 & 15u);
    const uint8_t* pa = p0 - x0;
    const uint32_t have = rlen - cur0 + x0;  // staged bytes that belong to the region (+ the x0 bytes in front)
    __syncthreads();
    for (uint32_t x = tid * 16; x < SW_TILE && x < have; x += 256 * 16) *(uint4*)(S->tile + x) = *(const uint4*)(pa + x);
    __syncthreads();
    // several rounds of (walk, emit) per staged tile
    for (;;) {
      if (tid == 0) {
        uint32_t cur = S->cur, c = 0, e = 0;
        while (k + c < count && c < 256) {
          const uint32_t x = cur - cur0 + x0;
          if (x + 4 > SW_TILE) break;  // the next length prefix is not (entirely) staged
          if (rlen - cur < 4) { e = 1; break; }
          uint32_t len;
          memcpy(&len, S->tile + x, 4);
          if (rlen - cur - 4 < len) { e = 1; break; }
          S->queue[c++] = cur + 4;
          cur += 4 + len;
        }
        S->cur = cur; S->cnt = c; S->err = e;
      }
      __syncthreads();
      const uint32_t c = S->cnt;
      if (S->err) return false;
      if (tid < c) store_view(img, (uint32_t)(base + S->queue[tid]), out, o0 + k + tid);
      k += c;
      __syncthreads();
      if (c == 0 || k >= count) break;  // c == 0: restage from S->cur (its prefix then lies at x0 <= 15: the walk advances)
    }
  }
  return true;
}

__device__ __forceinline__ void dv_store_int(const PqConv& cv, void* out, uint64_t o, uint64_t v) {
  if (cv.physical == PT_INT32) {
    const uint32_t x = (uint32_t)v;
    switch (cv.esize) {
      case 1: ((uint8_t*)out)[o] = (uint8_t)x; break;
      case 2: ((uint16_t*)out)[o] = (uint16_t)x; break;
      case 4: ((uint32_t*)out)[o] = x; break;
      default: ((int64_t*)out)[o] = (int64_t)(int32_t)x; break;
    }
  } else if (cv.esize == 16) {
    ((i128*)out)[o] = (i128)(int64_t)v;
  } else {
    ((uint64_t*)out)[o] = v;
  }
}

__device__ __forceinline__ uint64_t dv_unpack64(const uint8_t* __restrict__ src, uint32_t i, uint32_t b) {
  if (b == 0) return 0;
  const uint64_t bit = (uint64_t)i * b;
  const uint8_t* p = src + (bit >> 3);
  const uint32_t sh = (uint32_t)(bit & 7);
  const uint32_t nb = (sh + b + 7) >> 3;  // <= 9
  uint64_t v = load_le(p, nb < 8 ? (int)nb : 8) >> sh;
  if (nb > 8) v |= (uint64_t)p[8] << (64 - sh);
  return b >= 64 ? v : (v & ((1ull << b) - 1));
}

struct DvDeltaShared {
  uint64_t wt[4];
};

// DELTA_BINARY_PACKED (Encodings.md): <block size> <miniblocks per block> <total count> <first value>, then per block
// <min delta> <bit width per miniblock> <miniblocks>. The first `count` values -> put(i, v) (called by the thread that owns value i);
// exact: the stream holds exactly `count` values (the length streams of DELTA_(LENGTH_)BYTE_ARRAY). *end: where the stream ends (past the
// last miniblock that holds a value).
template <class Put>
__device__ __forceinline__ bool dv_delta_walk(const uint8_t* __restrict__ s, uint32_t rlen, uint32_t count, bool exact, DvDeltaShared* S, Put&& put,
                                              uint32_t* end) {
  const uint32_t tid = threadIdx.x;
  uint32_t pos = 0;
  uint64_t bs, mb, total, zz;
  if (!dv_varint(s, &pos, rlen, &bs) || !dv_varint(s, &pos, rlen, &mb) || !dv_varint(s, &pos, rlen, &total) || !dv_varint(s, &pos, rlen, &zz))
    return false;
  if (mb == 0 || mb > 4096 || bs == 0 || bs > (1u << 24) || bs % mb != 0) return false;
  const uint32_t vpm = (uint32_t)(bs / mb);
  if (vpm % 8 != 0) return false;
  if (total < (uint64_t)count || (exact && total != (uint64_t)count)) return false;
  *end = pos;
  if (count == 0) return true;
  uint64_t last = (zz >> 1) ^ (0 - (zz & 1));
  if (tid == 0) put(0u, last);
  uint32_t produced = 1;
  while (produced < count) {
    uint64_t mz;
    if (!dv_varint(s, &pos, rlen, &mz)) return false;
    const uint64_t min_delta = (mz >> 1) ^ (0 - (mz & 1));
    if (rlen - pos < (uint32_t)mb) return false;
    const uint32_t bwpos = pos;
    pos += (uint32_t)mb;
    for (uint32_t m = 0; m < (uint32_t)mb && produced < count; ++m) {
      const uint32_t b = s[bwpos + m];
      if (b > 64) return false;
      const uint32_t need = (count - produced) < vpm ? (count - produced) : vpm;
      const uint64_t need_bytes = ((uint64_t)need * b + 7) >> 3;
      if ((uint64_t)(rlen - pos) < need_bytes) return false;
      for (uint32_t c0 = 0; c0 < need; c0 += 256) {
        const uint32_t i = c0 + tid;
        const uint64_t dlt = i < need ? min_delta + dv_unpack64(s + pos, i, b) : 0;
        uint64_t incl = dlt;
        for (int dd = 1; dd < 64; dd <<= 1) {
          const uint64_t t = __shfl_up(incl, dd, 64);
          if ((int)(tid & 63) >= dd) incl += t;
        }
        __syncthreads();
        if ((tid & 63) == 63) S->wt[tid >> 6] = incl;
        __syncthreads();
        uint64_t wb = last;
        for (uint32_t w = 0; w < (tid >> 6); ++w) wb += S->wt[w];
        if (i < need) put(produced + i, wb + incl);
        last += S->wt[0] + S->wt[1] + S->wt[2] + S->wt[3];
      }
      const uint64_t mbytes = ((uint64_t)vpm * b) >> 3;
      pos += mbytes < (uint64_t)(rlen - pos) ? (uint32_t)mbytes : rlen - pos;
      produced += need;
    }
  }
  *end = pos;
  return true;
}

// DELTA_BINARY_PACKED values (INT32 / INT64) -> out[o0 ..)
__device__ bool dv_delta(const uint8_t* __restrict__ s, uint32_t rlen, uint32_t count, const PqConv& cv, void* __restrict__ out, uint64_t o0,
                         DvDeltaShared* S) {
  uint32_t end;
  return dv_delta_walk(s, rlen, count, false, S, [&](uint32_t i, uint64_t v) { dv_store_int(cv, out, o0 + i, v); }, &end);
}

__device__ __forceinline__ void dv_put_dict(const PqConv& cv, const void* __restrict__ dict, uint32_t idx, void* __restrict__ out, uint64_t o) {
  switch (cv.esize) {
    case 1: ((uint8_t*)out)[o] = ((const uint8_t*)dict)[idx]; break;
    case 2: ((uint16_t*)out)[o] = ((const uint16_t*)dict)[idx]; break;
    case 4: ((uint32_t*)out)[o] = ((const uint32_t*)dict)[idx]; break;
    case 8: ((uint64_t*)out)[o] = ((const uint64_t*)dict)[idx]; break;
    default: ((uint4*)out)[o] = ((const uint4*)dict)[idx]; break;
  }
}

union DvValShared {
  DvStrShared str;
  DvDeltaShared delta;
};

// the dictionary page (PLAIN) -> dictionary in the output type. One workgroup per chunk that has one.
__global__ __launch_bounds__(256) void dv_dict_kernel(const DvChunkD* __restrict__ cds, const uint32_t* __restrict__ list) {
  __shared__ DvStrShared S;
  const DvChunkD& C = cds[list[blockIdx.x]];
  const uint8_t* __restrict__ img = C.img;
  const PqConv cv = C.cv;
  void* __restrict__ dict = C.dict_out;
  uint32_t* __restrict__ ctl = C.hdr;
  const DvPage P = C.pages[C.dict_page];
  if (P.num_values == 0) return;
  if (cv.physical == PT_BYTE_ARRAY) {
    if (!dv_walk_strings(img, P.img_off, P.uncomp_len, P.num_values, dict, 0, &S)) dv_fail(ctl, DV_CORRUPT);
    return;
  }
  const uint32_t w = (uint32_t)plain_width(cv.physical, cv.type_length);
  if (w == 0 || P.uncomp_len / w < P.num_values) { dv_fail(ctl, DV_CORRUPT); return; }
  for (uint32_t i = threadIdx.x; i < P.num_values; i += 256) store_plain(cv, img + P.img_off + (uint64_t)i * w, dict, i);
}

// one workgroup per (data page, slice): blockIdx.y splits PLAIN fixed-width pages; the serial encodings run in slice 0
__global__ __launch_bounds__(256) void dv_values_kernel(const DvChunkD* __restrict__ cds, const uint2* __restrict__ map) {
  __shared__ DvValShared S;
  const uint2 m = map[blockIdx.x];
  const DvChunkD& C = cds[m.x];
  if (blockIdx.y >= C.slices) return;
  const uint32_t d = m.y, tid = threadIdx.x;
  const uint8_t* __restrict__ img = C.img;
  const PqConv cv = C.cv;
  const void* __restrict__ dict = C.dict;
  const uint32_t dict_n = C.dict_n;
  void* __restrict__ out = C.target;
  const uint64_t out_cap = C.rows;
  uint32_t* __restrict__ ctl = C.hdr;
  const DvPage P = C.pages[C.dp[d]];
  const uint32_t n = C.nn[d], vo = C.voff[d];
  const uint64_t o0 = C.vbase[d];
  if (n == 0) return;
  if (vo > P.uncomp_len || n > P.num_values || o0 + n > out_cap) { dv_fail(ctl, DV_CORRUPT); return; }
  const uint8_t* s = img + P.img_off + vo;
  const uint32_t rlen = P.uncomp_len - vo;
  const uint32_t enc = P.enc;
  if (enc == ENC_PLAIN && cv.physical != PT_BOOLEAN && cv.physical != PT_BYTE_ARRAY) {
    const uint32_t w = (uint32_t)plain_width(cv.physical, cv.type_length);
    if (w == 0 || rlen / w < n) { dv_fail(ctl, DV_CORRUPT); return; }
    const uint32_t lo = (uint32_t)((uint64_t)n * blockIdx.y / C.slices), hi = (uint32_t)((uint64_t)n * (blockIdx.y + 1) / C.slices);
    for (uint32_t i = lo + tid; i < hi; i += 256) store_plain(cv, s + (uint64_t)i * w, out, o0 + i);
    return;
  }
  if (blockIdx.y != 0) return;
  bool ok = true;
  if (enc == ENC_PLAIN && cv.physical == PT_BOOLEAN) {
    if ((uint64_t)rlen * 8 < n) { dv_fail(ctl, DV_CORRUPT); return; }
    (void)dv_put_bits((uint32_t*)out, o0, n, s, tid, 256);
  } else if (enc == ENC_PLAIN) {
    ok = dv_walk_strings(img, P.img_off + vo, rlen, n, out, o0, &S.str);
  } else if (enc == ENC_PLAIN_DICT || enc == ENC_RLE_DICT) {
    if (rlen < 1 || dict_n == 0 || !dict) { dv_fail(ctl, DV_CORRUPT); return; }
    const int bitw = s[0];
    if (bitw > 32) { dv_fail(ctl, DV_CORRUPT); return; }
    ok = dv_walk_hybrid(
        s + 1, rlen - 1, bitw, n,
        [&](uint32_t first, uint32_t cnt, uint32_t v) {
          if (v >= dict_n) dv_fail(ctl, DV_CORRUPT);             // (parquet-rs raises; the index is clamped for memory safety only)
          const uint32_t idx = v < dict_n ? v : dict_n - 1;
          for (uint32_t i = tid; i < cnt; i += 256) dv_put_dict(cv, dict, idx, out, o0 + first + i);
        },
        [&](uint32_t first, uint32_t cnt, const uint8_t* src) {
          for (uint32_t i = tid; i < cnt; i += 256) {
            uint32_t idx = extract_bits(src, i, bitw);
            if (idx >= dict_n) { dv_fail(ctl, DV_CORRUPT); idx = dict_n - 1; }
            dv_put_dict(cv, dict, idx, out, o0 + first + i);
          }
        });
  } else if (enc == ENC_RLE && cv.physical == PT_BOOLEAN) {
    if (rlen < 4) { dv_fail(ctl, DV_CORRUPT); return; }
    const uint32_t len = (uint32_t)load_le(s, 4);
    if (len > rlen - 4) { dv_fail(ctl, DV_CORRUPT); return; }
    ok = dv_walk_hybrid(
        s + 4, len, 1, n,
        [&](uint32_t first, uint32_t cnt, uint32_t v) { if (v == 1) (void)dv_put_bits((uint32_t*)out, o0 + first, cnt, nullptr, tid, 256); },
        [&](uint32_t first, uint32_t cnt, const uint8_t* src) { (void)dv_put_bits((uint32_t*)out, o0 + first, cnt, src, tid, 256); });
  } else if (enc == ENC_DELTA_BINARY_PACKED && (cv.physical == PT_INT32 || cv.physical == PT_INT64)) {
    ok = dv_delta(s, rlen, n, cv, out, o0, &S.delta);
  } else {
    dv_fail(ctl, DV_UNSUPPORTED);
    return;
  }
  if (!ok) dv_fail(ctl, DV_CORRUPT);
}

// ---------------------------------------------------------------------------------------------
// DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY, BYTE_STREAM_SPLIT (Encodings.md): kernels of their own, launched only for batches that
// hold such pages, so that dv_values_kernel (the scan's hot path) keeps its registers and LDS
// ---------------------------------------------------------------------------------------------
// one data page in one of those encodings
struct DvXJob {
  uint32_t k, d;        // chunk of the batch, data page of the chunk
  uint32_t enc, sec;    // encoding; DELTA_BYTE_ARRAY: where the suffix bytes start, from the page's values (dv_dba_size_kernel)
  uint32_t* lens;       // DELTA_(LENGTH_)BYTE_ARRAY: scratch for the lengths (DELTA_BYTE_ARRAY: the prefix lengths, then the suffix lengths)
  uint8_t* dst;         // DELTA_BYTE_ARRAY: the page's values in the chunk's arena
  uint64_t aoff;        // DELTA_BYTE_ARRAY: offset of dst in the arena
  uint64_t bytes;       // DELTA_BYTE_ARRAY: bytes of the page's values (dv_dba_size_kernel)
  uint32_t live, pad;   // DELTA_BYTE_ARRAY: 1 = the chunk passed its sizing checks and has its arena (set by the host)
};

// 16-byte view of the `len` bytes at p, which lie at offset `off` of buffer `buf` of the column (store_view for a length known apart)
__device__ __forceinline__ void dv_view(const uint8_t* __restrict__ p, uint32_t len, uint32_t buf, uint32_t off, void* __restrict__ out, uint64_t o) {
  uint32_t w[4];
  sv_make(p, len, buf, off, w);
  ((uint4*)out)[o] = make_uint4(w[0], w[1], w[2], w[3]);
}

// exclusive prefix sum of v over the workgroup (256 threads); *tot: the workgroup's sum. Called by all threads.
__device__ __forceinline__ uint64_t dv_block_xscan(uint64_t v, uint64_t* wt, uint64_t* tot) {
  const uint32_t tid = threadIdx.x;
  uint64_t incl = v;
  for (int dd = 1; dd < 64; dd <<= 1) {
    const uint64_t t = __shfl_up(incl, dd, 64);
    if ((int)(tid & 63) >= dd) incl += t;
  }
  __syncthreads();
  if ((tid & 63) == 63) wt[tid >> 6] = incl;
  __syncthreads();
  uint64_t wb = 0;
  for (uint32_t w = 0; w < (tid >> 6); ++w) wb += wt[w];
  *tot = wt[0] + wt[1] + wt[2] + wt[3];
  return wb + incl - v;
}

// value i of a BYTE_STREAM_SPLIT page of n values (byte k of value i at s[k n + i]) -> element o of out, converted as store_plain converts
// the same bytes in PLAIN order (the bytes are gathered into registers, not into a private array)
__device__ __forceinline__ void dv_store_bss(const PqConv& cv, const uint8_t* __restrict__ s, uint32_t n, uint32_t i, void* __restrict__ out, uint64_t o) {
  if (cv.physical == PT_FLBA) {
    // big-endian two's complement of type_length (1..16) bytes
    const int L = cv.type_length;
    u128 v = (s[i] & 0x80) ? ~(u128)0 : (u128)0;
#pragma unroll
    for (int b = 0; b < 16; ++b)
      if (b < L) v = (v << 8) | s[(uint64_t)b * n + i];
    if (cv.esize == 16) ((u128*)out)[o] = v; else ((uint64_t*)out)[o] = (uint64_t)v;
    return;
  }
  const int w = (cv.physical == PT_INT32 || cv.physical == PT_FLOAT) ? 4 : 8;
  uint64_t v = 0;
#pragma unroll
  for (int b = 0; b < 8; ++b)
    if (b < w) v |= (uint64_t)s[(uint64_t)b * n + i] << (8 * b);
  if (w == 4) {
    const uint32_t x = (uint32_t)v;
    switch (cv.esize) {
      case 1: ((uint8_t*)out)[o] = (uint8_t)x; break;
      case 2: ((uint16_t*)out)[o] = (uint16_t)x; break;
      case 4: ((uint32_t*)out)[o] = x; break;
      default: ((int64_t*)out)[o] = (int64_t)(int32_t)x; break;
    }
    return;
  }
  if (cv.esize == 16) ((i128*)out)[o] = (i128)(int64_t)v; else ((uint64_t*)out)[o] = v;
}

// DELTA_BYTE_ARRAY, step 1 (after dv_scan_kernel: the page's non-null count is known). One workgroup per page: both length streams
// -> scratch, checked (prefix[0] = 0, prefix[i] <= length of value i - 1, no negative length, each stream holds exactly the page's
// count, the suffixes fit the bytes after the streams, FIXED_LEN_BYTE_ARRAY: every value is type_length long) -> the page's bytes of
// values and where its suffix bytes start. The host reads the byte counts back and allocates the arena the values are replayed into.
__global__ __launch_bounds__(256) void dv_dba_size_kernel(const DvChunkD* __restrict__ cds, DvXJob* __restrict__ jobs) {
  __shared__ DvDeltaShared S;
  __shared__ uint64_t wt[4];
  DvXJob* J = jobs + blockIdx.x;
  const DvChunkD& C = cds[J->k];
  const uint32_t d = J->d, tid = threadIdx.x;
  uint32_t* __restrict__ ctl = C.hdr;
  const DvPage P = C.pages[C.dp[d]];
  const uint32_t n = C.nn[d], vo = C.voff[d];
  const uint64_t o0 = C.vbase[d];
  if (n == 0) return;
  if (vo > P.uncomp_len || n > P.num_values || o0 + n > C.rows) { dv_fail(ctl, DV_CORRUPT); return; }
  const uint8_t* s = C.img + P.img_off + vo;
  const uint32_t rlen = P.uncomp_len - vo;
  uint32_t* __restrict__ pre = J->lens;
  uint32_t* __restrict__ suf = J->lens + n;
  bool bad = false;
  uint32_t e1 = 0, e2 = 0;
  bool ok = dv_delta_walk(s, rlen, n, true, &S, [&](uint32_t i, uint64_t v) { bad |= (int32_t)v < 0; pre[i] = (uint32_t)v; }, &e1);
  ok = ok && dv_delta_walk(s + e1, rlen - e1, n, true, &S, [&](uint32_t i, uint64_t v) { bad |= (int32_t)v < 0; suf[i] = (uint32_t)v; }, &e2);
  if (__syncthreads_or(!ok || bad)) { dv_fail(ctl, DV_CORRUPT); return; }   // (also: the lengths are visible to the workgroup)
  const uint32_t sec = e1 + e2;
  const bool fixed = C.cv.physical == PT_FLBA;
  const uint64_t tl = (uint64_t)C.cv.type_length;
  uint64_t sufsum = 0, lensum = 0;
  for (uint32_t i = tid; i < n; i += 256) {
    const uint32_t p = pre[i], q = suf[i];
    if (i == 0 ? p != 0 : (uint64_t)p > (uint64_t)pre[i - 1] + suf[i - 1]) bad = true;
    if (fixed && (uint64_t)p + q != tl) bad = true;
    sufsum += q;
    lensum += (uint64_t)p + q;
  }
  uint64_t st, lt;
  (void)dv_block_xscan(sufsum, wt, &st);
  (void)dv_block_xscan(lensum, wt, &lt);
  if (__syncthreads_or(bad) || st > (uint64_t)(rlen - sec)) { dv_fail(ctl, DV_CORRUPT); return; }
  if (tid == 0) { J->sec = sec; J->bytes = lt; }
}

// DELTA_BYTE_ARRAY, step 2: the values into the arena. Value i is the first prefix[i] bytes of value i - 1, then suffix i — an LZ77
// sequence stream: sequence i is the literal suffix i, then a match of prefix[i + 1] bytes at distance len(value i). One wave per page
// replays it with ZWave (dv_wave.h: 64 sequences per step, one lane per output byte, an LDS ring, references beyond it read from the
// arena), the suffixes read from the page as one forward stream. The sizing kernel has checked every sequence.
__global__ __launch_bounds__(64) void dv_dba_replay_kernel(const DvChunkD* __restrict__ cds, const DvXJob* __restrict__ jobs, uint32_t ring) {
  extern __shared__ __align__(16) uint8_t dv_lds[];
  const DvXJob J = jobs[blockIdx.x];
  if (!J.live || J.bytes == 0) return;
  const DvChunkD& C = cds[J.k];
  const DvPage P = C.pages[C.dp[J.d]];
  const uint32_t n = C.nn[J.d], vo = C.voff[J.d];
  const uint32_t lane = threadIdx.x;
  const uint8_t* s = C.img + P.img_off + vo;
  const uint32_t rlen = P.uncomp_len - vo;
  DvJob Q;
  Q.src = s; Q.dst = J.dst;
  Q.comp_len = rlen; Q.uncomp_len = (uint32_t)J.bytes; Q.lev_len = 0; Q.compressed = 1;
  // readable: the page's bytes up to the next 4-byte boundary (image pages start 16-byte aligned and the image has 16 bytes of slack;
  // an UNCOMPRESSED chunk is readable up to the 16-byte boundary past its end)
  const uint32_t a = (uint32_t)((uintptr_t)s & 3u);
  Q.src_safe = ((a + rlen + 3u) & ~3u) - a;
  Q.codec = 0; Q.ctl = C.hdr;
  ZWave w;
  w.begin(Q, dv_lds, ring, lane);
  // replay() rejects a batch whose matches reach before the frame; every match here is checked, and a lane without a match (ml = 0)
  // carries off = 1, which must pass even before the first byte (a page that starts with empty strings): the frame starts one byte early
  w.frame0 = ~0u;
  FwdStream ls;
  uint32_t lp = w.a0 + J.sec;
  ls.open(w.srcA, w.safeA, lp, lane);
  const uint32_t* __restrict__ pre = J.lens;
  const uint32_t* __restrict__ suf = J.lens + n;
  for (uint32_t b0 = 0; b0 < n; b0 += 64) {
    const uint32_t m = n - b0 < 64 ? n - b0 : 64;
    const uint32_t i = b0 + lane;
    uint32_t ll = 0, ml = 0, off = 1;
    if (lane < m) {
      ll = suf[i];
      ml = i + 1 < n ? pre[i + 1] : 0u;
      off = ml ? pre[i] + ll : 1u;
    }
    uint32_t lits = 0;
    (void)w.replay<true>(ls, m, ll, ml, off, lp, false, lits);
    lp = rfl(lp + lits);
  }
  w.flush(true);
}

// the values of the pages in those encodings; one workgroup per (page, slice) — BYTE_STREAM_SPLIT and FIXED_LEN_BYTE_ARRAY from the arena
// are split like PLAIN fixed-width pages, the others run in slice 0
__global__ __launch_bounds__(256) void dv_values_ext_kernel(const DvChunkD* __restrict__ cds, const DvXJob* __restrict__ jobs) {
  __shared__ DvDeltaShared S;
  __shared__ uint64_t wt[4];
  const DvXJob J = jobs[blockIdx.x];
  const DvChunkD& C = cds[J.k];
  if (blockIdx.y >= C.slices) return;
  const uint32_t d = J.d, tid = threadIdx.x;
  const PqConv cv = C.cv;
  void* __restrict__ out = C.target;
  uint32_t* __restrict__ ctl = C.hdr;
  const DvPage P = C.pages[C.dp[d]];
  const uint32_t n = C.nn[d], vo = C.voff[d];
  const uint64_t o0 = C.vbase[d];
  if (n == 0) return;
  if (vo > P.uncomp_len || n > P.num_values || o0 + n > C.rows) { dv_fail(ctl, DV_CORRUPT); return; }
  const uint8_t* s = C.img + P.img_off + vo;
  const uint32_t rlen = P.uncomp_len - vo;
  const uint32_t lo = (uint32_t)((uint64_t)n * blockIdx.y / C.slices), hi = (uint32_t)((uint64_t)n * (blockIdx.y + 1) / C.slices);
  if (P.enc == ENC_BYTE_STREAM_SPLIT) {
    // a streaming transpose: lane-consecutive values read consecutive bytes of each of the w streams
    const uint32_t w = (uint32_t)plain_width(cv.physical, cv.type_length);
    if (w == 0 || rlen / w < n) { dv_fail(ctl, DV_CORRUPT); return; }
    for (uint32_t i = lo + tid; i < hi; i += 256) dv_store_bss(cv, s, n, i, out, o0 + i);
    return;
  }
  if (P.enc == ENC_DELTA_BYTE_ARRAY) {
    if (!J.live) return;   // not materialised: the chunk failed its checks (or its arena would be too large), decode reports it
    if (cv.physical == PT_FLBA) {
      const uint32_t w = (uint32_t)cv.type_length;
      for (uint32_t i = lo + tid; i < hi; i += 256) store_plain(cv, J.dst + (uint64_t)i * w, out, o0 + i);
      return;
    }
    if (blockIdx.y != 0) return;
    const uint32_t* __restrict__ pre = J.lens;
    const uint32_t* __restrict__ suf = J.lens + n;
    uint64_t carry = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 256) {
      const uint32_t i = c0 + tid;
      const uint32_t len = i < n ? pre[i] + suf[i] : 0u;
      uint64_t tot;
      const uint64_t x = carry + dv_block_xscan(len, wt, &tot);
      if (i < n) dv_view(J.dst + x, len, 1u, (uint32_t)(J.aoff + x), out, o0 + i);   // (the host keeps the arena below 4 GiB)
      carry += tot;
    }
    return;
  }
  // DELTA_LENGTH_BYTE_ARRAY: the lengths (DELTA_BINARY_PACKED) -> scratch, then the bytes of all values back to back: views into the page
  if (blockIdx.y != 0) return;
  uint32_t* __restrict__ lens = J.lens;
  bool bad = false;
  uint32_t e = 0;
  const bool ok = dv_delta_walk(s, rlen, n, true, &S, [&](uint32_t i, uint64_t v) { bad |= (int32_t)v < 0; lens[i] = (uint32_t)v; }, &e);
  if (__syncthreads_or(!ok || bad)) { dv_fail(ctl, DV_CORRUPT); return; }
  uint64_t sum = 0;
  for (uint32_t i = tid; i < n; i += 256) sum += lens[i];
  uint64_t total;
  (void)dv_block_xscan(sum, wt, &total);
  if (total > (uint64_t)(rlen - e)) { dv_fail(ctl, DV_CORRUPT); return; }
  const uint64_t base = P.img_off + vo + e;   // offset of the first value's bytes in the image (< 4 GiB: open checked)
  uint64_t carry = 0;
  for (uint32_t c0 = 0; c0 < n; c0 += 256) {
    const uint32_t i = c0 + tid;
    const uint32_t len = i < n ? lens[i] : 0u;
    uint64_t tot;
    const uint64_t x = carry + dv_block_xscan(len, wt, &tot);
    if (i < n) dv_view(s + e + x, len, 0u, (uint32_t)(base + x), out, o0 + i);
    carry += tot;
  }
}

int32_t dv_unsupported(const char* what) {
  set_error("dbhip_pq_chunk_open_device: %s (use dbhip_pq_chunk_open, or keep the CPU reader for this chunk)", what);
  return DBHIP_ERR_UNSUPPORTED;
}
int32_t dv_malformed(const char* what) {
  set_error("dbhip_pq_chunk_open_device: malformed column chunk: %s", what);
  return DBHIP_ERR_INVALID;
}

}  // namespace

extern "C" {

}  // extern "C"
namespace {
// list_mode: a List<primitive> leaf (one repeated ancestor): max_def_level = list_nullable + 1 + element_nullable, max_rep_level = 1
// nest_rep >= 0: a nested leaf (dbhip_pq_chunk_open_device_nested) with that many repeated levels; max_def_level is then the leaf's
int32_t open_device_impl(const uint8_t* chunk_host, int64_t chunk_len, int32_t codec, int32_t physical_type, int32_t type_length,
                         int32_t max_def_level, int32_t max_rep_level, int32_t out_type, bool list_mode, int32_t list_nullable, int32_t elem_nullable,
                         dbhip_pq_chunk** out_host, dbhip_pq_info* info_host, int32_t nest_rep = -1) {
  const bool nested = nest_rep >= 0;
  const bool lv_mode = list_mode || nested;     // rows = level entries, the leaf a nullable column over them
  DBHIP_REQUIRE(chunk_host && out_host && chunk_len >= 0, "dbhip_pq_chunk_open_device: NULL argument");
  *out_host = nullptr;
  if (codec != CODEC_NONE && codec != CODEC_SNAPPY && codec != CODEC_LZ4_RAW && codec != CODEC_ZSTD)
    return dv_unsupported("compression codec other than UNCOMPRESSED / SNAPPY / ZSTD / LZ4_RAW");
  if (!lv_mode && (max_rep_level != 0 || max_def_level < 0 || max_def_level > 1))
    return dv_unsupported("nested column (repetition / definition level > 1; List<primitive>: dbhip_pq_chunk_open_device_list)");
  const int32_t list_max_def = list_mode ? max_def_level : 0;
  const int32_t nest_max_def = nested ? max_def_level : 0;
  if (list_mode) max_def_level = 1;   // (for the flat pipeline the leaf is a nullable column over the level entries)
  if (nested) max_def_level = max_def_level > 0 ? 1 : 0;   // (no levels at all: every entry is a row with a value)
  if (chunk_len >= (1LL << 32)) return dv_unsupported("column chunk of 4 GiB or more");
  if (!type_pair_ok(physical_type, type_length, out_type)) {
    set_error("dbhip_pq_chunk_open_device: physical type %d (length %d) cannot be decoded into dbhip type %d", physical_type, type_length, out_type);
    return DBHIP_ERR_UNSUPPORTED;
  }
  dbhip_pq_chunk* c = new (std::nothrow) dbhip_pq_chunk();
  if (!c) { set_error("dbhip_pq_chunk_open_device: out of host memory"); return DBHIP_ERR_HIP; }
  c->device_mode = true; c->codec = codec;
  c->physical = physical_type; c->type_length = type_length; c->max_def = max_def_level; c->out_type = out_type;
  c->list = list_mode; c->list_nullable = list_nullable; c->elem_nullable = elem_nullable; c->list_max_def = list_max_def;
  c->nested = nested; c->n_lists = nested ? nest_rep : 0; c->nest_max_def = nest_max_def;
  c->chunk_len = chunk_len; c->rows = 0; c->nulls = -1; c->nonnull = 0; c->n_pages = 0;
  c->dict_n = -1; c->dict_off = 0; c->dict_bytes = 0;
  c->d_valid = nullptr; c->d_val = nullptr; c->d_str_off = nullptr; c->d_dict_str_off = nullptr; c->d_dict = nullptr; c->d_dense = nullptr;
  c->d_wcnt = nullptr; c->d_woff = nullptr; c->d_blk = nullptr; c->uploaded = false; c->n_val_small = 0;
  Rd r{chunk_host, chunk_host + chunk_len, true};
  int32_t rc = DBHIP_OK;
  uint64_t img = 0;
  bool all_v2_no_nulls = true;
  while (rc == DBHIP_OK && r.p < r.end) {
    PageHdr h;
    if (!read_page_header(r, h)) { rc = dv_malformed("page header"); break; }
    if ((uint64_t)h.compressed > (uint64_t)(r.end - r.p)) { rc = dv_malformed("page runs past the chunk"); break; }
    DvPage P{};
    P.type = (uint32_t)h.type;
    P.enc = (uint32_t)h.encoding;
    P.src_off = (uint64_t)(r.p - chunk_host);
    P.comp_len = (uint32_t)h.compressed;
    P.uncomp_len = (uint32_t)h.uncompressed;
    P.def_enc = (uint32_t)h.def_enc;
    const uint8_t* next = r.p + h.compressed;
    if (h.type == PG_DICT || h.type == PG_DATA || h.type == PG_DATA_V2) {
      if (h.num_values < 0) { rc = dv_malformed("page without num_values"); break; }
      P.num_values = (uint32_t)h.num_values;
      if (h.type == PG_DATA_V2) {
        if (h.rep_len != 0 && !list_mode && !(nested && nest_rep > 0)) { rc = nested ? dv_malformed("repetition levels in a leaf without a LIST") : dv_unsupported("repetition levels"); break; }
        if (h.def_len < 0 || h.rep_len < 0) { rc = dv_malformed("level byte length"); break; }
        P.rep_len = (uint32_t)h.rep_len;
        P.lev_len = (uint32_t)h.def_len + (uint32_t)h.rep_len;
        if (c->max_def == 0 && P.lev_len != 0) { rc = dv_malformed("definition levels in a required column"); break; }
        if (P.lev_len > P.comp_len || P.lev_len > P.uncomp_len) { rc = dv_malformed("level bytes exceed the page"); break; }
      }
      if (codec == CODEC_NONE) {
        if (h.compressed != h.uncompressed) { rc = dv_unsupported("compressed page in a chunk declared UNCOMPRESSED"); break; }
        P.compressed = 0;
        P.img_off = P.src_off;
      } else {
        P.compressed = (h.type == PG_DATA_V2) ? (h.v2_compressed ? 1u : 0u) : 1u;
        if (!P.compressed && h.compressed != h.uncompressed) { rc = dv_malformed("uncompressed page with differing sizes"); break; }
        img = (img + 15) & ~15ull;
        P.img_off = img;
        img += (uint64_t)P.uncomp_len;
      }
      if (h.type == PG_DICT) {
        if (c->dict_page >= 0 || c->n_pages > 0) { rc = dv_malformed("dictionary page not first / repeated"); break; }
        if (h.encoding != ENC_PLAIN && h.encoding != ENC_PLAIN_DICT) { rc = dv_unsupported("dictionary page encoding"); break; }
        if (c->physical == PT_BOOLEAN) { rc = dv_malformed("dictionary page"); break; }
        // (the dictionary is allocated on this count's word: every entry takes at least its PLAIN width / a length prefix in the page)
        const uint64_t per = c->physical == PT_BYTE_ARRAY ? 4 : (uint64_t)plain_width(c->physical, c->type_length);
        if (per == 0 || (uint64_t)h.num_values * per > (uint64_t)P.uncomp_len) { rc = dv_malformed("dictionary page shorter than its entries"); break; }
        c->dict_page = (int64_t)c->pages.size();
        c->dict_n = h.num_values;
      } else {
        const int e = h.encoding;
        const int pt = c->physical;
        const bool enc_ok = e == ENC_PLAIN || e == ENC_PLAIN_DICT || e == ENC_RLE_DICT || (e == ENC_RLE && pt == PT_BOOLEAN) ||
                            (e == ENC_DELTA_BINARY_PACKED && (pt == PT_INT32 || pt == PT_INT64)) ||
                            (e == ENC_DELTA_LENGTH_BYTE_ARRAY && pt == PT_BYTE_ARRAY) ||
                            (e == ENC_DELTA_BYTE_ARRAY && (pt == PT_BYTE_ARRAY || pt == PT_FLBA)) ||
                            (e == ENC_BYTE_STREAM_SPLIT && (pt == PT_FLOAT || pt == PT_DOUBLE || pt == PT_INT32 || pt == PT_INT64 || pt == PT_FLBA));
        if (!enc_ok) {
          rc = dv_unsupported("value encoding other than PLAIN / RLE_DICTIONARY / RLE (BOOLEAN) / DELTA_BINARY_PACKED (INT32, INT64) / "
                              "DELTA_LENGTH_BYTE_ARRAY (BYTE_ARRAY) / DELTA_BYTE_ARRAY (BYTE_ARRAY, FIXED_LEN_BYTE_ARRAY) / "
                              "BYTE_STREAM_SPLIT (FLOAT, DOUBLE, INT32, INT64, FIXED_LEN_BYTE_ARRAY)");
          break;
        }
        if ((e == ENC_PLAIN_DICT || e == ENC_RLE_DICT) && c->dict_page < 0) { rc = dv_malformed("dictionary-encoded page without a dictionary page"); break; }
        if (h.type == PG_DATA && c->max_def == 1 && h.def_enc != ENC_RLE) { rc = dv_unsupported("definition levels not RLE encoded"); break; }
        // List mode, v1 pages: dv_levels_kernel reads BOTH level streams as <4-byte length><RLE / bit-packed hybrid runs>; a legacy
        // BIT_PACKED stream (no length prefix) would be read as a length and runs
        if (list_mode && h.type == PG_DATA && (h.def_enc != ENC_RLE || h.rep_enc != ENC_RLE)) { rc = dv_unsupported("List column: definition / repetition levels not RLE encoded"); break; }
        if (nested && h.type == PG_DATA && nest_rep > 0 && h.rep_enc != ENC_RLE) { rc = dv_unsupported("nested leaf: repetition levels not RLE encoded"); break; }
        if ((uint64_t)c->rows + (uint64_t)P.num_values >= 0xFFFFFFF0ULL) { rc = dv_unsupported("more than 2^32 rows in one chunk"); break; }
        P.row_start = (uint64_t)c->rows;
        if (!(h.type == PG_DATA_V2 && h.num_nulls == 0) || lv_mode) all_v2_no_nulls = false;
        if (dv_ext_enc((uint32_t)e)) {
          c->n_ext += 1;
          if (e == ENC_DELTA_BYTE_ARRAY) { c->n_dba += 1; c->ext_lens += 2 * (int64_t)P.num_values; }
          else if (e == ENC_DELTA_LENGTH_BYTE_ARRAY) c->ext_lens += (int64_t)P.num_values;
        }
        c->data_pages.push_back((uint32_t)c->pages.size());
        c->nn_init.push_back(P.num_values);
        c->voff_init.push_back(h.type == PG_DATA_V2 ? P.lev_len : 0u);
        c->rows += (int64_t)P.num_values;
        c->n_pages += 1;
      }
      c->pages.push_back(P);
    }  // index pages and unknown page types are skipped
    r.p = next;
  }
  if (rc == DBHIP_OK && codec != CODEC_NONE) {
    if (img + 16 >= (1ULL << 32)) rc = dv_unsupported("column chunk that decompresses to 4 GiB or more");
    // the sizes come from untrusted headers: the caller allocates image_bytes of HBM on their word
    else if (img > (1ULL << 30) && img > 1024ULL * (uint64_t)chunk_len) rc = dv_malformed("declared uncompressed size out of proportion to the chunk");
  }
  if (rc) { delete c; return rc; }
  c->image_len = codec == CODEC_NONE ? 0 : (int64_t)img + 16;
  c->known_no_nulls = c->max_def == 0 || all_v2_no_nulls;
  if (c->known_no_nulls) { c->nulls = 0; c->nonnull = c->rows; }
  if (info_host) {
    info_host->num_values = c->rows;
    info_host->num_nulls = c->known_no_nulls ? 0 : -1;  // known after decode (dbhip_pq_chunk_decode_device's out_nulls_host)
    info_host->out_type = out_type;
    info_host->has_validity = c->max_def;
    info_host->out_bytes = out_type == DBHIP_T_BOOL ? ceil_div(c->rows, 64) * 8 : c->rows * (int64_t)out_elem_size(out_type);
    info_host->validity_bytes = ceil_div(c->rows, 64) * 8;
    info_host->n_pages = c->n_pages;
    info_host->n_dict_values = c->dict_n < 0 ? 0 : c->dict_n;
    info_host->image_bytes = c->image_len;
  }
  *out_host = c;
  return DBHIP_OK;
}
}  // namespace

extern "C" {

int32_t dbhip_pq_chunk_open_device(const uint8_t* chunk_host, int64_t chunk_len, int32_t codec, int32_t physical_type, int32_t type_length,
                                   int32_t max_def_level, int32_t max_rep_level, int32_t out_type, dbhip_pq_chunk** out_host,
                                   dbhip_pq_info* info_host) {
  return open_device_impl(chunk_host, chunk_len, codec, physical_type, type_length, max_def_level, max_rep_level, out_type, false, 0, 0, out_host, info_host);
}

int32_t dbhip_pq_chunk_open_device_list(const uint8_t* chunk_host, int64_t chunk_len, int32_t codec, int32_t physical_type, int32_t type_length,
                                        int32_t list_nullable, int32_t element_nullable, int32_t out_type, dbhip_pq_chunk** out_host,
                                        dbhip_pq_info* info_host) {
  DBHIP_REQUIRE((list_nullable == 0 || list_nullable == 1) && (element_nullable == 0 || element_nullable == 1), "dbhip_pq_chunk_open_device_list: nullability flags are 0 / 1");
  int32_t rc = open_device_impl(chunk_host, chunk_len, codec, physical_type, type_length, list_nullable + 1 + element_nullable, 1, out_type, true, list_nullable,
                                element_nullable, out_host, info_host);
  if (rc == DBHIP_OK && info_host) info_host->has_validity = element_nullable;   // (num_values = level entries: the bound of rows and of elements)
  return rc;
}

int32_t dbhip_pq_chunk_open_device_nested(const uint8_t* chunk_host, int64_t chunk_len, int32_t codec, int32_t physical_type, int32_t type_length,
                                          const dbhip_pq_node* path, int32_t n_nodes, int32_t leaf_nullable, int32_t out_type, dbhip_pq_chunk** out_host,
                                          dbhip_pq_info* info_host) {
  DBHIP_REQUIRE(out_host, "dbhip_pq_chunk_open_device_nested: NULL argument");
  *out_host = nullptr;
  DBHIP_REQUIRE(path, "dbhip_pq_chunk_open_device_nested: NULL path");
  DBHIP_REQUIRE(leaf_nullable == 0 || leaf_nullable == 1, "dbhip_pq_chunk_open_device_nested: leaf_nullable is 0 / 1");
  if (n_nodes < 1 || n_nodes > 8) {
    set_error("dbhip_pq_chunk_open_device_nested: %d path nodes (1 .. 8 are decoded)", n_nodes);
    return DBHIP_ERR_UNSUPPORTED;
  }
  int32_t lists = 0, max_def = leaf_nullable;
  for (int32_t j = 0; j < n_nodes; ++j) {
    DBHIP_REQUIRE(path[j].kind == PQ_NODE_LIST || path[j].kind == PQ_NODE_STRUCT, "dbhip_pq_chunk_open_device_nested: a node kind is LIST (1) or STRUCT (2)");
    DBHIP_REQUIRE(path[j].nullable == 0 || path[j].nullable == 1, "dbhip_pq_chunk_open_device_nested: node nullability is 0 / 1");
    lists += path[j].kind == PQ_NODE_LIST;
    max_def += path[j].nullable + (path[j].kind == PQ_NODE_LIST);
  }
  if (lists > 4) {
    set_error("dbhip_pq_chunk_open_device_nested: %d LIST nodes (at most 4 repeated levels are decoded)", lists);
    return DBHIP_ERR_UNSUPPORTED;
  }
  const int32_t rc = open_device_impl(chunk_host, chunk_len, codec, physical_type, type_length, max_def, lists, out_type, false, 0, 0, out_host, info_host, lists);
  if (rc != DBHIP_OK) return rc;
  dbhip_pq_chunk* c = *out_host;
  c->n_nodes = n_nodes; c->leaf_nullable = leaf_nullable;
  for (int32_t j = 0; j < n_nodes; ++j) { c->node_kind[j] = path[j].kind; c->node_null[j] = path[j].nullable; }
  if (info_host) info_host->has_validity = leaf_nullable;   // (num_values = level entries: the bound of rows, items and values)
  return DBHIP_OK;
}

}  // extern "C"

// ---- the batch: one launch set for many chunks ------------------------------------------------------------------------------
namespace {

struct BlobLayout {
  size_t hdr, cds, dict_list, lv_map, val_map, jobs, xjobs, per_chunk, total;
};
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

int32_t decode_many(dbhip_pq_chunk* const* cs, int32_t n, const uint8_t* const* chunk_dev, uint8_t* const* image_dev, void* const* out_values_dev,
                    uint8_t* const* out_validity_dev, int64_t* out_nulls_host, int32_t* out_status_host, void* stream, bool list_pass = false) {
  const char* who = "dbhip_pq_chunks_decode_device";
  if (n <= 0) return DBHIP_OK;
  hipStream_t s = resolve_stream(stream);
  // ---- checks + what has to be allocated once per chunk
  size_t n_jobs = 0, n_lv = 0, n_dp = 0, per_chunk = 0;
  size_t n_ext = 0, n_dba = 0, lens_words = 0;   // pages in DELTA_(LENGTH_)BYTE_ARRAY / BYTE_STREAM_SPLIT, of them DELTA_BYTE_ARRAY, scratch for lengths
  std::vector<int> live;      // chunks with rows
  for (int i = 0; i < n; ++i) {
    dbhip_pq_chunk* c = cs[i];
    if (out_nulls_host) out_nulls_host[i] = 0;
    if (out_status_host) out_status_host[i] = DBHIP_OK;
    DBHIP_REQUIRE(c && c->device_mode, "dbhip_pq_chunk_decode_device: the handle was not opened by dbhip_pq_chunk_open_device");
    DBHIP_REQUIRE(!c->list || list_pass, "dbhip_pq_chunk_decode_device: a List chunk is decoded by dbhip_pq_chunk_decode_device_list");
    DBHIP_REQUIRE(!c->nested || list_pass, "dbhip_pq_chunk_decode_device: a nested leaf is decoded by dbhip_pq_chunk_decode_device_nested");
    // the arena of the previous decode, if the caller did not take it (dbhip_pq_chunk_take_arena)
    if (c->d_arena) { (void)dbhip_free(c->d_arena); c->d_arena = nullptr; c->arena_bytes = 0; }
    if (c->rows == 0) continue;
    n_ext += (size_t)c->n_ext; n_dba += (size_t)c->n_dba; lens_words += (size_t)c->ext_lens;
    DBHIP_REQUIRE(chunk_dev[i] && out_values_dev[i], "dbhip_pq_chunk_decode_device: NULL buffer");
    DBHIP_REQUIRE(((uintptr_t)chunk_dev[i] & 15) == 0, "dbhip_pq_chunk_decode_device: chunk_dev must be 16-byte aligned");
    DBHIP_REQUIRE(c->codec == CODEC_NONE || image_dev[i], "dbhip_pq_chunk_decode_device: a compressed chunk needs an image buffer (info.image_bytes)");
    DBHIP_REQUIRE(c->codec == CODEC_NONE || ((uintptr_t)image_dev[i] & 15) == 0, "dbhip_pq_chunk_decode_device: the image buffer must be 16-byte aligned");
    DBHIP_REQUIRE(c->max_def == 0 || out_validity_dev[i], "dbhip_pq_chunk_decode_device: a nullable column needs a validity buffer");
    live.push_back(i);
    const size_t nd = c->data_pages.size();
    if (c->codec != CODEC_NONE) n_jobs += c->pages.size();
    if (c->max_def == 1) n_lv += nd;
    n_dp += nd;
    per_chunk += up16(c->pages.size() * sizeof(DvPage)) + 3 * up16(nd * 4) + up16((nd + 1) * 8);
    const int esize = out_elem_size(c->out_type);
    const bool is_bool = c->out_type == DBHIP_T_BOOL;
    const bool spread = c->max_def == 1 && !c->known_no_nulls;
    const int64_t nwords = ceil_div(c->rows, 32);
    if (c->dict_n > 0 && !c->d_dict) DBHIP_TRY(dbhip_alloc((size_t)c->dict_n * (size_t)esize, &c->d_dict));
    if (spread) {
      if (!c->d_dense) DBHIP_TRY(dbhip_alloc(is_bool ? (size_t)ceil_div(c->rows + 1, 64) * 8 : (size_t)(c->rows + 1) * (size_t)esize, &c->d_dense));
      if (!c->d_wcnt) DBHIP_TRY(dbhip_alloc((size_t)nwords * 4, (void**)&c->d_wcnt));
      if (!c->d_woff) DBHIP_TRY(dbhip_alloc((size_t)nwords * 8, (void**)&c->d_woff));
      if (!c->d_blk) DBHIP_TRY(dbhip_alloc((size_t)(ceil_div(nwords, SCAN_TILE) + 2) * 8, (void**)&c->d_blk));
    }
  }
  if (live.empty()) return DBHIP_OK;
  static const bool lds_ok = [] {
    return hipFuncSetAttribute((const void*)dv_inflate_lz_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LZ_RING) == hipSuccess &&
           hipFuncSetAttribute((const void*)dv_inflate_zstd2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ZW2_LDS) == hipSuccess &&
           hipFuncSetAttribute((const void*)dv_dba_replay_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LZ_RING) == hipSuccess;
  }();
  if (!lds_ok) { set_error("%s: cannot reserve LDS for the decompression kernels", who); return DBHIP_ERR_HIP; }
  // ---- the blob: everything the kernels read about the batch, one upload
  const size_t nl = live.size();
  BlobLayout L;
  L.hdr = 0;
  L.cds = up16(nl * 32);
  L.dict_list = L.cds + up16(nl * sizeof(DvChunkD));
  L.lv_map = L.dict_list + up16(nl * 4);
  L.val_map = L.lv_map + up16(n_lv * 8);
  L.jobs = L.val_map + up16(n_dp * 8);
  L.xjobs = L.jobs + up16(n_jobs * sizeof(DvJob));
  L.per_chunk = L.xjobs + up16(n_ext * sizeof(DvXJob));
  L.total = L.per_chunk + per_chunk;
  uint8_t* blob = (uint8_t*)scratch(L.total, 20, s);
  if (!blob) { set_error("%s: out of device memory (%zu bytes of page tables)", who, L.total); return DBHIP_ERR_HIP; }
  uint32_t* lens = nullptr;
  if (lens_words) {
    lens = (uint32_t*)scratch(lens_words * 4 + 64, 21, s);
    if (!lens) { set_error("%s: out of device memory (%zu bytes of string lengths)", who, lens_words * 4); return DBHIP_ERR_HIP; }
  }
  std::vector<uint8_t> H(L.total, 0);
  DvChunkD* cds = (DvChunkD*)(H.data() + L.cds);
  uint32_t* dict_list = (uint32_t*)(H.data() + L.dict_list);
  uint2* lv_map = (uint2*)(H.data() + L.lv_map);
  uint2* val_map = (uint2*)(H.data() + L.val_map);
  DvJob* jobs = (DvJob*)(H.data() + L.jobs);
  DvXJob* xjobs = (DvXJob*)(H.data() + L.xjobs);   // DELTA_BYTE_ARRAY pages first
  size_t at = L.per_chunk, n_dict = 0, k_lv = 0, k_dp = 0, k_dba = 0, k_x = n_dba, lens_at = 0;
  unsigned max_slices_x = 1;
  // jobs: ZSTD pages first (their own kernel), then Snappy / LZ4
  size_t n_z = 0;
  for (int i : live)
    if (cs[i]->codec == CODEC_ZSTD) n_z += cs[i]->pages.size();
  size_t jz = 0, jo = n_z;
  bool any_list = false, any_nested = false;
  unsigned max_slices = 1;
  for (size_t k = 0; k < nl; ++k) {
    const int i = live[k];
    dbhip_pq_chunk* c = cs[i];
    const uint32_t nd = (uint32_t)c->data_pages.size();
    const int esize = out_elem_size(c->out_type);
    const bool spread = c->max_def == 1 && !c->known_no_nulls;
    DvChunkD& D = cds[k];
    auto place = [&](const void* src, size_t bytes) {
      const size_t o = at;
      if (src && bytes) memcpy(H.data() + o, src, bytes);
      at += up16(bytes);
      return blob + o;
    };
    D.pages = (const DvPage*)place(c->pages.data(), c->pages.size() * sizeof(DvPage));
    D.dp = (const uint32_t*)place(c->data_pages.data(), (size_t)nd * 4);
    D.nn = (uint32_t*)place(c->nn_init.data(), (size_t)nd * 4);
    D.voff = (uint32_t*)place(c->voff_init.data(), (size_t)nd * 4);
    D.vbase = (uint64_t*)place(nullptr, (size_t)(nd + 1) * 8);
    D.img = c->codec == CODEC_NONE ? chunk_dev[i] : image_dev[i];
    D.dict = c->d_dict; D.dict_out = c->d_dict;
    D.target = spread ? c->d_dense : out_values_dev[i];
    D.bitmap = (uint32_t*)out_validity_dev[i];
    D.hdr = (uint32_t*)(blob + L.hdr + k * 32);
    D.cv = PqConv{c->physical, c->type_length, c->out_type, esize};
    D.dict_n = (uint32_t)(c->dict_n > 0 ? c->dict_n : 0);
    D.dict_page = (uint32_t)(c->dict_page >= 0 ? c->dict_page : 0);
    D.nd = nd;
    D.rows = (uint64_t)c->rows;
    // slices of a PLAIN fixed-width page: enough workgroups to fill the chip even from a few large pages
    unsigned slices = 1;
    const bool fixed = c->physical != PT_BOOLEAN && c->physical != PT_BYTE_ARRAY;
    if (fixed && nd > 0) {
      const int64_t per_page = c->rows / (int64_t)nd;
      while (slices < 64 && (int64_t)n_dp * slices < 2048 && per_page / (int64_t)slices > 4096) slices <<= 1;
    }
    D.slices = slices;
    if (slices > max_slices) max_slices = slices;
    if (c->list) {
      any_list = true;
      D.ldw = c->list_max_def > 1 ? 2u : 1u; D.lmax = (uint32_t)c->list_max_def; D.lnull = (uint32_t)c->list_nullable;
      D.isrep = c->d_isrep; D.iselem = c->d_iselem; D.lvalid = c->d_lvalid;
      D.rw = 1; D.rmax = 1;
    } else if (c->nested) {
      any_list = true; any_nested = true;
      D.ldw = bit_width_u32((uint32_t)c->nest_max_def); D.lmax = (uint32_t)c->nest_max_def;
      D.rw = bit_width_u32((uint32_t)c->n_lists); D.rmax = (uint32_t)c->n_lists;
      D.lrep = c->d_lrep; D.ldef = c->d_ldef;
    }
    if (c->dict_n > 0) dict_list[n_dict++] = (uint32_t)k;
    for (uint32_t d = 0; d < nd; ++d) {
      if (c->max_def == 1) lv_map[k_lv++] = make_uint2((unsigned)k, d);
      if (c->n_ext == 0 || !dv_ext_enc(c->pages[c->data_pages[d]].enc)) { val_map[k_dp++] = make_uint2((unsigned)k, d); continue; }
      const DvPage& P = c->pages[c->data_pages[d]];
      DvXJob& X = P.enc == ENC_DELTA_BYTE_ARRAY ? xjobs[k_dba++] : xjobs[k_x++];
      X.k = (uint32_t)k; X.d = d; X.enc = P.enc;
      if (P.enc != ENC_BYTE_STREAM_SPLIT) {
        X.lens = lens + lens_at;
        lens_at += (P.enc == ENC_DELTA_BYTE_ARRAY ? 2 : 1) * (size_t)P.num_values;
      }
      if (slices > max_slices_x) max_slices_x = slices;
    }
    if (c->codec != CODEC_NONE) {
      const uint64_t safe_end = ((uint64_t)c->chunk_len + 15) & ~15ull;   // chunk_dev is readable up to here
      for (const DvPage& P : c->pages) {
        DvJob& J = c->codec == CODEC_ZSTD ? jobs[jz++] : jobs[jo++];
        J.src = chunk_dev[i] + P.src_off;
        J.dst = image_dev[i] + P.img_off;
        J.comp_len = P.comp_len; J.uncomp_len = P.uncomp_len; J.lev_len = P.lev_len; J.compressed = P.compressed;
        J.src_safe = (uint32_t)(safe_end - P.src_off);
        J.codec = (uint32_t)c->codec;
        J.ctl = D.hdr;
      }
    }
  }
  // the longest pages first: a page is one wave's serial work, the short ones fill the slots the long ones leave
  auto by_size = [](const DvJob& a, const DvJob& b) { return a.uncomp_len > b.uncomp_len; };
  std::sort(jobs, jobs + n_z, by_size);
  std::sort(jobs + n_z, jobs + n_jobs, by_size);
  DBHIP_CHECK(hipMemcpyAsync(blob, H.data(), L.total, hipMemcpyHostToDevice, s));
  const DvChunkD* d_cds = (const DvChunkD*)(blob + L.cds);
  const DvJob* d_jobs = (const DvJob*)(blob + L.jobs);
  // validity / BOOLEAN targets start from zero (the kernels OR bits in)
  for (int i : live) {
    dbhip_pq_chunk* c = cs[i];
    const bool spread = c->max_def == 1 && !c->known_no_nulls;
    uint32_t* vbits = (uint32_t*)out_validity_dev[i];
    if (c->max_def == 1) DBHIP_CHECK(hipMemsetAsync(vbits, 0, (size_t)ceil_div(c->rows, 64) * 8, s));
    else if (vbits) DBHIP_CHECK(hipMemsetAsync(vbits, 0xFF, (size_t)ceil_div(c->rows, 64) * 8, s));
    if (c->out_type == DBHIP_T_BOOL)
      DBHIP_CHECK(hipMemsetAsync(spread ? c->d_dense : out_values_dev[i], 0, (size_t)ceil_div(spread ? c->rows + 1 : c->rows, 64) * 8, s));
  }
  kernel_timer_start(s);
  // ring sizes (dv_wave.h): smaller rings = more pages resident per CU, more back-references served from the image instead of the ring.
  // ZSTD: two waves per page — parse | copy
  if (n_z) hipLaunchKernelGGL(dv_inflate_zstd2_kernel, dim3((unsigned)n_z), dim3(128), ZW2_LDS, s, d_jobs, ZW_RING);
  if (n_jobs > n_z) hipLaunchKernelGGL(dv_inflate_lz_kernel, dim3((unsigned)(n_jobs - n_z)), dim3(64), LZ_RING, s, d_jobs + n_z, LZ_RING);
  if (n_dict) hipLaunchKernelGGL(dv_dict_kernel, dim3((unsigned)n_dict), dim3(256), 0, s, d_cds, (const uint32_t*)(blob + L.dict_list));
  if (n_lv && any_nested)   // (a nested leaf is decoded alone: dbhip_pq_chunks_decode_device refuses its handle)
    hipLaunchKernelGGL(dv_levels_kernel<true>, dim3((unsigned)n_lv), dim3(256), LV_LDS, s, d_cds, (const uint2*)(blob + L.lv_map), LV_LDS);
  else if (n_lv)
    hipLaunchKernelGGL(dv_levels_kernel<false>, dim3((unsigned)n_lv), dim3(256), any_list ? LV_LDS : 0u, s, d_cds, (const uint2*)(blob + L.lv_map), any_list ? LV_LDS : 0u);
  hipLaunchKernelGGL(dv_scan_kernel, dim3((unsigned)nl), dim3(256), 0, s, d_cds);
  if (k_dp) hipLaunchKernelGGL(dv_values_kernel, dim3((unsigned)k_dp, max_slices), dim3(256), 0, s, d_cds, (const uint2*)(blob + L.val_map));
  // DELTA_BYTE_ARRAY: size every page, read the sizes back (the one extra read-back, only for batches that hold such pages), give each chunk
  // one arena, replay the values into it
  DvXJob* d_xjobs = (DvXJob*)(blob + L.xjobs);
  std::vector<uint8_t> arena_unsupported(nl, 0);
  if (n_dba) {
    hipLaunchKernelGGL(dv_dba_size_kernel, dim3((unsigned)n_dba), dim3(256), 0, s, d_cds, d_xjobs);
    DBHIP_LAUNCH_CHECK();
    std::vector<uint32_t> hdr0(nl * 8, 0);
    DBHIP_CHECK(hipMemcpyAsync(hdr0.data(), blob + L.hdr, nl * 32, hipMemcpyDeviceToHost, s));
    DBHIP_CHECK(hipMemcpyAsync(xjobs, d_xjobs, n_dba * sizeof(DvXJob), hipMemcpyDeviceToHost, s));
    DBHIP_CHECK(hipStreamSynchronize(s));
    std::vector<uint64_t> total(nl, 0);
    for (size_t j = 0; j < n_dba; ++j) {
      const uint32_t k = xjobs[j].k;
      if (xjobs[j].bytes >= (1ull << 31)) arena_unsupported[k] = 1;   // (ZWave's replay keeps a page's output below 2^31 bytes)
      xjobs[j].aoff = total[k];
      total[k] += xjobs[j].bytes;
    }
    for (size_t k = 0; k < nl; ++k) {
      if (total[k] >= (1ull << 32)) arena_unsupported[k] = 1;         // views carry 32-bit offsets
      if (total[k] == 0 || hdr0[k * 8] != DV_OK || arena_unsupported[k]) continue;
      dbhip_pq_chunk* c = cs[live[k]];
      DBHIP_TRY(dbhip_alloc((size_t)total[k] + 16, &c->d_arena));
      c->arena_bytes = (int64_t)total[k];
    }
    for (size_t j = 0; j < n_dba; ++j) {
      const uint32_t k = xjobs[j].k;
      dbhip_pq_chunk* c = cs[live[k]];
      xjobs[j].live = hdr0[k * 8] == DV_OK && !arena_unsupported[k];
      xjobs[j].dst = c->d_arena ? (uint8_t*)c->d_arena + xjobs[j].aoff : nullptr;   // (no arena: every value of the chunk is empty)
    }
    DBHIP_CHECK(hipMemcpyAsync(d_xjobs, xjobs, n_dba * sizeof(DvXJob), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(dv_dba_replay_kernel, dim3((unsigned)n_dba), dim3(64), LZ_RING, s, d_cds, (const DvXJob*)d_xjobs, LZ_RING);
  }
  if (n_ext) hipLaunchKernelGGL(dv_values_ext_kernel, dim3((unsigned)n_ext, max_slices_x), dim3(256), 0, s, d_cds, (const DvXJob*)d_xjobs);
  for (int i : live) {
    dbhip_pq_chunk* c = cs[i];
    if (!(c->max_def == 1 && !c->known_no_nulls)) continue;
    const int esize = out_elem_size(c->out_type);
    const int64_t nwords = ceil_div(c->rows, 32);
    uint32_t* vbits = (uint32_t*)out_validity_dev[i];
    void* out = out_values_dev[i];
    hipLaunchKernelGGL(pq_popc_kernel, dim3(grid_for(nwords, 256)), dim3(256), 0, s, vbits, nwords, c->d_wcnt);
    DBHIP_TRY(dbscan::exclusive_scan_u32(c->d_wcnt, nwords, c->d_blk, c->d_woff, s));
    const int grid = grid_for(c->rows, 256);
    if (c->out_type == DBHIP_T_BOOL) {
      hipLaunchKernelGGL(pq_spread_bool_kernel, dim3(grid_for(nwords, 256)), dim3(256), 0, s, vbits, c->d_woff, (const uint32_t*)c->d_dense, nwords, (uint32_t*)out);
      if (nwords & 1) DBHIP_CHECK(hipMemsetAsync((uint32_t*)out + nwords, 0, 4, s));
    } else if (esize == 1) {
      hipLaunchKernelGGL(pq_spread_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, vbits, c->d_woff, (const uint8_t*)c->d_dense, c->rows, (uint8_t*)out);
    } else if (esize == 2) {
      hipLaunchKernelGGL(pq_spread_kernel<uint16_t>, dim3(grid), dim3(256), 0, s, vbits, c->d_woff, (const uint16_t*)c->d_dense, c->rows, (uint16_t*)out);
    } else if (esize == 4) {
      hipLaunchKernelGGL(pq_spread_kernel<uint32_t>, dim3(grid), dim3(256), 0, s, vbits, c->d_woff, (const uint32_t*)c->d_dense, c->rows, (uint32_t*)out);
    } else if (esize == 8) {
      hipLaunchKernelGGL(pq_spread_kernel<uint64_t>, dim3(grid), dim3(256), 0, s, vbits, c->d_woff, (const uint64_t*)c->d_dense, c->rows, (uint64_t*)out);
    } else {
      hipLaunchKernelGGL(pq_spread_kernel<uint4>, dim3(grid), dim3(256), 0, s, vbits, c->d_woff, (const uint4*)c->d_dense, c->rows, (uint4*)out);
    }
  }
  kernel_timer_stop(s);
  DBHIP_LAUNCH_CHECK();
  // the verdict of the device-side checks (and the null counts) is only known once the kernels ran: one read-back for the batch
  std::vector<uint32_t> hdr(nl * 8, 0);
  DBHIP_CHECK(hipMemcpyAsync(hdr.data(), blob + L.hdr, nl * 32, hipMemcpyDeviceToHost, s));
  DBHIP_CHECK(hipStreamSynchronize(s));
  int32_t first_rc = DBHIP_OK;
  for (size_t k = 0; k < nl; ++k) {
    const int i = live[k];
    dbhip_pq_chunk* c = cs[i];
    const uint32_t verdict = hdr[k * 8];
    uint64_t nonnull;
    memcpy(&nonnull, &hdr[k * 8 + 2], 8);
    int32_t rc = DBHIP_OK;
    if (verdict == DV_OK && arena_unsupported[k]) {
      set_error("dbhip_pq_chunk_decode_device: chunk %d: its DELTA_BYTE_ARRAY values take 4 GiB or more (or 2 GiB or more in one page); "
                "use the CPU reader for this chunk", i);
      rc = DBHIP_ERR_UNSUPPORTED;
    } else if (verdict == DV_UNSUPPORTED) {
      set_error("dbhip_pq_chunk_decode_device: chunk %d uses a form the device path does not decode (a Snappy back-reference beyond 64 KiB, a ZSTD "
                "dictionary, or an encoding that changes between pages); use dbhip_pq_chunk_open", i);
      rc = DBHIP_ERR_UNSUPPORTED;
    } else if (verdict != DV_OK) {
      set_error("dbhip_pq_chunk_decode_device: malformed column chunk %d (a page does not decompress to its declared size, or a level / index / "
                "length stream runs past its page)", i);
      rc = DBHIP_ERR_INVALID;
    } else if (c->known_no_nulls && (int64_t)nonnull != c->rows) {
      set_error("dbhip_pq_chunk_decode_device: malformed column chunk %d (the pages say num_nulls = 0, the definition levels disagree)", i);
      rc = DBHIP_ERR_INVALID;
    } else {
      c->nonnull = (int64_t)nonnull;
      c->nulls = c->rows - c->nonnull;
      if (out_nulls_host) out_nulls_host[i] = c->nulls;
    }
    if (rc && c->d_arena) { (void)dbhip_free(c->d_arena); c->d_arena = nullptr; c->arena_bytes = 0; }
    if (out_status_host) out_status_host[i] = rc;
    if (rc && !first_rc) first_rc = rc;
  }
  return first_rc;
}

}  // namespace

namespace {
// ---- List<primitive> (round 5; the reference reads nested columns through arrow-rs, deserialize.rs:33-81) ---------------------------
// per 32-entry word: rows that start in it (entries that do not continue a row) and element slots in it
__global__ __launch_bounds__(256) void pq_list_count_kernel(const uint32_t* __restrict__ isrep, const uint32_t* __restrict__ iselem, int64_t entries, int64_t nwords,
                                                            uint32_t* __restrict__ rcnt, uint32_t* __restrict__ ecnt) {
  for (int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x; w < nwords; w += (int64_t)gridDim.x * 256) {
    const int64_t left = entries - w * 32;
    const uint32_t live = left >= 32 ? 0xFFFFFFFFu : ((1u << (uint32_t)left) - 1u);
    rcnt[w] = (uint32_t)__popc(~isrep[w] & live);
    ecnt[w] = (uint32_t)__popc(iselem[w] & live);
  }
}
// entry e: an element slot -> its value moves to the element's place (+ its validity bit); a row start -> offsets[row] = elements before it
// (+ the list's validity bit). counts: [0] rows, [1] elements, [2] NULL lists, [3] != 0: the first entry continues a row (malformed)
// bit `rank` of `bitmap` := 1 for the lanes with `set`; the ranks of a wave's setting lanes lie within 64 of each other. Called by whole
// waves (lanes past the end of the data call it with set = false).
__device__ __forceinline__ void list_put_bits(uint32_t* __restrict__ bitmap, bool set, uint64_t rank) {
  const uint64_t any = __ballot(set);
  if (any == 0) return;
  if (__ballot(true) != ~0ull) {   // (the last, partial wave of the data: its idle lanes hold nothing a shuffle may read)
    if (set) atomicOr(&bitmap[rank >> 5], 1u << (uint32_t)(rank & 31));
    return;
  }
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r0 = __shfl(rank, (int)__ffsll((long long)any) - 1, 64);      // the lowest rank: ranks grow with the lane
  const uint64_t w0 = r0 >> 5;
  const uint32_t pos = set ? (uint32_t)(rank - (w0 << 5)) : 0u;                 // 0 .. 95
  uint32_t m0 = set && pos < 32 ? 1u << pos : 0u, m1 = set && pos >= 32 && pos < 64 ? 1u << (pos - 32) : 0u, m2 = set && pos >= 64 ? 1u << (pos - 64) : 0u;
  for (int d = 32; d >= 1; d >>= 1) {
    m0 |= (uint32_t)__shfl_xor((int)m0, d, 64);
    m1 |= (uint32_t)__shfl_xor((int)m1, d, 64);
    m2 |= (uint32_t)__shfl_xor((int)m2, d, 64);
  }
  const uint32_t m = lane == 0 ? m0 : lane == 1 ? m1 : m2;
  if (lane < 3 && m) atomicOr(&bitmap[w0 + lane], m);
}

template <typename V>
__global__ __launch_bounds__(256) void pq_list_finish_kernel(int64_t entries, const uint32_t* __restrict__ isrep, const uint32_t* __restrict__ iselem,
                                                             const uint32_t* __restrict__ lvalid, const uint32_t* __restrict__ valid,
                                                             const uint64_t* __restrict__ roff, const uint64_t* __restrict__ eoff, const V* __restrict__ ent_values,
                                                             uint64_t* __restrict__ out_offsets, uint32_t* __restrict__ out_lvalid, V* __restrict__ out_values,
                                                             uint32_t* __restrict__ out_evalid, unsigned long long* __restrict__ counts, int move_values) {
  uint32_t wave_nulls = 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < entries; e += (int64_t)gridDim.x * 256) {
    const int64_t w = e >> 5;
    const uint32_t b = (uint32_t)(e & 31), below = (1u << b) - 1u, bit = 1u << b;
    const uint32_t rep = isrep[w], el = iselem[w];
    const uint64_t erank = eoff[w] + (uint32_t)__popc(el & below);
    bool ev = false, lv = false;
    if (el & bit) {
      if (move_values) out_values[erank] = ent_values[e];
      ev = out_evalid && (valid[w] & bit);
    }
    bool null_list = false;
    uint64_t rrank = 0;
    if (!(rep & bit)) {
      rrank = roff[w] + (uint32_t)__popc(~rep & below);
      out_offsets[rrank] = erank;
      if (lvalid) {
        if (lvalid[w] & bit) lv = out_lvalid != nullptr;
        else null_list = true;
      }
    } else if (e == 0) counts[3] = 1;
    // The validity bits of a wave's 64 entries land in at most three consecutive words of each output bitmap (the ranks of the wave's
    // elements / rows are consecutive): the wave ORs them together and lanes 0..2 put the words — one atomic per entry on two or three
    // words was most of this kernel's 3.1 ms per 20 M entries.
    list_put_bits(out_evalid, ev, erank);
    list_put_bits(out_lvalid, lv, rrank);
    wave_nulls += (uint32_t)__popcll(__ballot(null_list));
    if (e == entries - 1) {
      const uint64_t rows = roff[w] + (uint32_t)__popc(~rep & (below | bit));
      const uint64_t elems = erank + ((el & bit) ? 1 : 0);
      out_offsets[rows] = elems;
      counts[0] = rows; counts[1] = elems;
    }
  }
  // the NULL lists: ONE add per workgroup on the counter, and a grid of at most 2 048 workgroups — adds on one word are serialised in L2
  // (round 5: one per entry, 480 K; then one per wave and iteration, 320 K: still the 3 ms this kernel took for 20 M entries)
  __shared__ uint32_t wn[4];
  if ((threadIdx.x & 63u) == 0) wn[threadIdx.x >> 6] = wave_nulls;
  __syncthreads();
  if (threadIdx.x == 0 && wn[0] + wn[1] + wn[2] + wn[3]) atomicAdd(&counts[2], (unsigned long long)(wn[0] + wn[1] + wn[2] + wn[3]));
}
// BOOLEAN elements: the values are a bitmap over the entries
__global__ __launch_bounds__(256) void pq_list_finish_bool_kernel(int64_t entries, const uint32_t* __restrict__ iselem, const uint64_t* __restrict__ eoff,
                                                                  const uint32_t* __restrict__ ent_bits, uint32_t* __restrict__ out_bits) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < entries; e += (int64_t)gridDim.x * 256) {
    const int64_t w = e >> 5;
    const uint32_t b = (uint32_t)(e & 31), bit = 1u << b;
    if ((iselem[w] & bit) && (ent_bits[w] & bit)) {
      const uint64_t erank = eoff[w] + (uint32_t)__popc(iselem[w] & (bit - 1u));
      atomicOr(&out_bits[erank >> 5], 1u << (uint32_t)(erank & 31));
    }
  }
}

int32_t decode_list(dbhip_pq_chunk* c, const uint8_t* chunk_dev, uint8_t* image_dev, uint64_t* out_offsets_dev, uint8_t* out_list_validity_dev,
                    void* out_values_dev, uint8_t* out_elem_validity_dev, int64_t* out_rows_host, int64_t* out_elems_host, int64_t* out_null_lists_host,
                    void* stream) {
  const char* who = "dbhip_pq_chunk_decode_device_list";
  DBHIP_REQUIRE(c && c->device_mode && c->list, "dbhip_pq_chunk_decode_device_list: the handle was not opened by dbhip_pq_chunk_open_device_list");
  DBHIP_REQUIRE(out_offsets_dev && out_rows_host && out_elems_host, "dbhip_pq_chunk_decode_device_list: NULL argument");
  DBHIP_REQUIRE(!c->list_nullable || out_list_validity_dev, "dbhip_pq_chunk_decode_device_list: a nullable list needs a validity buffer");
  DBHIP_REQUIRE(!c->elem_nullable || out_elem_validity_dev, "dbhip_pq_chunk_decode_device_list: nullable elements need a validity buffer");
  hipStream_t s = resolve_stream(stream);
  *out_rows_host = 0; *out_elems_host = 0;
  if (out_null_lists_host) *out_null_lists_host = 0;
  const int64_t entries = c->rows;
  if (entries == 0) { DBHIP_CHECK(hipMemsetAsync(out_offsets_dev, 0, 8, s)); DBHIP_CHECK(hipStreamSynchronize(s)); return DBHIP_OK; }
  DBHIP_REQUIRE(out_values_dev, "dbhip_pq_chunk_decode_device_list: NULL values buffer");
  const int esize = out_elem_size(c->out_type);
  const bool is_bool = c->out_type == DBHIP_T_BOOL;
  const int64_t nwords = ceil_div(entries, 32), wbytes = ceil_div(entries, 64) * 8;
  // (each buffer behind its own check: an allocation that fails part way leaves the handle retryable, not half-built)
  if (!c->d_isrep) DBHIP_TRY(dbhip_alloc((size_t)wbytes, (void**)&c->d_isrep));
  if (!c->d_iselem) DBHIP_TRY(dbhip_alloc((size_t)wbytes, (void**)&c->d_iselem));
  if (!c->d_lvalid) DBHIP_TRY(dbhip_alloc((size_t)wbytes, (void**)&c->d_lvalid));
  if (!c->d_ent_valid) DBHIP_TRY(dbhip_alloc((size_t)wbytes, (void**)&c->d_ent_valid));
  if (!c->d_ent_values) DBHIP_TRY(dbhip_alloc(is_bool ? (size_t)wbytes : (size_t)entries * (size_t)esize, &c->d_ent_values));
  if (!c->d_rcnt) DBHIP_TRY(dbhip_alloc((size_t)nwords * 4, (void**)&c->d_rcnt));
  if (!c->d_ecnt) DBHIP_TRY(dbhip_alloc((size_t)nwords * 4, (void**)&c->d_ecnt));
  if (!c->d_roff) DBHIP_TRY(dbhip_alloc((size_t)nwords * 8, (void**)&c->d_roff));
  if (!c->d_eoff) DBHIP_TRY(dbhip_alloc((size_t)nwords * 8, (void**)&c->d_eoff));
  if (!c->d_lblk) DBHIP_TRY(dbhip_alloc((size_t)(ceil_div(nwords, SCAN_TILE) + 2) * 8, (void**)&c->d_lblk));
  if (!c->d_lcounts) DBHIP_TRY(dbhip_alloc(64, (void**)&c->d_lcounts));
  DBHIP_CHECK(hipMemsetAsync(c->d_isrep, 0, (size_t)wbytes, s));
  DBHIP_CHECK(hipMemsetAsync(c->d_iselem, 0, (size_t)wbytes, s));
  DBHIP_CHECK(hipMemsetAsync(c->d_lvalid, 0, (size_t)wbytes, s));
  DBHIP_CHECK(hipMemsetAsync(c->d_lcounts, 0, 64, s));
  // the leaf as a nullable column over the level entries (the flat pipeline; its levels kernel fills the entry bitmaps)
  void* ent_values = c->d_ent_values;
  uint8_t* ent_valid = (uint8_t*)c->d_ent_valid;
  int64_t nulls = 0;
  int32_t rc = decode_many(&c, 1, &chunk_dev, &image_dev, &ent_values, &ent_valid, &nulls, nullptr, stream, true);
  if (rc) return rc;
  // entries -> rows and elements
  hipLaunchKernelGGL(pq_list_count_kernel, dim3(grid_for(nwords, 256)), dim3(256), 0, s, c->d_isrep, c->d_iselem, entries, nwords, c->d_rcnt, c->d_ecnt);
  DBHIP_TRY(dbscan::exclusive_scan_u32(c->d_rcnt, nwords, c->d_lblk, c->d_roff, s));
  DBHIP_TRY(dbscan::exclusive_scan_u32(c->d_ecnt, nwords, c->d_lblk, c->d_eoff, s));
  if (out_list_validity_dev) DBHIP_CHECK(hipMemsetAsync(out_list_validity_dev, c->list_nullable ? 0 : 0xFF, (size_t)wbytes, s));
  if (out_elem_validity_dev) DBHIP_CHECK(hipMemsetAsync(out_elem_validity_dev, c->elem_nullable ? 0 : 0xFF, (size_t)wbytes, s));
  const uint32_t* lv = c->list_nullable ? c->d_lvalid : nullptr;
  uint32_t* olv = c->list_nullable ? (uint32_t*)out_list_validity_dev : nullptr;
  uint32_t* oev = c->elem_nullable ? (uint32_t*)out_elem_validity_dev : nullptr;
  unsigned long long* counts = (unsigned long long*)c->d_lcounts;
  const int grid = grid_for(entries, 256) < 2048 ? grid_for(entries, 256) : 2048;
#define LIST_FINISH(V_) hipLaunchKernelGGL(pq_list_finish_kernel<V_>, dim3(grid), dim3(256), 0, s, entries, c->d_isrep, c->d_iselem, lv, c->d_ent_valid, c->d_roff, \
                                           c->d_eoff, (const V_*)c->d_ent_values, out_offsets_dev, olv, (V_*)out_values_dev, oev, counts, 1)
  if (is_bool) {
    DBHIP_CHECK(hipMemsetAsync(out_values_dev, 0, (size_t)wbytes, s));
    // (the value bits by their own kernel; offsets, validities and counts from the generic one, which moves no values here)
    hipLaunchKernelGGL(pq_list_finish_bool_kernel, dim3(grid), dim3(256), 0, s, entries, c->d_iselem, c->d_eoff, (const uint32_t*)c->d_ent_values, (uint32_t*)out_values_dev);
    hipLaunchKernelGGL(pq_list_finish_kernel<uint8_t>, dim3(grid), dim3(256), 0, s, entries, c->d_isrep, c->d_iselem, lv, c->d_ent_valid, c->d_roff, c->d_eoff,
                       (const uint8_t*)nullptr, out_offsets_dev, olv, (uint8_t*)nullptr, oev, counts, 0);
  } else if (esize == 1) LIST_FINISH(uint8_t);
  else if (esize == 2) LIST_FINISH(uint16_t);
  else if (esize == 4) LIST_FINISH(uint32_t);
  else if (esize == 8) LIST_FINISH(uint64_t);
  else LIST_FINISH(uint4);
#undef LIST_FINISH
  DBHIP_LAUNCH_CHECK();
  unsigned long long hc[4] = {0, 0, 0, 0};
  DBHIP_CHECK(hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, s));
  DBHIP_CHECK(hipStreamSynchronize(s));
  if (hc[3]) { set_error("%s: malformed column chunk (the first level entry continues a row)", who); return DBHIP_ERR_INVALID; }
  *out_rows_host = (int64_t)hc[0];
  *out_elems_host = (int64_t)hc[1];
  if (out_null_lists_host) *out_null_lists_host = (int64_t)hc[2];
  return DBHIP_OK;
}

// ---- nested leaves (any path of LIST / STRUCT nodes; include/dbhip.h has the rules) ----------------------------------------------
// The levels kernel leaves every entry's (r, d) as bytes. Entry e opens a slot in space m iff r <= m && d >= Ê_m: per 32-entry word and
// space, the slots are counted (pq_nest_count_kernel), scanned (one exclusive_scan_u32 per space), and the finish kernel gives each
// entry its rank in every space from the word's offset + a ballot of its wave — no per-space bitmap is stored.
struct NestK {
  int32_t n_nodes, R, max_def, leaf_null;
  int32_t kind[8], nul[8], V[8], space[8];
  uint32_t E[5];          // Ê_m, m = 0..R (Ê_0 = 0)
  uint64_t* off[8];       // LIST nodes: offsets
  uint32_t* val[9];       // nullable nodes: validity; [8]: the leaf's
};
enum { NK_TOTAL = 0, NK_NULLS = 5, NK_BAD = 14, NK_WORDS = 16 };   // counts: [0..4] slots per space, [5..13] NULLs per node (13: the leaf)

// Ê_r of a per-lane r (constant indices: the kernel arguments stay in scalar registers)
__device__ __forceinline__ uint32_t nest_ehat(const NestK& K, uint32_t r) {
  uint32_t e = 0;
#pragma unroll
  for (uint32_t m = 1; m < 5; ++m)
    if (r == m) e = K.E[m];
  return e;
}

// one entry per lane, whole waves: slots per word of every space (lane 0 writes the wave's two words) + the well-formedness rules
__global__ __launch_bounds__(256) void pq_nest_count_kernel(const uint8_t* __restrict__ lrep, const uint8_t* __restrict__ ldef, int64_t entries, int64_t nwords,
                                                            NestK K, uint32_t* __restrict__ scnt, unsigned long long* __restrict__ counts) {
  const uint32_t lane = threadIdx.x & 63u;
  for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < entries; base += (int64_t)gridDim.x * 256) {
    const int64_t e = base + lane;
    const bool in = e < entries;
    const uint32_t r = in ? lrep[e] : 0u, d = in ? ldef[e] : 0u;
    const bool bad = in && ((e == 0 && r != 0) || (r > 0 && d < nest_ehat(K, r)));
    if (__ballot(bad) != 0 && lane == 0) counts[NK_BAD] = 1;
    const int64_t w0 = base >> 5;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      if (m > K.R) break;
      const uint64_t mk = __ballot(in && r <= (uint32_t)m && d >= K.E[m]);
      if (lane == 0) {
        scnt[m * nwords + w0] = (uint32_t)__popc((uint32_t)mk);
        if (w0 + 1 < nwords) scnt[m * nwords + w0 + 1] = (uint32_t)__popc((uint32_t)(mk >> 32));
      }
    }
  }
}

// per entry: for every node, a validity bit / an offset at its slot; the leaf value moves to its slot (BITS: a BOOLEAN leaf, the values
// are a bitmap over the entries). ent_values of an entry without a value is zero (pq_spread), so a NULL slot gets zero bytes.
template <typename V, bool BITS>
__global__ __launch_bounds__(256) void pq_nest_finish_kernel(const uint8_t* __restrict__ lrep, const uint8_t* __restrict__ ldef, int64_t entries, int64_t nwords,
                                                             NestK K, const uint32_t* __restrict__ scnt, const uint64_t* __restrict__ soff,
                                                             const V* __restrict__ ent_values, V* __restrict__ out_values, unsigned long long* __restrict__ counts) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t lt = (1ull << lane) - 1ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // the totals of every space; each LIST node's closing offset
    uint64_t tot[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < 5; ++m)
      if (m <= K.R) { tot[m] = soff[m * nwords + nwords - 1] + scnt[m * nwords + nwords - 1]; counts[NK_TOTAL + m] = tot[m]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= K.n_nodes) break;
      if (K.kind[j] != PQ_NODE_LIST) continue;
      uint64_t own = 0, child = 0;
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (K.space[j] == m) { own = tot[m]; child = tot[m + 1]; }
      K.off[j][own] = child;
    }
  }
  uint32_t nl[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < entries; base += (int64_t)gridDim.x * 256) {
    const int64_t e = base + lane;
    const bool in = e < entries;
    const uint32_t r = in ? lrep[e] : 0u, d = in ? ldef[e] : 0u;
    const int64_t w0 = base >> 5;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= K.n_nodes) break;
      const int m = K.space[j];
      const bool opens = in && r <= (uint32_t)m && d >= K.E[m];
      const uint64_t mk = __ballot(opens);
      if (mk == 0) continue;
      const uint64_t rank = soff[m * nwords + w0] + (uint64_t)__popcll(mk & lt);
      if (K.nul[j]) {
        const bool v = opens && d >= (uint32_t)K.V[j];
        list_put_bits(K.val[j], v, rank);
        nl[j] += (uint32_t)__popcll(__ballot(opens && !v));
      }
      if (K.kind[j] == PQ_NODE_LIST) {
        const uint64_t mc = __ballot(in && r <= (uint32_t)(m + 1) && d >= K.E[m + 1]);
        if (opens) K.off[j][rank] = soff[(m + 1) * nwords + w0] + (uint64_t)__popcll(mc & lt);
      }
    }
    // the leaf (space R)
    const bool opens = in && r <= (uint32_t)K.R && d >= K.E[K.R];
    const uint64_t mk = __ballot(opens);
    if (mk == 0) continue;
    const uint64_t rank = soff[K.R * nwords + w0] + (uint64_t)__popcll(mk & lt);
    const bool valid = opens && d == (uint32_t)K.max_def;
    if (BITS) {
      const bool bit = valid && ((((const uint32_t*)ent_values)[e >> 5] >> (uint32_t)(e & 31)) & 1u);
      list_put_bits((uint32_t*)out_values, bit, rank);
    } else if (opens) {
      out_values[rank] = ent_values[e];
    }
    if (K.leaf_null) {
      list_put_bits(K.val[8], valid, rank);
      nl[8] += (uint32_t)__popcll(__ballot(opens && !valid));
    }
  }
  // NULL counts: one add per workgroup and node (adds on one word serialise in L2, see pq_list_finish_kernel)
  __shared__ uint32_t wn[9][4];
#pragma unroll
  for (int j = 0; j < 9; ++j)
    if (lane == 0) wn[j][threadIdx.x >> 6] = nl[j];
  __syncthreads();
  if (threadIdx.x < 9) {
    const uint32_t t = wn[threadIdx.x][0] + wn[threadIdx.x][1] + wn[threadIdx.x][2] + wn[threadIdx.x][3];
    if (t) atomicAdd(&counts[NK_NULLS + threadIdx.x], (unsigned long long)t);
  }
}

int32_t decode_nested(dbhip_pq_chunk* c, const uint8_t* chunk_dev, uint8_t* image_dev, dbhip_pq_node_out* nodes, void* out_values_dev, int64_t* out_rows_host,
                      void* stream) {
  const char* who = "dbhip_pq_chunk_decode_device_nested";
  DBHIP_REQUIRE(c && c->device_mode && c->nested, "dbhip_pq_chunk_decode_device_nested: the handle was not opened by dbhip_pq_chunk_open_device_nested");
  DBHIP_REQUIRE(nodes && out_rows_host, "dbhip_pq_chunk_decode_device_nested: NULL argument");
  const int nn = c->n_nodes;
  for (int j = 0; j < nn; ++j) {
    DBHIP_REQUIRE(c->node_kind[j] != PQ_NODE_LIST || nodes[j].offsets_dev, "dbhip_pq_chunk_decode_device_nested: a LIST node needs an offsets buffer");
    DBHIP_REQUIRE(!c->node_null[j] || nodes[j].validity_dev, "dbhip_pq_chunk_decode_device_nested: a nullable node needs a validity buffer");
  }
  DBHIP_REQUIRE(!c->leaf_nullable || nodes[nn].validity_dev, "dbhip_pq_chunk_decode_device_nested: a nullable leaf needs a validity buffer");
  for (int j = 0; j <= nn; ++j) { nodes[j].items = 0; nodes[j].nulls = 0; }
  *out_rows_host = 0;
  hipStream_t s = resolve_stream(stream);
  const int64_t entries = c->rows;
  if (entries == 0) {
    for (int j = 0; j < nn; ++j)
      if (c->node_kind[j] == PQ_NODE_LIST) DBHIP_CHECK(hipMemsetAsync(nodes[j].offsets_dev, 0, 8, s));
    DBHIP_CHECK(hipStreamSynchronize(s));
    return DBHIP_OK;
  }
  DBHIP_REQUIRE(out_values_dev, "dbhip_pq_chunk_decode_device_nested: NULL values buffer");
  const int esize = out_elem_size(c->out_type);
  const bool is_bool = c->out_type == DBHIP_T_BOOL;
  const int R = c->n_lists;
  const int64_t nwords = ceil_div(entries, 32), wbytes = ceil_div(entries, 64) * 8;
  if (!c->d_lrep) DBHIP_TRY(dbhip_alloc((size_t)entries + 16, (void**)&c->d_lrep));
  if (!c->d_ldef) DBHIP_TRY(dbhip_alloc((size_t)entries + 16, (void**)&c->d_ldef));
  if (!c->d_ent_valid) DBHIP_TRY(dbhip_alloc((size_t)wbytes, (void**)&c->d_ent_valid));
  if (!c->d_ent_values) DBHIP_TRY(dbhip_alloc(is_bool ? (size_t)wbytes : (size_t)entries * (size_t)esize, &c->d_ent_values));
  if (!c->d_scnt) DBHIP_TRY(dbhip_alloc((size_t)(R + 1) * (size_t)nwords * 4, (void**)&c->d_scnt));
  if (!c->d_soff) DBHIP_TRY(dbhip_alloc((size_t)(R + 1) * (size_t)nwords * 8, (void**)&c->d_soff));
  if (!c->d_lblk) DBHIP_TRY(dbhip_alloc((size_t)(ceil_div(nwords, SCAN_TILE) + 2) * 8, (void**)&c->d_lblk));
  if (!c->d_lcounts) DBHIP_TRY(dbhip_alloc(NK_WORDS * 8, (void**)&c->d_lcounts));
  // levels the pages do not carry read as 0: no LIST above the leaf (no repetition stream), no levels at all (max_def_level 0)
  if (R == 0) DBHIP_CHECK(hipMemsetAsync(c->d_lrep, 0, (size_t)entries, s));
  if (c->nest_max_def == 0) DBHIP_CHECK(hipMemsetAsync(c->d_ldef, 0, (size_t)entries, s));
  DBHIP_CHECK(hipMemsetAsync(c->d_lcounts, 0, NK_WORDS * 8, s));
  void* ent_values = c->d_ent_values;
  uint8_t* ent_valid = (uint8_t*)c->d_ent_valid;
  int64_t ent_nulls = 0;
  int32_t rc = decode_many(&c, 1, &chunk_dev, &image_dev, &ent_values, &ent_valid, &ent_nulls, nullptr, stream, true);
  if (rc) return rc;
  NestK K{};
  K.n_nodes = nn; K.R = R; K.max_def = c->nest_max_def; K.leaf_null = c->leaf_nullable;
  uint32_t before = 0;
  int lists = 0;
  for (int j = 0; j < nn; ++j) {
    K.kind[j] = c->node_kind[j]; K.nul[j] = c->node_null[j];
    K.space[j] = lists;
    K.V[j] = (int32_t)(before + (uint32_t)c->node_null[j]);
    before += (uint32_t)c->node_null[j];
    if (c->node_kind[j] == PQ_NODE_LIST) { K.E[++lists] = ++before; K.off[j] = nodes[j].offsets_dev; }
    if (c->node_null[j]) K.val[j] = (uint32_t*)nodes[j].validity_dev;
    if (nodes[j].validity_dev) DBHIP_CHECK(hipMemsetAsync(nodes[j].validity_dev, c->node_null[j] ? 0 : 0xFF, (size_t)wbytes, s));
  }
  if (c->leaf_nullable) K.val[8] = (uint32_t*)nodes[nn].validity_dev;
  if (nodes[nn].validity_dev) DBHIP_CHECK(hipMemsetAsync(nodes[nn].validity_dev, c->leaf_nullable ? 0 : 0xFF, (size_t)wbytes, s));
  if (is_bool) DBHIP_CHECK(hipMemsetAsync(out_values_dev, 0, (size_t)wbytes, s));
  unsigned long long* counts = (unsigned long long*)c->d_lcounts;
  const int grid = grid_for(entries, 256) < 2048 ? grid_for(entries, 256) : 2048;
  hipLaunchKernelGGL(pq_nest_count_kernel, dim3(grid), dim3(256), 0, s, c->d_lrep, c->d_ldef, entries, nwords, K, c->d_scnt, counts);
  for (int m = 0; m <= R; ++m) DBHIP_TRY(dbscan::exclusive_scan_u32(c->d_scnt + (size_t)m * nwords, nwords, c->d_lblk, c->d_soff + (size_t)m * nwords, s));
#define NEST_FINISH(V_, B_) hipLaunchKernelGGL((pq_nest_finish_kernel<V_, B_>), dim3(grid), dim3(256), 0, s, c->d_lrep, c->d_ldef, entries, nwords, K, \
                                               c->d_scnt, c->d_soff, (const V_*)c->d_ent_values, (V_*)out_values_dev, counts)
  if (is_bool) NEST_FINISH(uint32_t, true);
  else if (esize == 1) NEST_FINISH(uint8_t, false);
  else if (esize == 2) NEST_FINISH(uint16_t, false);
  else if (esize == 4) NEST_FINISH(uint32_t, false);
  else if (esize == 8) NEST_FINISH(uint64_t, false);
  else NEST_FINISH(uint4, false);
#undef NEST_FINISH
  DBHIP_LAUNCH_CHECK();
  unsigned long long hc[NK_WORDS] = {};
  DBHIP_CHECK(hipMemcpyAsync(hc, counts, sizeof(hc), hipMemcpyDeviceToHost, s));
  DBHIP_CHECK(hipStreamSynchronize(s));
  if (hc[NK_BAD]) {
    set_error("%s: malformed column chunk (the first level entry continues a row, or a repetition level has no element of its list)", who);
    return DBHIP_ERR_INVALID;
  }
  *out_rows_host = (int64_t)hc[NK_TOTAL];
  for (int j = 0; j < nn; ++j) { nodes[j].items = (int64_t)hc[NK_TOTAL + K.space[j]]; nodes[j].nulls = (int64_t)hc[NK_NULLS + j]; }
  nodes[nn].items = (int64_t)hc[NK_TOTAL + R];
  nodes[nn].nulls = (int64_t)hc[NK_NULLS + 8];
  return DBHIP_OK;
}
}  // namespace

extern "C" {

int32_t dbhip_pq_chunk_decode_device_list(dbhip_pq_chunk* c, const uint8_t* chunk_dev, uint8_t* image_dev, uint64_t* out_offsets_dev,
                                          uint8_t* out_list_validity_dev, void* out_values_dev, uint8_t* out_elem_validity_dev,
                                          int64_t* out_rows_host, int64_t* out_elems_host, int64_t* out_null_lists_host, void* stream) {
  return decode_list(c, chunk_dev, image_dev, out_offsets_dev, out_list_validity_dev, out_values_dev, out_elem_validity_dev, out_rows_host, out_elems_host,
                     out_null_lists_host, stream);
}

int32_t dbhip_pq_chunk_decode_device_nested(dbhip_pq_chunk* c, const uint8_t* chunk_dev, uint8_t* image_dev, dbhip_pq_node_out* nodes_host,
                                            void* out_values_dev, int64_t* out_rows_host, void* stream) {
  return decode_nested(c, chunk_dev, image_dev, nodes_host, out_values_dev, out_rows_host, stream);
}

int32_t dbhip_pq_chunk_take_arena(dbhip_pq_chunk* c, void** out_dev_ptr_host, int64_t* out_bytes_host) {
  DBHIP_REQUIRE(c && out_dev_ptr_host && out_bytes_host, "dbhip_pq_chunk_take_arena: NULL argument");
  *out_dev_ptr_host = c->d_arena;
  *out_bytes_host = c->d_arena ? c->arena_bytes : 0;
  c->d_arena = nullptr;
  c->arena_bytes = 0;
  return DBHIP_OK;
}

int32_t dbhip_pq_chunk_decode_device(dbhip_pq_chunk* c, const uint8_t* chunk_dev, uint8_t* image_dev, void* out_values_dev,
                                     uint8_t* out_validity_dev, int64_t* out_nulls_host, void* stream) {
  return decode_many(&c, 1, &chunk_dev, &image_dev, &out_values_dev, &out_validity_dev, out_nulls_host, nullptr, stream);
}

int32_t dbhip_pq_chunks_decode_device(dbhip_pq_chunk* const* chunks, int32_t n_chunks, const uint8_t* const* chunk_dev, uint8_t* const* image_dev,
                                      void* const* out_values_dev, uint8_t* const* out_validity_dev, int64_t* out_nulls_host,
                                      int32_t* out_status_host, void* stream) {
  DBHIP_REQUIRE(n_chunks >= 0 && (n_chunks == 0 || (chunks && chunk_dev && image_dev && out_values_dev && out_validity_dev)),
                "dbhip_pq_chunks_decode_device: NULL argument");
  return decode_many(chunks, n_chunks, chunk_dev, image_dev, out_values_dev, out_validity_dev, out_nulls_host, out_status_host, stream);
}

}  // extern "C"
