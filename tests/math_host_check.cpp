// math_host_check.cpp — databend_amd/csrc/dev_math.h compiled for the host (the same text the kernels of k_math.hip inline) and run
// over files of raw values; tests/test_math_host_cpu.py compares every output bit for bit with tests/math_ref.py.
//   math_host_check num <fn> <type> <digits> <in> <out>            type: a dbhip_type code 2 .. 11; out holds the result type's values
//   math_host_check dec <fn> <bits> <p> <s> <digits> <in> <out>    bits: 64 | 128; out holds the storage's values (SIGN: int8)
//   math_host_check div <in> <out>                                  in: triples of u64 (hi, lo, v); out: the two words of (hi:lo) / v
// Built with -fsanitize=address,undefined where the compiler links it: an out-of-range shift, a signed overflow or a division by
// zero anywhere on these inputs ends the run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../databend_amd/csrc/dev_math.h"

static std::vector<uint8_t> read_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<uint8_t> b((size_t)size);
  if (size && fread(b.data(), 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "short read of %s\n", path); exit(2); }
  fclose(f);
  return b;
}
static void write_file(const char* path, const void* p, size_t bytes) {
  FILE* f = fopen(path, "wb");
  if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

template <typename T> static T get(const std::vector<uint8_t>& b, size_t i) {
  T v;
  memcpy(&v, b.data() + i * sizeof(T), sizeof(T));
  return v;
}
template <typename T> static void put(std::vector<uint8_t>& b, T v) {
  const size_t at = b.size();
  b.resize(at + sizeof(T));
  memcpy(b.data() + at, &v, sizeof(T));
}

// fn over the values of one number type, exactly as k_math.hip's function classes dispatch it
template <typename T, typename U, typename Bits>
static void run_number(int fn, int32_t digits, bool is_float, const std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
  const size_t n = in.size() / sizeof(T);
  const MtNum m = mt_num_decode(fn, digits);
  for (size_t i = 0; i < n; ++i) {
    const T v = get<T>(in, i);
    if (fn == MT_ABS) {
      if (is_float) {
        const Bits b = get<Bits>(in, i);
        if (sizeof(Bits) == 4) put<uint32_t>(out, mt_abs_f32_bits((uint32_t)b));
        else put<uint64_t>(out, mt_abs_f64_bits((uint64_t)b));
      } else {
        put<U>(out, mt_abs_int<T, U>(v));
      }
    } else if (fn == MT_SIGN) {
      put<int8_t>(out, mt_sign<T>(v));
    } else {
      put<double>(out, mt_num_f64(m, (double)v));
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<uint8_t> out;
  if (!strcmp(argv[1], "num") && argc == 7) {
    const int fn = atoi(argv[2]), type = atoi(argv[3]);
    const int32_t digits = (int32_t)atol(argv[4]);
    const std::vector<uint8_t> in = read_file(argv[5]);
    switch (type) {
      case 2: run_number<int8_t, uint8_t, uint8_t>(fn, digits, false, in, out); break;
      case 3: run_number<int16_t, uint16_t, uint16_t>(fn, digits, false, in, out); break;
      case 4: run_number<int32_t, uint32_t, uint32_t>(fn, digits, false, in, out); break;
      case 5: run_number<int64_t, uint64_t, uint64_t>(fn, digits, false, in, out); break;
      case 6: run_number<uint8_t, uint8_t, uint8_t>(fn, digits, false, in, out); break;
      case 7: run_number<uint16_t, uint16_t, uint16_t>(fn, digits, false, in, out); break;
      case 8: run_number<uint32_t, uint32_t, uint32_t>(fn, digits, false, in, out); break;
      case 9: run_number<uint64_t, uint64_t, uint64_t>(fn, digits, false, in, out); break;
      case 10: run_number<float, uint32_t, uint32_t>(fn, digits, true, in, out); break;
      case 11: run_number<double, uint64_t, uint64_t>(fn, digits, true, in, out); break;
      default: return 2;
    }
    write_file(argv[6], out.data(), out.size());
    return 0;
  }
  if (!strcmp(argv[1], "dec") && argc == 9) {
    const int fn = atoi(argv[2]), bits = atoi(argv[3]), p = atoi(argv[4]), s = atoi(argv[5]);
    const int32_t digits = (int32_t)atol(argv[6]);
    const std::vector<uint8_t> in = read_file(argv[7]);
    const MtDec d = fn == MT_SIGN ? MtDec() : mt_dec_decode(fn, p, s, digits);
    const size_t n = in.size() / (size_t)(bits / 8);
    for (size_t i = 0; i < n; ++i) {
      if (bits == 64) {
        const int64_t v = get<int64_t>(in, i);
        if (fn == MT_SIGN) put<int8_t>(out, mt_sign<int64_t>(v));
        else put<int64_t>(out, mt_dec64(d, v));
      } else {
        const mt_i128 v = get<mt_i128>(in, i);
        if (fn == MT_SIGN) put<int8_t>(out, mt_sign<mt_i128>(v));
        else put<mt_i128>(out, mt_dec128(d, v));
      }
    }
    write_file(argv[8], out.data(), out.size());
    return 0;
  }
  if (!strcmp(argv[1], "div") && argc == 4) {
    const std::vector<uint8_t> in = read_file(argv[2]);
    const size_t n = in.size() / 24;
    for (size_t i = 0; i < n; ++i) {
      const uint64_t hi = get<uint64_t>(in, 3 * i), lo = get<uint64_t>(in, 3 * i + 1), v = get<uint64_t>(in, 3 * i + 2);
      const mt_u128 q = mt_div128_64(((mt_u128)hi << 64) | lo, v);
      put<uint64_t>(out, (uint64_t)q);
      put<uint64_t>(out, (uint64_t)(q >> 64));
    }
    write_file(argv[3], out.data(), out.size());
    return 0;
  }
  fprintf(stderr, "usage: math_host_check num|dec|div ...\n");
  return 2;
}
