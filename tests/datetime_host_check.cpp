// Host driver of databend_amd/csrc/dev_datetime.h for tests/test_datetime_host_cpu.py: the header's own text compiled by the host
// compiler, applied to arrays read from files. Every file is raw little-endian int64 (one value per row).
//   part  <part> date|ts <offset_s> <tz file|-> <in> <out>          tz file: offset_s, count, at_utc_s[count], offset_after_s[count]
//   trunc <unit> <flags> date|ts date|ts <offset_s> <in> <out>
//   add   <unit> date|ts <offset_s> <in> <delta: n values or one> <out> <err: 1 = the row raises>
//   diff  <unit> date|ts <offset_s> <a> <b> <out>                   a or b may hold one value (a scalar)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../databend_amd/csrc/dev_datetime.h"

static std::vector<int64_t> read_all(const char* path) {
  std::vector<int64_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / 8);
  if (!v.empty() && fread(v.data(), 8, v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
  fclose(f);
  return v;
}
static void write_all(const char* path, const std::vector<int64_t>& v) {
  FILE* f = fopen(path, "wb");
  if (!f || (!v.empty() && fwrite(v.data(), 8, v.size(), f) != v.size())) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
  fclose(f);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "part" && argc == 8) {
    const int part = atoi(argv[2]);
    const bool ts = !strcmp(argv[3], "ts");
    int32_t offset = atoi(argv[4]);
    std::vector<int64_t> at;
    std::vector<int32_t> after;
    if (strcmp(argv[5], "-")) {
      const std::vector<int64_t> t = read_all(argv[5]);
      offset = (int32_t)t[0];
      const size_t k = (size_t)t[1];
      at.assign(t.begin() + 2, t.begin() + 2 + k);
      for (size_t i = 0; i < k; ++i) after.push_back((int32_t)t[2 + k + i]);
    }
    const std::vector<int64_t> in = read_all(argv[6]);
    std::vector<int64_t> out(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
      if (!ts) { out[i] = (int64_t)dt_part_date(part, (int32_t)in[i]); continue; }
      int32_t off = offset;
      if (!at.empty()) {
        uint32_t us;
        off = dt_tz_offset((int64_t)(dt_seconds(in[i], us) - DT_SHIFT_S), offset, (int32_t)at.size(), at.data(), after.data());
      }
      out[i] = (int64_t)dt_part_ts(part, in[i], off);
    }
    write_all(argv[7], out);
    return 0;
  }
  if (cmd == "trunc" && argc == 9) {
    const int unit = atoi(argv[2]), flags = atoi(argv[3]);
    const bool ts_in = !strcmp(argv[4], "ts"), ts_out = !strcmp(argv[5], "ts");
    const int32_t offset = atoi(argv[6]);
    const std::vector<int64_t> in = read_all(argv[7]);
    std::vector<int64_t> out(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
      if (!ts_in) out[i] = ts_out ? dt_trunc_date_to_ts(unit, flags, (int32_t)in[i], offset) : (int64_t)dt_trunc_date_to_date(unit, flags, (int32_t)in[i]);
      else out[i] = ts_out ? dt_trunc_ts_to_ts(unit, flags, in[i], offset) : (int64_t)dt_trunc_ts_to_date(unit, flags, in[i], offset);
    }
    write_all(argv[8], out);
    return 0;
  }
  if (cmd == "add" && argc == 9) {
    const int unit = atoi(argv[2]);
    const bool ts = !strcmp(argv[3], "ts");
    const int32_t offset = atoi(argv[4]);
    const std::vector<int64_t> in = read_all(argv[5]), delta = read_all(argv[6]);
    std::vector<int64_t> out(in.size()), err(in.size());
    for (size_t i = 0; i < in.size(); ++i) {
      const int64_t d = delta.size() == 1 ? delta[0] : delta[i];
      bool ok;
      if (ts) { int64_t r; ok = dt_add_ts(unit, in[i], d, offset, r); out[i] = r; }
      else { int32_t r; ok = in[i] >= INT32_MIN && in[i] <= INT32_MAX && dt_add_date(unit, (int32_t)in[i], d, r); out[i] = ok ? r : 0; }
      err[i] = !ok;
    }
    write_all(argv[7], out);
    write_all(argv[8], err);
    return 0;
  }
  if (cmd == "diff" && argc == 8) {
    const int unit = atoi(argv[2]);
    const bool ts = !strcmp(argv[3], "ts");
    const int32_t offset = atoi(argv[4]);
    const std::vector<int64_t> a = read_all(argv[5]), b = read_all(argv[6]);
    const size_t n = a.size() > b.size() ? a.size() : b.size();
    std::vector<int64_t> out(n);
    for (size_t i = 0; i < n; ++i) {
      const int64_t x = a.size() == 1 ? a[0] : a[i], y = b.size() == 1 ? b[0] : b[i];
      out[i] = ts ? dt_diff_ts(unit, x, y, offset) : dt_diff_date(unit, (int32_t)x, (int32_t)y);
    }
    write_all(argv[7], out);
    return 0;
  }
  fprintf(stderr, "usage: see the head of tests/datetime_host_check.cpp\n");
  return 2;
}
