// Host twin of the kernels' String-view helpers: compiles databend_amd/csrc/dev_strview.h — the very text every kernel includes — with
// g++. tests/test_strview_cpu.py drives it and asserts against plain Python bytes.
// stdin, one command per line (hex strings, "-" for an empty one); stdout, one line per command:
//   canon   <view>                                -> "<inline 0|1> <w1> <w2> <w3>"      the words after sv_canon
//   keys    <view>                                -> "<inline 0|1> <k0> <k1>"           sv_key_words (decimal u64)
//   bytes   <view> <buf0> <buf1>                  -> "<where> <offset> <value>"         sv_bytes: where = -1 the view itself, 0 / 1 the buffer
//   bytesw  <view> <buf0> <buf1>                  -> the same                           sv_bytes from the view's words
//   checked <view> <buf0> <buf1> <n_buffers>      -> the same, or "null"                sv_bytes_checked; a buffer given as "-" is a NULL entry
//   make    <bytes> <index> <offset>              -> "<view>"                           sv_make
//   rebase  <view> <index_add> <offset_add>       -> "<view>"                           sv_rebase
// The buffer table of `checked` has exactly n_buffers entries and ends where an inaccessible page begins, and the view's index is used
// as it is: a helper that reads the table at or past n_buffers ends the program with a fault.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>
#include <unistd.h>
#include <string>
#include <vector>

#include "../databend_amd/csrc/dev_strview.h"

static std::vector<uint8_t> unhex(const char* s) {
  std::vector<uint8_t> out;
  if (s[0] == '-') return out;
  for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
    unsigned x;
    sscanf(s + i, "%2x", &x);
    out.push_back((uint8_t)x);
  }
  return out;
}
static void put_hex(const uint8_t* p, size_t n) {
  if (n == 0) printf("-");
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
}
static bool read_view(const char* s, uint32_t (&w)[4]) {
  const std::vector<uint8_t> b = unhex(s);
  if (b.size() != 16) return false;
  memcpy(w, b.data(), 16);
  return true;
}
static void put_where(const uint8_t* p, const uint32_t* view, const std::vector<uint8_t>* buf) {
  if (!p) { printf("null\n"); return; }
  int where = -2;
  long long off = 0;
  if (p >= (const uint8_t*)view && p < (const uint8_t*)view + 16) { where = -1; off = p - (const uint8_t*)view; }
  for (int k = 0; k < 2; ++k)
    if (!buf[k].empty() && p >= buf[k].data() && p + view[0] <= buf[k].data() + buf[k].size()) { where = k; off = p - buf[k].data(); }
  printf("%d %lld ", where, off);
  if (where == -2) printf("?");     // points nowhere we know: nothing is read
  else put_hex(p, view[0]);
  printf("\n");
}

int main() {
  static char cmd[16], a[400000], b[400000], c[400000];
  const long page = sysconf(_SC_PAGESIZE);
  uint8_t* guard = (uint8_t*)mmap(nullptr, 2 * page, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (guard == (uint8_t*)MAP_FAILED || mprotect(guard + page, page, PROT_NONE)) return 2;
  while (scanf("%15s", cmd) == 1) {
    uint32_t w[4];
    if (!strcmp(cmd, "canon")) {
      if (scanf("%399999s", a) != 1 || !read_view(a, w)) return 2;
      const bool in = sv_canon(w[0], w[1], w[2], w[3]);
      printf("%d %u %u %u\n", (int)in, w[1], w[2], w[3]);
    } else if (!strcmp(cmd, "keys")) {
      if (scanf("%399999s", a) != 1 || !read_view(a, w)) return 2;
      uint64_t k0 = 0, k1 = 0;
      const bool in = sv_key_words(w[0], w[1], w[2], w[3], k0, k1);
      printf("%d %llu %llu\n", (int)in, (unsigned long long)k0, (unsigned long long)k1);
    } else if (!strcmp(cmd, "bytes") || !strcmp(cmd, "bytesw") || !strcmp(cmd, "checked")) {
      if (scanf("%399999s %399999s %399999s", a, b, c) != 3 || !read_view(a, w)) return 2;
      const std::vector<uint8_t> buf[2] = {unhex(b), unhex(c)};
      if (strcmp(cmd, "checked")) {
        const void* table[2] = {buf[0].data(), buf[1].data()};
        put_where(cmd[5] ? sv_bytes(w, w[0], w[2], w[3], table) : sv_bytes(w, table), w, buf);
      } else {
        int n;
        if (scanf("%d", &n) != 1 || n < 0 || n > 2) return 2;
        const void** table = (const void**)(guard + page) - n;      // entries [0, n), then the inaccessible page
        for (int k = 0; k < n; ++k) table[k] = buf[k].empty() ? nullptr : buf[k].data();
        const uint8_t* at = nullptr;
        const bool ok = sv_bytes_checked(w, w[0], w[2], w[3], n ? table : nullptr, n, &at);
        if (ok != (at != nullptr)) return 2;       // false leaves *bytes untouched, true sets it
        put_where(at, w, buf);
      }
    } else if (!strcmp(cmd, "make")) {
      unsigned index, offset;
      if (scanf("%399999s %u %u", a, &index, &offset) != 3) return 2;
      const std::vector<uint8_t> v = unhex(a);
      sv_make(v.data(), (uint32_t)v.size(), index, offset, w);
      put_hex((const uint8_t*)w, 16);
      printf("\n");
    } else if (!strcmp(cmd, "rebase")) {
      unsigned ia, oa;
      if (scanf("%399999s %u %u", a, &ia, &oa) != 3 || !read_view(a, w)) return 2;
      sv_rebase(w[0], w[2], w[3], ia, oa);
      put_hex((const uint8_t*)w, 16);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
