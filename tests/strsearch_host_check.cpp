// Host twin of the String search and rewrite kernels' row logic: compiles databend_amd/csrc/dev_strsearch.h (with dev_strfn.h and
// dev_strview.h) — the very text k_strsearch.hip includes — with g++ under -fsanitize=address,undefined.
// tests/test_strsearch_host_cpu.py drives it and asserts against tests/strsearch_ref.py.
// stdin, one command per line (hex strings, "-" for an empty one); stdout, one line per command:
//   val   <value> <lead>                       -> "ok"                         the current value, `lead` (0..3) bytes into its heap block
//   pos   <needle> <start> <unit_byte>         -> "<position>"                 ss_position
//   split <delim> <part>                       -> "<found> <start> <end> <view>"  ss_field_range + sf_slice_view
//   rw    <op> <k> <x> <y> <unit_byte>         -> "<length|toolong> <bytes>"   ss_rewrite_len + ss_emit (and ss_len_walks, see below)
// A long value lies in a heap block of exactly lead + len bytes and is read the way the kernels read it: through SfValue::byte, whose
// aligned word loads come here (checked_u32): a word that holds no byte of the value ends the program, bytes of the word outside the
// value are not touched, and AddressSanitizer reports whatever reads past the block. The constants are copied into exactly sized
// heap blocks before ss_prepare reads them. Result views of long values name buffer 7, offset 1000.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct SfValue;
static uint32_t checked_u32(uintptr_t a, const SfValue& v);
#define SF_LOAD_U32(addr, value) checked_u32((addr), (value))
#include "../databend_amd/csrc/dev_strsearch.h"

static uint32_t checked_u32(uintptr_t a, const SfValue& v) {
  if ((a & 3) || a + 4 <= v.base || a >= v.base + v.len) { fprintf(stderr, "a load outside the value's own words\n"); abort(); }
  uint32_t w = 0;
  for (int j = 0; j < 4; ++j) {
    const uintptr_t p = a + j;
    const uint32_t c = (p >= v.base && p < v.base + v.len) ? *(const uint8_t*)p : 0xEEu;   // a neighbour's byte
    w |= c << (8 * j);
  }
  return w;
}

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

// a value in an exactly sized heap block; the view's words as a column would hold them (dirty bytes past an inline value)
struct Held {
  uint8_t* block = nullptr;
  uint32_t len = 0, lead = 0;
  void set(const std::vector<uint8_t>& v, uint32_t ld) {
    free(block);
    len = (uint32_t)v.size();
    lead = ld;
    block = (uint8_t*)malloc(lead + len ? lead + len : 1);
    memset(block, 0xEE, lead);
    if (len) memcpy(block + lead, v.data(), len);
  }
  SfValue value() const {
    uint32_t w[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    memcpy(w, block + lead, len <= 12 ? len : 4);
    return sf_value(len, w[0], w[1], w[2], block + lead);
  }
};
struct VectorSink {
  std::vector<uint8_t> out;
  void put(uint32_t at, uint32_t c) { if (at != out.size() || c > 0xFF) abort(); out.push_back((uint8_t)c); }
};
// the call's constants, prepared from exactly sized blocks
static void prepare(SsConst& C, const std::vector<uint8_t>& x, const std::vector<uint8_t>& y, bool unit_byte) {
  uint8_t* px = (uint8_t*)malloc(x.size() ? x.size() : 1);
  uint8_t* py = (uint8_t*)malloc(y.size() ? y.size() : 1);
  if (x.size()) memcpy(px, x.data(), x.size());
  if (y.size()) memcpy(py, y.data(), y.size());
  ss_prepare(C, px, (uint32_t)x.size(), py, (uint32_t)y.size(), unit_byte);
  free(px);
  free(py);
}

int main() {
  static char cmd[16], a[4096], b[4096], c[64];
  Held cur;
  cur.set({}, 0);
  SsConst* C = (SsConst*)malloc(sizeof(SsConst));
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "val")) {
      unsigned lead;
      if (scanf("%4095s %u", a, &lead) != 2 || lead > 3) return 2;
      cur.set(unhex(a), lead);
      printf("ok\n");
    } else if (!strcmp(cmd, "pos")) {
      int ub;
      if (scanf("%4095s %63s %d", a, c, &ub) != 3) return 2;
      prepare(*C, unhex(a), {}, ub != 0);
      SfValue v = cur.value();
      const int64_t s = strtoll(c, nullptr, 10);
      const uint64_t r = ss_position(v, C->x, C->x_len, s, ub != 0);
      // what pass 1 leaves to the wave must be a row that needs the bytes, never one whose answer is plain
      if (!ss_position_walks(v.len, C->x_len, s, ub != 0) && r != 0 && C->x_len != 0) return 3;
      printf("%llu\n", (unsigned long long)r);
    } else if (!strcmp(cmd, "split")) {
      if (scanf("%4095s %63s", a, c) != 2) return 2;
      prepare(*C, unhex(a), {}, true);
      SfValue v = cur.value();
      uint32_t s = 0, e = 0, w[4] = {0, 0, 0, 0};
      const bool found = ss_field_range(v, C->x, C->x_len, strtoll(c, nullptr, 10), &s, &e);
      if (found) sf_slice_view(v, 7, 1000, s, e, w);
      printf("%d %u %u ", (int)found, s, e);
      put_hex((const uint8_t*)w, 16);
      printf("\n");
    } else if (!strcmp(cmd, "rw")) {
      int op, ub;
      if (scanf("%d %63s %4095s %4095s %d", &op, c, a, b, &ub) != 5 || op < 0 || op >= SS_OP_COUNT) return 2;
      prepare(*C, unhex(a), unhex(b), ub != 0);
      SfValue v = cur.value();
      const int64_t k = strtoll(c, nullptr, 10);
      const uint64_t total = ss_rewrite_len(op, v, k, *C, ub != 0);
      if (total == SS_TOO_LONG) { printf("toolong -\n"); continue; }
      VectorSink sink;
      ss_emit(op, v, *C, (uint32_t)total, ub != 0, sink);
      if (sink.out.size() != total) return 3;
      if (total <= 12) {      // the same bytes through the sink of inline results
        SfInlineSink in{0, 0};
        ss_emit(op, v, *C, (uint32_t)total, ub != 0, in);
        uint8_t w[12];
        memcpy(w, &in.lo, 8);
        memcpy(w + 8, &in.hi, 4);
        for (size_t i = 0; i < 12; ++i)
          if (w[i] != (i < sink.out.size() ? sink.out[i] : 0)) return 3;
      }
      printf("%llu ", (unsigned long long)total);
      put_hex(sink.out.data(), sink.out.size());
      printf("\n");
    } else {
      return 2;
    }
  }
  free(cur.block);
  free(C);
  return 0;
}
