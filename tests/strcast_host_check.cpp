// Host twin of the String cast kernels' row logic: compiles databend_amd/csrc/dev_strcast.h (with dev_strfn.h, dev_strview.h and
// dev_datetime.h) — the very text k_strcast.hip includes — with g++ under -fsanitize=address,undefined.
// tests/test_strcast_host_cpu.py drives it and asserts against tests/strcast_ref.py.
// stdin, one command per line (hex strings, "-" for an empty one); stdout, one line per command:
//   val   <value> <lead>                                      -> "ok"                       the current value, `lead` (0..3) bytes into its heap block
//   parse <type> <precision> <scale> <rounding> <offset_s>    -> "<status> <lo> <hi>"       sc_parse: 0 ok / 1 error / 2 declined, the image in hex
//   fmt   <type> <scale> <offset_s> <lo> <hi> <data offset>   -> "<status> <text> <view>"   sc_format + sc_text_view (lo, hi in hex)
//   split <hi> <lo>                                           -> "<q> <r>"                  sc_split19 (hex in, decimal out)
// A long value lies in a heap block of exactly lead + len bytes and is read the way the kernels read it: through SfValue::byte, whose
// aligned word loads come here (checked_u32): a word that holds no byte of the value ends the program, bytes of the word outside the
// value are not touched, and AddressSanitizer reports whatever reads past the block.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct SfValue;
static uint32_t checked_u32(uintptr_t a, const SfValue& v);
#define SF_LOAD_U32(addr, value) checked_u32((addr), (value))
#include "../databend_amd/csrc/dev_strcast.h"

static uint32_t checked_u32(uintptr_t a, const SfValue& v) {
  if ((a & 3) || a + 4 <= v.base || a >= v.base + v.len) { fprintf(stderr, "a load outside the value's own words\n"); abort(); }
  uint32_t w = 0;
  for (int j = 0; j < 4; ++j) {
    const uintptr_t p = a + j;
    const uint32_t c = (p >= v.base && p < v.base + v.len) ? *(const uint8_t*)p : 0x31u;   // a neighbour's byte: a digit
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
    memset(block, 0x31, lead);
    if (len) memcpy(block + lead, v.data(), len);
  }
  SfValue value() const {
    uint32_t w[3] = {0x31313131u, 0x31313131u, 0x31313131u};
    memcpy(w, block + lead, len <= 12 ? len : 4);
    return sf_value(len, w[0], w[1], w[2], block + lead);
  }
};

int main() {
  static char cmd[16], a[4096];
  Held cur;
  cur.set({}, 0);
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "val")) {
      unsigned lead;
      if (scanf("%4095s %u", a, &lead) != 2 || lead > 3) return 2;
      cur.set(unhex(a), lead);
      printf("ok\n");
    } else if (!strcmp(cmd, "parse")) {
      int type, precision, scale, rounding, offset;
      if (scanf("%d %d %d %d %d", &type, &precision, &scale, &rounding, &offset) != 5) return 2;
      const ScSpec S{type, (uint32_t)precision, (uint32_t)scale, rounding, offset};
      SfValue v = cur.value();
      uint64_t lo = 1, hi = 1;
      const int st = sc_parse(v, S, &lo, &hi);
      printf("%d %016llx %016llx\n", st, (unsigned long long)lo, (unsigned long long)hi);
    } else if (!strcmp(cmd, "fmt")) {
      int type, scale, offset;
      unsigned long long lo, hi;
      unsigned at;
      if (scanf("%d %d %d %llx %llx %u", &type, &scale, &offset, &lo, &hi, &at) != 6) return 2;
      ScText T;
      memset(&T, 0xEE, sizeof(T));
      const int st = sc_format(type, (uint32_t)scale, offset, sc_widen(type, lo), hi, T);
      if (T.len > SC_TEXT_MAX) return 3;
      const uint8_t* bytes = (const uint8_t*)T.w;
      for (uint32_t k = T.len; k < 4 * SC_TEXT_WORDS; ++k)
        if (bytes[k]) return 3;                                 // zero behind the text: the kernel ORs these words next to a neighbour's
      uint32_t w[4];
      sc_text_view(T, at, w);
      printf("%d ", st);
      put_hex(bytes, T.len);
      printf(" ");
      put_hex((const uint8_t*)w, 16);
      printf("\n");
    } else if (!strcmp(cmd, "split")) {
      unsigned long long hi, lo;
      if (scanf("%llx %llx", &hi, &lo) != 2) return 2;
      uint64_t q, r;
      sc_split19(hi, lo, &q, &r);
      printf("%llu %llu\n", (unsigned long long)q, (unsigned long long)r);
    } else {
      return 2;
    }
  }
  free(cur.block);
  return 0;
}
