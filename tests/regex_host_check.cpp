// Host twin of the regular-expression predicates: compiles databend_amd/csrc/regex_compile.h (the pattern compiler dbhip_regex_check
// and dbhip_regex_create run) and databend_amd/csrc/dev_regex.h (the row walk of k_regex.hip) — the very text the library includes —
// with g++ under -fsanitize=address,undefined. tests/test_regex_host_cpu.py drives it and asserts against tests/regex_ref.py.
// stdin, one command per line (hex strings, "-" for an empty one); stdout, one line per command:
//   pat <pattern> <flags>   -> "<rc> <states> <classes> <table bytes> <needs ascii>"   rc 0 = compiled, 1 = invalid, 2 = unsupported
//   val <value>             -> "<a0> <a1> <a2> <a3>"   regex_walk's answer (0 no, 1 yes, 2 declined) with the value `lead` = 0..3 bytes
//                              into an exactly sized heap block (an inline value, <= 12 bytes, lives in the view: four equal answers)
// A long value is read only through LIKE_LOAD_U32, which comes here (checked_u32): a word that holds no byte of the value ends the
// program, bytes of the word outside the value read as 0xEE, and AddressSanitizer reports whatever reads past the block. The tables the
// walk reads are exactly sized heap copies as well.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../include/dbhip.h"

struct LaneValue;
struct WaveValue;
static uint32_t checked_u32(uintptr_t a, const LaneValue& v);
static uint8_t checked_u8(const uint8_t* a, const WaveValue& v);
#define REGEX_FN inline
#define LIKE_LOAD_U32(addr, value) checked_u32((addr), (value))
#define LIKE_LOAD_U8(addr, value) checked_u8((addr), (value))
#include "../databend_amd/csrc/dev_regex.h"
#include "../databend_amd/csrc/regex_compile.h"

static uint32_t checked_u32(uintptr_t a, const LaneValue& v) {
  if ((a & 3) || v.len <= 12 || a + 4 <= v.base || a >= v.base + v.len) { fprintf(stderr, "a load outside the value's own words\n"); abort(); }
  uint32_t w = 0;
  for (int j = 0; j < 4; ++j) {
    const uintptr_t p = a + j;
    const uint32_t c = (p >= v.base && p < v.base + v.len) ? *(const uint8_t*)p : 0xEEu;   // a neighbour's byte
    w |= c << (8 * j);
  }
  return w;
}
static uint8_t checked_u8(const uint8_t* a, const WaveValue& v) {
  if (a < v.base || a >= v.base + v.len) abort();
  return *a;
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

int main() {
  static char cmd[16], a[2 * 6000];
  RxProgram prog;
  bool have = false;
  // exactly sized copies of what the kernels stage
  std::vector<uint16_t> table;
  std::vector<uint8_t> flags, cmap;
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "pat")) {
      int fl;
      if (scanf("%11999s %d", a, &fl) != 2) return 2;
      const std::vector<uint8_t> p = unhex(a);
      const char* why = "";
      prog = RxProgram();
      const int rc = rx_compile(p.empty() ? nullptr : p.data(), (int32_t)p.size(), fl, &prog, &why);
      have = rc == RX_OK;
      if (have) {
        if (prog.table.size() != prog.flags.size() * prog.n_classes || prog.flags.size() > (size_t)RX_MAX_STATES || prog.table.size() * 2 > (size_t)RX_MAX_TABLE_BYTES) abort();
        for (uint16_t t : prog.table) if (t >= prog.flags.size()) abort();
        for (int b = 0; b < 256; ++b) if (prog.cmap[b] >= prog.n_classes) abort();
        table = prog.table;
        flags = prog.flags;
        cmap.assign(prog.cmap, prog.cmap + 256);
      } else if (!why[0] || strstr(why, "DBHIP_")) abort();
      printf("%d %zu %u %zu %d\n", rc, have ? prog.flags.size() : (size_t)0, have ? prog.n_classes : 0u, have ? prog.table.size() * 2 : (size_t)0, have && prog.needs_ascii ? 1 : 0);
    } else if (!strcmp(cmd, "val")) {
      if (scanf("%11999s", a) != 1 || !have) return 2;
      const std::vector<uint8_t> b = unhex(a);
      const uint32_t len = (uint32_t)b.size();
      const RegexTables R{table.data(), flags.data(), cmap.data(), prog.n_classes, prog.needs_ascii ? 1u : 0u};
      uint32_t ans[4];
      for (uint32_t lead = 0; lead < 4; ++lead) {
        uint8_t* block = (uint8_t*)malloc(lead + len ? lead + len : 1);
        memset(block, 0xEE, lead);
        if (len) memcpy(block + lead, b.data(), len);
        uint32_t w[3] = {0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu};   // what lies past an inline value's bytes is not defined
        if (len <= 12) memcpy(w, block + lead, len);
        else { memcpy(w, block + lead, 4); w[1] = 0; w[2] = lead; }
        LaneValue v{len, w[0], w[1], w[2], len <= 12 ? 0 : (uintptr_t)(block + lead), 1, 0};
        ans[lead] = regex_walk(v, R);
        free(block);
      }
      printf("%u %u %u %u\n", ans[0], ans[1], ans[2], ans[3]);
    } else {
      return 2;
    }
  }
  return 0;
}
