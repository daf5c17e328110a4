// Host twin of the String function kernels' row logic: compiles databend_amd/csrc/dev_strfn.h (and dev_strview.h) — the very text
// k_strfn.hip includes — with g++ under -fsanitize=address,undefined. tests/test_strfn_host_cpu.py drives it and asserts against
// tests/str_ref.py.
// stdin, one command per line (hex strings, "-" for an empty one); stdout, one line per command:
//   val   <value> <lead>                  -> "ok"                      the current value, `lead` (0..3) bytes into its heap block
//   len   <unit_byte>                     -> "<units>"                 sf_units (unit_byte: the length itself, as the kernel does)
//   sub   <op> <a> <b|-> <unit_byte>      -> "<start> <end> <view>"    sf_plan + sf_plan_range + sf_slice_view
//   trim  <op> <pad>                      -> "<start> <end> <view>"    sf_trim_range + sf_slice_view
//   build <op> <nargs> <value> ...        -> "<non_ascii 0|1> <bytes>" sf_emit
// A long value lies in a heap block of exactly lead + len bytes and is read the way the kernels read it: through SfValue::byte, whose
// aligned word loads come here (checked_u32): a word that holds no byte of the value ends the program, bytes of the word outside the
// value are not touched, and AddressSanitizer reports whatever reads past the block. Result views of long values name buffer 7, offset 1000.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct SfValue;
static uint32_t checked_u32(uintptr_t a, const SfValue& v);
#define SF_LOAD_U32(addr, value) checked_u32((addr), (value))
#include "../databend_amd/csrc/dev_strfn.h"

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
struct HeldArgs {
  std::vector<Held> held;
  SfValue get(int32_t k) const { return held[k].value(); }
};
struct VectorSink {
  std::vector<uint8_t> out;
  void put(uint32_t at, uint32_t c) { if (at != out.size()) abort(); out.push_back((uint8_t)c); }
};

static void put_slice(SfValue& v, uint32_t s, uint32_t e) {
  uint32_t w[4];
  sf_slice_view(v, 7, 1000, s, e, w);
  printf("%u %u ", s, e);
  put_hex((const uint8_t*)w, 16);
  printf("\n");
}

int main() {
  static char cmd[16], a[4096], b[64], c[64];
  Held cur;
  cur.set({}, 0);
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "val")) {
      unsigned lead;
      if (scanf("%4095s %u", a, &lead) != 2 || lead > 3) return 2;
      cur.set(unhex(a), lead);
      printf("ok\n");
    } else if (!strcmp(cmd, "len")) {
      int ub;
      if (scanf("%d", &ub) != 1) return 2;
      SfValue v = cur.value();
      printf("%u\n", ub ? v.len : sf_units(v));
    } else if (!strcmp(cmd, "sub")) {
      int op, ub;
      if (scanf("%d %63s %63s %d", &op, b, c, &ub) != 4) return 2;
      const bool has_b = c[0] != '-' || c[1];
      const int64_t pa = strtoll(b, nullptr, 10), pb = has_b ? strtoll(c, nullptr, 10) : 0;
      SfValue v = cur.value();
      const SfPlan plan = sf_plan(op, v.len, pa, pb, has_b);
      uint32_t s, e;
      sf_plan_range(op, plan, v, ub != 0, &s, &e);
      put_slice(v, s, e);
    } else if (!strcmp(cmd, "trim")) {
      int op;
      if (scanf("%d %4095s", &op, a) != 2) return 2;
      const std::vector<uint8_t> pad = unhex(a);
      uint8_t* pp = (uint8_t*)malloc(pad.size() ? pad.size() : 1);       // exactly sized as well
      if (pad.size()) memcpy(pp, pad.data(), pad.size());
      SfValue v = cur.value();
      uint32_t s, e;
      sf_trim_range(op, v, pp, (uint32_t)pad.size(), &s, &e);
      put_slice(v, s, e);
      free(pp);
    } else if (!strcmp(cmd, "build")) {
      int op, nargs;
      if (scanf("%d %d", &op, &nargs) != 2 || nargs < 1 || nargs > SF_MAX_ARGS) return 2;
      HeldArgs args;
      args.held.resize(nargs);
      for (int k = 0; k < nargs; ++k) {
        if (scanf("%4095s", a) != 1) return 2;
        args.held[k].set(unhex(a), (uint32_t)(k % 4));
      }
      VectorSink sink;
      const bool high = sf_emit(op, args, nargs, sink);
      // the same bytes through the sink of inline results
      if (sink.out.size() <= 12) {
        SfInlineSink in{0, 0};
        sf_emit(op, args, nargs, in);
        uint8_t w[12];
        memcpy(w, &in.lo, 8);
        memcpy(w + 8, &in.hi, 4);
        for (size_t i = 0; i < 12; ++i)
          if (w[i] != (i < sink.out.size() ? sink.out[i] : 0)) return 3;
      }
      printf("%d ", (int)high);
      put_hex(sink.out.data(), sink.out.size());
      printf("\n");
      for (auto& h : args.held) free(h.block);
    } else {
      return 2;
    }
  }
  free(cur.block);
  return 0;
}
