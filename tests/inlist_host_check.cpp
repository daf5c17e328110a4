// Host twin of the IN-list kernels' row logic: compiles databend_amd/csrc/dev_inlist.h (and dev_strview.h) — the very text
// k_inlist.hip includes — with g++ under -fsanitize=address,undefined. tests/test_inlist_host_cpu.py drives it and asserts against
// tests/inlist_ref.py.
// stdin, one command per line (hex strings, "-" for an empty one); stdout, one line per command:
//   new   <kind> <force_table>   -> "ok"     a new, empty set; kind: raw (8-byte integers) | f32 | f64 | d128 | str
//   add   <element>              -> "ok"     little-endian bytes of the element (8, 4, 8, 16 bytes) or the String's bytes
//   build                        -> "<path> <slots> <distinct> <has_sentinel>"   path 1 = COMPARE, 2 = TABLE; slots 0 for COMPARE
//   hash  <value>                -> "<hash, 16 hex digits> <home slot>"          inl_hash of the value's key image; slot in the built table
//   where <value>                -> "<slot>"  the slot that holds the value's key, -1 if none (TABLE)
//   probe <value> <lead>         -> "0" | "1" inl_member. A String value lies `lead` (0..3) bytes into an exactly sized heap block
//   bad   <value>                -> "0" | "1" the same for a view whose buffer index is past the table (nothing may be read)
// A long String value is read only through IN_LOAD_U32, which comes here (checked_u32): a word that holds no byte of the value ends
// the program, bytes of the word outside the value are not touched, and AddressSanitizer reports whatever reads past the block.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

static uint32_t checked_u32(uintptr_t a, uintptr_t base, uint32_t len);
#define IN_LOAD_U32(addr, base, len) checked_u32((addr), (base), (len))
#include "../databend_amd/csrc/dev_inlist.h"

static uint32_t checked_u32(uintptr_t a, uintptr_t base, uint32_t len) {
  if ((a & 3) || a + 4 <= base || a >= base + len) { fprintf(stderr, "a load outside the value's own words\n"); abort(); }
  uint32_t w = 0;
  for (int j = 0; j < 4; ++j) {
    const uintptr_t p = a + j;
    const uint32_t c = (p >= base && p < base + len) ? *(const uint8_t*)p : 0xEEu;   // a neighbour's byte
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

enum Kind { RAW, F32, F64, D128, STR };

// the set, prepared by the text dbhip_inlist_create uses (inl_set_* in dev_inlist.h)
struct Set : InlSet {
  Kind kind = RAW;
  bool force_table = false;
  void start(Kind k, bool force) {
    inl_set_init(*this, k == F32 ? 4 : k == RAW || k == F64 ? 8 : 16, k == F32 || k == F64, k == STR);
    kind = k;
    force_table = force;
  }
  void add(const std::vector<uint8_t>& b) {
    static const uint8_t none = 0;
    if (kind != STR) inl_set_add_fixed(*this, b.data());
    else if (inl_set_add_string(*this, b.empty() ? &none : b.data(), (uint32_t)b.size()) != INL_ADD_OK) abort();
  }
  int build() {
    inl_set_finish(*this, force_table);
    return path;
  }
  const uint64_t* table() const { return (const uint64_t*)image.data(); }
  const uint32_t* longs() const { return image.data() + long_at; }
};

// the value as the kernel sees it; a String lies in a heap block of exactly lead + len bytes
struct Held {
  uint8_t* block = nullptr;
  const void* bufs[1] = {nullptr};
  ~Held() { free(block); }
  InlValue make(const Set& s, const std::vector<uint8_t>& b, uint32_t lead, bool bad_index) {
    if (s.kind == F32) { uint32_t x; memcpy(&x, b.data(), 4); return inl_value(inl_canon_f32(x), 0); }
    if (s.kind == F64) { uint64_t x; memcpy(&x, b.data(), 8); return inl_value(inl_canon_f64(x), 0); }
    if (s.kind == RAW) { uint64_t x; memcpy(&x, b.data(), 8); return inl_value(x, 0); }
    if (s.kind == D128) { uint64_t x, y; memcpy(&x, b.data(), 8); memcpy(&y, b.data() + 8, 8); return inl_value(x, y); }
    const uint32_t len = (uint32_t)b.size();
    free(block);
    block = (uint8_t*)malloc(lead + len ? lead + len : 1);
    memset(block, 0xEE, lead);
    if (len) memcpy(block + lead, b.data(), len);
    uint32_t w[3] = {0xEEEEEEEEu, 0xEEEEEEEEu, 0xEEEEEEEEu};   // what lies past an inline value's bytes is not defined
    if (len <= 12) memcpy(w, block + lead, len);
    else { memcpy(w, block + lead, 4); w[1] = bad_index ? 1u : 0u; w[2] = lead; }
    bufs[0] = block;
    return inl_string_value(len, w[0], w[1], w[2], bufs, 1);   // one buffer: index 1 points nowhere
  }
};

int main() {
  static char cmd[16], a[2 * 5000];
  Set set;
  set.start(RAW, false);
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "new")) {
      int force;
      if (scanf("%15s %d", a, &force) != 2) return 2;
      set.start(!strcmp(a, "f32") ? F32 : !strcmp(a, "f64") ? F64 : !strcmp(a, "d128") ? D128 : !strcmp(a, "str") ? STR : RAW, force != 0);
      printf("ok\n");
    } else if (!strcmp(cmd, "add")) {
      if (scanf("%9999s", a) != 1) return 2;
      set.add(unhex(a));
      printf("ok\n");
    } else if (!strcmp(cmd, "build")) {
      const int path = set.build();
      printf("%d %u %zu %d\n", path, set.slots, set.k0s.size(), (int)set.has_sentinel);
    } else if (!strcmp(cmd, "hash") || !strcmp(cmd, "where")) {
      if (scanf("%9999s", a) != 1) return 2;
      Held h;
      const InlValue v = h.make(set, unhex(a), 0, false);
      const uint64_t hv = inl_hash(v.k0, v.k1);
      if (cmd[0] == 'h') { printf("%016llx %u\n", (unsigned long long)hv, set.slots ? (uint32_t)hv & (set.slots - 1) : 0u); continue; }
      int found = -1;
      for (uint32_t s = 0; s < set.slots && found < 0; ++s) {
        const uint64_t s0 = set.wide() ? set.table()[2 * s] : set.table()[s], s1 = set.wide() ? set.table()[2 * s + 1] : 0;
        if (!(s0 == INL_EMPTY && (!set.wide() || s1 == INL_EMPTY)) && inl_key_equal(s0, s1, v, set.wide(), set.longs())) found = (int)s;
      }
      printf("%d\n", found);
    } else if (!strcmp(cmd, "probe") || !strcmp(cmd, "bad")) {
      unsigned lead = 0;
      if (scanf("%9999s", a) != 1) return 2;
      if (cmd[0] == 'p' && (scanf("%u", &lead) != 1 || lead > 3)) return 2;
      Held h;
      const InlValue v = h.make(set, unhex(a), lead, cmd[0] == 'b');
      // an exactly sized copy of the image the kernels stage, so that a read past the table or the long-byte block is reported
      std::vector<uint32_t> image(set.image);
      const bool hit = inl_member(v, set.wide(), set.has_sentinel, (const uint64_t*)image.data(), set.slots, set.items, set.slots ? 0 : (uint32_t)set.k0s.size(),
                                  image.data() + set.long_at);
      printf("%d\n", (int)hit);
    } else {
      return 2;
    }
  }
  return 0;
}
