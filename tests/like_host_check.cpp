// Host twin of k_like.hip's matching steps: compiles databend_amd/csrc/like_match.h — the parser and the per-value steps the kernels
// run — with g++ and CHECKED loads: every 4-byte load must be 4-byte aligned and hold at least one byte of the value, every 1-byte
// load must lie inside the value; a violation ends the program with exit code 3. tests/test_like_ref_cpu.py drives it.
// stdin, one case per line (hex strings, "-" for an empty one):
//     pattern escape literal_kind flags value before behind misalign
// literal_kind >= 0: the pattern is dbhip_str_match's needle. The value is laid out at an address that is `misalign` (0..15) past a
// 16-byte boundary, with the bytes `before` directly in front of it and `behind` directly behind it (the neighbours a packed buffer
// would have). stdout per case: "rc kind bit".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../include/dbhip.h"

struct LaneValue;
struct WaveValue;
static uint32_t checked_u32(uintptr_t a, const LaneValue& v);
static uint8_t checked_u8(const uint8_t* a, const WaveValue& v);
#define LIKE_FN inline
#define LIKE_LOAD_U32(addr, value) checked_u32((addr), (value))
#define LIKE_LOAD_U8(addr, value) checked_u8((addr), (value))
#include "../databend_amd/csrc/like_match.h"

static uint32_t checked_u32(uintptr_t a, const LaneValue& v) {
  if ((a & 3) || v.len <= 12 || a + 4 <= v.base || a >= v.base + v.len) {
    fprintf(stderr, "bad 4-byte load at value offset %lld (len %u)\n", (long long)(a - v.base), v.len);
    exit(3);
  }
  return *(const uint32_t*)a;
}
static uint8_t checked_u8(const uint8_t* a, const WaveValue& v) {
  if (a < v.base || a >= v.base + v.len) {
    fprintf(stderr, "bad 1-byte load at value offset %lld (len %u)\n", (long long)(a - v.base), v.len);
    exit(3);
  }
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

// pass 2 of k_like.hip with the 64 lanes run one after the other
static bool wave_match(const WaveValue& v0, const LikeShared& S, uint32_t nseg, bool a_start, bool a_end, bool unit_byte) {
  WaveValue v = v0;
  const uint8_t* sb = (const uint8_t*)S.words;
  uint32_t pos = 0, tail = v.len, first = 0, last = nseg;
  if (a_start) {
    if (!seg_forward(v, sb, S.under, S.seg_off[1], 0, unit_byte, &pos)) return false;
    first = 1;
    if (nseg == 1 && a_end) return pos == v.len;
  }
  if (a_end) {
    const uint32_t o = S.seg_off[nseg - 1];
    if (!seg_backward(v, sb + o, S.under + o, S.seg_off[nseg] - o, v.len, unit_byte, &tail)) return false;
    last = nseg - 1;
  }
  for (uint32_t s = first; s < last; ++s) {
    const uint32_t o = S.seg_off[s], L = S.seg_off[s + 1] - o;
    bool found = false;
    for (uint32_t b0 = pos; b0 + L <= tail && !found; b0 += 64)
      for (uint32_t lane = 0; lane < 64 && !found; ++lane) {
        uint32_t e = 0;
        if (b0 + lane + L <= tail && seg_forward(v, sb + o, S.under + o, L, b0 + lane, unit_byte, &e)) { pos = e; found = true; }
      }
    if (!found) return false;
  }
  return pos <= tail;
}

int main() {
  static char pat[1024], val[400000], before[1024], behind[1024];
  int escape, literal_kind, flags, misalign;
  while (scanf("%1023s %d %d %d %399999s %1023s %1023s %d", pat, &escape, &literal_kind, &flags, val, before, behind, &misalign) == 8) {
    const std::vector<uint8_t> p = unhex(pat), v = unhex(val), b0 = unhex(before), b1 = unhex(behind);
    LikeTable t;
    const char* why = "";
    const int32_t rc = literal_kind >= 0 ? like_parse_needle(literal_kind, p.data(), (int32_t)p.size(), &t, &why)
                                         : like_parse(p.data(), (int32_t)p.size(), escape, false, &t, &why);
    if (rc) { printf("%d -1 0\n", rc); continue; }
    LikeShared S;
    memcpy(S.words, t.bytes, sizeof(S.words));
    for (int i = 0; i < 256; ++i) S.under[i] = (uint8_t)((t.under[i >> 5] >> (i & 31)) & 1u);
    memcpy(S.seg_off, t.seg_off, sizeof(S.seg_off));
    // the value between its neighbours, at the wanted misalignment; 32 bytes of 0xEE on both sides keep a stray load inside the allocation
    std::vector<uint8_t> mem(64 + b0.size() + v.size() + b1.size() + 64 + 32, 0xEE);
    uintptr_t at = (uintptr_t)mem.data() + 32 + b0.size();
    at = ((at + 15) & ~(uintptr_t)15) + (uintptr_t)misalign;
    uint8_t* vp = (uint8_t*)at;
    memcpy(vp - b0.size(), b0.data(), b0.size());
    memcpy(vp, v.data(), v.size());
    memcpy(vp + v.size(), b1.data(), b1.size());
    uint32_t w[3] = {0, 0, 0};
    if (v.size() <= 12) memcpy(w, v.data(), v.size());
    else memcpy(w, v.data(), 4);      // a long view: the prefix, then buffer index and offset (not used here)
    LaneValue lv{(uint32_t)v.size(), w[0], w[1], w[2], v.size() > 12 ? at : 0, 1, 0};
    bool listed = false;
    bool hit = like_lane_decide(lv, S, t.kind, t.nseg, t.min_len, t.anchor_start, t.anchor_end, (flags & DBHIP_LIKE_UNIT_BYTE) != 0, &listed);
    if (listed) hit = wave_match(WaveValue{(uint32_t)v.size(), vp}, S, t.nseg, t.anchor_start, t.anchor_end, (flags & DBHIP_LIKE_UNIT_BYTE) != 0);
    printf("0 %d %d\n", (int)t.kind, (int)(hit != ((flags & DBHIP_LIKE_NEGATE) != 0)));
  }
  return 0;
}
