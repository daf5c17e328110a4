// Host twin of the Array kernels' row logic: compiles databend_amd/csrc/dev_array.h (with dev_strfn.h and dev_strview.h) — the very text
// k_array.hip includes — with g++ under -fsanitize=address,undefined. tests/test_array_host_cpu.py drives it and asserts against
// tests/array_ref.py.
// stdin, one command per line (hex strings, "-" for an empty one); stdout, one line per command:
//   row   <a> <b> <n_elems>                    -> "<good> <start> <len>"       ar_row over the pair of offsets
//   pos   <i> <len>                            -> "<found> <pos>"              ar_get_pos
//   run   <es> <elements> <validity>           -> "ok"    the current run: its elements in a heap block of exactly len * es bytes; the
//                                                          validity is a string of 0 / 1 per element, "-" for all valid
//   get   <i>                                  -> "<valid> <element>"          ar_get_pos + ar_load + ar_store (the zero value when not valid)
//   find  <mode> <needle|null>                 -> "<position>"                 the first non-NULL element with ar_eq, 1-based, 0: none
//   red   <kind> <type> <split>                -> "<valid> <err> <value>"      ar_fold over [0, split) and [split, len), ar_merge, ar_finish
//   rtype <kind> <type> <precision> <scale>    -> "<rc> <type> <precision> <scale>"   ar_reduce_result
//   strs  <lead> <dirty> <validity> <value>... -> "ok"    the current run of String views: every long value in a heap block of exactly
//                                                          lead + len bytes, its view naming the value's own buffer; "!" is a 20-byte view
//                                                          that names a buffer past the table; dirty: 0xAA behind an inline value
//   finds <needle>                             -> "<position>"                 the first non-NULL view with ar_str_eq
// A long value is read the way the kernels read it: through SfValue::byte, whose aligned word loads come here (checked_u32): a word
// that holds no byte of the value ends the program, and AddressSanitizer reports whatever reads past a block.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

struct SfValue;
static uint32_t checked_u32(uintptr_t a, const SfValue& v);
#define SF_LOAD_U32(addr, value) checked_u32((addr), (value))
#include "../databend_amd/csrc/dev_array.h"

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
static std::vector<std::string> words(const char* line) {
  std::vector<std::string> out;
  std::string cur;
  for (const char* p = line; *p; ++p) {
    if (*p == ' ' || *p == '\n' || *p == '\r') { if (!cur.empty()) out.push_back(cur); cur.clear(); }
    else cur.push_back(*p);
  }
  if (!cur.empty()) out.push_back(cur);
  return out;
}

// the current run: elements (or views) in an exactly sized block, one validity flag per element
static uint8_t* g_block = nullptr;
static uint64_t g_len = 0;
static int g_es = 0;
static std::vector<uint8_t> g_valid;
static std::vector<uint8_t*> g_buffers;      // a String run: the values' own blocks; entry k belongs to element k (NULL for an inline value)
static std::vector<const void*> g_table;

static void clear_run() {
  free(g_block);
  g_block = nullptr;
  for (uint8_t* b : g_buffers) free(b);
  g_buffers.clear();
  g_table.clear();
  g_valid.clear();
  g_len = 0;
}
static void set_validity(const std::string& bits) {
  g_valid.assign(g_len, 1);
  if (bits != "-")
    for (uint64_t k = 0; k < g_len && k < bits.size(); ++k) g_valid[k] = bits[k] == '1';
}

template <int CLS>
static void reduce_run(int kind, int out_es, uint64_t split) {
  ArAcc a, b;
  ar_acc_init(a);
  ar_acc_init(b);
  for (uint64_t k = 0; k < g_len; ++k)
    if (g_valid[k]) ar_fold<CLS>(kind, k < split ? a : b, ar_load(g_block, k, g_es, CLS == AR_CLS_I));
  ar_merge<CLS>(kind, a, b);
  ArBits r;
  bool err;
  const bool ok = ar_finish<CLS>(kind, a, &r, &err);
  uint8_t* out = (uint8_t*)malloc((size_t)out_es);      // exactly the result's bytes
  ar_store(out, 0, out_es, r);
  printf("%d %d ", ok ? 1 : 0, err ? 1 : 0);
  put_hex(out, (size_t)out_es);
  printf("\n");
  free(out);
}

int main() {
  static char line[1 << 22];
  while (fgets(line, sizeof(line), stdin)) {
    const std::vector<std::string> w = words(line);
    if (w.empty()) continue;
    const std::string& cmd = w[0];
    if (cmd == "row") {
      uint64_t* off = (uint64_t*)malloc(16);
      off[0] = strtoull(w[1].c_str(), nullptr, 10);
      off[1] = strtoull(w[2].c_str(), nullptr, 10);
      uint64_t start, len;
      const bool good = ar_row(off, 0, strtoull(w[3].c_str(), nullptr, 10), &start, &len);
      printf("%d %llu %llu\n", good ? 1 : 0, (unsigned long long)start, (unsigned long long)len);
      free(off);
    } else if (cmd == "pos") {
      uint64_t pos;
      const bool found = ar_get_pos(strtoll(w[1].c_str(), nullptr, 10), strtoull(w[2].c_str(), nullptr, 10), &pos);
      printf("%d %llu\n", found ? 1 : 0, (unsigned long long)pos);
    } else if (cmd == "run") {
      clear_run();
      g_es = atoi(w[1].c_str());
      const std::vector<uint8_t> v = unhex(w[2].c_str());
      g_len = v.size() / (size_t)g_es;
      g_block = (uint8_t*)malloc(v.size() ? v.size() : 1);
      if (!v.empty()) memcpy(g_block, v.data(), v.size());
      set_validity(w[3]);
      printf("ok\n");
    } else if (cmd == "get") {
      uint64_t pos;
      ArBits v{0, 0};
      bool ok = false;
      if (ar_get_pos(strtoll(w[1].c_str(), nullptr, 10), g_len, &pos)) {
        v = ar_load(g_block, pos, g_es, false);
        ok = g_valid[pos] != 0;
      }
      uint8_t* out = (uint8_t*)malloc((size_t)g_es);
      ar_store(out, 0, g_es, v);
      printf("%d ", ok ? 1 : 0);
      put_hex(out, (size_t)g_es);
      printf("\n");
      free(out);
    } else if (cmd == "find") {
      const int mode = atoi(w[1].c_str());
      uint64_t at = 0;
      if (w[2] != "null") {
        const std::vector<uint8_t> nv = unhex(w[2].c_str());
        uint8_t* nb = (uint8_t*)malloc(nv.size());
        memcpy(nb, nv.data(), nv.size());
        const ArBits nd = ar_load(nb, 0, g_es, false);
        for (uint64_t k = 0; k < g_len && !at; ++k)
          if (g_valid[k] && ar_eq(mode, ar_load(g_block, k, g_es, false), nd)) at = k + 1;
        free(nb);
      }
      printf("%llu\n", (unsigned long long)at);
    } else if (cmd == "red") {
      const int kind = atoi(w[1].c_str()), type = atoi(w[2].c_str());
      const uint64_t split = strtoull(w[3].c_str(), nullptr, 10);
      int32_t t = 0;
      uint8_t p = 0, s = 0;
      if (ar_reduce_result(kind, type, 0, 0, &t, &p, &s)) { printf("refused\n"); continue; }
      const int out_es = ar_size(t);
      switch (ar_class(type)) {
        case AR_CLS_I: reduce_run<AR_CLS_I>(kind, out_es, split); break;
        case AR_CLS_U: reduce_run<AR_CLS_U>(kind, out_es, split); break;
        case AR_CLS_F32: reduce_run<AR_CLS_F32>(kind, out_es, split); break;
        case AR_CLS_F64: reduce_run<AR_CLS_F64>(kind, out_es, split); break;
        default: reduce_run<AR_CLS_D128>(kind, out_es, split); break;
      }
    } else if (cmd == "rtype") {
      int32_t t = 0;
      uint8_t p = 0, s = 0;
      const int rc = ar_reduce_result(atoi(w[1].c_str()), atoi(w[2].c_str()), (uint8_t)atoi(w[3].c_str()), (uint8_t)atoi(w[4].c_str()), &t, &p, &s);
      if (rc) printf("%d 0 0 0\n", rc);
      else printf("0 %d %d %d\n", t, p, s);
    } else if (cmd == "strs") {
      clear_run();
      const uint32_t lead = (uint32_t)atoi(w[1].c_str());
      const bool dirty = atoi(w[2].c_str()) != 0;
      g_es = 16;
      g_len = w.size() - 4;
      g_block = (uint8_t*)malloc(g_len ? g_len * 16 : 1);
      for (uint64_t k = 0; k < g_len; ++k) {
        uint32_t vw[4] = {0, 0, 0, 0};
        uint8_t* buf = nullptr;
        if (w[4 + k] == "!") {
          vw[0] = 20; vw[1] = 0x64636261u; vw[2] = 1000000u; vw[3] = 0;
        } else {
          const std::vector<uint8_t> v = unhex(w[4 + k].c_str());
          vw[0] = (uint32_t)v.size();
          if (v.size() <= 12) {
            uint8_t raw[12];
            memset(raw, dirty ? 0xAA : 0, 12);
            if (!v.empty()) memcpy(raw, v.data(), v.size());
            memcpy(&vw[1], raw, 12);
          } else {
            buf = (uint8_t*)malloc(lead + v.size());
            memset(buf, 0xEE, lead);
            memcpy(buf + lead, v.data(), v.size());
            memcpy(&vw[1], v.data(), 4);
            vw[2] = (uint32_t)k;
            vw[3] = lead;
          }
        }
        memcpy(g_block + 16 * k, vw, 16);
        g_buffers.push_back(buf);
        g_table.push_back(buf);
      }
      set_validity(w[3]);
      printf("ok\n");
    } else if (cmd == "finds") {
      const std::vector<uint8_t> nv = unhex(w[1].c_str());
      uint8_t* nb = (uint8_t*)malloc(nv.size() ? nv.size() : 1);      // exactly the needle's bytes
      if (!nv.empty()) memcpy(nb, nv.data(), nv.size());
      uint64_t at = 0;
      for (uint64_t k = 0; k < g_len && !at; ++k) {
        if (!g_valid[k]) continue;
        uint32_t vw[4];
        memcpy(vw, g_block + 16 * k, 16);
        const uint8_t* bytes = nullptr;
        if (!sv_bytes_checked(g_block + 16 * k, vw[0], vw[2], vw[3], g_table.data(), (int32_t)g_table.size(), &bytes)) continue;
        SfValue v = sf_value(vw[0], vw[1], vw[2], vw[3], bytes);
        if (ar_str_eq(v, nb, (uint32_t)nv.size())) at = k + 1;
      }
      free(nb);
      printf("%llu\n", (unsigned long long)at);
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  clear_run();
  return 0;
}
