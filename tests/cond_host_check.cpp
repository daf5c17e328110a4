// cond_host_check.cpp — databend_amd/csrc/dev_cond.h (and dev_strview.h's sv_rebase) compiled for the host, stand-alone: the text the
// kernels of k_cond.hip inline, driven by a plain loop in place of the waves. tests/test_cond_host_cpu.py builds it (with
// -fsanitize=address,undefined where that links), feeds it the shared case list and compares with tests/cond_ref.py.
//
//   fetch  <bitmap> <misalign> <nbits> <offset> <out>        cd_fetch64 of every 64-row word of bits [offset, nbits): u64 each
//   select <size> <n> <n_conds> <n_vals> <is_string> <misalign> <out> {<data|-> <validity|-> <voff> <scalar> <n_buffers>} ...
//          conditions first, then values; n_conds 0 is a coalesce. out: n elements (size 0: Bitmap words), validity words, n branch bytes
//   logic  <op> <n> <misalign> <out> {column} [{column}]      out: `true` words, `valid` words
//   check  <coalesce> <n_conds> <n_vals> <out> {<type> <is_scalar> <n_buffers> <precision> <scale>} ...   out: the status as text
// misalign 1: every Bitmap is loaded one byte off 8-byte alignment into an allocation of exactly its size, so cd_fetch64 takes its
// byte path and a byte read past the Bitmap is an error; 0: 8-byte aligned, in whole words.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../databend_amd/csrc/dev_cond.h"
#include "../databend_amd/csrc/dev_strview.h"

namespace {

struct Blob {
  uint8_t* base = nullptr;   // what was allocated
  uint8_t* p = nullptr;      // where the bytes are
  size_t size = 0;
  ~Blob() { free(base); }
};

// a file's bytes; a Bitmap either 8-byte aligned and padded to whole words, or one byte off and exact
void load(const char* path, bool bitmap, bool misalign, Blob& b) {
  if (!strcmp(path, "-")) return;
  FILE* f = fopen(path, "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  fseek(f, 0, SEEK_END);
  b.size = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  if (bitmap && misalign) {
    b.base = (uint8_t*)malloc(b.size + 1);   // malloc's result is at least 8-byte aligned, so base + 1 is not
    b.p = b.base + 1;
  } else {
    const size_t padded = bitmap ? ((b.size + 7) / 8) * 8 + 8 : b.size + 16;
    if (posix_memalign((void**)&b.base, 16, padded)) exit(2);
    memset(b.base, 0, padded);
    b.p = b.base;
  }
  if (b.size && fread(b.p, 1, b.size, f) != b.size) exit(2);
  fclose(f);
}

struct Column {
  Blob data, validity;
  int64_t voff = 0;
  bool scalar = false;
  int32_t n_buffers = 0;
  uint32_t table_base = 0;
};

void read_column(char** a, bool bool_data, bool misalign, Column& c) {
  load(a[0], bool_data, misalign, c.data);
  load(a[1], true, misalign, c.validity);
  c.voff = atoll(a[2]);
  c.scalar = atoi(a[3]) != 0;
  c.n_buffers = atoi(a[4]);
}

uint64_t validity_word(const Column& c, int64_t row0, int count) {
  if (!c.validity.p) return ~0ull;
  if (c.scalar) return cd_splat(cd_fetch64(c.validity.p, c.voff, 1) != 0);
  return cd_fetch64(c.validity.p, c.voff + row0, count);
}
uint64_t bool_word(const Column& c, uint64_t vv, int64_t row0, int count) {
  if (c.scalar) return vv ? cd_splat(cd_fetch64(c.data.p, 0, 1) != 0) : 0ull;
  return cd_fetch64(c.data.p, row0, count);
}

void write_out(const char* path, const std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "wb");
  if (!f || (out.size() && fwrite(out.data(), 1, out.size(), f) != out.size())) exit(2);
  fclose(f);
}

template <int SIZE>
void merge_runs(const Column& c, bool is_string, int64_t row0, int count, uint64_t mv, uint8_t* out) {
  constexpr int R = SIZE >= 16 ? 1 : 16 / SIZE;
  constexpr int W = R * SIZE / 4;
  for (int sh = 0; sh < count; sh += R) {                         // one lane's run of rows
    const uint32_t minev = (uint32_t)(mv >> sh) & ((1u << R) - 1);
    if (!minev) continue;                                         // a run that took nothing of this branch reads nothing of it
    const int lr = count - sh < R ? count - sh : R;
    uint32_t v[W];
    memset(v, 0, sizeof(v));
    for (int r = 0; r < lr; ++r) {
      if (!((minev >> r) & 1)) continue;
      memcpy((uint8_t*)v + r * SIZE, c.data.p + (c.scalar ? 0 : (row0 + sh + r) * SIZE), SIZE);
    }
    if (SIZE == 16 && is_string) sv_rebase(v[0], v[2], v[3], c.table_base, 0);
    uint32_t o[W];
    memset(o, 0, sizeof(o));
    memcpy(o, out + (row0 + sh) * SIZE, (size_t)lr * SIZE);
    for (int d = 0; d < W && d * 4 < lr * SIZE; ++d) o[d] |= v[d] & cd_word_mask<SIZE>(minev, d);
    memcpy(out + (row0 + sh) * SIZE, o, (size_t)lr * SIZE);
  }
}

int run_select(int argc, char** argv) {
  const int size = atoi(argv[2]);
  const int64_t n = atoll(argv[3]);
  const int n_conds = atoi(argv[4]), n_vals = atoi(argv[5]);
  const bool is_string = atoi(argv[6]) != 0, misalign = atoi(argv[7]) != 0;
  const char* out_path = argv[8];
  if (argc != 9 + 5 * (n_conds + n_vals)) return 2;
  std::vector<Column> conds(n_conds), vals(n_vals);
  char** a = argv + 9;
  for (int k = 0; k < n_conds; ++k, a += 5) read_column(a, true, misalign, conds[k]);
  for (int k = 0; k < n_vals; ++k, a += 5) read_column(a, size == 0, misalign, vals[k]);
  std::vector<int32_t> nb(n_vals);
  std::vector<uint32_t> base(n_vals);
  for (int k = 0; k < n_vals; ++k) nb[k] = vals[k].n_buffers;
  cd_table_bases(nb.data(), n_vals, base.data());
  for (int k = 0; k < n_vals; ++k) vals[k].table_base = base[k];
  const int64_t words = (n + 63) / 64;
  const size_t data_bytes = size ? (size_t)n * size : (size_t)words * 8;
  std::vector<uint8_t> out(data_bytes + words * 8 + n, 0);
  uint8_t* o_data = out.data();
  uint8_t* o_valid = o_data + data_bytes;
  uint8_t* o_branch = o_valid + words * 8;
  for (int64_t w = 0; w < words; ++w) {
    const int64_t row0 = w * 64;
    const int count = n - row0 >= 64 ? 64 : (int)(n - row0);
    CdChooser ch = cd_chooser(cd_live(row0, n));
    uint64_t validw = 0, bits = 0;
    for (int k = 0; k < n_vals; ++k) {
      uint64_t t, vv = validity_word(vals[k], row0, count);
      if (n_conds == 0) t = vv;
      else if (k == n_conds) t = ~0ull;
      else {
        const uint64_t cv = validity_word(conds[k], row0, count);
        t = cd_true_rows(bool_word(conds[k], cv, row0, count), cv);
      }
      const uint64_t m = cd_take(ch, t), mv = m & vv;
      validw |= mv;
      for (int b = 0; b < count; ++b) if ((m >> b) & 1) o_branch[row0 + b] = (uint8_t)k;
      if (!mv) continue;
      switch (size) {
        case 0: bits |= mv & bool_word(vals[k], mv, row0, count); break;
        case 1: merge_runs<1>(vals[k], false, row0, count, mv, o_data); break;
        case 2: merge_runs<2>(vals[k], false, row0, count, mv, o_data); break;
        case 4: merge_runs<4>(vals[k], false, row0, count, mv, o_data); break;
        case 8: merge_runs<8>(vals[k], false, row0, count, mv, o_data); break;
        case 16: merge_runs<16>(vals[k], is_string, row0, count, mv, o_data); break;
        default: merge_runs<32>(vals[k], false, row0, count, mv, o_data); break;
      }
    }
    for (int b = 0; b < count; ++b) if ((cd_rest(ch) >> b) & 1) o_branch[row0 + b] = (uint8_t)n_vals;
    if (size == 0) memcpy(o_data + w * 8, &bits, 8);
    memcpy(o_valid + w * 8, &validw, 8);
  }
  write_out(out_path, out);
  return 0;
}

int run_logic(int argc, char** argv) {
  const int op = atoi(argv[2]);
  const int64_t n = atoll(argv[3]);
  const bool misalign = atoi(argv[4]) != 0;
  const int ncols = op == CD_NOT ? 1 : 2;
  if (argc != 6 + 5 * ncols) return 2;
  Column c[2];
  for (int k = 0; k < ncols; ++k) read_column(argv + 6 + 5 * k, true, misalign, c[k]);
  const int64_t words = (n + 63) / 64;
  std::vector<uint8_t> out(words * 16, 0);
  for (int64_t w = 0; w < words; ++w) {
    const int64_t row0 = w * 64;
    const int count = n - row0 >= 64 ? 64 : (int)(n - row0);
    const uint64_t va = validity_word(c[0], row0, count), a = bool_word(c[0], va, row0, count);
    uint64_t vb = ~0ull, b = 0, t, v;
    if (op != CD_NOT) { vb = validity_word(c[1], row0, count); b = bool_word(c[1], vb, row0, count); }
    cd_kleene(op, a, va, b, vb, t, v);
    t &= cd_live(row0, n);
    v &= cd_live(row0, n);
    memcpy(out.data() + w * 8, &t, 8);
    memcpy(out.data() + (words + w) * 8, &v, 8);
  }
  write_out(argv[5], out);
  return 0;
}

int run_fetch(char** argv) {
  Blob b;
  load(argv[2], true, atoi(argv[3]) != 0, b);
  const int64_t nbits = atoll(argv[4]), off = atoll(argv[5]);
  std::vector<uint8_t> out;
  for (int64_t row0 = 0; off + row0 < nbits; row0 += 64) {
    const int64_t left = nbits - off - row0;
    const uint64_t w = cd_fetch64(b.p, off + row0, left >= 64 ? 64 : (int)left);
    out.insert(out.end(), (const uint8_t*)&w, (const uint8_t*)&w + 8);
  }
  write_out(argv[6], out);
  return 0;
}

int run_check(int argc, char** argv) {
  const bool coalesce = atoi(argv[2]) != 0;
  const int n_conds = atoi(argv[3]), n_vals = atoi(argv[4]);
  std::vector<CdDesc> d;
  for (int i = 6; i + 4 < argc; i += 5) {
    CdDesc x;
    x.type = atoi(argv[i]); x.is_scalar = atoi(argv[i + 1]); x.n_buffers = atoi(argv[i + 2]);
    x.precision = (uint8_t)atoi(argv[i + 3]); x.scale = (uint8_t)atoi(argv[i + 4]);
    d.push_back(x);
  }
  const int given_conds = coalesce ? 0 : (n_conds > 0 ? n_conds : 0);
  if ((int)d.size() < given_conds) return 2;
  int why = -1;
  d.resize(d.size() + 1);   // so that data() of an empty list is a pointer all the same
  const int rc = cd_check(coalesce ? nullptr : d.data(), n_conds, d.data() + given_conds, n_vals, &why);
  const std::string text = std::to_string(rc) + " " + std::to_string(why) + "\n";
  write_out(argv[5], std::vector<uint8_t>(text.begin(), text.end()));
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 7 && !strcmp(argv[1], "fetch")) return run_fetch(argv);
  if (argc >= 9 && !strcmp(argv[1], "select")) return run_select(argc, argv);
  if (argc >= 6 && !strcmp(argv[1], "logic")) return run_logic(argc, argv);
  if (argc >= 6 && !strcmp(argv[1], "check")) return run_check(argc, argv);
  fprintf(stderr, "usage: see the head of cond_host_check.cpp\n");
  return 2;
}
