// Host twin of the device's Decimal64 / Decimal128 row function: compiles the PRODUCT's dev_decimal.h (dec_row, dec_row_nodiv and what
// they call) and the u256 / division / pow10_i128 part of dev_common.h with g++, so tests/test_dec_edges_cpu.py can check them against
// Python integers without a GPU, and once more under -fsanitize=undefined,address. The test driver cuts the two texts out of the headers
// into dec_under_test.h (as tests/test_div_cpu.py does for the division alone); the macros below stand in for the HIP qualifiers.
// One request per input line, values as 32 hex digits of the i128 the kernel's load_operand produces (sign / zero extended):
//   op a_dec a_scale b_dec b_scale left_p left_s right_p right_s ret_p ret_s x y      -> "ok <hex>" | "err"
// Nodes that do not divide (dec_op_needs_division false) are evaluated by dec_row AND dec_row_nodiv, which must agree ("split" if not).
#include <stdint.h>
#include <stdio.h>

#include "../include/dbhip.h"

#define __host__
#define __device__
#define __forceinline__ inline
typedef __int128 i128;
typedef unsigned __int128 u128;
#include "dec_under_test.h"

static i128 parse_hex(const char* s) {
  u128 r = 0;
  for (int i = 0; i < 32; ++i) {
    const char c = s[i];
    r = (r << 4) | (u128)(c <= '9' ? c - '0' : (c | 32) - 'a' + 10);
  }
  return (i128)r;
}

int main() {
  char line[512], xs[64], ys[64];
  while (fgets(line, sizeof line, stdin)) {
    int op, a_dec, a_scale, b_dec, b_scale, lp, ls, rp, rs, retp, rets;
    if (sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %32s %32s", &op, &a_dec, &a_scale, &b_dec, &b_scale, &lp, &ls, &rp, &rs, &retp, &rets, xs, ys) != 13)
      return 2;
    // mirrors dbhip_decimal_decode_internal, k_decimal.hip:278-296 (the sizes come from the caller: tests/dec256_ref.result_size)
    DecOp p;
    p.op = op;
    p.a_from_scale = a_scale; p.a_to_scale = ls; p.a_to_precision = lp;
    p.a_check = a_dec ? (a_scale != ls) : 1;
    p.b_from_scale = b_scale; p.b_to_scale = rs; p.b_to_precision = rp;
    p.b_check = b_dec ? (b_scale != rs) : 1;
    p.t_is_128 = retp > 18;
    p.ret_precision = retp; p.ret_scale = rets;
    p.overflow = retp == (p.t_is_128 ? 38 : 18);
    p.scale_mul = op == DBHIP_OP_MULTIPLY ? a_scale + b_scale - rets : (op == DBHIP_OP_DIVIDE ? b_scale + rets - a_scale : 0);
    if (p.scale_mul < 0 || p.scale_mul > 38) { puts("nofn"); continue; }
    p.trivial = 0;
    const i128 x = parse_hex(xs), y = parse_hex(ys);
    i128 out = 0;
    const bool ok = dec_row(p, x, y, a_dec != 0, b_dec != 0, p.t_is_128 != 0, &out);
    if (!dec_op_needs_division(p)) {
      i128 out2 = 0;
      const bool ok2 = dec_row_nodiv(p, x, y, a_dec != 0, b_dec != 0, p.t_is_128 != 0, &out2);
      if (ok2 != ok || out2 != out) { puts("split"); continue; }
    }
    if (!ok) { puts("err"); continue; }
    // what the kernel stores: the i128 for a Decimal128 result, its low 64 bits for Decimal64 — printed sign extended
    if (!p.t_is_128) out = (i128)(int64_t)out;
    printf("ok %016llx%016llx\n", (unsigned long long)(uint64_t)((u128)out >> 64), (unsigned long long)(uint64_t)out);
  }
  return 0;
}
