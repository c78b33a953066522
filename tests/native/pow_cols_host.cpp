// Host build of lodestar_amd/csrc/bls_fp_pow.h for tests/test_fp_pow_cols.py: the resident
// exponentiation and its four primitives as plain C++ (g++), checked against Python big
// integers.  With -DPOW_COLS_MAIN it is a stand-alone program (for a -fsanitize=undefined
// build: the shifts are the risk) that runs the same primitives over edge values and
// cross-checks the exponentiation against a square-and-multiply over the resident product.
#define __device__
#define __constant__
#include "../../lodestar_amd/csrc/bls_constants.h"
#define LB_HD static inline
#include "../../lodestar_amd/csrc/bls_fp_pow.h"

using lb::pw::d13;

extern "C" {
// 12 limbs -> 13 digits
void pw_enter(uint32_t* d, const uint32_t* a) {
  d13 r;
  lb::pw::enter(r, a);
  for (int i = 0; i < 13; i++) d[i] = r.d[i];
}
// 13 digits (value < 2p) -> 12 canonical limbs
void pw_leave(uint32_t* r, const uint32_t* d) {
  d13 a;
  for (int i = 0; i < 13; i++) a.d[i] = d[i];
  lb::pw::leave(r, a);
}
// digits in, digits out
void pw_mul(uint32_t* r, const uint32_t* a, const uint32_t* b) {
  d13 x, y;
  for (int i = 0; i < 13; i++) {
    x.d[i] = a[i];
    y.d[i] = b[i];
  }
  lb::pw::mul(x, x, y);
  for (int i = 0; i < 13; i++) r[i] = x.d[i];
}
void pw_sqr(uint32_t* r, const uint32_t* a) {
  d13 x;
  for (int i = 0; i < 13; i++) x.d[i] = a[i];
  lb::pw::sqr(x, x);
  for (int i = 0; i < 13; i++) r[i] = x.d[i];
}
// 12 limbs in, 12 limbs out (R = 2^384 Montgomery form)
void pw_pow_p34(uint32_t* r, const uint32_t* a) { lb::pw::pow_p34(r, a); }
// the window program, for the exponent check
int pw_win_steps() { return LB_P34_WIN_STEPS; }
int pw_win(int k) { return LB_P34_WIN[k]; }
}

#ifdef POW_COLS_MAIN
#include <stdio.h>
int main() {
  constexpr uint32_t P32[12] = LB_P_LIMBS;
  uint32_t in[6][12] = {};
  in[1][0] = 1;
  for (int j = 0; j < 12; j++) {
    in[2][j] = P32[j];  // p - 1
    in[3][j] = 0xffffffffu;  // 2^384 - 1: beyond the contract, within enter()'s domain
    in[4][j] = j < 11 ? 0xffffffffu : 0u;
    in[5][j] = 0x9e3779b9u * (j + 1);
  }
  in[2][0] -= 1;
  in[5][11] &= 0x0fffffffu;
  int bad = 0;
  for (auto& a : in) {
    uint32_t r[12], d[13], e[13], back[12];
    pw_pow_p34(r, a);
    // the same power by plain square-and-multiply over the resident product: x^((p-3)/4)
    // in 2^390-form, then compared after leave() with the exit constant applied
    pw_enter(d, a);
    uint32_t acc[13];
    bool first = true;
    // exponent bits of (p - 3) / 4, most significant first
    uint32_t ex[12];
    {
      uint64_t br = 3;
      for (int j = 0; j < 12; j++) {
        const uint64_t v = (uint64_t)P32[j] - br;
        ex[j] = (uint32_t)v;
        br = (v >> 63) & 1;
      }
      for (int j = 0; j < 12; j++) ex[j] = (ex[j] >> 2) | (j < 11 ? ex[j + 1] << 30 : 0u);
    }
    for (int bit = 383; bit >= 0; bit--) {
      const bool one = (ex[bit / 32] >> (bit % 32)) & 1;
      if (!first) pw_sqr(acc, acc);
      if (one) {
        if (first) {
          for (int i = 0; i < 13; i++) acc[i] = d[i];
          first = false;
        } else {
          pw_mul(acc, acc, d);
        }
      }
    }
    const uint32_t exitc[13] = LB_POW_EXIT30;
    pw_mul(e, acc, exitc);
    pw_leave(back, e);
    for (int j = 0; j < 12; j++) bad |= back[j] != r[j];
  }
  printf(bad ? "MISMATCH\n" : "ok\n");
  return bad;
}
#endif
